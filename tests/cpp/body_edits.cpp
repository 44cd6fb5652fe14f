// Bodies edited on a running world through the C++ drop-in shim: set_rigidbody_mass / _inertia / _friction, rigidbody_set_shape and
// rigidbody_set_kind (util/rigidbody.hpp:105-260) are applied to the device context in place (edynhip_edit_bodies) - the same program
// run with init_config::rebuild_on_body_edit, which re-creates the context for every edit as before, must compute the same bits.
//   scene    a 4x4x4 pile, a hinge chain, a puck on the floor; ten updates between the edits of the puck (and of a chain link)
//   checks   position, orientation and velocities of every body bitwise equal after every update, in place against rebuild;
//            context_rebuilds == 0 in place; the contact entities of two resting pile boxes that no edit touches survive every edit in
//            place and are made again by the rebuild; the program in execution_mode::asynchronous stays in place and its edits take
//            effect (the checks of lifecycle.cpp on the same edits)
#include <edyn/edyn.hpp>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED: %s (line %d)\n", #cond, __LINE__); ++failures; } } while (0)

namespace {
struct watched_mark { int edit; };   // a component of this program's own on the watched contact entities: it goes when its entity is destroyed
struct Trace {
    std::vector<std::vector<float>> frames;         // 13 floats per body after every update
    std::vector<std::set<uint32_t>> watched;        // the watched pair's contact entities (manifold + points) around every edit: before, after
    std::vector<size_t> still_marked;               // per edit: how many of the entities after it carry the mark put on the ones before it
    uint64_t rebuilds = 0;
    float weight = 0, ice_x = 0, ice_v = 0, frozen_dx = 1;
    bool sphere = false, is_static = false;
};

std::set<uint32_t> contact_entities_of(entt::registry &registry, entt::entity a, entt::entity b) {
    std::set<uint32_t> out;
    entt::entity manifold = entt::null;
    registry.view<edyn::contact_manifold>().each([&](entt::entity e, edyn::contact_manifold &cm) {
        if ((cm.body[0] == a && cm.body[1] == b) || (cm.body[0] == b && cm.body[1] == a)) manifold = e;
    });
    if (manifold == entt::null) return out;
    out.insert((uint32_t)manifold);
    registry.view<edyn::contact_point_list>().each([&](entt::entity e, edyn::contact_point_list &l) { if (l.parent == manifold) out.insert((uint32_t)e); });
    return out;
}

Trace run_program(edyn::execution_mode mode, bool rebuild) {
    Trace tr;
    entt::registry registry;
    auto config = edyn::init_config{};
    config.num_solver_velocity_iterations = 10;
    config.execution_mode = mode;
    config.rebuild_on_body_edit = rebuild;
    config.max_bodies = 128;   // (no capacity growth in this program: every rebuild counted is an edit's)
    edyn::attach(registry, config);

    std::vector<entt::entity> all;
    auto floor_def = edyn::rigidbody_def{};
    floor_def.kind = edyn::rigidbody_kind::rb_static;
    floor_def.shape = edyn::plane_shape{{0, 1, 0}, 0};
    all.push_back(edyn::make_rigidbody(registry, floor_def));

    auto def = edyn::rigidbody_def{};
    def.shape = edyn::box_shape{{0.5f, 0.5f, 0.5f}};
    def.sleeping_disabled = true;   // (a re-created context does not wake an edited island, the edit in place does: kept out of the comparison)
    entt::entity pile[4][4][4];
    for (int k = 0; k < 4; ++k) for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) {
        def.position = {1.02f * i + 0.5f * (k & 1), 0.505f + 1.005f * k, 1.02f * j + 0.5f * (k & 1)};
        all.push_back(pile[k][i][j] = edyn::make_rigidbody(registry, def));
    }
    // a chain of four links hanging from a static anchor, hinges about z
    auto anchor_def = edyn::rigidbody_def{};
    anchor_def.kind = edyn::rigidbody_kind::rb_static;
    anchor_def.position = {-6, 6, 0};
    entt::entity prev = edyn::make_rigidbody(registry, anchor_def);
    all.push_back(prev);
    entt::entity links[4];
    for (int k = 0; k < 4; ++k) {
        auto link_def = edyn::rigidbody_def{};
        link_def.position = {-6 + 0.5f * (k + 0.5f), 6, 0};
        link_def.sleeping_disabled = true;
        link_def.inertia = edyn::matrix3x3{{edyn::vector3{0.01f, 0, 0}, edyn::vector3{0, 0.01f, 0}, edyn::vector3{0, 0, 0.01f}}};
        links[k] = edyn::make_rigidbody(registry, link_def);
        all.push_back(links[k]);
        const bool first = k == 0;
        edyn::make_constraint<edyn::hinge_constraint>(registry, prev, links[k], [&](edyn::hinge_constraint &h) {
            h.pivot = {first ? edyn::vector3{0, 0, 0} : edyn::vector3{0.25f, 0, 0}, edyn::vector3{-0.25f, 0, 0}};
            h.set_axes({0, 0, 1}, {0, 0, 1});
        });
        prev = links[k];
    }
    def.position = {12, 0.5f, 0};
    const entt::entity puck = edyn::make_rigidbody(registry, def);
    all.push_back(puck);
    const entt::entity wa = pile[0][1][1], wb = pile[1][1][1];   // a box of the bottom layer and one resting on it

    double t = 0;
    auto run = [&](int frames) {
        for (int f = 0; f < frames; ++f) {
            t += 1.0 / 60 + 1e-6;
            edyn::update(registry, t);
            std::vector<float> fr;
            for (entt::entity e : all) {
                const auto &p = registry.get<edyn::position>(e); const auto &q = registry.get<edyn::orientation>(e);
                const auto *vp = registry.try_get<edyn::linvel>(e); const auto *wp = registry.try_get<edyn::angvel>(e);   // (a static body may have none)
                const edyn::linvel v = vp ? *vp : edyn::linvel{}; const edyn::angvel w = wp ? *wp : edyn::angvel{};
                for (float x : {p.x, p.y, p.z, q.x, q.y, q.z, q.w, v.x, v.y, v.z, w.x, w.y, w.z}) fr.push_back(x);
            }
            tr.frames.push_back(fr);
        }
    };
    // an edit, the update that applies it, and the watched pair's contact entities on both sides of it
    auto edit = [&](auto &&what) {
        const int number = (int)tr.still_marked.size();
        tr.watched.push_back(contact_entities_of(registry, wa, wb));
        for (uint32_t e : tr.watched.back()) registry.emplace_or_replace<watched_mark>((entt::entity)e, watched_mark{number});
        what();
        run(1);
        tr.watched.push_back(contact_entities_of(registry, wa, wb));
        size_t marked = 0;
        for (uint32_t e : tr.watched.back())
            if (auto *m = registry.try_get<watched_mark>((entt::entity)e)) marked += m->edit == number ? 1 : 0;
        tr.still_marked.push_back(marked);
        run(9);
    };
    auto puck_weight = [&]() {
        auto &s = registry.ctx().get<edyn::detail::gpu_stepper>();
        uint32_t nm = 0; edynhip_num_manifolds(s.ctx, &nm);
        std::vector<edynhip_manifold> recs(nm); if (nm) edynhip_get_manifolds(s.ctx, recs.data(), nm, &nm);
        const uint32_t pi = registry.get<edyn::detail::body_index>(puck).value;
        float weight = 0;
        for (auto &r : recs) if (r.body[0] == pi || r.body[1] == pi) for (uint32_t k = 0; k < r.num_points; ++k) weight += r.pt[k].normal_impulse;
        return weight;
    };

    run(40);
    CHECK(contact_entities_of(registry, wa, wb).size() >= 2);
    edit([&] { edyn::set_rigidbody_mass(registry, puck, 4.0f); edyn::set_rigidbody_mass(registry, links[3], 0.5f); });
    run(20);
    tr.weight = puck_weight();   // a heavier body presses harder on the floor; its contact survived the edit
    edit([&] { edyn::set_rigidbody_friction(registry, puck, 0.0f); });
    edyn::rigidbody_apply_impulse(registry, puck, {8, 0, 0}, {0, 0, 0});   // 2 m/s on ice
    run(30);
    tr.ice_x = registry.get<edyn::position>(puck).x; tr.ice_v = registry.get<edyn::linvel>(puck).x;
    edit([&] { edyn::rigidbody_set_shape(registry, puck, edyn::shapes_variant_t{edyn::sphere_shape{0.5f}}); });
    tr.sphere = edyn::rigidbody_has_shape(registry, puck) && registry.all_of<edyn::sphere_shape>(puck) && !registry.all_of<edyn::box_shape>(puck);
    edit([&] {
        edyn::rigidbody_set_kind(registry, puck, edyn::rigidbody_kind::rb_kinematic);
        const auto p = registry.get<edyn::position>(puck);
        edyn::set_kinematic_position(registry, puck, {p.x, p.y + 0.5f, p.z}, 0.5f);
    });
    edit([&] { edyn::rigidbody_set_kind(registry, puck, edyn::rigidbody_kind::rb_dynamic); });
    edit([&] { edyn::set_rigidbody_inertia(registry, puck, edyn::matrix3x3{{edyn::vector3{0.9f, 0, 0}, edyn::vector3{0, 0.8f, 0}, edyn::vector3{0, 0, 0.7f}}}); });
    edit([&] { edyn::rigidbody_set_kind(registry, puck, edyn::rigidbody_kind::rb_static); });
    const float frozen_x = registry.get<edyn::position>(puck).x;
    run(10);
    tr.is_static = registry.all_of<edyn::static_tag>(puck);
    tr.frozen_dx = registry.get<edyn::position>(puck).x - frozen_x;
    tr.rebuilds = edyn::get_shim_timings(registry).context_rebuilds;
    edyn::detach(registry);
    return tr;
}

void check_effects(const Trace &tr) {
    CHECK(std::fabs(tr.weight - 4.0f * 9.8f / 60.0f) < 0.02f);
    CHECK(tr.ice_x > 12.8f && std::fabs(tr.ice_v - 2.0f) < 0.05f);
    CHECK(tr.sphere);
    CHECK(tr.is_static && tr.frozen_dx == 0.0f);
}
}  // namespace

int main() {
    std::setvbuf(stdout, nullptr, _IONBF, 0);
    const Trace in_place = run_program(edyn::execution_mode::sequential, false);
    const Trace rebuilt = run_program(edyn::execution_mode::sequential, true);
    CHECK(in_place.rebuilds == 0);
    CHECK(rebuilt.rebuilds >= 7);   // one per edit
    check_effects(in_place);
    check_effects(rebuilt);
    CHECK(in_place.frames.size() == rebuilt.frames.size());
    for (size_t f = 0; f < in_place.frames.size() && f < rebuilt.frames.size(); ++f)
        if (in_place.frames[f].size() != rebuilt.frames[f].size() ||
            std::memcmp(in_place.frames[f].data(), rebuilt.frames[f].data(), in_place.frames[f].size() * sizeof(float)) != 0) {
            size_t at = 0;
            while (at < in_place.frames[f].size() && std::memcmp(&in_place.frames[f][at], &rebuilt.frames[f][at], sizeof(float)) == 0) ++at;
            std::printf("FAILED: update %zu differs between the run in place and the rebuild (body %zu, component %zu: %.9g against %.9g)\n", f, at / 13, at % 13,
                        (double)in_place.frames[f][at], (double)rebuilt.frames[f][at]);
            ++failures;
            break;
        }
    // the watched pair: in place the same manifold and point entities on both sides of every edit; the rebuild makes them again
    CHECK(in_place.watched.size() == 14 && rebuilt.watched.size() == 14 && in_place.still_marked.size() == 7 && rebuilt.still_marked.size() == 7);
    for (size_t k = 0; k < in_place.still_marked.size() && 2 * k + 1 < in_place.watched.size(); ++k) {
        CHECK(in_place.watched[2 * k].size() >= 2);
        CHECK(in_place.watched[2 * k] == in_place.watched[2 * k + 1]);
        CHECK(in_place.still_marked[k] == in_place.watched[2 * k + 1].size());
    }
    for (size_t k = 0; k < rebuilt.still_marked.size() && 2 * k + 1 < rebuilt.watched.size(); ++k) {
        CHECK(rebuilt.watched[2 * k + 1].size() >= 2);
        CHECK(rebuilt.still_marked[k] == 0);
    }
    // asynchronous mode: the registry receives every update one update late; the edits stay in place and take effect
    const Trace async = run_program(edyn::execution_mode::asynchronous, false);
    CHECK(async.rebuilds == 0);
    check_effects(async);
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("BODY_EDITS_OK\n");
    return 0;
}
