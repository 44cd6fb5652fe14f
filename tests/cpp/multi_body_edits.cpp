// Bodies edited and woken on a running multi-device world through the C++ drop-in shim (init_config::devices): set_rigidbody_mass /
// _inertia / _friction, rigidbody_set_shape, rigidbody_set_kind there and back and wake_up_entity reach the world in place
// (edynhip_world_edit_bodies / edynhip_world_wake_bodies). The registry program of body_edits.cpp - a 4x4x4 pile, a hinge chain, a puck,
// ten updates between the edits - runs on one device and on two shards of device 0:
//   checks   position, orientation, velocities and the sleeping tag of every body bitwise equal after every update;
//            context_rebuilds == 0 on the world; the contact entities of two resting pile boxes that no edit touches are the same entities
//            across every edit; with init_config::rebuild_on_body_edit on the world they are made again (the A/B switch still works);
//            with island sleeping on, wake_up_entity wakes the pile - and nobody else - with the next update on the world as on one device, a
//            mass edit wakes nobody and a shape edit wakes the edited body. (The sleeping runs are not compared bit for bit: one device
//            steps on the update's time stamps, edynhip_step_timed, the world on its step count, so an island's sleep timer may run out one
//            step apart; tests/test_world_body_edits.py holds the wake to the one context bit for bit where both count the same clock.)
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
    std::vector<std::vector<float>> frames;         // 14 floats per body after every update: the state and the sleeping tag
    std::vector<std::set<uint32_t>> watched;        // the watched pair's contact entities (manifold + points) around every edit: before, after
    std::vector<size_t> still_marked;               // per edit: how many of the entities after it carry the mark put on the ones before it
    uint64_t rebuilds = 0;
    bool sphere = false, is_static = false;
    bool slept = false, woke = false, others_slept_on = false, mass_woke_nobody = false, shape_woke_the_puck = false;   // the sleeping run
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

Trace run_program(bool shards, bool rebuild, bool sleeping) {
    Trace tr;
    entt::registry registry;
    auto config = edyn::init_config{};
    config.num_solver_velocity_iterations = 10;
    config.rebuild_on_body_edit = rebuild;
    config.island_sleeping = sleeping;
    config.max_bodies = 128;
    if (shards) config.devices = {0, 0};
    edyn::attach(registry, config);

    std::vector<entt::entity> all;
    auto floor_def = edyn::rigidbody_def{};
    floor_def.kind = edyn::rigidbody_kind::rb_static;
    floor_def.shape = edyn::plane_shape{{0, 1, 0}, 0};
    all.push_back(edyn::make_rigidbody(registry, floor_def));

    auto def = edyn::rigidbody_def{};
    def.shape = edyn::box_shape{{0.5f, 0.5f, 0.5f}};
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
                fr.push_back(registry.all_of<edyn::sleeping_tag>(e) ? 1.0f : 0.0f);
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

    if (sleeping) {   // the pile falls asleep; wake_up_entity of one of its boxes wakes it, and only it
        for (int k = 0; k < 20 && !registry.all_of<edyn::sleeping_tag>(wa); ++k) run(30);
        tr.slept = registry.all_of<edyn::sleeping_tag>(wa) && registry.all_of<edyn::sleeping_tag>(wb);
        for (int k = 0; k < 4 && !registry.all_of<edyn::sleeping_tag>(puck); ++k) run(30);
        tr.slept = tr.slept && registry.all_of<edyn::sleeping_tag>(puck);
        edyn::wake_up_entity(registry, wb);
        run(1);
        tr.woke = !registry.all_of<edyn::sleeping_tag>(wa) && !registry.all_of<edyn::sleeping_tag>(wb);
        tr.others_slept_on = registry.all_of<edyn::sleeping_tag>(puck);
        run(10);
        // an edit of a sleeping world: the mass wakes nobody, the shape wakes the puck's island
        edit([&] { edyn::set_rigidbody_mass(registry, puck, 4.0f); });
        tr.mass_woke_nobody = registry.all_of<edyn::sleeping_tag>(puck);
        tr.watched.push_back(contact_entities_of(registry, wa, wb));
        edyn::rigidbody_set_shape(registry, puck, edyn::shapes_variant_t{edyn::sphere_shape{0.5f}});
        run(1);
        tr.shape_woke_the_puck = !registry.all_of<edyn::sleeping_tag>(puck);
        tr.rebuilds = edyn::get_shim_timings(registry).context_rebuilds;
        edyn::detach(registry);
        return tr;
    }
    run(40);
    CHECK(contact_entities_of(registry, wa, wb).size() >= 2);
    edit([&] { edyn::set_rigidbody_mass(registry, puck, 4.0f); edyn::set_rigidbody_mass(registry, links[3], 0.5f); });
    run(20);
    edit([&] { edyn::set_rigidbody_friction(registry, puck, 0.0f); });
    edyn::rigidbody_apply_impulse(registry, puck, {8, 0, 0}, {0, 0, 0});   // 2 m/s on ice
    run(30);
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
    tr.is_static = registry.all_of<edyn::static_tag>(puck) && registry.get<edyn::position>(puck).x == frozen_x;
    tr.rebuilds = edyn::get_shim_timings(registry).context_rebuilds;
    edyn::detach(registry);
    return tr;
}

void same_frames(const Trace &a, const Trace &b, const char *what) {
    CHECK(a.frames.size() == b.frames.size());
    for (size_t f = 0; f < a.frames.size() && f < b.frames.size(); ++f)
        if (a.frames[f].size() != b.frames[f].size() || std::memcmp(a.frames[f].data(), b.frames[f].data(), a.frames[f].size() * sizeof(float)) != 0) {
            size_t at = 0;
            while (at < a.frames[f].size() && std::memcmp(&a.frames[f][at], &b.frames[f][at], sizeof(float)) == 0) ++at;
            std::printf("FAILED: %s: update %zu differs (body %zu, component %zu: %.9g against %.9g)\n", what, f, at / 14, at % 14, (double)a.frames[f][at], (double)b.frames[f][at]);
            ++failures;
            return;
        }
}
}  // namespace

int main() {
    std::setvbuf(stdout, nullptr, _IONBF, 0);
    const Trace one = run_program(false, false, false);
    const Trace world = run_program(true, false, false);
    CHECK(one.rebuilds == 0 && world.rebuilds == 0);
    CHECK(one.sphere && world.sphere && one.is_static && world.is_static);
    same_frames(one, world, "one device against two shards");
    // the watched pair: the same manifold and point entities on both sides of every edit, on one device and on the world
    for (const Trace *tr : {&one, &world}) {
        CHECK(tr->watched.size() == 14 && tr->still_marked.size() == 7);
        for (size_t k = 0; k < tr->still_marked.size() && 2 * k + 1 < tr->watched.size(); ++k) {
            CHECK(tr->watched[2 * k].size() >= 2);
            CHECK(tr->watched[2 * k] == tr->watched[2 * k + 1]);
            CHECK(tr->still_marked[k] == tr->watched[2 * k + 1].size());
        }
    }
    // the A/B switch on the world: every edit makes the world again, and with it the watched pair's entities
    const Trace rebuilt = run_program(true, true, false);
    CHECK(rebuilt.rebuilds >= 7);
    CHECK(rebuilt.still_marked.size() == 7);
    for (size_t k = 0; k < rebuilt.still_marked.size() && 2 * k + 1 < rebuilt.watched.size(); ++k) {
        CHECK(rebuilt.watched[2 * k + 1].size() >= 2);
        CHECK(rebuilt.still_marked[k] == 0);
    }
    // island sleeping on: wake_up_entity and the edits of a sleeping world
    const Trace one_s = run_program(false, false, true);
    const Trace world_s = run_program(true, false, true);
    for (const Trace *tr : {&one_s, &world_s}) {
        CHECK(tr->slept && tr->woke && tr->others_slept_on);
        CHECK(tr->mass_woke_nobody && tr->shape_woke_the_puck);
        CHECK(tr->rebuilds == 0);
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("MULTI_BODY_EDITS_OK\n");
    return 0;
}
