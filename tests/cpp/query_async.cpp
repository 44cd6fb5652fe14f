// edyn::raycast_async / query_aabb_async / query_aabb_of_interest_async through the shim in execution_mode::asynchronous
// (include/edyn/collision/raycast.hpp:170-182, query_aabb.hpp:37-44). A scene of a floor, a row of boxes (every other one static), a
// few falling boxes and a hinge is run twice over the same times: in sequential mode, where edyn::raycast / query_*_aabb and the
// island labels give the expected answers after every update, and in asynchronous mode, where the same requests are made after every
// update and must arrive during the next one - once each, in id order, with the same bits, while the registry holds the state the
// sequential run had after that update. Then: requests before the first update, inside a delegate, on a destroyed entity, pending at
// detach, query_islands, and the sequential modes' refusals. Built with EDYN_QUERY_IDS_CAPACITY = 4 (query_async_small.cpp) it runs the
// capacity overflow instead. Prints QUERY_ASYNC_OK 1 when every check holds.
#include <edyn/edyn.hpp>
#include <edyn/collision/raycast.hpp>
#include <edyn/collision/query_aabb.hpp>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++failures; } } while (0)

constexpr int kUpdates = 12, kRays = 16, kBoxes = 4;

struct Scene {
    std::vector<entt::entity> bodies;     // creation order = body index
    std::vector<bool> dynamic;
    std::vector<entt::entity> all;        // bodies, then the constraint
    entt::entity floor, hinge;
};
static Scene build(entt::registry &registry) {
    Scene sc;
    auto add = [&](const edyn::rigidbody_def &def) {
        sc.bodies.push_back(edyn::make_rigidbody(registry, def));
        sc.dynamic.push_back(def.kind == edyn::rigidbody_kind::rb_dynamic);
        return sc.bodies.back();
    };
    auto def = edyn::rigidbody_def{};
    def.kind = edyn::rigidbody_kind::rb_static;
    def.shape = edyn::plane_shape{{0, 1, 0}, 0};
    sc.floor = add(def);
    for (int i = 0; i < 10; ++i) {   // the row: every other box static
        auto d = edyn::rigidbody_def{};
        d.kind = i % 2 ? edyn::rigidbody_kind::rb_static : edyn::rigidbody_kind::rb_dynamic;
        d.shape = edyn::box_shape{{0.5f, 0.5f, 0.5f}};
        d.position = {-6.0f + 1.02f * i, 0.5f, 0};
        add(d);
    }
    for (int i = 0; i < 6; ++i) {   // falling boxes, some onto the row, two far from it
        auto d = edyn::rigidbody_def{};
        d.shape = edyn::box_shape{{0.4f, 0.4f, 0.4f}};
        d.position = {i < 4 ? -5.7f + 2.1f * i : 8.0f + 3.0f * (i - 4), 1.7f + 0.45f * i, 0.1f * i};
        add(d);
    }
    sc.hinge = edyn::make_constraint<edyn::hinge_constraint>(registry, sc.bodies[15], sc.bodies[16], [](edyn::hinge_constraint &h) {
        h.pivot = {edyn::vector3{1.5f, 0, 0}, edyn::vector3{-1.5f, 0, 0}};
        h.set_axes({0, 0, 1}, {0, 0, 1});
    });
    sc.all = sc.bodies;
    sc.all.push_back(sc.hinge);
    return sc;
}
static int index_of(const Scene &sc, entt::entity e) {
    if (e == entt::entity{entt::null}) return -1;
    const auto it = std::find(sc.all.begin(), sc.all.end(), e);
    return it == sc.all.end() ? -2 : (int)(it - sc.all.begin());
}
static void ray(int i, edyn::vector3 &p0, edyn::vector3 &p1) {
    if (i < 10) { p0 = {-6.2f + 1.3f * i, 6, 0.05f * i}; p1 = {-6.0f + 1.25f * i, -1, 0.02f * i}; }        // down onto the row and the fallers
    else if (i < 13) { p0 = {-9, 0.45f + 0.3f * (i - 10), 0.1f}; p1 = {14, 0.5f + 0.2f * (i - 10), 0}; }   // along the row
    else { p0 = {8.0f + 3.0f * (i - 13), 7, 0.45f}; p1 = {8.1f + 3.0f * (i - 13), -2, 0.4f}; }             // onto the hinged pair
}
static std::vector<entt::entity> ignore_of(const Scene &sc, int i) {
    if (i % 4 == 1) return {sc.floor};
    if (i % 4 == 2) return {sc.bodies[11], sc.bodies[1], sc.bodies[15]};
    if (i % 4 == 3) return {sc.bodies[2], sc.bodies[2], sc.floor, sc.bodies[16]};
    return {};
}
static edyn::AABB box(int i) {
    if (i == 0) return {{-4.6f, 0.2f, -0.4f}, {-3.4f, 0.8f, 0.4f}};   // about one box of the row
    if (i == 1) return {{-100, -100, -100}, {100, 100, 100}};       // everything
    if (i == 2) return {{7.6f, 0, -1}, {8.4f, 9, 1}};               // the first of the hinged pair
    return {{50, 50, 50}, {51, 51, 51}};                            // nothing
}
static double time_of(int update) { return update * (1.0 / 60 + 1e-6); }

struct Answer {
    std::vector<edyn::raycast_result> rays;
    std::vector<int> ray_body;
    std::vector<int> proc[kBoxes], nonproc[kBoxes], interest[kBoxes];
    std::vector<edyn::vector3> pos;
};
static std::vector<int> indices(const Scene &sc, const std::vector<entt::entity> &v) {
    std::vector<int> out;
    for (auto e : v) out.push_back(index_of(sc, e));
    return out;
}
static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; }
static bool same_info(const edyn::raycast_result &a, const edyn::raycast_result &b) {
    if (a.info_var.index() != b.info_var.index()) return false;
    if (auto *x = std::get_if<edyn::box_raycast_info>(&a.info_var)) return x->face_index == std::get<edyn::box_raycast_info>(b.info_var).face_index;
    if (auto *x = std::get_if<edyn::cylinder_raycast_info>(&a.info_var)) {
        const auto &y = std::get<edyn::cylinder_raycast_info>(b.info_var);
        return x->feature == y.feature && x->face_index == y.face_index;
    }
    if (auto *x = std::get_if<edyn::capsule_raycast_info>(&a.info_var)) {
        const auto &y = std::get<edyn::capsule_raycast_info>(b.info_var);
        return x->feature == y.feature && x->hemisphere_index == y.hemisphere_index;
    }
    if (auto *x = std::get_if<edyn::polyhedron_raycast_info>(&a.info_var)) return x->face_index == std::get<edyn::polyhedron_raycast_info>(b.info_var).face_index;
    return std::holds_alternative<std::monostate>(a.info_var);   // (the shim reports no other kind)
}

// the sequential run: what the synchronous calls answer now
static Answer record(entt::registry &registry, const Scene &sc) {
    Answer a;
    for (int i = 0; i < kRays; ++i) {
        edyn::vector3 p0, p1;
        ray(i, p0, p1);
        a.rays.push_back(edyn::raycast(registry, p0, p1, ignore_of(sc, i)));
        a.ray_body.push_back(index_of(sc, a.rays.back().entity));
    }
    edynhip_ctx *ctx = registry.ctx().get<edyn::detail::gpu_stepper>().ctx;
    const uint32_t n = (uint32_t)sc.bodies.size();
    std::vector<uint32_t> label(n);
    CHECK(edynhip_get_derived(ctx, nullptr, nullptr, label.data()) == EDYNHIP_OK);
    for (int i = 0; i < kBoxes; ++i) {
        const edyn::AABB b = box(i);
        std::vector<entt::entity> got;
        edyn::query_procedural_aabb(registry, b, [&](entt::entity e) { got.push_back(e); });
        a.proc[i] = indices(sc, got);
        got.clear();
        edyn::query_non_procedural_aabb(registry, b, [&](entt::entity e) { got.push_back(e); });
        a.nonproc[i] = indices(sc, got);
        // of interest: the dynamic bodies of the islands the box meets, then the constraints that hold one
        const float b6[6] = {b.min.x, b.min.y, b.min.z, b.max.x, b.max.y, b.max.z};
        uint32_t off[2] = {0, 0}, total = 0;
        CHECK(edynhip_query_aabb(ctx, EDYNHIP_QUERY_ISLANDS, 1, b6, 0, off, nullptr, 0, &total) == EDYNHIP_OK);
        std::vector<uint32_t> islands(total + 1);
        if (total) CHECK(edynhip_query_aabb(ctx, EDYNHIP_QUERY_ISLANDS, 1, b6, 0, off, islands.data(), total, &total) == EDYNHIP_OK);
        islands.resize(total);
        for (uint32_t k = 0; k < n; ++k)
            if (sc.dynamic[k] && std::find(islands.begin(), islands.end(), label[k]) != islands.end()) a.interest[i].push_back((int)k);
        const bool holds = std::find(a.interest[i].begin(), a.interest[i].end(), 15) != a.interest[i].end() ||
                           std::find(a.interest[i].begin(), a.interest[i].end(), 16) != a.interest[i].end();
        if (holds) a.interest[i].push_back((int)n);   // the hinge: index n in Scene::all
    }
    for (auto e : sc.bodies) a.pos.push_back(registry.get<edyn::position>(e));
    return a;
}

struct Probe {   // what the asynchronous run's delegates note
    int update = 0;           // the update in progress (0: none)
    bool in_update = false;
    int fired = 0, out_of_turn = 0;
    unsigned last_ray = 0, last_box = 0;
    bool any_ray = false, any_box = false;
};

#if __has_include(<entt/entt.hpp>)
static int delegate_rays = 0, delegate_boxes = 0;
static void on_ray_delegate(edyn::raycast_id_type, const edyn::raycast_result &r, edyn::vector3, edyn::vector3) { delegate_rays += r.entity != entt::entity{entt::null}; }
static void on_box_delegate(edyn::query_aabb_id_type, const edyn::query_aabb_result &r) { delegate_boxes += (int)r.procedural_entities.size(); }
#endif

[[maybe_unused]] static void run_main() {
    std::vector<Answer> expected;   // [k]: after update k (0: before the first)
    {
        entt::registry registry;
        auto config = edyn::init_config{};
        config.execution_mode = edyn::execution_mode::sequential;
        edyn::attach(registry, config);
        const Scene sc = build(registry);
        expected.push_back(record(registry, sc));
        for (int u = 1; u <= kUpdates; ++u) {
            edyn::update(registry, time_of(u));
            expected.push_back(record(registry, sc));
        }
        // the scene does what the test needs: something moved, the hinged pair is one island, the everything-box lists every body
        CHECK(!same_bits(expected[0].pos[11].y, expected[kUpdates].pos[11].y));
        CHECK(expected[kUpdates].interest[2].size() == 3 && expected[kUpdates].interest[1].size() == 12);
        CHECK(expected[3].proc[1].size() == 11 && expected[3].nonproc[1].size() == 6 && expected[3].proc[3].empty());
        int hit = 0;
        for (int i = 0; i < kRays; ++i) hit += expected[kUpdates].ray_body[i] >= 0;
        CHECK(hit >= 10);
        edyn::detach(registry);
    }
    entt::registry registry;
    auto config = edyn::init_config{};
    config.execution_mode = edyn::execution_mode::asynchronous;
    edyn::attach(registry, config);
    const Scene sc = build(registry);
    Probe pr;
    std::vector<unsigned> ray_ids, box_ids;
    auto request = [&](int issued) {   // the same requests as the sequential run's record(): answered by update issued + 1
        const Answer &want = expected[(size_t)issued];
        for (int i = 0; i < kRays; ++i) {
            edyn::vector3 p0, p1;
            ray(i, p0, p1);
            const unsigned id = edyn::raycast_async(registry, p0, p1, [&, i, issued, p0, p1](edyn::raycast_id_type rid, const edyn::raycast_result &r, edyn::vector3 a, edyn::vector3 b) {
                ++pr.fired;
                if (!pr.in_update || pr.update != issued + 1) ++pr.out_of_turn;
                CHECK(!pr.any_ray || rid > pr.last_ray);
                pr.any_ray = true; pr.last_ray = rid;
                CHECK(std::memcmp(&a, &p0, sizeof a) == 0 && std::memcmp(&b, &p1, sizeof b) == 0);
                const edyn::raycast_result &e = want.rays[(size_t)i];
                CHECK(index_of(sc, r.entity) == want.ray_body[(size_t)i]);
                CHECK(same_bits(r.fraction, e.fraction));
                CHECK(same_bits(r.normal.x, e.normal.x) && same_bits(r.normal.y, e.normal.y) && same_bits(r.normal.z, e.normal.z));
                CHECK(same_info(r, e));
                if (r.entity != entt::entity{entt::null}) {   // the registry holds the state the ray was answered on
                    const edyn::vector3 p = registry.get<edyn::position>(r.entity), q = want.pos[(size_t)want.ray_body[(size_t)i]];
                    CHECK(same_bits(p.x, q.x) && same_bits(p.y, q.y) && same_bits(p.z, q.z));
                }
            }, ignore_of(sc, i));
            ray_ids.push_back(id);
        }
        for (int i = 0; i < kBoxes; ++i) {
            auto check_order = [&pr, issued](edyn::query_aabb_id_type qid) {
                ++pr.fired;
                if (!pr.in_update || pr.update != issued + 1) ++pr.out_of_turn;
                CHECK(!pr.any_box || qid > pr.last_box);
                pr.any_box = true; pr.last_box = qid;
            };
            box_ids.push_back(edyn::query_aabb_async(registry, box(i), [&, i, check_order](edyn::query_aabb_id_type qid, const edyn::query_aabb_result &r) {
                check_order(qid);
                CHECK(indices(sc, r.procedural_entities) == want.proc[i]);
                CHECK(indices(sc, r.non_procedural_entities) == want.nonproc[i]);
                CHECK(r.island_entities.empty());
            }, true, true, false));
            box_ids.push_back(edyn::query_aabb_of_interest_async(registry, box(i), [&, i, check_order](edyn::query_aabb_id_type qid, const edyn::query_aabb_result &r) {
                check_order(qid);
                CHECK(indices(sc, r.procedural_entities) == want.interest[i]);
                CHECK(indices(sc, r.non_procedural_entities) == want.nonproc[i]);
                CHECK(r.island_entities.empty());
            }));
        }
    };
    request(0);   // before the first update: answered for the initial state
    CHECK(pr.fired == 0);
    const int per_update = kRays + 2 * kBoxes;
    for (int u = 1; u <= kUpdates + 1; ++u) {
        pr.update = u; pr.in_update = true;
        edyn::update(registry, time_of(u));
        pr.in_update = false;
        CHECK(pr.fired == per_update * u);   // each delegate exactly once, during the update after its request
        if (u <= kUpdates) request(u);
        CHECK(pr.fired == per_update * u);   // ... and not before
    }
    CHECK(pr.out_of_turn == 0);
    for (size_t k = 1; k < ray_ids.size(); ++k) CHECK(ray_ids[k] == ray_ids[k - 1] + 1);   // ids ascend per kind
    for (size_t k = 1; k < box_ids.size(); ++k) CHECK(box_ids[k] == box_ids[k - 1] + 1);
    edyn::update(registry, time_of(kUpdates + 2));   // nothing pending: nobody is called
    CHECK(pr.fired == per_update * (kUpdates + 1));

    // a request made inside a delegate arrives one update later
    int outer_at = 0, inner_at = 0, now = 0;
    edyn::raycast_async(registry, edyn::vector3{0, 6, 0}, edyn::vector3{0, -1, 0}, [&](edyn::raycast_id_type, const edyn::raycast_result &, edyn::vector3, edyn::vector3) {
        outer_at = now;
        edyn::raycast_async(registry, edyn::vector3{0, 6, 0}, edyn::vector3{0, -1, 0},
                            [&](edyn::raycast_id_type, const edyn::raycast_result &r, edyn::vector3, edyn::vector3) { inner_at = now; CHECK(r.entity != entt::entity{entt::null}); });
        edyn::query_aabb_async(registry, box(1), [&](edyn::query_aabb_id_type, const edyn::query_aabb_result &r) { CHECK(inner_at == now && r.procedural_entities.size() == 11); }, true, false, false);
    });
    int t = kUpdates + 2;
    now = 1; edyn::update(registry, time_of(++t));
    CHECK(outer_at == 1 && inner_at == 0);
    now = 2; edyn::update(registry, time_of(++t));
    CHECK(outer_at == 1 && inner_at == 2);

    // edits made since the last update are not seen - also when a body was made since, which goes up in the same update
    {
        const entt::entity mover = sc.bodies[12];
        const edyn::vector3 was = registry.get<edyn::position>(mover);
        int seen = 0;
        auto probe = [&](bool expect_mover) {
            edyn::raycast_async(registry, edyn::vector3{was.x, was.y + 5, was.z}, edyn::vector3{was.x, was.y - 0.1f, was.z},
                                [&, expect_mover](edyn::raycast_id_type, const edyn::raycast_result &r, edyn::vector3, edyn::vector3) { ++seen; CHECK((r.entity == mover) == expect_mover); });
        };
        probe(true);
        registry.get<edyn::position>(mover) = edyn::position{edyn::vector3{was.x, was.y + 30, was.z}};
        edyn::refresh(registry);
        auto d = edyn::rigidbody_def{};
        d.kind = edyn::rigidbody_kind::rb_static;
        d.shape = edyn::box_shape{{0.5f, 0.5f, 0.5f}};
        d.position = {40, 0.5f, 40};
        edyn::make_rigidbody(registry, d);
        edyn::update(registry, time_of(++t));   // answered where the body was when the last update ended
        CHECK(seen == 1);
        probe(false);
        edyn::update(registry, time_of(++t));   // the edit went up with that update: now the ray passes where the body was
        CHECK(seen == 2);
    }

    // an entity destroyed between request and flush is never reported, and drops out of an ignore list
    const entt::entity victim = sc.bodies[16];
    int answered = 0;
    const edyn::vector3 vp = registry.get<edyn::position>(victim);
    edyn::raycast_async(registry, edyn::vector3{vp.x, vp.y + 5, vp.z}, edyn::vector3{vp.x, -2, vp.z},
                        [&](edyn::raycast_id_type, const edyn::raycast_result &r, edyn::vector3, edyn::vector3) { ++answered; CHECK(r.entity == sc.floor); });
    edyn::raycast_async(registry, edyn::vector3{vp.x, vp.y + 5, vp.z}, edyn::vector3{vp.x, -2, vp.z},
                        [&](edyn::raycast_id_type, const edyn::raycast_result &r, edyn::vector3, edyn::vector3) { ++answered; CHECK(r.entity == entt::entity{entt::null}); }, {victim, sc.floor});
    auto without_victim = [&](edyn::query_aabb_id_type, const edyn::query_aabb_result &r) {
        ++answered;
        CHECK(std::find(r.procedural_entities.begin(), r.procedural_entities.end(), victim) == r.procedural_entities.end());
        CHECK(std::find(r.procedural_entities.begin(), r.procedural_entities.end(), sc.hinge) == r.procedural_entities.end());   // the hinge went with its body
        CHECK(r.procedural_entities.size() == 10);
    };
    edyn::query_aabb_async(registry, box(1), without_victim, true, true, false);
    edyn::query_aabb_of_interest_async(registry, box(1), without_victim);
    registry.destroy(victim);
    edyn::update(registry, time_of(++t));
    CHECK(answered == 4);

    // query_islands: no island entities here
    bool threw = false;
    try { edyn::query_aabb_async(registry, box(1), [](edyn::query_aabb_id_type, const edyn::query_aabb_result &) {}, true, true, true); }
    catch (const edyn::stepper_error &) { threw = true; }
    CHECK(threw);

#if __has_include(<entt/entt.hpp>)
    {   // the reference's delegate aliases
        edyn::raycast_delegate_type on_ray{entt::connect_arg<&on_ray_delegate>};
        edyn::query_aabb_delegate_type on_box{entt::connect_arg<&on_box_delegate>};
        edyn::raycast_async(registry, edyn::vector3{0, 6, 0}, edyn::vector3{0, -1, 0}, on_ray);
        edyn::query_aabb_async(registry, box(1), on_box, true, false, false);
        edyn::query_aabb_of_interest_async(registry, box(1), on_box);
        edyn::update(registry, time_of(++t));
        CHECK(delegate_rays == 1 && delegate_boxes == 20);
    }
#endif

    // detach with requests pending: dropped, nobody is called
    int late = 0;
    edyn::raycast_async(registry, edyn::vector3{0, 6, 0}, edyn::vector3{0, -1, 0}, [&](edyn::raycast_id_type, const edyn::raycast_result &, edyn::vector3, edyn::vector3) { ++late; });
    edyn::query_aabb_of_interest_async(registry, box(1), [&](edyn::query_aabb_id_type, const edyn::query_aabb_result &) { ++late; });
    edyn::detach(registry);
    CHECK(late == 0);
}

[[maybe_unused]] static void run_sequential_refusals() {
    for (auto mode : {edyn::execution_mode::sequential, edyn::execution_mode::sequential_multithreaded}) {
        entt::registry registry;
        auto config = edyn::init_config{};
        config.execution_mode = mode;
        edyn::attach(registry, config);
        int threw = 0, called = 0;
        auto on_box = [&](edyn::query_aabb_id_type, const edyn::query_aabb_result &) { ++called; };
        try { edyn::raycast_async(registry, edyn::vector3{0, 1, 0}, edyn::vector3{0, -1, 0}, [&](edyn::raycast_id_type, const edyn::raycast_result &, edyn::vector3, edyn::vector3) { ++called; }); }
        catch (const edyn::stepper_error &) { ++threw; }
        try { edyn::query_aabb_async(registry, box(1), on_box, true, true, false); } catch (const edyn::stepper_error &) { ++threw; }
        try { edyn::query_aabb_of_interest_async(registry, box(1), on_box); } catch (const edyn::stepper_error &) { ++threw; }
        edyn::update(registry, 1.0);
        CHECK(threw == 3 && called == 0);
        edyn::detach(registry);
    }
}

// EDYN_QUERY_IDS_CAPACITY = 4: a request whose lists need more ids arrives one update later than it would, complete
[[maybe_unused]] static void run_overflow() {
    entt::registry registry;
    auto config = edyn::init_config{};
    config.execution_mode = edyn::execution_mode::asynchronous;
    edyn::attach(registry, config);
    const Scene sc = build(registry);
    int now = 0, small_at = 0, big_at = 0, next_at = 0;
    edyn::update(registry, time_of(++now));
    edyn::query_aabb_async(registry, box(3), [&](edyn::query_aabb_id_type, const edyn::query_aabb_result &r) { small_at = now; CHECK(r.procedural_entities.empty()); }, true, true, false);
    edyn::update(registry, time_of(++now));
    CHECK(small_at == 2);   // within the capacity: the next update
    edyn::query_aabb_async(registry, box(1), [&](edyn::query_aabb_id_type, const edyn::query_aabb_result &r) {
        big_at = now;
        CHECK(r.procedural_entities.size() == 11 && r.non_procedural_entities.size() == 6);
        for (size_t k = 0; k < r.procedural_entities.size(); ++k) CHECK(sc.dynamic[(size_t)index_of(sc, r.procedural_entities[k])]);
        for (size_t k = 1; k < r.procedural_entities.size(); ++k) CHECK(index_of(sc, r.procedural_entities[k - 1]) < index_of(sc, r.procedural_entities[k]));
    }, true, true, false);
    edyn::update(registry, time_of(++now));
    CHECK(big_at == 0);     // 17 ids do not fit 4: asked again with the total
    edyn::query_aabb_of_interest_async(registry, box(1), [&](edyn::query_aabb_id_type, const edyn::query_aabb_result &r) { next_at = now; CHECK(r.procedural_entities.size() == 12); });
    edyn::update(registry, time_of(++now));
    CHECK(big_at == 4);     // one update later, complete
    CHECK(next_at == 4);    // later tickets start with that room: its 17 ids fit at once
    edyn::detach(registry);
}

int main() {
#if EDYN_QUERY_IDS_CAPACITY < 64
    run_overflow();
#else
    run_main();
    run_sequential_refusals();
#endif
    std::printf("QUERY_ASYNC_OK %d\n", failures == 0 ? 1 : 0);
    return failures == 0 ? 0 : 1;
}
