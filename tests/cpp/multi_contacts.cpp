// Contact entities and step callbacks on init_config::devices = {0, 0}: the registry program a single device runs - materialize_contacts,
// contact_point_data, pre / post step callbacks, an edyn::refresh-ed kick from a callback, registry.destroy - run unchanged on a
// multi-device world, and the two registries agree at EVERY update: state and presentation bit for bit, the same contact_manifold
// entities (body pair, point count), the same number of contact_point entities, per manifold the same point data bit for bit,
// manifold_exists, and the callbacks' call counts. The shim reads the world's record hand-over in place
// (edynhip_world_snapshot_records / _map) and keeps the contact entities in step through the view's events.
//
// The scene is multi_shim.cpp's (four small piles, a hinge door, a ball), except that the ball starts behind the second pile and rolls
// into the third: two shards cut the piles between those two, so the run goes through an approach-triggered re-partition.
#include <edyn/edyn.hpp>
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s (update %d)\n", __FILE__, __LINE__, #c, g_update); return 1; } } while (0)

static int g_update = 0;
struct side {
    entt::registry registry;
    std::vector<entt::entity> bodies;
    int pre = 0, post = 0;
};
static side g_one, g_many;
static side &side_of(entt::registry &r) { return &r == &g_one.registry ? g_one : g_many; }
static void pre_step(entt::registry &r) { ++side_of(r).pre; }
static void post_step(entt::registry &r) {
    side &s = side_of(r);
    if (++s.post == 40) {   // a kick from inside the step loop: uploaded before the next step
        r.get<edyn::linvel>(s.bodies[20]) = edyn::linvel{{0, 3.0f, 0}};
        edyn::refresh(r);
    }
}

static void build(side &s) {
    entt::registry &registry = s.registry;
    auto floor_def = edyn::rigidbody_def{};
    floor_def.kind = edyn::rigidbody_kind::rb_static;
    floor_def.shape = edyn::plane_shape{{0, 1, 0}, 0};
    edyn::make_rigidbody(registry, floor_def);
    for (int site = 0; site < 4; ++site)
        for (int k = 0; k < 8; ++k) {
            auto def = edyn::rigidbody_def{};
            def.mass = 1;
            def.shape = edyn::box_shape{{0.5f, 0.5f, 0.5f}};
            def.position = {7.0f * site + 1.02f * (k % 2), 0.505f + 1.005f * ((k / 2) % 2), 1.02f * (k / 4)};
            def.sleeping_disabled = true;
            s.bodies.push_back(edyn::make_rigidbody(registry, def));
        }
    auto post = edyn::rigidbody_def{}; post.kind = edyn::rigidbody_kind::rb_static; post.position = {30.0f, 2.0f, 0};
    auto door = edyn::rigidbody_def{}; door.mass = 1; door.position = {31.0f, 2.0f, 0}; door.shape = edyn::box_shape{{0.5f, 0.5f, 0.1f}}; door.sleeping_disabled = true;
    const auto e_post = edyn::make_rigidbody(registry, post), e_door = edyn::make_rigidbody(registry, door);
    edyn::make_constraint<edyn::hinge_constraint>(registry, e_post, e_door, [](edyn::hinge_constraint &h) {
        h.pivot[0] = {0, 0, 0}; h.pivot[1] = {-1.0f, 0, 0}; h.set_axes({0, 0, 1}, {0, 0, 1});
    });
    s.bodies.push_back(e_door);
    auto ball = edyn::rigidbody_def{};
    ball.mass = 1; ball.shape = edyn::sphere_shape{0.5f}; ball.position = {10.2f, 0.5f, 0.5f}; ball.linvel = {4.0f, 0, 0}; ball.sleeping_disabled = true;
    s.bodies.push_back(edyn::make_rigidbody(registry, ball));
}

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static uint32_t index_of(entt::registry &registry, entt::entity e) {
    const auto *bi = registry.valid(e) ? registry.try_get<edyn::detail::body_index>(e) : nullptr;
    return bi ? bi->value : ~0u;
}
using manifold_row = std::array<uint32_t, 3>;    // body index A, body index B, points
using point_row = std::array<uint32_t, 15>;      // body index A, body index B, then the bits of pivotA pivotB normal distance normal_impulse friction_impulse
static void contacts_of(entt::registry &registry, std::vector<manifold_row> &manifolds, std::vector<point_row> &points) {
    manifolds.clear(); points.clear();
    registry.view<edyn::contact_manifold>().each([&](auto, edyn::contact_manifold &m) {
        manifolds.push_back({index_of(registry, m.body[0]), index_of(registry, m.body[1]), m.num_points});
    });
    registry.view<edyn::contact_point_list>().each([&](auto e, edyn::contact_point_list &l) {
        const auto &m = registry.get<edyn::contact_manifold>(l.parent);
        const auto &cp = registry.get<edyn::contact_point>(e);
        const auto &g = registry.get<edyn::contact_point_geometry>(e);
        const auto &imp = registry.get<edyn::contact_point_impulse>(e);
        points.push_back({index_of(registry, m.body[0]), index_of(registry, m.body[1]), bits(cp.pivotA.x), bits(cp.pivotA.y), bits(cp.pivotA.z),
                          bits(cp.pivotB.x), bits(cp.pivotB.y), bits(cp.pivotB.z), bits(cp.normal.x), bits(cp.normal.y), bits(cp.normal.z),
                          bits(g.distance), bits(imp.normal_impulse), bits(imp.friction_impulse[0]), bits(imp.friction_impulse[1])});
    });
    std::sort(manifolds.begin(), manifolds.end());
    std::sort(points.begin(), points.end());
}
template <typename T> static size_t count(entt::registry &registry) {
    size_t n = 0;
    registry.view<T>().each([&](auto, auto &) { ++n; });
    return n;
}
static uint32_t repartitions(entt::registry &registry) {
    auto &s = registry.ctx().get<edyn::detail::gpu_stepper>();
    edynhip_world_stats st{};
    return s.world && edynhip_world_get_stats(s.world, &st) == EDYNHIP_OK ? st.repartitions : 0u;
}

int main() {
    entt::registry &one = g_one.registry, &many = g_many.registry;
    auto cfg = edyn::init_config{};
    cfg.num_solver_velocity_iterations = 10;
    cfg.materialize_contacts = true;
    cfg.contact_point_data = true;
    edyn::attach(one, cfg);
    cfg.devices = {0, 0};
    edyn::attach(many, cfg);
    for (entt::registry *r : {&one, &many}) { edyn::set_pre_step_callback(*r, &pre_step); edyn::set_post_step_callback(*r, &post_step); }
    build(g_one); build(g_many);
    const std::vector<entt::entity> &b1 = g_one.bodies, &b2 = g_many.bodies;
    double t = 0;
    uint32_t seen_repartitions = 0, updates_that_repartitioned = 0;
    size_t most_points = 0;
    float ball_farthest = 0;
    std::vector<manifold_row> m1, m2;
    std::vector<point_row> p1, p2;
    for (g_update = 0; g_update < 150; ++g_update) {
        t += 1.0 / 60;
        edyn::update(one, t); edyn::update(many, t);
        ball_farthest = std::fmax(ball_farthest, many.get<edyn::position>(b2.back()).x);
        const uint32_t reps = repartitions(many);
        if (reps > seen_repartitions) { ++updates_that_repartitioned; seen_repartitions = reps; }
        for (size_t k = 0; k < b1.size(); ++k) {
            if (!one.valid(b1[k])) { REQUIRE(!many.valid(b2[k])); continue; }
            const auto &p = one.get<edyn::position>(b1[k]), &q = many.get<edyn::position>(b2[k]);
            const auto &o = one.get<edyn::orientation>(b1[k]), &u = many.get<edyn::orientation>(b2[k]);
            const auto &v = one.get<edyn::linvel>(b1[k]), &w = many.get<edyn::linvel>(b2[k]);
            const auto &a = one.get<edyn::angvel>(b1[k]), &c = many.get<edyn::angvel>(b2[k]);
            const auto &pp = one.get<edyn::present_position>(b1[k]), &pq = many.get<edyn::present_position>(b2[k]);
            const auto &po = one.get<edyn::present_orientation>(b1[k]), &pu = many.get<edyn::present_orientation>(b2[k]);
            const bool same = p.x == q.x && p.y == q.y && p.z == q.z && o.x == u.x && o.y == u.y && o.z == u.z && o.w == u.w &&
                              v.x == w.x && v.y == w.y && v.z == w.z && a.x == c.x && a.y == c.y && a.z == c.z;
            const bool same_present = pp.x == pq.x && pp.y == pq.y && pp.z == pq.z && po.x == pu.x && po.y == pu.y && po.z == pu.z && po.w == pu.w;
            if (!same || !same_present) {
                std::printf("FAILED: body %zu differs at update %d (%s; %.9g %.9g %.9g vs %.9g %.9g %.9g)\n", k, g_update, same ? "presentation" : "state", p.x, p.y, p.z, q.x, q.y, q.z);
                return 1;
            }
        }
        contacts_of(one, m1, p1); contacts_of(many, m2, p2);
        REQUIRE(m1 == m2);                                                                  // the same manifolds: body pair and point count
        REQUIRE(count<edyn::contact_point>(one) == count<edyn::contact_point>(many));
        REQUIRE(p1.size() == count<edyn::contact_point>(one) && p1 == p2);                  // per manifold the same points, bit for bit
        most_points = std::max(most_points, p1.size());
        REQUIRE(edyn::manifold_exists(one, b1[2], b1[0]) == edyn::manifold_exists(many, b2[2], b2[0]));
        REQUIRE(edyn::manifold_exists(one, b1[0], b1[31]) == edyn::manifold_exists(many, b2[0], b2[31]));
        if (g_update >= 30) {   // box 2 rests on box 0; the first and the last pile never meet
            REQUIRE(edyn::manifold_exists(many, b2[2], b2[0]) && many.all_of<edyn::contact_manifold>(edyn::get_manifold_entity(many, b2[2], b2[0])));
            REQUIRE(!edyn::manifold_exists(many, b2[0], b2[31]));
            size_t n1 = 0, n2 = 0;
            edyn::visit_neighbors(one, b1[2], [&](entt::entity) { ++n1; });
            edyn::visit_neighbors(many, b2[2], [&](entt::entity) { ++n2; });
            REQUIRE(n1 == n2 && n2 >= 1);
        }
        REQUIRE(g_one.pre == g_many.pre && g_one.post == g_many.post && g_one.pre == g_one.post);
        if (g_update == 100) { one.destroy(b1[3]); many.destroy(b2[3]); }
    }
    REQUIRE(g_many.post >= 140);                                              // a callback pair per fixed step
    REQUIRE(most_points > 32);                                                // the piles' contacts were mirrored (and compared)
    REQUIRE(ball_farthest > 12.8f);                                           // the ball reached the third pile
    REQUIRE(many.get<edyn::linvel>(b2[20]).y < 2.9f);                        // the kick from the callback was taken, gravity worked on it since
    REQUIRE(updates_that_repartitioned >= 1);                                 // ... across a re-partition of the multi-device world
    std::printf("MULTI_CONTACTS_OK (%u re-partitions, %d steps, at most %zu points)\n", seen_repartitions, g_many.post, most_points);
    return 0;
}
