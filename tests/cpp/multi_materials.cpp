// edyn::attach with init_config::devices and materials: `material` with its contact_extras fields (rolling / spinning friction, soft
// contacts), material ids and edyn::insert_material_mixing on ONE simulation over two shards (both on the one GPU of the test box).
// The application code is the reference's; the trajectory and the contact points' data must equal the same registry program on one
// device, bit for bit, through the re-partition the rolling ball forces, a table entry inserted, a body made and materials changed
// (edyn::refresh<edyn::material>) while the world runs. The contact entities carry no material fields, so friction, restitution and the
// points' extras are compared where they live: edynhip_get_manifolds / _get_point_extras of the one context against the world's.
#include <edyn/edyn.hpp>
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static void build(entt::registry &registry, std::vector<entt::entity> &bodies, entt::entity &roller) {
    auto floor_def = edyn::rigidbody_def{};
    floor_def.kind = edyn::rigidbody_kind::rb_static;
    floor_def.shape = edyn::plane_shape{{0, 1, 0}, 0};
    floor_def.material->spin_friction = 0.05f; floor_def.material->roll_friction = 0.005f; floor_def.material->id = 0;
    edyn::make_rigidbody(registry, floor_def);
    for (int site = 0; site < 4; ++site)
        for (int k = 0; k < 8; ++k) {
            auto def = edyn::rigidbody_def{};
            def.mass = 1;
            def.shape = edyn::box_shape{{0.5f, 0.5f, 0.5f}};
            def.position = {7.0f * site + 1.02f * (k % 2), 0.505f + 1.005f * ((k / 2) % 2), 1.02f * (k / 4)};
            def.sleeping_disabled = true;
            def.material->id = (edyn::material::id_type)(1 + k % 2);
            if (site == 1) { def.material->stiffness = 3000.0f; def.material->damping = 30.0f; }   // a soft pile
            if (site == 2) def.material->spin_friction = 0.03f;
            bodies.push_back(edyn::make_rigidbody(registry, def));
        }
    // a sphere rolling from the second pile into the third - across the cut two shards make between them -, a capsule on its side beside it
    auto ball = edyn::rigidbody_def{};
    ball.mass = 1; ball.shape = edyn::sphere_shape{0.5f}; ball.position = {10.2f, 0.5f, 0.5f}; ball.linvel = {4.0f, 0, 0}; ball.sleeping_disabled = true;
    ball.material->roll_friction = 0.02f; ball.material->spin_friction = 0.1f; ball.material->id = 2;
    roller = edyn::make_rigidbody(registry, ball);
    bodies.push_back(roller);
    auto pill = edyn::rigidbody_def{};
    pill.mass = 1; pill.shape = edyn::capsule_shape{0.3f, 0.3f, edyn::coordinate_axis::z}; pill.position = {10.2f, 0.3f, 2.4f}; pill.linvel = {4.0f, 0, 0}; pill.sleeping_disabled = true;
    pill.material->roll_friction = 0.015f; pill.material->id = 1;
    bodies.push_back(edyn::make_rigidbody(registry, pill));
    edyn::material_base m01; m01.friction = 0.4f; m01.roll_friction = 0.05f;
    edyn::material_base m10; m10.friction = 0.45f; m10.spin_friction = 0.02f;
    edyn::material_base m12; m12.friction = 0.3f; m12.restitution = 0.25f;
    edyn::insert_material_mixing(registry, 0, 1, m01);
    edyn::insert_material_mixing(registry, 1, 0, m10);   // both orders
    edyn::insert_material_mixing(registry, 1, 2, m12);   // one order only
}

// every contact point of the registry as (normal impulse, friction impulses, pivots, normal), sorted: the entities' order is the host's
static std::vector<std::array<float, 12>> points(entt::registry &registry) {
    std::vector<std::array<float, 12>> out;
    registry.view<edyn::contact_point>().each([&](auto e, edyn::contact_point &p) {
        const auto &i = registry.get<edyn::contact_point_impulse>(e);
        out.push_back(std::array<float, 12>{(float)i.normal_impulse, (float)i.friction_impulse[0], (float)i.friction_impulse[1], (float)p.pivotA.x, (float)p.pivotA.y, (float)p.pivotA.z,
                                            (float)p.pivotB.x, (float)p.pivotB.y, (float)p.pivotB.z, (float)p.normal.x, (float)p.normal.y, (float)p.normal.z});
    });
    std::sort(out.begin(), out.end());
    return out;
}

// the device's manifold records (friction and restitution per point) and point extras of either registry, as bytes
static bool device_contacts(entt::registry &registry, std::vector<edynhip_manifold> &recs, std::vector<float> &extras) {
    auto &s = registry.ctx().get<edyn::detail::gpu_stepper>();
    uint32_t n = 0, m = 0;
    if (s.world ? edynhip_world_get_manifolds(s.world, nullptr, 0, &n) : edynhip_num_manifolds(s.ctx, &n)) return false;
    recs.assign(n, edynhip_manifold{}); extras.assign((size_t)28 * n, 0.0f);
    if (n == 0) return true;
    if (s.world ? edynhip_world_get_manifolds(s.world, recs.data(), n, &n) : edynhip_get_manifolds(s.ctx, recs.data(), n, &n)) return false;
    if (s.world ? edynhip_world_get_point_extras(s.world, extras.data(), n, &m) : edynhip_get_point_extras(s.ctx, extras.data(), n, &m)) return false;
    return m == n;
}

int main() {
    entt::registry one, many;
    auto cfg = edyn::init_config{};
    cfg.num_solver_velocity_iterations = 10;
    cfg.materialize_contacts = true;
    cfg.contact_point_data = true;
    edyn::attach(one, cfg);
    cfg.devices = {0, 0};
    edyn::attach(many, cfg);
    std::vector<entt::entity> b1, b2;
    entt::entity r1, r2;
    build(one, b1, r1); build(many, b2, r2);
    double t = 0;
    size_t most_points = 0;
    int changed_roll = 0, changed_spin = 0, soft = 0, rolling = 0, bouncy = 0, tabled = 0;
    for (int step = 0; step < 150; ++step) {
        t += 1.0 / 60;
        edyn::update(one, t); edyn::update(many, t);
        for (size_t k = 0; k < b1.size(); ++k) {
            const auto &p = one.get<edyn::position>(b1[k]), &q = many.get<edyn::position>(b2[k]);
            const auto &o = one.get<edyn::orientation>(b1[k]), &u = many.get<edyn::orientation>(b2[k]);
            const auto &v = one.get<edyn::linvel>(b1[k]), &w = many.get<edyn::linvel>(b2[k]);
            const auto &a = one.get<edyn::angvel>(b1[k]), &c = many.get<edyn::angvel>(b2[k]);
            const bool same = p.x == q.x && p.y == q.y && p.z == q.z && o.x == u.x && o.y == u.y && o.z == u.z && o.w == u.w && v.x == w.x && v.y == w.y && v.z == w.z &&
                              a.x == c.x && a.y == c.y && a.z == c.z;
            if (!same) {
                std::printf("FAILED: body %zu differs at step %d (%.9g %.9g %.9g vs %.9g %.9g %.9g)\n", k, step, p.x, p.y, p.z, q.x, q.y, q.z);
                return 1;
            }
        }
        const auto c1 = points(one), c2 = points(many);
        if (c1 != c2) { std::printf("FAILED: the contact points differ at step %d (%zu vs %zu)\n", step, c1.size(), c2.size()); return 1; }
        most_points = std::max(most_points, c1.size());
        if (step % 10 == 9 || step == 149) {   // friction, restitution, every other field of the records and the points' extras
            std::vector<edynhip_manifold> m1, m2;
            std::vector<float> x1, x2;
            REQUIRE(device_contacts(one, m1, x1) && device_contacts(many, m2, x2));
            REQUIRE(m1.size() == m2.size() && !m1.empty());
            if (std::memcmp(m1.data(), m2.data(), m1.size() * sizeof(edynhip_manifold)) != 0) { std::printf("FAILED: the manifold records differ at step %d\n", step); return 1; }
            if (std::memcmp(x1.data(), x2.data(), x1.size() * sizeof(float)) != 0) { std::printf("FAILED: the point extras differ at step %d\n", step); return 1; }
            if (step == 149) {
                for (size_t k = 0; k < m1.size(); ++k)
                    for (uint32_t q = 0; q < m1[k].num_points; ++q) {
                        const float *x = &x1[28 * k + 7 * q];
                        changed_roll += x[3] == 0.33f; changed_spin += x[4] == 0.21f; soft += x[5] < 1e17f; rolling += x[0] != 0 || x[1] != 0 || x[2] != 0;
                        bouncy += m1[k].pt[q].restitution == 0.25f; tabled += m1[k].pt[q].friction == 0.45f || m1[k].pt[q].friction == 0.3f;
                    }
            }
        }
        if (step == 60) {   // the table changes while the worlds run: in place on both
            edyn::material_base m02; m02.friction = 0.6f; m02.spin_friction = 0.1f; m02.roll_friction = 0.07f; m02.stiffness = 3000.0f; m02.damping = 30.0f;
            edyn::insert_material_mixing(one, 0, 2, m02); edyn::insert_material_mixing(many, 0, 2, m02);
        }
        if (step == 80)     // a body made while the worlds run, with a material of its own: dropped onto a top box of the third pile
            for (auto *reg : {&one, &many}) {
                auto def = edyn::rigidbody_def{};
                def.mass = 1; def.shape = edyn::sphere_shape{0.4f}; def.position = {14.05f, 3.2f, 0.05f}; def.sleeping_disabled = true;
                def.material->roll_friction = 0.1f; def.material->spin_friction = 0.2f; def.material->id = 2;
                (reg == &one ? b1 : b2).push_back(edyn::make_rigidbody(*reg, def));
            }
        if (step == 90)     // materials changed while the worlds run: the falling sphere before it lands, a box it lands on - in place on both
            for (auto *reg : {&one, &many}) {
                auto &b = reg == &one ? b1 : b2;
                auto &ms = reg->get<edyn::material>(b.back());
                ms.roll_friction = 0.33f; ms.spin_friction = 0.01f; ms.id = edyn::material::UnassignedID;
                edyn::refresh<edyn::material>(*reg, b.back());
                auto &mb = reg->get<edyn::material>(b[16 + 2]);    // a top box of the third pile
                mb.spin_friction = 0.21f; mb.id = edyn::material::UnassignedID;
                edyn::refresh<edyn::material>(*reg, b[16 + 2]);
            }
    }
    {   // the two-shard world did re-partition, with the points' extras carried, and was never rebuilt from the registry
        auto &s = many.ctx().get<edyn::detail::gpu_stepper>();
        edynhip_world_stats st{};
        REQUIRE(s.world && edynhip_world_get_stats(s.world, &st) == EDYNHIP_OK);
        REQUIRE(st.repartitions >= 1 && st.extras_carries >= 1 && st.steps >= 140);
    }
    REQUIRE(changed_roll > 0 && changed_spin > 0);                         // points made after the change mix the new materials
    REQUIRE(soft > 0 && rolling > 0 && bouncy > 0 && tabled > 0);          // ... beside soft, rolling and table-mixed ones
    REQUIRE(one.get<edyn::position>(r1).x > 12.0f);                        // the ball did reach the third pile
    REQUIRE(one.get<edyn::position>(b1.back()).y < 2.7f);                  // the late sphere did land
    REQUIRE(most_points > 40);
    std::printf("MULTI_MATERIALS_OK\n");
    return 0;
}
