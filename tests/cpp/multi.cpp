// The multi-GPU world of the C-ABI (include/edynhip.h "Multi-GPU world", edyn_amd/csrc/multi*.hip) next to ONE context stepping the
// same scene: six mini-piles (six islands) and a sphere that rolls from the first pile into the fourth - its island meets an
// island that lives on the other shard, which forces a re-partition with the contact manifolds carried along; later a forced
// re-partition. Positions, orientations and velocities must be bit-equal after every step. Two shards on one physical GPU
// (the reference's island parallelism: src/edyn/dynamics/solver.cpp:408-428).
#include <edynhip.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s (%s | %s)\n", __FILE__, __LINE__, #c, edynhip_world_last_error(world), one ? edynhip_last_error(one) : ""); return 1; } } while (0)

struct Scene {
    std::vector<int32_t> kind, shape;
    std::vector<float> pos, orn, lv, av, mass, param, fric, rest;
    std::vector<uint64_t> group, mask;
    std::vector<uint8_t> nosleep;
    std::vector<float> com;
    void add(int k, int s, float x, float y, float z, float p0, float p1, float p2, float p3, float vx = 0, float cx = 0, float cy = 0, float cz = 0) {
        com.insert(com.end(), {cx, cy, cz});
        kind.push_back(k); shape.push_back(s);
        pos.insert(pos.end(), {x, y, z}); orn.insert(orn.end(), {0, 0, 0, 1}); lv.insert(lv.end(), {vx, 0, 0}); av.insert(av.end(), {0, 0, 0});
        mass.push_back(1); param.insert(param.end(), {p0, p1, p2, p3}); fric.push_back(0.5f); rest.push_back(0);
        group.push_back(~0ull); mask.push_back(~0ull); nosleep.push_back(1);
    }
    edynhip_bodies view() const {
        edynhip_bodies b{};
        b.kind = kind.data(); b.pos = pos.data(); b.orn = orn.data(); b.linvel = lv.data(); b.angvel = av.data(); b.mass = mass.data();
        b.shape_type = shape.data(); b.shape_param = param.data(); b.friction = fric.data(); b.restitution = rest.data();
        b.group = group.data(); b.mask = mask.data(); b.sleeping_disabled = nosleep.data();
        b.center_of_mass = com.data();
        return b;
    }
    uint32_t n() const { return (uint32_t)kind.size(); }
};

// Joints are island edges the host knows: a re-partition BEFORE the first step (the shards' device labels are still the identity) must
// keep two far-apart bodies tied by a joint on one shard (they were split and the joint silently dropped), and the
// scene-description calls are refused once the world has stepped.
static int jointed_pairs() {
    edynhip_world *world = nullptr;
    edynhip_ctx *one = nullptr;
    Scene sc;
    sc.add(EDYNHIP_KIND_STATIC, EDYNHIP_SHAPE_PLANE, 0, 0, 0, 0, 1, 0, 0);
    for (int k = 0; k < 8; ++k) {   // eight pairs of spheres 3 m apart, each pair tied by a distance constraint, swinging sideways
        sc.add(EDYNHIP_KIND_DYNAMIC, EDYNHIP_SHAPE_SPHERE, 10.0f * k, 4.0f, 0, 0.4f, 0, 0, 0, 0.5f);
        sc.add(EDYNHIP_KIND_DYNAMIC, EDYNHIP_SHAPE_SPHERE, 10.0f * k + 3.0f, 4.0f, 0, 0.4f, 0, 0, 0, -0.5f);
    }
    const uint32_t n = sc.n(), nj = 8;
    std::vector<int32_t> jt(nj, EDYNHIP_JOINT_DISTANCE);
    std::vector<uint32_t> jb; std::vector<float> jp(6 * nj, 0.0f), ja(6 * nj, 0.0f), jq(10 * nj, 0.0f);
    for (uint32_t k = 0; k < nj; ++k) { jb.push_back(1 + 2 * k); jb.push_back(2 + 2 * k); jq[10 * k] = 3.0f; }
    edynhip_joints js{jt.data(), jb.data(), jp.data(), ja.data(), jq.data()};
    edynhip_config cfg{};
    cfg.device = 0; cfg.max_bodies = n + 16; cfg.max_joints = nj + 4; cfg.fixed_dt = 1.0f / 60; cfg.num_velocity_iterations = 10; cfg.num_position_iterations = 3;
    cfg.gravity[1] = -9.8f;
    int status = 0;
    one = edynhip_create(&cfg, &status);
    REQUIRE(one != nullptr);
    const edynhip_bodies b = sc.view();
    REQUIRE(edynhip_set_bodies(one, n, &b) == EDYNHIP_OK && edynhip_set_joints(one, nj, &js) == EDYNHIP_OK);
    const int32_t devices[2] = {0, 0};
    cfg.max_bodies = 0; cfg.max_joints = 0;
    world = edynhip_world_create(&cfg, devices, 2, &status);
    REQUIRE(world != nullptr);
    REQUIRE(edynhip_world_set_bodies(world, n, &b) == EDYNHIP_OK && edynhip_world_set_joints(world, nj, &js) == EDYNHIP_OK);
    REQUIRE(edynhip_world_repartition(world) == EDYNHIP_OK);   // before the first step: no device labels yet
    std::vector<int32_t> part(n);
    REQUIRE(edynhip_world_get_partition(world, part.data()) == EDYNHIP_OK);
    for (uint32_t k = 0; k < nj; ++k) REQUIRE(part[1 + 2 * k] == part[2 + 2 * k] && part[1 + 2 * k] >= 0);
    std::vector<float> p1(3 * n), p2(3 * n), v1(3 * n), v2(3 * n);
    for (int step = 0; step < 90; ++step) {
        REQUIRE(edynhip_step(one, 1) == EDYNHIP_OK && edynhip_world_step(world, 1) == EDYNHIP_OK);
        if (step == 30) REQUIRE(edynhip_world_repartition(world) == EDYNHIP_OK);   // and right after a step
        REQUIRE(edynhip_get_state(one, p1.data(), nullptr, v1.data(), nullptr) == EDYNHIP_OK);
        REQUIRE(edynhip_world_get_state(world, p2.data(), nullptr, v2.data(), nullptr) == EDYNHIP_OK);
        if (std::memcmp(p1.data(), p2.data(), p1.size() * 4) || std::memcmp(v1.data(), v2.data(), v1.size() * 4)) {
            std::printf("FAILED: jointed pairs: the sharded world left the single context's trajectory at step %d\n", step);
            return 1;
        }
    }
    const float d0 = p2[3] - p2[6], d1 = p2[4] - p2[7], d2 = p2[5] - p2[8];
    REQUIRE(std::fabs(std::sqrt(d0 * d0 + d1 * d1 + d2 * d2) - 3.0f) < 0.05f);   // the constraint is alive
    REQUIRE(edynhip_world_exclude_collision(world, 1, 2) == EDYNHIP_ERR_UNSUPPORTED);   // a stepped world is not silently reset
    REQUIRE(edynhip_world_set_joints(world, nj, &js) == EDYNHIP_ERR_UNSUPPORTED);
    edynhip_world_destroy(world);
    edynhip_destroy(one);
    return 0;
}

// settings.should_collide_func on a world over several devices (edynhip_world_set_pair_filter, VERDICT r04 missing #5): a predicate that
// lets every third pair of boxes pass through each other - asked with GLOBAL indices by whichever shard holds the pair - against ONE
// context with the same predicate; also set on a running world and taken away again.
static int g_asked = 0;
static edynhip_world *g_world = nullptr;
static int third_pairs_are_ghosts(void *user, uint32_t body, uint32_t other) {
    ++g_asked;
    if (body == 0 || other == 0) return 1;                          // the plane
    if ((body + other) % 3u == 0) return 0;
    return user ? edynhip_default_should_collide((edynhip_ctx *)user, body, other) : edynhip_world_default_should_collide(g_world, body, other);
}
static int filtered_piles() {
    edynhip_world *world = nullptr;
    edynhip_ctx *one = nullptr;
    Scene sc;
    sc.add(EDYNHIP_KIND_STATIC, EDYNHIP_SHAPE_PLANE, 0, 0, 0, 0, 1, 0, 0);
    for (int site = 0; site < 4; ++site)
        for (int k = 0; k < 27; ++k) {
            const int i = k % 3, j = (k / 3) % 3, l = k / 9;
            const float off = (j & 1) ? 0.5f : 0.0f;
            sc.add(EDYNHIP_KIND_DYNAMIC, EDYNHIP_SHAPE_BOX, 8.0f * site + 1.02f * i + off + 0.003f * k, 0.505f + 1.005f * j, 1.02f * l + off, 0.5f, 0.5f, 0.5f, 0);
        }
    const uint32_t n = sc.n();
    edynhip_config cfg{};
    cfg.device = 0; cfg.max_bodies = n + 16; cfg.fixed_dt = 1.0f / 60; cfg.num_velocity_iterations = 10; cfg.num_position_iterations = 3;
    cfg.gravity[1] = -9.8f;
    int status = 0;
    one = edynhip_create(&cfg, &status);
    REQUIRE(one != nullptr);
    const edynhip_bodies b = sc.view();
    REQUIRE(edynhip_set_bodies(one, n, &b) == EDYNHIP_OK);
    const int32_t devices[2] = {0, 0};
    cfg.max_bodies = 0;
    world = edynhip_world_create(&cfg, devices, 2, &status);
    REQUIRE(world != nullptr);
    g_world = world;
    REQUIRE(edynhip_world_set_bodies(world, n, &b) == EDYNHIP_OK);
    REQUIRE(edynhip_set_pair_filter(one, &third_pairs_are_ghosts, one) == EDYNHIP_OK);
    REQUIRE(edynhip_world_set_pair_filter(world, &third_pairs_are_ghosts, nullptr) == EDYNHIP_OK);   // before the shards exist
    std::vector<float> p1(3 * n), p2(3 * n), v1(3 * n), v2(3 * n);
    for (int step = 0; step < 120; ++step) {
        if (step == 60) {   // the default test again, on the running world and the running context
            REQUIRE(edynhip_set_pair_filter(one, nullptr, nullptr) == EDYNHIP_OK && edynhip_world_set_pair_filter(world, nullptr, nullptr) == EDYNHIP_OK);
        }
        if (step == 90) {   // ... and the predicate back
            REQUIRE(edynhip_set_pair_filter(one, &third_pairs_are_ghosts, one) == EDYNHIP_OK && edynhip_world_set_pair_filter(world, &third_pairs_are_ghosts, nullptr) == EDYNHIP_OK);
        }
        if (step == 40) REQUIRE(edynhip_world_repartition(world) == EDYNHIP_OK);   // rebuilt shards ask the same predicate
        REQUIRE(edynhip_step(one, 1) == EDYNHIP_OK && edynhip_world_step(world, 1) == EDYNHIP_OK);
        REQUIRE(edynhip_get_state(one, p1.data(), nullptr, v1.data(), nullptr) == EDYNHIP_OK);
        REQUIRE(edynhip_world_get_state(world, p2.data(), nullptr, v2.data(), nullptr) == EDYNHIP_OK);
        if (std::memcmp(p1.data(), p2.data(), p1.size() * 4) || std::memcmp(v1.data(), v2.data(), v1.size() * 4)) {
            std::printf("FAILED: filtered piles: the sharded world left the single context's trajectory at step %d\n", step);
            return 1;
        }
    }
    REQUIRE(g_asked > 200);
    uint32_t m1 = 0, m2 = 0;
    REQUIRE(edynhip_num_manifolds(one, &m1) == EDYNHIP_OK && edynhip_world_get_manifolds(world, nullptr, 0, &m2) == EDYNHIP_OK && m1 == m2);
    edynhip_world_destroy(world);
    edynhip_destroy(one);
    g_world = nullptr;
    return 0;
}

// Island sleeping on a world over several devices: a re-partition rebuilds every shard, and the islands' sleep timers
// (island::sleep_timestamp) travel with them (edynhip_get / set_sleep_timers) - four piles settle and fall asleep at the same steps as in ONE
// context although the shards are rebuilt four times on the way (each rebuild used to start every timer again: nothing fell asleep while
// re-partitions came more often than island_time_to_sleep).
static int sleeping_piles() {
    edynhip_world *world = nullptr;
    edynhip_ctx *one = nullptr;
    Scene sc;
    sc.add(EDYNHIP_KIND_STATIC, EDYNHIP_SHAPE_PLANE, 0, 0, 0, 0, 1, 0, 0);
    for (int site = 0; site < 4; ++site)
        for (int k = 0; k < 27; ++k) {
            const int i = k % 3, j = (k / 3) % 3, l = k / 9;
            const float off = (j & 1) ? 0.5f : 0.0f;
            sc.add(EDYNHIP_KIND_DYNAMIC, EDYNHIP_SHAPE_BOX, 8.0f * site + 1.02f * i + off + 0.003f * k, 0.505f + 1.005f * j, 1.02f * l + off, 0.5f, 0.5f, 0.5f, 0);
        }
    std::fill(sc.nosleep.begin(), sc.nosleep.end(), (uint8_t)0);
    const uint32_t n = sc.n();
    edynhip_config cfg{};
    cfg.device = 0; cfg.max_bodies = n + 16; cfg.fixed_dt = 1.0f / 60; cfg.num_velocity_iterations = 10; cfg.num_position_iterations = 3;
    cfg.gravity[1] = -9.8f; cfg.flags = EDYNHIP_FLAG_SLEEPING;
    int status = 0;
    one = edynhip_create(&cfg, &status);
    REQUIRE(one != nullptr);
    const edynhip_bodies b = sc.view();
    REQUIRE(edynhip_set_bodies(one, n, &b) == EDYNHIP_OK);
    const int32_t devices[2] = {0, 0};
    cfg.max_bodies = 0;
    world = edynhip_world_create(&cfg, devices, 2, &status);
    REQUIRE(world != nullptr);
    REQUIRE(edynhip_world_set_bodies(world, n, &b) == EDYNHIP_OK);
    std::vector<float> p1(3 * n), p2(3 * n), v1(3 * n), v2(3 * n), w1(3 * n), w2(3 * n);
    std::vector<uint8_t> asleep(n);
    int first_sleep = -1, all_asleep = -1;
    for (int step = 0; step < 480; ++step) {
        if (step == 100 || step == 180 || step == 250 || step == 330) REQUIRE(edynhip_world_repartition(world) == EDYNHIP_OK);
        REQUIRE(edynhip_step(one, 1) == EDYNHIP_OK && edynhip_world_step(world, 1) == EDYNHIP_OK);
        REQUIRE(edynhip_get_state(one, p1.data(), nullptr, v1.data(), w1.data()) == EDYNHIP_OK);
        REQUIRE(edynhip_world_get_state(world, p2.data(), nullptr, v2.data(), w2.data()) == EDYNHIP_OK);
        if (std::memcmp(p1.data(), p2.data(), p1.size() * 4) || std::memcmp(v1.data(), v2.data(), v1.size() * 4) || std::memcmp(w1.data(), w2.data(), w1.size() * 4)) {
            std::printf("FAILED: sleeping piles: the sharded world left the single context's trajectory at step %d (first sleep in the single context at step %d)\n", step, first_sleep);
            return 1;
        }
        REQUIRE(edynhip_get_asleep(one, asleep.data()) == EDYNHIP_OK);
        uint32_t count = 0;
        for (uint32_t i = 1; i < n; ++i) count += asleep[i];
        if (count && first_sleep < 0) first_sleep = step;
        if (count == n - 1 && all_asleep < 0) all_asleep = step;
    }
    REQUIRE(first_sleep > 130 && all_asleep > 0);   // the piles did fall asleep - later than one island_time_to_sleep (120 steps) after the start
    std::printf("sleeping piles: first island asleep at step %d, all asleep at step %d, four re-partitions on the way\n", first_sleep, all_asleep);
    edynhip_world_destroy(world);
    edynhip_destroy(one);
    return 0;
}

int main() {
    if (jointed_pairs() != 0) return 1;
    if (filtered_piles() != 0) return 1;
    if (sleeping_piles() != 0) return 1;
    edynhip_world *world = nullptr;
    edynhip_ctx *one = nullptr;
    Scene sc;
    sc.add(EDYNHIP_KIND_STATIC, EDYNHIP_SHAPE_PLANE, 0, 0, 0, 0, 1, 0, 0);
    for (int site = 0; site < 6; ++site)                 // 3 x 2 sites, 8 m apart, a brick-offset 3 x 3 x 3 pile on each
        for (int k = 0; k < 27; ++k) {
            const int i = k % 3, j = (k / 3) % 3, l = k / 9;
            const float off = (j & 1) ? 0.5f : 0.0f;
            // every fifth box carries a centre-of-mass offset (rigidbody_def::center_of_mass): a re-partition hands the CENTRE-OF-MASS state
            // back to freshly built shards, whose origins / AABBs must follow it (they were displaced by R com)
            const bool offset = k % 5 == 2;
            sc.add(EDYNHIP_KIND_DYNAMIC, EDYNHIP_SHAPE_BOX, 8.0f * (site % 3) + 1.02f * i + off + 0.003f * k, 0.505f + 1.005f * j, 8.0f * (site / 3) + 1.02f * l + off, 0.5f, 0.5f, 0.5f, 0,
                   0, offset ? 0.12f : 0.0f, offset ? -0.08f : 0.0f, offset ? 0.05f : 0.0f);
        }
    // between site 0 and site 3, rolling towards +z: the world places islands along a space-filling curve (neighbours mostly share a shard);
    // with two shards the cut runs between the z = 0 row and the z = 8 row of sites, so this sphere's island has to change shards
    sc.add(EDYNHIP_KIND_DYNAMIC, EDYNHIP_SHAPE_SPHERE, 1.0f, 0.5f, 4.3f, 0.5f, 0, 0, 0, 0.0f);
    sc.lv[sc.lv.size() - 1] = 4.0f;
    const uint32_t n = sc.n();

    edynhip_config cfg{};
    cfg.device = 0; cfg.max_bodies = n + 16; cfg.fixed_dt = 1.0f / 60; cfg.num_velocity_iterations = 10; cfg.num_position_iterations = 3;
    cfg.gravity[1] = -9.8f;
    int status = 0;
    one = edynhip_create(&cfg, &status);
    REQUIRE(one != nullptr);
    const edynhip_bodies b = sc.view();
    REQUIRE(edynhip_set_bodies(one, n, &b) == EDYNHIP_OK);

    const int32_t devices[2] = {0, 0};
    cfg.max_bodies = 0;
    world = edynhip_world_create(&cfg, devices, 2, &status);
    REQUIRE(world != nullptr);
    REQUIRE(edynhip_world_set_bodies(world, n, &b) == EDYNHIP_OK);

    std::vector<int32_t> part(n), part2(n);
    REQUIRE(edynhip_world_get_partition(world, part.data()) == EDYNHIP_OK);
    int on[2] = {0, 0};
    for (uint32_t i = 1; i < n; ++i) { REQUIRE(part[i] == 0 || part[i] == 1); ++on[part[i]]; }
    REQUIRE(part[0] == -1 && on[0] > 27 && on[1] > 27);
    for (int site = 0; site < 6; ++site)                 // an island is never split
        for (int k = 1; k < 27; ++k) REQUIRE(part[1 + 27 * site + k] == part[1 + 27 * site]);

    std::vector<float> p1(3 * n), q1(4 * n), v1(3 * n), w1(3 * n), p2(3 * n), q2(4 * n), v2(3 * n), w2(3 * n);
    for (int step = 0; step < 120; ++step) {
        REQUIRE(edynhip_step(one, 1) == EDYNHIP_OK);
        REQUIRE(edynhip_world_step(world, 1) == EDYNHIP_OK);
        REQUIRE(edynhip_get_state(one, p1.data(), q1.data(), v1.data(), w1.data()) == EDYNHIP_OK);
        REQUIRE(edynhip_world_get_state(world, p2.data(), q2.data(), v2.data(), w2.data()) == EDYNHIP_OK);
        if (std::memcmp(p1.data(), p2.data(), p1.size() * 4) || std::memcmp(q1.data(), q2.data(), q1.size() * 4) ||
            std::memcmp(v1.data(), v2.data(), v1.size() * 4) || std::memcmp(w1.data(), w2.data(), w1.size() * 4)) {
            std::printf("FAILED: the sharded world left the single context's trajectory at step %d\n", step);
            return 1;
        }
        if (step == 80) REQUIRE(edynhip_world_repartition(world) == EDYNHIP_OK);   // forced: every shard rebuilt mid-run
    }
    edynhip_world_stats st{};
    REQUIRE(edynhip_world_get_stats(world, &st) == EDYNHIP_OK);
    REQUIRE(st.repartitions >= 2);                       // the sphere's approach + the forced one
    REQUIRE(st.approach_checks < st.steps);              // the growth budget spares most steps the box sweep
    REQUIRE(st.bodies_per_shard[0] + st.bodies_per_shard[1] == n);
    REQUIRE(edynhip_world_get_partition(world, part2.data()) == EDYNHIP_OK);
    REQUIRE(part[1] != part[1 + 27 * 3]);                // (site 0 and site 3 started on different shards)
    REQUIRE(part2[n - 1] == part2[1 + 27 * 3]);          // the sphere now lives with the pile it ran into
    uint32_t m1 = 0, m2 = 0;
    REQUIRE(edynhip_num_manifolds(one, &m1) == EDYNHIP_OK);
    REQUIRE(edynhip_world_get_manifolds(world, nullptr, 0, &m2) == EDYNHIP_OK && m1 == m2);
    std::vector<edynhip_manifold> a(m1), c(m2);
    REQUIRE(edynhip_get_manifolds(one, a.data(), m1, &m1) == EDYNHIP_OK && edynhip_world_get_manifolds(world, c.data(), m2, &m2) == EDYNHIP_OK);
    REQUIRE(std::memcmp(a.data(), c.data(), (size_t)m1 * sizeof(edynhip_manifold)) == 0);
    std::printf("MULTI_OK %u bodies, %u steps, %u approach checks, %u re-partitions, shards %u + %u bodies, %u manifolds identical\n", n, st.steps,
                st.approach_checks, st.repartitions, st.bodies_per_shard[0], st.bodies_per_shard[1], m1);
    edynhip_world_destroy(world);
    edynhip_destroy(one);
    return 0;
}
