// The host rules of the single-context C-ABI (edyn_amd/csrc/ctx_rules.hpp) on a machine without a GPU: plain g++, no library.
// Every expected value below is written from the rule's statement, none by running the rule.
#include "../../edyn_amd/csrc/ctx_rules.hpp"
#include <cstdio>
#include <initializer_list>

using namespace eh;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

template <typename T> static bool same(const std::vector<T> &a, std::initializer_list<T> b) { return a == std::vector<T>(b); }

static bool coloured(std::initializer_list<uint32_t> ends, std::initializer_list<uint8_t> dynamic, std::vector<uint32_t> &colour) {
    const std::vector<uint32_t> e(ends);
    return colour_joints((uint32_t)e.size() / 2, e.data(), std::vector<uint8_t>(dynamic), colour);
}

// Per round every dynamic body nominates its uncoloured joint of the lowest caller index; a joint that all of its dynamic ends
// nominated takes the lowest colour free at those ends.
static void colouring() {
    std::vector<uint32_t> c;
    // path 0 - 1 - 2 - 3: round 1 colours joint 0 (body 1 held joint 1 back, body 2 joint 2), round 2 joint 1 - colour 0 is taken at
    // body 1 -, round 3 joint 2, whose ends carry colour 1 (body 2) and nothing (body 3)
    CHECK(coloured({0, 1, 1, 2, 2, 3}, {1, 1, 1, 1}, c) && same(c, {0u, 1u, 0u}));
    // star on body 0: the centre nominates one joint per round, each finds one more colour taken there
    CHECK(coloured({0, 1, 0, 2, 0, 3}, {1, 1, 1, 1}, c) && same(c, {0u, 1u, 2u}));
    CHECK(coloured({1, 0, 0, 2, 3, 0}, {1, 1, 1, 1}, c) && same(c, {0u, 1u, 2u}));   // (which end the centre is makes no difference)
    // triangle: joints 0 = (0, 1), 1 = (1, 2), 2 = (0, 2) meet pairwise, so three colours, in caller order
    CHECK(coloured({0, 1, 1, 2, 0, 2}, {1, 1, 1}, c) && same(c, {0u, 1u, 2u}));
    // a static body constrains nothing: two joints that share only static body 0 are both coloured in the first round, with colour 0
    CHECK(coloured({0, 1, 0, 2}, {0, 1, 1}, c) && same(c, {0u, 0u}));
    // ... while the same two joints on a dynamic body 0 need two colours; a kinematic body counts as not dynamic (the flag says so)
    CHECK(coloured({0, 1, 0, 2}, {1, 1, 1}, c) && same(c, {0u, 1u}));
    // a joint between two bodies that are not dynamic has nobody to wait for
    CHECK(coloured({0, 1, 0, 1}, {0, 0}, c) && same(c, {0u, 0u}));
    CHECK(coloured({}, {1, 1}, c) && c.empty());
}

static void colour_order() {
    // stable in caller order inside a colour; colour_start[k] = first position with colour >= k, the trailing entry [number of colours] = n
    const std::vector<uint32_t> colour = {1, 0, 1, 0, 2};
    std::vector<uint32_t> order;
    uint32_t start[kJointMaxColours + 1];
    for (uint32_t &s : start) s = 77;
    CHECK(colour_sorted_order(colour, order, start) == 3);
    CHECK(same(order, {1u, 3u, 0u, 2u, 4u}));
    CHECK(start[0] == 0 && start[1] == 2 && start[2] == 4 && start[3] == 5);
    CHECK(start[4] == 77);   // left alone beyond the trailing entry
    // a colour nobody has (possible only in hand-made input) is an empty range
    const std::vector<uint32_t> gap = {2, 0};
    CHECK(colour_sorted_order(gap, order, start) == 3 && same(order, {1u, 0u}));
    CHECK(start[0] == 0 && start[1] == 1 && start[2] == 1 && start[3] == 2);
    CHECK(colour_sorted_order({}, order, start) == 0 && order.empty() && start[0] == 0);
}

static void colour_overflow() {   // 64 colours: a dynamic body carries at most 64 joints
    for (uint32_t n : {64u, 65u}) {
        std::vector<uint32_t> ends, c;
        for (uint32_t e = 0; e < n; ++e) { ends.push_back(0); ends.push_back(1 + e); }
        std::vector<uint8_t> dynamic(n + 1, 0);
        dynamic[0] = 1;   // the leaves are static: only the centre counts
        const bool ok = colour_joints(n, ends.data(), dynamic, c);
        CHECK(ok == (n == 64));
        if (ok) for (uint32_t e = 0; e < n; ++e) CHECK(c[e] == e);
    }
    // on a static centre the same 65 joints all take colour 0
    std::vector<uint32_t> ends, c;
    for (uint32_t e = 0; e < 65; ++e) { ends.push_back(0); ends.push_back(1 + e); }
    std::vector<uint8_t> dynamic(66, 1);
    dynamic[0] = 0;
    CHECK(colour_joints(65, ends.data(), dynamic, c) && c == std::vector<uint32_t>(65, 0u));
}

static void rows() {
    CHECK(joint_row_count(EDYNHIP_JOINT_HINGE) == 5 && joint_row_count(EDYNHIP_JOINT_CONE) == 2 && joint_row_count(EDYNHIP_JOINT_CVJOINT) == 9);
    CHECK(joint_row_count(EDYNHIP_JOINT_GENERIC) == 24);
    for (int32_t t : {EDYNHIP_JOINT_POINT, EDYNHIP_JOINT_DISTANCE, EDYNHIP_JOINT_SOFT_DISTANCE, EDYNHIP_JOINT_GRAVITY, EDYNHIP_JOINT_NULL}) CHECK(joint_row_count(t) == 3);
}

static void exclusion_list() {
    const uint32_t N = kExclNone;
    std::vector<uint32_t> l(kExclCap, N);
    CHECK(kExclCap == 16);
    CHECK(!excl_listed(l.data(), 5));
    CHECK(excl_add(l.data(), 5) && excl_add(l.data(), 5));   // idempotent
    CHECK(l[0] == 5 && l[1] == N && excl_listed(l.data(), 5));
    excl_drop(l.data(), 5);
    CHECK(l == std::vector<uint32_t>(16, N));
    for (uint32_t k = 0; k < 16; ++k) CHECK(excl_add(l.data(), 100 + k));
    const std::vector<uint32_t> full = l;
    CHECK(!excl_add(l.data(), 999) && l == full);   // the 17th entry fails and leaves the list as it was
    CHECK(excl_add(l.data(), 107) && l == full);    // an entry that is there is no 17th
    CHECK(excl_listed(l.data(), 115) && !excl_listed(l.data(), 999));
    excl_drop(l.data(), 103);   // the last entry takes the hole
    CHECK(l[3] == 115 && l[15] == N && l[14] == 114 && l[2] == 102 && l[4] == 104);
    const std::vector<uint32_t> before = l;
    excl_drop(l.data(), 103);   // absent now: a no-op
    CHECK(l == before);
    excl_drop(l.data(), 114);   // the last entry itself
    CHECK(l[14] == N && l[13] == 113 && l[3] == 115);
    std::vector<uint32_t> four = {10, 11, 12, 13, N, N, N, N, N, N, N, N, N, N, N, N};
    excl_drop(four.data(), 11);
    CHECK(four[0] == 10 && four[1] == 13 && four[2] == 12 && four[3] == N);
}

static void should_collide() {
    // bodies 0..3; body 2's group is not in body 3's mask (one direction only); everything else collides by group
    const std::vector<uint64_t> group = {1, 1, 2, 1}, mask = {~0ull, ~0ull, ~0ull, 1};
    std::vector<uint32_t> none, excl(4 * kExclCap, kExclNone);
    CHECK(should_collide_default(0, 1, group, mask, none) == 1);
    CHECK(should_collide_default(1, 1, group, mask, none) == 0);   // same body
    CHECK(should_collide_default(2, 3, group, mask, none) == 0);   // a's group misses b's mask
    CHECK(should_collide_default(3, 2, group, mask, none) == 0);   // ... and the other way round
    CHECK(should_collide_default(0, 3, group, mask, none) == 1);
    CHECK(should_collide_default(0, 1, group, mask, excl) == 1);   // lists that name nobody
    excl_add(&excl[0 * kExclCap], 1);   // one way only: 0 lists 1
    CHECK(should_collide_default(0, 1, group, mask, excl) == 0 && should_collide_default(1, 0, group, mask, excl) == 0);
    excl_drop(&excl[0 * kExclCap], 1);
    excl_add(&excl[1 * kExclCap], 0);   // 1 lists 0
    CHECK(should_collide_default(0, 1, group, mask, excl) == 0 && should_collide_default(1, 0, group, mask, excl) == 0);
    CHECK(should_collide_default(0, 2, group, mask, excl) == 1);
    // bodies beyond the group arrays have every bit set
    const std::vector<uint64_t> g1 = {0}, m1 = {0};
    CHECK(should_collide_default(0, 1, g1, m1, none) == 1);
}

static void pair_keys() {
    CHECK(pair_owner(3, 7, true, true) == 7 && pair_owner(7, 3, true, true) == 7);   // both procedural: the higher index
    CHECK(pair_owner(3, 7, true, false) == 3 && pair_owner(3, 7, false, true) == 7);
    CHECK(canonical_pair_key(3, 7, true, true) == ((7ull << 32) | 3) && canonical_pair_key(7, 3, true, true) == ((7ull << 32) | 3));
    CHECK(canonical_pair_key(3, 7, true, false) == ((3ull << 32) | 7) && canonical_pair_key(7, 3, false, true) == ((3ull << 32) | 7));
    auto asc = [](std::initializer_list<uint64_t> k) { const std::vector<uint64_t> v(k); return strictly_ascending((uint32_t)v.size(), [&](uint32_t i) { return v[i]; }); };
    CHECK(asc({}) && asc({5}) && asc({1, 2, 3}));
    CHECK(!asc({1, 2, 2}));   // equal keys are rejected
    CHECK(!asc({2, 1}) && !asc({1, 3, 2}));
}

static void participants() {
    const int32_t DYN = EDYNHIP_KIND_DYNAMIC, KIN = EDYNHIP_KIND_KINEMATIC, STA = EDYNHIP_KIND_STATIC;
    uint32_t num_np = 99;
    // shapeless bodies take no part; static and kinematic ones first, then the dynamic ones, each in index order
    const std::vector<uint32_t> l = broadphase_participants({DYN, STA, DYN, KIN, STA, DYN}, {EDYNHIP_SHAPE_BOX, EDYNHIP_SHAPE_NONE, EDYNHIP_SHAPE_SPHERE, EDYNHIP_SHAPE_BOX, EDYNHIP_SHAPE_PLANE, EDYNHIP_SHAPE_NONE}, num_np);
    CHECK(same(l, {3u, 4u, 0u, 2u}) && num_np == 2);
    CHECK(broadphase_participants({}, {}, num_np).empty() && num_np == 0);
}

static void plane_space() {   // both branches, either side of |n.z| = sqrt(1/2): p, q, n orthonormal within 1e-6
    auto check = [](double x, double y, double z) {
        const double len = std::sqrt(x * x + y * y + z * z);
        const float n[3] = {(float)(x / len), (float)(y / len), (float)(z / len)};
        float p[3], q[3];
        plane_space_h(n, p, q);
        auto dot = [](const float *a, const float *b) { return (double)a[0] * b[0] + (double)a[1] * b[1] + (double)a[2] * b[2]; };
        const double tol = 1e-6;
        CHECK(std::fabs(dot(p, n)) <= tol && std::fabs(dot(q, n)) <= tol && std::fabs(dot(p, q)) <= tol);
        CHECK(std::fabs(dot(p, p) - 1.0) <= tol && std::fabs(dot(q, q) - 1.0) <= tol);
    };
    check(0, 0, 1); check(0, 0, -1); check(1, 0, 0); check(0, 1, 0);
    check(1, 2, 0.5); check(-0.3, 0.2, -2.0);
    for (double nz : {0.70, 0.7071, 0.7072, 0.715, -0.70, -0.715}) {   // sqrt(1/2) = 0.70710678...
        const double r = std::sqrt(1.0 - nz * nz);
        check(r * 0.6, r * 0.8, nz);
        check(-r, 0.0, nz);
    }
}

int main() {
    colouring();
    colour_order();
    colour_overflow();
    rows();
    exclusion_list();
    should_collide();
    pair_keys();
    participants();
    plane_space();
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("CTX_RULES_OK\n");
    return 0;
}
