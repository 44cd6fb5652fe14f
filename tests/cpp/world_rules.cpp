// The host rules of the multi-device world (edyn_amd/csrc/world_rules.hpp) on a machine without a GPU: plain g++, no library.
// Every expected value below is written from the rule's statement, none by running the rule.
#include "../../edyn_amd/csrc/world_rules.hpp"
#include <cstdio>
#include <limits>

using namespace eh;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

constexpr int32_t DYN = EDYNHIP_KIND_DYNAMIC, KIN = EDYNHIP_KIND_KINEMATIC, STA = EDYNHIP_KIND_STATIC;
template <typename T> static bool same(const std::vector<T> &a, std::initializer_list<T> b) { return a == std::vector<T>(b); }
static bool near(float a, double b) { return std::fabs((double)a - b) <= 1e-6 * std::max(1.0, std::fabs(b)); }

static void sticky() {   // W = 3
    //                                  group 0: 2 on shard 0, 3 on shard 1 | group 5: 2 / 2 on shards 1, 2 | group 9: one shard | not dynamic
    const std::vector<int32_t> kind = {DYN, DYN, DYN, DYN, DYN, DYN, DYN, DYN, DYN, DYN, DYN, STA, KIN};
    const std::vector<uint32_t> welded = {0, 0, 0, 0, 0, 5, 5, 5, 5, 9, 9, 11, 12};
    const std::vector<int32_t> rank = {0, 1, 0, 1, 1, 2, 1, 2, 1, 2, 2, -1, -1};
    const std::vector<int32_t> next = sticky_targets(13, welded.data(), kind.data(), rank.data(), 3);
    CHECK(same(next, {1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, -1, -1}));
    // the members of a group need not be neighbours in index
    const std::vector<uint32_t> welded2 = {0, 1, 0, 1, 0, 1};
    const std::vector<int32_t> kind2(6, DYN), rank2 = {0, 2, 0, 2, 1, 2};
    CHECK(same(sticky_targets(6, welded2.data(), kind2.data(), rank2.data(), 3), {0, 2, 0, 2, 0, 2}));
}

static std::vector<int32_t> split(uint32_t on0, uint32_t on1, uint32_t replicated) {
    std::vector<int32_t> r(on0, 0);
    r.insert(r.end(), on1, 1);
    r.insert(r.end(), replicated, -1);
    return r;
}
static void rebalance() {   // W = 2: more than 1.5 x the mean on the heaviest shard, of at least 8 bodies per shard
    CHECK(!needs_rebalance(16, split(12, 4, 0).data(), 2));   // 12 * 2 = 24 is not greater than 1.5 * 16 = 24
    CHECK(needs_rebalance(16, split(13, 3, 0).data(), 2));
    CHECK(needs_rebalance(21, split(13, 3, 5).data(), 2));    // replicated bodies are nobody's load
    CHECK(!needs_rebalance(15, split(15, 0, 0).data(), 2));   // below 8 * W
    CHECK(!needs_rebalance(15, split(14, 1, 0).data(), 2));
    CHECK(!needs_rebalance(100, split(100, 0, 0).data(), 1));
}

static void placement() {   // W = 3
    std::vector<uint32_t> load = {2, 2, 5}, extra = {0, 0, 0};
    const std::vector<int32_t> kind = {DYN, DYN, STA, DYN};
    const std::vector<uint32_t> group = {0, 1, 2, 1};   // body 3 touches body 1
    const std::vector<int32_t> place = place_new_bodies(4, kind.data(), group.data(), load, extra);
    // 0: a 2 / 2 tie goes to shard 0; 1: shard 1 is the lightest then; 2: replicated, a slot on every shard; 3: with its root on shard 1
    // although shard 0 carries as little
    CHECK(same(place, {0, 1, -1, 1}));
    CHECK(same(load, {3u, 4u, 5u}));
    CHECK(same(extra, {2u, 3u, 1u}));
}

static void ownership() {
    CHECK(joint_home(owner_rank(DYN, 1), owner_rank(DYN, 1)) == 1);
    CHECK(joint_home(owner_rank(DYN, 0), owner_rank(DYN, 2)) == -2);
    CHECK(joint_home(owner_rank(DYN, 2), owner_rank(STA, -1)) == 2);
    CHECK(joint_home(owner_rank(STA, -1), owner_rank(DYN, 2)) == 2);
    CHECK(joint_home(owner_rank(STA, -1), owner_rank(STA, -1)) == -1);
    CHECK(joint_home(owner_rank(KIN, 1), owner_rank(DYN, 0)) == 0);   // a kinematic body counts as not dynamic, whatever rank it is given
    CHECK(joint_home(owner_rank(KIN, 1), owner_rank(KIN, 1)) == -1);
    // who reports a body: its owner; shard 0 the replicated ones
    CHECK(shard_reports_body(1, 1) && !shard_reports_body(1, 0) && !shard_reports_body(1, 2));
    CHECK(shard_reports_body(-1, 0) && !shard_reports_body(-1, 1) && !shard_reports_body(-1, 2));
    CHECK(shard_reports_body(0, 0));
    // who holds a body: its owner; every shard a replicated one
    CHECK(shard_holds_body(1, 1) && !shard_holds_body(1, 0) && shard_holds_body(-1, 0) && shard_holds_body(-1, 2));
    // an exclusion pair: the shard that holds both bodies and owns one
    for (uint32_t r = 0; r < 3; ++r) {
        CHECK(shard_holds_exclusion(1, 1, r) == (r == 1));
        CHECK(shard_holds_exclusion(1, -1, r) == (r == 1));
        CHECK(shard_holds_exclusion(-1, 0, r) == (r == 0));
        CHECK(!shard_holds_exclusion(1, 2, r));     // on two shards: the scene's until the bodies meet
        CHECK(!shard_holds_exclusion(-1, -1, r));   // two replicated bodies never collide
    }
}

static void radius() {
    std::vector<float> cube;
    for (int k = 0; k < 8; ++k) { cube.push_back(k & 1 ? 1.f : -1.f); cube.push_back(k & 2 ? 1.f : -1.f); cube.push_back(k & 4 ? 1.f : -1.f); }
    MeshRadii meshes;
    meshes.add(cube.data(), 8);
    const float box[4] = {1, 2, 2, 0}, sphere[4] = {0.7f, 0, 0, 0}, capsule[4] = {0.25f, 0.5f, 0, 0}, cylinder[4] = {3, 4, 0, 0}, mesh0[4] = {0, 0, 0, 0}, mesh7[4] = {7, 0, 0, 0};
    const float com[3] = {0, 3, 4};
    CHECK(near(bounding_radius(meshes, EDYNHIP_SHAPE_BOX, box, nullptr), 3.0));
    CHECK(near(bounding_radius(meshes, EDYNHIP_SHAPE_SPHERE, sphere, nullptr), 0.7));
    CHECK(near(bounding_radius(meshes, EDYNHIP_SHAPE_CAPSULE, capsule, nullptr), 0.75));
    CHECK(near(bounding_radius(meshes, EDYNHIP_SHAPE_CYLINDER, cylinder, nullptr), 5.0));
    CHECK(near(bounding_radius(meshes, EDYNHIP_SHAPE_POLYHEDRON, mesh0, nullptr), 2.0 * std::sqrt(3.0)));
    CHECK(bounding_radius(meshes, EDYNHIP_SHAPE_POLYHEDRON, mesh7, nullptr) == 0.0f);
    CHECK(bounding_radius(meshes, EDYNHIP_SHAPE_NONE, box, nullptr) < 0);
    CHECK(bounding_radius(meshes, EDYNHIP_SHAPE_NONE, box, com) < 0);
    CHECK(near(bounding_radius(meshes, EDYNHIP_SHAPE_SPHERE, sphere, com), 5.7));
    CHECK(near(bounding_radius(meshes, EDYNHIP_SHAPE_POLYHEDRON, mesh0, com), 2.0 * std::sqrt(3.0) + 5.0));
    // a mesh's radius is computed once per call site's MeshRadii: the vertices are not read again
    for (float &x : cube) x *= 10.f;
    CHECK(near(bounding_radius(meshes, EDYNHIP_SHAPE_POLYHEDRON, mesh0, nullptr), 2.0 * std::sqrt(3.0)));
}

static void estimate() {
    //  0, 1, 2: spheres of radius 0.5 at x = 0, 1.02, 3 - the gap 0.02 is below 2 x 0.026, the gap 0.98 is not
    //  3, 4: far apart, a live joint | 5: static, jointed to 6 and to 7 | 8, 9: a removed joint | 10: dynamic without a shape, inside body 0
    const uint32_t n = 11;
    const float xs[n] = {0, 1.02f, 3, 100, 200, 300, 400, 500, 600, 700, 0};
    std::vector<int32_t> kind(n, DYN), shape(n, EDYNHIP_SHAPE_SPHERE);
    kind[5] = STA; shape[10] = EDYNHIP_SHAPE_NONE;
    std::vector<float> param(4 * n, 0.f), pos(3 * n, 0.f);
    for (uint32_t i = 0; i < n; ++i) { param[4 * i] = 0.5f; pos[3 * i] = xs[i]; }
    const uint32_t jbody[] = {3, 4, 5, 6, 7, 5, 8, 9};
    const uint8_t jalive[] = {1, 1, 1, 0};
    MeshRadii none;
    std::vector<uint32_t> labels(n, 99);
    std::vector<float> aabb(6 * n, 7.f);
    estimate_islands({n, kind.data(), shape.data(), param.data(), pos.data(), nullptr}, none, 4, jbody, jalive, labels.data(), aabb.data());
    CHECK(same(labels, {0u, 0u, 2u, 3u, 3u, 5u, 6u, 7u, 8u, 9u, 10u}));
    CHECK(aabb[0] == -0.5f && aabb[3] == 0.5f && aabb[1] == -0.5f && aabb[5] == 0.5f);
    CHECK(near(aabb[6 * 2], 2.5) && near(aabb[6 * 2 + 3], 3.5));
    for (int d = 0; d < 6; ++d) CHECK(aabb[6 * 5 + d] == 0.f && aabb[6 * 10 + d] == 0.f);   // no box of their own
    // with every joint alive (no flags), 8 and 9 are one island
    estimate_islands({n, kind.data(), shape.data(), param.data(), pos.data(), nullptr}, none, 4, jbody, nullptr, labels.data(), nullptr);
    CHECK(same(labels, {0u, 0u, 2u, 3u, 3u, 5u, 6u, 7u, 8u, 8u, 10u}));
    // the offset of the centre of mass widens the sphere: 2 reaches 1 with |com| = 0.5 on both (gap 0.98 - 2 x 0.5 < 0.052)
    std::vector<float> com(3 * n, 0.f);
    com[3 * 1 + 1] = 0.5f; com[3 * 2 + 2] = 0.5f;
    estimate_islands({n, kind.data(), shape.data(), param.data(), pos.data(), com.data()}, none, 0, nullptr, nullptr, labels.data(), nullptr);
    CHECK(labels[0] == 0 && labels[1] == 0 && labels[2] == 0 && labels[3] == 3 && labels[4] == 4);
}

static void welding() {
    // islands {0, 1}, {2}, {3}, {4}; boxes: 0-1 around x = 0, 2 at x = 1.03 (within 2 x 0.026 of island 0), 3 and 4 far; an edge ties 3 to 4
    const uint32_t n = 6;
    const std::vector<int32_t> kind = {DYN, DYN, DYN, DYN, DYN, STA}, shape(n, EDYNHIP_SHAPE_BOX);
    const std::vector<uint32_t> labels = {0, 0, 2, 3, 4, 5};
    std::vector<float> aabb(6 * n, 0.f);
    auto box = [&](uint32_t i, float x0, float x1) { aabb[6 * i] = x0; aabb[6 * i + 3] = x1; aabb[6 * i + 1] = aabb[6 * i + 2] = -0.5f; aabb[6 * i + 4] = aabb[6 * i + 5] = 0.5f; };
    box(0, -1, 0); box(1, 0, 1); box(2, 1.03f, 2); box(3, 50, 51); box(4, 90, 91); box(5, -1000, 1000);
    const uint32_t edge[] = {3, 4, 5, 0};   // the second names a static body: no tie
    std::vector<IslandBox> boxes;
    const std::vector<uint32_t> welded = weld_islands(n, labels.data(), kind.data(), shape.data(), aabb.data(), {{edge, 8, 2, nullptr}}, boxes);
    CHECK(same(welded, {0u, 0u, 0u, 3u, 3u, 5u}));
    CHECK(boxes.size() == 4 && boxes[0].label == 0 && boxes[0].lo[0] == -1.f && boxes[0].hi[0] == 1.f);   // the islands' boxes, before welding
    // no edges, island 2 a little further away: nothing welds
    box(2, 1.06f, 2);
    CHECK(same(weld_islands(n, labels.data(), kind.data(), shape.data(), aabb.data(), {}, boxes), {0u, 0u, 2u, 3u, 4u, 5u}));
    // the approach check's verdict: close within 2 x 0.026; otherwise the budget is what is left of the gap
    auto two = [](float gap) { std::vector<IslandBox> b(2); b[0] = {{0, 0, 0}, {1, 1, 1}, 0, 0}; b[1] = {{1 + gap, 0, 0}, {2 + gap, 1, 1}, 1, 1}; return b; };
    bool close = false; float budget = -1;
    std::vector<IslandBox> b = two(0.25f);
    approach_verdict(b, close, budget);
    CHECK(!close && near(budget, 0.25 - 0.052));
    b = two(0.05f); approach_verdict(b, close, budget);
    CHECK(close && budget == 0.f);
    b = two(5.f); approach_verdict(b, close, budget);
    CHECK(!close && near(budget, 1.0 - 0.052));   // beyond the horizon: not tracked, the horizon stands in
    b = two(0.25f); b[1].owner = 0; approach_verdict(b, close, budget);
    CHECK(!close && near(budget, 1.0 - 0.052));   // one owner: nothing to watch
}

static void spatial() {
    // 16 islands of 1 to 7 bodies on a 4 x 4 grid of sites 10 apart; label = the island's lowest index; one static body at the end
    std::vector<uint32_t> labels; std::vector<int32_t> kind; std::vector<float> aabb; std::vector<double> weights;
    for (uint32_t s = 0; s < 16; ++s) {
        const uint32_t first = (uint32_t)labels.size(), members = 1 + (s * 5) % 7;
        for (uint32_t k = 0; k < members; ++k) {
            labels.push_back(first); kind.push_back(DYN); weights.push_back(1.0 + (k % 3));
            const float c[3] = {10.f * (s % 4) + 0.5f * k, 0.f, 10.f * (s / 4)};
            for (int d = 0; d < 3; ++d) aabb.push_back(c[d] - 0.5f);
            for (int d = 0; d < 3; ++d) aabb.push_back(c[d] + 0.5f);
        }
    }
    labels.push_back((uint32_t)labels.size()); kind.push_back(STA); weights.push_back(1.0);
    for (int d = 0; d < 6; ++d) aabb.push_back(d < 3 ? -100.f : 100.f);
    const uint32_t n = (uint32_t)labels.size();
    auto check = [&](uint32_t W) {
        std::vector<int32_t> rank(n, 77), again(n, 78);
        partition_islands_spatial(n, labels.data(), kind.data(), weights.data(), aabb.data(), W, rank.data());
        partition_islands_spatial(n, labels.data(), kind.data(), weights.data(), aabb.data(), W, again.data());
        CHECK(rank == again);
        std::vector<double> load(W, 0.0), island(n, 0.0);
        double total = 0, heaviest = 0;
        for (uint32_t i = 0; i < n; ++i) {
            if (kind[i] != DYN) { CHECK(rank[i] == -1); continue; }
            CHECK(rank[i] >= 0 && rank[i] < (int32_t)W);
            if (rank[i] < 0 || rank[i] >= (int32_t)W) continue;
            CHECK(rank[i] == rank[labels[i]]);   // every island whole on one rank
            if (W == 1) CHECK(rank[i] == 0);
            load[rank[i]] += weights[i]; island[labels[i]] += weights[i]; total += weights[i];
        }
        for (double x : island) heaviest = std::max(heaviest, x);
        for (double x : load) CHECK(x <= total / W + heaviest + 1e-9);
    };
    for (uint32_t W : {1u, 2u, 3u, 4u, 8u}) check(W);
    // a body with a NaN box has no place of its own: it does not poison its island's centre, the bounds or anybody's rank
    aabb[6 * 20 + 1] = std::numeric_limits<float>::quiet_NaN();
    aabb[6 * 21 + 3] = std::numeric_limits<float>::infinity();
    for (uint32_t W : {1u, 3u, 4u}) check(W);
    // the longest-processing-time rule keeps the same promises
    std::vector<int32_t> rank(n, 77);
    partition_islands(n, labels.data(), kind.data(), weights.data(), 3, rank.data());
    for (uint32_t i = 0; i < n; ++i) CHECK(kind[i] == DYN ? rank[i] == rank[labels[i]] && rank[i] >= 0 && rank[i] < 3 : rank[i] == -1);
}

int main() {
    sticky(); rebalance(); placement(); ownership(); radius(); estimate(); welding(); spatial();
    if (failures) { std::printf("WORLD_RULES_FAILED %d\n", failures); return 1; }
    std::printf("WORLD_RULES_OK\n");
    return 0;
}
