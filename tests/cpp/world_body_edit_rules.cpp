// The host rules of edynhip_world_edit_bodies (edyn_amd/csrc/world_rules.hpp "body edits", with validate_body_edit of ctx_rules.hpp as
// the world calls it): which shards take an edit, when an edit crosses the replication boundary, which shard a body made dynamic goes
// to, when the approach check is due, what the scene writes out before a shape or a mass changes. Plain C++, its own main, no library.
#include "../../edyn_amd/csrc/world_rules.hpp"
#include "../../edyn_amd/csrc/ctx_rules.hpp"
#include <cstdio>
#include <cstring>
#include <string>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED: %s (line %d)\n", #cond, __LINE__); ++failures; } } while (0)

int main() {
    using namespace eh;
    const int32_t DYN = EDYNHIP_KIND_DYNAMIC, KIN = EDYNHIP_KIND_KINEMATIC, STA = EDYNHIP_KIND_STATIC;
    const uint32_t ALL = EDYNHIP_EDIT_MASS | EDYNHIP_EDIT_INERTIA | EDYNHIP_EDIT_MATERIAL | EDYNHIP_EDIT_SHAPE | EDYNHIP_EDIT_KIND;

    // ---- which shards take an edit: the owner of a dynamic body, every shard for a replicated one
    for (uint32_t r = 0; r < 4; ++r) {
        CHECK(shard_takes_body_edit(DYN, 2, r) == (r == 2));
        CHECK(shard_takes_body_edit(STA, -1, r));
        CHECK(shard_takes_body_edit(KIN, -1, r));
        // (the kind before the edit decides: a body about to be made dynamic is still on every shard, whatever rank it is about to get)
        CHECK(shard_takes_body_edit(STA, 1, r));
    }
    // ---- crossing the replication boundary: dynamic <-> not dynamic only
    CHECK(edit_crosses_boundary(DYN, STA) && edit_crosses_boundary(DYN, KIN) && edit_crosses_boundary(STA, DYN) && edit_crosses_boundary(KIN, DYN));
    CHECK(!edit_crosses_boundary(DYN, DYN) && !edit_crosses_boundary(STA, KIN) && !edit_crosses_boundary(KIN, STA) && !edit_crosses_boundary(STA, STA));
    CHECK(kind_after_edit(EDYNHIP_EDIT_MASS, DYN, STA) == DYN);   // KIND not named: the kind given is not read
    CHECK(kind_after_edit(EDYNHIP_EDIT_KIND | EDYNHIP_EDIT_MASS, DYN, STA) == STA);
    CHECK(kind_after_edit(ALL, KIN, DYN) == DYN);
    // ---- the owner of a body made dynamic: fewest live dynamic bodies, ties to the lowest shard, one after the other
    {
        std::vector<uint32_t> load = {5, 3, 3, 7};
        CHECK(owner_of_new_dynamic(load) == 1 && load[1] == 4);
        CHECK(owner_of_new_dynamic(load) == 2 && load[2] == 4);
        CHECK(owner_of_new_dynamic(load) == 1 && load[1] == 5);
        CHECK(owner_of_new_dynamic(load) == 2);
        CHECK(owner_of_new_dynamic(load) == 0 && load[0] == 6);   // 5 5 5 7: the lowest of three
        std::vector<uint32_t> one = {9};
        CHECK(owner_of_new_dynamic(one) == 0 && one[0] == 10);
        std::vector<uint32_t> empty_world = {0, 0, 0};
        CHECK(owner_of_new_dynamic(empty_world) == 0 && owner_of_new_dynamic(empty_world) == 1 && owner_of_new_dynamic(empty_world) == 2 && owner_of_new_dynamic(empty_world) == 0);
        // the same rule as place_new_bodies for bodies that touch nobody of their call
        std::vector<uint32_t> la = {2, 1, 1}, lb = la, extra(3, 0);
        const int32_t kinds[3] = {DYN, DYN, DYN};
        const uint32_t group[3] = {0, 1, 2};
        const std::vector<int32_t> place = place_new_bodies(3, kinds, group, la, extra);
        for (int k = 0; k < 3; ++k) CHECK((int32_t)owner_of_new_dynamic(lb) == place[k]);
    }
    // ---- when the approach check is due at once
    for (uint32_t W = 1; W <= 3; ++W) {
        const bool many = W > 1;
        CHECK(edit_needs_approach_check(EDYNHIP_EDIT_SHAPE, DYN, DYN, W) == many);                       // a dynamic body reshaped
        CHECK(edit_needs_approach_check(EDYNHIP_EDIT_SHAPE | EDYNHIP_EDIT_MASS, DYN, DYN, W) == many);
        CHECK(edit_needs_approach_check(ALL, STA, DYN, W) == many);                                      // made dynamic
        CHECK(edit_needs_approach_check(EDYNHIP_EDIT_KIND | EDYNHIP_EDIT_MASS | EDYNHIP_EDIT_INERTIA, KIN, DYN, W) == many);
        CHECK(!edit_needs_approach_check(EDYNHIP_EDIT_MASS | EDYNHIP_EDIT_INERTIA | EDYNHIP_EDIT_MATERIAL, DYN, DYN, W));
        CHECK(!edit_needs_approach_check(EDYNHIP_EDIT_KIND | EDYNHIP_EDIT_MASS | EDYNHIP_EDIT_INERTIA, DYN, DYN, W));   // stays dynamic, same shape
        CHECK(!edit_needs_approach_check(EDYNHIP_EDIT_SHAPE, STA, STA, W));                              // replicated: on every shard already
        CHECK(!edit_needs_approach_check(EDYNHIP_EDIT_SHAPE | EDYNHIP_EDIT_KIND, STA, KIN, W));
        CHECK(!edit_needs_approach_check(EDYNHIP_EDIT_SHAPE | EDYNHIP_EDIT_KIND, DYN, STA, W));          // leaves the dynamic bodies
    }
    // ---- the inertia written out before a shape or a mass changes without it
    {
        float I[9];
        const float box[4] = {0.5f, 1.0f, 1.5f, 0};
        CHECK(bake_shape_inertia(EDYNHIP_SHAPE_BOX, box, 3.0f, false, I));
        const float c = 1.0f / 12.0f * 3.0f;
        CHECK(I[0] == c * (2.0f * 2.0f + 3.0f * 3.0f) && I[4] == c * (3.0f * 3.0f + 1.0f * 1.0f) && I[8] == c * (1.0f * 1.0f + 2.0f * 2.0f));
        CHECK(I[1] == 0 && I[2] == 0 && I[3] == 0 && I[5] == 0 && I[6] == 0 && I[7] == 0);
        const float ball[4] = {0.25f, 0, 0, 0};
        CHECK(bake_shape_inertia(EDYNHIP_SHAPE_SPHERE, ball, 2.0f, false, I));
        CHECK(I[0] == 0.4f * 2.0f * 0.25f * 0.25f && I[4] == I[0] && I[8] == I[0] && I[1] == 0);
        CHECK(!bake_shape_inertia(EDYNHIP_SHAPE_BOX, box, 3.0f, true, I));        // a centre-of-mass offset shifts it: left to the device
        CHECK(!bake_shape_inertia(EDYNHIP_SHAPE_CAPSULE, box, 3.0f, false, I));
        CHECK(!bake_shape_inertia(EDYNHIP_SHAPE_CYLINDER, box, 3.0f, false, I));
        CHECK(!bake_shape_inertia(EDYNHIP_SHAPE_POLYHEDRON, box, 3.0f, false, I));
        CHECK(!bake_shape_inertia(EDYNHIP_SHAPE_NONE, box, 3.0f, false, I));
    }
    // ---- validation as the world calls it: global indices, the world's tombstones, the scene's mesh count - in the documented order
    {
        const uint32_t N = 10;
        std::vector<uint8_t> tombs(N, 0);
        tombs[4] = 1;
        const uint32_t meshes = 2;
        const char *why = "";
        edynhip_bodies v;
        std::memset(&v, 0, sizeof(v));
        const float mass[3] = {1, 2, 3}, inertia[27] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1}, fr[3] = {0.5f, 0.5f, 0.5f};
        const uint8_t has[3] = {1, 1, 1};
        int32_t shape[3] = {EDYNHIP_SHAPE_BOX, EDYNHIP_SHAPE_POLYHEDRON, EDYNHIP_SHAPE_SPHERE}, kind[3] = {STA, KIN, STA};
        float param[12] = {0.5f, 0.5f, 0.5f, 0, 1, 0, 0, 0, 0.5f, 0, 0, 0};
        v.mass = mass; v.inertia = inertia; v.has_inertia = has; v.friction = fr; v.restitution = fr; v.shape_type = shape; v.shape_param = param; v.kind = kind;
        uint32_t idx[3] = {0, 9, 3};
        auto run = [&](uint32_t fields) { why = ""; return validate_body_edit(3, idx, &v, fields, N, tombs, meshes, &why); };
        CHECK(run(ALL) == EDYNHIP_OK);
        CHECK(run(32) == EDYNHIP_ERR_INVALID && std::string(why) == "unknown field group");
        // an unknown group is found before a bad index, a bad index before a tombstone, a tombstone before a repeat
        idx[1] = N; CHECK(run(ALL | 64) == EDYNHIP_ERR_INVALID && std::string(why) == "unknown field group");
        CHECK(run(ALL) == EDYNHIP_ERR_INVALID && std::string(why) == "index out of range");
        idx[1] = 9; idx[0] = 4; idx[2] = 4; CHECK(run(ALL) == EDYNHIP_ERR_INVALID && std::string(why) == "index of a removed body");
        idx[0] = 3; idx[2] = 3; CHECK(run(ALL) == EDYNHIP_ERR_INVALID && std::string(why) == "index listed twice");
        idx[0] = 0;
        // a repeat before the mesh id, the mesh id before the kind
        param[4] = (float)meshes; kind[0] = 7;
        CHECK(run(ALL) == EDYNHIP_ERR_INVALID && std::string(why).find("mesh") != std::string::npos);
        param[4] = 1; CHECK(run(ALL) == EDYNHIP_ERR_INVALID && std::string(why).find("kind") != std::string::npos);
        kind[0] = DYN;
        CHECK(run(ALL) == EDYNHIP_OK);
        CHECK(run(EDYNHIP_EDIT_KIND | EDYNHIP_EDIT_MASS) == EDYNHIP_ERR_INVALID && std::string(why).find("MASS and INERTIA") != std::string::npos);
        CHECK(run(EDYNHIP_EDIT_KIND) == EDYNHIP_ERR_INVALID);
        // a world whose scene holds no mesh refuses every polyhedron
        CHECK(validate_body_edit(3, idx, &v, EDYNHIP_EDIT_SHAPE, N, tombs, 0, &why) == EDYNHIP_ERR_INVALID);
        // no tombstones yet (the world's vector is shorter than the scene, or empty)
        idx[2] = 4;
        CHECK(validate_body_edit(3, idx, &v, EDYNHIP_EDIT_MASS, N, std::vector<uint8_t>{}, meshes, &why) == EDYNHIP_OK);
        CHECK(validate_body_edit(3, idx, &v, EDYNHIP_EDIT_MASS, N, std::vector<uint8_t>(3, 0), meshes, &why) == EDYNHIP_OK);
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("WORLD_BODY_EDIT_RULES_OK\n");
    return 0;
}
