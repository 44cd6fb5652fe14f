// What edynhip_edit_bodies refuses (edyn_amd/csrc/ctx_rules.hpp validate_body_edit), checked against the statements of
// include/edynhip.h: plain C++, no HIP, no library. Own main: the test builds it a second time with the address and undefined-behaviour
// sanitizers and runs it as a stand-alone program.
#include "../../edyn_amd/csrc/ctx_rules.hpp"
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED: %s (line %d)\n", #cond, __LINE__); ++failures; } } while (0)

namespace {
struct Edit {   // the arrays a caller hands over, exactly as long as the list: a rule that reads past the end is caught by the sanitizer
    std::vector<uint32_t> idx;
    std::vector<int32_t> kind, shape;
    std::vector<float> mass, inertia, param, friction, restitution;
    std::vector<uint8_t> has;
    edynhip_bodies view() const {
        edynhip_bodies b;
        std::memset(&b, 0, sizeof(b));
        b.kind = kind.empty() ? nullptr : kind.data(); b.shape_type = shape.empty() ? nullptr : shape.data();
        b.mass = mass.empty() ? nullptr : mass.data(); b.inertia = inertia.empty() ? nullptr : inertia.data();
        b.shape_param = param.empty() ? nullptr : param.data(); b.friction = friction.empty() ? nullptr : friction.data();
        b.restitution = restitution.empty() ? nullptr : restitution.data(); b.has_inertia = has.empty() ? nullptr : has.data();
        return b;
    }
};
int run(const Edit &e, uint32_t fields, uint32_t bodies, const std::vector<uint8_t> &removed, uint32_t meshes, std::string *why = nullptr) {
    const edynhip_bodies b = e.view();
    const char *w = "";
    const int rc = eh::validate_body_edit((uint32_t)e.idx.size(), e.idx.empty() ? nullptr : e.idx.data(), &b, fields, bodies, removed, meshes, &w);
    if (why) *why = w;
    return rc;
}
}  // namespace

int main() {
    const uint32_t N = 10;
    std::vector<uint8_t> removed(N, 0);
    removed[4] = 1;
    const uint32_t ALL = EDYNHIP_EDIT_MASS | EDYNHIP_EDIT_INERTIA | EDYNHIP_EDIT_MATERIAL | EDYNHIP_EDIT_SHAPE | EDYNHIP_EDIT_KIND;
    static_assert(EDYNHIP_EDIT_MASS == 1 && EDYNHIP_EDIT_INERTIA == 2 && EDYNHIP_EDIT_MATERIAL == 4 && EDYNHIP_EDIT_SHAPE == 8 && EDYNHIP_EDIT_KIND == 16, "edynhip.h");
    CHECK(eh::kEditGroups == ALL);

    // n == 0 is valid, with or without arrays; an unknown group is not
    CHECK(run(Edit{}, ALL, N, removed, 0) == EDYNHIP_OK);
    CHECK(eh::validate_body_edit(0, nullptr, nullptr, 0, N, removed, 0, nullptr) == EDYNHIP_OK);
    CHECK(eh::validate_body_edit(0, nullptr, nullptr, 32, N, removed, 0, nullptr) == EDYNHIP_ERR_INVALID);

    Edit mass;
    mass.idx = {0, 9, 3}; mass.mass = {1, 2, 3};
    CHECK(run(mass, EDYNHIP_EDIT_MASS, N, removed, 0) == EDYNHIP_OK);
    {   // missing arrays
        const edynhip_bodies b = mass.view();
        CHECK(eh::validate_body_edit(3, nullptr, &b, EDYNHIP_EDIT_MASS, N, removed, 0, nullptr) == EDYNHIP_ERR_INVALID);
        CHECK(eh::validate_body_edit(3, mass.idx.data(), nullptr, EDYNHIP_EDIT_MASS, N, removed, 0, nullptr) == EDYNHIP_ERR_INVALID);
        CHECK(run(mass, EDYNHIP_EDIT_MATERIAL, N, removed, 0) == EDYNHIP_ERR_INVALID);
        CHECK(run(mass, EDYNHIP_EDIT_SHAPE, N, removed, 0) == EDYNHIP_ERR_INVALID);
        CHECK(run(mass, EDYNHIP_EDIT_KIND, N, removed, 0) == EDYNHIP_ERR_INVALID);
    }
    // indices: out of range (the last entry of a list that is fine otherwise), a removed body, listed twice
    std::string why;
    { Edit e = mass; e.idx = {0, 9, N}; CHECK(run(e, EDYNHIP_EDIT_MASS, N, removed, 0, &why) == EDYNHIP_ERR_INVALID && why == "index out of range"); }
    { Edit e = mass; e.idx = {0, 0xFFFFFFFFu, 1}; CHECK(run(e, EDYNHIP_EDIT_MASS, N, removed, 0) == EDYNHIP_ERR_INVALID); }
    { Edit e = mass; e.idx = {0, 4, 3}; CHECK(run(e, EDYNHIP_EDIT_MASS, N, removed, 0, &why) == EDYNHIP_ERR_INVALID && why == "index of a removed body"); }
    { Edit e = mass; e.idx = {7, 2, 7}; CHECK(run(e, EDYNHIP_EDIT_MASS, N, removed, 0, &why) == EDYNHIP_ERR_INVALID && why == "index listed twice"); }
    { Edit e = mass; e.idx = {0, 9, 3}; CHECK(run(e, EDYNHIP_EDIT_MASS, N, std::vector<uint8_t>{}, 0) == EDYNHIP_OK); }   // no tombstones known: none

    // INERTIA: given needs the array; derived (has_inertia 0 or no has_inertia at all) needs MASS
    Edit in;
    in.idx = {1, 2}; in.mass = {1, 1}; in.inertia.assign(18, 0.1f); in.has = {1, 1};
    CHECK(run(in, EDYNHIP_EDIT_INERTIA, N, removed, 0) == EDYNHIP_OK);
    { Edit e = in; e.has = {1, 0}; CHECK(run(e, EDYNHIP_EDIT_INERTIA, N, removed, 0) == EDYNHIP_ERR_INVALID); CHECK(run(e, EDYNHIP_EDIT_INERTIA | EDYNHIP_EDIT_MASS, N, removed, 0) == EDYNHIP_OK); }
    { Edit e = in; e.has.clear(); e.inertia.clear(); CHECK(run(e, EDYNHIP_EDIT_INERTIA, N, removed, 0) == EDYNHIP_ERR_INVALID); CHECK(run(e, EDYNHIP_EDIT_INERTIA | EDYNHIP_EDIT_MASS, N, removed, 0) == EDYNHIP_OK); }
    { Edit e = in; e.inertia.clear(); CHECK(run(e, EDYNHIP_EDIT_INERTIA | EDYNHIP_EDIT_MASS, N, removed, 0) == EDYNHIP_ERR_INVALID); }

    // SHAPE: box .. polyhedron; a polyhedron names one of the context's meshes by a whole, non-negative number
    Edit sh;
    sh.idx = {5, 6}; sh.shape = {EDYNHIP_SHAPE_BOX, EDYNHIP_SHAPE_POLYHEDRON}; sh.param = {0.5f, 0.5f, 0.5f, 0, 2, 0, 0, 0};
    CHECK(run(sh, EDYNHIP_EDIT_SHAPE, N, removed, 3) == EDYNHIP_OK);
    CHECK(run(sh, EDYNHIP_EDIT_SHAPE, N, removed, 2, &why) == EDYNHIP_ERR_INVALID && why.find("mesh") != std::string::npos);
    { Edit e = sh; e.shape[0] = EDYNHIP_SHAPE_NONE; CHECK(run(e, EDYNHIP_EDIT_SHAPE, N, removed, 3) == EDYNHIP_ERR_UNSUPPORTED); }
    { Edit e = sh; e.shape[1] = EDYNHIP_SHAPE_POLYHEDRON + 1; CHECK(run(e, EDYNHIP_EDIT_SHAPE, N, removed, 3) == EDYNHIP_ERR_UNSUPPORTED); }
    { Edit e = sh; e.shape[0] = -1; CHECK(run(e, EDYNHIP_EDIT_SHAPE, N, removed, 3) == EDYNHIP_ERR_UNSUPPORTED); }
    for (float bad : {-1.0f, 0.5f, 3.0f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()}) {
        Edit e = sh; e.param[4] = bad;
        CHECK(run(e, EDYNHIP_EDIT_SHAPE, N, removed, 3) == EDYNHIP_ERR_INVALID);
    }
    for (int t = EDYNHIP_SHAPE_BOX; t <= EDYNHIP_SHAPE_POLYHEDRON; ++t) { Edit e = sh; e.shape[0] = t; e.param[0] = 0; CHECK(run(e, EDYNHIP_EDIT_SHAPE, N, removed, 3) == EDYNHIP_OK); }

    // KIND: one of the three; dynamic only together with MASS and INERTIA
    Edit kd;
    kd.idx = {8, 7}; kd.kind = {EDYNHIP_KIND_KINEMATIC, EDYNHIP_KIND_STATIC}; kd.mass = {1, 1}; kd.inertia.assign(18, 0.1f); kd.has = {1, 1};
    CHECK(run(kd, EDYNHIP_EDIT_KIND, N, removed, 0) == EDYNHIP_OK);
    { Edit e = kd; e.kind[1] = 3; CHECK(run(e, EDYNHIP_EDIT_KIND, N, removed, 0) == EDYNHIP_ERR_INVALID); }
    { Edit e = kd; e.kind[0] = -1; CHECK(run(e, EDYNHIP_EDIT_KIND, N, removed, 0) == EDYNHIP_ERR_INVALID); }
    {
        Edit e = kd; e.kind[1] = EDYNHIP_KIND_DYNAMIC;
        CHECK(run(e, EDYNHIP_EDIT_KIND, N, removed, 0) == EDYNHIP_ERR_INVALID);
        CHECK(run(e, EDYNHIP_EDIT_KIND | EDYNHIP_EDIT_MASS, N, removed, 0) == EDYNHIP_ERR_INVALID);
        CHECK(run(e, EDYNHIP_EDIT_KIND | EDYNHIP_EDIT_INERTIA, N, removed, 0) == EDYNHIP_ERR_INVALID);
        CHECK(run(e, EDYNHIP_EDIT_KIND | EDYNHIP_EDIT_MASS | EDYNHIP_EDIT_INERTIA, N, removed, 0) == EDYNHIP_OK);
    }
    // the first fault found decides: an unsupported shape behind a bad index reads INVALID
    { Edit e = sh; e.idx = {5, N + 3}; e.shape[0] = EDYNHIP_SHAPE_NONE; CHECK(run(e, EDYNHIP_EDIT_SHAPE, N, removed, 3) == EDYNHIP_ERR_INVALID); }

    // a long list: every index once is fine, one repeat anywhere is not
    {
        Edit e;
        const uint32_t big = 5000;
        std::vector<uint8_t> none(big, 0);
        for (uint32_t i = 0; i < big; ++i) { e.idx.push_back((i * 7u + 3u) % big); e.mass.push_back(1); }   // (7 and 5000 are coprime: a permutation)
        CHECK(run(e, EDYNHIP_EDIT_MASS, big, none, 0) == EDYNHIP_OK);
        e.idx[big - 1] = e.idx[17];
        CHECK(run(e, EDYNHIP_EDIT_MASS, big, none, 0) == EDYNHIP_ERR_INVALID);
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("BODY_EDIT_RULES_OK\n");
    return 0;
}
