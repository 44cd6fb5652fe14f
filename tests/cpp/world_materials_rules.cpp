// The host rules of materials on a multi-device world (edyn_amd/csrc/world_rules.hpp "materials") on a machine without a GPU.
// Every expected value below is written from the rule's statement, none by running the rule.
#include "../../edyn_amd/csrc/world_rules.hpp"
#include <cstdio>
#include <cstring>

using namespace eh;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static const float L = 1e18f;   // large_scalar

static void defaults() {   // comp/material.hpp:15-22: spin 0, roll 0, stiffness and damping large_scalar
    CHECK(kMaterialLarge == L && kUnassignedMaterial == 0xFFFFu);
    CHECK(material_extras_default(0, 0, L, L));
    CHECK(!material_extras_default(0.1f, 0, L, L));
    CHECK(!material_extras_default(0, 0.1f, L, L));
    CHECK(!material_extras_default(0, 0, 1000.0f, L));
    CHECK(!material_extras_default(0, 0, L, 10.0f));
    CHECK(material_extras_valid(0, 0, L, L) && material_extras_valid(0.5f, 2.0f, 1.0f, 1e-3f));
    CHECK(!material_extras_valid(-0.1f, 0, L, L) && !material_extras_valid(0, -1.0f, L, L));
    CHECK(!material_extras_valid(0, 0, 0.0f, L) && !material_extras_valid(0, 0, L, 0.0f) && !material_extras_valid(0, 0, -1.0f, L));
    const float nan = std::nanf("");
    CHECK(!material_extras_valid(0, 0, nan, L) && !material_extras_valid(0, 0, L, nan));
}

static void rows() {   // 32 floats per manifold: point k at [8 k, 8 k + 8) = (roll, spin, stiffness, damping), (imp0, imp1, spin imp, -)
    CHECK(kExtrasRowFloats == 32);
    float row[32];
    for (uint32_t np = 0; np <= 4; ++np) {
        std::memset(row, 0x5A, sizeof(row));
        extras_row_default(row, np);
        for (uint32_t k = 0; k < 4; ++k) {
            const float *p = row + 8 * k;
            CHECK(p[0] == 0 && p[1] == 0 && p[4] == 0 && p[5] == 0 && p[6] == 0 && p[7] == 0);
            CHECK(p[2] == (k < np ? L : 0.0f) && p[3] == (k < np ? L : 0.0f));   // a dead slot is all zero
        }
        CHECK(extras_row_is_default(row, np));
    }
    extras_row_default(row, 3);
    float out[28];
    extras_row_to_out7(row, out);   // edynhip_get_point_extras: rolling impulse[2], spin impulse, roll, spin, stiffness, damping
    for (uint32_t k = 0; k < 4; ++k)
        for (uint32_t f = 0; f < 7; ++f) CHECK(out[7 * k + f] == (k < 3 && f >= 5 ? L : 0.0f));
    // every field of a living point counts, a dead slot's content does not
    for (uint32_t f = 0; f < 7; ++f) {
        extras_row_default(row, 2);
        row[8 + f] = (f == 2 || f == 3) ? 4000.0f : 0.25f;
        CHECK(!extras_row_is_default(row, 2));
        CHECK(extras_row_is_default(row, 1));
    }
    for (uint32_t i = 0; i < 32; ++i) row[i] = (float)(i + 1);
    extras_row_to_out7(row, out);
    const float want[28] = {5, 6, 7, 1, 2, 3, 4, 13, 14, 15, 9, 10, 11, 12, 21, 22, 23, 17, 18, 19, 20, 29, 30, 31, 25, 26, 27, 28};
    CHECK(std::memcmp(out, want, sizeof(want)) == 0);
}

static void ranges() {   // W = 3; rank -1: replicated on every shard
    const int32_t rank[8] = {-1, 0, 0, 2, 2, 1, -1, 2};
    uint8_t t[3];
    auto is = [&](uint8_t a, uint8_t b, uint8_t c) { return t[0] == a && t[1] == b && t[2] == c; };
    shards_of_body_range(rank, 1, 2, 3, t); CHECK(is(1, 0, 0));
    shards_of_body_range(rank, 1, 4, 3, t); CHECK(is(1, 0, 1));
    shards_of_body_range(rank, 5, 1, 3, t); CHECK(is(0, 1, 0));
    shards_of_body_range(rank, 3, 3, 3, t); CHECK(is(0, 1, 1));
    shards_of_body_range(rank, 0, 1, 3, t); CHECK(is(1, 1, 1));     // the ground goes to everybody
    shards_of_body_range(rank, 5, 2, 3, t); CHECK(is(1, 1, 1));
    shards_of_body_range(rank, 4, 0, 3, t); CHECK(is(0, 0, 0));     // an empty range touches nobody
    shards_of_body_range(rank, 7, 1, 3, t); CHECK(is(0, 0, 1));
    const int32_t one[2] = {-1, 0};
    uint8_t t1[1];
    shards_of_body_range(one, 0, 2, 1, t1); CHECK(t1[0] == 1);
}

static void carry() {   // carried once the world has seen a contact_extras material or holds a mix entry; never otherwise
    CHECK(!extras_carry_needed(false, 0));
    CHECK(extras_carry_needed(true, 0));
    CHECK(extras_carry_needed(false, 1));
    CHECK(extras_carry_needed(true, 7));
}

int main() {
    defaults();
    rows();
    ranges();
    carry();
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("WORLD_MATERIALS_RULES_OK\n");
    return 0;
}
