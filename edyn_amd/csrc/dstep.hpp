// Device code that more than one stage file needs (islands.hip, colouring.hip, solver.hip): the launch-grid helper, the body-kind
// test and the per-body start of the solve, which k_solve_begin (solver.hip) and k_cc_flatten<true> (islands.hip) both run.
//   apply_gravity               include/edyn/sys/apply_gravity.hpp:12-17
#pragma once
#include "ctx.hpp"
#include "dmath.hpp"

namespace eh {
using namespace dm;

static inline uint32_t blocks(uint32_t n, uint32_t bs) { return (n + bs - 1) / bs; }

DI bool is_dynamic(uint32_t flags) { return (flags & BF_KIND_MASK) == EDYNHIP_KIND_DYNAMIC; }

// The per-body start of the solve (k_solve_begin: gravity, zeroed deltas, hand-off chain heads) - also folded into k_cc_flatten, the
// per-body kernel that precedes it, when nothing that runs in between reads velocities or sleep flags (no island sleeping, no restitution).
DI void solve_begin_body(uint32_t i, Bodies &b, float dt, uint32_t *first_slot) {
    first_slot[i] = 0xFFFFFFFFu;
    uint32_t fl = b.flags[i];
    float inv_m = 0;
    if (is_dynamic(fl)) {
        inv_m = B_POS(b, i).w;
        f3 g = from4(b.grav[i]);
        if (!(g.x == 0 && g.y == 0 && g.z == 0) && !(fl & BF_ASLEEP)) {   // apply_gravity.hpp:13 excludes sleeping bodies
            f3 v = from4(b.linvel[i]);
            v += g * dt;
            b.linvel[i] = to4(v, 0);
        }
    }
    B_DV(b, i) = make_float4(0, 0, 0, inv_m);
    B_DW(b, i) = make_float4(0, 0, 0, 0);
}

}  // namespace eh
