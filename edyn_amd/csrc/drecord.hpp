// The 96-byte registry record of one body (include/edynhip.h edynhip_body_record), computed once: k_pack_records (capi.hip, one context)
// and k_world_pack_records (world_records.hip, a shard of a multi-device world) both call body_record, so the two hand-overs cannot drift.
//   update_presentation.cpp:73-79   pre = pos + vel * interpolation_dt; pre = integrate(orn, vel, interpolation_dt)
//   update_origins.cpp:13-15        origin (meaningful when EDYNHIP_RECORD_HAS_ORIGIN is set)
#pragma once
#include "ctx.hpp"
#include "dmath.hpp"

namespace eh {
using namespace dm;

// o[0..5]: the record as six float4 (pos orn linvel angvel | present_pos present_orn | origin flags), body i of `b`
DI void body_record(const Bodies &b, uint32_t i, float present_dt, float4 (&o)[6]) {
    const float4 p4 = B_POS(b, i), q4v = B_ORN(b, i), v4 = b.linvel[i], w4 = b.angvel[i];
    const uint32_t fl = b.flags[i];
    const f3 p = from4(p4), v = from4(v4), w = from4(w4);
    const q4 q{q4v.x, q4v.y, q4v.z, q4v.w};
    const f3 pp = p + v * present_dt;
    const q4 po = integrate(q, w, present_dt);
    const bool has_origin = b.origin && b.com[i].w != 0.0f;
    const f3 org = has_origin ? from4(b.origin[i]) : p;
    uint32_t rf = 0;
    if ((fl & BF_KIND_MASK) == EDYNHIP_KIND_DYNAMIC) rf |= EDYNHIP_RECORD_DYNAMIC;
    if (fl & BF_ASLEEP) rf |= EDYNHIP_RECORD_ASLEEP;
    if (has_origin) rf |= EDYNHIP_RECORD_HAS_ORIGIN;
    if (fl & BF_REMOVED) rf |= EDYNHIP_RECORD_REMOVED;
    o[0] = make_float4(p.x, p.y, p.z, q.x);
    o[1] = make_float4(q.y, q.z, q.w, v.x);
    o[2] = make_float4(v.y, v.z, w.x, w.y);
    o[3] = make_float4(w.z, pp.x, pp.y, pp.z);
    o[4] = make_float4(po.x, po.y, po.z, po.w);
    o[5] = make_float4(org.x, org.y, org.z, __uint_as_float(rf));
}

}  // namespace eh
