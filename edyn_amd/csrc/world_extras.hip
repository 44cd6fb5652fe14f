// contact_extras materials on a multi-device world (multi_materials.hip): what a contact point carries beyond edynhip_manifold - its material
// as mixed when it was created (Manifolds::xmat) and the warm-start impulses of its rolling pair and spinning row (Manifolds::ximp) - as one
// table on the shard's device, and back:
//   - the slot-major xmat / ximp columns of the current manifold array as one 128-byte row per manifold, [m][4][2] float4 in
//     edynhip_get_manifolds order (k_world_gather_extras): what a re-partition carries and what edynhip_world_get_point_extras reads;
//   - the same table written back over what edynhip_set_manifolds mixed afresh (k_world_inject_extras), living slots only.
// Both stream: one manifold per lane, 16-byte loads and stores, no LDS, no atomics. The row layout is world_rules.hpp's.
#include "ctx.hpp"
#include "dmath.hpp"
#include "world_rules.hpp"

namespace eh {

static_assert(kExtrasRowFloats * sizeof(float) == 2 * kMaxPts * sizeof(float4), "one float4 pair per point slot");
static_assert(kMaterialLarge == dm::kLarge, "the rules' default stiffness is the device's");

// rows[8 m + 2 k] = xmat, rows[8 m + 2 k + 1] = ximp of point k of manifold m; zeros where there is no point (a dead slot of
// edynhip_get_point_extras). A lane reads 4 + 4 columns 16 bytes wide - consecutive lanes, consecutive addresses - and writes its 128 bytes.
__global__ void __launch_bounds__(256) k_world_gather_extras(uint32_t M, const float4 *__restrict__ xmat, const float4 *__restrict__ ximp, uint32_t cap,
                                                             const uint32_t *__restrict__ info, float4 *__restrict__ rows) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const uint32_t np = info[m] & 0xFFu;
    const float4 zero = make_float4(0, 0, 0, 0);
    float4 a[kMaxPts], b[kMaxPts];
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kMaxPts; ++k) {
        const bool live = k < np;
        a[k] = live ? xmat[slot_at(cap, k, m)] : zero;
        b[k] = live ? ximp[slot_at(cap, k, m)] : zero;
    }
    float4 *o = rows + 2 * (size_t)kMaxPts * m;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kMaxPts; ++k) { o[2 * k] = a[k]; o[2 * k + 1] = b[k]; }
}

__global__ void __launch_bounds__(256) k_world_inject_extras(uint32_t M, const float4 *__restrict__ rows, float4 *__restrict__ xmat, float4 *__restrict__ ximp, uint32_t cap,
                                                             const uint32_t *__restrict__ info) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const uint32_t np = info[m] & 0xFFu;
    const float4 *s = rows + 2 * (size_t)kMaxPts * m;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kMaxPts; ++k)
        if (k < np) { xmat[slot_at(cap, k, m)] = s[2 * k]; ximp[slot_at(cap, k, m)] = s[2 * k + 1]; }
}

// rows_dev[num_manifolds][4][2] float4 on the context's device, enqueued on its stream. A context without extras storage: nothing to do.
int shard_gather_point_extras(edynhip_ctx *c, void *rows_dev) {
    const Manifolds &mf = c->m[c->cur];
    const uint32_t M = c->num_manifolds;
    if (!mf.xmat || M == 0) return EDYNHIP_OK;
    if (M > mf.cap) return set_error(c, EDYNHIP_ERR_INTERNAL, "shard_gather_point_extras: more manifolds than the array holds");
    hipLaunchKernelGGL(k_world_gather_extras, dim3((M + 255) / 256), dim3(256), 0, c->stream, M, (const float4 *)mf.xmat, (const float4 *)mf.ximp, mf.cap,
                       (const uint32_t *)mf.info, (float4 *)rows_dev);
    EH_HIP(c, hipGetLastError());
    return EDYNHIP_OK;
}

int shard_inject_point_extras(edynhip_ctx *c, const void *rows_dev, uint32_t M) {
    const Manifolds &mf = c->m[c->cur];
    if (!mf.xmat) return EDYNHIP_OK;
    if (M != c->num_manifolds || M > mf.cap) return set_error(c, EDYNHIP_ERR_INVALID, "shard_inject_point_extras: one row per manifold of the current array");
    if (M == 0) return EDYNHIP_OK;
    hipLaunchKernelGGL(k_world_inject_extras, dim3((M + 255) / 256), dim3(256), 0, c->stream, M, (const float4 *)rows_dev, mf.xmat, mf.ximp, mf.cap, (const uint32_t *)mf.info);
    EH_HIP(c, hipGetLastError());
    return EDYNHIP_OK;
}

bool shard_has_extras_storage(const edynhip_ctx *c) { return c->m[c->cur].xmat != nullptr; }

}  // namespace eh
