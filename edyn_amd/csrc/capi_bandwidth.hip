// C-ABI, measurement aid (include/edynhip.h edynhip_measure_bandwidth): what this chip streams - the practical denominator printed
// next to the HBM spec peak.
#include "ctx.hpp"
#include <algorithm>

extern "C" {

__global__ void __launch_bounds__(256) k_bw_read(const float4 *__restrict__ src, size_t n, float4 *sink) {
    float4 acc = make_float4(0, 0, 0, 0);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float4 v = src[i];
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    if (acc.x == 12345.678f) sink[0] = acc;   // never true for the zero-filled buffer: keeps the loads alive
}
__global__ void __launch_bounds__(256) k_bw_copy(const float4 *__restrict__ src, float4 *__restrict__ dst, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = src[i];
}
int edynhip_measure_bandwidth(edynhip_ctx *c, uint64_t bytes, float *read_gbs, float *copy_gbs) {
    if (!c || bytes < (1u << 20)) return EDYNHIP_ERR_INVALID;
    EH_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)(bytes / sizeof(float4));
    eh::DeviceBuf<float4> a, b;
    if (a.alloc(n) != hipSuccess) return eh::set_error(c, EDYNHIP_ERR_HIP, "edynhip_measure_bandwidth: hipMalloc");
    if (b.alloc(n) != hipSuccess) return eh::set_error(c, EDYNHIP_ERR_HIP, "edynhip_measure_bandwidth: hipMalloc");
    eh::Event e0, e1;
    hipError_t err = e0.create();
    if (err == hipSuccess) err = e1.create();
    if (err == hipSuccess) err = hipMemsetAsync(a, 0, n * sizeof(float4), c->stream);
    if (err == hipSuccess) err = hipMemsetAsync(b, 0, n * sizeof(float4), c->stream);
    int ncu = 256;
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device);
    const dim3 grid((unsigned)ncu * 8u), block(256);
    float best_r = 0, best_c = 0;
    for (int rep = 0; rep < 6 && err == hipSuccess; ++rep) {   // the first pass of each is a warm-up
        float ms = 0;
        (void)hipEventRecord(e0, c->stream);
        hipLaunchKernelGGL(k_bw_read, grid, block, 0, c->stream, (const float4 *)a, n, (float4 *)b);
        (void)hipEventRecord(e1, c->stream);
        err = hipEventSynchronize(e1);
        if (err == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms > 0 && rep > 0) best_r = std::max(best_r, (float)(n * sizeof(float4) / 1e6 / ms));
        (void)hipEventRecord(e0, c->stream);
        hipLaunchKernelGGL(k_bw_copy, grid, block, 0, c->stream, (const float4 *)a, (float4 *)b, n);
        (void)hipEventRecord(e1, c->stream);
        if (err == hipSuccess) err = hipEventSynchronize(e1);
        if (err == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms > 0 && rep > 0) best_c = std::max(best_c, (float)(2.0 * n * sizeof(float4) / 1e6 / ms));
    }
    if (err != hipSuccess) return eh::set_error(c, EDYNHIP_ERR_HIP, "edynhip_measure_bandwidth", err);
    if (read_gbs) *read_gbs = best_r;
    if (copy_gbs) *copy_gbs = best_c;
    return EDYNHIP_OK;
}

}  // extern "C"
