// C-ABI implementation (include/edynhip.h), the context: its lifetime and allocation, the development knobs, the counter hand-shake
// with the device, step orchestration, statistics and timings. Scene edits are capi_scene.hip's, read-back capi_readback.hip's, the
// bandwidth probe capi_bandwidth.hip's. Host-side logic only; every simulation stage runs in the HIP kernels of
// broadphase.hip / narrowphase.hip / islands.hip / colouring.hip / solver.hip. There is no CPU fallback.
#include "ctx.hpp"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>

namespace eh {

static std::string g_create_error;

int set_error(edynhip_ctx *c, int code, const char *what, hipError_t e) {
    std::string msg = what ? what : "";
    if (e != hipSuccess) { msg += ": "; msg += hipGetErrorString(e); }
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

// The development knobs (ctx.hpp Knobs). One row per variable: its name, its kind, its default, the field it fills and one line of
// meaning. ON: on unless the value starts with '0'. OFF: off unless the value starts with '1'. SET: off unless the variable is set, to
// whatever value. NUM: a number. PATH: a file name. The default column is the value of an unset variable (PATH: none).
// scripts/README.md carries the same rows (tests/test_knobs.py compares the two lists).
namespace {
enum KnobKind { KNOB_ON, KNOB_OFF, KNOB_SET, KNOB_NUM, KNOB_PATH };
struct KnobRow {
    const char *name; KnobKind kind; long def;
    bool Knobs::*flag; long Knobs::*num; std::string Knobs::*path;
    const char *meaning;
};
constexpr KnobRow kKnobTable[] = {
    {"EDYNHIP_DATAFLOW", KNOB_ON, 1, &Knobs::dataflow, nullptr, nullptr, "0: no dataflow launches, the per-colour schedule"},
    {"EDYNHIP_DATAFLOW_POS", KNOB_ON, 1, &Knobs::dataflow_pos, nullptr, nullptr, "0: the position solve per colour"},
    {"EDYNHIP_DF_LANES", KNOB_NUM, 0, nullptr, &Knobs::df_lanes, nullptr, "1, 2 or 4: lanes per manifold of the dataflow velocity kernel (0: chosen per step)"},
    {"EDYNHIP_DF_WAVES", KNOB_NUM, 0, nullptr, &Knobs::df_waves, nullptr, "resident waves of the dataflow velocity kernel (0: chosen per step)"},
    {"EDYNHIP_DFP_WAVES", KNOB_NUM, 0, nullptr, &Knobs::dfp_waves, nullptr, "resident waves of the dataflow position kernel (0: chosen per step)"},
    {"EDYNHIP_DF_NAP", KNOB_NUM, 1, nullptr, &Knobs::df_nap, nullptr, "pause between two polls of a wave that found nothing in the dataflow velocity kernels: 0 none, 1 short, else longer"},
    {"EDYNHIP_DF_XCD", KNOB_OFF, 0, &Knobs::df_xcd, nullptr, nullptr, "1: XCD-local task lists in the two-lane velocity kernel and the position kernel"},
    {"EDYNHIP_DF_TRACE", KNOB_PATH, 0, nullptr, nullptr, &Knobs::df_trace, "file that receives four timestamps per task of one dataflow velocity solve (scripts/df_trace.py)"},
    {"EDYNHIP_DFP_TRACE", KNOB_PATH, 0, nullptr, nullptr, &Knobs::dfp_trace, "the same for one dataflow position solve"},
    {"EDYNHIP_DF_TRACE_STEP", KNOB_NUM, 100, nullptr, &Knobs::df_trace_step, nullptr, "which of the context's dataflow solves the two traces record"},
    {"EDYNHIP_ISLAND_FUSED", KNOB_ON, 1, &Knobs::island_fused, nullptr, nullptr, "0: no island-fused schedule"},
    {"EDYNHIP_MIXED", KNOB_ON, 1, &Knobs::mixed, nullptr, nullptr, "0: no mixed schedule"},
    {"EDYNHIP_SPECULATE", KNOB_ON, 1, &Knobs::speculate, nullptr, nullptr, "0: wait for the counters before the manifold build and the row preparation"},
    {"EDYNHIP_INPLACE", KNOB_ON, 1, &Knobs::inplace, nullptr, nullptr, "0: rebuild the manifold array every step"},
    {"EDYNHIP_BP_LISTS", KNOB_ON, 1, &Knobs::bp_lists, nullptr, nullptr, "0: walk the tree every step instead of keeping candidate lists"},
    {"EDYNHIP_BP_ADAPT", KNOB_ON, 1, &Knobs::bp_adapt, nullptr, nullptr, "0: the candidate lists' look-ahead stays fixed"},
    {"EDYNHIP_BP_STATS", KNOB_SET, 0, &Knobs::bp_stats, nullptr, nullptr, "set: what k_bp_pairs had to do, on stderr every 100 steps"},
    {"EDYNHIP_DIRECT_COMPACT", KNOB_ON, 1, &Knobs::direct_compact, nullptr, nullptr, "0: the library-scan form of the pair compaction"},
    {"EDYNHIP_DIRECT_SORT", KNOB_ON, 1, &Knobs::direct_sort, nullptr, nullptr, "0: the library-scan form of the colour sort"},
    {"EDYNHIP_COL_LDS", KNOB_OFF, 0, &Knobs::col_lds, nullptr, nullptr, "1: the one-workgroup colouring rounds keep their marks in a hashed LDS table (k_col_rounds_lds)"},
    {"EDYNHIP_CC_COMPRESS", KNOB_NUM, 1, nullptr, &Knobs::cc_compress, nullptr, "pointer-jumping passes of a full island relabel"},
    {"EDYNHIP_TREE_STATS", KNOB_SET, 0, &Knobs::tree_stats, nullptr, nullptr, "set: on destruction, how many steps relabelled the islands in full and incrementally"},
    {"EDYNHIP_NP_FUSED", KNOB_ON, 1, &Knobs::np_fused, nullptr, nullptr, "0: k_np_detect + k_np_merge through the staging arrays instead of k_np_contacts"},
    {"EDYNHIP_POLY_GROUP", KNOB_NUM, 8, nullptr, &Knobs::poly_group, nullptr, "polyhedron pairs: 0 = one lane per pair in k_np_detect_poly, 8 or 16 = lanes per pair in k_np_pp_axes"},
    {"EDYNHIP_POLY_GROUP2", KNOB_NUM, 4, nullptr, &Knobs::poly_group2, nullptr, "4, 8 or 16: lanes per surviving pair in k_np_pp_contacts"},
    {"EDYNHIP_POLY_HINT", KNOB_ON, 1, &Knobs::poly_hint, nullptr, nullptr, "0: no separating-axis hints"},
    {"EDYNHIP_PP_PROF", KNOB_SET, 0, &Knobs::pp_prof, nullptr, nullptr, "set: phase profile of the two polyhedron-pair kernels, on stderr every 100 steps"},
    {"EDYNHIP_QUERY_SCAN_RATIO", KNOB_NUM, 0, nullptr, &Knobs::query_scan_ratio, nullptr, "AABB queries: a query with more than bodies / ratio hits is packed by a wave (0: the built-in ratio)"},
    {"EDYNHIP_RECORDS_DIRECT", KNOB_NUM, -1, nullptr, &Knobs::records_direct, nullptr, "0 or 1: overrides EDYNHIP_SNAPSHOT_DIRECT of edynhip_snapshot_records (-1: the caller's flag)"},
    {"EDYNHIP_WORLD_SERIAL", KNOB_SET, 0, &Knobs::world_serial, nullptr, nullptr, "set: a multi-device world runs every shard on the caller's thread"},
    {"EDYNHIP_WORLD_TRACE", KNOB_SET, 0, &Knobs::world_trace, nullptr, nullptr, "set: wall time of the phases of a re-partition, on stderr"},
};
}  // namespace
Knobs read_knobs() {
    Knobs k{};
    for (const KnobRow &r : kKnobTable) {
        const char *e = getenv(r.name);
        switch (r.kind) {
        case KNOB_ON: k.*r.flag = e ? e[0] != '0' : r.def != 0; break;
        case KNOB_OFF: k.*r.flag = e ? e[0] == '1' : r.def != 0; break;
        case KNOB_SET: k.*r.flag = e != nullptr; break;
        case KNOB_NUM: k.*r.num = e ? atol(e) : r.def; break;
        case KNOB_PATH: k.*r.path = e ? e : ""; break;
        }
    }
    return k;
}

// Host <- device counters without a stream synchronisation: a one-workgroup kernel copies the counter block into pinned
// host memory, fences, and then publishes a sequence number; the host spins on that number. hipStreamSynchronize wakes
// the host through an interrupt (~25-50 us of idle GPU per sync, scripts/prof_timeline.py); the spin sees the write
// within a few microseconds. If the number does not arrive (a kernel faulted), a real synchronise reports the error.
__global__ void k_publish_counters(const uint32_t *__restrict__ src, uint32_t *dst, uint32_t words, volatile uint32_t *seq, uint32_t value) {
    for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) dst[i] = src[i];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) { __hip_atomic_store((uint32_t *)seq, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }
}
// The two halves of a fetch: the publish kernel is enqueued, then the caller may enqueue work that does not need the host's answer
// (speculative launches whose kernels read their element counts from device memory) before it waits - the GPU then runs that work
// while the sequence number travels to the host and the next launches travel back, instead of idling (~11-14 us per fetch).
int publish_counters(edynhip_ctx *c, size_t bytes, uint32_t *ticket) {
    const uint32_t value = ++c->cnt_seq_next;
    c->last_fetch_step = c->step_index;
    hipLaunchKernelGGL(k_publish_counters, dim3(1), dim3(256), 0, c->stream, (const uint32_t *)c->cnt, (uint32_t *)c->cnt_host,
                       (uint32_t)(bytes / sizeof(uint32_t)), c->cnt_seq, value);
    EH_HIP(c, hipGetLastError());
    *ticket = value;
    return EDYNHIP_OK;
}
int wait_counters(edynhip_ctx *c, uint32_t value) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0; *c->cnt_seq != value; ++spins) {
        __builtin_ia32_pause();
        if ((spins & 0xFFFFu) == 0xFFFFu && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
            EH_HIP(c, hipStreamSynchronize(c->stream));   // surfaces a device fault; otherwise the counters are there now
            if (*c->cnt_seq != value) return set_error(c, EDYNHIP_ERR_INTERNAL, "fetch_counters: the published sequence number never arrived");
            break;
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return EDYNHIP_OK;
}
int fetch_counters(edynhip_ctx *c, size_t bytes) {
    uint32_t ticket = 0;
    EH_TRY(publish_counters(c, bytes, &ticket));
    return wait_counters(c, ticket);
}

static int alloc_manifolds(edynhip_ctx *c, Manifolds &m, uint32_t cap, uint32_t nb) {
    m.cap = cap;
    if (c->cfg.flags & EDYNHIP_FLAG_CONTACT_EVENTS) EH_TRY(dalloc(c, m.pid, (size_t)cap * kMaxPts));
    EH_TRY(dalloc(c, m.seg_start, nb)); EH_TRY(dalloc(c, m.seg_end, nb)); EH_TRY(dalloc(c, m.prev_idx, cap)); EH_TRY(dalloc(c, m.tree, cap));
    EH_TRY(dalloc(c, m.skey, cap)); EH_TRY(dalloc(c, m.bodyA, cap)); EH_TRY(dalloc(c, m.bodyB, cap)); EH_TRY(dalloc(c, m.info, cap));
    if (kPointRecords) {   // one allocation, five interleaved base pointers: element pt_at(cap, k, m) of each is a field of point k of manifold m
        float4 *pts = nullptr;
        EH_TRY(dalloc(c, pts, (size_t)cap * kMaxPts * kPointF));
        m.pA = pts; m.pB = pts + 1; m.nrm = pts + 2; m.lnrm = pts + 3; m.imp = pts + 4;
    } else {
        EH_TRY(dalloc(c, m.pA, (size_t)cap * kMaxPts)); EH_TRY(dalloc(c, m.pB, (size_t)cap * kMaxPts));
        EH_TRY(dalloc(c, m.nrm, (size_t)cap * kMaxPts)); EH_TRY(dalloc(c, m.lnrm, (size_t)cap * kMaxPts));
        EH_TRY(dalloc(c, m.imp, (size_t)cap * kMaxPts));
    }
    return EDYNHIP_OK;
}

static int allocate(edynhip_ctx *c) {
    const uint32_t nb = c->cfg.max_bodies, M = c->cfg.max_manifolds, nj = c->cfg.max_joints;
    Bodies &b = c->b;
    b.cap = nb;
    EH_TRY(dalloc(c, b.xf, (size_t)nb * 8)); EH_TRY(dalloc(c, b.dvw, (size_t)nb * 2)); EH_TRY(dalloc(c, b.linvel, nb)); EH_TRY(dalloc(c, b.angvel, nb));
    EH_TRY(dalloc(c, b.amin, nb)); EH_TRY(dalloc(c, b.amax, nb)); EH_TRY(dalloc(c, b.shape, nb)); EH_TRY(dalloc(c, b.grav, nb));
    EH_TRY(dalloc(c, b.mat, nb)); EH_TRY(dalloc(c, b.mat2, nb)); EH_TRY(dalloc(c, b.flags, nb)); EH_TRY(dalloc(c, b.group, nb)); EH_TRY(dalloc(c, b.mask, nb));
    EH_TRY(dalloc(c, b.island, nb));
    EH_TRY(alloc_manifolds(c, c->m[0], M, nb));
    EH_TRY(alloc_manifolds(c, c->m[1], M, nb));
    Rows &r = c->rows;
    EH_TRY(dalloc(c, r.order, M)); EH_TRY(dalloc(c, r.bA, M)); EH_TRY(dalloc(c, r.bB, M)); EH_TRY(dalloc(c, r.np, M)); EH_TRY(dalloc(c, r.label, M));
    EH_TRY(dalloc(c, r.rw, (size_t)M * kMaxPts * kRowsPerPoint * kRowF));
    EH_TRY(dalloc(c, r.iw, (size_t)M * 6));
    EH_TRY(dalloc(c, r.dslot, ((size_t)M + 64) * 4));   // whole 64-lane blocks (dslot_at)
    EH_TRY(dalloc(c, r.pslot, ((size_t)M + 32) * 6));   // whole 32-lane blocks (pslot_at)
    EH_TRY(dalloc(c, r.next, (size_t)M * 2)); EH_TRY(dalloc(c, r.im, (size_t)M * 2));
    EH_TRY(dalloc(c, r.pw, (size_t)M * kMaxPts * kPosF));
    EH_TRY(dalloc(c, r.slot_of, (size_t)nb * kMaxColours)); EH_TRY(dalloc(c, r.first_slot, nb)); EH_TRY(dalloc(c, r.skip, M));
    LBVH &t = c->bvh;
    EH_TRY(dalloc(c, t.keys, nb)); EH_TRY(dalloc(c, t.keys_sorted, nb));
    EH_TRY(dalloc(c, t.parent, (size_t)2 * nb)); EH_TRY(dalloc(c, t.left, nb)); EH_TRY(dalloc(c, t.right, nb));
    EH_TRY(dalloc(c, t.nmin, (size_t)2 * nb)); EH_TRY(dalloc(c, t.nmax, (size_t)2 * nb)); EH_TRY(dalloc(c, t.visit, nb));
    EH_TRY(dalloc(c, t.np_list, nb)); EH_TRY(dalloc(c, t.rope, (size_t)2 * nb)); EH_TRY(dalloc(c, t.split, 8));
    EH_TRY(dalloc(c, t.cand_list, (size_t)nb * kListCap)); EH_TRY(dalloc(c, t.cand_count, nb)); EH_TRY(dalloc(c, t.ref_min, nb)); EH_TRY(dalloc(c, t.ref_max, nb));
    EH_TRY(dalloc(c, c->np_ra, (size_t)M * kMaxPts)); EH_TRY(dalloc(c, c->np_rb, (size_t)M * kMaxPts)); EH_TRY(dalloc(c, c->np_rn, (size_t)M * kMaxPts));
    EH_TRY(dalloc(c, c->np_rnum, M));
    if (c->cfg.flags & EDYNHIP_FLAG_CONTACT_EVENTS) {
        c->event_cap = 5u * M + 1024u;
        EH_TRY(dalloc(c, c->events, c->event_cap)); EH_TRY(dalloc(c, c->event_count, 4)); EH_TRY(dalloc(c, c->prev_matched, M));
    }
    EH_TRY(dalloc(c, c->pair_keys, M)); EH_TRY(dalloc(c, c->pair_keys_sorted, M)); EH_TRY(dalloc(c, c->new_edges, M)); EH_TRY(dalloc(c, c->new_edge_m, M));
    EH_TRY(dalloc(c, c->isl_top, nb)); EH_TRY(dalloc(c, c->rot_off, nb)); EH_HIP(c, hipMemsetAsync(c->rot_off, 0xFF, (size_t)nb * sizeof(uint32_t), c->stream));
    EH_TRY(dalloc(c, c->own_keys, (size_t)nb * kOwnCap)); EH_TRY(dalloc(c, c->own_count, (size_t)nb + 1)); EH_TRY(dalloc(c, c->own_offset, (size_t)nb + 1));
    EH_TRY(dalloc(c, c->col_keys, M)); EH_TRY(dalloc(c, c->col_keys_sorted, M));
    EH_TRY(dalloc(c, c->col_unc, kColUncCap));
    { const size_t cs = 256 * (((size_t)M + 1023) / 1024) + 1; EH_TRY(dalloc(c, c->cs_hist, cs)); EH_TRY(dalloc(c, c->cs_start, cs)); EH_TRY(dalloc(c, c->cs_sup, 16 * 256)); EH_HIP(c, hipMemset(c->cs_sup, 0, 16 * 256 * sizeof(uint32_t))); }
    EH_TRY(dalloc(c, c->used, nb)); EH_TRY(dalloc(c, c->best[0], nb)); EH_TRY(dalloc(c, c->best[1], nb));
    EH_TRY(dalloc(c, c->com_store, nb)); EH_TRY(dalloc(c, c->origin_store, nb));
    EH_TRY(dalloc(c, c->isl_cnt, (size_t)nb + 1)); EH_TRY(dalloc(c, c->isl_off, (size_t)nb + 1)); EH_TRY(dalloc(c, c->isl_list, nb));
    EH_TRY(dalloc(c, c->isl_items, (size_t)M + nj)); EH_TRY(dalloc(c, c->isl_sorted, (size_t)M + nj)); EH_TRY(dalloc(c, c->isl_joint, nb));
    EH_TRY(dalloc(c, c->isl_err, nb)); EH_TRY(dalloc(c, c->isl_done, nb)); EH_TRY(dalloc(c, c->pos_err, (size_t)nb * kMaxDfPosIters));
    EH_TRY(dalloc(c, c->state.dev, (size_t)nb * 13));
    EH_HIP(c, c->state.host.alloc((size_t)nb * 13));
    EH_TRY(dalloc(c, c->sleep_state, nb)); EH_TRY(dalloc(c, c->sleep_action, nb)); EH_TRY(dalloc(c, c->sleep_since, nb));
    EH_TRY(dalloc(c, c->sleep_old_label, nb)); EH_TRY(dalloc(c, c->sleep_size, nb)); EH_TRY(dalloc(c, c->sleep_best, nb)); EH_TRY(dalloc(c, c->sleep_carried, nb));
    EH_HIP(c, hipMemsetAsync(c->sleep_since, 0xFF, (size_t)nb * sizeof(double), c->stream));   // all ones (a NaN): no timer running
    Joints &j = c->j;
    j.cap = nj;
    EH_TRY(dalloc(c, j.orig, nj)); EH_TRY(dalloc(c, j.type, nj)); EH_TRY(dalloc(c, j.bodyA, nj)); EH_TRY(dalloc(c, j.bodyB, nj));
    EH_TRY(dalloc(c, j.pivA, nj)); EH_TRY(dalloc(c, j.pivB, nj)); EH_TRY(dalloc(c, j.axA, nj)); EH_TRY(dalloc(c, j.pA, nj));
    EH_TRY(dalloc(c, j.qA, nj)); EH_TRY(dalloc(c, j.axB, nj)); EH_TRY(dalloc(c, j.pB, nj)); EH_TRY(dalloc(c, j.impulse, (size_t)nj * kJointSlots));
    EH_TRY(dalloc(c, j.wbx, nj)); EH_TRY(dalloc(c, j.gJ, (size_t)nj * 18)); EH_TRY(dalloc(c, j.params, (size_t)nj * kJointParams)); EH_TRY(dalloc(c, j.angle, nj)); EH_TRY(dalloc(c, j.rmask, nj));
    EH_TRY(dalloc(c, j.rA, nj)); EH_TRY(dalloc(c, j.rB, nj)); EH_TRY(dalloc(c, j.wp, nj)); EH_TRY(dalloc(c, j.wq, nj)); EH_TRY(dalloc(c, j.wax, nj));
    EH_TRY(dalloc(c, j.eff, (size_t)nj * kJointSlots)); EH_TRY(dalloc(c, j.rhs, (size_t)nj * kJointSlots));
    EH_TRY(dalloc(c, j.lo, (size_t)nj * kJointSlots)); EH_TRY(dalloc(c, j.hi, (size_t)nj * kJointSlots));
    c->sort_tmp_bytes = sort_temp_bytes(std::max(std::max(M, nb + 1), 256u * ((M + 1023u) / 1024u) + 1u));
    { void *q = nullptr; EH_HIP(c, hipMalloc(&q, c->sort_tmp_bytes)); c->allocs.push_back(q); c->sort_tmp = q; }
    EH_TRY(dalloc(c, c->cnt, 1));
    EH_HIP(c, c->cnt_host_mem.alloc(1));
    c->cnt_host = c->cnt_host_mem;
    std::memset(c->cnt_host, 0, sizeof(Counters));
    EH_HIP(c, c->cnt_seq_mem.alloc(16));   // a 64-byte line of its own
    std::memset(c->cnt_seq_mem, 0, 64);
    c->cnt_seq = (volatile uint32_t *)(uint32_t *)c->cnt_seq_mem;
    EH_HIP(c, hipStreamSynchronize(c->stream));
    return EDYNHIP_OK;
}

constexpr uint32_t kMaxTimedSteps = 4096;
static int begin_timed_step(edynhip_ctx *c) {
    StageTimer &t = c->timer;
    t.e = nullptr;
    if (!(c->cfg.flags & (EDYNHIP_FLAG_TIMING | EDYNHIP_FLAG_TIMING_SOLVE)) || t.recorded >= kMaxTimedSteps) return EDYNHIP_OK;
    t.mask = (c->cfg.flags & EDYNHIP_FLAG_TIMING) ? 0x7FFu : ((1u << 5) | (1u << 6));
    if (t.recorded >= t.capacity) {
        for (int k = 0; k < StageTimer::kEvents; ++k) { hipEvent_t e; EH_HIP(c, hipEventCreate(&e)); t.ev.push_back(e); }
        t.capacity += 1;
    }
    t.e = &t.ev[(size_t)t.recorded * StageTimer::kEvents];
    return EDYNHIP_OK;
}
static void resolve_timings(edynhip_ctx *c) {
    StageTimer &tm = c->timer;
    edynhip_timings &t = c->timings;
    const uint32_t launches = t.solve_velocity_launches;
    t = edynhip_timings{};
    t.solve_velocity_launches = launches;
    if (tm.recorded == 0) return;
    const bool all = tm.mask == 0x7FFu;
    (void)hipEventSynchronize(tm.ev[(size_t)(tm.recorded - 1) * StageTimer::kEvents + (all ? 10 : 6)]);
    for (uint32_t s = 0; s < tm.recorded; ++s) {
        hipEvent_t *e = &tm.ev[(size_t)s * StageTimer::kEvents];
        auto el = [&](int a, int b) { float ms = 0; if (all || (a == 5 && b == 6)) (void)hipEventElapsedTime(&ms, e[a], e[b]); return ms; };
        t.broadphase_ms += el(0, 1); t.narrowphase_ms += el(1, 2); t.islands_ms += el(2, 3); t.colouring_ms += el(3, 4);
        t.prepare_ms += el(4, 5); t.solve_velocity_ms += el(5, 6); t.integrate_ms += el(6, 7); t.solve_position_ms += el(7, 8);
        t.finish_ms += el(8, 9); t.step_ms += el(0, 10);
    }
    t.steps = tm.recorded;
}

static int run_stages(edynhip_ctx *c, uint32_t mask) {
    c->timer.e = nullptr;
    invalidate_step_began(c);   // (raycast.hip: the query tree is stale)
    c->full_step = mask == EDYNHIP_STAGE_ALL && c->clears_primed;
    if (mask == EDYNHIP_STAGE_ALL) EH_TRY(begin_timed_step(c));
    else invalidate_graph_changed(c, false);   // partial runs (tests) never rely on a previous step's labels
    auto rec = [&](int i) { if (c->timer.e && ((c->timer.mask >> i) & 1u)) (void)hipEventRecord(c->timer.e[i], c->stream); };
    // A stage that fails (capacity, colour limit, device-side invariant) leaves the step half done: k_finish did not run, so
    // nothing pre-cleared the next step's scratch and the island labels are stale. The next call must start from the
    // stand-alone path (memsets + k_step_reset, which also clears the sticky error counters) and relabel the islands.
    auto guarded = [&](int rc) {
        if (rc != EDYNHIP_OK) { invalidate_step_failed(c); c->timer.e = nullptr; }
        return rc;
    };
    rec(0);
    if (mask & EDYNHIP_STAGE_BROADPHASE) EH_TRY(guarded(broadphase(c)));
    rec(1);
    if (mask & EDYNHIP_STAGE_NARROWPHASE) EH_TRY(guarded(narrowphase(c)));
    rec(2);
    if (c->evp.now && c->events) EH_TRY(enqueue_event_prefetch(c));   // every event of a step is emitted by the broadphase and the narrowphase: the list of this call is complete
    if (mask & EDYNHIP_STAGE_ISLANDS) EH_TRY(guarded(islands(c)));
    if (mask & EDYNHIP_STAGE_SOLVE) EH_TRY(guarded(solve(c)));   // records events 3..9
    rec(10);
    c->clears_primed = (mask & EDYNHIP_STAGE_SOLVE) != 0;   // k_finish left the next step's scratch cleared
    if (c->timer.e) { c->timer.recorded += 1; c->timer.e = nullptr; }
    return EDYNHIP_OK;
}

}  // namespace eh

using namespace eh;

extern "C" {

uint32_t edynhip_abi_version(void) { return 15; }   // 15: edynhip_snapshot_records / edynhip_snapshot_map (the registry write-back read in place), edynhip_set_event_prefetch / edynhip_prefetched_events; 14: EDYNHIP_FLAG_FUSED_VELOCITY_ROWS / EDYNHIP_FLAG_BLOCK_POSITION (the default contact arithmetic is the reference's); 13: edynhip_set_pair_filter (settings.should_collide_func); 12: multi-GPU world (edynhip_world_*, multi*.hip); 11: polyhedron shapes (edynhip_create_convex_mesh); 10: edynhip_stats::solve_schedule, edynhip_measure_bandwidth; 9: edynhip_set_center_of_mass; 8: edynhip_bodies::center_of_mass; 7: edynhip_wake_bodies; 6: every constraint type, capsules, material mix table; 5: contact_extras materials; 4: contact events + point ids, double-buffered snapshots;   // 3: joint slots/params, add/remove joints, remove bodies, params, timed steps, exclusions

const char *edynhip_last_error(const edynhip_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

edynhip_ctx *edynhip_create(const edynhip_config *cfg, int *status_out) {
    auto fail = [&](int code, const char *msg, hipError_t e = hipSuccess) -> edynhip_ctx * {
        set_error(nullptr, code, msg, e);
        if (status_out) *status_out = code;
        return nullptr;
    };
    if (!cfg || cfg->max_bodies == 0) return fail(EDYNHIP_ERR_INVALID, "edynhip_create: bad config");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail(EDYNHIP_ERR_NO_DEVICE, "edynhip_create: no HIP device (this library has no CPU fallback)", e);
    if (cfg->device < 0 || cfg->device >= ndev) return fail(EDYNHIP_ERR_INVALID, "edynhip_create: device ordinal out of range");
    e = hipSetDevice(cfg->device);
    if (e != hipSuccess) return fail(EDYNHIP_ERR_HIP, "hipSetDevice", e);
    edynhip_ctx *c = new edynhip_ctx();
    c->cfg = *cfg;
    c->sleeping = (cfg->flags & EDYNHIP_FLAG_SLEEPING) != 0;
    c->knobs = read_knobs();
    c->device = cfg->device;
    if (c->cfg.max_manifolds == 0) c->cfg.max_manifolds = 16 * c->cfg.max_bodies + 1024;
    if (c->cfg.fixed_dt <= 0) c->cfg.fixed_dt = 1.0f / 60.0f;
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return fail(EDYNHIP_ERR_HIP, "hipStreamCreate", e); }
    int rc = allocate(c);
    if (rc != EDYNHIP_OK) {
        g_create_error = c->err;
        if (status_out) *status_out = rc;
        edynhip_destroy(c);
        return nullptr;
    }
    if (status_out) *status_out = EDYNHIP_OK;
    return c;
}

// By hand, because the order matters: the context's device is made current, its stream runs dry, and the queries and the raycast let
// go of what they enqueue on it before it goes. The arena is released here; pinned buffers, events, the side stream and the scratch
// buffers go with their owners when the context is deleted.
void edynhip_destroy(edynhip_ctx *c) {
    if (!c) return;
    if (c->knobs.tree_stats)   // developer knob: how the island labels were kept up to date (islands.hip islands)
        fprintf(stderr, "[edynhip] island labels: %llu steps relabelled in full, %llu incrementally\n", (unsigned long long)c->cc_full_steps, (unsigned long long)c->cc_incremental_steps);
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    eh::raycast_free(c);
    eh::query_aabb_free(c);
    eh::query_tickets_free(c);
    c->allocs.insert(c->allocs.end(), c->mesh_allocs.begin(), c->mesh_allocs.end());   // what mesh.hip allocated for this context joins the arena
    c->allocs.push_back(c->rot); c->allocs.push_back(c->poly_work);
    for (void *p : c->allocs) (void)hipFree(p);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int edynhip_set_stream(edynhip_ctx *c, void *hip_stream) {
    if (!c) return EDYNHIP_ERR_INVALID;
    EH_HIP(c, hipStreamSynchronize(c->stream));
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    if (hip_stream) { c->stream = (hipStream_t)hip_stream; c->own_stream = false; }
    else { EH_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }
    return EDYNHIP_OK;
}

int edynhip_synchronize(edynhip_ctx *c) {
    if (!c) return EDYNHIP_ERR_INVALID;
    EH_HIP(c, hipStreamSynchronize(c->stream));
    return EDYNHIP_OK;
}

int edynhip_run_stages(edynhip_ctx *c, uint32_t mask) {
    if (!c) return EDYNHIP_ERR_INVALID;
    EH_HIP(c, hipSetDevice(c->device));
    EH_TRY(flush_joint_redefs(c));
    EH_TRY(flush_exclusions(c));
    return run_stages(c, mask);
}

static int step_stamped(edynhip_ctx *c, uint32_t nsteps, bool timed, double first_time, double step_dt) {
    EH_HIP(c, hipSetDevice(c->device));
    EH_TRY(flush_joint_redefs(c));
    EH_TRY(flush_exclusions(c));
    c->timings = edynhip_timings{};
    c->timer.recorded = 0;
    if (c->events) EH_HIP(c, hipMemsetAsync(c->event_count, 0, sizeof(uint32_t), c->stream));   // the events of THIS call
    c->evp.state = c->evp.max ? 2 : 0;
    bool ran = false;
    for (uint32_t i = 0; i < nsteps; ++i) {
        c->evp.now = c->evp.max != 0 && i + 1 == nsteps;
        // island_manager::update runs put_islands_to_sleep() against the PREVIOUS step's stamp and only then takes the new one
        // (island_manager.cpp:533-539): the kernels read c->sim_clock, which is advanced after the step
        const double stamp = timed ? first_time + step_dt * (double)i : c->sim_clock + (double)c->cfg.fixed_dt;
        // every procedural body asleep and nothing edited since: the step changes nothing (each stage excludes sleeping
        // entities), so it is not run at all - a world at rest costs no GPU time, as in the reference
        if (c->all_asleep) { ++c->step_index; c->sim_clock = stamp; continue; }
        const int rc = run_stages(c, EDYNHIP_STAGE_ALL);
        c->sim_clock = stamp;
        ran = true;
        if (rc != EDYNHIP_OK) { c->evp.now = false; return rc; }
    }
    c->evp.now = false;
    // a step before the last put every island to sleep and the last was skipped: the events of the steps that ran are
    // still to be handed over (state 2 stays "no step ran, nothing happened")
    if (c->evp.max != 0 && c->evp.state == 2 && ran) EH_TRY(enqueue_event_prefetch(c));
    return EDYNHIP_OK;
}
int edynhip_step(edynhip_ctx *c, uint32_t nsteps) {
    if (!c) return EDYNHIP_ERR_INVALID;
    return step_stamped(c, nsteps, false, 0, 0);
}
int edynhip_step_timed(edynhip_ctx *c, uint32_t nsteps, double first_step_time, double step_dt) {
    if (!c) return EDYNHIP_ERR_INVALID;
    return step_stamped(c, nsteps, true, first_step_time, step_dt);
}

int edynhip_debug_collide(edynhip_ctx *c, uint32_t n, const int32_t *shape_type, const float *shape_param, const float *pos,
                          const float *orn, float threshold, float *out_points, uint32_t *out_count) {
    if (!c || (n && (!shape_type || !shape_param || !pos || !orn || !out_points || !out_count))) return EDYNHIP_ERR_INVALID;
    EH_HIP(c, hipSetDevice(c->device));
    return debug_collide(c, n, shape_type, shape_param, pos, orn, threshold, out_points, out_count);
}

int edynhip_debug_paths(edynhip_ctx *c, uint64_t *mask) {
    if (!c || !mask) return EDYNHIP_ERR_INVALID;
    *mask = c->paths;
    return EDYNHIP_OK;
}
int edynhip_debug_relabel_steps(edynhip_ctx *c, uint64_t *full, uint64_t *incremental) {
    if (!c || !full || !incremental) return EDYNHIP_ERR_INVALID;
    *full = c->cc_full_steps;
    *incremental = c->cc_incremental_steps;
    return EDYNHIP_OK;
}

int edynhip_get_timings(edynhip_ctx *c, edynhip_timings *out) {
    if (!c || !out) return EDYNHIP_ERR_INVALID;
    resolve_timings(c);
    *out = c->timings;
    return EDYNHIP_OK;
}

int edynhip_get_stats(edynhip_ctx *c, edynhip_stats *out) {
    if (!c || !out) return EDYNHIP_ERR_INVALID;
    EH_HIP(c, hipSetDevice(c->device));
    EH_TRY(count_points(c));
    EH_HIP(c, hipMemcpyAsync(c->cnt_host, c->cnt, sizeof(Counters), hipMemcpyDeviceToHost, c->stream));
    EH_HIP(c, hipStreamSynchronize(c->stream));
    c->stats.num_bodies = c->b.n;
    c->stats.num_manifolds = c->num_manifolds;
    c->stats.num_points = c->cnt_host->num_points;
    c->stats.num_active_manifolds = c->cnt_host->num_active;
    c->stats.num_islands = c->cnt_host->num_islands;
    c->stats.num_colours = c->num_colours;
    for (uint32_t k = 0; k < kMaxColours; ++k) c->stats.colour_size[k] = k < c->num_colours ? c->colour_end[k] - c->colour_start[k] : 0;
    *out = c->stats;
    return EDYNHIP_OK;
}

}  // extern "C"
