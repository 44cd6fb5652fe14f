// Queries as tickets (edynhip_raycast_submit, edynhip_query_aabb_submit, edynhip_query_poll, edynhip_*_collect, edynhip_query_release):
// what edyn::raycast_async / query_aabb_async / query_aabb_of_interest_async need (include/edyn/collision/raycast.hpp:170-182,
// query_aabb.hpp:37-44, answered by the reference's worker in simulation_worker.cpp:600-692). A submit packs its inputs into the slot's
// pinned block, enqueues one copy of it to the device, the query kernels of raycast.hip / query_aabb.hip on the slot's own buffers, and
// a kernel that publishes the ticket's sequence number into pinned memory - the way k_publish_counters does (capi.hip) - and returns.
// Nothing here waits for the device on the steady path: a slot's buffers grow by synchronising (as qa_reserve does), and a slot whose
// previous ticket was released before it was done waits for that one before its pinned input block is packed again.
//   Results: the rays' records are stored by the trace kernel straight into the slot's pinned block (32 bytes per ray, coalesced);
// a box ticket's offsets, total and ids are written there by k_qt_export, which knows the total - no copy sized by the capacity.
//   The of-interest list (list 3 of a box): a marked pass over the bodies. A body is reported when it is dynamic, shaped and not
// removed and the box of its island - the islands category's own boxes, found through the label - passes the islands category's
// test. Waves stride pieces of the body range, ballot + prefix pack in ascending body index. Cost: two passes (count, fill) of
// ceil(bodies / 64) wave iterations per wanting box - each a chain of four dependent loads (flags, label, slot, island box) -
// spread over about 2^17 waves whatever the number of boxes; no member lists are kept, so nothing is rebuilt when the state moves on.
#include "ctx.hpp"
#include "dmath.hpp"
#include "query_tickets.hpp"
#include "raytree.hpp"
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>

namespace eh {
using namespace dm;

constexpr uint32_t kQtSat = 0xFFFFFFFFu;           // a saturated offset (query_aabb.hip kSat)
constexpr uint32_t kQtMaxBoxes = 1u << 28;         // 4 n + 1 offsets fit 32 bits

struct TicketSlot {
    GrowBuf dev;                          // the device block: the inputs' copy, the scratch, the ids
    PinnedBuf<uint8_t> in, out;           // pinned: the packed inputs; the results
    size_t in_cap = 0, out_cap = 0;
    uint32_t n = 0, capacity = 0;         // of the ticket that holds the slot
    uint32_t last_seq = 0;                // sequence number of the last ticket submitted in this slot (0: none yet)
};
struct QueryTickets {
    TicketTable table;
    TicketSlot slot[EDYNHIP_QUERY_TICKETS_MAX];
    PinnedBuf<uint32_t> seq;              // [EDYNHIP_QUERY_TICKETS_MAX] the sequence number each slot published last
};

void query_tickets_free(edynhip_ctx *c) {
    delete c->qt;   // (edynhip_destroy has synchronised the stream; the owners release the buffers)
    c->qt = nullptr;
}

static inline uint32_t nblocks(uint32_t n, uint32_t bs) { return (n + bs - 1) / bs; }
static inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// After everything the ticket enqueued: the results are in place (the kernels before this one have completed), publish the number.
__global__ void k_qt_publish(volatile uint32_t *seq, uint32_t value) {
    __threadfence_system();
    __hip_atomic_store((uint32_t *)seq, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// boxes_k[k][2 n]: the boxes of category k, NaN where box i does not want it (a NaN box passes none of the six comparisons)
__global__ void k_qt_expand(uint32_t n, const float4 *__restrict__ boxes, const uint8_t *__restrict__ want, float4 *__restrict__ boxes_k) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 mn = boxes[2 * (size_t)i], mx = boxes[2 * (size_t)i + 1];
    const float qn = __uint_as_float(0x7FC00000u);
    const float4 none = make_float4(qn, qn, qn, 0.0f);
    const uint32_t w = want[i];
    for (uint32_t k = 0; k < 3; ++k) {
        const bool on = (w >> k) & 1u;
        boxes_k[2 * ((size_t)k * n + i)] = on ? mn : none;
        boxes_k[2 * ((size_t)k * n + i) + 1] = on ? mx : none;
    }
}
// by category -> by box (list 4 i + 3 is counted by k_qi_count when a box wants it; `interest` == 0: nobody does)
__global__ void k_qt_gather(uint32_t n, const uint32_t *__restrict__ cnt_k, uint32_t *__restrict__ cnt4, uint32_t interest) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (uint32_t k = 0; k < 3; ++k) cnt4[4 * (size_t)i + k] = cnt_k[(size_t)k * n + i];
    if (!interest) cnt4[4 * (size_t)i + 3] = 0u;
}
// by box -> by category: where the fill kernels of category k find the offset of box i
__global__ void k_qt_scatter(uint32_t n, const uint32_t *__restrict__ off4, uint32_t *__restrict__ off_k) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (uint32_t k = 0; k < 3; ++k) off_k[(size_t)k * n + i] = off4[4 * (size_t)i + k];
}

struct QiArgs {
    IslandView v;
    const uint32_t *flags;
    uint32_t n_bodies;
};
// the islands category's own test (query_aabb.hip qa_walk) on the box of the body's island
DI bool qi_hit(const QiArgs &a, uint32_t b, f3 qmn, f3 qmx) {
    const uint32_t fl = a.flags[b];
    if ((fl & BF_KIND_MASK) != EDYNHIP_KIND_DYNAMIC || (fl & BF_REMOVED) || (fl & BF_SHAPE_MASK) == 0) return false;
    uint32_t l = a.v.label[b];
    if (l >= a.n_bodies) l = b;
    if (!a.v.flag[l]) return false;
    const uint32_t k = a.v.slot[l];
    return qa_overlap(qmn, qmx, qa_fat_min(a.v.imin[k]), qa_fat_max(a.v.imax[k]));
}
// The marked pass. The body range is cut into `chunks` pieces of `chunk_len` bodies (a multiple of 64) and one wave takes one
// (box, piece): a lone box still spreads over the device, and many boxes do not multiply the waves beyond what fills it
// (qi_chunks). First the members are counted per piece ...
__global__ void __launch_bounds__(64) k_qi_count(QiArgs a, uint32_t n, const float4 *__restrict__ boxes, const uint8_t *__restrict__ want, uint32_t chunks,
                                                 uint32_t chunk_len, uint32_t *__restrict__ ccnt) {
    const uint32_t box = blockIdx.x / chunks, ch = blockIdx.x % chunks, lane = threadIdx.x;
    if (box >= n) return;
    uint32_t total = 0;
    if (want[box] & EDYNHIP_WANT_OF_INTEREST) {   // (block-uniform)
        const f3 qmn = from4(boxes[2 * (size_t)box]), qmx = from4(boxes[2 * (size_t)box + 1]);
        const uint32_t begin = ch * chunk_len, end = min(a.n_bodies, begin + chunk_len);
        for (uint32_t base = begin; base < end; base += 64) {
            const uint32_t b = base + lane;
            const bool hit = b < end && qi_hit(a, b, qmn, qmx);
            total += (uint32_t)__popcll(__ballot(hit));
        }
    }
    if (lane == 0) ccnt[(size_t)box * chunks + ch] = total;
}
// ... then one lane per box adds its pieces up (list 4 i + 3 of the counts) and leaves each piece's start within the list ...
__global__ void k_qi_sum(uint32_t n, uint32_t chunks, uint32_t *__restrict__ ccnt, uint32_t *__restrict__ cnt4) {
    const uint32_t box = blockIdx.x * blockDim.x + threadIdx.x;
    if (box >= n) return;
    uint32_t run = 0;
    for (uint32_t ch = 0; ch < chunks; ++ch) {
        const uint32_t v = ccnt[(size_t)box * chunks + ch];
        ccnt[(size_t)box * chunks + ch] = run;
        run += v;   // (at most the body count: fits)
    }
    cnt4[4 * (size_t)box + 3] = run;
}
// ... and after the scan every piece writes its members at the list's offset + its start, in ascending body index (ballot + prefix;
// nothing at or beyond `capacity`)
__global__ void __launch_bounds__(64) k_qi_fill(QiArgs a, uint32_t n, const float4 *__restrict__ boxes, const uint8_t *__restrict__ want, uint32_t chunks,
                                                uint32_t chunk_len, const uint32_t *__restrict__ ccnt, const uint32_t *__restrict__ off4,
                                                uint32_t *__restrict__ ids, uint32_t capacity) {
    const uint32_t box = blockIdx.x / chunks, ch = blockIdx.x % chunks, lane = threadIdx.x;
    if (box >= n || !(want[box] & EDYNHIP_WANT_OF_INTEREST)) return;
    const uint32_t start = off4[4 * (size_t)box + 3];
    if (start == kQtSat || start >= capacity) return;
    const f3 qmn = from4(boxes[2 * (size_t)box]), qmx = from4(boxes[2 * (size_t)box + 1]);
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long pos = (unsigned long long)start + ccnt[(size_t)box * chunks + ch];
    const uint32_t begin = ch * chunk_len, end = min(a.n_bodies, begin + chunk_len);
    for (uint32_t base = begin; base < end; base += 64) {
        const uint32_t b = base + lane;
        const bool hit = b < end && qi_hit(a, b, qmn, qmx);
        const unsigned long long m = __ballot(hit);
        if (hit) {
            const unsigned long long at = pos + (unsigned long long)__popcll(m & below);
            if (at < capacity) ids[at] = b;
        }
        pos += (unsigned long long)__popcll(m);
    }
}
// pieces per box: about kQiWaves waves in all, no piece shorter than 64 bodies; n_boxes x chunks <= kQiWaves + n_boxes
constexpr uint32_t kQiWaves = 1u << 17;
static void qi_chunks(uint32_t n_boxes, uint32_t n_bodies, uint32_t *chunks, uint32_t *chunk_len) {
    const uint32_t want = std::max(1u, kQiWaves / std::max(n_boxes, 1u)), most = std::max(1u, (n_bodies + 63) / 64);
    const uint32_t c = std::min(want, most);
    const uint32_t len = ((std::max(n_bodies, 1u) + c - 1) / c + 63) / 64 * 64;
    *chunk_len = len;
    *chunks = std::max(1u, (n_bodies + len - 1) / len);
}
// The result block in pinned memory: [total 8 B | pad 8 B | offsets 4 n + 1 | ids]; the ids only when all of them fit.
__global__ void __launch_bounds__(256) k_qt_export(uint32_t n4p1, const uint32_t *__restrict__ off4, const unsigned long long *__restrict__ tot,
                                                   const uint32_t *__restrict__ ids, uint32_t capacity, unsigned long long *out_tot, uint32_t *out_off, uint32_t *out_ids) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    const unsigned long long total = *tot;
    if (i == 0) *out_tot = total;
    for (uint32_t k = i; k < n4p1; k += stride) out_off[k] = off4[k];
    if (total > capacity) return;
    for (uint32_t k = i; k < (uint32_t)total; k += stride) out_ids[k] = ids[k];
}

static int tickets_of(edynhip_ctx *c, const char *who) {
    if (c->world_shard) return set_error(c, EDYNHIP_ERR_UNSUPPORTED, (std::string(who) + ": a shard of a multi-device world has no ticketed queries").c_str());
    if (!c->qt) {
        c->qt = new QueryTickets();
        EH_HIP(c, c->qt->seq.alloc(EDYNHIP_QUERY_TICKETS_MAX));
        memset((uint32_t *)c->qt->seq, 0, EDYNHIP_QUERY_TICKETS_MAX * sizeof(uint32_t));
    }
    return EDYNHIP_OK;
}

// the sequence number `value` of slot s: spin on the pinned word; after 2 s a real synchronise (it surfaces a device fault)
static int wait_sequence(edynhip_ctx *c, int s, uint32_t value) {
    volatile uint32_t *seq = (uint32_t *)c->qt->seq + s;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0; *seq != value; ++spins) {
        __builtin_ia32_pause();
        if ((spins & 0xFFFFu) == 0xFFFFu && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
            EH_HIP(c, hipStreamSynchronize(c->stream));
            if (*seq != value) return set_error(c, EDYNHIP_ERR_INTERNAL, "query ticket: the published sequence number never arrived");
            break;
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return EDYNHIP_OK;
}

// The slot's blocks for this ticket. Growth synchronises first: work enqueued earlier may still use the old blocks. A slot that was
// released before its ticket was done is waited for, since the host is about to pack the pinned input block again.
static int slot_reserve(edynhip_ctx *c, int s, size_t in_bytes, size_t dev_bytes, size_t out_bytes) {
    TicketSlot &sl = c->qt->slot[s];
    if (sl.last_seq) EH_TRY(wait_sequence(c, s, sl.last_seq));
    if (in_bytes > sl.in_cap || out_bytes > sl.out_cap || dev_bytes > sl.dev.cap) EH_HIP(c, hipStreamSynchronize(c->stream));
    if (in_bytes > sl.in_cap) { sl.in_cap = 0; EH_HIP(c, sl.in.alloc(in_bytes)); sl.in_cap = in_bytes; }
    if (out_bytes > sl.out_cap) { sl.out_cap = 0; EH_HIP(c, sl.out.alloc(out_bytes)); sl.out_cap = out_bytes; }
    EH_HIP(c, sl.dev.grow(dev_bytes));
    return EDYNHIP_OK;
}
static int publish(edynhip_ctx *c, int s, uint64_t ticket) {
    TicketSlot &sl = c->qt->slot[s];
    const uint32_t value = ticket_sequence(ticket);
    hipLaunchKernelGGL(k_qt_publish, dim3(1), dim3(1), 0, c->stream, (volatile uint32_t *)((uint32_t *)c->qt->seq + s), value);
    EH_HIP(c, hipGetLastError());
    sl.last_seq = value;
    return EDYNHIP_OK;
}

static int submit_rays(edynhip_ctx *c, int s, uint64_t ticket, uint32_t n, const float *p0, const float *p1, const uint32_t *ign_off, const uint32_t *ign_ids, uint32_t flags) {
    const uint32_t m = ign_off ? ign_off[n] - ign_off[0] : 0u;
    // [p0 n float4 | p1 n float4 | offsets n + 1 | ids m], the same layout in the pinned block and on the device
    const size_t at_p1 = (size_t)n * sizeof(float4), at_off = 2 * at_p1, at_ids = at_off + align16(((size_t)n + 1) * sizeof(uint32_t));
    const size_t in_bytes = at_ids + align16((size_t)m * sizeof(uint32_t));
    EH_TRY(slot_reserve(c, s, std::max<size_t>(in_bytes, 16), std::max<size_t>(in_bytes, 16), std::max<size_t>((size_t)n * sizeof(edynhip_raycast_hit), 16)));
    TicketSlot &sl = c->qt->slot[s];
    sl.n = n; sl.capacity = 0;
    if (n) {
        uint8_t *in = sl.in;
        float4 *h0 = (float4 *)in, *h1 = (float4 *)(in + at_p1);
        for (uint32_t r = 0; r < n; ++r) {
            h0[r] = make_float4(p0[3 * (size_t)r], p0[3 * (size_t)r + 1], p0[3 * (size_t)r + 2], 0.0f);
            h1[r] = make_float4(p1[3 * (size_t)r], p1[3 * (size_t)r + 1], p1[3 * (size_t)r + 2], 0.0f);
        }
        if (ign_off) {   // (rebased: the ticket holds only the ids its rays name)
            uint32_t *ho = (uint32_t *)(in + at_off);
            for (uint32_t r = 0; r <= n; ++r) ho[r] = ign_off[r] - ign_off[0];
            if (m) memcpy(in + at_ids, ign_ids + ign_off[0], (size_t)m * sizeof(uint32_t));
        }
        uint8_t *d = (uint8_t *)sl.dev.h;
        EH_HIP(c, hipMemcpyAsync(d, in, ign_off ? in_bytes : at_off, hipMemcpyHostToDevice, c->stream));
        EH_TRY(ticket_trace(c, n, (const float4 *)d, (const float4 *)(d + at_p1), ign_off ? (const uint32_t *)(d + at_off) : nullptr,
                            (const uint32_t *)(d + at_ids), flags, (uint4 *)(uint8_t *)sl.out));
    }
    return publish(c, s, ticket);
}

// the pinned result block of a box ticket
static inline size_t box_out_off() { return 16; }
static inline size_t box_out_ids(uint32_t n) { return 16 + align16((4 * (size_t)n + 1) * sizeof(uint32_t)); }

static int submit_boxes(edynhip_ctx *c, int s, uint64_t ticket, uint32_t n, const float *boxes6, const uint8_t *want, uint32_t capacity, uint32_t flags) {
    // pinned input and its device copy: [boxes 2 n float4 | want n bytes]; then the device scratch
    const size_t at_want = 2 * (size_t)n * sizeof(float4), in_bytes = std::max<size_t>(at_want + align16(n), 16);
    size_t at = in_bytes;
    auto carve = [&](size_t bytes) { const size_t o = at; at += align16(bytes); return o; };
    const size_t at_boxes_k = carve(6 * (size_t)n * sizeof(float4));
    const size_t at_cnt_k = carve(3 * (size_t)n * 4), at_off_k = carve(3 * (size_t)n * 4), at_mid = carve(3 * (size_t)n * 4), at_big = carve(3 * (size_t)n * 4);
    const size_t at_cnt4 = carve(4 * (size_t)n * 4), at_off4 = carve((4 * (size_t)n + 1) * 4), at_ctl = carve(8 * 4), at_tot = carve(16);
    const size_t at_ccnt = carve(((size_t)kQiWaves + n) * 4);   // of-interest counts per (box, piece): qi_chunks
    const size_t at_ids = carve((size_t)capacity * 4);
    EH_TRY(slot_reserve(c, s, in_bytes, at, box_out_ids(n) + std::max<size_t>((size_t)capacity * 4, 16)));
    TicketSlot &sl = c->qt->slot[s];
    sl.n = n; sl.capacity = capacity;
    uint8_t *in = sl.in, *d = (uint8_t *)sl.dev.h, *out = sl.out;
    float4 *hb = (float4 *)in;
    for (uint32_t i = 0; i < n; ++i) {
        const float *b = boxes6 + 6 * (size_t)i;
        hb[2 * (size_t)i] = make_float4(b[0], b[1], b[2], 0.0f);
        hb[2 * (size_t)i + 1] = make_float4(b[3], b[4], b[5], 0.0f);
    }
    if (n) memcpy(in + at_want, want, n);
    QaTicket t;
    t.n = n; t.flags = flags; t.want_any = want_union(n, want); t.capacity = capacity;
    t.boxes_k = (const float4 *)(d + at_boxes_k);
    t.cnt_k = (uint32_t *)(d + at_cnt_k); t.off_k = (uint32_t *)(d + at_off_k); t.mid = (uint32_t *)(d + at_mid); t.big = (uint32_t *)(d + at_big);
    t.cnt4 = (uint32_t *)(d + at_cnt4); t.off4 = (uint32_t *)(d + at_off4); t.ctl = (uint32_t *)(d + at_ctl);
    t.tot = (unsigned long long *)(d + at_tot); t.ids = (uint32_t *)(d + at_ids);
    const float4 *boxes = (const float4 *)d;
    const uint8_t *dwant = d + at_want;
    const bool interest = (t.want_any & EDYNHIP_WANT_OF_INTEREST) != 0;
    if (n) {
        EH_HIP(c, hipMemcpyAsync(d, in, in_bytes, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_qt_expand, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, n, boxes, dwant, (float4 *)(d + at_boxes_k));
    }
    EH_TRY(ticket_query_count(c, t));
    QiArgs qi{};
    uint32_t chunks = 1, chunk_len = 64;
    uint32_t *ccnt = (uint32_t *)(d + at_ccnt);
    if (interest) { qi = QiArgs{ticket_island_view(c), c->b.flags, c->b.n}; qi_chunks(n, c->b.n, &chunks, &chunk_len); }
    if (n) {
        hipLaunchKernelGGL(k_qt_gather, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, n, t.cnt_k, t.cnt4, interest ? 1u : 0u);
        if (interest) {
            hipLaunchKernelGGL(k_qi_count, dim3(n * chunks), dim3(64), 0, c->stream, qi, n, boxes, dwant, chunks, chunk_len, ccnt);
            hipLaunchKernelGGL(k_qi_sum, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, n, chunks, ccnt, t.cnt4);
        }
    }
    EH_TRY(ticket_query_scan(c, t));
    if (n && capacity) {
        hipLaunchKernelGGL(k_qt_scatter, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, n, t.off4, t.off_k);
        EH_TRY(ticket_query_fill(c, t));
        if (interest) hipLaunchKernelGGL(k_qi_fill, dim3(n * chunks), dim3(64), 0, c->stream, qi, n, boxes, dwant, chunks, chunk_len, ccnt, t.off4, t.ids, capacity);
    }
    hipLaunchKernelGGL(k_qt_export, dim3((uint32_t)std::min<size_t>((4 * (size_t)n + 1 + capacity + 255) / 256, 1024)), dim3(256), 0, c->stream, 4 * n + 1, t.off4, t.tot, t.ids, capacity,
                       (unsigned long long *)out, (uint32_t *)(out + box_out_off()), (uint32_t *)(out + box_out_ids(n)));
    EH_HIP(c, hipGetLastError());
    return publish(c, s, ticket);
}

// A submit that failed half way: what it enqueued may still read the slot's pinned input block, and no sequence number will tell the
// next ticket of the slot when that is over - so wait for the stream before the slot goes back (error path only).
static int submit_failed(edynhip_ctx *c, uint64_t ticket, int rc) {
    (void)hipStreamSynchronize(c->stream);
    c->qt->table.release(ticket);
    return rc;
}

}  // namespace eh

using namespace eh;

int edynhip_raycast_submit(edynhip_ctx *c, uint32_t n, const float *p0, const float *p1, const uint32_t *ignore_offsets, const uint32_t *ignore_ids,
                           uint32_t flags, uint64_t *ticket) {
    if (!c || !ticket || (n && (!p0 || !p1))) return EDYNHIP_ERR_INVALID;
    if (!ray_flags_ok(flags)) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_raycast_submit: unknown flag bits");
    if (!ignore_offsets_ok(n, ignore_offsets, ignore_ids)) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_raycast_submit: ignore_offsets descend, or ids are missing");
    EH_TRY(tickets_of(c, "edynhip_raycast_submit"));
    EH_HIP(c, hipSetDevice(c->device));
    uint64_t id = 0;
    const int s = c->qt->table.acquire(TICKET_RAYS, &id);
    if (s < 0) return set_error(c, EDYNHIP_ERR_CAPACITY, "edynhip_raycast_submit: EDYNHIP_QUERY_TICKETS_MAX tickets are outstanding");
    const int rc = submit_rays(c, s, id, n, p0, p1, ignore_offsets, ignore_ids, flags);
    if (rc != EDYNHIP_OK) return submit_failed(c, id, rc);
    *ticket = id;
    return EDYNHIP_OK;
}

int edynhip_query_aabb_submit(edynhip_ctx *c, uint32_t n, const float *boxes6, const uint8_t *want, uint32_t ids_capacity, uint32_t flags, uint64_t *ticket) {
    if (!c || !ticket || (n && !boxes6)) return EDYNHIP_ERR_INVALID;
    if (!box_flags_ok(flags)) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_query_aabb_submit: unknown flag bits");
    if (!want_masks_ok(n, want)) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_query_aabb_submit: unknown want bits");
    if (n > kQtMaxBoxes) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_query_aabb_submit: too many boxes for 32-bit offsets");
    EH_TRY(tickets_of(c, "edynhip_query_aabb_submit"));
    EH_HIP(c, hipSetDevice(c->device));
    uint64_t id = 0;
    const int s = c->qt->table.acquire(TICKET_BOXES, &id);
    if (s < 0) return set_error(c, EDYNHIP_ERR_CAPACITY, "edynhip_query_aabb_submit: EDYNHIP_QUERY_TICKETS_MAX tickets are outstanding");
    const int rc = submit_boxes(c, s, id, n, boxes6, want, ids_capacity, flags);
    if (rc != EDYNHIP_OK) return submit_failed(c, id, rc);
    *ticket = id;
    return EDYNHIP_OK;
}

// the slot of an outstanding ticket of `kind` (0: either), or an error
static int slot_of(edynhip_ctx *c, uint64_t ticket, int kind, const char *who, int *s) {
    EH_TRY(tickets_of(c, who));
    *s = c->qt->table.find(ticket);
    if (*s < 0 || (kind && c->qt->table.slot[*s].kind != kind))
        return set_error(c, EDYNHIP_ERR_INVALID, (std::string(who) + ": not an outstanding ticket of this kind").c_str());
    return EDYNHIP_OK;
}

int edynhip_query_poll(edynhip_ctx *c, uint64_t ticket, int *done) {
    if (!c || !done) return EDYNHIP_ERR_INVALID;
    int s = -1;
    EH_TRY(slot_of(c, ticket, 0, "edynhip_query_poll", &s));
    *done = *(volatile uint32_t *)((uint32_t *)c->qt->seq + s) == ticket_sequence(ticket) ? 1 : 0;
    if (*done) std::atomic_thread_fence(std::memory_order_acquire);
    return EDYNHIP_OK;
}

int edynhip_raycast_collect(edynhip_ctx *c, uint64_t ticket, const edynhip_raycast_hit **hits, uint32_t *n) {
    if (!c || !hits || !n) return EDYNHIP_ERR_INVALID;
    int s = -1;
    EH_TRY(slot_of(c, ticket, TICKET_RAYS, "edynhip_raycast_collect", &s));
    EH_TRY(wait_sequence(c, s, ticket_sequence(ticket)));
    const TicketSlot &sl = c->qt->slot[s];
    *hits = (const edynhip_raycast_hit *)(uint8_t *)sl.out;
    *n = sl.n;
    return EDYNHIP_OK;
}

int edynhip_query_aabb_collect(edynhip_ctx *c, uint64_t ticket, edynhip_query_aabb_view *view) {
    if (!c || !view) return EDYNHIP_ERR_INVALID;
    int s = -1;
    EH_TRY(slot_of(c, ticket, TICKET_BOXES, "edynhip_query_aabb_collect", &s));
    EH_TRY(wait_sequence(c, s, ticket_sequence(ticket)));
    const TicketSlot &sl = c->qt->slot[s];
    const uint8_t *out = sl.out;
    view->n = sl.n;
    view->total = *(const uint64_t *)out;
    view->offsets = (const uint32_t *)(out + box_out_off());
    view->ids = nullptr;
    if (!lists_fit(view->total, sl.capacity))
        return set_error(c, EDYNHIP_ERR_CAPACITY, "edynhip_query_aabb_collect: capacity (offsets and total are valid: submit again with ids_capacity = total)");
    view->ids = (const uint32_t *)(out + box_out_ids(sl.n));
    return EDYNHIP_OK;
}

int edynhip_query_release(edynhip_ctx *c, uint64_t ticket) {
    if (!c) return EDYNHIP_ERR_INVALID;
    int s = -1;
    EH_TRY(slot_of(c, ticket, 0, "edynhip_query_release", &s));
    c->qt->table.release(ticket);
    return EDYNHIP_OK;
}
