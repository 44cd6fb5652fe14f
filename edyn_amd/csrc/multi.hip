// edynhip_world: ONE simulation over several GPUs of a node, behind the C-ABI (include/edynhip.h "Multi-GPU world").
//
// The reference's unit of parallelism is the island: solver.cpp:408-428 hands every island to a worker, islands share only
// non-procedural bodies, which a step never writes (comp/island.hpp:34-41). Here a shard = one GPU = one edynhip_ctx that owns the
// dynamic bodies of its islands plus a replica of every non-dynamic body and steps them with NO data-path exchange; after every
// step the shard's packed state goes to pinned host memory (N independent device-to-host copies - the registry write-back of
// SURVEY 8e; processes that own one GPU each gather with RCCL instead, edyn_amd/parallel.py) and lands in the world's global arrays.
//
// What keeps the partition valid: islands of different shards must not come within the manifold-creation margin of each other
// unnoticed. Each shard reduces, ON THE DEVICE, (a) per island the union of its bodies' AABBs (k_island_box_*), when a check is
// due, and (b) every step, how far any body's AABB has grown out of the AABB it had at the last check (k_shard_growth: one float
// per shard and step). The host sweeps the island boxes of all shards (sort along x) for cross-shard pairs and remembers the
// smallest gap; until twice the largest growth has eaten that gap no check is needed - a resting world checks every few hundred
// steps, a world in motion as often as its motion requires, and no contact between two shards can appear unseen. When a gap closes
// the islands are re-partitioned (welded where their boxes overlap, longest-processing-time-first over the summed weights) and
// every shard is rebuilt with what its islands carry: contact manifolds (warm-start impulses, colours), the joints' applied impulses
// and tracked angles, sleeping tags, collision exclusions, joint definitions, meshes.
//
// Body order inside a shard is ascending global index, so canonical pair keys, island labels (lowest index) and the colouring keep
// their relative order: a shard computes for its islands exactly what one context computes for the whole world
// (tests/cpp/multi.cpp: bit-equal through a forced and an approach-triggered re-partition).
//
// The rules that decide where things live - islands, partitioners, box sweep, welding, sticky targets, rebalance, placement, ownership -
// are plain C++ in world_rules.hpp; this file holds the world, its shards and everything that touches a device.
#include "ctx.hpp"
#include "world_query.hpp"
#include "world_rules.hpp"
#include <chrono>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <numeric>
#include <thread>
#include <unordered_map>

namespace eh {

// ------------------------------------------------------------------------------------------------ device pieces
__device__ __forceinline__ uint32_t ordered_bits(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__host__ __device__ inline float from_ordered_bits(uint32_t u) {
    const uint32_t v = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    float f; memcpy(&f, &v, 4); return f;
}
__device__ __forceinline__ bool shard_body_counts(uint32_t fl) { return (fl & BF_KIND_MASK) == EDYNHIP_KIND_DYNAMIC && !(fl & BF_REMOVED) && (fl & BF_SHAPE_MASK) != 0; }

// (b) above: the largest distance by which a dynamic body's AABB sticks out of the AABB recorded at the last check (0 = nothing moved out)
__global__ void k_shard_growth(uint32_t n, Bodies b, const float4 *__restrict__ amin0, const float4 *__restrict__ amax0, uint32_t *out_bits) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    float g = 0.0f;
    if (i < n && shard_body_counts(b.flags[i])) {
        const float4 lo = b.amin[i], hi = b.amax[i], lo0 = amin0[i], hi0 = amax0[i];
        g = fmaxf(fmaxf(fmaxf(lo0.x - lo.x, lo0.y - lo.y), lo0.z - lo.z), fmaxf(fmaxf(hi.x - hi0.x, hi.y - hi0.y), hi.z - hi0.z));
        g = fmaxf(g, 0.0f);
        if (!(g == g)) g = 3.0e38f;   // a NaN box: force a check (and let the check fail loudly)
    }
    for (int off = 32; off > 0; off >>= 1) g = fmaxf(g, __shfl_xor(g, off));
    if ((threadIdx.x & 63) == 0 && g > 0.0f) atomicMax(out_bits, __float_as_uint(g));   // non-negative floats order like their bits
}
__global__ void k_island_box_clear(uint32_t n, uint32_t *lo, uint32_t *hi) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 3 * n) { lo[i] = 0xFFFFFFFFu; hi[i] = 0u; }
}
// (a) above, also records the boxes the growth is measured against
__global__ void k_island_box_reduce(uint32_t n, Bodies b, uint32_t *lo, uint32_t *hi, float4 *amin0, float4 *amax0, bool per_body) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 mn = b.amin[i], mx = b.amax[i];
    amin0[i] = mn; amax0[i] = mx;
    if (!shard_body_counts(b.flags[i])) return;
    uint32_t l = per_body ? i : b.island[i];
    if (l >= n) l = i;
    atomicMin(&lo[3 * l], ordered_bits(mn.x)); atomicMin(&lo[3 * l + 1], ordered_bits(mn.y)); atomicMin(&lo[3 * l + 2], ordered_bits(mn.z));
    atomicMax(&hi[3 * l], ordered_bits(mx.x)); atomicMax(&hi[3 * l + 1], ordered_bits(mx.y)); atomicMax(&hi[3 * l + 2], ordered_bits(mx.z));
}
__global__ void k_island_box_compact(uint32_t n, const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, uint32_t *count, uint32_t *out_label, float *out_box) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n || lo[3 * l] == 0xFFFFFFFFu) return;   // no shaped dynamic body carries this label
    const uint32_t k = atomicAdd(count, 1u);
    out_label[k] = l;
    for (int d = 0; d < 3; ++d) { out_box[6 * k + d] = from_ordered_bits(lo[3 * l + d]); out_box[6 * k + 3 + d] = from_ordered_bits(hi[3 * l + d]); }
}

}  // namespace eh

using namespace eh;

// ------------------------------------------------------------------------------------------------ the world
namespace {

struct HostScene {   // deep copy of what the caller described, in global indices
    uint32_t n = 0;
    std::vector<int32_t> kind, shape_type;
    std::vector<float> pos, orn, linvel, angvel, mass, inertia, shape_param, friction, restitution, gravity, com;
    std::vector<uint8_t> has_inertia, sleeping_disabled;
    std::vector<uint64_t> group, mask;
    uint32_t nj = 0;
    std::vector<int32_t> jtype;
    std::vector<uint32_t> jbody;
    std::vector<float> jpivot, jaxis, jparams;
    std::vector<uint8_t> jalive;          // per joint: 0 once removed (edits of a running world: the index stays reserved)
    struct Def { uint32_t joint; bool generic; std::vector<float> fa, fb, p; };
    std::vector<Def> defs;
    std::vector<std::array<uint32_t, 2>> exclusions;
    struct Mesh { std::vector<float> v; std::vector<uint32_t> idx, faces; uint32_t flags; };
    std::vector<Mesh> meshes;
};

struct DevBuf { void *p = nullptr; size_t cap = 0; };   // a device buffer that only grows (the caller has set the device)
hipError_t dev_grow(DevBuf &b, size_t bytes) {
    if (bytes <= b.cap) return hipSuccess;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
    const hipError_t e = hipMalloc(&b.p, bytes);
    if (e == hipSuccess) b.cap = bytes;
    return e;
}
void dev_free(DevBuf &b) { if (b.p) (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }

struct Shard {
    edynhip_ctx *ctx = nullptr;
    int device = 0;
    std::vector<uint32_t> local_ids;      // local index -> global index (ascending)
    std::vector<int32_t> to_local;        // global index -> local index or -1
    std::vector<uint32_t> owned_local;    // local indices of the bodies whose state this shard contributes
    std::vector<uint32_t> local_joints;   // local joint index -> global joint index
    float *pack_dev = nullptr, *pack_host = nullptr;   // [n_local][13]
    // monitor scratch on the device: [0] growth bits, [1] island count | per label 3 lo + 3 hi ordered bits | out labels | out boxes | amin0 | amax0
    uint32_t *mon_dev = nullptr, *mon_host = nullptr;
    uint32_t cap = 0, joint_cap = 0, meshes_created = 0;
    uint32_t want_bodies = 0, want_joints = 0;   // head-room an edit asks of the next build_shard beyond what the scene holds now
    int rc = EDYNHIP_OK;
    std::string err;
    uint64_t paths_gone = 0;              // edynhip_debug_paths of the contexts this shard had before (free_shard)
    // collected for a re-partition
    std::vector<uint32_t> labels; std::vector<float> aabb; std::vector<edynhip_manifold> manifolds; std::vector<float> imp24, imp10; std::vector<uint8_t> asleep;
    std::vector<uint32_t> sleep_label; std::vector<double> sleep_since; double sleep_clock = 0;
    // queries (edynhip_world_raycast / edynhip_world_query_aabb). Per context, [cap]: local_ids on the device, the bit per local body this
    // shard answers for, island labels carried through a re-partition. Scratch: the queries and the local results of a shard that is not on
    // the home device, the hit lists of any shard; the last count pass (the context's buffers) and its 64-bit total (pinned).
    uint32_t *ids_dev = nullptr, *ans_dev = nullptr, *qisl_dev = nullptr;
    DevBuf q_in, q_out, q_ids;
    std::vector<uint32_t> q_ignore;
    const void *q_boxes = nullptr;
    const uint32_t *q_cnt = nullptr, *q_off = nullptr;
    unsigned long long *q_tot = nullptr;
    // contact events (EDYNHIP_FLAG_CONTACT_EVENTS only): the last step's event count, fetched with the state (pinned), and how many of them
    // the shard holds; the step's events in global indices (device, [event_cap]); the point ids of `manifolds` as [m][4], device and host
    uint32_t *ev_cnt_host = nullptr, ev_held = 0;
    DevBuf ev_out, pid_buf;
    std::vector<uint64_t> pids;
    // record hand-over (edynhip_world_snapshot_records): per pinned slot the event that completes this shard's pack, and whether one is out
    hipEvent_t rec_ev[2] = {nullptr, nullptr};
    bool rec_pending[2] = {false, false};
};

class Pool {   // one persistent host thread per shard (a context is single-threaded; its step spins on its own counters)
public:
    Pool(uint32_t n, bool serial) : n_(n), serial_(serial) {   // (serial: developer knob EDYNHIP_WORLD_SERIAL=1, every shard on the caller's thread)
        if (!serial_) for (uint32_t r = 0; r < n; ++r) threads_.emplace_back([this, r] { loop(r); });
    }
    ~Pool() {
        { std::lock_guard<std::mutex> g(m_); stop_ = true; ++gen_; }
        cv_.notify_all();
        for (auto &t : threads_) t.join();
    }
    bool run(const std::function<void(uint32_t)> &fn) {   // true: several shards, one after the other on the caller's thread
        if (n_ == 1) { fn(0); return false; }
        if (serial_) { for (uint32_t r = 0; r < n_; ++r) fn(r); return true; }
        { std::lock_guard<std::mutex> g(m_); fn_ = &fn; pending_ = n_; ++gen_; }
        cv_.notify_all();
        std::unique_lock<std::mutex> l(m_);
        done_.wait(l, [this] { return pending_ == 0; });
        return false;
    }
private:
    void loop(uint32_t r) {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(uint32_t)> *fn;
            {
                std::unique_lock<std::mutex> l(m_);
                cv_.wait(l, [&] { return gen_ != seen; });
                seen = gen_;
                if (stop_) return;
                fn = fn_;
            }
            (*fn)(r);
            { std::lock_guard<std::mutex> g(m_); if (--pending_ == 0) done_.notify_one(); }
        }
    }
    uint32_t n_;
    bool serial_;
    std::vector<std::thread> threads_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(uint32_t)> *fn_ = nullptr;
    uint32_t pending_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
};


}  // namespace

struct edynhip_world {
    edynhip_config cfg{};
    eh::Knobs knobs{};   // read when the world is created (world_serial, world_trace; every shard context reads its own)
    std::vector<int> devices;
    std::vector<Shard> shards;
    std::unique_ptr<Pool> pool;
    HostScene scene;
    std::vector<int32_t> rank_of;
    std::vector<float> pos, orn, linvel, angvel;   // the gathered state, global order
    // settings.should_collide_func on a world over several devices (broadphase.cpp:143-153): the user's predicate speaks GLOBAL body
    // indices; every shard's context asks it through a thunk that maps its local indices back (ShardFilter, one per shard, stable
    // across re-partitions). The shards step on their own host threads: the calls are serialised (the reference's sequential stepper
    // asks from one thread).
    edynhip_pair_filter filter = nullptr;
    void *filter_user = nullptr;
    std::mutex filter_mutex;
    struct ShardFilter { edynhip_world *w; uint32_t shard; };
    std::vector<ShardFilter> shard_filters;
    bool built = false;
    bool stepped = false;                          // stepped since the scene was last described (set_bodies): scene-description calls are refused then
    float budget = 0.0f;                           // how much two islands of different shards may still approach before a check is due
    edynhip_world_stats stats{};
    uint64_t paths = 0;                            // the world's own EDYNHIP_PATH_* bits (edynhip_world_debug_paths)
    std::string err;
    int fail(int code, const std::string &what) { err = what; return code; }
    // queries: the home device is devices[0]; a stream of the world's own there, the shards' answers side by side, the scan's scratch, and
    // the device copies of the host entry points' arrays
    hipStream_t qstream = nullptr;
    DevBuf h_hits, h_cnt, h_off, h_ids, h_scan, h_in, h_out, h_off_out, h_ids_out;
    unsigned long long *q_pin = nullptr;           // pinned: the 64-bit total of the last count
    std::vector<uint32_t> query_labels;            // island labels (global) of the state the shards were last rebuilt from
    std::vector<float4> q_stage;
    // contact events (EDYNHIP_FLAG_CONTACT_EVENTS only): the events of the last edynhip_world_step call, global indices, on the home device -
    // every step appends every shard's block -, whether a shard's own list overflowed in that call, and the steps since the scene was described
    DevBuf ev_list;
    uint32_t ev_n = 0, step_count = 0;
    bool ev_overflow = false;
    bool events_on() const { return (cfg.flags & EDYNHIP_FLAG_CONTACT_EVENTS) != 0; }
    // edits of a running world (edynhip_world_add_bodies ...): tombstones per global body, the settings last given to
    // edynhip_world_set_params (applied to every context built afterwards), and which path the edits took
    std::vector<uint8_t> removed;
    std::vector<uint32_t> pending_tombs;           // removed since the last step: still described as they were (scene_tombstones)
    bool params_set = false;
    edynhip_params params{};
    edynhip_world_edit_stats edit_stats{};
    bool is_removed(uint32_t g) const { return g < removed.size() && removed[g] != 0; }
    // record hand-over (edynhip_world_snapshot_records / _map): two pinned slots used alternately, each [records: body_cap x 96 B | events:
    // ev_cap x 24 B], allocated portable and mapped so that every shard's device stores its records into them; what the slot holds; the home
    // device's side stream and per slot the event that completes the copy of the event block; the events that OCCURRED in the last
    // edynhip_world_step call (the sum of the shards' own counts, also where a shard's list overflowed); every body removed so far.
    struct RecSlot {
        uint8_t *host = nullptr;
        uint32_t body_cap = 0, ev_cap = 0;
        uint32_t bodies = 0, step = 0, events = 0, total = 0, tombs = 0;
        bool ev_pending = false;
    };
    RecSlot rec[2];
    int rec_last = -1;
    hipStream_t rec_stream = nullptr;
    hipEvent_t rec_ev_done[2] = {nullptr, nullptr};
    uint64_t ev_occurred = 0;
    std::vector<uint32_t> tombs;
};

namespace {

int shard_error(edynhip_world *w) {
    for (uint32_t r = 0; r < w->shards.size(); ++r)
        if (w->shards[r].rc != EDYNHIP_OK) return w->fail(w->shards[r].rc, "shard " + std::to_string(r) + ": " + w->shards[r].err);
    return EDYNHIP_OK;
}
#define SH_TRY(s, expr) do { int r__ = (expr); if (r__ != EDYNHIP_OK) { (s).rc = r__; (s).err = (s).ctx ? edynhip_last_error((s).ctx) : edynhip_last_error(nullptr); return; } } while (0)
#define W_HIP(w, call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return (w)->fail(EDYNHIP_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); } while (0)
#define SH_HIP(s, call) do { hipError_t e__ = (call); if (e__ != hipSuccess) { (s).rc = EDYNHIP_ERR_HIP; (s).err = std::string(#call) + ": " + hipGetErrorString(e__); return; } } while (0)

void free_shard(Shard &s) {
    if (s.ctx) { (void)hipSetDevice(s.device); (void)edynhip_synchronize(s.ctx); }
    for (int k = 0; k < 2; ++k) {   // (a pack that was out has landed: the context's stream is idle)
        if (s.rec_ev[k]) (void)hipEventDestroy(s.rec_ev[k]);
        s.rec_ev[k] = nullptr; s.rec_pending[k] = false;
    }
    if (s.pack_dev) (void)hipFree(s.pack_dev);
    if (s.pack_host) (void)hipHostFree(s.pack_host);
    if (s.mon_dev) (void)hipFree(s.mon_dev);
    if (s.mon_host) (void)hipHostFree(s.mon_host);
    if (s.ids_dev) (void)hipFree(s.ids_dev);
    if (s.ans_dev) (void)hipFree(s.ans_dev);
    if (s.qisl_dev) (void)hipFree(s.qisl_dev);
    if (s.q_tot) (void)hipHostFree(s.q_tot);
    dev_free(s.q_in); dev_free(s.q_out); dev_free(s.q_ids);
    if (s.ev_cnt_host) (void)hipHostFree(s.ev_cnt_host);
    dev_free(s.ev_out); dev_free(s.pid_buf);
    s.ev_cnt_host = nullptr; s.ev_held = 0;
    if (s.ctx) { uint64_t m = 0; if (edynhip_debug_paths(s.ctx, &m) == EDYNHIP_OK) s.paths_gone |= m; }
    if (s.ctx) edynhip_destroy(s.ctx);
    s.ctx = nullptr; s.pack_dev = s.pack_host = nullptr; s.mon_dev = s.mon_host = nullptr;
    s.ids_dev = s.ans_dev = s.qisl_dev = nullptr; s.q_tot = nullptr; s.q_cnt = s.q_off = nullptr; s.q_boxes = nullptr;
    s.cap = s.joint_cap = s.meshes_created = 0;
}

template <typename T>
std::vector<T> take(const std::vector<T> &src, const std::vector<uint32_t> &ids, size_t width) {
    std::vector<T> out;
    if (src.empty()) return out;
    out.resize(ids.size() * width);
    for (size_t k = 0; k < ids.size(); ++k) std::memcpy(&out[k * width], &src[(size_t)ids[k] * width], width * sizeof(T));
    return out;
}

template <typename T> std::vector<T> rows_of(const T *src, const std::vector<uint32_t> &rows, size_t width) {
    std::vector<T> out;
    if (!src) return out;
    out.resize(rows.size() * width);
    for (size_t k = 0; k < rows.size(); ++k) std::memcpy(&out[k * width], src + (size_t)rows[k] * width, width * sizeof(T));
    return out;
}
template <typename T> const T *data_or_null(const std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }

// The rows `rows` of a body set as a body set of their own (what a shard's context is given): every array edynhip_bodies has, in one
// place - build_shard slices the scene with it, edynhip_world_add_bodies the caller's new bodies.
struct BodyRows {
    std::vector<int32_t> kind, shape_type;
    std::vector<float> pos, orn, linvel, angvel, mass, inertia, shape_param, friction, restitution, gravity, com;
    std::vector<uint8_t> has_inertia, sleeping_disabled;
    std::vector<uint64_t> group, mask;
    BodyRows(const edynhip_bodies &in, const std::vector<uint32_t> &rows) {
        const bool own_inertia = in.inertia && in.has_inertia;
        kind = rows_of(in.kind, rows, 1); shape_type = rows_of(in.shape_type, rows, 1);
        pos = rows_of(in.pos, rows, 3); orn = rows_of(in.orn, rows, 4); linvel = rows_of(in.linvel, rows, 3); angvel = rows_of(in.angvel, rows, 3);
        mass = rows_of(in.mass, rows, 1); shape_param = rows_of(in.shape_param, rows, 4); friction = rows_of(in.friction, rows, 1); restitution = rows_of(in.restitution, rows, 1);
        inertia = rows_of(own_inertia ? in.inertia : nullptr, rows, 9); has_inertia = rows_of(own_inertia ? in.has_inertia : nullptr, rows, 1);
        group = rows_of(in.group, rows, 1); mask = rows_of(in.mask, rows, 1); gravity = rows_of(in.gravity, rows, 3);
        sleeping_disabled = rows_of(in.sleeping_disabled, rows, 1); com = rows_of(in.center_of_mass, rows, 3);
    }
    edynhip_bodies view() const {
        edynhip_bodies b{};
        b.kind = kind.data(); b.pos = pos.data(); b.orn = orn.data(); b.linvel = linvel.data(); b.angvel = angvel.data(); b.mass = mass.data();
        b.inertia = data_or_null(inertia); b.has_inertia = data_or_null(has_inertia);
        b.shape_type = shape_type.data(); b.shape_param = shape_param.data(); b.friction = friction.data(); b.restitution = restitution.data();
        b.group = data_or_null(group); b.mask = data_or_null(mask); b.gravity = data_or_null(gravity);
        b.sleeping_disabled = data_or_null(sleeping_disabled); b.center_of_mass = data_or_null(com);
        return b;
    }
};

// layout of the monitor scratch (Shard::mon_dev, edynhip_get_island_boxes), in 32-bit words, for `cap` bodies:
//   [0] growth bits  [1] island count | per label 3 lo + 3 hi ordered bits | out labels | out boxes (6 floats) | pad | amin0 | amax0 (float4 each)
struct MonLayout {
    size_t lo, hi, out_label, out_box, amin0, amax0, words;
    explicit MonLayout(size_t cap) {
        lo = 2; hi = lo + 3 * cap; out_label = hi + 3 * cap; out_box = out_label + cap;
        amin0 = (out_box + 6 * cap + 3) & ~(size_t)3; amax0 = amin0 + 4 * cap; words = amax0 + 4 * cap;
    }
};

struct Carry {   // what travels with the islands through a re-partition (global indices)
    std::vector<edynhip_manifold> manifolds;   // canonical order
    std::vector<float> imp24, angle;           // per global joint
    std::vector<uint8_t> asleep;               // per global body
    std::vector<uint32_t> label;               // per global body: its island (global index of the island's lowest body) - with
    std::vector<double> since;                 // ... the islands' sleep timers by that label, and the clock they are measured on (ADVICE r04:
    double clock = 0;                          //     every re-partition used to restart every island's timer)
    bool any = false;
    // sticky re-partitions: the manifolds already sorted out per NEW shard (global indices, canonical order) - the bodies of a shard that
    // stay keep their relative order, so their manifolds are taken over in place and only the few that arrive are merged in; `manifolds`
    // above (one merged, sorted list of everything) is then empty. Consumed (moved from) by build_shard.
    mutable std::vector<std::vector<edynhip_manifold>> per_shard;
    // island boxes of the state the shards are built from, owners = the new partition: the approach check after the rebuild sweeps these
    // (thousands) instead of every body's box (hundreds of thousands)
    std::vector<IslandBox> island_boxes;
    std::vector<uint32_t> island;              // per global body: its island label at the re-partition (what the island query reports until the next step)
    // contact events: the ids of the carried points by body pair (body[0] << 32 | body[1], global) - a rebuilt shard puts them back over the
    // ids edynhip_set_manifolds issues, so a point keeps its id whichever shards it lives on
    std::unordered_map<uint64_t, std::array<uint64_t, 4>> point_ids;
};

int shard_filter_thunk(void *user, uint32_t body, uint32_t other) {
    auto *sf = static_cast<edynhip_world::ShardFilter *>(user);
    edynhip_world *w = sf->w;
    const Shard &s = w->shards[sf->shard];
    std::lock_guard<std::mutex> lock(w->filter_mutex);
    return w->filter(w->filter_user, s.local_ids[body], s.local_ids[other]);
}

// developer aid (EDYNHIP_WORLD_TRACE=1): wall time of the phases of a re-partition, to stderr
struct PhaseTrace {
    bool on; std::chrono::steady_clock::time_point t0; const char *what;
    PhaseTrace(const edynhip_world *w, const char *w_) : on(w->knobs.world_trace), t0(std::chrono::steady_clock::now()), what(w_) {}
    void mark(const char *phase) {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[edynhip_world] %s: %s %.2f ms\n", what, phase, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

// An edit's or a getter's work on the shards, on their threads: every shard starts with its error cleared; `work(s, r)` runs on the
// shards that `wants(s, r)` names, with the shard's device current. Returns the first shard's error.
template <typename Wants, typename Work>
int on_shards(edynhip_world *w, Wants &&wants, Work &&work) {
    w->pool->run([&](uint32_t r) {
        Shard &s = w->shards[r];
        s.rc = EDYNHIP_OK; s.err.clear();
        if (!wants(s, r)) return;
        SH_HIP(s, hipSetDevice(s.device));
        work(s, r);
    });
    return shard_error(w);
}

void refresh_bodies_per_shard(edynhip_world *w) {
    for (uint32_t r = 0; r < w->shards.size(); ++r) w->stats.bodies_per_shard[r < 16 ? r : 15] = (uint32_t)w->shards[r].owned_local.size();
}

// the three island-box kernels over the monitor scratch `d` of n bodies (k_island_box_*), behind a clear of the growth bits and the count
hipError_t launch_island_boxes(hipStream_t st, uint32_t n, const Bodies &b, uint32_t *d, const MonLayout &L, bool per_body) {
    const hipError_t e = hipMemsetAsync(d, 0, 2 * sizeof(uint32_t), st);
    hipLaunchKernelGGL(k_island_box_clear, dim3((3 * n + 255) / 256), dim3(256), 0, st, n, d + L.lo, d + L.hi);
    hipLaunchKernelGGL(k_island_box_reduce, dim3((n + 255) / 256), dim3(256), 0, st, n, b, d + L.lo, d + L.hi, (float4 *)(d + L.amin0), (float4 *)(d + L.amax0), per_body);
    hipLaunchKernelGGL(k_island_box_compact, dim3((n + 255) / 256), dim3(256), 0, st, n, d + L.lo, d + L.hi, d + 1, d + L.out_label, (float *)(d + L.out_box));
    return e;
}

// The world's query tables of shard r from local index l0 onwards (0: a shard just built; otherwise bodies [l0, nl) were appended to
// its context). Every body is answered by one shard - the bodies whose state this shard reports (shard 0: the replicated ones too):
// the global ids, the answer bits, and the island labels the island query reads until the context's first step. island (l0 = 0 only):
// per GLOBAL body the label the shard is built with, or nullptr = none; an appended body is an island of its own beside the labels
// the shard was built with.
void upload_query_tables(edynhip_world *w, uint32_t r, uint32_t l0, const std::vector<uint32_t> *island = nullptr) {
    Shard &s = w->shards[r];
    const uint32_t nl = (uint32_t)s.local_ids.size(), n = w->scene.n;
    std::vector<uint32_t> bits;
    if (r != 0) {
        bits.assign((size_t)nl / 32 + 1, 0u);
        for (uint32_t l : s.owned_local) bits[l >> 5] |= 1u << (l & 31u);
        SH_HIP(s, hipMemcpy(s.ans_dev, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (nl > l0) SH_HIP(s, hipMemcpy(s.ids_dev + l0, s.local_ids.data() + l0, (size_t)(nl - l0) * sizeof(uint32_t), hipMemcpyHostToDevice));
    const bool labels = l0 ? s.ctx->query_island != nullptr : island && nl;
    if (labels && nl > l0) {   // (an island lives on one shard: its label is local)
        std::vector<uint32_t> lab(nl - l0);
        for (uint32_t l = l0; l < nl; ++l) {
            const uint32_t g = s.local_ids[l], root = island ? (*island)[g] : g;
            const int32_t lr = w->rank_of[g] == (int32_t)r && root < n ? s.to_local[root] : -1;
            lab[l - l0] = lr >= 0 ? (uint32_t)lr : l;
        }
        SH_HIP(s, hipMemcpy(s.qisl_dev + l0, lab.data(), lab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    shard_set_answers(s.ctx, r != 0 ? s.ans_dev : nullptr, std::move(bits), labels ? s.qisl_dev : nullptr);
}

// (Re)builds shard r for the partition w->rank_of from the scene, the current global state and what the islands carry.
void build_shard(edynhip_world *w, uint32_t r, const Carry &carry, bool from_state) {
    Shard &s = w->shards[r];
    const HostScene &sc = w->scene;
    s.rc = EDYNHIP_OK; s.err.clear();
    PhaseTrace trace(w, "build_shard");
    SH_HIP(s, hipSetDevice(s.device));
    const uint32_t n = sc.n;
    s.local_ids.clear(); s.owned_local.clear();
    s.to_local.assign(n, -1);
    for (uint32_t i = 0; i < n; ++i)
        if (shard_holds_body(w->rank_of[i], r)) {
            s.to_local[i] = (int32_t)s.local_ids.size();
            if (shard_reports_body(w->rank_of[i], r)) s.owned_local.push_back((uint32_t)s.local_ids.size());
            s.local_ids.push_back(i);
        }
    const uint32_t nl = (uint32_t)s.local_ids.size();
    // joints whose bodies are here and of which this shard owns one (a joint to a replicated anchor lives on one shard)
    s.local_joints.clear();
    for (uint32_t g = 0; g < sc.nj; ++g) {
        if (!sc.jalive[g]) continue;   // removed on the running world: its index stays reserved, no context holds it any more
        const uint32_t a = sc.jbody[2 * g], b = sc.jbody[2 * g + 1];
        // a joint is an island edge: a partition that puts its two dynamic bodies on different shards is wrong - never drop it silently
        const int32_t home = joint_home(w->rank_of[a], w->rank_of[b]);
        if (home == -2) {
            s.rc = EDYNHIP_ERR_INTERNAL; s.err = "partition splits joint " + std::to_string(g) + " (bodies " + std::to_string(a) + ", " + std::to_string(b) + ") over two shards";
            return;
        }
        if (home == (int32_t)r) s.local_joints.push_back(g);
    }
    edynhip_config cfg = w->cfg;
    cfg.device = s.device;
    if (w->cfg.max_manifolds) cfg.max_manifolds = w->cfg.max_manifolds; else cfg.max_manifolds = 0;
    // A shard that is rebuilt keeps its context when the new body / joint set fits the old capacities: edynhip_set_bodies starts a new
    // world on an existing context (manifolds, joints, exclusions, sleep state, clocks - everything but the meshes, which are the scene's
    // and stay), and a context's ~100 device allocations - over a gigabyte for a 32k-body shard - are neither freed nor made again
    // (round 6: the frees and allocations were ~0.1 s of every re-partition). A context that is too small is replaced with head-room.
    // (an edit that did not fit asks for room beyond the scene as it stands: want_bodies / want_joints)
    const uint32_t need_b = nl + s.want_bodies, need_j = (uint32_t)s.local_joints.size() + s.want_joints;
    s.want_bodies = s.want_joints = 0;
    const bool reuse = s.ctx != nullptr && need_b <= s.cap && need_j <= s.joint_cap && (uint32_t)sc.meshes.size() == s.meshes_created;
    if (!reuse) {
        free_shard(s);
        trace.mark("free the old context");
        cfg.max_bodies = std::max<uint32_t>(need_b + need_b / 4 + 64, 64);
        cfg.max_joints = std::max<uint32_t>(need_j + need_j / 4 + 16, 16);
        int status = 0;
        s.ctx = edynhip_create(&cfg, &status);
        if (!s.ctx) { s.rc = status; s.err = edynhip_last_error(nullptr); return; }
        s.ctx->world_shard = true;   // (the public queries refuse a shard: it holds part of a world, which answers through edynhip_world_raycast / _query_aabb)
        s.cap = cfg.max_bodies; s.joint_cap = cfg.max_joints;
        trace.mark("edynhip_create");
        for (const HostScene::Mesh &m : sc.meshes) {
            uint32_t id = 0;
            SH_TRY(s, edynhip_create_convex_mesh(s.ctx, (uint32_t)m.v.size() / 3, m.v.data(), (uint32_t)m.idx.size(), m.idx.data(), (uint32_t)m.faces.size() / 2, m.faces.data(), m.flags, &id));
        }
        s.meshes_created = (uint32_t)sc.meshes.size();
    } else {
        SH_TRY(s, edynhip_synchronize(s.ctx));
    }
    if (w->params_set) SH_TRY(s, edynhip_set_params(s.ctx, &w->params));   // (gravity equals cfg.gravity: only the settings a config does not carry)
    if (w->events_on()) {
        // World point ids: (world step of creation + 1) << 32 | shard << 28 | manifold index << 2 | slot. The context counts the world's steps
        // (its own step_index restarts with edynhip_set_bodies below) and tags the ids it issues, so events and ids are in world terms natively.
        if (r >= kEventTagShards || s.ctx->m[0].cap > (1u << (kEventTagShift - 2))) {
            s.rc = EDYNHIP_ERR_CAPACITY; s.err = "contact events on a multi-device world: at most 16 shards of at most 2^26 manifolds each";
            return;
        }
        s.ctx->event_step_base = w->step_count; s.ctx->event_id_tag = r << kEventTagShift;
        if (!s.ev_cnt_host) SH_HIP(s, hipHostMalloc((void **)&s.ev_cnt_host, sizeof(uint32_t), hipHostMallocDefault));
        *s.ev_cnt_host = 0; s.ev_held = 0;
        SH_HIP(s, dev_grow(s.ev_out, (size_t)std::max<uint32_t>(s.ctx->event_cap, 1) * sizeof(ContactEvent)));
    }
    // bodies: the scene's definitions with the CURRENT state
    const std::vector<float> &P = from_state ? w->pos : sc.pos, &Q = from_state ? w->orn : sc.orn, &V = from_state ? w->linvel : sc.linvel, &W = from_state ? w->angvel : sc.angvel;
    edynhip_bodies whole{};
    whole.kind = sc.kind.data(); whole.pos = P.data(); whole.orn = Q.data(); whole.linvel = V.data(); whole.angvel = W.data(); whole.mass = sc.mass.data();
    whole.inertia = data_or_null(sc.inertia); whole.has_inertia = data_or_null(sc.has_inertia);
    whole.shape_type = sc.shape_type.data(); whole.shape_param = sc.shape_param.data(); whole.friction = sc.friction.data(); whole.restitution = sc.restitution.data();
    whole.group = data_or_null(sc.group); whole.mask = data_or_null(sc.mask); whole.gravity = data_or_null(sc.gravity);
    whole.sleeping_disabled = data_or_null(sc.sleeping_disabled); whole.center_of_mass = data_or_null(sc.com);
    const BodyRows mine(whole, s.local_ids);
    const edynhip_bodies b = mine.view();
    SH_TRY(s, edynhip_set_bodies(s.ctx, nl, &b));
    trace.mark("take + edynhip_set_bodies");
    if (from_state && !mine.com.empty()) {   // set_bodies read `pos` as the origin of bodies with an offset: put the centre-of-mass state back ...
        SH_TRY(s, edynhip_set_state(s.ctx, mine.pos.data(), mine.orn.data(), mine.linvel.data(), mine.angvel.data()));
        // ... and with it what set_bodies derived from the misread position: origins, AABBs (displaced by R com otherwise - the first
        // broadphase / narrowphase after a re-partition would place those shapes wrong) and world inertias. Before the sleep tags below:
        // the derivation skips sleeping bodies
        SH_TRY(s, edynhip_refresh_derived(s.ctx));
    }
    // joints, in local indices
    const uint32_t njl = (uint32_t)s.local_joints.size();
    if (njl) {
        auto jt = take(sc.jtype, s.local_joints, 1);
        auto jb = take(sc.jbody, s.local_joints, 2);
        for (uint32_t &x : jb) x = (uint32_t)s.to_local[x];
        auto jp = take(sc.jpivot, s.local_joints, 6), ja = take(sc.jaxis, s.local_joints, 6), jq = take(sc.jparams, s.local_joints, 10);
        edynhip_joints j{};
        j.type = jt.data(); j.body = jb.data(); j.pivot = jp.data(); j.axis = ja.empty() ? nullptr : ja.data(); j.params = jq.empty() ? nullptr : jq.data();
        SH_TRY(s, edynhip_set_joints(s.ctx, njl, &j));
        for (const HostScene::Def &d : sc.defs) {
            const auto it = std::lower_bound(s.local_joints.begin(), s.local_joints.end(), d.joint);
            if (it == s.local_joints.end() || *it != d.joint) continue;
            const uint32_t lj = (uint32_t)(it - s.local_joints.begin());
            if (d.generic) SH_TRY(s, edynhip_set_generic_definition(s.ctx, lj, d.fa.data(), d.fb.data(), d.p.data()));
            else SH_TRY(s, edynhip_set_joint_definition(s.ctx, lj, d.fa.data(), d.fb.data(), d.p.data()));
        }
    }
    for (const auto &e : sc.exclusions)
        if (shard_holds_exclusion(w->rank_of[e[0]], w->rank_of[e[1]], r))
            SH_TRY(s, edynhip_exclude_collision(s.ctx, (uint32_t)s.to_local[e[0]], (uint32_t)s.to_local[e[1]]));
    if (w->filter) SH_TRY(s, edynhip_set_pair_filter(s.ctx, &shard_filter_thunk, &w->shard_filters[r]));
    if (carry.any) {
        std::vector<edynhip_manifold> mine;
        if (!carry.per_shard.empty()) mine.swap(carry.per_shard[r]);
        else
            for (const edynhip_manifold &m : carry.manifolds)
                if (w->rank_of[m.body[0]] == (int32_t)r || w->rank_of[m.body[1]] == (int32_t)r) mine.push_back(m);
        std::vector<uint64_t> mine_ids;   // contact events: the carried points keep their ids
        if (w->events_on() && !mine.empty()) {
            mine_ids.resize(4 * mine.size());
            for (size_t k = 0; k < mine.size(); ++k) {
                const auto it = carry.point_ids.find(((uint64_t)mine[k].body[0] << 32) | mine[k].body[1]);
                if (it == carry.point_ids.end()) {
                    s.rc = EDYNHIP_ERR_INTERNAL; s.err = "a carried manifold (bodies " + std::to_string(mine[k].body[0]) + ", " + std::to_string(mine[k].body[1]) + ") has no point ids";
                    return;
                }
                std::memcpy(&mine_ids[4 * k], it->second.data(), 4 * sizeof(uint64_t));
            }
        }
        for (edynhip_manifold &m : mine) { m.body[0] = (uint32_t)s.to_local[m.body[0]]; m.body[1] = (uint32_t)s.to_local[m.body[1]]; }   // a monotone map: the canonical order is kept
        trace.mark("joints, exclusions, select carried manifolds");
        if (!mine.empty()) SH_TRY(s, edynhip_set_manifolds(s.ctx, mine.data(), (uint32_t)mine.size()));
        if (!mine_ids.empty()) {
            SH_HIP(s, dev_grow(s.pid_buf, mine_ids.size() * sizeof(uint64_t)));
            SH_HIP(s, hipMemcpyAsync(s.pid_buf.p, mine_ids.data(), mine_ids.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s.ctx->stream));
            SH_TRY(s, shard_inject_point_ids(s.ctx, (const uint64_t *)s.pid_buf.p, (uint32_t)mine.size()));
            SH_HIP(s, hipStreamSynchronize(s.ctx->stream));   // (mine_ids is read by the copy until here)
        }
        trace.mark("edynhip_set_manifolds");
        if (njl && !carry.imp24.empty()) {
            auto i24 = take(carry.imp24, s.local_joints, 24), ang = take(carry.angle, s.local_joints, 1);
            SH_TRY(s, edynhip_set_joint_warm_start(s.ctx, i24.data(), ang.data()));
        }
        if (!carry.asleep.empty() && std::any_of(carry.asleep.begin(), carry.asleep.end(), [](uint8_t a) { return a != 0; })) {
            auto as = take(carry.asleep, s.local_ids, 1);
            SH_TRY(s, edynhip_set_asleep(s.ctx, as.data()));
        }
        if (!carry.label.empty()) {   // the islands' sleep timers go on where they were (edynhip_set_sleep_timers), in local indices
            std::vector<uint32_t> lab(nl);
            std::vector<double> since(nl, -1.0);
            for (uint32_t l = 0; l < nl; ++l) {
                const uint32_t g = s.local_ids[l], root = carry.label[g];
                const int32_t lr = w->rank_of[g] == (int32_t)r && root < n ? s.to_local[root] : -1;   // an island lives on one shard: its root is local
                lab[l] = lr >= 0 ? (uint32_t)lr : l;
                if (lr >= 0 && root == g) since[l] = carry.since[g];
            }
            SH_TRY(s, edynhip_set_sleep_timers(s.ctx, lab.data(), since.data(), carry.clock));
        }
    }
    {   // bodies removed since the last step went up as they were described, with their manifolds: now the removal itself, as the old context took it
        std::vector<uint32_t> gone;
        for (uint32_t g : w->pending_tombs) if (s.to_local[g] >= 0) gone.push_back((uint32_t)s.to_local[g]);
        if (!gone.empty()) SH_TRY(s, edynhip_remove_bodies(s.ctx, (uint32_t)gone.size(), gone.data()));
    }
    // gather and monitor buffers (sized by the context's capacity: they live as long as the context does)
    const size_t words = MonLayout(s.cap).words;
    if (!s.pack_dev) {
        SH_HIP(s, hipMalloc((void **)&s.pack_dev, (size_t)std::max<uint32_t>(s.cap, 1) * 13 * sizeof(float)));
        SH_HIP(s, hipHostMalloc((void **)&s.pack_host, (size_t)std::max<uint32_t>(s.cap, 1) * 13 * sizeof(float), hipHostMallocDefault));
        SH_HIP(s, hipMalloc((void **)&s.mon_dev, words * sizeof(uint32_t)));
        SH_HIP(s, hipHostMalloc((void **)&s.mon_host, (2 + 7 * (size_t)s.cap) * sizeof(uint32_t), hipHostMallocDefault));
        SH_HIP(s, hipMalloc((void **)&s.ids_dev, (size_t)std::max<uint32_t>(s.cap, 1) * sizeof(uint32_t)));
        SH_HIP(s, hipMalloc((void **)&s.ans_dev, ((size_t)s.cap / 32 + 1) * sizeof(uint32_t)));
        SH_HIP(s, hipMalloc((void **)&s.qisl_dev, (size_t)std::max<uint32_t>(s.cap, 1) * sizeof(uint32_t)));
        SH_HIP(s, hipHostMalloc((void **)&s.q_tot, sizeof(unsigned long long), hipHostMallocDefault));
    }
    SH_HIP(s, hipMemset(s.mon_dev, 0, words * sizeof(uint32_t)));
    // queries: every body is answered by one shard - the bodies whose state this shard reports (shard 0: the replicated ones too)
    upload_query_tables(w, r, 0, carry.any && carry.island.size() == n ? &carry.island : nullptr);
    if (s.rc != EDYNHIP_OK) return;
    trace.mark("warm start, sleep state, gather / monitor buffers");
}

// the shard's state into the world's global arrays (its own bodies; shard 0: also the replicated ones)
void scatter_state(edynhip_world *w, Shard &s) {
    for (uint32_t l : s.owned_local) {
        const float *row = s.pack_host + 13 * (size_t)l;
        const uint32_t g = s.local_ids[l];
        std::memcpy(&w->pos[3 * (size_t)g], row, 12); std::memcpy(&w->orn[4 * (size_t)g], row + 3, 16);
        std::memcpy(&w->linvel[3 * (size_t)g], row + 7, 12); std::memcpy(&w->angvel[3 * (size_t)g], row + 10, 12);
    }
}

void gather_shard(edynhip_world *w, uint32_t r, bool with_growth) {
    Shard &s = w->shards[r];
    if (s.rc != EDYNHIP_OK) return;
    const uint32_t nl = (uint32_t)s.local_ids.size();
    if (nl == 0) return;
    SH_HIP(s, hipSetDevice(s.device));
    hipStream_t st = s.ctx->stream;
    const MonLayout L(s.cap);
    if (with_growth)
        hipLaunchKernelGGL(k_shard_growth, dim3((nl + 255) / 256), dim3(256), 0, st, nl, s.ctx->b, (const float4 *)(s.mon_dev + L.amin0),
                           (const float4 *)(s.mon_dev + L.amax0), s.mon_dev);
    SH_TRY(s, edynhip_pack_state_device(s.ctx, s.pack_dev, 0, nl));
    SH_HIP(s, hipMemcpyAsync(s.pack_host, s.pack_dev, (size_t)nl * 13 * sizeof(float), hipMemcpyDeviceToHost, st));
    SH_HIP(s, hipMemcpyAsync(s.mon_host, s.mon_dev, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    const bool events = with_growth && s.ctx->events && s.ev_cnt_host;   // (with_growth: after a step)
    if (events) SH_HIP(s, hipMemcpyAsync(s.ev_cnt_host, s.ctx->event_count, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SH_HIP(s, hipStreamSynchronize(st));
    scatter_state(w, s);
    if (events) {   // the step's events in global indices, enqueued behind the step: the world appends the block to its list (append_events)
        s.ev_held = std::min(*s.ev_cnt_host, s.ctx->event_cap);
        SH_TRY(s, shard_translate_events(s.ctx, s.ev_held, s.ids_dev, nl, s.ev_out.p));
    }
}

// After a step of every shard: the shards' translated blocks go to the end of the world's list on the home device, device to device, each
// on its shard's stream (behind the translation; the next step of that shard queues up behind the copy). The offsets follow from the
// counts the shards fetched with their state.
int append_events(edynhip_world *w) {
    size_t total = 0;
    for (Shard &s : w->shards) {
        if (s.local_ids.empty() || !s.ctx || !s.ev_cnt_host) { s.ev_held = 0; continue; }
        if (*s.ev_cnt_host > s.ctx->event_cap) w->ev_overflow = true;
        w->ev_occurred += *s.ev_cnt_host;
        total += s.ev_held;
    }
    if (total == 0) return EDYNHIP_OK;
    const int home = w->devices[0];
    const size_t need = ((size_t)w->ev_n + total) * sizeof(ContactEvent);
    if ((size_t)w->ev_n + total > 0xFFFFFFFFull) return w->fail(EDYNHIP_ERR_CAPACITY, "edynhip_world_step: more than 2^32 - 1 contact events in one call");
    if (need > w->ev_list.cap) {   // grow and keep what the earlier steps of this call appended (copies of theirs may still be in flight)
        for (Shard &s : w->shards) if (s.ctx) { W_HIP(w, hipSetDevice(s.device)); W_HIP(w, hipStreamSynchronize(s.ctx->stream)); }
        W_HIP(w, hipSetDevice(home));
        DevBuf bigger;
        W_HIP(w, dev_grow(bigger, std::max(std::max(need, 2 * w->ev_list.cap), (size_t)4096 * sizeof(ContactEvent))));
        if (w->ev_n) {
            const hipError_t e = hipMemcpy(bigger.p, w->ev_list.p, (size_t)w->ev_n * sizeof(ContactEvent), hipMemcpyDeviceToDevice);
            if (e != hipSuccess || hipDeviceSynchronize() != hipSuccess) { dev_free(bigger); return w->fail(EDYNHIP_ERR_HIP, "edynhip_world_step: growing the event list"); }
        }
        dev_free(w->ev_list);
        w->ev_list = bigger;
    }
    size_t at = w->ev_n;
    for (Shard &s : w->shards) {
        if (s.ev_held == 0) continue;
        uint8_t *dst = (uint8_t *)w->ev_list.p + at * sizeof(ContactEvent);
        const size_t bytes = (size_t)s.ev_held * sizeof(ContactEvent);
        W_HIP(w, hipSetDevice(s.device));
        if (s.device == home) W_HIP(w, hipMemcpyAsync(dst, s.ev_out.p, bytes, hipMemcpyDeviceToDevice, s.ctx->stream));
        else W_HIP(w, hipMemcpyPeerAsync(dst, home, s.ev_out.p, s.device, bytes, s.ctx->stream));
        at += s.ev_held;
        s.ev_held = 0;
    }
    w->ev_n = (uint32_t)at;
    return EDYNHIP_OK;
}

// island boxes of shard r, reduced on its device; also records the AABBs the growth is measured against and clears the growth.
// per_body: every body is its own "island" (right after a shard was built its device labels are not computed yet; body boxes are
// the exact criterion anyway - island boxes are the cheaper, more conservative aggregate).
void island_boxes_shard(edynhip_world *w, uint32_t r, bool per_body) {
    Shard &s = w->shards[r];
    if (s.rc != EDYNHIP_OK) return;
    const uint32_t nl = (uint32_t)s.local_ids.size();
    s.mon_host[1] = 0;
    if (nl == 0) return;
    SH_HIP(s, hipSetDevice(s.device));
    hipStream_t st = s.ctx->stream;
    const MonLayout L(s.cap);
    uint32_t *d = s.mon_dev;
    SH_HIP(s, launch_island_boxes(st, nl, s.ctx->b, d, L, per_body));
    SH_HIP(s, hipMemcpyAsync(s.mon_host, d, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SH_HIP(s, hipStreamSynchronize(st));
    const uint32_t k = s.mon_host[1];
    if (k) {
        SH_HIP(s, hipMemcpyAsync(s.mon_host + 2, d + L.out_label, (size_t)k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SH_HIP(s, hipMemcpyAsync(s.mon_host + 2 + s.cap, d + L.out_box, (size_t)k * 6 * sizeof(float), hipMemcpyDeviceToHost, st));
        SH_HIP(s, hipStreamSynchronize(st));
    }
}

// The approach check on the device-reduced island boxes. Returns true when islands of different shards are within the creation
// margin of each other; otherwise w->budget = how far they may still approach.
int approach_check(edynhip_world *w, bool &close, bool per_body = false, const std::vector<IslandBox> *host_boxes = nullptr) {
    w->pool->run([w, per_body](uint32_t r) { island_boxes_shard(w, r, per_body); });
    EH_TRY(shard_error(w));
    std::vector<IslandBox> boxes;
    if (host_boxes) {   // the caller knows the islands of this state (a re-partition): their boxes, owned by the shard their bodies went to
        boxes = *host_boxes;
        for (IslandBox &b : boxes) b.owner = b.label < w->rank_of.size() ? w->rank_of[b.label] : -1;
    } else
    for (uint32_t r = 0; r < w->shards.size(); ++r) {
        Shard &s = w->shards[r];
        const uint32_t k = s.local_ids.empty() ? 0 : s.mon_host[1];
        const float *bx = (const float *)(s.mon_host + 2 + s.cap);
        for (uint32_t q = 0; q < k; ++q) {
            const uint32_t lead = s.local_ids[s.mon_host[2 + q]];
            if (w->rank_of[lead] != (int32_t)r) continue;   // (cannot happen: replicated bodies are not dynamic)
            IslandBox b;
            for (int d = 0; d < 3; ++d) { b.lo[d] = bx[6 * q + d]; b.hi[d] = bx[6 * q + 3 + d]; }
            b.label = lead; b.owner = (int32_t)r;
            boxes.push_back(b);
        }
    }
    ++w->stats.approach_checks;
    approach_verdict(boxes, close, w->budget);
    return EDYNHIP_OK;
}

// What the islands carry, per shard, in two parts: LIGHT - island labels, AABBs, sleeping tags and timers (28-45 bytes per body: what a
// re-partition decides on) - and HEAVY - the manifolds with their warm-start impulses and the joints' applied impulses (336 bytes per
// manifold: only worth reading from the shards that are rebuilt).
void collect_shard(edynhip_world *w, uint32_t r, bool light, bool heavy) {
    Shard &s = w->shards[r];
    if (s.rc != EDYNHIP_OK) return;
    const uint32_t nl = (uint32_t)s.local_ids.size();
    if (light) { s.labels.assign(nl, 0); s.aabb.assign((size_t)nl * 6, 0.f); s.asleep.assign(nl, 0); }
    s.manifolds.clear(); s.imp24.clear(); s.imp10.clear(); s.pids.clear();
    if (nl == 0) return;
    SH_HIP(s, hipSetDevice(s.device));
    if (light) {
        SH_TRY(s, edynhip_get_derived(s.ctx, s.aabb.data(), nullptr, s.labels.data()));
        if (w->cfg.flags & EDYNHIP_FLAG_SLEEPING) {
            SH_TRY(s, edynhip_get_asleep(s.ctx, s.asleep.data()));
            s.sleep_label.assign(nl, 0); s.sleep_since.assign(nl, -1.0);
            SH_TRY(s, edynhip_get_sleep_timers(s.ctx, s.sleep_label.data(), s.sleep_since.data(), &s.sleep_clock));
        }
    }
    if (!heavy) return;
    uint32_t nm = 0;
    SH_TRY(s, edynhip_num_manifolds(s.ctx, &nm));
    s.manifolds.resize(nm);
    if (nm) SH_TRY(s, edynhip_get_manifolds(s.ctx, s.manifolds.data(), nm, &nm));
    s.manifolds.resize(nm);
    if (nm && s.ctx->events) {   // contact events: the points' ids travel with the records, [m][4] in the same order
        s.pids.resize(4 * (size_t)nm);
        SH_HIP(s, dev_grow(s.pid_buf, s.pids.size() * sizeof(uint64_t)));
        SH_TRY(s, shard_gather_point_ids(s.ctx, (uint64_t *)s.pid_buf.p));
        SH_HIP(s, hipMemcpyAsync(s.pids.data(), s.pid_buf.p, s.pids.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s.ctx->stream));
        SH_HIP(s, hipStreamSynchronize(s.ctx->stream));
    }
    const uint32_t njl = (uint32_t)s.local_joints.size();
    if (njl) {
        s.imp24.assign((size_t)njl * 24, 0.f); s.imp10.assign((size_t)njl * 10, 0.f);
        SH_TRY(s, edynhip_get_joint_slot_impulses(s.ctx, s.imp24.data()));
        SH_TRY(s, edynhip_get_joint_impulses(s.ctx, s.imp10.data()));
    }
}

// gathers the manifolds of all shards, each once, global indices, canonical order; ids (or nullptr): their points' ids [m][4], in that order
void merge_manifolds(edynhip_world *w, std::vector<edynhip_manifold> &out, std::vector<uint64_t> *ids = nullptr) {
    out.clear();
    std::vector<const uint64_t *> from;   // per gathered record: its row of the shard's id table
    for (uint32_t r = 0; r < w->shards.size(); ++r) {
        Shard &s = w->shards[r];
        for (size_t k = 0; k < s.manifolds.size(); ++k) {
            edynhip_manifold m = s.manifolds[k];
            m.body[0] = s.local_ids[m.body[0]]; m.body[1] = s.local_ids[m.body[1]];
            const int32_t ra = w->rank_of[m.body[0]], rb = w->rank_of[m.body[1]];
            if (ra == (int32_t)r || (ra < 0 && rb == (int32_t)r)) { out.push_back(m); if (ids) from.push_back(s.pids.size() == 4 * s.manifolds.size() ? &s.pids[4 * k] : nullptr); }
        }
    }
    // canonical order: sort (key, position) pairs and move every 336-byte record once (a stable sort of the records themselves, with
    // the key recomputed in every comparison, was 0.15-0.3 s of a re-partition)
    std::vector<std::pair<uint64_t, uint32_t>> order(out.size());
    for (uint32_t k = 0; k < out.size(); ++k) order[k] = {canonical_key(w->scene.kind.data(), out[k].body[0], out[k].body[1]), k};
    std::sort(order.begin(), order.end());   // (ties keep their gathering order: the position is the second key)
    std::vector<edynhip_manifold> sorted(out.size());
    for (uint32_t k = 0; k < out.size(); ++k) sorted[k] = out[order[k].second];
    out.swap(sorted);
    if (ids) {
        ids->assign(4 * out.size(), 0);
        for (uint32_t k = 0; k < out.size(); ++k) if (const uint64_t *row = from[order[k].second]) std::memcpy(&(*ids)[4 * (size_t)k], row, 4 * sizeof(uint64_t));
    }
}

// contact events: the ids of a collected shard's points go with the re-partition, by global body pair (before s.manifolds is taken apart)
void carry_point_ids(const Shard &s, Carry &carry) {
    if (s.pids.size() != 4 * s.manifolds.size()) return;
    for (size_t k = 0; k < s.manifolds.size(); ++k) {
        const edynhip_manifold &m = s.manifolds[k];
        std::array<uint64_t, 4> row;
        std::memcpy(row.data(), &s.pids[4 * k], sizeof(row));
        carry.point_ids[((uint64_t)s.local_ids[m.body[0]] << 32) | s.local_ids[m.body[1]]] = row;
    }
}

// the applied impulses and tracked angles of a collected shard's joints go with the re-partition, by global joint
void carry_joint_impulses(const Shard &s, Carry &carry) {
    for (uint32_t lj = 0; lj < s.local_joints.size() && !s.imp24.empty(); ++lj) {
        const uint32_t g = s.local_joints[lj];
        std::memcpy(&carry.imp24[(size_t)g * 24], &s.imp24[(size_t)lj * 24], 24 * sizeof(float));
        carry.angle[g] = s.imp10[(size_t)lj * 10 + 9];
    }
}

// `only` (or nullptr = all): the shards to build; the others keep their contexts - their bodies, and therefore their local indices, are unchanged.
int rebuild(edynhip_world *w, const Carry &carry, bool from_state, const std::vector<uint8_t> *only = nullptr) {
    PhaseTrace trace(w, "rebuild");
    w->pool->run([&](uint32_t r) { if (!only || (*only)[r]) build_shard(w, r, carry, from_state); });
    EH_TRY(shard_error(w));
    trace.mark("build the shards (in parallel)");
    w->pool->run([w](uint32_t r) { gather_shard(w, r, false); });
    EH_TRY(shard_error(w));
    trace.mark("gather");
    refresh_bodies_per_shard(w);
    w->built = true;
    bool close = false;
    // a fresh partition keeps close islands together: the check sets the budget and records the reference boxes the growth is measured against
    const int rc_check = approach_check(w, close, true, carry.island_boxes.empty() ? nullptr : &carry.island_boxes);
    trace.mark(carry.island_boxes.empty() ? "approach check on body boxes" : "approach check (reference boxes on the devices, island boxes from the host)");
    return rc_check;
}

// Re-partition. FULL (edynhip_world_repartition, on request): everything the islands carry is read from every shard, the islands are
// balanced afresh (longest processing time first over their contact rows) and every shard is rebuilt. STICKY (the approach check found
// islands of different shards within the creation margin of each other - what a step does by itself): the islands stay where they are, a
// group of islands that has to live together moves to the shard that already holds most of it, and only the shards that gain or lose a
// body are read in full and rebuilt - the cost of an island meeting its neighbour follows the two shards involved, not the world
// (round 5: a collapsing 262 144-box scene re-partitioned 18 times in 160 steps at 8 s each when every meeting rebuilt all shards from an
// unrelated partition; scripts/multi_overhead.py).
// Edits of a running world come in with `edges` (body pairs that have to share a shard: a joint about to be made between two shards),
// `force` (shards to rebuild whatever moves: one that needs a larger context) and from_edit: no step may have run since a shard was
// built, so its device labels are not those of its islands - the labels it was built with stand in (the state has not moved since).
int repartition(edynhip_world *w, bool sticky, const std::vector<std::array<uint32_t, 2>> *edges = nullptr, const std::vector<uint8_t> *force = nullptr, bool from_edit = false) {
    const HostScene &sc = w->scene;
    const uint32_t n = sc.n, W = (uint32_t)w->shards.size();
    // A body removed since the last step is its own island by the device labels (k_mark_removed) while its manifolds still tie it to its
    // old one: only the full pass reads every manifold before it welds, so an edit that rebuilds shards in that state takes it (rare: a
    // removal and a rebuilding edit with no step in between)
    if (from_edit && !w->pending_tombs.empty()) sticky = false;
    PhaseTrace trace(w, sticky ? "sticky re-partition" : "full re-partition");
    w->pool->run([w, sticky](uint32_t r) { collect_shard(w, r, true, !sticky); });
    EH_TRY(shard_error(w));
    trace.mark("collect light state of every shard");
    std::vector<uint32_t> labels(n);
    std::iota(labels.begin(), labels.end(), 0u);
    std::vector<float> aabb((size_t)n * 6, 0.f);
    std::vector<double> weights(n, 1.0);
    Carry carry;
    carry.any = true;
    if (sc.nj) { carry.imp24.assign((size_t)sc.nj * 24, 0.f); carry.angle.assign(sc.nj, 0.f); }
    if (w->cfg.flags & EDYNHIP_FLAG_SLEEPING) { carry.asleep.assign(n, 0); carry.label.resize(n); std::iota(carry.label.begin(), carry.label.end(), 0u); carry.since.assign(n, -1.0); }
    for (uint32_t r = 0; r < W; ++r) {
        Shard &s = w->shards[r];
        if (!carry.label.empty() && !s.local_ids.empty()) carry.clock = std::max(carry.clock, s.sleep_clock);   // (every shard has taken the same steps)
        for (uint32_t l = 0; l < s.local_ids.size(); ++l) {
            const uint32_t g = s.local_ids[l];
            if (w->rank_of[g] != (int32_t)r) continue;
            labels[g] = s.local_ids[s.labels[l]];
            std::memcpy(&aabb[6 * (size_t)g], &s.aabb[6 * (size_t)l], 24);
            if (!carry.asleep.empty()) carry.asleep[g] = s.asleep[l];
            if (!carry.label.empty() && s.sleep_label[l] < s.local_ids.size()) {
                carry.label[g] = s.local_ids[s.sleep_label[l]];
                if (s.sleep_label[l] == l) carry.since[g] = s.sleep_since[l];
            }
        }
    }
    if (from_edit)
        for (uint32_t r = 0; r < W; ++r) {
            const Shard &s = w->shards[r];
            if (!s.ctx || s.ctx->step_index != 0) continue;
            for (uint32_t g : s.local_ids) if (w->rank_of[g] == (int32_t)r) labels[g] = w->query_labels.size() == n ? w->query_labels[g] : g;
        }
    // the island query's labels: a shard that has not stepped since it was rebuilt still answers with the labels it was rebuilt with
    carry.island = labels;
    if (w->query_labels.size() == n)
        for (uint32_t r = 0; r < W; ++r) {
            const Shard &s = w->shards[r];
            if (!s.ctx || !s.ctx->query_island || s.ctx->step_index != 0) continue;
            for (uint32_t g : s.local_ids) if (w->rank_of[g] == (int32_t)r) carry.island[g] = w->query_labels[g];
        }
    w->query_labels = carry.island;
    // what travels with the bodies of the shards read in full (all of them / later: the ones that change)
    auto take_heavy = [&](const std::vector<uint8_t> *only) {
        for (uint32_t r = 0; r < W; ++r) {
            Shard &s = w->shards[r];
            if (only && !(*only)[r]) { s.manifolds.clear(); continue; }
            carry_point_ids(s, carry);
            for (const edynhip_manifold &m : s.manifolds) {   // weight = 1 + the contact points the body takes part in (balance the rows)
                const uint32_t a = s.local_ids[m.body[0]], b = s.local_ids[m.body[1]];
                if (w->rank_of[a] == (int32_t)r) weights[a] += m.num_points;
                if (w->rank_of[b] == (int32_t)r) weights[b] += m.num_points;
            }
            carry_joint_impulses(s, carry);
        }
        merge_manifolds(w, carry.manifolds);
    };
    if (!sticky) take_heavy(nullptr);
    // The islands that must end up on one shard, welded (weld_islands): overlapping boxes, live joints, the edit's edges, carried
    // manifolds. (A sticky re-partition follows a step of every shard: labels are current, and it carries no manifold list.)
    std::vector<IslandBox> boxes;
    std::vector<EdgeSpan> tied;
    if (sc.nj) tied.push_back({sc.jbody.data(), 2 * sizeof(uint32_t), sc.nj, sc.jalive.data()});
    if (edges && !edges->empty()) tied.push_back({edges->data(), sizeof((*edges)[0]), edges->size(), nullptr});
    if (!carry.manifolds.empty()) tied.push_back({carry.manifolds[0].body, sizeof(edynhip_manifold), carry.manifolds.size(), nullptr});
    const std::vector<uint32_t> welded = weld_islands(n, labels.data(), sc.kind.data(), sc.shape_type.data(), aabb.data(), tied, boxes);
    ++w->stats.repartitions;
    trace.mark("island boxes, welding");
    if (!sticky) {
        w->rank_of.assign(n, -1);
        partition_islands_spatial(n, welded.data(), sc.kind.data(), weights.data(), aabb.data(), W, w->rank_of.data());
        return rebuild(w, carry, true);
    }
    const std::vector<int32_t> next = sticky_targets(n, welded.data(), sc.kind.data(), w->rank_of.data(), W);
    if (needs_rebalance(n, next.data(), W)) {   // this meeting takes the full, spatially balanced re-partition instead
        ++w->stats.rebalances; --w->stats.repartitions;   // (counted again by the full pass)
        return repartition(w, false, edges, nullptr, from_edit);
    }
    std::vector<uint8_t> changed(W, 0);
    for (uint32_t i = 0; i < n; ++i) if (next[i] != w->rank_of[i]) { changed[(uint32_t)next[i]] = 1; changed[(uint32_t)w->rank_of[i]] = 1; }
    if (force) for (uint32_t r = 0; r < W; ++r) if ((*force)[r]) changed[r] = 1;
    if (std::none_of(changed.begin(), changed.end(), [](uint8_t c) { return c != 0; })) {
        // nothing has to move (the close islands already share a shard): only the budget is taken again
        bool close = false;
        EH_TRY(approach_check(w, close, true));
        return EDYNHIP_OK;
    }
    trace.mark("sticky targets");
    w->pool->run([w, &changed](uint32_t r) { if (changed[r]) collect_shard(w, r, false, true); });
    EH_TRY(shard_error(w));
    trace.mark("collect manifolds / joint impulses of the changed shards");
    for (uint32_t r = 0; r < W; ++r) if (changed[r]) { carry_point_ids(w->shards[r], carry); carry_joint_impulses(w->shards[r], carry); }
    // Manifolds: a body that stays in its shard keeps its place among the others that stay (local indices ascend with the global ones), so
    // the manifolds that stay ARE in canonical order already; only those whose island moves are taken out, sorted among themselves and
    // merged into their new shard's list. No global sort, one copy per record at most (the merged, sorted list of every changed shard's
    // manifolds was 0.1-0.3 s of a re-partition).
    std::vector<std::vector<edynhip_manifold>> leaving(W);
    w->pool->run([&](uint32_t q) {
        if (!changed[q]) return;
        Shard &s = w->shards[q];
        size_t keep = 0;
        for (size_t k = 0; k < s.manifolds.size(); ++k) {
            edynhip_manifold m = s.manifolds[k];
            m.body[0] = s.local_ids[m.body[0]]; m.body[1] = s.local_ids[m.body[1]];
            const uint32_t dyn = w->rank_of[m.body[0]] >= 0 ? m.body[0] : m.body[1];
            if (w->rank_of[dyn] != (int32_t)q) continue;          // (not this shard's to report: cannot happen - a manifold lives where its dynamic body does)
            if (next[dyn] == (int32_t)q) s.manifolds[keep++] = m; else leaving[q].push_back(m);
        }
        s.manifolds.resize(keep);
    });
    std::vector<std::vector<edynhip_manifold>> incoming(W);
    for (uint32_t q = 0; q < W; ++q)
        for (const edynhip_manifold &m : leaving[q]) {
            const uint32_t dyn = w->rank_of[m.body[0]] >= 0 ? m.body[0] : m.body[1];
            incoming[(uint32_t)next[dyn]].push_back(m);
        }
    carry.per_shard.assign(W, {});
    w->pool->run([&](uint32_t r) {
        if (!changed[r]) return;
        Shard &s = w->shards[r];
        auto key_less = [&](const edynhip_manifold &x, const edynhip_manifold &y) { return canonical_key(sc.kind.data(), x.body[0], x.body[1]) < canonical_key(sc.kind.data(), y.body[0], y.body[1]); };
        if (incoming[r].empty()) { carry.per_shard[r].swap(s.manifolds); return; }
        std::sort(incoming[r].begin(), incoming[r].end(), key_less);
        carry.per_shard[r].resize(s.manifolds.size() + incoming[r].size());
        std::merge(s.manifolds.begin(), s.manifolds.end(), incoming[r].begin(), incoming[r].end(), carry.per_shard[r].begin(), key_less);
        s.manifolds.clear(); s.manifolds.shrink_to_fit();
    });
    trace.mark("sort out the carried manifolds per new shard");
    carry.island_boxes = boxes;
    w->rank_of = next;
    const int rc_rebuild = rebuild(w, carry, true, &changed);
    trace.mark("rebuild changed shards (+ gather, approach check)");
    return rc_rebuild;
}

// the scene's meshes as the island estimate reads them
MeshRadii scene_meshes(const HostScene &sc) {
    MeshRadii m;
    for (const HostScene::Mesh &mesh : sc.meshes) m.add(mesh.v.data(), mesh.v.size() / 3);
    return m;
}

int ensure_built(edynhip_world *w) {
    if (w->built) return EDYNHIP_OK;
    const HostScene &sc = w->scene;
    const uint32_t n = sc.n, W = (uint32_t)w->shards.size();
    if (n == 0) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world: no bodies");
    // The islands of the initial state, estimated on the HOST (round 6; until round 5 a probe context on devices[0] held the WHOLE scene and
    // ran broadphase, narrowphase and the island stage - a sharded scene had to fit one GPU, and a quarter-million-body probe cost seconds).
    // The partition only has to keep every true island on one shard: estimate_islands (bounding-sphere boxes within the creation margin, joints).
    std::vector<uint32_t> labels(n);
    std::vector<float> aabb0((size_t)n * 6, 0.f);
    MeshRadii meshes = scene_meshes(sc);
    estimate_islands({n, sc.kind.data(), sc.shape_type.data(), sc.shape_param.data(), sc.pos.data(), data_or_null(sc.com)}, meshes, sc.nj, sc.jbody.data(), sc.jalive.data(),
                     labels.data(), aabb0.data());
    w->rank_of.assign(n, -1);
    partition_islands_spatial(n, labels.data(), sc.kind.data(), nullptr, aabb0.data(), W, w->rank_of.data());
    w->pos = sc.pos; w->orn = sc.orn; w->linvel = sc.linvel; w->angvel = sc.angvel;
    Carry none;
    return rebuild(w, none, false);
}

// k bodies as they are described appended to the scene (onto an empty scene: edynhip_world_set_bodies)
void scene_append_bodies(edynhip_world *w, uint32_t k, const edynhip_bodies *in) {
    HostScene &sc = w->scene;
    const size_t n0 = sc.n;
    auto app = [&](auto &vec, const auto *src, size_t width) { vec.insert(vec.end(), src, src + (size_t)k * width); };
    // an optional array the scene or the new bodies lack reads as its default there
    auto opt = [&](auto &vec, const auto *src, size_t width, const auto *def_row) {
        if (vec.empty() && !src) return;
        if (vec.empty()) { vec.resize(n0 * width); for (size_t i = 0; i < vec.size(); ++i) vec[i] = def_row[i % width]; }
        if (src) vec.insert(vec.end(), src, src + (size_t)k * width);
        else for (size_t i = 0; i < (size_t)k * width; ++i) vec.push_back(def_row[i % width]);
    };
    app(sc.kind, in->kind, 1); app(sc.shape_type, in->shape_type, 1);
    app(sc.pos, in->pos, 3); app(sc.orn, in->orn, 4); app(sc.linvel, in->linvel, 3); app(sc.angvel, in->angvel, 3);
    app(sc.mass, in->mass, 1); app(sc.shape_param, in->shape_param, 4); app(sc.friction, in->friction, 1); app(sc.restitution, in->restitution, 1);
    const bool own_inertia = in->inertia && in->has_inertia;
    const float zeros[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const uint8_t zero8 = 0;
    const uint64_t all = ~0ull;
    opt(sc.inertia, own_inertia ? in->inertia : (const float *)nullptr, 9, zeros);
    opt(sc.has_inertia, own_inertia ? in->has_inertia : (const uint8_t *)nullptr, 1, &zero8);
    opt(sc.group, in->group, 1, &all); opt(sc.mask, in->mask, 1, &all);
    opt(sc.gravity, in->gravity, 3, w->cfg.gravity);
    opt(sc.sleeping_disabled, in->sleeping_disabled, 1, &zero8);
    opt(sc.com, in->center_of_mass, 3, zeros);
    sc.n += k;
    w->removed.resize(sc.n, 0);
    w->stats.num_bodies = sc.n;
}

// n joints appended to the scene, alive (onto a scene without joints: edynhip_world_set_joints)
void scene_append_joints(HostScene &sc, uint32_t n, const edynhip_joints *in) {
    if (n == 0) return;
    sc.jtype.insert(sc.jtype.end(), in->type, in->type + n); sc.jbody.insert(sc.jbody.end(), in->body, in->body + 2 * (size_t)n);
    sc.jpivot.insert(sc.jpivot.end(), in->pivot, in->pivot + 6 * (size_t)n);
    if (in->axis) sc.jaxis.insert(sc.jaxis.end(), in->axis, in->axis + 6 * (size_t)n); else sc.jaxis.resize(sc.jaxis.size() + 6 * (size_t)n, 0.f);
    if (in->params) sc.jparams.insert(sc.jparams.end(), in->params, in->params + 10 * (size_t)n); else sc.jparams.resize(sc.jparams.size() + 10 * (size_t)n, 0.f);
    sc.nj += n;
    sc.jalive.resize(sc.nj, 1);
}

HostScene::Def make_def(uint32_t joint, const float *frame_a9, const float *frame_b9, const float *params, bool generic) {
    HostScene::Def d;
    d.joint = joint; d.generic = generic;
    d.fa.assign(frame_a9, frame_a9 + 9); d.fb.assign(frame_b9, frame_b9 + 9); d.p.assign(params, params + (generic ? 60 : 16));
    return d;
}

// the removed bodies' manifolds are gone (a step dropped them, or no context ever held them): their slots are shapeless static bodies from here on
void finish_tombstones(edynhip_world *w) {
    for (uint32_t g : w->pending_tombs) { w->scene.kind[g] = EDYNHIP_KIND_STATIC; w->scene.shape_type[g] = EDYNHIP_SHAPE_NONE; }
    w->pending_tombs.clear();
}

}  // namespace

extern "C" {

int edynhip_partition_islands(uint32_t n, const uint32_t *labels, const int32_t *kind, const double *weights, uint32_t world_size, int32_t *rank_of) {
    if ((n && (!labels || !kind || !rank_of)) || world_size == 0) return EDYNHIP_ERR_INVALID;
    partition_islands(n, labels, kind, weights, world_size, rank_of);
    return EDYNHIP_OK;
}

int edynhip_island_boxes_overlap(uint32_t num_islands, const float *boxes6, const uint32_t *labels, const int32_t *owner, float margin, int any_owner,
                                 uint32_t *pairs, uint32_t capacity, uint32_t *num_pairs) {
    if ((num_islands && (!boxes6 || !labels || !owner)) || !num_pairs) return EDYNHIP_ERR_INVALID;
    std::vector<IslandBox> boxes(num_islands);
    for (uint32_t k = 0; k < num_islands; ++k) {
        for (int d = 0; d < 3; ++d) { boxes[k].lo[d] = boxes6[6 * k + d]; boxes[k].hi[d] = boxes6[6 * k + 3 + d]; }
        boxes[k].label = labels[k]; boxes[k].owner = owner[k];
    }
    std::vector<std::pair<uint32_t, uint32_t>> hits;
    sweep_boxes(boxes, margin, !any_owner, [&](const IslandBox &a, const IslandBox &b, float) { hits.emplace_back(std::min(a.label, b.label), std::max(a.label, b.label)); });
    std::sort(hits.begin(), hits.end());
    hits.erase(std::unique(hits.begin(), hits.end()), hits.end());
    *num_pairs = (uint32_t)hits.size();
    if (pairs) {
        if (capacity < hits.size()) return EDYNHIP_ERR_CAPACITY;
        for (size_t k = 0; k < hits.size(); ++k) { pairs[2 * k] = hits[k].first; pairs[2 * k + 1] = hits[k].second; }
    }
    return EDYNHIP_OK;
}

int edynhip_get_island_boxes(edynhip_ctx *c, uint32_t *labels, float *boxes6, uint32_t capacity, uint32_t *num_islands) {
    if (!c || !num_islands) return EDYNHIP_ERR_INVALID;
    const uint32_t n = c->b.n;
    *num_islands = 0;
    if (n == 0) return EDYNHIP_OK;
    EH_HIP(c, hipSetDevice(c->device));
    uint32_t *d = nullptr;
    const MonLayout L(n);
    EH_HIP(c, hipMalloc((void **)&d, L.words * sizeof(uint32_t)));
    uint32_t *count = d + 1, *out_label = d + L.out_label;
    float *out_box = (float *)(d + L.out_box);
    hipError_t e = launch_island_boxes(c->stream, n, c->b, d, L, false);
    uint32_t k = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&k, count, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    int rc = EDYNHIP_OK;
    if (e == hipSuccess) {
        *num_islands = k;
        if (labels && boxes6) {
            if (capacity < k) rc = set_error(c, EDYNHIP_ERR_CAPACITY, "edynhip_get_island_boxes: capacity");
            else if (k) {
                e = hipMemcpyAsync(labels, out_label, (size_t)k * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
                if (e == hipSuccess) e = hipMemcpyAsync(boxes6, out_box, (size_t)k * 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            }
        }
    }
    (void)hipFree(d);
    if (e != hipSuccess) return set_error(c, EDYNHIP_ERR_HIP, "edynhip_get_island_boxes", e);
    return rc;
}

static std::string g_world_create_error;

edynhip_world *edynhip_world_create(const edynhip_config *cfg, const int32_t *devices, uint32_t num_devices, int *status_out) {
    auto fail = [&](int code, const char *msg) -> edynhip_world * { g_world_create_error = msg; if (status_out) *status_out = code; return nullptr; };
    if (!cfg || !devices || num_devices == 0 || num_devices > 64) return fail(EDYNHIP_ERR_INVALID, "edynhip_world_create: bad arguments");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(EDYNHIP_ERR_NO_DEVICE, "edynhip_world_create: no HIP device (this library has no CPU fallback)");
    for (uint32_t r = 0; r < num_devices; ++r) if (devices[r] < 0 || devices[r] >= ndev) return fail(EDYNHIP_ERR_INVALID, "edynhip_world_create: device ordinal out of range");
    edynhip_world *w = new edynhip_world();
    w->cfg = *cfg;
    w->knobs = eh::read_knobs();
    w->devices.assign(devices, devices + num_devices);
    w->shards.resize(num_devices);
    for (uint32_t r = 0; r < num_devices; ++r) w->shards[r].device = devices[r];
    // several shards on ONE device (functional tests) must not promise that device to each of them
    for (uint32_t r = 0; r < num_devices; ++r) for (uint32_t q = 0; q < r; ++q) if (devices[q] == devices[r]) w->cfg.flags &= ~(uint32_t)EDYNHIP_FLAG_EXCLUSIVE_DEVICE;
    w->pool.reset(new Pool(num_devices, w->knobs.world_serial));
    w->shard_filters.resize(num_devices);
    for (uint32_t r = 0; r < num_devices; ++r) w->shard_filters[r] = edynhip_world::ShardFilter{w, r};
    w->stats.num_shards = num_devices;
    if (status_out) *status_out = EDYNHIP_OK;
    return w;
}

void edynhip_world_destroy(edynhip_world *w) {
    if (!w) return;
    for (Shard &s : w->shards) free_shard(s);
    if (!w->devices.empty()) (void)hipSetDevice(w->devices[0]);
    if (w->qstream) { (void)hipStreamSynchronize(w->qstream); (void)hipStreamDestroy(w->qstream); }
    for (DevBuf *b : {&w->h_hits, &w->h_cnt, &w->h_off, &w->h_ids, &w->h_scan, &w->h_in, &w->h_out, &w->h_off_out, &w->h_ids_out, &w->ev_list}) dev_free(*b);
    if (w->q_pin) (void)hipHostFree(w->q_pin);
    if (w->rec_stream) { (void)hipStreamSynchronize(w->rec_stream); (void)hipStreamDestroy(w->rec_stream); }
    for (int k = 0; k < 2; ++k) {
        if (w->rec_ev_done[k]) (void)hipEventDestroy(w->rec_ev_done[k]);
        if (w->rec[k].host) (void)hipHostFree(w->rec[k].host);
    }
    delete w;
}

const char *edynhip_world_last_error(const edynhip_world *w) { return w ? w->err.c_str() : g_world_create_error.c_str(); }

int edynhip_world_create_convex_mesh(edynhip_world *w, uint32_t num_vertices, const float *vertices, uint32_t num_indices, const uint32_t *indices,
                                     uint32_t num_faces, const uint32_t *faces, uint32_t flags, uint32_t *mesh_id) {
    if (!w || !vertices || !indices || !faces || !mesh_id) return EDYNHIP_ERR_INVALID;
    if (w->built) return w->fail(EDYNHIP_ERR_UNSUPPORTED, "edynhip_world_create_convex_mesh: meshes are created before the bodies");
    HostScene::Mesh m;
    m.v.assign(vertices, vertices + 3 * (size_t)num_vertices); m.idx.assign(indices, indices + num_indices); m.faces.assign(faces, faces + 2 * (size_t)num_faces); m.flags = flags;
    w->scene.meshes.push_back(std::move(m));
    *mesh_id = (uint32_t)w->scene.meshes.size() - 1;
    return EDYNHIP_OK;
}

int edynhip_world_set_bodies(edynhip_world *w, uint32_t n, const edynhip_bodies *in) {
    if (!w || !in || n == 0) return EDYNHIP_ERR_INVALID;
    if (!in->kind || !in->pos || !in->orn || !in->linvel || !in->angvel || !in->mass || !in->shape_type || !in->shape_param || !in->friction || !in->restitution)
        return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_set_bodies: missing array");
    HostScene &sc = w->scene;
    sc.n = 0;
    sc.kind.clear(); sc.shape_type.clear(); sc.pos.clear(); sc.orn.clear(); sc.linvel.clear(); sc.angvel.clear(); sc.mass.clear(); sc.shape_param.clear();
    sc.friction.clear(); sc.restitution.clear(); sc.inertia.clear(); sc.has_inertia.clear(); sc.group.clear(); sc.mask.clear(); sc.gravity.clear();
    sc.sleeping_disabled.clear(); sc.com.clear();
    scene_append_bodies(w, n, in);
    sc.nj = 0; sc.jtype.clear(); sc.jbody.clear(); sc.jpivot.clear(); sc.jaxis.clear(); sc.jparams.clear(); sc.jalive.clear(); sc.defs.clear(); sc.exclusions.clear();
    w->removed.assign(n, 0); w->pending_tombs.clear();
    w->built = false; w->stepped = false;
    w->step_count = 0; w->ev_n = 0; w->ev_overflow = false; w->ev_occurred = 0;
    w->tombs.clear();
    w->stats.num_bodies = n;
    return EDYNHIP_OK;
}

int edynhip_world_set_joints(edynhip_world *w, uint32_t n, const edynhip_joints *in) {
    if (!w || (n && (!in || !in->type || !in->body || !in->pivot))) return EDYNHIP_ERR_INVALID;
    // The scene description is what the world is (re)built from - with the INITIAL state of edynhip_world_set_bodies. Once the world has
    // stepped, such a rebuild would silently reset the simulation: refused (a running world is edited through edynhip_world_add_joints,
    // _remove_joints, _edit_joint, _edit_exclusion ... below; edynhip_world_set_bodies with the current state starts a new world)
    if (w->stepped) return w->fail(EDYNHIP_ERR_UNSUPPORTED, "edynhip_world_set_joints: the world has been stepped; describe the scene again (edynhip_world_set_bodies with the current state) before editing it");
    HostScene &sc = w->scene;
    for (uint32_t k = 0; k < 2 * n; ++k) if (in->body[k] >= sc.n) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_set_joints: body index out of range");
    sc.nj = 0; sc.jtype.clear(); sc.jbody.clear(); sc.jpivot.clear(); sc.jaxis.clear(); sc.jparams.clear(); sc.jalive.clear();
    scene_append_joints(sc, n, in);
    sc.defs.clear();
    w->built = false;
    return EDYNHIP_OK;
}

int edynhip_world_set_joint_definition(edynhip_world *w, uint32_t joint, const float *frame_a9, const float *frame_b9, const float *params, int generic) {
    if (!w || !frame_a9 || !frame_b9 || !params || joint >= w->scene.nj) return EDYNHIP_ERR_INVALID;
    if (w->stepped) return w->fail(EDYNHIP_ERR_UNSUPPORTED, "edynhip_world_set_joint_definition: the world has been stepped; describe the scene again first (see edynhip_world_set_joints)");
    w->scene.defs.push_back(make_def(joint, frame_a9, frame_b9, params, generic != 0));
    w->built = false;
    return EDYNHIP_OK;
}

int edynhip_world_exclude_collision(edynhip_world *w, uint32_t a, uint32_t b) {
    if (!w || a >= w->scene.n || b >= w->scene.n) return EDYNHIP_ERR_INVALID;
    if (w->stepped) return w->fail(EDYNHIP_ERR_UNSUPPORTED, "edynhip_world_exclude_collision: the world has been stepped; describe the scene again first (see edynhip_world_set_joints)");
    w->scene.exclusions.push_back({a, b});
    w->built = false;
    return EDYNHIP_OK;
}

int edynhip_world_set_pair_filter(edynhip_world *w, edynhip_pair_filter filter, void *user) {
    if (!w) return EDYNHIP_ERR_INVALID;
    w->filter = filter; w->filter_user = user;
    if (!w->built) return EDYNHIP_OK;   // installed when the shards are built
    for (uint32_t r = 0; r < w->shards.size(); ++r) {
        Shard &s = w->shards[r];
        if (!s.ctx) continue;
        const int rc = edynhip_set_pair_filter(s.ctx, filter ? &shard_filter_thunk : nullptr, &w->shard_filters[r]);
        if (rc != EDYNHIP_OK) return w->fail(rc, std::string("edynhip_world_set_pair_filter: shard ") + std::to_string(r) + ": " + edynhip_last_error(s.ctx));
    }
    return EDYNHIP_OK;
}

int edynhip_world_default_should_collide(edynhip_world *w, uint32_t a, uint32_t b) {   // should_collide_default in global indices
    if (!w || a >= w->scene.n || b >= w->scene.n) return EDYNHIP_ERR_INVALID;
    if (a == b) return 0;
    const HostScene &sc = w->scene;
    const uint64_t ga = sc.group.empty() ? ~0ull : sc.group[a], gb = sc.group.empty() ? ~0ull : sc.group[b];
    const uint64_t ma = sc.mask.empty() ? ~0ull : sc.mask[a], mb = sc.mask.empty() ? ~0ull : sc.mask[b];
    if ((ga & mb) == 0 || (gb & ma) == 0) return 0;
    for (const auto &e : sc.exclusions) if ((e[0] == a && e[1] == b) || (e[0] == b && e[1] == a)) return 0;
    return 1;
}

int edynhip_world_step(edynhip_world *w, uint32_t nsteps) {
    if (!w) return EDYNHIP_ERR_INVALID;
    EH_TRY(ensure_built(w));
    const bool events = w->events_on();
    w->ev_n = 0; w->ev_overflow = false; w->ev_occurred = 0;   // the events of THIS call
    for (uint32_t k = 0; k < nsteps; ++k) {
        const bool on_callers_thread = w->pool->run([w](uint32_t r) {
            Shard &s = w->shards[r];
            if (s.rc != EDYNHIP_OK || s.local_ids.empty()) return;
            if (hipSetDevice(s.device) != hipSuccess) { s.rc = EDYNHIP_ERR_HIP; s.err = "hipSetDevice"; return; }
            SH_TRY(s, edynhip_step(s.ctx, 1));
            gather_shard(w, r, true);
        });
        if (on_callers_thread) w->paths |= EDYNHIP_PATH_WORLD_SERIAL;
        EH_TRY(shard_error(w));
        ++w->stats.steps; ++w->step_count;
        w->stepped = true;
        finish_tombstones(w);   // the step dropped the removed bodies' manifolds
        if (events) EH_TRY(append_events(w));
        if (w->shards.size() < 2) continue;
        float growth = 0.0f;
        for (Shard &s : w->shards) if (!s.local_ids.empty()) { float g; std::memcpy(&g, s.mon_host, 4); growth = std::max(growth, g); }
        if (2 * growth < w->budget) continue;   // nobody has moved far enough out of the boxes of the last check
        bool close = false;
        EH_TRY(approach_check(w, close));
        if (close) EH_TRY(repartition(w, true));
    }
    return EDYNHIP_OK;
}

int edynhip_world_repartition(edynhip_world *w) {
    if (!w) return EDYNHIP_ERR_INVALID;
    EH_TRY(ensure_built(w));
    return repartition(w, false);
}

int edynhip_world_get_state(edynhip_world *w, float *pos, float *orn, float *linvel, float *angvel) {
    if (!w) return EDYNHIP_ERR_INVALID;
    EH_TRY(ensure_built(w));
    const size_t n = w->scene.n;
    if (pos) std::memcpy(pos, w->pos.data(), 3 * n * sizeof(float));
    if (orn) std::memcpy(orn, w->orn.data(), 4 * n * sizeof(float));
    if (linvel) std::memcpy(linvel, w->linvel.data(), 3 * n * sizeof(float));
    if (angvel) std::memcpy(angvel, w->angvel.data(), 3 * n * sizeof(float));
    return EDYNHIP_OK;
}

int edynhip_world_get_partition(edynhip_world *w, int32_t *rank_of) {
    if (!w || !rank_of) return EDYNHIP_ERR_INVALID;
    EH_TRY(ensure_built(w));
    std::memcpy(rank_of, w->rank_of.data(), w->scene.n * sizeof(int32_t));
    for (uint32_t g = 0; g < w->scene.n; ++g) if (w->is_removed(g)) rank_of[g] = -1;   // a tombstone is nobody's
    return EDYNHIP_OK;
}

int edynhip_world_get_manifolds(edynhip_world *w, edynhip_manifold *out, uint32_t capacity, uint32_t *n) {
    if (!w || !n) return EDYNHIP_ERR_INVALID;
    EH_TRY(ensure_built(w));
    w->pool->run([w](uint32_t r) { collect_shard(w, r, false, true); });
    EH_TRY(shard_error(w));
    std::vector<edynhip_manifold> all;
    merge_manifolds(w, all);
    *n = (uint32_t)all.size();
    if (out) {
        if (capacity < all.size()) return w->fail(EDYNHIP_ERR_CAPACITY, "edynhip_world_get_manifolds: capacity");
        if (!all.empty()) std::memcpy(out, all.data(), all.size() * sizeof(edynhip_manifold));
    }
    return EDYNHIP_OK;
}

int edynhip_world_get_contact_events(edynhip_world *w, edynhip_contact_event *out, uint32_t capacity, uint32_t *n) {
    static_assert(sizeof(edynhip_contact_event) == sizeof(ContactEvent), "event record layout");
    if (!w || !n) return EDYNHIP_ERR_INVALID;
    *n = 0;
    if (!w->events_on()) return w->fail(EDYNHIP_ERR_UNSUPPORTED, "edynhip_world_get_contact_events: create the world with EDYNHIP_FLAG_CONTACT_EVENTS");
    *n = w->ev_n;
    if (out) {
        if (capacity < w->ev_n) return w->fail(EDYNHIP_ERR_CAPACITY, "edynhip_world_get_contact_events: capacity too small");
        if (w->ev_n) {   // the last step's blocks were appended on the shards' streams
            for (Shard &s : w->shards) if (s.ctx) { W_HIP(w, hipSetDevice(s.device)); W_HIP(w, hipStreamSynchronize(s.ctx->stream)); }
            W_HIP(w, hipSetDevice(w->devices[0]));
            W_HIP(w, hipMemcpy(out, w->ev_list.p, (size_t)w->ev_n * sizeof(ContactEvent), hipMemcpyDeviceToHost));
        }
    }
    if (w->ev_overflow) return w->fail(EDYNHIP_ERR_CAPACITY, "edynhip_world_get_contact_events: a shard recorded more events than it holds; resynchronise from edynhip_world_get_manifolds and edynhip_world_get_point_ids");
    return EDYNHIP_OK;
}

int edynhip_world_get_point_ids(edynhip_world *w, uint64_t *ids, uint32_t capacity_manifolds, uint32_t *n) {
    if (!w || !n) return EDYNHIP_ERR_INVALID;
    *n = 0;
    if (!w->events_on()) return w->fail(EDYNHIP_ERR_UNSUPPORTED, "edynhip_world_get_point_ids: create the world with EDYNHIP_FLAG_CONTACT_EVENTS");
    EH_TRY(ensure_built(w));
    w->pool->run([w](uint32_t r) { collect_shard(w, r, false, true); });
    EH_TRY(shard_error(w));
    std::vector<edynhip_manifold> all;
    std::vector<uint64_t> all_ids;
    merge_manifolds(w, all, &all_ids);
    *n = (uint32_t)all.size();
    if (ids) {
        if (capacity_manifolds < all.size()) return w->fail(EDYNHIP_ERR_CAPACITY, "edynhip_world_get_point_ids: capacity too small");
        if (!all_ids.empty()) std::memcpy(ids, all_ids.data(), all_ids.size() * sizeof(uint64_t));
    }
    return EDYNHIP_OK;
}

int edynhip_world_get_stats(edynhip_world *w, edynhip_world_stats *out) {
    if (!w || !out) return EDYNHIP_ERR_INVALID;
    *out = w->stats;
    return EDYNHIP_OK;
}

int edynhip_world_debug_paths(edynhip_world *w, uint64_t *mask) {
    if (!w || !mask) return EDYNHIP_ERR_INVALID;
    uint64_t m = w->paths;
    for (const Shard &s : w->shards) {
        uint64_t sm = 0;
        if (s.ctx && edynhip_debug_paths(s.ctx, &sm) == EDYNHIP_OK) m |= sm;
        m |= s.paths_gone;
    }
    *mask = m;
    return EDYNHIP_OK;
}

edynhip_ctx *edynhip_world_context(edynhip_world *w, uint32_t shard) {
    if (!w || shard >= w->shards.size() || ensure_built(w) != EDYNHIP_OK) return nullptr;
    return w->shards[shard].ctx;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ edits of a running world
// edynhip_world_add_bodies / _remove_bodies / _add_joints / _remove_joints / _edit_joint / _edit_exclusion / _set_state / _set_params:
// the single context's edits in global indices. The scene (HostScene) stays the truth the shards are rebuilt from - bodies are appended,
// a removed body becomes what the context itself turns the slot into (a shapeless static body), joints get an alive flag - and the
// edit is forwarded to the context(s) that hold the bodies, so nobody else's manifolds, impulses, timers or point ids are touched.
// The global-to-local maps stay ascending because a new body or joint has the highest global AND the highest local index.
namespace {

void scene_tombstones(edynhip_world *w, const std::vector<uint32_t> &gone) {
    HostScene &sc = w->scene;
    // A context keeps a removed body's manifolds until its next step drops them (with their destroy events). Until then the scene keeps
    // the body as it was described, so that a shard rebuilt in between gets the body, its manifolds and their point ids as the old
    // context held them and has the removal replayed on it (build_shard); the world's next step makes the slot what the context made of
    // it for good: a shapeless static body (finish_tombstones).
    for (uint32_t g : gone) { w->removed[g] = 1; w->pending_tombs.push_back(g); w->tombs.push_back(g); }
    if (!w->built) finish_tombstones(w);
    for (uint32_t j = 0; j < sc.nj; ++j) if (sc.jalive[j] && (w->removed[sc.jbody[2 * j]] || w->removed[sc.jbody[2 * j + 1]])) sc.jalive[j] = 0;
    sc.exclusions.erase(std::remove_if(sc.exclusions.begin(), sc.exclusions.end(), [&](const std::array<uint32_t, 2> &e) { return w->removed[e[0]] || w->removed[e[1]]; }),
                        sc.exclusions.end());
}

// the shard that holds global joint j in its context (-1: none - a removed joint, or one between two replicated bodies) and its index there
int32_t joint_shard(const edynhip_world *w, uint32_t j, uint32_t &local) {
    for (uint32_t r = 0; r < w->shards.size(); ++r) {
        const std::vector<uint32_t> &lj = w->shards[r].local_joints;
        const auto it = std::lower_bound(lj.begin(), lj.end(), j);
        if (it != lj.end() && *it == j) { local = (uint32_t)(it - lj.begin()); return (int32_t)r; }
    }
    return -1;
}

// the shard a joint between global bodies a and b lives on by the partition as it stands (joint_home: -1 no context holds it, -2 two shards)
int32_t joint_home_of(const edynhip_world *w, uint32_t a, uint32_t b) {
    return joint_home(owner_rank(w->scene.kind[a], w->rank_of[a]), owner_rank(w->scene.kind[b], w->rank_of[b]));
}

// Rebuilds the shards marked in `force` (each with the head-room its want_bodies / want_joints ask for) through what a sticky
// re-partition carries; nothing else moves.
int grow_shards(edynhip_world *w, const std::vector<uint8_t> &force) {
    for (uint8_t f : force) if (f) ++w->edit_stats.shard_rebuilds;
    return repartition(w, true, nullptr, &force, true);
}

// A shard whose context cannot take its share of an edit - extra[r] more bodies, or joints - is rebuilt with head-room first, through
// the carry. recount (or nullptr): refreshes `extra` after the rebuild (a rebalance may have moved islands). who: the entry point.
int make_room(edynhip_world *w, bool joints, std::vector<uint32_t> &extra, const char *who, bool &grown, const std::function<int()> &recount = nullptr) {
    const uint32_t W = (uint32_t)w->shards.size();
    auto lacks = [&](uint32_t r) {
        const Shard &s = w->shards[r];
        return extra[r] && (!s.ctx || (joints ? s.local_joints.size() + extra[r] > s.joint_cap : s.local_ids.size() + extra[r] > s.cap));
    };
    std::vector<uint8_t> force(W, 0);
    grown = false;
    for (uint32_t r = 0; r < W; ++r) if (lacks(r)) { force[r] = 1; (joints ? w->shards[r].want_joints : w->shards[r].want_bodies) = extra[r]; grown = true; }
    if (!grown) return EDYNHIP_OK;
    EH_TRY(grow_shards(w, force));
    if (recount) EH_TRY(recount());
    for (uint32_t r = 0; r < W; ++r) if (lacks(r)) return w->fail(EDYNHIP_ERR_INTERNAL, std::string(who) + ": shard " + std::to_string(r) + " was rebuilt and still lacks room");
    return EDYNHIP_OK;
}

// The safety condition after an edit that can bring islands of different shards together (a shaped dynamic body was added): the approach
// check - body boxes while a shard has not stepped since it was built, island boxes otherwise; a new body is an island of its own either
// way - which also records the boxes the growth monitor measures the new bodies against, and the sticky re-partition if it says "close".
int edit_approach(edynhip_world *w, bool &moved) {
    moved = false;
    if (w->shards.size() < 2) return EDYNHIP_OK;
    bool per_body = false;
    for (const Shard &s : w->shards) if (s.ctx && !s.local_ids.empty() && s.ctx->step_index == 0) per_body = true;
    bool close = false;
    ++w->edit_stats.approach_checks_by_edit;
    EH_TRY(approach_check(w, close, per_body));
    if (!close) return EDYNHIP_OK;
    moved = true;
    ++w->edit_stats.repartitions_by_edit;
    return repartition(w, true, nullptr, nullptr, true);
}

}  // namespace

extern "C" {

int edynhip_world_add_bodies(edynhip_world *w, uint32_t n, const edynhip_bodies *in, uint32_t *first_index) {
    if (!w) return EDYNHIP_ERR_INVALID;
    HostScene &sc = w->scene;
    if (first_index) *first_index = sc.n;
    if (n == 0) return EDYNHIP_OK;
    if (!in || !in->kind || !in->pos || !in->orn || !in->linvel || !in->angvel || !in->mass || !in->shape_type || !in->shape_param || !in->friction || !in->restitution)
        return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_add_bodies: missing array");
    if (sc.n == 0) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_add_bodies: describe the world first (edynhip_world_set_bodies)");
    if ((uint64_t)sc.n + n > 0x7FFFFFFFull) return w->fail(EDYNHIP_ERR_CAPACITY, "edynhip_world_add_bodies: too many bodies");
    for (uint32_t k = 0; k < n; ++k) {
        if (in->kind[k] < EDYNHIP_KIND_DYNAMIC || in->kind[k] > EDYNHIP_KIND_STATIC) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_add_bodies: unknown body kind");
        if (in->shape_type[k] < EDYNHIP_SHAPE_NONE || in->shape_type[k] > EDYNHIP_SHAPE_POLYHEDRON) return w->fail(EDYNHIP_ERR_UNSUPPORTED, "edynhip_world_add_bodies: shape type");
        if (in->shape_type[k] == EDYNHIP_SHAPE_POLYHEDRON && !(in->shape_param[4 * (size_t)k] >= 0 && (size_t)in->shape_param[4 * (size_t)k] < sc.meshes.size()))
            return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_add_bodies: a polyhedron refers to a mesh the world does not hold");
    }
    const uint32_t n0 = sc.n, W = (uint32_t)w->shards.size();
    if (!w->built) { scene_append_bodies(w, n, in); return EDYNHIP_OK; }
    ++w->edit_stats.edits;
    // placement (place_new_bodies): replicated, or the shard with the fewest live dynamic bodies; bodies of the call that touch (the
    // boxes of their bounding spheres within the creation margin: estimate_islands over the new bodies alone) land on one shard
    std::vector<uint32_t> load(W, 0), extra(W, 0);
    for (uint32_t g = 0; g < n0; ++g) if (sc.kind[g] == EDYNHIP_KIND_DYNAMIC && !w->is_removed(g) && w->rank_of[g] >= 0) ++load[(uint32_t)w->rank_of[g]];
    std::vector<uint32_t> group(n);
    MeshRadii meshes = scene_meshes(sc);
    estimate_islands({n, in->kind, in->shape_type, in->shape_param, in->pos, in->center_of_mass}, meshes, 0, nullptr, nullptr, group.data(), nullptr);
    const std::vector<int32_t> place = place_new_bodies(n, in->kind, group.data(), load, extra);
    bool shaped_dynamic = false;
    for (uint32_t k = 0; k < n; ++k) if (in->kind[k] == EDYNHIP_KIND_DYNAMIC && in->shape_type[k] != EDYNHIP_SHAPE_NONE) shaped_dynamic = true;
    bool grown = false;
    EH_TRY(make_room(w, false, extra, "edynhip_world_add_bodies", grown));
    scene_append_bodies(w, n, in);
    for (uint32_t k = 0; k < n; ++k) w->rank_of.push_back(place[k]);
    w->pos.insert(w->pos.end(), in->pos, in->pos + 3 * (size_t)n); w->orn.insert(w->orn.end(), in->orn, in->orn + 4 * (size_t)n);
    w->linvel.insert(w->linvel.end(), in->linvel, in->linvel + 3 * (size_t)n); w->angvel.insert(w->angvel.end(), in->angvel, in->angvel + 3 * (size_t)n);
    if (w->query_labels.size() == n0) for (uint32_t k = 0; k < n; ++k) w->query_labels.push_back(n0 + k);
    std::vector<std::vector<uint32_t>> mine(W);
    for (uint32_t r = 0; r < W; ++r) {
        w->shards[r].to_local.resize((size_t)n0 + n, -1);
        for (uint32_t k = 0; k < n; ++k) if (shard_holds_body(place[k], r)) mine[r].push_back(k);
    }
    EH_TRY(on_shards(w, [&](Shard &, uint32_t r) { return !mine[r].empty(); }, [&](Shard &s, uint32_t r) {
        const BodyRows sub(*in, mine[r]);
        const edynhip_bodies b = sub.view();
        SH_TRY(s, edynhip_add_bodies(s.ctx, (uint32_t)mine[r].size(), &b));
        const uint32_t l0 = (uint32_t)s.local_ids.size();
        for (uint32_t k : mine[r]) {
            const uint32_t l = (uint32_t)s.local_ids.size();
            s.to_local[n0 + k] = (int32_t)l;
            if (shard_reports_body(place[k], r)) s.owned_local.push_back(l);
            s.local_ids.push_back(n0 + k);
        }
        upload_query_tables(w, r, l0);
        if (s.rc != EDYNHIP_OK) return;
        gather_shard(w, r, false);   // the state the context holds for them (the centre of mass where the caller gave an origin)
    }));
    refresh_bodies_per_shard(w);
    bool moved = false;
    if (shaped_dynamic) EH_TRY(edit_approach(w, moved));
    if (!grown && !moved) ++w->edit_stats.in_place;
    return EDYNHIP_OK;
}

int edynhip_world_remove_bodies(edynhip_world *w, uint32_t n, const uint32_t *indices) {
    if (!w || (n && !indices)) return EDYNHIP_ERR_INVALID;
    HostScene &sc = w->scene;
    for (uint32_t k = 0; k < n; ++k) if (indices[k] >= sc.n) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_remove_bodies: index out of range");
    std::vector<uint32_t> gone;
    for (uint32_t k = 0; k < n; ++k) if (!w->is_removed(indices[k]) && std::find(gone.begin(), gone.end(), indices[k]) == gone.end()) gone.push_back(indices[k]);
    if (gone.empty()) return EDYNHIP_OK;
    w->removed.resize(sc.n, 0);
    if (w->built) {
        ++w->edit_stats.edits;
        std::vector<std::vector<uint32_t>> mine(w->shards.size());   // the owner of a dynamic body, every shard for a replicated one
        for (uint32_t r = 0; r < w->shards.size(); ++r) {
            const Shard &s = w->shards[r];
            for (uint32_t g : gone) if (g < s.to_local.size() && s.to_local[g] >= 0) mine[r].push_back((uint32_t)s.to_local[g]);
        }
        EH_TRY(on_shards(w, [&](Shard &s, uint32_t r) { return !mine[r].empty() && s.ctx; }, [&](Shard &s, uint32_t r) {
            SH_TRY(s, edynhip_remove_bodies(s.ctx, (uint32_t)mine[r].size(), mine[r].data()));
        }));
        ++w->edit_stats.in_place;
    }
    scene_tombstones(w, gone);
    return EDYNHIP_OK;
}

int edynhip_world_add_joints(edynhip_world *w, uint32_t n, const edynhip_joints *in, uint32_t *first_index) {
    if (!w) return EDYNHIP_ERR_INVALID;
    HostScene &sc = w->scene;
    if (first_index) *first_index = sc.nj;
    if (n == 0) return EDYNHIP_OK;
    if (!in || !in->type || !in->body || !in->pivot) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_add_joints: missing array");
    for (uint32_t e = 0; e < n; ++e) {
        const uint32_t a = in->body[2 * e], b = in->body[2 * e + 1];
        if (a >= sc.n || b >= sc.n) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_add_joints: body index out of range");
        // (a null constraint has no rows: it may name any slot - a caller reserves a joint index with one, as the C++ shim does)
        if (in->type[e] != EDYNHIP_JOINT_NULL && (w->is_removed(a) || w->is_removed(b))) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_add_joints: joint " + std::to_string(e) + " names a removed body");
        if (in->type[e] < EDYNHIP_JOINT_POINT || in->type[e] > EDYNHIP_JOINT_NULL) return w->fail(EDYNHIP_ERR_UNSUPPORTED, "edynhip_world_add_joints: joint type");
        if (in->type[e] == EDYNHIP_JOINT_HINGE && !in->axis) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_add_joints: hinge needs axes");
    }
    const uint32_t nj0 = sc.nj, W = (uint32_t)w->shards.size();
    if (!w->built) { scene_append_joints(sc, n, in); return EDYNHIP_OK; }
    ++w->edit_stats.edits;
    // a joint between two shards: its islands move together first (the welding unites the pair), then the joint is made in place
    bool moved = false;
    {
        std::vector<std::array<uint32_t, 2>> edges;
        for (uint32_t e = 0; e < n; ++e) if (joint_home_of(w, in->body[2 * e], in->body[2 * e + 1]) == -2) edges.push_back({in->body[2 * e], in->body[2 * e + 1]});
        if (!edges.empty()) {
            moved = true;
            ++w->edit_stats.repartitions_by_edit;
            EH_TRY(repartition(w, true, &edges, nullptr, true));
            for (const auto &e : edges) if (joint_home_of(w, e[0], e[1]) == -2) return w->fail(EDYNHIP_ERR_INTERNAL, "edynhip_world_add_joints: the re-partition left a joint's bodies on two shards");
        }
    }
    std::vector<int32_t> home(n);
    std::vector<uint32_t> extra(W, 0);
    auto count_homes = [&]() -> int {   // (again after shards were rebuilt: a rebalance may have moved islands)
        std::fill(extra.begin(), extra.end(), 0u);
        for (uint32_t e = 0; e < n; ++e) {
            home[e] = joint_home_of(w, in->body[2 * e], in->body[2 * e + 1]);
            if (home[e] == -2) return w->fail(EDYNHIP_ERR_INTERNAL, "edynhip_world_add_joints: a joint's bodies are on two shards");
            if (home[e] >= 0) ++extra[(uint32_t)home[e]];
        }
        return EDYNHIP_OK;
    };
    EH_TRY(count_homes());
    bool grown = false;
    EH_TRY(make_room(w, true, extra, "edynhip_world_add_joints", grown, count_homes));
    std::vector<std::vector<uint32_t>> mine(W);
    for (uint32_t e = 0; e < n; ++e) if (home[e] >= 0) mine[(uint32_t)home[e]].push_back(e);
    EH_TRY(on_shards(w, [&](Shard &, uint32_t r) { return !mine[r].empty(); }, [&](Shard &s, uint32_t r) {
        auto jt = rows_of(in->type, mine[r], 1);
        auto jb = rows_of(in->body, mine[r], 2);
        for (uint32_t &x : jb) x = (uint32_t)s.to_local[x];
        auto jp = rows_of(in->pivot, mine[r], 6), ja = rows_of(in->axis, mine[r], 6), jq = rows_of(in->params, mine[r], 10);
        edynhip_joints j{};
        j.type = jt.data(); j.body = jb.data(); j.pivot = jp.data(); j.axis = ja.empty() ? nullptr : ja.data(); j.params = jq.empty() ? nullptr : jq.data();
        uint32_t first = 0;
        SH_TRY(s, edynhip_add_joints(s.ctx, (uint32_t)mine[r].size(), &j, &first));
        if (first != s.local_joints.size()) { s.rc = EDYNHIP_ERR_INTERNAL; s.err = "the context's joint indices and the shard's joint map disagree"; return; }
        for (uint32_t e : mine[r]) s.local_joints.push_back(nj0 + e);
    }));
    scene_append_joints(sc, n, in);
    if (!grown && !moved) ++w->edit_stats.in_place;
    return EDYNHIP_OK;
}

int edynhip_world_remove_joints(edynhip_world *w, uint32_t n, const uint32_t *indices) {
    if (!w || (n && !indices)) return EDYNHIP_ERR_INVALID;
    HostScene &sc = w->scene;
    for (uint32_t k = 0; k < n; ++k) if (indices[k] >= sc.nj) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_remove_joints: index out of range");
    std::vector<uint32_t> gone;
    for (uint32_t k = 0; k < n; ++k) if (sc.jalive[indices[k]] && std::find(gone.begin(), gone.end(), indices[k]) == gone.end()) gone.push_back(indices[k]);
    if (gone.empty()) return EDYNHIP_OK;
    if (w->built) {
        ++w->edit_stats.edits;
        std::vector<std::vector<uint32_t>> mine(w->shards.size());
        for (uint32_t j : gone) { uint32_t l = 0; const int32_t r = joint_shard(w, j, l); if (r >= 0) mine[(uint32_t)r].push_back(l); }
        EH_TRY(on_shards(w, [&](Shard &, uint32_t r) { return !mine[r].empty(); }, [&](Shard &s, uint32_t r) {
            SH_TRY(s, edynhip_remove_joints(s.ctx, (uint32_t)mine[r].size(), mine[r].data()));
        }));
        ++w->edit_stats.in_place;
    }
    for (uint32_t j : gone) sc.jalive[j] = 0;
    return EDYNHIP_OK;
}

int edynhip_world_edit_joint(edynhip_world *w, uint32_t joint, const float *frame_a9, const float *frame_b9, const float *params, int generic) {
    if (!w) return EDYNHIP_ERR_INVALID;
    HostScene &sc = w->scene;
    if (!params || generic < -1 || generic > 1 || (generic >= 0 && (!frame_a9 || !frame_b9))) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_edit_joint: missing array");
    if (joint >= sc.nj) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_edit_joint: joint index out of range");
    if (!sc.jalive[joint]) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_edit_joint: the joint has been removed");
    const int t = sc.jtype[joint];
    if (generic == 0 && t != EDYNHIP_JOINT_CONE && t != EDYNHIP_JOINT_CVJOINT) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_edit_joint: cone and cvjoint constraints only");
    if (generic == 0 && t == EDYNHIP_JOINT_CONE && !(params[0] > 0 && params[1] > 0)) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_edit_joint: cone span tangents must be positive");
    if (generic == 1 && t != EDYNHIP_JOINT_GENERIC) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_edit_joint: generic constraints only");
    if (generic == 1) for (int d = 0; d < 6; ++d) if (params[10 * d] != 0 && params[10 * d + 1] > params[10 * d + 2]) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_edit_joint: a limit's minimum exceeds its maximum");
    if (w->built) {
        ++w->edit_stats.edits;
        uint32_t l = 0;
        const int32_t r = joint_shard(w, joint, l);
        if (r >= 0) {
            Shard &s = w->shards[(uint32_t)r];
            W_HIP(w, hipSetDevice(s.device));
            const int rc = generic < 0 ? edynhip_set_joint_params(s.ctx, l, params) : (generic ? edynhip_set_generic_definition(s.ctx, l, frame_a9, frame_b9, params) : edynhip_set_joint_definition(s.ctx, l, frame_a9, frame_b9, params));
            if (rc != EDYNHIP_OK) return w->fail(rc, std::string("edynhip_world_edit_joint: shard ") + std::to_string(r) + ": " + edynhip_last_error(s.ctx));
        }
        ++w->edit_stats.in_place;
    }
    if (generic < 0) { std::memcpy(&sc.jparams[10 * (size_t)joint], params, 10 * sizeof(float)); return EDYNHIP_OK; }
    HostScene::Def d = make_def(joint, frame_a9, frame_b9, params, generic != 0);
    for (HostScene::Def &old : sc.defs) if (old.joint == joint && old.generic == d.generic) { old = std::move(d); return EDYNHIP_OK; }
    sc.defs.push_back(std::move(d));
    return EDYNHIP_OK;
}

int edynhip_world_edit_exclusion(edynhip_world *w, uint32_t a, uint32_t b, int exclude) {
    if (!w) return EDYNHIP_ERR_INVALID;
    HostScene &sc = w->scene;
    if (a >= sc.n || b >= sc.n) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_edit_exclusion: body index out of range");
    if (a == b) return exclude ? w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_edit_exclusion: a body cannot exclude itself") : (int)EDYNHIP_OK;
    if (w->is_removed(a) || w->is_removed(b)) return EDYNHIP_OK;   // (a tombstone collides with nothing)
    auto same = [&](const std::array<uint32_t, 2> &e) { return (e[0] == a && e[1] == b) || (e[0] == b && e[1] == a); };
    const bool listed = std::any_of(sc.exclusions.begin(), sc.exclusions.end(), same);
    if (exclude && !listed) {
        uint32_t na = 0, nb = 0;
        for (const auto &e : sc.exclusions) { if (e[0] == a || e[1] == a) ++na; if (e[0] == b || e[1] == b) ++nb; }
        if (na >= 16 || nb >= 16) return w->fail(EDYNHIP_ERR_CAPACITY, "edynhip_world_edit_exclusion: more than 16 exclusions on one body (collision_exclusion::max_exclusions)");
    }
    if (w->built) {
        ++w->edit_stats.edits;
        for (uint32_t r = 0; r < w->shards.size(); ++r) {   // the shard build_shard gives the pair to; a pair on two shards is the scene's until its bodies meet
            Shard &s = w->shards[r];
            if (!s.ctx || !shard_holds_exclusion(w->rank_of[a], w->rank_of[b], r)) continue;
            W_HIP(w, hipSetDevice(s.device));
            const int rc = exclude ? edynhip_exclude_collision(s.ctx, (uint32_t)s.to_local[a], (uint32_t)s.to_local[b]) : edynhip_remove_collision_exclusion(s.ctx, (uint32_t)s.to_local[a], (uint32_t)s.to_local[b]);
            if (rc != EDYNHIP_OK) return w->fail(rc, std::string("edynhip_world_edit_exclusion: shard ") + std::to_string(r) + ": " + edynhip_last_error(s.ctx));
        }
        ++w->edit_stats.in_place;
    }
    if (exclude) { if (!listed) sc.exclusions.push_back({a, b}); }
    else sc.exclusions.erase(std::remove_if(sc.exclusions.begin(), sc.exclusions.end(), same), sc.exclusions.end());
    return EDYNHIP_OK;
}

int edynhip_world_set_state(edynhip_world *w, const float *pos, const float *orn, const float *linvel, const float *angvel) {
    if (!w) return EDYNHIP_ERR_INVALID;
    if (!pos || !orn || !linvel || !angvel) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_set_state: missing array");
    HostScene &sc = w->scene;
    const size_t n = sc.n;
    if (n == 0) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_set_state: no bodies");
    if (!w->built && sc.com.empty()) {   // the description's state (with centre-of-mass offsets `pos` is no longer the origin it describes: build first)
        sc.pos.assign(pos, pos + 3 * n); sc.orn.assign(orn, orn + 4 * n); sc.linvel.assign(linvel, linvel + 3 * n); sc.angvel.assign(angvel, angvel + 3 * n);
        return EDYNHIP_OK;
    }
    EH_TRY(ensure_built(w));
    ++w->edit_stats.edits;
    w->pos.assign(pos, pos + 3 * n); w->orn.assign(orn, orn + 4 * n); w->linvel.assign(linvel, linvel + 3 * n); w->angvel.assign(angvel, angvel + 3 * n);
    EH_TRY(on_shards(w, [](Shard &s, uint32_t) { return !s.local_ids.empty() && s.ctx; }, [&](Shard &s, uint32_t) {
        auto p = take(w->pos, s.local_ids, 3), q = take(w->orn, s.local_ids, 4), v = take(w->linvel, s.local_ids, 3), o = take(w->angvel, s.local_ids, 3);
        SH_TRY(s, edynhip_set_state(s.ctx, p.data(), q.data(), v.data(), o.data()));
    }));
    // A context's boxes follow the new state at the end of its next step (edynhip_set_state), which is when its broadphase - and the growth
    // monitor - first see where the bodies went: the approach check is due right after that step, whatever the budget said before.
    w->budget = 0.0f;
    ++w->edit_stats.in_place;
    return EDYNHIP_OK;
}

int edynhip_world_get_params(edynhip_world *w, edynhip_params *out) {
    if (!w || !out) return EDYNHIP_ERR_INVALID;
    if (w->built && !w->shards.empty() && w->shards[0].ctx) return edynhip_get_params(w->shards[0].ctx, out);
    if (w->params_set) { *out = w->params; return EDYNHIP_OK; }
    out->fixed_dt = w->cfg.fixed_dt > 0 ? w->cfg.fixed_dt : 1.0f / 60.0f;
    out->num_velocity_iterations = w->cfg.num_velocity_iterations; out->num_position_iterations = w->cfg.num_position_iterations;
    std::memcpy(out->gravity, w->cfg.gravity, sizeof(out->gravity));
    out->num_restitution_iterations = 8; out->num_individual_restitution_iterations = 3;   // settings.hpp:28-29, as a context starts
    return EDYNHIP_OK;
}

int edynhip_world_set_params(edynhip_world *w, const edynhip_params *p) {
    if (!w) return EDYNHIP_ERR_INVALID;
    if (!p || !(p->fixed_dt > 0)) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_set_params: bad settings");
    HostScene &sc = w->scene;
    if (w->built) {
        ++w->edit_stats.edits;
        for (uint32_t r = 0; r < w->shards.size(); ++r) {
            Shard &s = w->shards[r];
            if (!s.ctx) continue;
            const int rc = edynhip_set_params(s.ctx, p);
            if (rc != EDYNHIP_OK) return w->fail(rc, std::string("edynhip_world_set_params: shard ") + std::to_string(r) + ": " + edynhip_last_error(s.ctx));
        }
        ++w->edit_stats.in_place;
    }
    // what later contexts are created with: set_gravity replaces the gravity of every dynamic body (gravity_util.cpp:12-20)
    if (std::memcmp(w->cfg.gravity, p->gravity, sizeof(p->gravity)) != 0 && !sc.gravity.empty())
        for (uint32_t g = 0; g < sc.n; ++g) if (sc.kind[g] == EDYNHIP_KIND_DYNAMIC) std::memcpy(&sc.gravity[3 * (size_t)g], p->gravity, sizeof(p->gravity));
    w->params = *p; w->params_set = true;
    w->cfg.fixed_dt = p->fixed_dt; w->cfg.num_velocity_iterations = p->num_velocity_iterations; w->cfg.num_position_iterations = p->num_position_iterations;
    std::memcpy(w->cfg.gravity, p->gravity, sizeof(p->gravity));
    return EDYNHIP_OK;
}

int edynhip_world_get_asleep(edynhip_world *w, uint8_t *asleep) {
    if (!w || !asleep) return EDYNHIP_ERR_INVALID;
    EH_TRY(ensure_built(w));
    std::memset(asleep, 0, w->scene.n);
    if (!(w->cfg.flags & EDYNHIP_FLAG_SLEEPING)) return EDYNHIP_OK;
    return on_shards(w, [](Shard &s, uint32_t) { return !s.local_ids.empty() && s.ctx; }, [&](Shard &s, uint32_t) {   // every body's tag from the shard that reports its state
        s.asleep.assign(s.local_ids.size(), 0);
        SH_TRY(s, edynhip_get_asleep(s.ctx, s.asleep.data()));
        for (uint32_t l : s.owned_local) asleep[s.local_ids[l]] = s.asleep[l];
    });
}

int edynhip_world_get_edit_stats(edynhip_world *w, edynhip_world_edit_stats *out) {
    if (!w || !out) return EDYNHIP_ERR_INVALID;
    *out = w->edit_stats;
    return EDYNHIP_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ record hand-over of the world
// edynhip_snapshot_records / edynhip_snapshot_map on a multi-device world: every shard packs the records of the bodies it reports with the
// single context's arithmetic and stores them at their global indices straight into one of the world's two pinned slots
// (world_records.hip); the event block is one copy from the list on the home device, behind the shards' appends. A step call returns with
// every shard idle, so "behind the steps issued so far" holds by construction; the map waits for the snapshot's own events only.
namespace {

// what is still being written into slot k (by the snapshot that used it last) has landed
int rec_wait(edynhip_world *w, int k) {
    for (Shard &s : w->shards) {
        if (!s.rec_pending[k]) continue;
        W_HIP(w, hipSetDevice(s.device));
        W_HIP(w, hipEventSynchronize(s.rec_ev[k]));
        s.rec_pending[k] = false;
    }
    if (w->rec[k].ev_pending) {
        W_HIP(w, hipSetDevice(w->devices[0]));
        W_HIP(w, hipEventSynchronize(w->rec_ev_done[k]));
        w->rec[k].ev_pending = false;
    }
    return EDYNHIP_OK;
}

// The record of a body that no context holds, from the world's own arrays and the scene description. By build_shard's rule every body
// is held by its owner or, replicated, by shard 0, so today this writes nothing; it keeps the slot complete should a partition ever leave
// a body out. Such a body is simulated by nobody: the state is the gathered one; the presentation follows dm::integrate's formula.
void host_record(const edynhip_world *w, uint32_t g, float dt, edynhip_body_record &o) {
    const HostScene &sc = w->scene;
    const float *p = &w->pos[3 * (size_t)g], *q = &w->orn[4 * (size_t)g], *v = &w->linvel[3 * (size_t)g], *a = &w->angvel[3 * (size_t)g];
    std::memcpy(o.pos, p, 12); std::memcpy(o.orn, q, 16); std::memcpy(o.linvel, v, 12); std::memcpy(o.angvel, a, 12);
    for (int d = 0; d < 3; ++d) o.present_pos[d] = p[d] + v[d] * dt;
    const float ws = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const float t = ws < 0.001f ? 0.5f * dt - dt * dt * dt * (1.0f / 48.0f) * ws * ws : (float)std::sin((double)(0.5f * ws * dt)) / ws;
    const float r[4] = {a[0] * t, a[1] * t, a[2] * t, (float)std::cos((double)(0.5f * ws * dt))};
    float m[4] = {r[3] * q[0] + r[0] * q[3] + r[1] * q[2] - r[2] * q[1], r[3] * q[1] + r[1] * q[3] + r[2] * q[0] - r[0] * q[2],
                  r[3] * q[2] + r[2] * q[3] + r[0] * q[1] - r[1] * q[0], r[3] * q[3] - r[0] * q[0] - r[1] * q[1] - r[2] * q[2]};
    const float len = std::sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2] + m[3] * m[3]);
    for (int d = 0; d < 4; ++d) o.present_orn[d] = m[d] / len;
    const float *c = sc.com.empty() ? nullptr : &sc.com[3 * (size_t)g];
    const bool has_origin = c && !(c[0] == 0 && c[1] == 0 && c[2] == 0);
    std::memcpy(o.origin, p, 12);
    if (has_origin) {   // origin = pos + rotate(orn, -com)
        const float x[3] = {-c[0], -c[1], -c[2]}, u[3] = {2.0f * q[0], 2.0f * q[1], 2.0f * q[2]};
        const float k[3] = {q[1] * x[2] - q[2] * x[1] + q[3] * x[0], q[2] * x[0] - q[0] * x[2] + q[3] * x[1], q[0] * x[1] - q[1] * x[0] + q[3] * x[2]};
        o.origin[0] = p[0] + (x[0] + (u[1] * k[2] - u[2] * k[1])); o.origin[1] = p[1] + (x[1] + (u[2] * k[0] - u[0] * k[2])); o.origin[2] = p[2] + (x[2] + (u[0] * k[1] - u[1] * k[0]));
    }
    o.flags = (sc.kind[g] == EDYNHIP_KIND_DYNAMIC && !w->is_removed(g) ? EDYNHIP_RECORD_DYNAMIC : 0u) | (has_origin ? EDYNHIP_RECORD_HAS_ORIGIN : 0u) |
              (w->is_removed(g) ? EDYNHIP_RECORD_REMOVED : 0u);
}

}  // namespace

extern "C" {

int edynhip_world_snapshot_records(edynhip_world *w, float present_dt, uint32_t max_events, uint32_t flags) {
    static_assert(sizeof(edynhip_body_record) == 96 && sizeof(ContactEvent) == 24, "slot layout");
    if (!w) return EDYNHIP_ERR_INVALID;
    if (flags & ~(uint32_t)EDYNHIP_SNAPSHOT_DIRECT) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_snapshot_records: flags must be 0 or EDYNHIP_SNAPSHOT_DIRECT");
    EH_TRY(ensure_built(w));
    const int k = (w->rec_last + 1) & 1, home = w->devices[0];
    edynhip_world::RecSlot &sl = w->rec[k];
    EH_TRY(rec_wait(w, k));   // (a snapshot that was never mapped may still be writing into this slot)
    const uint32_t n = w->scene.n;
    const uint32_t copy = w->events_on() ? std::min(max_events, w->ev_n) : 0u;
    if (!sl.host || n > sl.body_cap || copy > sl.ev_cap) {
        // the views into this slot expired with this call (valid until the next-but-one): it may move. Portable and mapped: every shard's
        // device stores into it.
        // (sized for the scene as it stands; a slot that has to grow - bodies were added to the running world - takes head-room)
        const uint32_t body_cap = n <= sl.body_cap ? sl.body_cap : sl.body_cap ? n + n / 4 + 64 : n;
        const uint32_t ev_cap = w->events_on() ? std::max(std::max<uint32_t>(copy, 4096u), sl.ev_cap) : 0u;
        W_HIP(w, hipSetDevice(home));
        if (sl.host) (void)hipHostFree(sl.host);
        sl.host = nullptr; sl.body_cap = sl.ev_cap = 0;
        W_HIP(w, hipHostMalloc((void **)&sl.host, (size_t)body_cap * sizeof(edynhip_body_record) + (size_t)ev_cap * sizeof(ContactEvent), hipHostMallocPortable | hipHostMallocMapped));
        sl.body_cap = body_cap; sl.ev_cap = ev_cap;
    }
    size_t reported = 0;
    for (Shard &s : w->shards) {   // every shard's pack on its own stream, behind its last step and its event append
        if (!s.ctx || s.local_ids.empty()) continue;
        W_HIP(w, hipSetDevice(s.device));
        if (!s.rec_ev[k]) W_HIP(w, hipEventCreateWithFlags(&s.rec_ev[k], hipEventDisableTiming));
        void *dst = nullptr;
        W_HIP(w, hipHostGetDevicePointer(&dst, sl.host, 0));
        const int rc = shard_pack_records(s.ctx, s.ids_dev, (uint32_t)s.local_ids.size(), n, present_dt, dst);
        if (rc != EDYNHIP_OK) return w->fail(rc, std::string("edynhip_world_snapshot_records: ") + edynhip_last_error(s.ctx));
        W_HIP(w, hipEventRecord(s.rec_ev[k], s.ctx->stream));
        s.rec_pending[k] = true;
        reported += s.owned_local.size();
    }
    if (copy) {   // the event block: one copy from the home device's list, after every shard's append
        W_HIP(w, hipSetDevice(home));
        if (!w->rec_stream) W_HIP(w, hipStreamCreateWithFlags(&w->rec_stream, hipStreamNonBlocking));
        if (!w->rec_ev_done[k]) W_HIP(w, hipEventCreateWithFlags(&w->rec_ev_done[k], hipEventDisableTiming));
        for (Shard &s : w->shards) if (s.rec_pending[k]) W_HIP(w, hipStreamWaitEvent(w->rec_stream, s.rec_ev[k], 0));
        W_HIP(w, hipMemcpyAsync(sl.host + (size_t)sl.body_cap * sizeof(edynhip_body_record), w->ev_list.p, (size_t)copy * sizeof(ContactEvent), hipMemcpyDeviceToHost, w->rec_stream));
        W_HIP(w, hipEventRecord(w->rec_ev_done[k], w->rec_stream));
        sl.ev_pending = true;
    }
    if (reported != n) {   // a body no shard reports (every shard reports a body at most once): the world writes its record
        std::vector<uint8_t> seen(n, 0);
        for (const Shard &s : w->shards) if (s.ctx) for (uint32_t l : s.owned_local) seen[s.local_ids[l]] = 1;
        for (uint32_t g = 0; g < n; ++g) if (!seen[g]) host_record(w, g, present_dt, ((edynhip_body_record *)sl.host)[g]);
    }
    sl.bodies = n; sl.step = w->step_count; sl.events = copy;
    sl.total = w->events_on() ? (uint32_t)std::min<uint64_t>(w->ev_occurred, 0xFFFFFFFFull) : 0u;
    sl.tombs = (uint32_t)w->tombs.size();
    w->rec_last = k;
    return EDYNHIP_OK;
}

int edynhip_world_snapshot_map(edynhip_world *w, edynhip_record_view *view) {
    if (!w || !view) return EDYNHIP_ERR_INVALID;
    if (w->rec_last < 0) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_snapshot_map: no record snapshot was taken");
    const int k = w->rec_last;
    edynhip_world::RecSlot &sl = w->rec[k];
    EH_TRY(rec_wait(w, k));   // that snapshot only
    edynhip_body_record *rec = (edynhip_body_record *)sl.host;
    // a context rebuilt after the step that dropped a removed body holds the slot as a plain shapeless static body: the tombstone is the world's
    for (uint32_t t = 0; t < sl.tombs && t < w->tombs.size(); ++t) if (w->tombs[t] < sl.bodies) rec[w->tombs[t]].flags |= EDYNHIP_RECORD_REMOVED;
    view->records = rec;
    view->num_bodies = sl.bodies;
    view->step_index = sl.step;
    view->events = w->events_on() ? (const edynhip_contact_event *)(sl.host + (size_t)sl.body_cap * sizeof(edynhip_body_record)) : nullptr;
    view->num_events = sl.events;
    view->total_events = sl.total;
    return EDYNHIP_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ queries on the world
// Every shard answers for its own bodies with the single context's kernels (eh::shard_raycast / shard_query_*), on its pool thread and
// its context's stream; local indices become global ones on the shard's device; the answers meet on the home device (devices[0]),
// where world_query.hip merges them into what ONE context holding the whole scene returns. A shard on the home device reads the
// caller's arrays and writes its answer in place; any other shard's queries and answers travel device to device.
namespace {

constexpr uint32_t kWorldChunk = 1u << 20;   // rays per pass (raycast.hip kChunk)
constexpr unsigned long long kSat32 = 0xFFFFFFFFull;

int query_begin(edynhip_world *w) {
    EH_TRY(ensure_built(w));
    W_HIP(w, hipSetDevice(w->devices[0]));
    if (!w->qstream) W_HIP(w, hipStreamCreateWithFlags(&w->qstream, hipStreamNonBlocking));
    if (!w->q_pin) W_HIP(w, hipHostMalloc((void **)&w->q_pin, 2 * sizeof(unsigned long long), hipHostMallocDefault));
    return EDYNHIP_OK;
}

// the shards that hold bodies, and each one's slot among them
uint32_t active_slots(const edynhip_world *w, std::vector<int32_t> &slot) {
    uint32_t k = 0;
    slot.assign(w->shards.size(), -1);
    for (uint32_t r = 0; r < w->shards.size(); ++r) if (w->shards[r].ctx && !w->shards[r].local_ids.empty()) slot[r] = (int32_t)k++;
    return k;
}

// m <= kWorldChunk rays, arrays on the home device
int world_raycast_chunk(edynhip_world *w, uint32_t m, const float4 *p0, const float4 *p1, uint32_t num_ignore, const uint32_t *ignore, uint32_t flags, void *out) {
    const int home = w->devices[0];
    std::vector<int32_t> slot;
    const uint32_t A = active_slots(w, slot);
    W_HIP(w, hipSetDevice(home));
    W_HIP(w, dev_grow(w->h_hits, (size_t)std::max(A, 1u) * m * sizeof(edynhip_raycast_hit)));
    w->pool->run([&](uint32_t r) {
        Shard &s = w->shards[r];
        if (slot[r] < 0 || s.rc != EDYNHIP_OK) return;
        SH_HIP(s, hipSetDevice(s.device));
        hipStream_t st = s.ctx->stream;
        const uint32_t nl = (uint32_t)s.local_ids.size();
        uint8_t *dst = (uint8_t *)w->h_hits.p + (size_t)slot[r] * m * sizeof(edynhip_raycast_hit);
        const void *a = p0, *b = p1;
        void *o = dst;
        if (s.device != home) {
            SH_HIP(s, dev_grow(s.q_in, 2 * (size_t)m * sizeof(float4)));
            SH_HIP(s, dev_grow(s.q_out, (size_t)m * sizeof(edynhip_raycast_hit)));
            SH_HIP(s, hipMemcpyPeerAsync(s.q_in.p, s.device, p0, home, (size_t)m * sizeof(float4), st));
            SH_HIP(s, hipMemcpyPeerAsync((float4 *)s.q_in.p + m, s.device, p1, home, (size_t)m * sizeof(float4), st));
            a = s.q_in.p; b = (const float4 *)s.q_in.p + m; o = s.q_out.p;
        }
        s.q_ignore.clear();
        for (uint32_t k = 0; k < num_ignore; ++k)
            if (ignore[k] < w->scene.n && s.to_local[ignore[k]] >= 0) s.q_ignore.push_back((uint32_t)s.to_local[ignore[k]]);
        SH_TRY(s, shard_raycast(s.ctx, m, a, b, (uint32_t)s.q_ignore.size(), s.q_ignore.data(), flags, o));
        wq_translate_hits(st, m, o, s.ids_dev, nl);
        SH_HIP(s, hipGetLastError());
        if (s.device != home) SH_HIP(s, hipMemcpyPeerAsync(dst, home, o, s.device, (size_t)m * sizeof(edynhip_raycast_hit), st));
        SH_HIP(s, hipStreamSynchronize(st));
    });
    EH_TRY(shard_error(w));
    W_HIP(w, hipSetDevice(home));
    wq_rc_merge(w->qstream, A, m, w->h_hits.p, m, out);
    W_HIP(w, hipGetLastError());
    W_HIP(w, hipStreamSynchronize(w->qstream));   // (the shards' answers are overwritten by the next pass)
    return EDYNHIP_OK;
}

// The count pass: offsets [n + 1] and total [1] on the home device; the 64-bit total in *tot. The shards keep their counts and lists for
// world_query_fill.
int world_query_count(edynhip_world *w, int category, uint32_t n, const float4 *boxes, uint32_t flags, uint32_t *offsets, uint32_t *total, unsigned long long *tot) {
    const int home = w->devices[0];
    std::vector<int32_t> slot;
    const uint32_t A = n ? active_slots(w, slot) : 0u;
    W_HIP(w, hipSetDevice(home));
    W_HIP(w, dev_grow(w->h_cnt, (size_t)std::max(A, 1u) * std::max(n, 1u) * sizeof(uint32_t)));
    if (A) w->pool->run([&](uint32_t r) {
        Shard &s = w->shards[r];
        if (slot[r] < 0 || s.rc != EDYNHIP_OK) return;
        SH_HIP(s, hipSetDevice(s.device));
        hipStream_t st = s.ctx->stream;
        s.q_boxes = boxes;
        if (s.device != home) {
            SH_HIP(s, dev_grow(s.q_in, 2 * (size_t)n * sizeof(float4)));
            SH_HIP(s, hipMemcpyPeerAsync(s.q_in.p, s.device, boxes, home, 2 * (size_t)n * sizeof(float4), st));
            s.q_boxes = s.q_in.p;
        }
        const unsigned long long *t64 = nullptr;
        SH_TRY(s, shard_query_count(s.ctx, category, n, s.q_boxes, flags, &s.q_cnt, &s.q_off, &t64));
        SH_HIP(s, hipMemcpyAsync(s.q_tot, t64, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        if (s.device != home)
            SH_HIP(s, hipMemcpyPeerAsync((uint32_t *)w->h_cnt.p + (size_t)slot[r] * n, home, s.q_cnt, s.device, (size_t)n * sizeof(uint32_t), st));
        SH_HIP(s, hipStreamSynchronize(st));
    });
    EH_TRY(shard_error(w));
    WqShards sh{};
    sh.W = A;
    for (uint32_t r = 0; r < w->shards.size() && A; ++r)
        if (slot[r] >= 0) sh.cnt[slot[r]] = w->shards[r].device == home ? w->shards[r].q_cnt : (const uint32_t *)w->h_cnt.p + (size_t)slot[r] * n;
    W_HIP(w, hipSetDevice(home));
    const size_t nb = (size_t)n / 256 + 2;   // scratch: total | block sums | their scan | summed counts
    W_HIP(w, dev_grow(w->h_scan, (1 + 2 * nb) * sizeof(unsigned long long) + (size_t)std::max(n, 1u) * sizeof(uint32_t)));
    unsigned long long *t64 = (unsigned long long *)w->h_scan.p, *bsum = t64 + 1, *boff = bsum + nb;
    wq_qa_offsets(w->qstream, sh, n, (uint32_t *)(boff + nb), bsum, boff, t64, offsets, total);
    W_HIP(w, hipGetLastError());
    W_HIP(w, hipMemcpyAsync(w->q_pin, t64, sizeof(unsigned long long), hipMemcpyDeviceToHost, w->qstream));
    W_HIP(w, hipStreamSynchronize(w->qstream));
    *tot = w->q_pin[0];
    return EDYNHIP_OK;
}

// The fill pass of the queries counted last: ids [capacity] on the home device; nothing is written at or beyond capacity.
int world_query_fill(edynhip_world *w, int category, uint32_t n, uint32_t flags, const uint32_t *offsets, uint32_t *ids, uint32_t capacity) {
    const int home = w->devices[0];
    std::vector<int32_t> slot;
    const uint32_t A = active_slots(w, slot);
    if (n == 0 || A == 0 || capacity == 0) return EDYNHIP_OK;
    // a shard's own list is sized by its own total: it must be addressable with 32 bits
    std::vector<size_t> base(w->shards.size(), 0);
    size_t remote_ids = 0;
    for (uint32_t r = 0; r < w->shards.size(); ++r) {
        if (slot[r] < 0) continue;
        if (*w->shards[r].q_tot >= kSat32) return w->fail(EDYNHIP_ERR_CAPACITY, "edynhip_world_query_aabb: a shard reports 2^32 - 1 hits or more");
        if (w->shards[r].device != home) { base[r] = remote_ids; remote_ids += (size_t)*w->shards[r].q_tot; }
    }
    W_HIP(w, hipSetDevice(home));
    W_HIP(w, dev_grow(w->h_ids, std::max<size_t>(remote_ids, 1) * sizeof(uint32_t)));
    W_HIP(w, dev_grow(w->h_off, (size_t)A * ((size_t)n + 1) * sizeof(uint32_t)));
    w->pool->run([&](uint32_t r) {
        Shard &s = w->shards[r];
        if (slot[r] < 0 || s.rc != EDYNHIP_OK) return;
        SH_HIP(s, hipSetDevice(s.device));
        hipStream_t st = s.ctx->stream;
        const size_t t = (size_t)*s.q_tot;
        if (t == 0 && s.device == home) return;
        SH_HIP(s, dev_grow(s.q_ids, std::max<size_t>(t, 1) * sizeof(uint32_t)));
        SH_TRY(s, shard_query_fill(s.ctx, category, n, s.q_boxes, flags, (uint32_t *)s.q_ids.p, (uint32_t)t));
        wq_translate_ids(st, (uint32_t *)s.q_ids.p, t, s.ids_dev, (uint32_t)s.local_ids.size());   // (island labels are body indices too)
        SH_HIP(s, hipGetLastError());
        if (s.device != home) {
            SH_HIP(s, hipMemcpyPeerAsync((uint32_t *)w->h_off.p + (size_t)slot[r] * ((size_t)n + 1), home, s.q_off, s.device, ((size_t)n + 1) * sizeof(uint32_t), st));
            if (t) SH_HIP(s, hipMemcpyPeerAsync((uint32_t *)w->h_ids.p + base[r], home, s.q_ids.p, s.device, t * sizeof(uint32_t), st));
        }
        SH_HIP(s, hipStreamSynchronize(st));
    });
    EH_TRY(shard_error(w));
    WqShards sh{};
    sh.W = A;
    for (uint32_t r = 0; r < w->shards.size(); ++r) {
        if (slot[r] < 0) continue;
        const Shard &s = w->shards[r];
        const bool here = s.device == home;
        sh.off[slot[r]] = here ? s.q_off : (const uint32_t *)w->h_off.p + (size_t)slot[r] * ((size_t)n + 1);
        sh.ids[slot[r]] = here ? (const uint32_t *)s.q_ids.p : (const uint32_t *)w->h_ids.p + base[r];
    }
    W_HIP(w, hipSetDevice(home));
    for (uint32_t r = 0; r < w->shards.size(); ++r)
        if (slot[r] >= 0) wq_qa_merge(w->qstream, sh, (uint32_t)slot[r], n, (uint32_t)*w->shards[r].q_tot, offsets, ids, capacity);
    W_HIP(w, hipGetLastError());
    W_HIP(w, hipStreamSynchronize(w->qstream));
    return EDYNHIP_OK;
}

int check_world_query(edynhip_world *w, int category, uint32_t flags, const char *who) {
    if (category != EDYNHIP_QUERY_PROCEDURAL && category != EDYNHIP_QUERY_NON_PROCEDURAL && category != EDYNHIP_QUERY_ISLANDS)
        return w->fail(EDYNHIP_ERR_INVALID, std::string(who) + ": unknown category");
    if (flags & ~(uint32_t)EDYNHIP_QUERY_BRUTE_FORCE) return w->fail(EDYNHIP_ERR_INVALID, std::string(who) + ": unknown flag bits");
    return EDYNHIP_OK;
}

}  // namespace

extern "C" {

int edynhip_world_raycast_device(edynhip_world *w, uint32_t n, const void *p0_f4, const void *p1_f4, uint32_t num_ignore, const uint32_t *ignore,
                                 uint32_t flags, void *out) {
    if (!w || (n && (!p0_f4 || !p1_f4 || !out)) || (num_ignore && !ignore)) return EDYNHIP_ERR_INVALID;
    if (flags & ~(uint32_t)EDYNHIP_RAYCAST_BRUTE_FORCE) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_raycast_device: unknown flag bits");
    if (n == 0) return EDYNHIP_OK;
    EH_TRY(query_begin(w));
    for (uint32_t off = 0; off < n; off += kWorldChunk)
        EH_TRY(world_raycast_chunk(w, std::min(kWorldChunk, n - off), (const float4 *)p0_f4 + off, (const float4 *)p1_f4 + off, num_ignore, ignore, flags,
                                   (edynhip_raycast_hit *)out + off));
    return EDYNHIP_OK;
}

int edynhip_world_raycast(edynhip_world *w, uint32_t n, const float *p0, const float *p1, uint32_t num_ignore, const uint32_t *ignore, uint32_t flags,
                          edynhip_raycast_hit *out) {
    if (!w || (n && (!p0 || !p1 || !out)) || (num_ignore && !ignore)) return EDYNHIP_ERR_INVALID;
    if (flags & ~(uint32_t)EDYNHIP_RAYCAST_BRUTE_FORCE) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_raycast: unknown flag bits");
    if (n == 0) return EDYNHIP_OK;
    EH_TRY(query_begin(w));
    const uint32_t chunk = std::min(n, kWorldChunk);
    W_HIP(w, dev_grow(w->h_in, 2 * (size_t)chunk * sizeof(float4)));
    W_HIP(w, dev_grow(w->h_out, (size_t)chunk * sizeof(edynhip_raycast_hit)));
    w->q_stage.resize(2 * (size_t)chunk);
    for (uint32_t off = 0; off < n; off += kWorldChunk) {
        const uint32_t m = std::min(kWorldChunk, n - off);
        for (uint32_t r = 0; r < m; ++r) {
            const float *q0 = p0 + 3 * ((size_t)off + r), *q1 = p1 + 3 * ((size_t)off + r);
            w->q_stage[r] = make_float4(q0[0], q0[1], q0[2], 0.0f);
            w->q_stage[(size_t)chunk + r] = make_float4(q1[0], q1[1], q1[2], 0.0f);
        }
        W_HIP(w, hipSetDevice(w->devices[0]));
        float4 *d = (float4 *)w->h_in.p;
        W_HIP(w, hipMemcpyAsync(d, w->q_stage.data(), (size_t)m * sizeof(float4), hipMemcpyHostToDevice, w->qstream));
        W_HIP(w, hipMemcpyAsync(d + chunk, w->q_stage.data() + chunk, (size_t)m * sizeof(float4), hipMemcpyHostToDevice, w->qstream));
        W_HIP(w, hipStreamSynchronize(w->qstream));
        EH_TRY(world_raycast_chunk(w, m, d, d + chunk, num_ignore, ignore, flags, w->h_out.p));
        W_HIP(w, hipMemcpyAsync(out + off, w->h_out.p, (size_t)m * sizeof(edynhip_raycast_hit), hipMemcpyDeviceToHost, w->qstream));
        W_HIP(w, hipStreamSynchronize(w->qstream));
    }
    return EDYNHIP_OK;
}

int edynhip_world_query_aabb_device(edynhip_world *w, int category, uint32_t n, const void *boxes_f4, uint32_t flags, void *offsets, void *ids,
                                    uint32_t capacity, void *total) {
    if (!w || !offsets || !total || (n && !boxes_f4)) return EDYNHIP_ERR_INVALID;
    EH_TRY(check_world_query(w, category, flags, "edynhip_world_query_aabb_device"));
    EH_TRY(query_begin(w));
    unsigned long long tot = 0;
    EH_TRY(world_query_count(w, category, n, (const float4 *)boxes_f4, flags, (uint32_t *)offsets, (uint32_t *)total, &tot));
    if (!ids || capacity == 0 || tot == 0) return EDYNHIP_OK;
    return world_query_fill(w, category, n, flags, (const uint32_t *)offsets, (uint32_t *)ids, capacity);
}

int edynhip_world_query_aabb(edynhip_world *w, int category, uint32_t n, const float *boxes6, uint32_t flags, uint32_t *offsets, uint32_t *ids,
                             uint32_t capacity, uint32_t *total) {
    if (!w || !offsets || !total || (n && !boxes6)) return EDYNHIP_ERR_INVALID;
    EH_TRY(check_world_query(w, category, flags, "edynhip_world_query_aabb"));
    EH_TRY(query_begin(w));
    W_HIP(w, dev_grow(w->h_in, std::max<size_t>(2 * (size_t)n, 1) * sizeof(float4)));
    W_HIP(w, dev_grow(w->h_off_out, ((size_t)n + 2) * sizeof(uint32_t)));
    w->q_stage.resize(2 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
        const float *b = boxes6 + 6 * (size_t)i;
        w->q_stage[2 * (size_t)i] = make_float4(b[0], b[1], b[2], 0.0f);
        w->q_stage[2 * (size_t)i + 1] = make_float4(b[3], b[4], b[5], 0.0f);
    }
    if (n) W_HIP(w, hipMemcpyAsync(w->h_in.p, w->q_stage.data(), 2 * (size_t)n * sizeof(float4), hipMemcpyHostToDevice, w->qstream));
    W_HIP(w, hipStreamSynchronize(w->qstream));
    uint32_t *d_off = (uint32_t *)w->h_off_out.p;
    unsigned long long tot = 0;
    EH_TRY(world_query_count(w, category, n, (const float4 *)w->h_in.p, flags, d_off, d_off + n + 1, &tot));
    W_HIP(w, hipMemcpyAsync(offsets, d_off, ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, w->qstream));
    W_HIP(w, hipStreamSynchronize(w->qstream));
    *total = tot >= kSat32 ? 0xFFFFFFFFu : (uint32_t)tot;
    if (!ids) return EDYNHIP_OK;
    if (tot > capacity || tot >= kSat32) return w->fail(EDYNHIP_ERR_CAPACITY, "edynhip_world_query_aabb: capacity (offsets and total are valid: size ids by *total and ask again)");
    if (tot == 0) return EDYNHIP_OK;
    W_HIP(w, dev_grow(w->h_ids_out, (size_t)tot * sizeof(uint32_t)));
    EH_TRY(world_query_fill(w, category, n, flags, d_off, (uint32_t *)w->h_ids_out.p, (uint32_t)tot));
    W_HIP(w, hipMemcpyAsync(ids, w->h_ids_out.p, (size_t)tot * sizeof(uint32_t), hipMemcpyDeviceToHost, w->qstream));
    W_HIP(w, hipStreamSynchronize(w->qstream));
    return EDYNHIP_OK;
}

}  // extern "C"
