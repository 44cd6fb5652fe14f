// What the files of the multi-device world (multi.hip, multi_shard.hip, multi_partition.hip, multi_edit.hip, multi_body_edit.hip, multi_materials.hip,
// multi_records.hip, multi_query.hip) share: the world and its shards, what travels through a re-partition, the error macros, and the functions that cross a
// file boundary. Internal: nothing here is part of the C-ABI.
#pragma once
#include "ctx.hpp"
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

// multi_partition.hip, launched by gather_shard (multi_shard.hip): how far a body's AABB has grown out of the one recorded at the last check
__global__ void k_shard_growth(uint32_t n, Bodies b, const float4 *__restrict__ amin0, const float4 *__restrict__ amax0, uint32_t *out_bits);

namespace world {

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
    // materials (multi_materials.hip), each empty until it is first set: per body spin, roll, stiffness, damping; per body the material id
    // (0xFFFF = unassigned); the mix table as the ordered list of insertions (id0, id1, material6), replayed on every context that is built
    std::vector<float> mat_extras;
    std::vector<uint32_t> mat_id;
    struct MixEntry { uint32_t id0, id1; float m[6]; };
    std::vector<MixEntry> mix;
};

// What a shard holds on its device for as long as its context lives. Owners release on the device that is current, so these are given up
// in one place only: free_shard, which makes the shard's device current and lets the context's stream run dry first. Nothing is
// allocated before the shard has a context, and edynhip_world_destroy calls free_shard for every shard before it deletes the world: the
// destructor of a Shard always finds them empty.
struct ShardResources {
    DeviceBuf<float> pack_dev; PinnedBuf<float> pack_host;   // [n_local][13]
    // monitor scratch on the device: [0] growth bits, [1] island count | per label 3 lo + 3 hi ordered bits | out labels | out boxes | amin0 | amax0
    DeviceBuf<uint32_t> mon_dev; PinnedBuf<uint32_t> mon_host;
    // queries (edynhip_world_raycast / edynhip_world_query_aabb). Per context, [cap]: local_ids on the device, the bit per local body this
    // shard answers for, island labels carried through a re-partition. Scratch: the queries and the local results of a shard that is not on
    // the home device, the hit lists of any shard; the last count pass (the context's buffers) and its 64-bit total (pinned).
    DeviceBuf<uint32_t> ids_dev, ans_dev, qisl_dev;
    GrowBuf q_in, q_out, q_ids;
    const void *q_boxes = nullptr;
    const uint32_t *q_cnt = nullptr, *q_off = nullptr;
    PinnedBuf<unsigned long long> q_tot;
    // contact events (EDYNHIP_FLAG_CONTACT_EVENTS only): the last step's event count, fetched with the state (pinned), and how many of them
    // the shard holds; the step's events in global indices (device, [event_cap]); the point ids of `manifolds` as [m][4] on the device
    PinnedBuf<uint32_t> ev_cnt_host; uint32_t ev_held = 0;
    GrowBuf ev_out, pid_buf;
    // materials: the point extras of `manifolds` as [m][4][2] float4 rows (world_rules.hpp) on the device, and pinned: what a collect
    // read (Shard::xrows of them) until build_shard writes the rows it injects there
    GrowBuf xtr_buf; PinnedBuf<float> xtr_host; size_t xtr_host_cap = 0;
    // record hand-over (edynhip_world_snapshot_records): per pinned slot the event that completes this shard's pack, and whether one is out
    Event rec_ev[2];
    bool rec_pending[2] = {false, false};
};

struct Shard {   // (move-only: its resources are)
    edynhip_ctx *ctx = nullptr;
    int device = 0;
    std::vector<uint32_t> local_ids;      // local index -> global index (ascending)
    std::vector<int32_t> to_local;        // global index -> local index or -1
    std::vector<uint32_t> owned_local;    // local indices of the bodies whose state this shard contributes
    std::vector<uint32_t> local_joints;   // local joint index -> global joint index
    ShardResources res;
    uint32_t cap = 0, joint_cap = 0, meshes_created = 0;
    uint32_t want_bodies = 0, want_joints = 0;   // head-room an edit asks of the next build_shard beyond what the scene holds now
    int rc = EDYNHIP_OK;
    std::string err;
    uint64_t paths_gone = 0;              // edynhip_debug_paths of the contexts this shard had before (free_shard)
    // collected for a re-partition
    std::vector<uint32_t> labels; std::vector<float> aabb; std::vector<edynhip_manifold> manifolds; std::vector<float> imp24, imp10; std::vector<uint8_t> asleep;
    std::vector<uint32_t> sleep_label; std::vector<double> sleep_since; double sleep_clock = 0;
    std::vector<uint32_t> q_ignore;       // queries: the caller's ignore list in local indices
    std::vector<uint64_t> pids;           // contact events: the point ids of `manifolds` as [m][4]
    size_t xrows = 0;                     // materials: how many of `manifolds` have their extras row in res.xtr_host, [m][32] (world_rules.hpp); 0 or all
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

}  // namespace world
}  // namespace eh

struct edynhip_world {   // (the member order keeps `pool` - the shards' threads - destroyed before `shards`)
    edynhip_config cfg{};
    eh::Knobs knobs{};   // read when the world is created (world_serial, world_trace; every shard context reads its own)
    std::vector<int> devices;
    std::vector<eh::world::Shard> shards;
    std::unique_ptr<eh::world::Pool> pool;
    eh::world::HostScene scene;
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
    eh::Stream qstream;
    eh::GrowBuf h_hits, h_cnt, h_off, h_ids, h_scan, h_in, h_out, h_off_out, h_ids_out;
    eh::PinnedBuf<unsigned long long> q_pin;        // pinned: the 64-bit total of the last count
    std::vector<uint32_t> query_labels;            // island labels (global) of the state the shards were last rebuilt from
    std::vector<float4> q_stage;
    // contact events (EDYNHIP_FLAG_CONTACT_EVENTS only): the events of the last edynhip_world_step call, global indices, on the home device -
    // every step appends every shard's block -, whether a shard's own list overflowed in that call, and the steps since the scene was described
    eh::GrowBuf ev_list;
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
    // materials: some body has had a contact_extras material since the scene was described (points mixed from it may live on after the
    // material is gone) - with the mix table's entries what decides whether a re-partition carries the points' extras
    bool extras_seen = false;
    bool carries_extras() const { return eh::extras_carry_needed(extras_seen, scene.mix.size()); }
    // record hand-over (edynhip_world_snapshot_records / _map): two pinned slots used alternately, each [records: body_cap x 96 B | events:
    // ev_cap x 24 B], allocated portable and mapped so that every shard's device stores its records into them; what the slot holds; the home
    // device's side stream and per slot the event that completes the copy of the event block; the events that OCCURRED in the last
    // edynhip_world_step call (the sum of the shards' own counts, also where a shard's list overflowed); every body removed so far.
    struct RecSlot {
        eh::PinnedBuf<uint8_t> host;
        uint32_t body_cap = 0, ev_cap = 0;
        uint32_t bodies = 0, step = 0, events = 0, total = 0, tombs = 0;
        bool ev_pending = false;
    };
    RecSlot rec[2];
    int rec_last = -1;
    eh::Stream rec_stream;
    eh::Event rec_ev_done[2];
    uint64_t ev_occurred = 0;
    std::vector<uint32_t> tombs;
};

namespace eh {
namespace world {

inline int shard_error(edynhip_world *w) {
    for (uint32_t r = 0; r < w->shards.size(); ++r)
        if (w->shards[r].rc != EDYNHIP_OK) return w->fail(w->shards[r].rc, "shard " + std::to_string(r) + ": " + w->shards[r].err);
    return EDYNHIP_OK;
}
#define SH_TRY(s, expr) do { int r__ = (expr); if (r__ != EDYNHIP_OK) { (s).rc = r__; (s).err = (s).ctx ? edynhip_last_error((s).ctx) : edynhip_last_error(nullptr); return; } } while (0)
#define W_HIP(w, call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return (w)->fail(EDYNHIP_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); } while (0)
#define SH_HIP(s, call) do { hipError_t e__ = (call); if (e__ != hipSuccess) { (s).rc = EDYNHIP_ERR_HIP; (s).err = std::string(#call) + ": " + hipGetErrorString(e__); return; } } while (0)

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
    // materials: the extras rows of the carried points by the same key (world_rules.hpp: the row layout) - a rebuilt shard puts them back over
    // what edynhip_set_manifolds mixed from today's materials. Empty in a world without materials (extras_carry_needed).
    std::unordered_map<uint64_t, std::array<float, kExtrasRowFloats>> point_extras;
};

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

inline void refresh_bodies_per_shard(edynhip_world *w) {
    for (uint32_t r = 0; r < w->shards.size(); ++r) w->stats.bodies_per_shard[r < 16 ? r : 15] = (uint32_t)w->shards[r].owned_local.size();
}

// ---- the functions that cross a file boundary (they were one file's statics: kept out of the library's exported symbols)
// multi.hip: the scene description and the first build
EH_LOCAL int ensure_built(edynhip_world *w);
EH_LOCAL MeshRadii scene_meshes(const HostScene &sc);
EH_LOCAL void scene_append_bodies(edynhip_world *w, uint32_t k, const edynhip_bodies *in);
EH_LOCAL void scene_append_joints(HostScene &sc, uint32_t n, const edynhip_joints *in);
EH_LOCAL HostScene::Def make_def(uint32_t joint, const float *frame_a9, const float *frame_b9, const float *params, bool generic);
EH_LOCAL void finish_tombstones(edynhip_world *w);
EH_LOCAL int append_event_blocks(edynhip_world *w);
// multi_edit.hip: the safety condition after an edit that can bring islands of different shards together
EH_LOCAL int edit_approach(edynhip_world *w, bool &moved);
// multi_shard.hip: one shard - its context, what goes up to it and what comes back
EH_LOCAL int shard_filter_thunk(void *user, uint32_t body, uint32_t other);
EH_LOCAL void free_shard(Shard &s);
EH_LOCAL void upload_query_tables(edynhip_world *w, uint32_t r, uint32_t l0, const std::vector<uint32_t> *island = nullptr);
EH_LOCAL void build_shard(edynhip_world *w, uint32_t r, const Carry &carry, bool from_state);
EH_LOCAL void gather_shard(edynhip_world *w, uint32_t r, bool with_growth);
EH_LOCAL void collect_shard(edynhip_world *w, uint32_t r, bool light, bool heavy, bool extras = false);
EH_LOCAL void merge_manifolds(edynhip_world *w, std::vector<edynhip_manifold> &out, std::vector<uint64_t> *ids = nullptr, std::vector<float> *extras = nullptr);
EH_LOCAL void apply_materials(edynhip_world *w, Shard &s);
// multi_partition.hip: the approach check and the re-partition
EH_LOCAL int approach_check(edynhip_world *w, bool &close, bool per_body = false, const std::vector<IslandBox> *host_boxes = nullptr);
EH_LOCAL int rebuild(edynhip_world *w, const Carry &carry, bool from_state, const std::vector<uint8_t> *only = nullptr);
EH_LOCAL int repartition(edynhip_world *w, bool sticky, const std::vector<std::array<uint32_t, 2>> *edges = nullptr, const std::vector<uint8_t> *force = nullptr, bool from_edit = false);

}  // namespace world
}  // namespace eh
