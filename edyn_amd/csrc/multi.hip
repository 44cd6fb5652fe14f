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
// are plain C++ in world_rules.hpp. What touches a device is split by concern, with what the files share in multi.hpp: this file holds the
// world's life cycle, the scene description, the first build, the step and the plain getters; multi_shard.hip one shard's context and
// its traffic; multi_partition.hip the monitor kernels, the approach check and the re-partition; multi_edit.hip the edits of a running
// world; multi_body_edit.hip the edits of its bodies; multi_materials.hip materials and the mix table; multi_records.hip the record hand-over; multi_query.hip the queries.
#include "multi.hpp"

using namespace eh;
using namespace eh::world;

namespace {

// After a step of every shard: the shards' translated blocks go to the end of the world's list on the home device, device to device, each
// on its shard's stream (behind the translation; the next step of that shard queues up behind the copy). The offsets follow from the
// counts the shards fetched with their state.
int append_events(edynhip_world *w) {
    for (Shard &s : w->shards) {
        if (s.local_ids.empty() || !s.ctx || !s.res.ev_cnt_host) { s.res.ev_held = 0; continue; }
        if (*s.res.ev_cnt_host > s.ctx->event_cap) w->ev_overflow = true;
        w->ev_occurred += *s.res.ev_cnt_host;
    }
    return append_event_blocks(w);
}

}  // namespace

namespace eh {
namespace world {

// The blocks the shards hold translated (Shard res.ev_held records each, in res.ev_out) go to the end of the world's list: after a step
// (above) and after an edit that destroyed points (multi_body_edit.hip).
int append_event_blocks(edynhip_world *w) {
    size_t total = 0;
    for (const Shard &s : w->shards) total += s.res.ev_held;
    if (total == 0) return EDYNHIP_OK;
    const int home = w->devices[0];
    const size_t need = ((size_t)w->ev_n + total) * sizeof(ContactEvent);
    if ((size_t)w->ev_n + total > 0xFFFFFFFFull) return w->fail(EDYNHIP_ERR_CAPACITY, "edynhip_world_step: more than 2^32 - 1 contact events in one call");
    if (need > w->ev_list.cap) {   // grow and keep what the earlier steps of this call appended (copies of theirs may still be in flight)
        for (Shard &s : w->shards) if (s.ctx) { W_HIP(w, hipSetDevice(s.device)); W_HIP(w, hipStreamSynchronize(s.ctx->stream)); }
        W_HIP(w, hipSetDevice(home));
        GrowBuf bigger;
        W_HIP(w, bigger.grow(std::max(std::max(need, 2 * w->ev_list.cap), (size_t)4096 * sizeof(ContactEvent))));
        if (w->ev_n) {
            const hipError_t e = hipMemcpy(bigger.h, w->ev_list.h, (size_t)w->ev_n * sizeof(ContactEvent), hipMemcpyDeviceToDevice);
            if (e != hipSuccess || hipDeviceSynchronize() != hipSuccess) return w->fail(EDYNHIP_ERR_HIP, "edynhip_world_step: growing the event list");
        }
        w->ev_list = std::move(bigger);
    }
    size_t at = w->ev_n;
    for (Shard &s : w->shards) {
        if (s.res.ev_held == 0) continue;
        uint8_t *dst = (uint8_t *)w->ev_list.h + at * sizeof(ContactEvent);
        const size_t bytes = (size_t)s.res.ev_held * sizeof(ContactEvent);
        W_HIP(w, hipSetDevice(s.device));
        if (s.device == home) W_HIP(w, hipMemcpyAsync(dst, s.res.ev_out.h, bytes, hipMemcpyDeviceToDevice, s.ctx->stream));
        else W_HIP(w, hipMemcpyPeerAsync(dst, home, s.res.ev_out.h, s.device, bytes, s.ctx->stream));
        at += s.res.ev_held;
        s.res.ev_held = 0;
    }
    w->ev_n = (uint32_t)at;
    return EDYNHIP_OK;
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
    // new bodies come with the default material and no material id (multi_materials.hip)
    if (!sc.mat_extras.empty()) for (uint32_t i = 0; i < k; ++i) sc.mat_extras.insert(sc.mat_extras.end(), {0.0f, 0.0f, kMaterialLarge, kMaterialLarge});
    if (!sc.mat_id.empty()) sc.mat_id.resize(n0 + k, kUnassignedMaterial);
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

}  // namespace world
}  // namespace eh

extern "C" {

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
    for (Shard &s : w->shards) free_shard(s);   // each on its own device; what is left - streams, events, buffers - is the home device's
    if (!w->devices.empty()) (void)hipSetDevice(w->devices[0]);
    if (w->qstream) (void)hipStreamSynchronize(w->qstream);
    if (w->rec_stream) (void)hipStreamSynchronize(w->rec_stream);
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
    sc.mat_extras.clear(); sc.mat_id.clear(); w->extras_seen = false;   // (the mix table is not the bodies': it stays, as on one context)
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
        for (Shard &s : w->shards) if (!s.local_ids.empty()) { float g; std::memcpy(&g, s.res.mon_host, 4); growth = std::max(growth, g); }
        if (2 * growth < w->budget) continue;   // nobody has moved far enough out of the boxes of the last check
        bool close = false;
        EH_TRY(approach_check(w, close));
        if (close) EH_TRY(repartition(w, true));
    }
    return EDYNHIP_OK;
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
            W_HIP(w, hipMemcpy(out, w->ev_list.h, (size_t)w->ev_n * sizeof(ContactEvent), hipMemcpyDeviceToHost));
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
