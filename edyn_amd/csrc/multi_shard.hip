// One shard of the multi-device world (multi.hpp): its context is built from the scene, the global state and what the islands carry
// (build_shard) and freed (free_shard); its state comes back after every step (gather_shard), what a re-partition carries on request
// (collect_shard, merge_manifolds).
#include "multi.hpp"

using namespace eh;
using namespace eh::world;

namespace {

// the shard's state into the world's global arrays (its own bodies; shard 0: also the replicated ones)
void scatter_state(edynhip_world *w, Shard &s) {
    for (uint32_t l : s.owned_local) {
        const float *row = s.res.pack_host + 13 * (size_t)l;
        const uint32_t g = s.local_ids[l];
        std::memcpy(&w->pos[3 * (size_t)g], row, 12); std::memcpy(&w->orn[4 * (size_t)g], row + 3, 16);
        std::memcpy(&w->linvel[3 * (size_t)g], row + 7, 12); std::memcpy(&w->angvel[3 * (size_t)g], row + 10, 12);
    }
}

}  // namespace

namespace eh {
namespace world {

int shard_filter_thunk(void *user, uint32_t body, uint32_t other) {
    auto *sf = static_cast<edynhip_world::ShardFilter *>(user);
    edynhip_world *w = sf->w;
    const Shard &s = w->shards[sf->shard];
    std::lock_guard<std::mutex> lock(w->filter_mutex);
    return w->filter(w->filter_user, s.local_ids[body], s.local_ids[other]);
}

void free_shard(Shard &s) {
    if (s.ctx) { (void)hipSetDevice(s.device); (void)edynhip_synchronize(s.ctx); }
    s.res = ShardResources{};   // (a pack that was out has landed: the context's stream is idle)
    if (s.ctx) { uint64_t m = 0; if (edynhip_debug_paths(s.ctx, &m) == EDYNHIP_OK) s.paths_gone |= m; }
    if (s.ctx) edynhip_destroy(s.ctx);
    s.ctx = nullptr;
    s.cap = s.joint_cap = s.meshes_created = 0;
    s.xrows = 0;
}

// The world's query tables of shard r from local index l0 onwards (0: a shard just built; otherwise bodies [l0, nl) were appended to
// its context). Every body is answered by one shard - the bodies whose state this shard reports (shard 0: the replicated ones too):
// the global ids, the answer bits, and the island labels the island query reads until the context's first step. island (l0 = 0 only):
// per GLOBAL body the label the shard is built with, or nullptr = none; an appended body is an island of its own beside the labels
// the shard was built with.
void upload_query_tables(edynhip_world *w, uint32_t r, uint32_t l0, const std::vector<uint32_t> *island) {
    Shard &s = w->shards[r];
    const uint32_t nl = (uint32_t)s.local_ids.size(), n = w->scene.n;
    std::vector<uint32_t> bits;
    if (r != 0) {
        bits.assign((size_t)nl / 32 + 1, 0u);
        for (uint32_t l : s.owned_local) bits[l >> 5] |= 1u << (l & 31u);
        SH_HIP(s, hipMemcpy(s.res.ans_dev, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (nl > l0) SH_HIP(s, hipMemcpy(s.res.ids_dev + l0, s.local_ids.data() + l0, (size_t)(nl - l0) * sizeof(uint32_t), hipMemcpyHostToDevice));
    const bool labels = l0 ? s.ctx->query_island != nullptr : island && nl;
    if (labels && nl > l0) {   // (an island lives on one shard: its label is local)
        std::vector<uint32_t> lab(nl - l0);
        for (uint32_t l = l0; l < nl; ++l) {
            const uint32_t g = s.local_ids[l], root = island ? (*island)[g] : g;
            const int32_t lr = w->rank_of[g] == (int32_t)r && root < n ? s.to_local[root] : -1;
            lab[l - l0] = lr >= 0 ? (uint32_t)lr : l;
        }
        SH_HIP(s, hipMemcpy(s.res.qisl_dev + l0, lab.data(), lab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    shard_set_answers(s.ctx, r != 0 ? s.res.ans_dev : nullptr, std::move(bits), labels ? s.res.qisl_dev : nullptr);
}

// The world's materials of the bodies a context has just been given (and with them the default materials), and the mix table, as the
// single context's calls would have set them. Bodies without a contact_extras material set none: a shard none of whose bodies has one
// keeps its fast schedule (every schedule computes the same bits, include/edynhip.h "solve_schedule"). The table was emptied before
// the bodies went up (build_shard): the insertions are replayed, in their order, into none.
void apply_materials(edynhip_world *w, Shard &s) {
    const HostScene &sc = w->scene;
    const uint32_t nl = (uint32_t)s.local_ids.size();
    if (nl && !sc.mat_extras.empty()) {
        std::vector<float> col[4];
        bool any = false;
        for (int d = 0; d < 4; ++d) col[d].resize(nl);
        for (uint32_t l = 0; l < nl; ++l) {
            const float *m = &sc.mat_extras[4 * (size_t)s.local_ids[l]];
            for (int d = 0; d < 4; ++d) col[d][l] = m[d];
            any = any || !material_extras_default(m[0], m[1], m[2], m[3]);
        }
        if (any) SH_TRY(s, shard_set_material_extras(s.ctx, 0, nl, col[0].data(), col[1].data(), col[2].data(), col[3].data()));
    }
    if (nl && !sc.mat_id.empty()) {
        std::vector<uint32_t> ids(nl);
        bool any = false;
        for (uint32_t l = 0; l < nl; ++l) { ids[l] = sc.mat_id[s.local_ids[l]]; any = any || ids[l] != kUnassignedMaterial; }
        if (any) SH_TRY(s, shard_set_material_ids(s.ctx, 0, nl, ids.data()));
    }
    for (const HostScene::MixEntry &e : sc.mix) SH_TRY(s, shard_insert_material_mixing(s.ctx, e.id0, e.id1, e.m));
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
        if (!s.res.ev_cnt_host) SH_HIP(s, s.res.ev_cnt_host.alloc(1));
        *s.res.ev_cnt_host = 0; s.res.ev_held = 0;
        SH_HIP(s, s.res.ev_out.grow((size_t)std::max<uint32_t>(s.ctx->event_cap, 1) * sizeof(ContactEvent)));
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
    // (a kept context still holds the mix table: emptied before the bodies go up, so that what edynhip_set_bodies derives from it - the
    // restitution solver's switch - and the replay in apply_materials start from none)
    SH_TRY(s, shard_reset_material_mixing(s.ctx));
    SH_TRY(s, edynhip_set_bodies(s.ctx, nl, &b));
    trace.mark("take + edynhip_set_bodies");
    if (from_state && !mine.com.empty()) {   // set_bodies read `pos` as the origin of bodies with an offset: put the centre-of-mass state back ...
        SH_TRY(s, edynhip_set_state(s.ctx, mine.pos.data(), mine.orn.data(), mine.linvel.data(), mine.angvel.data()));
        // ... and with it what set_bodies derived from the misread position: origins, AABBs (displaced by R com otherwise - the first
        // broadphase / narrowphase after a re-partition would place those shapes wrong) and world inertias. Before the sleep tags below:
        // the derivation skips sleeping bodies
        SH_TRY(s, edynhip_refresh_derived(s.ctx));
    }
    apply_materials(w, s);
    if (s.rc != EDYNHIP_OK) return;
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
        // materials: the carried points keep the mix they were created with and the impulses of their rolling and spinning rows
        const bool with_extras = !carry.point_extras.empty() && !mine.empty();
        if (with_extras) {
            const size_t floats = kExtrasRowFloats * mine.size();
            if (s.res.xtr_host_cap < floats) { s.res.xtr_host_cap = 0; SH_HIP(s, s.res.xtr_host.alloc(floats + floats / 2)); s.res.xtr_host_cap = floats + floats / 2; }
            bool plain = true;
            for (size_t k = 0; k < mine.size(); ++k) {
                float *row = s.res.xtr_host + kExtrasRowFloats * k;
                const auto it = carry.point_extras.find(((uint64_t)mine[k].body[0] << 32) | mine[k].body[1]);
                if (it == carry.point_extras.end()) {
                    s.rc = EDYNHIP_ERR_INTERNAL; s.err = "a carried manifold (bodies " + std::to_string(mine[k].body[0]) + ", " + std::to_string(mine[k].body[1]) + ") has no point extras";
                    return;
                }
                std::memcpy(row, it->second.data(), sizeof(it->second));
                plain = plain && extras_row_is_default(row, mine[k].num_points);
            }
            // (a point may outlive its bodies' materials: a context that no material of this build has put on the extras schedule - it may
            // still own the storage from an earlier one - is put there for such a point)
            if (!plain) SH_TRY(s, shard_ensure_extras_storage(s.ctx));
        }
        for (edynhip_manifold &m : mine) { m.body[0] = (uint32_t)s.to_local[m.body[0]]; m.body[1] = (uint32_t)s.to_local[m.body[1]]; }   // a monotone map: the canonical order is kept
        trace.mark("joints, exclusions, select carried manifolds");
        if (!mine.empty()) SH_TRY(s, edynhip_set_manifolds(s.ctx, mine.data(), (uint32_t)mine.size()));
        if (!mine_ids.empty()) {
            SH_HIP(s, s.res.pid_buf.grow(mine_ids.size() * sizeof(uint64_t)));
            SH_HIP(s, hipMemcpyAsync(s.res.pid_buf.h, mine_ids.data(), mine_ids.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s.ctx->stream));
            SH_TRY(s, shard_inject_point_ids(s.ctx, (const uint64_t *)s.res.pid_buf.h, (uint32_t)mine.size()));
            SH_HIP(s, hipStreamSynchronize(s.ctx->stream));   // (mine_ids is read by the copy until here)
        }
        if (with_extras && shard_has_extras_storage(s.ctx)) {
            const size_t bytes = kExtrasRowFloats * mine.size() * sizeof(float);
            SH_HIP(s, s.res.xtr_buf.grow(bytes));
            SH_HIP(s, hipMemcpyAsync(s.res.xtr_buf.h, s.res.xtr_host, bytes, hipMemcpyHostToDevice, s.ctx->stream));
            SH_TRY(s, shard_inject_point_extras(s.ctx, s.res.xtr_buf.h, (uint32_t)mine.size()));
            SH_HIP(s, hipStreamSynchronize(s.ctx->stream));   // (the pinned rows are rewritten by the next collect)
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
    if (!s.res.pack_dev) {
        SH_HIP(s, s.res.pack_dev.alloc((size_t)std::max<uint32_t>(s.cap, 1) * 13));
        SH_HIP(s, s.res.pack_host.alloc((size_t)std::max<uint32_t>(s.cap, 1) * 13));
        SH_HIP(s, s.res.mon_dev.alloc(words));
        SH_HIP(s, s.res.mon_host.alloc(2 + 7 * (size_t)s.cap));
        SH_HIP(s, s.res.ids_dev.alloc(std::max<uint32_t>(s.cap, 1)));
        SH_HIP(s, s.res.ans_dev.alloc((size_t)s.cap / 32 + 1));
        SH_HIP(s, s.res.qisl_dev.alloc(std::max<uint32_t>(s.cap, 1)));
        SH_HIP(s, s.res.q_tot.alloc(1));
    }
    SH_HIP(s, hipMemset(s.res.mon_dev, 0, words * sizeof(uint32_t)));
    // queries: every body is answered by one shard - the bodies whose state this shard reports (shard 0: the replicated ones too)
    upload_query_tables(w, r, 0, carry.any && carry.island.size() == n ? &carry.island : nullptr);
    if (s.rc != EDYNHIP_OK) return;
    trace.mark("warm start, sleep state, gather / monitor buffers");
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
        hipLaunchKernelGGL(k_shard_growth, dim3((nl + 255) / 256), dim3(256), 0, st, nl, s.ctx->b, (const float4 *)(s.res.mon_dev + L.amin0),
                           (const float4 *)(s.res.mon_dev + L.amax0), s.res.mon_dev);
    SH_TRY(s, edynhip_pack_state_device(s.ctx, s.res.pack_dev, 0, nl));
    SH_HIP(s, hipMemcpyAsync(s.res.pack_host, s.res.pack_dev, (size_t)nl * 13 * sizeof(float), hipMemcpyDeviceToHost, st));
    SH_HIP(s, hipMemcpyAsync(s.res.mon_host, s.res.mon_dev, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    const bool events = with_growth && s.ctx->events && s.res.ev_cnt_host;   // (with_growth: after a step)
    if (events) SH_HIP(s, hipMemcpyAsync(s.res.ev_cnt_host, s.ctx->event_count, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SH_HIP(s, hipStreamSynchronize(st));
    scatter_state(w, s);
    if (events) {   // the step's events in global indices, enqueued behind the step: the world appends the block to its list (append_events)
        s.res.ev_held = std::min(*s.res.ev_cnt_host, s.ctx->event_cap);
        SH_TRY(s, shard_translate_events(s.ctx, s.res.ev_held, s.res.ids_dev, nl, s.res.ev_out.h));
    }
}

// What the islands carry, per shard, in two parts: LIGHT - island labels, AABBs, sleeping tags and timers (28-45 bytes per body: what a
// re-partition decides on) - and HEAVY - the manifolds with their warm-start impulses and the joints' applied impulses (336 bytes per
// manifold: only worth reading from the shards that are rebuilt).
void collect_shard(edynhip_world *w, uint32_t r, bool light, bool heavy, bool extras) {
    Shard &s = w->shards[r];
    if (s.rc != EDYNHIP_OK) return;
    const uint32_t nl = (uint32_t)s.local_ids.size();
    if (light) { s.labels.assign(nl, 0); s.aabb.assign((size_t)nl * 6, 0.f); s.asleep.assign(nl, 0); }
    s.manifolds.clear(); s.imp24.clear(); s.imp10.clear(); s.pids.clear(); s.xrows = 0;
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
        SH_HIP(s, s.res.pid_buf.grow(s.pids.size() * sizeof(uint64_t)));
        SH_TRY(s, shard_gather_point_ids(s.ctx, (uint64_t *)s.res.pid_buf.h));
        SH_HIP(s, hipMemcpyAsync(s.pids.data(), s.res.pid_buf.h, s.pids.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s.ctx->stream));
        SH_HIP(s, hipStreamSynchronize(s.ctx->stream));
    }
    if (nm && extras) {   // materials: the points' extras travel with the records, [m][32] in the same order, in the shard's pinned buffer
        const size_t floats = kExtrasRowFloats * (size_t)nm;
        if (s.res.xtr_host_cap < floats) { s.res.xtr_host_cap = 0; SH_HIP(s, s.res.xtr_host.alloc(floats + floats / 2)); s.res.xtr_host_cap = floats + floats / 2; }
        if (shard_has_extras_storage(s.ctx)) {
            SH_HIP(s, s.res.xtr_buf.grow(floats * sizeof(float)));
            SH_TRY(s, shard_gather_point_extras(s.ctx, s.res.xtr_buf.h));
            SH_HIP(s, hipMemcpyAsync(s.res.xtr_host, s.res.xtr_buf.h, floats * sizeof(float), hipMemcpyDeviceToHost, s.ctx->stream));
            SH_HIP(s, hipStreamSynchronize(s.ctx->stream));
        } else   // (no material has reached this context: its points are plain)
            for (uint32_t k = 0; k < nm; ++k) extras_row_default(s.res.xtr_host + kExtrasRowFloats * (size_t)k, s.manifolds[k].num_points);
        s.xrows = nm;
    }
    const uint32_t njl = (uint32_t)s.local_joints.size();
    if (njl) {
        s.imp24.assign((size_t)njl * 24, 0.f); s.imp10.assign((size_t)njl * 10, 0.f);
        SH_TRY(s, edynhip_get_joint_slot_impulses(s.ctx, s.imp24.data()));
        SH_TRY(s, edynhip_get_joint_impulses(s.ctx, s.imp10.data()));
    }
}

// gathers the manifolds of all shards, each once, global indices, canonical order; ids (or nullptr): their points' ids [m][4], in that order
void merge_manifolds(edynhip_world *w, std::vector<edynhip_manifold> &out, std::vector<uint64_t> *ids, std::vector<float> *extras) {
    out.clear();
    std::vector<const uint64_t *> from;   // per gathered record: its row of the shard's id table
    std::vector<const float *> xfrom;     // ... and of its extras table
    for (uint32_t r = 0; r < w->shards.size(); ++r) {
        Shard &s = w->shards[r];
        for (size_t k = 0; k < s.manifolds.size(); ++k) {
            edynhip_manifold m = s.manifolds[k];
            m.body[0] = s.local_ids[m.body[0]]; m.body[1] = s.local_ids[m.body[1]];
            const int32_t ra = w->rank_of[m.body[0]], rb = w->rank_of[m.body[1]];
            if (ra == (int32_t)r || (ra < 0 && rb == (int32_t)r)) { out.push_back(m); if (ids) from.push_back(s.pids.size() == 4 * s.manifolds.size() ? &s.pids[4 * k] : nullptr); if (extras) xfrom.push_back(s.xrows == s.manifolds.size() ? s.res.xtr_host + kExtrasRowFloats * k : nullptr); }
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
    if (extras) {   // (a world without materials gathers no rows: every point is plain)
        extras->resize(kExtrasRowFloats * out.size());
        for (uint32_t k = 0; k < out.size(); ++k) {
            float *dst = &(*extras)[kExtrasRowFloats * (size_t)k];
            if (const float *row = xfrom[order[k].second]) std::memcpy(dst, row, kExtrasRowFloats * sizeof(float));
            else extras_row_default(dst, out[k].num_points);
        }
    }
}

}  // namespace world
}  // namespace eh
