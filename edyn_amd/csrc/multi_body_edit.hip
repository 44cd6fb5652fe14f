// Bodies of a running multi-device world edited and woken in place (multi.hpp; include/edynhip.h edynhip_world_edit_bodies /
// edynhip_world_wake_bodies): edynhip_edit_bodies and edynhip_wake_bodies in global indices.
//
// An edit goes to every context that holds the body - the owner of a dynamic body, every shard for a replicated one - in that shard's
// local indices, through the function the single context itself runs (body_edit.hip edit_bodies), so a shard computes for its bodies
// exactly what one context computes for the whole world. The scene (HostScene) stays the truth the shards are rebuilt from: every
// edited member lands there. What an edit destroys - the points and manifolds of a reshaped body or of one whose kind changed - the
// shard appends to its event list behind the last step's: that tail is translated on the shard's device and appended to the world's list.
// An edit whose kind crosses between dynamic and not dynamic changes who holds the body; local indices ascend with the global ones, so
// the body cannot be appended to another shard's context: the shards that gain or lose the replica are rebuilt through what a sticky
// re-partition carries. Which shards, which owner, when the approach check is due: world_rules.hpp.
#include "multi.hpp"
#include "ctx_rules.hpp"

using namespace eh;
using namespace eh::world;

namespace {

template <typename T>
void materialise(std::vector<T> &vec, size_t n, size_t width, const T *def_row) {   // an optional array of the scene, with its default rows
    if (!vec.empty()) return;
    vec.resize(n * width);
    for (size_t i = 0; i < vec.size(); ++i) vec[i] = def_row[i % width];
}

// The edit as the scene describes the bodies from here on (and, for a body made static, the world's velocities)
void scene_apply_edit(edynhip_world *w, uint32_t n, const uint32_t *indices, const edynhip_bodies *in, uint32_t fields) {
    HostScene &sc = w->scene;
    const float zeros[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const uint8_t zero8 = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const size_t g = indices[k];
        const int32_t kind_before = sc.kind[g], kind = kind_after_edit(fields, kind_before, (fields & EDYNHIP_EDIT_KIND) ? in->kind[k] : kind_before);
        // the inertia the scene leaves to the shape and mass the body had: written out before either changes without it (bake_shape_inertia)
        if (kind_before == EDYNHIP_KIND_DYNAMIC && !(fields & EDYNHIP_EDIT_INERTIA) && (fields & (EDYNHIP_EDIT_MASS | EDYNHIP_EDIT_SHAPE)) &&
            (sc.has_inertia.empty() || !sc.has_inertia[g])) {
            const bool has_com = !sc.com.empty() && (sc.com[3 * g] != 0 || sc.com[3 * g + 1] != 0 || sc.com[3 * g + 2] != 0);
            float baked[9];
            if (bake_shape_inertia(sc.shape_type[g], &sc.shape_param[4 * g], sc.mass[g], has_com, baked)) {
                materialise(sc.inertia, sc.n, 9, zeros); materialise(sc.has_inertia, sc.n, 1, &zero8);
                std::memcpy(&sc.inertia[9 * g], baked, sizeof(baked));
                sc.has_inertia[g] = 1;
            }
        }
        if (fields & EDYNHIP_EDIT_MASS) sc.mass[g] = in->mass[k];
        if (fields & EDYNHIP_EDIT_INERTIA) {
            const bool given = in->has_inertia && in->has_inertia[k];
            if (given || !sc.has_inertia.empty()) {
                materialise(sc.inertia, sc.n, 9, zeros); materialise(sc.has_inertia, sc.n, 1, &zero8);
                sc.has_inertia[g] = given ? 1 : 0;
                std::memcpy(&sc.inertia[9 * g], given ? in->inertia + 9 * (size_t)k : zeros, 9 * sizeof(float));
            }
        }
        if (fields & EDYNHIP_EDIT_MATERIAL) { sc.friction[g] = in->friction[k]; sc.restitution[g] = in->restitution[k]; }
        if (fields & EDYNHIP_EDIT_SHAPE) { sc.shape_type[g] = in->shape_type[k]; std::memcpy(&sc.shape_param[4 * g], in->shape_param + 4 * (size_t)k, 4 * sizeof(float)); }
        if (fields & EDYNHIP_EDIT_KIND) {
            sc.kind[g] = kind;
            if (kind == EDYNHIP_KIND_DYNAMIC && (in->gravity || !sc.gravity.empty())) {
                materialise(sc.gravity, sc.n, 3, w->cfg.gravity);
                std::memcpy(&sc.gravity[3 * g], in->gravity ? in->gravity + 3 * (size_t)k : w->cfg.gravity, 3 * sizeof(float));
            }
            if (kind == EDYNHIP_KIND_STATIC) {
                for (int d = 0; d < 3; ++d) { sc.linvel[3 * g + d] = 0; sc.angvel[3 * g + d] = 0; }
                if (w->linvel.size() == 3 * (size_t)sc.n) for (int d = 0; d < 3; ++d) { w->linvel[3 * g + d] = 0; w->angvel[3 * g + d] = 0; }
            }
        }
    }
}

hipError_t read_event_count(const edynhip_ctx *c, uint32_t &out) {
    hipError_t e = hipMemcpyAsync(&out, c->event_count, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e;
}

bool has_local_joint(const Shard &s, uint32_t j) { return std::binary_search(s.local_joints.begin(), s.local_joints.end(), j); }

}  // namespace

extern "C" {

int edynhip_world_edit_bodies(edynhip_world *w, uint32_t n, const uint32_t *indices, const edynhip_bodies *in, uint32_t fields) {
    if (!w) return EDYNHIP_ERR_INVALID;
    HostScene &sc = w->scene;
    {   // everything is decided before anything changes on any shard
        const char *why = "";
        const int rc = validate_body_edit(n, indices, in, fields, sc.n, w->removed, (uint32_t)sc.meshes.size(), &why);
        if (rc != EDYNHIP_OK) return w->fail(rc, std::string("edynhip_world_edit_bodies: ") + why);
    }
    if (n == 0 || fields == 0) return EDYNHIP_OK;
    if (!w->built) { scene_apply_edit(w, n, indices, in, fields); return EDYNHIP_OK; }
    const uint32_t W = (uint32_t)w->shards.size();
    ++w->edit_stats.edits;
    const bool rekind = fields & EDYNHIP_EDIT_KIND, drops = fields & (EDYNHIP_EDIT_SHAPE | EDYNHIP_EDIT_KIND);
    std::vector<uint32_t> to_dynamic, from_dynamic;
    bool check_due = false;
    std::vector<std::vector<uint32_t>> mine(W);   // per shard: the rows of the call it takes
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t g = indices[k];
        const int32_t before = sc.kind[g], after = kind_after_edit(fields, before, rekind ? in->kind[k] : before);
        if (edit_crosses_boundary(before, after)) (after == EDYNHIP_KIND_DYNAMIC ? to_dynamic : from_dynamic).push_back(g);
        check_due = check_due || edit_needs_approach_check(fields, before, after, W);
        for (uint32_t r = 0; r < W; ++r) {
            if (!shard_takes_body_edit(before, w->rank_of[g], r)) continue;
            if (!w->shards[r].ctx || w->shards[r].to_local[g] < 0) return w->fail(EDYNHIP_ERR_INTERNAL, "edynhip_world_edit_bodies: shard " + std::to_string(r) + " does not hold body " + std::to_string(g));
            mine[r].push_back(k);
        }
    }
    // ---- in place, on the shards' threads; the events the edit appended (the tail of each shard's list) translated on its device
    const bool events = w->events_on() && drops;
    std::vector<uint32_t> occurred(W, 0);
    std::vector<uint8_t> overflow(W, 0);
    EH_TRY(on_shards(w, [&](Shard &, uint32_t r) { return !mine[r].empty(); }, [&](Shard &s, uint32_t r) {
        if (fields & EDYNHIP_EDIT_SHAPE)   // a polyhedron needs its mesh on this shard
            for (; s.meshes_created < sc.meshes.size(); ++s.meshes_created) {
                const HostScene::Mesh &m = sc.meshes[s.meshes_created];
                uint32_t id = 0;
                SH_TRY(s, edynhip_create_convex_mesh(s.ctx, (uint32_t)m.v.size() / 3, m.v.data(), (uint32_t)m.idx.size(), m.idx.data(), (uint32_t)m.faces.size() / 2, m.faces.data(), m.flags, &id));
            }
        const BodyRows sub(*in, mine[r]);
        const edynhip_bodies b = sub.view();
        std::vector<uint32_t> local(mine[r].size());
        for (size_t q = 0; q < local.size(); ++q) local[q] = (uint32_t)s.to_local[indices[mine[r][q]]];
        uint32_t first = 0, last = 0;
        if (events) SH_HIP(s, read_event_count(s.ctx, first));
        SH_TRY(s, edit_bodies(s.ctx, (uint32_t)local.size(), local.data(), &b, fields));
        if (!events) return;
        SH_HIP(s, read_event_count(s.ctx, last));
        occurred[r] = last - first;
        overflow[r] = last > s.ctx->event_cap;
        first = std::min(first, s.ctx->event_cap); last = std::min(last, s.ctx->event_cap);
        if (last <= first) return;
        SH_TRY(s, shard_translate_event_tail(s.ctx, first, last, s.res.ids_dev, (uint32_t)s.local_ids.size(), s.res.ev_out.h));
        s.res.ev_held = last - first;
    }));
    if (events) {
        for (uint32_t r = 0; r < W; ++r) { w->ev_occurred += occurred[r]; if (overflow[r]) w->ev_overflow = true; }
        EH_TRY(append_event_blocks(w));
    }
    // ---- the scene follows. Who is dynamic decides where a body lives: the live dynamic bodies per shard before the bodies of this call move
    std::vector<uint32_t> load(W, 0);
    if (!to_dynamic.empty())
        for (uint32_t g = 0; g < sc.n; ++g) if (sc.kind[g] == EDYNHIP_KIND_DYNAMIC && !w->is_removed(g) && w->rank_of[g] >= 0) ++load[(uint32_t)w->rank_of[g]];
    scene_apply_edit(w, n, indices, in, fields);
    bool moved = false;
    if (to_dynamic.empty() && from_dynamic.empty()) {
        if (check_due) EH_TRY(edit_approach(w, moved));
        if (!moved) ++w->edit_stats.in_place;
        return EDYNHIP_OK;
    }
    // ---- crossing the replication boundary: rank_of and the tables of the shards that keep their contexts follow, the others are rebuilt
    std::vector<uint8_t> force(W, 0), retable(W, 0);
    auto set_reports = [&](Shard &s, uint32_t g, bool reports) {   // owned_local stays ascending
        const uint32_t l = (uint32_t)s.to_local[g];
        const auto it = std::lower_bound(s.owned_local.begin(), s.owned_local.end(), l);
        const bool listed = it != s.owned_local.end() && *it == l;
        if (reports && !listed) s.owned_local.insert(it, l);
        if (!reports && listed) s.owned_local.erase(it);
    };
    for (uint32_t g : from_dynamic) {
        const uint32_t o = (uint32_t)w->rank_of[g];
        if (load.size() == W && !to_dynamic.empty() && load[o]) --load[o];
        w->rank_of[g] = -1;
        for (uint32_t r = 0; r < W; ++r) if (r != o) force[r] = 1;
        set_reports(w->shards[o], g, shard_reports_body(-1, o));
        retable[o] = 1;
    }
    for (uint32_t g : to_dynamic) {
        const uint32_t o = owner_of_new_dynamic(load);
        w->rank_of[g] = (int32_t)o;
        for (uint32_t r = 0; r < W; ++r) if (r != o) force[r] = 1;
        set_reports(w->shards[o], g, true);
        retable[o] = 1;
        if (w->query_labels.size() == sc.n) w->query_labels[g] = g;
    }
    std::vector<std::array<uint32_t, 2>> edges;   // joints of a body made dynamic that now tie islands of two shards
    for (uint32_t g : to_dynamic) {
        const uint32_t o = (uint32_t)w->rank_of[g];
        for (uint32_t j = 0; j < sc.nj; ++j) {
            if (!sc.jalive[j] || (sc.jbody[2 * j] != g && sc.jbody[2 * j + 1] != g)) continue;
            const uint32_t a = sc.jbody[2 * j], b = sc.jbody[2 * j + 1];
            const int32_t home = joint_home(owner_rank(sc.kind[a], w->rank_of[a]), owner_rank(sc.kind[b], w->rank_of[b]));
            if (home == -2) edges.push_back({a, b});
            else if (home == (int32_t)o && !has_local_joint(w->shards[o], j)) force[o] = 1;   // (a joint to another replicated body: no context held it)
        }
        for (const auto &e : sc.exclusions) {   // an exclusion with a replicated body is now the owner's
            if (e[0] != g && e[1] != g) continue;
            const uint32_t x = e[0] == g ? e[1] : e[0];
            if (sc.kind[x] != EDYNHIP_KIND_DYNAMIC) force[o] = 1;
        }
    }
    refresh_bodies_per_shard(w);
    if (W < 2) { ++w->edit_stats.in_place; return EDYNHIP_OK; }   // one shard holds and reports every body: nothing moves
    EH_TRY(on_shards(w, [&](Shard &, uint32_t r) { return retable[r] && !force[r]; }, [&](Shard &s, uint32_t r) {
        upload_query_tables(w, r, (uint32_t)s.local_ids.size());
    }));
    for (uint8_t f : force) if (f) ++w->edit_stats.shard_rebuilds;
    if (!edges.empty()) ++w->edit_stats.repartitions_by_edit;
    if (check_due) ++w->edit_stats.approach_checks_by_edit;   // (the re-partition welds what the new boxes bring together and takes the budget again)
    EH_TRY(repartition(w, true, edges.empty() ? nullptr : &edges, &force, true));
    for (const auto &e : edges)
        if (joint_home(owner_rank(sc.kind[e[0]], w->rank_of[e[0]]), owner_rank(sc.kind[e[1]], w->rank_of[e[1]])) == -2)
            return w->fail(EDYNHIP_ERR_INTERNAL, "edynhip_world_edit_bodies: the re-partition left a joint's bodies on two shards");
    return EDYNHIP_OK;
}

int edynhip_world_wake_bodies(edynhip_world *w, uint32_t n, const uint32_t *indices) {
    if (!w || (n && !indices)) return EDYNHIP_ERR_INVALID;
    const HostScene &sc = w->scene;
    for (uint32_t k = 0; k < n; ++k) if (indices[k] >= sc.n) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_wake_bodies: index out of range");
    if (n == 0 || !w->built || !(w->cfg.flags & EDYNHIP_FLAG_SLEEPING)) return EDYNHIP_OK;
    ++w->edit_stats.edits;
    const uint32_t W = (uint32_t)w->shards.size();
    std::vector<std::vector<uint32_t>> mine(W);   // local indices: a body's island lives on the shard that holds it
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t g = indices[k];
        if (w->is_removed(g)) continue;
        for (uint32_t r = 0; r < W; ++r) if (w->shards[r].ctx && w->shards[r].to_local[g] >= 0) mine[r].push_back((uint32_t)w->shards[r].to_local[g]);
    }
    EH_TRY(on_shards(w, [&](Shard &, uint32_t r) { return !mine[r].empty(); }, [&](Shard &s, uint32_t r) {
        SH_TRY(s, edynhip_wake_bodies(s.ctx, (uint32_t)mine[r].size(), mine[r].data()));
    }));
    ++w->edit_stats.in_place;
    return EDYNHIP_OK;
}

}  // extern "C"
