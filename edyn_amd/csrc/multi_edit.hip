// Edits of a running multi-device world (multi.hpp).
//
// edynhip_world_add_bodies / _remove_bodies / _add_joints / _remove_joints / _edit_joint / _edit_exclusion / _set_state / _set_params:
// the single context's edits in global indices. The scene (HostScene) stays the truth the shards are rebuilt from - bodies are appended,
// a removed body becomes what the context itself turns the slot into (a shapeless static body), joints get an alive flag - and the
// edit is forwarded to the context(s) that hold the bodies, so nobody else's manifolds, impulses, timers or point ids are touched.
// The global-to-local maps stay ascending because a new body or joint has the highest global AND the highest local index.
#include "multi.hpp"

using namespace eh;
using namespace eh::world;

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

}  // namespace

// The safety condition after an edit that can bring islands of different shards together (a shaped dynamic body was added): the approach
// check - body boxes while a shard has not stepped since it was built, island boxes otherwise; a new body is an island of its own either
// way - which also records the boxes the growth monitor measures the new bodies against, and the sticky re-partition if it says "close".
int eh::world::edit_approach(edynhip_world *w, bool &moved) {
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
