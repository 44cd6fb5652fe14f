// Materials on a multi-device world (multi.hpp): edynhip_world_set_material_extras / _set_material_ids / _insert_material_mixing /
// _get_point_extras - the single context's calls in global indices.
//
// The world keeps the materials by global body (HostScene::mat_extras, mat_id) and the mix table as the ordered list of its insertions
// (HostScene::mix); whatever builds a shard applies them (apply_materials, multi_shard.hip): a body's slice goes to the shard that owns
// it, a replicated body's to every shard, the whole table to every shard. On a running world the calls are forwarded in place, like the
// edits of multi_edit.hip: no shard is rebuilt, nothing is re-partitioned, and - as on one context - only points created from then on
// see the change. What a point was created with travels with it: a re-partition carries the extras rows of the manifolds it carries
// (collect_shard gathers them on the device, build_shard puts them back after edynhip_set_manifolds; world_extras.hip), once the world
// holds any such material or mix-table entry. The host decisions - which shards a body range touches, whether a carry is needed, the
// row layout - are world_rules.hpp's.
#include "multi.hpp"

using namespace eh;
using namespace eh::world;

namespace {

// The bodies [first, first + n) on shard s as runs of consecutive local indices: run(l0, g0, count) for local l0 .. = global g0 ..
template <typename Run>
void local_runs(const Shard &s, uint32_t first, uint32_t n, Run &&run) {
    uint32_t g = first;
    const uint32_t end = first + n;
    while (g < end) {
        if (g >= s.to_local.size() || s.to_local[g] < 0) { ++g; continue; }
        uint32_t count = 1;
        while (g + count < end && g + count < s.to_local.size() && s.to_local[g + count] == s.to_local[g] + (int32_t)count) ++count;
        run((uint32_t)s.to_local[g], g, count);
        g += count;
    }
}

// an edit of the bodies [first, first + n) on the shards that hold any of them, on their threads
template <typename Work>
int on_shards_of_range(edynhip_world *w, uint32_t first, uint32_t n, Work &&work) {
    std::vector<uint8_t> touched(w->shards.size());
    shards_of_body_range(w->rank_of.data(), first, n, (uint32_t)w->shards.size(), touched.data());
    return on_shards(w, [&](Shard &s, uint32_t r) { return touched[r] && s.ctx; }, work);
}

}  // namespace

extern "C" {

int edynhip_world_set_material_extras(edynhip_world *w, uint32_t first, uint32_t n, const float *spin, const float *roll, const float *stiffness, const float *damping) {
    if (!w) return EDYNHIP_ERR_INVALID;
    HostScene &sc = w->scene;
    if ((uint64_t)first + n > sc.n) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_set_material_extras: body range out of bounds");
    if (n == 0) return EDYNHIP_OK;
    std::vector<float> rows(4 * (size_t)n);
    bool any = false;
    for (uint32_t i = 0; i < n; ++i) {
        float *m = &rows[4 * (size_t)i];
        m[0] = spin ? spin[i] : 0.0f; m[1] = roll ? roll[i] : 0.0f; m[2] = stiffness ? stiffness[i] : kMaterialLarge; m[3] = damping ? damping[i] : kMaterialLarge;
        if (!material_extras_valid(m[0], m[1], m[2], m[3])) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_set_material_extras: negative friction or non-positive stiffness / damping");
        any = any || !material_extras_default(m[0], m[1], m[2], m[3]);
    }
    if (sc.mat_extras.empty()) {
        if (!any) return EDYNHIP_OK;   // (defaults over defaults)
        sc.mat_extras.resize(4 * (size_t)sc.n);
        for (size_t g = 0; g < sc.n; ++g) { sc.mat_extras[4 * g] = 0.0f; sc.mat_extras[4 * g + 1] = 0.0f; sc.mat_extras[4 * g + 2] = kMaterialLarge; sc.mat_extras[4 * g + 3] = kMaterialLarge; }
    }
    std::memcpy(&sc.mat_extras[4 * (size_t)first], rows.data(), rows.size() * sizeof(float));
    w->extras_seen = w->extras_seen || any;
    if (!w->built) return EDYNHIP_OK;
    ++w->edit_stats.edits;
    EH_TRY(on_shards_of_range(w, first, n, [&](Shard &s, uint32_t) {
        local_runs(s, first, n, [&](uint32_t l0, uint32_t g0, uint32_t count) {
            if (s.rc != EDYNHIP_OK) return;
            std::vector<float> col[4];
            for (int d = 0; d < 4; ++d) { col[d].resize(count); for (uint32_t k = 0; k < count; ++k) col[d][k] = rows[4 * (size_t)(g0 - first + k) + d]; }
            SH_TRY(s, shard_set_material_extras(s.ctx, l0, count, col[0].data(), col[1].data(), col[2].data(), col[3].data()));
        });
    }));
    ++w->edit_stats.in_place;
    return EDYNHIP_OK;
}

int edynhip_world_set_material_ids(edynhip_world *w, uint32_t first, uint32_t n, const uint32_t *ids) {
    if (!w) return EDYNHIP_ERR_INVALID;
    HostScene &sc = w->scene;
    if (n && !ids) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_set_material_ids: missing array");
    if ((uint64_t)first + n > sc.n) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_set_material_ids: body range out of bounds");
    for (uint32_t i = 0; i < n; ++i) if (ids[i] > kUnassignedMaterial) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_set_material_ids: material::id_type is 16 bits (0xFFFF = unassigned)");
    if (n == 0) return EDYNHIP_OK;
    sc.mat_id.resize(sc.n, kUnassignedMaterial);
    std::memcpy(&sc.mat_id[first], ids, (size_t)n * sizeof(uint32_t));
    if (!w->built) return EDYNHIP_OK;
    ++w->edit_stats.edits;
    EH_TRY(on_shards_of_range(w, first, n, [&](Shard &s, uint32_t) {
        local_runs(s, first, n, [&](uint32_t l0, uint32_t g0, uint32_t count) {
            if (s.rc != EDYNHIP_OK) return;
            SH_TRY(s, shard_set_material_ids(s.ctx, l0, count, ids + (g0 - first)));
        });
    }));
    ++w->edit_stats.in_place;
    return EDYNHIP_OK;
}

int edynhip_world_insert_material_mixing(edynhip_world *w, uint32_t id0, uint32_t id1, const float *material6) {
    if (!w) return EDYNHIP_ERR_INVALID;
    if (!material6) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_insert_material_mixing: missing array");
    if (id0 >= kUnassignedMaterial || id1 >= kUnassignedMaterial) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_insert_material_mixing: unassigned material id");
    HostScene::MixEntry e{id0, id1, {material6[0], material6[1], material6[2], material6[3], material6[4], material6[5]}};
    w->scene.mix.push_back(e);
    if (!w->built) return EDYNHIP_OK;
    ++w->edit_stats.edits;
    EH_TRY(on_shards(w, [](Shard &s, uint32_t) { return s.ctx != nullptr; }, [&](Shard &s, uint32_t) {
        SH_TRY(s, shard_insert_material_mixing(s.ctx, e.id0, e.id1, e.m));
    }));
    ++w->edit_stats.in_place;
    return EDYNHIP_OK;
}

int edynhip_world_get_point_extras(edynhip_world *w, float *out7, uint32_t capacity_manifolds, uint32_t *n) {
    if (!w || !n) return EDYNHIP_ERR_INVALID;
    *n = 0;
    EH_TRY(ensure_built(w));
    w->pool->run([w](uint32_t r) { collect_shard(w, r, false, true, w->carries_extras()); });
    EH_TRY(shard_error(w));
    std::vector<edynhip_manifold> all;
    std::vector<float> rows;
    merge_manifolds(w, all, nullptr, &rows);
    *n = (uint32_t)all.size();
    if (!out7 || all.empty()) return EDYNHIP_OK;
    if (capacity_manifolds < all.size()) return w->fail(EDYNHIP_ERR_CAPACITY, "edynhip_world_get_point_extras: capacity too small");
    for (size_t k = 0; k < all.size(); ++k) extras_row_to_out7(&rows[kExtrasRowFloats * k], out7 + 28 * k);
    return EDYNHIP_OK;
}

}  // extern "C"
