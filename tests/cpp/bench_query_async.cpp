// What queries cost the drop-in in execution_mode::asynchronous: edyn::update on the headline pile (bench_update.cpp's scene) with
// 64 rays and 4 boxes requested per update (raycast_async, query_aabb_async) against the same run without queries, alternating, and
// what the same 64 rays and 4 boxes cost per update in sequential mode through edyn::raycast (batch overload) and
// query_procedural_aabb / query_non_procedural_aabb (batch overloads).
//
//   bench_query_async [n=32] [settle=60] [updates=200] [pairs=5]     prints one JSON line "BENCH_QUERY_ASYNC {...}"
#include <edyn/edyn.hpp>
#include <edyn/collision/raycast.hpp>
#include <edyn/collision/query_aabb.hpp>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static float splitmix_uniform(uint64_t i) {   // edyn_amd/scenes.py splitmix64_uniform
    uint64_t z = 0x9E3779B97F4A7C15ull + (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (float)((double)(z >> 40) / (double)(1 << 24));
}
static void build_pile(entt::registry &registry, int n) {   // bench_update.cpp build_pile
    auto floor_def = edyn::rigidbody_def{};
    floor_def.kind = edyn::rigidbody_kind::rb_static;
    floor_def.shape = edyn::plane_shape{{0, 1, 0}, 0};
    edyn::make_rigidbody(registry, floor_def);
    uint64_t b = 0;
    for (int k = 0; k < n; ++k)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j, ++b) {
                const double off = 0.5 * (k & 1);
                float x = (float)((i - (n - 1) / 2.0) * 1.02 + off), y = (float)(0.505 + k * 1.005), z = (float)((j - (n - 1) / 2.0) * 1.02 + off);
                x += (splitmix_uniform(3 * b) * 2 - 1) * 0.005f;
                z += (splitmix_uniform(3 * b + 1) * 2 - 1) * 0.005f;
                const float half = (splitmix_uniform(3 * b + 2) * 2 - 1) * 0.02f * 0.5f;
                auto def = edyn::rigidbody_def{};
                def.mass = 1;
                def.shape = edyn::box_shape{{0.5f, 0.5f, 0.5f}};
                def.position = {x, y, z};
                def.orientation = {0, std::sin(half), 0, std::cos(half)};
                def.sleeping_disabled = true;
                edyn::make_rigidbody(registry, def);
            }
}
constexpr int kRays = 64, kBoxes = 4;
static void queries(int n, int update, std::vector<edyn::vector3> &p0, std::vector<edyn::vector3> &p1, std::vector<edyn::AABB> &boxes) {
    p0.clear(); p1.clear(); boxes.clear();
    const float span = 0.5f * 1.02f * n;
    for (int i = 0; i < kRays; ++i) {   // down into the pile, a different fan every update
        const float x = (splitmix_uniform(1000 + 131 * (uint64_t)update + 2 * i) * 2 - 1) * span, z = (splitmix_uniform(1001 + 131 * (uint64_t)update + 2 * i) * 2 - 1) * span;
        p0.push_back({x, 1.2f * n, z});
        p1.push_back({x + 0.3f, -1, z - 0.2f});
    }
    for (int i = 0; i < kBoxes; ++i) {   // a few bodies each
        const float x = (splitmix_uniform(5000 + 17 * (uint64_t)update + i) * 2 - 1) * span, y = splitmix_uniform(6000 + 17 * (uint64_t)update + i) * n;
        boxes.push_back({{x - 1, y - 1, -1}, {x + 1, y + 1, 1}});
    }
}

struct result { double ms_per_update{0}, query_ms_per_update{0}; long answers{0}; };
static result run(int n, int settle, int updates, edyn::execution_mode mode, bool with_queries) {
    result r;
    entt::registry registry;
    auto cfg = edyn::init_config{};
    cfg.execution_mode = mode;
    cfg.num_solver_velocity_iterations = 10;
    cfg.num_solver_position_iterations = 3;
    edyn::attach(registry, cfg);
    build_pile(registry, n);
    const double dt = (double)cfg.fixed_dt;
    double t = 0.5 * dt;
    edyn::update(registry, t);
    std::vector<edyn::vector3> p0, p1;
    std::vector<edyn::AABB> boxes;
    const bool async = mode == edyn::execution_mode::asynchronous;
    long answers = 0;
    double query_s = 0;
    auto ask = [&](int u) {
        if (!with_queries) return;
        queries(n, u, p0, p1, boxes);
        if (async) {
            for (int i = 0; i < kRays; ++i)
                edyn::raycast_async(registry, p0[i], p1[i], [&answers](edyn::raycast_id_type, const edyn::raycast_result &res, edyn::vector3, edyn::vector3) { answers += res.entity != entt::entity{entt::null}; });
            for (int i = 0; i < kBoxes; ++i)
                edyn::query_aabb_async(registry, boxes[i], [&answers](edyn::query_aabb_id_type, const edyn::query_aabb_result &res) { answers += (long)(res.procedural_entities.size() + res.non_procedural_entities.size()); }, true, true, false);
        } else {
            const double q0 = now_s();
            for (const auto &res : edyn::raycast(registry, p0, p1)) answers += res.entity != entt::entity{entt::null};
            edyn::query_procedural_aabb(registry, boxes, [&answers](size_t, entt::entity) { ++answers; });
            edyn::query_non_procedural_aabb(registry, boxes, [&answers](size_t, entt::entity) { ++answers; });
            query_s += now_s() - q0;
        }
    };
    for (int k = 0; k < settle; ++k) { ask(k); t += dt; edyn::update(registry, t); }
    auto &st = registry.ctx().get<edyn::detail::gpu_stepper>();
    edynhip_synchronize(st.ctx);
    answers = 0; query_s = 0;
    const double t0 = now_s();
    for (int k = 0; k < updates; ++k) { ask(settle + k); t += dt; edyn::update(registry, t); }
    edynhip_synchronize(st.ctx);
    const double t1 = now_s();
    r.ms_per_update = 1e3 * (t1 - t0) / updates;
    r.query_ms_per_update = 1e3 * query_s / updates;
    r.answers = answers;
    edyn::detach(registry);
    return r;
}
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main(int argc, char **argv) {
    const int n = argc > 1 ? std::atoi(argv[1]) : 32;
    const int settle = argc > 2 ? std::atoi(argv[2]) : 60;
    const int updates = argc > 3 ? std::atoi(argv[3]) : 200;
    const int pairs = argc > 4 ? std::atoi(argv[4]) : 5;
    try {
        std::vector<double> plain, with, seq_total, seq_query;
        long answers_async = 0, answers_seq = 0;
        for (int k = 0; k < pairs; ++k) {   // alternating
            plain.push_back(run(n, settle, updates, edyn::execution_mode::asynchronous, false).ms_per_update);
            const result w = run(n, settle, updates, edyn::execution_mode::asynchronous, true);
            with.push_back(w.ms_per_update); answers_async = w.answers;
            const result s = run(n, settle, updates, edyn::execution_mode::sequential, true);
            seq_total.push_back(s.ms_per_update); seq_query.push_back(s.query_ms_per_update); answers_seq = s.answers;
        }
        auto list = [](const std::vector<double> &v) { std::string s = "["; for (size_t i = 0; i < v.size(); ++i) { char b[32]; std::snprintf(b, sizeof b, "%s%.4f", i ? ", " : "", v[i]); s += b; } return s + "]"; };
        std::printf("BENCH_QUERY_ASYNC {\"bodies\": %d, \"updates\": %d, \"rays_per_update\": %d, \"boxes_per_update\": %d, "
                    "\"async_ms_per_update\": %s, \"async_with_queries_ms_per_update\": %s, \"async_added_ms_median\": %.4f, "
                    "\"sequential_with_queries_ms_per_update\": %s, \"sequential_query_ms_per_update\": %s, \"sequential_query_ms_median\": %.4f, "
                    "\"answers_async\": %ld, \"answers_sequential\": %ld}\n",
                    n * n * n + 1, updates, kRays, kBoxes, list(plain).c_str(), list(with).c_str(), median(with) - median(plain),
                    list(seq_total).c_str(), list(seq_query).c_str(), median(seq_query), answers_async, answers_seq);
    } catch (const std::exception &e) {
        std::printf("bench_query_async: %s\n", e.what());
        return 2;
    }
    return 0;
}
