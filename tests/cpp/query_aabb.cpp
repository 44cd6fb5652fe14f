// edyn::query_procedural_aabb / query_non_procedural_aabb through the shim. The forwarding header is included alone and first: it must
// compile on its own. Entities returned for a box around one body, none after registry.destroy, the batched overload against single
// calls, and stepper_error in execution_mode::asynchronous and on a world over several devices. Prints QUERY_AABB_OK 1 when every
// check holds.
#include <edyn/collision/query_aabb.hpp>
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++failures; } } while (0)

static edyn::AABB around(edyn::vector3 c, float h) { return edyn::AABB{{c.x - h, c.y - h, c.z - h}, {c.x + h, c.y + h, c.z + h}}; }

template <typename Config>
static bool throws(Config config, const char *needle) {
    entt::registry registry;
    edyn::attach(registry, config);
    auto def = edyn::rigidbody_def{};
    def.shape = edyn::box_shape{{0.5f, 0.5f, 0.5f}};
    edyn::make_rigidbody(registry, def);
    bool threw = false;
    try {
        edyn::query_procedural_aabb(registry, around({0, 0, 0}, 1), [](entt::entity) {});
    } catch (const edyn::stepper_error &e) {
        threw = std::string(e.what()).find(needle) != std::string::npos;
    }
    bool threw_np = false;
    try {
        edyn::query_non_procedural_aabb(registry, std::vector<edyn::AABB>{around({0, 0, 0}, 1)}, [](size_t, entt::entity) {});
    } catch (const edyn::stepper_error &) {
        threw_np = true;
    }
    edyn::detach(registry);
    return threw && threw_np;
}

int main() {
    {
        entt::registry registry;
        edyn::attach(registry);
        auto floor_def = edyn::rigidbody_def{};
        floor_def.kind = edyn::rigidbody_kind::rb_static;
        floor_def.shape = edyn::plane_shape{{0, 1, 0}, 0};
        auto floor = edyn::make_rigidbody(registry, floor_def);
        std::vector<entt::entity> boxes;
        for (int i = 0; i < 8; ++i) {   // a row of boxes 3 apart, every other one static
            auto def = edyn::rigidbody_def{};
            def.position = {3.0f * i, 0.5f, 0};
            def.shape = edyn::box_shape{{0.5f, 0.5f, 0.5f}};
            if (i % 2) def.kind = edyn::rigidbody_kind::rb_static;
            boxes.push_back(edyn::make_rigidbody(registry, def));
        }
        double t = 0;
        for (int i = 0; i < 10; ++i) { t += 1.0 / 60 + 1e-6; edyn::update(registry, t); }
        // a box around one dynamic body: that entity and nothing else; static bodies and the floor are non-procedural
        std::vector<entt::entity> got;
        edyn::query_procedural_aabb(registry, around({6, 0.5f, 0}, 0.3f), [&](entt::entity e) { got.push_back(e); });
        CHECK(got.size() == 1 && got[0] == boxes[2]);
        got.clear();
        edyn::query_non_procedural_aabb(registry, around({6, 0.5f, 0}, 0.3f), [&](entt::entity e) { got.push_back(e); });
        CHECK(got.empty());   // (the plane's half-space box ends at y = 0, grown to 0.1)
        got.clear();
        edyn::query_non_procedural_aabb(registry, around({3, 0.5f, 0}, 0.3f), [&](entt::entity e) { got.push_back(e); });
        CHECK(got.size() == 1 && got[0] == boxes[1]);
        got.clear();
        edyn::query_non_procedural_aabb(registry, around({3, 0.5f, 0}, 0.45f), [&](entt::entity e) { got.push_back(e); });
        CHECK(got.size() == 2 && got[0] == floor && got[1] == boxes[1]);
        // the fat box: AABB + 0.1 is touched, one step beyond is not
        got.clear();
        edyn::query_procedural_aabb(registry, edyn::AABB{{6.55f, 0.4f, -0.1f}, {6.59f, 0.6f, 0.1f}}, [&](entt::entity e) { got.push_back(e); });
        CHECK(got.size() == 1 && got[0] == boxes[2]);
        got.clear();
        edyn::query_procedural_aabb(registry, edyn::AABB{{6.7f, 0.4f, -0.1f}, {6.9f, 0.6f, 0.1f}}, [&](entt::entity e) { got.push_back(e); });
        CHECK(got.empty());
        // the batched overload equals the single calls
        std::vector<edyn::AABB> qs;
        for (int i = 0; i < 40; ++i) qs.push_back(around({0.7f * i - 2, 0.5f, 0}, 0.2f + 0.1f * (i % 9)));
        std::vector<std::vector<entt::entity>> batch_p(qs.size()), batch_np(qs.size());
        edyn::query_procedural_aabb(registry, qs, [&](size_t q, entt::entity e) { batch_p[q].push_back(e); });
        edyn::query_non_procedural_aabb(registry, qs, [&](size_t q, entt::entity e) { batch_np[q].push_back(e); });
        size_t hits = 0;
        for (size_t i = 0; i < qs.size(); ++i) {
            std::vector<entt::entity> one_p, one_np;
            edyn::query_procedural_aabb(registry, qs[i], [&](entt::entity e) { one_p.push_back(e); });
            edyn::query_non_procedural_aabb(registry, qs[i], [&](entt::entity e) { one_np.push_back(e); });
            CHECK(one_p == batch_p[i]);
            CHECK(one_np == batch_np[i]);
            hits += one_p.size();
        }
        CHECK(hits > 8);
        // registry.destroy: never reported again (no update in between)
        registry.destroy(boxes[2]);
        got.clear();
        edyn::query_procedural_aabb(registry, around({6, 0.5f, 0}, 0.3f), [&](entt::entity e) { got.push_back(e); });
        CHECK(got.empty());
        got.clear();
        edyn::query_procedural_aabb(registry, around({12, 0.5f, 0}, 0.3f), [&](entt::entity e) { got.push_back(e); });
        CHECK(got.size() == 1 && got[0] == boxes[4]);
        edyn::query_aabb_result result;
        edyn::query_procedural_aabb(registry, around({0, 0, 0}, 100), [&](entt::entity e) { result.procedural_entities.push_back(e); });
        edyn::query_non_procedural_aabb(registry, around({0, 0, 0}, 100), [&](entt::entity e) { result.non_procedural_entities.push_back(e); });
        CHECK(result.procedural_entities.size() == 3 && result.non_procedural_entities.size() == 5 && result.island_entities.empty());
        edyn::detach(registry);
    }
    {
        auto config = edyn::init_config{};
        config.execution_mode = edyn::execution_mode::asynchronous;
        CHECK(throws(config, "query_aabb_async"));
        auto multi = edyn::init_config{};
        multi.devices = {0, 0};
        CHECK(throws(multi, "several devices"));
    }
    {   // the asynchronous queries are declared and rejected loudly in every mode
        entt::registry registry;
        edyn::attach(registry);
        bool threw = false;
        try {
            edyn::query_aabb_async(registry, around({0, 0, 0}, 1), 0, true, true, false);
        } catch (const edyn::stepper_error &) {
            threw = true;
        }
        CHECK(threw);
#if __has_include(<entt/entt.hpp>)
        edyn::query_aabb_delegate_type delegate{};   // the reference's alias, where the registry library has delegates
        threw = false;
        try {
            edyn::query_aabb_of_interest_async(registry, around({0, 0, 0}, 1), delegate);
        } catch (const edyn::stepper_error &) {
            threw = true;
        }
        CHECK(threw);
#endif
        edyn::detach(registry);
    }
    std::printf("QUERY_AABB_OK %d\n", failures == 0 ? 1 : 0);
    return failures == 0 ? 0 : 1;
}
