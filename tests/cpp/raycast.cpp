// edyn::raycast through the shim (include/edyn/collision/raycast.hpp): the reference's test/edyn/collision/test_raycast.cpp,
// a vertical probe onto a box resting on a plane, the ignore list, a registry edit seen without an update, the batch overload
// against single calls, and the rejection in execution_mode::asynchronous. Prints RAYCAST_OK 1 when every check holds.
#include <edyn/edyn.hpp>
#include <edyn/collision/raycast.hpp>
#include <cmath>
#include <cstdio>
#include <variant>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++failures; } } while (0)

int main() {
    {   // test_raycast.cpp, raycast_box
        entt::registry registry;
        auto config = edyn::init_config{};
        config.execution_mode = edyn::execution_mode::sequential;
        edyn::attach(registry, config);
        auto def = edyn::rigidbody_def{};
        def.shape = edyn::box_shape{{0.5f, 0.5f, 0.5f}};
        def.position = {0.5f, 0.5f, 0.5f};
        def.kind = edyn::rigidbody_kind::rb_static;
        auto box_entity = edyn::make_rigidbody(registry, def);
        edyn::update(registry);
        auto result = edyn::raycast(registry, edyn::vector3{2, 2, 2}, edyn::vector3{0, 0, 0});
        CHECK(result.entity == box_entity);
        CHECK(result.fraction == 0.5f);
        CHECK(std::holds_alternative<edyn::box_raycast_info>(result.info_var));
        result = edyn::raycast(registry, edyn::vector3{0.5f, 2, 0.5f}, edyn::vector3{0.5f, 0, 0.5f});
        CHECK(result.fraction == 0.5f);
        CHECK(std::holds_alternative<edyn::box_raycast_info>(result.info_var));
        CHECK(std::get<edyn::box_raycast_info>(result.info_var).face_index == 2);
        edyn::detach(registry);
    }
    {   // a box resting on a plane: probes from above, the ignore list, an edit without update, the batch overload
        entt::registry registry;
        edyn::attach(registry);
        auto floor_def = edyn::rigidbody_def{};
        floor_def.kind = edyn::rigidbody_kind::rb_static;
        floor_def.shape = edyn::plane_shape{{0, 1, 0}, 0};
        auto floor = edyn::make_rigidbody(registry, floor_def);
        auto def = edyn::rigidbody_def{};
        def.position = {0, 0.5f, 0};
        def.shape = edyn::box_shape{{0.5f, 0.5f, 0.5f}};
        auto box = edyn::make_rigidbody(registry, def);
        double t = 0;
        for (int i = 0; i < 60; ++i) { t += 1.0 / 60 + 1e-6; edyn::update(registry, t); }
        const float top = registry.get<edyn::position>(box).y + 0.5f;
        auto r = edyn::raycast(registry, edyn::vector3{0, 5, 0}, edyn::vector3{0, -5, 0});
        CHECK(r.entity == box);
        CHECK(std::fabs((5 - 10 * r.fraction) - top) < 2e-3f);
        CHECK(std::fabs(r.normal.y - 1) < 1e-3f);
        r = edyn::raycast(registry, edyn::vector3{0, 5, 0}, edyn::vector3{0, -5, 0}, {box});
        CHECK(r.entity == floor);
        CHECK(r.fraction == 0.5f);
        CHECK(std::holds_alternative<std::monostate>(r.info_var));
        r = edyn::raycast(registry, edyn::vector3{3, 5, 0}, edyn::vector3{3, 4, 0});   // misses everything
        CHECK(r.entity == entt::entity{entt::null});
        // an edit of the registry, no update: the ray sees the box where the registry now has it
        registry.get<edyn::position>(box) = edyn::position{edyn::vector3{10, 3, 0}};
        edyn::refresh(registry);
        r = edyn::raycast(registry, edyn::vector3{10, 5, 0}, edyn::vector3{10, -5, 0});
        CHECK(r.entity == box);
        CHECK(std::fabs((5 - 10 * r.fraction) - 3.5f) < 1e-3f);
        // the batch overload equals single calls
        std::vector<edyn::vector3> p0, p1;
        for (int i = 0; i < 64; ++i) {
            p0.push_back(edyn::vector3{-2.0f + 0.2f * i, 6, 0.1f * (i % 7)});
            p1.push_back(edyn::vector3{20.0f - 0.1f * i, -1, 0.05f * (i % 5)});
        }
        auto batch = edyn::raycast(registry, p0, p1, {floor});
        CHECK(batch.size() == p0.size());
        int hits = 0;
        for (size_t i = 0; i < p0.size(); ++i) {
            auto one = edyn::raycast(registry, p0[i], p1[i], {floor});
            CHECK(one.entity == batch[i].entity);
            CHECK(one.fraction == batch[i].fraction);
            CHECK(one.info_var.index() == batch[i].info_var.index());
            hits += batch[i].entity != entt::entity{entt::null};
        }
        CHECK(hits > 0);
        edyn::detach(registry);
    }
    {   // execution_mode::asynchronous: the reference asks for raycast_async; it is rejected loudly
        entt::registry registry;
        auto config = edyn::init_config{};
        config.execution_mode = edyn::execution_mode::asynchronous;
        edyn::attach(registry, config);
        auto def = edyn::rigidbody_def{};
        def.shape = edyn::box_shape{{0.5f, 0.5f, 0.5f}};
        edyn::make_rigidbody(registry, def);
        bool threw = false;
        try {
            edyn::raycast(registry, edyn::vector3{0, 5, 0}, edyn::vector3{0, -5, 0});
        } catch (const edyn::stepper_error &e) {
            threw = std::string(e.what()).find("raycast_async") != std::string::npos;
        }
        CHECK(threw);
        edyn::detach(registry);
    }
    std::printf("RAYCAST_OK %d\n", failures == 0 ? 1 : 0);
    return failures == 0 ? 0 : 1;
}
