// Edits of a RUNNING world through the registry API, on one device and on init_config::devices = {0, 0}: a body made, a constraint
// made, a body destroyed, a settings change and an edyn::refresh-ed velocity kick. The shim forwards each of them to the running
// multi-device world (edynhip_world_add_bodies / _add_joints / _remove_bodies / _set_params / _set_state) instead of rebuilding it, so
// the two registries agree bit for bit at EVERY step - also after the edits, where a rebuilt world had lost its contacts' warm start.
#include <edyn/edyn.hpp>
#include <cmath>
#include <cstdio>
#include <vector>

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// the scene of multi_shim.cpp: four small piles, a hinge door, a ball rolling from the first pile to the second
static void build(entt::registry &registry, std::vector<entt::entity> &bodies) {
    auto floor_def = edyn::rigidbody_def{};
    floor_def.kind = edyn::rigidbody_kind::rb_static;
    floor_def.shape = edyn::plane_shape{{0, 1, 0}, 0};
    edyn::make_rigidbody(registry, floor_def);
    for (int site = 0; site < 4; ++site)
        for (int k = 0; k < 8; ++k) {
            auto def = edyn::rigidbody_def{};
            def.mass = 1;
            def.shape = edyn::box_shape{{0.5f, 0.5f, 0.5f}};
            def.position = {7.0f * site + 1.02f * (k % 2), 0.505f + 1.005f * ((k / 2) % 2), 1.02f * (k / 4)};
            def.sleeping_disabled = true;
            bodies.push_back(edyn::make_rigidbody(registry, def));
        }
    auto post = edyn::rigidbody_def{}; post.kind = edyn::rigidbody_kind::rb_static; post.position = {30.0f, 2.0f, 0};
    auto door = edyn::rigidbody_def{}; door.mass = 1; door.position = {31.0f, 2.0f, 0}; door.shape = edyn::box_shape{{0.5f, 0.5f, 0.1f}}; door.sleeping_disabled = true;
    const auto e_post = edyn::make_rigidbody(registry, post), e_door = edyn::make_rigidbody(registry, door);
    edyn::make_constraint<edyn::hinge_constraint>(registry, e_post, e_door, [](edyn::hinge_constraint &h) {
        h.pivot[0] = {0, 0, 0}; h.pivot[1] = {-1.0f, 0, 0}; h.set_axes({0, 0, 1}, {0, 0, 1});
    });
    bodies.push_back(e_door);
    auto ball = edyn::rigidbody_def{};
    ball.mass = 1; ball.shape = edyn::sphere_shape{0.5f}; ball.position = {3.2f, 0.5f, 0.5f}; ball.linvel = {4.0f, 0, 0}; ball.sleeping_disabled = true;
    bodies.push_back(edyn::make_rigidbody(registry, ball));
}

static void edit(entt::registry &registry, std::vector<entt::entity> &b, int step) {
    if (step == 60) {          // a box dropped onto the first pile
        auto def = edyn::rigidbody_def{};
        def.mass = 1; def.shape = edyn::box_shape{{0.5f, 0.5f, 0.5f}}; def.position = {0.5f, 3.2f, 0.5f}; def.sleeping_disabled = true;
        b.push_back(edyn::make_rigidbody(registry, def));
    } else if (step == 80) {   // a hinge from a box of the first pile to a box of the second: its pivots meet where the first box is now
        const auto &pa = registry.get<edyn::position>(b[7]), &pb = registry.get<edyn::position>(b[10]);
        const edyn::vector3 arm{pa.x - pb.x, pa.y - pb.y, pa.z - pb.z};
        edyn::make_constraint<edyn::hinge_constraint>(registry, b[7], b[10], [&](edyn::hinge_constraint &h) {
            h.pivot[0] = {0, 0, 0}; h.pivot[1] = arm; h.set_axes({0, 0, 1}, {0, 0, 1});
        });
    } else if (step == 100) {
        registry.destroy(b[3]);
    } else if (step == 120) {  // settings and an edited state
        edyn::set_gravity(registry, {0, -5.0f, 0});
        registry.get<edyn::linvel>(b[20]) = edyn::linvel{{0, 3.0f, 0}};
        edyn::refresh(registry);
    }
}

int main() {
    entt::registry one, many;
    auto cfg = edyn::init_config{};
    cfg.num_solver_velocity_iterations = 10;
    cfg.materialize_contacts = false;
    edyn::attach(one, cfg);
    cfg.devices = {0, 0};
    edyn::attach(many, cfg);
    std::vector<entt::entity> b1, b2;
    build(one, b1); build(many, b2);
    double t = 0;
    for (int step = 0; step <= 160; ++step) {
        t += 1.0 / 60;
        edyn::update(one, t); edyn::update(many, t);
        REQUIRE(b1.size() == b2.size());
        for (size_t k = 0; k < b1.size(); ++k) {
            if (!one.valid(b1[k])) { REQUIRE(!many.valid(b2[k])); continue; }
            const auto &p = one.get<edyn::position>(b1[k]), &q = many.get<edyn::position>(b2[k]);
            const auto &o = one.get<edyn::orientation>(b1[k]), &u = many.get<edyn::orientation>(b2[k]);
            const auto &v = one.get<edyn::linvel>(b1[k]), &w = many.get<edyn::linvel>(b2[k]);
            const auto &a = one.get<edyn::angvel>(b1[k]), &c = many.get<edyn::angvel>(b2[k]);
            const bool same = p.x == q.x && p.y == q.y && p.z == q.z && o.x == u.x && o.y == u.y && o.z == u.z && o.w == u.w &&
                              v.x == w.x && v.y == w.y && v.z == w.z && a.x == c.x && a.y == c.y && a.z == c.z;
            if (!same) {
                std::printf("FAILED: body %zu differs at step %d (%.9g %.9g %.9g vs %.9g %.9g %.9g)\n", k, step, p.x, p.y, p.z, q.x, q.y, q.z);
                return 1;
            }
        }
        edit(one, b1, step); edit(many, b2, step);
    }
    REQUIRE(one.get<edyn::position>(b1.back()).y < 3.0f);            // the dropped box came down
    REQUIRE(one.get<edyn::linvel>(b1[20]).y < 2.9f);                 // the kick was taken and gravity worked on it since
    std::printf("MULTI_EDIT_OK\n");
    return 0;
}
