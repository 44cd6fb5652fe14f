// The registry's contact entities against the device, after every update (init_config::materialize_contacts): the contact_manifold /
// contact_point entities the shim builds from the device's events must be, as sets, the device's manifolds (by body pair, with their
// point counts) and points (by point id and parent pair), in every write-back path - sequential updates of two steps, step callbacks
// (one step per launch), a long frame clamped by max_steps_per_update (timed steps), and the asynchronous mode, which is held to a
// synchronous twin one update behind, through a landing whose events overflow the snapshot's slot and a user edit right after it.
#include <edyn/edyn.hpp>
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <tuple>
#include <vector>

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct mirror {
    std::set<std::tuple<uint32_t, uint32_t, uint32_t>> manifolds;   // (body A, body B, num_points)
    std::set<std::tuple<uint64_t, uint32_t, uint32_t>> points;      // (point id, parent's body A, parent's body B)
    bool operator==(const mirror &o) const { return manifolds == o.manifolds && points == o.points; }
};

static uint32_t index_of(entt::registry &registry, entt::entity e) {
    REQUIRE(e != entt::null && registry.valid(e) && registry.all_of<edyn::detail::body_index>(e));
    return registry.get<edyn::detail::body_index>(e).value;
}

// What the registry holds, checked for consistency on its own: every point's parent is a live manifold, each manifold's num_points
// is the number of points that name it, every contact_point_list entity is a whole contact point.
static mirror registry_mirror(entt::registry &registry) {
    mirror m;
    std::map<entt::entity, uint32_t> named;
    size_t manifolds = 0, lists = 0, points = 0;
    registry.view<edyn::contact_point_list>().each([&](entt::entity e, edyn::contact_point_list &l) {
        ++lists;
        REQUIRE(registry.valid(l.parent) && registry.all_of<edyn::contact_manifold>(l.parent));
        REQUIRE(registry.all_of<edyn::contact_point>(e));
        const auto &pm = registry.get<edyn::contact_manifold>(l.parent);
        const bool fresh = m.points.insert({l.id, index_of(registry, pm.body[0]), index_of(registry, pm.body[1])}).second;
        REQUIRE(fresh);   // one entity per point id
        ++named[l.parent];
    });
    registry.view<edyn::contact_point>().each([&](entt::entity, edyn::contact_point &) { ++points; });
    REQUIRE(points == lists);
    registry.view<edyn::contact_manifold>().each([&](entt::entity e, edyn::contact_manifold &cm) {
        ++manifolds;
        REQUIRE(cm.num_points == named[e]);
        const bool fresh = m.manifolds.insert({index_of(registry, cm.body[0]), index_of(registry, cm.body[1]), cm.num_points}).second;
        REQUIRE(fresh);   // one entity per pair
    });
    REQUIRE(m.manifolds.size() == manifolds);
    return m;
}

// What the device holds (edynhip_get_manifolds / edynhip_get_point_ids through the stepper's context).
static mirror device_mirror(entt::registry &registry) {
    auto &s = registry.ctx().get<edyn::detail::gpu_stepper>();
    mirror m;
    if (!s.ctx) return m;
    uint32_t n = 0;
    REQUIRE(edynhip_num_manifolds(s.ctx, &n) == EDYNHIP_OK);
    std::vector<edynhip_manifold> recs(n);
    std::vector<uint64_t> ids((size_t)4 * n);
    if (n) {
        REQUIRE(edynhip_get_manifolds(s.ctx, recs.data(), n, &n) == EDYNHIP_OK);
        REQUIRE(edynhip_get_point_ids(s.ctx, ids.data(), n, &n) == EDYNHIP_OK);
    }
    for (uint32_t i = 0; i < n; ++i) {
        m.manifolds.insert({recs[i].body[0], recs[i].body[1], recs[i].num_points});
        for (uint32_t k = 0; k < recs[i].num_points; ++k) m.points.insert({ids[(size_t)4 * i + k], recs[i].body[0], recs[i].body[1]});
    }
    return m;
}

static int checks = 0;
static void check_mirror(entt::registry &registry, const char *what) {
    const mirror r = registry_mirror(registry), d = device_mirror(registry);
    if (!(r.manifolds == d.manifolds) || !(r.points == d.points)) {
        std::printf("FAILED mirror (%s, check %d): registry %zu manifolds / %zu points, device %zu / %zu\n", what, checks,
                    r.manifolds.size(), r.points.size(), d.manifolds.size(), d.points.size());
        std::exit(1);
    }
    ++checks;
}

static edyn::init_config config(float dt = 1.0f / 60) {
    auto cfg = edyn::init_config{};
    cfg.fixed_dt = dt;
    cfg.num_solver_velocity_iterations = 10;
    cfg.num_solver_position_iterations = 3;
    return cfg;   // island_sleeping and materialize_contacts: the defaults (on)
}
static void add_floor(entt::registry &registry, float friction = 0.5f) {
    auto def = edyn::rigidbody_def{};
    def.kind = edyn::rigidbody_kind::rb_static;
    def.shape = edyn::plane_shape{{0, 1, 0}, 0};
    def.material = edyn::material{};
    def.material->friction = friction;
    edyn::make_rigidbody(registry, def);
}
static entt::entity add_box(entt::registry &registry, edyn::vector3 pos, edyn::vector3 vel = {0, 0, 0}, float friction = 0.5f) {
    auto def = edyn::rigidbody_def{};
    def.mass = 1;
    def.shape = edyn::box_shape{{0.5f, 0.5f, 0.5f}};
    def.position = pos;
    def.linvel = vel;
    def.material = edyn::material{};
    def.material->friction = friction;
    return edyn::make_rigidbody(registry, def);
}
static void add_pile(entt::registry &registry, float x0) {   // 3 x 3 x 3, as scenes.box_pile lays the bricks (no jitter)
    for (int i = 0; i < 27; ++i)
        add_box(registry, {x0 + 1.02f * (i % 3) + ((i / 3) % 2 ? 0.51f : 0.0f), 0.505f + 1.005f * ((i / 3) % 3), 1.02f * (i / 9)});
}
static int awake(entt::registry &registry) {   // dynamic bodies without sleeping_tag
    int n = 0;
    for (entt::entity e : registry.ctx().get<edyn::detail::gpu_stepper>().bodies)
        n += e != entt::null && registry.all_of<edyn::dynamic_tag>(e) && !registry.all_of<edyn::sleeping_tag>(e);
    return n;
}
static bool all_asleep(entt::registry &registry) { return awake(registry) == 0; }

// A pile that settles and sleeps, is woken by a dropped box and sleeps again; `frame` s per update, checked after every update.
static void pile_sleep_wake(entt::registry &registry, double frame, double &t, const char *what) {
    add_floor(registry);
    add_pile(registry, 0);
    int updates = 0;
    while (!all_asleep(registry)) { t += frame; edyn::update(registry, t); check_mirror(registry, what); REQUIRE(++updates < 2000); }
    for (int i = 0; i < 10; ++i) { t += frame; edyn::update(registry, t); check_mirror(registry, what); }
    add_box(registry, {1.1f, 5.5f, 1.02f});
    bool woke = false;
    for (updates = 0; !(woke && all_asleep(registry)); ++updates) {
        REQUIRE(updates < 2000);
        t += frame; edyn::update(registry, t); check_mirror(registry, what);
        woke = woke || awake(registry) > 1;
    }
}

static int callback_checks = 0;
static void post_step_check(entt::registry &registry) { check_mirror(registry, "post-step callback"); ++callback_checks; }
static void pre_step_nothing(entt::registry &) {}

static std::vector<entt::entity> landing_grid(entt::registry &registry) {   // contact_scenes.landing_grid: 32 x 32 boxes, 2 m apart, 0.5 m up
    add_floor(registry);
    std::vector<entt::entity> boxes;
    for (int i = 0; i < 1024; ++i) boxes.push_back(add_box(registry, {2.0f * (i % 32), 1.0f, 2.0f * (i / 32)}));
    return boxes;
}

int main() {
    // ---- sequential, 30 Hz frames at 60 Hz steps: collapse, sleep, wake, sleep
    {
        entt::registry registry;
        edyn::attach(registry, config());
        double t = 0;
        pile_sleep_wake(registry, 1.0 / 30, t, "pile, 30 Hz");
        edyn::detach(registry);
    }
    // ---- step callbacks: one step per launch, the write-back after each (checked inside the post-step callback too)
    {
        entt::registry registry;
        edyn::attach(registry, config());
        edyn::set_pre_step_callback(registry, &pre_step_nothing);
        edyn::set_post_step_callback(registry, &post_step_check);
        double t = 0;
        pile_sleep_wake(registry, 1.0 / 30, t, "pile, step callbacks");
        REQUIRE(callback_checks > 100);
        edyn::detach(registry);
    }
    // ---- long frames clamped by max_steps_per_update: timed steps with stretched stamps
    {
        entt::registry registry;
        edyn::attach(registry, config());
        edyn::set_max_steps_per_update(registry, 3);
        double t = 0;
        pile_sleep_wake(registry, 0.2, t, "pile, clamped long frames");
        edyn::detach(registry);
    }
    // ---- asynchronous mode against a synchronous twin: the async registry's contact entities after update k are the sync registry's
    // after update k - 1. A landing grid overflows the snapshot's event slot: the async shim then rebuilds its contact entities from the
    // device's current manifolds, which already include the update in flight (the twins agree on the same update there), and skips
    // the in-flight events when they arrive. A user edit (edyn::refresh, nothing changed) right after that must not apply them either.
    {
        entt::registry sreg, areg;
        auto scfg = config(), acfg = config();
        acfg.execution_mode = edyn::execution_mode::asynchronous;
        edyn::attach(sreg, scfg);
        edyn::attach(areg, acfg);
        landing_grid(sreg);
        landing_grid(areg);
        add_pile(sreg, 70); add_pile(areg, 70);
        auto &as = areg.ctx().get<edyn::detail::gpu_stepper>();
        std::vector<mirror> sync_after;   // the sync twin's mirror after each update
        double t = 0;
        bool overflowed = false, edited = false;
        for (int u = 0; u < 60; ++u) {
            if (overflowed && !edited) { edyn::refresh(sreg); edyn::refresh(areg); edited = true; }
            t += 1.0 / 30;
            const uint32_t stale_before = as.events_stale_through;
            edyn::update(sreg, t); edyn::update(areg, t);
            check_mirror(sreg, "synchronous twin");
            sync_after.push_back(registry_mirror(sreg));
            const mirror am = registry_mirror(areg);
            if (as.events_stale_through != stale_before) {   // rebuilt from the current manifolds in this update
                REQUIRE(am == sync_after[u]);
                overflowed = true;
            } else if (u > 0) {
                if (!(am == sync_after[u - 1])) {
                    std::printf("FAILED async mirror after update %d: %zu manifolds / %zu points, sync twin one update earlier %zu / %zu\n", u,
                                am.manifolds.size(), am.points.size(), sync_after[u - 1].manifolds.size(), sync_after[u - 1].points.size());
                    return 1;
                }
            }
        }
        REQUIRE(overflowed && edited && as.events_stale_through > 0);
        REQUIRE(sync_after.back().points.size() >= 4 * 1024);
        edyn::detach(sreg); edyn::detach(areg);
    }
    std::printf("CONTACT_MIRROR_OK %d checks\n", checks);
    return 0;
}
