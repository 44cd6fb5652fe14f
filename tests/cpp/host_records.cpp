// Host side of the record hand-over that needs no GPU - what the shim does with an edynhip_record_view, whether one context or a
// multi-device world filled it: import_records (state, presentation, origin, sleeping tags; static, removed and stripped bodies left
// alone; views that cover fewer or more bodies than the registry holds) and the contact table behind apply_contact_events (manifold and
// point entities from an event block in any order, duplicates, unknown ids, a rebuild with no device to ask). Written to run under
// -fsanitize=address,undefined as it stands.
#include <edyn/edyn.hpp>
#include <cstdio>
#include <vector>

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

template <typename T> static size_t count(entt::registry &registry) {
    size_t n = 0;
    registry.view<T>().each([&](auto, auto &) { ++n; });
    return n;
}
static edynhip_contact_event event(uint32_t type, uint32_t step, uint32_t a, uint32_t b, uint64_t id) {
    edynhip_contact_event e{};
    e.type = type; e.step = step; e.body[0] = a; e.body[1] = b; e.point_id = id;
    return e;
}

int main() {
    entt::registry registry;
    auto cfg = edyn::init_config{};
    cfg.num_worker_threads = 3;
    edyn::attach(registry, cfg);
    auto &s = registry.ctx().get<edyn::detail::gpu_stepper>();
    std::vector<entt::entity> bodies;
    auto floor_def = edyn::rigidbody_def{};
    floor_def.kind = edyn::rigidbody_kind::rb_static;
    floor_def.shape = edyn::plane_shape{{0, 1, 0}, 0};
    bodies.push_back(edyn::make_rigidbody(registry, floor_def));
    const uint32_t n = 1500;   // several chunks of the parallel write-back
    for (uint32_t i = 1; i < n; ++i) {
        auto def = edyn::rigidbody_def{};
        def.shape = edyn::box_shape{{0.5f, 0.5f, 0.5f}};
        def.position = {(float)i, 1, 0};
        if (i == 7) def.center_of_mass = edyn::vector3{0.25f, 0, 0};
        bodies.push_back(edyn::make_rigidbody(registry, def));
    }
    REQUIRE(s.bodies.size() == n);

    // ---- import_records
    std::vector<edynhip_body_record> recs(n + 40);   // the view may cover more bodies than the registry holds
    for (uint32_t i = 0; i < recs.size(); ++i) {
        edynhip_body_record &r = recs[i];
        r = edynhip_body_record{};
        r.pos[0] = 10.f + i; r.pos[1] = 2; r.orn[3] = 1; r.linvel[1] = -1.f * i; r.angvel[2] = 0.5f;
        r.present_pos[0] = 20.f + i; r.present_orn[2] = 1;
        r.origin[0] = 30.f + i;
        r.flags = i == 0 ? 0u : (uint32_t)EDYNHIP_RECORD_DYNAMIC;
    }
    recs[7].flags |= EDYNHIP_RECORD_HAS_ORIGIN;
    recs[9].flags |= EDYNHIP_RECORD_ASLEEP;
    recs[11].flags |= EDYNHIP_RECORD_REMOVED;
    registry.remove<edyn::angvel>(bodies[13]);   // stripped by the user since the last update
    edynhip_record_view view{};
    view.records = recs.data(); view.num_bodies = (uint32_t)recs.size(); view.step_index = 1;
    edyn::detail::import_records(registry, s, view, true);
    REQUIRE(registry.get<edyn::position>(bodies[0]).x == 0);                                             // static: the registry is the authority
    for (uint32_t i : {1u, 2u, 511u, 512u, 513u, n - 1}) {
        REQUIRE(registry.get<edyn::position>(bodies[i]).x == 10.f + i && registry.get<edyn::linvel>(bodies[i]).y == -1.f * i);
        REQUIRE(registry.get<edyn::angvel>(bodies[i]).z == 0.5f && registry.get<edyn::orientation>(bodies[i]).w == 1);
        REQUIRE(registry.get<edyn::present_position>(bodies[i]).x == 20.f + i && registry.get<edyn::present_orientation>(bodies[i]).z == 1);
    }
    REQUIRE(registry.get<edyn::origin>(bodies[7]).x == 37.f);
    REQUIRE(registry.all_of<edyn::sleeping_tag>(bodies[9]) && registry.get<edyn::position>(bodies[9]).x == 19.f);
    REQUIRE(registry.get<edyn::present_position>(bodies[9]).x == 9.f);                                   // a sleeping body's presentation stays
    REQUIRE(registry.get<edyn::position>(bodies[11]).x == 11.f && registry.get<edyn::position>(bodies[13]).x == 13.f);   // removed / stripped: left alone
    size_t tagged = 0;
    for (uint32_t i = 0; i < n; ++i) tagged += registry.all_of<edyn::sleeping_tag>(bodies[i]) ? 1 : 0;
    REQUIRE(tagged == 1);
    recs[9].flags &= ~(uint32_t)EDYNHIP_RECORD_ASLEEP;
    view.num_bodies = 10;                                                                                // ... or fewer (a snapshot taken before bodies were added)
    recs[12].pos[0] = -5;
    edyn::detail::import_records(registry, s, view, false);
    REQUIRE(!registry.all_of<edyn::sleeping_tag>(bodies[9]) && registry.get<edyn::position>(bodies[12]).x == 22.f);
    registry.destroy(bodies[5]);
    edyn::detail::sync_removed(registry, s);                                                             // (no device yet: only the tables follow)
    view.num_bodies = (uint32_t)recs.size();
    edyn::detail::import_records(registry, s, view, true);                                               // a destroyed body's slot is skipped
    REQUIRE(s.bodies[5] == entt::null && registry.get<edyn::position>(bodies[12]).x == -5.f);

    // ---- the contact table
    using namespace edyn;
    std::vector<edynhip_contact_event> ev;
    // one step, out of order: the point arrives before its manifold is announced, a duplicate, an unknown point leaves
    ev.push_back(event(EDYNHIP_EVENT_POINT_CREATED, 0, 1, 2, 0x100000005ull));
    ev.push_back(event(EDYNHIP_EVENT_MANIFOLD_CREATED, 0, 1, 2, 0));
    ev.push_back(event(EDYNHIP_EVENT_POINT_CREATED, 0, 1, 2, 0x100000006ull));
    ev.push_back(event(EDYNHIP_EVENT_POINT_CREATED, 0, 1, 2, 0x100000006ull));
    ev.push_back(event(EDYNHIP_EVENT_POINT_DESTROYED, 0, 3, 4, 0x7777ull));
    ev.push_back(event(EDYNHIP_EVENT_MANIFOLD_CREATED, 0, 0, 3, 0));
    ev.push_back(event(EDYNHIP_EVENT_MANIFOLD_CREATED, 0, 2, n + 100, 0));                               // a body the registry does not know
    detail::apply_contact_events(registry, s, ev, EDYNHIP_OK);
    REQUIRE(count<contact_manifold>(registry) == 3 && count<contact_point>(registry) == 2);
    REQUIRE(manifold_exists(registry, bodies[1], bodies[2]) && manifold_exists(registry, bodies[2], bodies[1]) && manifold_exists(registry, bodies[3], bodies[0]));
    REQUIRE(!manifold_exists(registry, bodies[1], bodies[3]));
    REQUIRE(registry.get<contact_manifold>(get_manifold_entity(registry, bodies[1], bodies[2])).num_points == 2);
    size_t neighbours = 0, edges = 0;
    visit_neighbors(registry, bodies[2], [&](entt::entity o) { neighbours += o == bodies[1] ? 1 : 100; });
    visit_edges(registry, bodies[2], [&](entt::entity) { ++edges; });
    REQUIRE(neighbours == 1 && edges == 2);   // (the manifold to the unknown body is an edge without a neighbour)
    // the next step: a point replaced (its end sorts before the beginning), then the manifold goes
    ev.clear();
    ev.push_back(event(EDYNHIP_EVENT_POINT_CREATED, 1, 1, 2, 0x200000005ull));
    ev.push_back(event(EDYNHIP_EVENT_POINT_DESTROYED, 1, 1, 2, 0x100000005ull));
    ev.push_back(event(EDYNHIP_EVENT_MANIFOLD_DESTROYED, 2, 0, 3, 0));
    ev.push_back(event(EDYNHIP_EVENT_MANIFOLD_DESTROYED, 2, 0, 3, 0));
    detail::apply_contact_events(registry, s, ev, EDYNHIP_OK);
    REQUIRE(count<contact_manifold>(registry) == 2 && count<contact_point>(registry) == 2);
    REQUIRE(registry.get<contact_manifold>(get_manifold_entity(registry, bodies[1], bodies[2])).num_points == 2 && !manifold_exists(registry, bodies[0], bodies[3]));
    // a pile hitting the ground: tens of thousands of points come, half of them go (the tables grow and shift)
    ev.clear();
    for (uint32_t k = 0; k < 30000; ++k) ev.push_back(event(EDYNHIP_EVENT_POINT_CREATED, 3, 20 + k % 700, 800 + (k / 4) % 600, (4ull << 32) | k));
    detail::apply_contact_events(registry, s, ev, EDYNHIP_OK);
    REQUIRE(count<contact_point>(registry) == 30002 && s.point_entities.size() == 30002);
    size_t listed = 0;
    registry.view<contact_manifold>().each([&](auto, contact_manifold &m) { listed += m.num_points; });
    REQUIRE(listed == 30002);
    ev.clear();
    for (uint32_t k = 0; k < 30000; k += 2) ev.push_back(event(EDYNHIP_EVENT_POINT_DESTROYED, 4, 20 + k % 700, 800 + (k / 4) % 600, (4ull << 32) | k));
    detail::apply_contact_events(registry, s, ev, EDYNHIP_OK);
    listed = 0;
    registry.view<contact_manifold>().each([&](auto, contact_manifold &m) { listed += m.num_points; });
    REQUIRE(count<contact_point>(registry) == 15002 && listed == 15002);
    // a list that was cut (or a rebuilt world): the entities are rebuilt from the device's manifolds - none without a device
    ev.clear();
    s.contacts_resync = true;
    detail::apply_contact_events(registry, s, ev, EDYNHIP_OK);
    REQUIRE(!s.contacts_resync && count<contact_manifold>(registry) == 0 && count<contact_point>(registry) == 0 && s.manifold_entities.size() == 0 && s.point_entities.size() == 0);
    refresh_contact_points(registry);   // (no device: nothing to refresh)
    edyn::detach(registry);
    std::printf("HOST_RECORDS_OK\n");
    return 0;
}
