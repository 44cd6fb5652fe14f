/* edynhip.h — C-ABI of the MI355X-native stepper that replaces Edyn's per-step simulation loop.
 *
 * The reference (xissburg/edyn v1.3.1) has no FFI layer: its seam is the C++ API over a caller-owned
 * entt::registry. This C-ABI sits UNDER a header-only C++ shim (include/edyn/edyn.hpp in this repo)
 * that keeps edyn::attach / edyn::update / edyn::make_rigidbody, so each entry point below cites the
 * reference interface it stands in for:
 *
 *   edynhip_create / edynhip_destroy   <- edyn::attach / edyn::detach            include/edyn/edyn.hpp:66-77, src/edyn/edyn.cpp:73-197
 *                                         + settings{fixed_dt, iterations, gravity} include/edyn/context/settings.hpp:21-57
 *   edynhip_set_bodies                 <- edyn::make_rigidbody(registry, def)     include/edyn/util/rigidbody.hpp:29-93, src/edyn/util/rigidbody.cpp:47-191
 *   edynhip_set_joints                 <- edyn::make_constraint<point|hinge>      include/edyn/util/constraint_util.hpp:38-54
 *   edynhip_step                       <- edyn::step_simulation / one fixed step of edyn::update
 *                                                                                 src/edyn/simulation/stepper_sequential.cpp:71-102,121-147
 *   edynhip_get_state / set_state      <- reading/patching position, orientation, linvel, angvel pools
 *                                                                                 include/edyn/comp/{position,orientation,linvel,angvel}.hpp
 *   edynhip_get_manifolds / set_       <- contact_manifold + contact_point* components
 *                                                                                 include/edyn/collision/contact_manifold.hpp:14-22, contact_point.hpp:17-58
 *   edynhip_get_timings / get_stats    <- profile_timers / profile_counters       include/edyn/context/profile.hpp:8-27
 *
 * Conventions: plain pointers and sizes, host arrays are borrowed for the duration of the call only,
 * every function returns 0 on success or a negative edynhip_status; nothing throws across the boundary.
 * A context is bound to one GPU and is single-threaded, like the reference's sequential stepper.
 * There is NO CPU fallback: if no gfx950 device is usable, edynhip_create fails with EDYNHIP_ERR_NO_DEVICE.
 */
#ifndef EDYNHIP_H
#define EDYNHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct edynhip_ctx edynhip_ctx;

typedef enum {
    EDYNHIP_OK = 0,
    EDYNHIP_ERR_INVALID = -1,       /* bad argument */
    EDYNHIP_ERR_NO_DEVICE = -2,     /* no usable HIP device */
    EDYNHIP_ERR_HIP = -3,           /* a HIP runtime call failed (see edynhip_last_error) */
    EDYNHIP_ERR_CAPACITY = -4,      /* pair / manifold capacity exceeded */
    EDYNHIP_ERR_COLOURS = -5,       /* a body has more joints than joint colours (64); contacts have no such limit */
    EDYNHIP_ERR_UNSUPPORTED = -6,   /* feature outside the hot-path scope (e.g. a cylinder / polyhedron / mesh shape) */
    EDYNHIP_ERR_INTERNAL = -7       /* a device-side invariant failed (e.g. the dataflow solve timed out waiting for a hand-off) */
} edynhip_status;

/* rigidbody_kind (include/edyn/util/rigidbody.hpp:22-27) */
enum { EDYNHIP_KIND_DYNAMIC = 0, EDYNHIP_KIND_KINEMATIC = 1, EDYNHIP_KIND_STATIC = 2 };
/* shapes on the hot path; NONE = amorphous body */
enum { EDYNHIP_SHAPE_NONE = 0, EDYNHIP_SHAPE_BOX = 1, EDYNHIP_SHAPE_SPHERE = 2, EDYNHIP_SHAPE_PLANE = 3,
       EDYNHIP_SHAPE_CAPSULE = 4, /* shape_param = radius, half_length, axis (0 x, 1 y, 2 z): shapes/capsule_shape.hpp:17-30 */
       EDYNHIP_SHAPE_CYLINDER = 5, /* shape_param = radius, half_length, axis: shapes/cylinder_shape.hpp:22-25 */
       EDYNHIP_SHAPE_POLYHEDRON = 6 /* shape_param[0] = id of a mesh made with edynhip_create_convex_mesh: shapes/polyhedron_shape.hpp:11-43 */ };
enum { EDYNHIP_JOINT_POINT = 0, EDYNHIP_JOINT_HINGE = 1,
       EDYNHIP_JOINT_DISTANCE = 2,       /* distance_constraint.cpp:7-31; params[0] = distance; impulse slot 0 */
       EDYNHIP_JOINT_SOFT_DISTANCE = 3,  /* soft_distance_constraint.cpp:8-62; params = distance, stiffness, damping; slots 0 spring, 1 damping */
       EDYNHIP_JOINT_CONE = 4,           /* cone_constraint.cpp:12-104; frames + params through edynhip_set_joint_definition */
       EDYNHIP_JOINT_CVJOINT = 5,        /* cvjoint_constraint.cpp:12-302; frames + params through edynhip_set_joint_definition */
       EDYNHIP_JOINT_GRAVITY = 6,        /* gravity_constraint.cpp:6-34: Newtonian attraction between the two bodies; impulse slot 0 */
       EDYNHIP_JOINT_GENERIC = 7,        /* generic_constraint.cpp:10-330; frames + 6 x 10 parameters through edynhip_set_generic_definition */
       EDYNHIP_JOINT_NULL = 8            /* null_constraint.hpp:12-17: no rows - an edge of the island graph that keeps two bodies in one island */ };
/* contact_normal_attachment (include/edyn/collision/contact_normal_attachment.hpp:17-21) */
enum { EDYNHIP_ATTACH_NONE = 0, EDYNHIP_ATTACH_ON_A = 1, EDYNHIP_ATTACH_ON_B = 2 };

typedef struct {
    int32_t device;                  /* HIP device ordinal */
    uint32_t max_bodies;
    uint32_t max_manifolds;          /* 0 = 16 * max_bodies + 1024 */
    uint32_t max_joints;
    float fixed_dt;                  /* settings.fixed_dt, default 1/60 */
    uint32_t num_velocity_iterations;/* settings.num_solver_velocity_iterations, default 8 */
    uint32_t num_position_iterations;/* settings.num_solver_position_iterations, default 3 */
    float gravity[3];                /* settings.gravity, default (0,-9.8,0) */
    uint32_t flags;                  /* EDYNHIP_FLAG_* */
} edynhip_config;

enum {
    EDYNHIP_FLAG_TIMING = 1u,        /* record per-stage HIP events (edynhip_get_timings); each event costs ~6 us of idle GPU */
    EDYNHIP_FLAG_TIMING_SOLVE = 16u, /* record only the two events around the velocity solve (solve_velocity_ms) */
    EDYNHIP_FLAG_SLEEPING = 4u,      /* island sleeping / waking (island_manager.cpp:524-623); off = every body sleeping_disabled */
    EDYNHIP_FLAG_CONTACT_EVENTS = 32u, /* record manifold / contact point creation and destruction (edynhip_get_contact_events) */
    /* Contact arithmetic of the solve. Default (neither flag): every contact row and every contact position correction is evaluated with the
       reference's operations in the reference's order (constraint_row.cpp:24-57, constraint_row_friction.cpp:11-54, contact_constraint.cpp:58-90,
       position_solver.hpp:16-51) - the stepper then differs from the reference in the Gauss-Seidel VISITING order only. The two flags opt in
       to faster forms of the same equations; each is a stated deviation (tests/test_arithmetic_fork.py):
         FUSED_VELOCITY_ROWS  fused multiply-adds, one division per friction-circle clamp (an fp-level change: ~1e-7 m/s per step);
         BLOCK_POSITION       the <= 4 points of a manifold corrected as one block from the transforms the manifold was entered with
                              (an algorithmic change: up to ~3e-4 m per step; SURVEY 8(d)(3) is NOT met in this mode). */
    EDYNHIP_FLAG_FUSED_VELOCITY_ROWS = 64u,
    EDYNHIP_FLAG_BLOCK_POSITION = 128u,
    EDYNHIP_FLAG_FULL_CONTACT_ROWS = 256u, /* A/B and test aid: a contact-only world's dataflow velocity solve reads full contact rows (the stored
                                        I^-1 J_ang planes) instead of rebuilding them from lean rows (edynhip_stats::lean_rows). Same bits either way. */
    EDYNHIP_FLAG_EXCLUSIVE_DEVICE = 8u /* promise: nothing else launches work on this device while a step runs (one stepper per
                                        GPU). The resident-grid solver kernels are then launched plainly instead of
                                        cooperatively (~0.1 ms per step less idle GPU). Without the promise the default,
                                        cooperative launches, is always safe. */
};

/* Scene description, one entry per body, index = body id. Arrays are packed row-major
 * (pos[n][3], orn[n][4] xyzw, ...), i.e. the memory layout of the corresponding EnTT pools. */
typedef struct {
    const int32_t *kind;             /* EDYNHIP_KIND_* */
    const float *pos;                /* [n][3] */
    const float *orn;                /* [n][4] */
    const float *linvel;             /* [n][3] */
    const float *angvel;             /* [n][3] */
    const float *mass;               /* [n]   (dynamic only) */
    const float *inertia;            /* [n][9] local inertia tensor, used where has_inertia[i] != 0; may be NULL */
    const uint8_t *has_inertia;      /* [n] or NULL: 0 = derive from mass and shape (moment_of_inertia.cpp) */
    const int32_t *shape_type;       /* EDYNHIP_SHAPE_* */
    const float *shape_param;        /* [n][4]: box half_extents xyz | sphere radius | plane normal xyz + constant */
    const float *friction;           /* [n] material.friction */
    const float *restitution;        /* [n] material.restitution; any value > 0 turns the restitution solver on
                                        (src/edyn/dynamics/restitution_solver.cpp:86-408) */
    const uint64_t *group;           /* [n] collision_filter.group (all ones = default) */
    const uint64_t *mask;            /* [n] collision_filter.mask */
    const float *gravity;            /* [n][3] per-body gravity or NULL = config gravity */
    const uint8_t *sleeping_disabled;/* [n] or NULL: sleeping_disabled_tag (only meaningful with EDYNHIP_FLAG_SLEEPING) */
    const float *center_of_mass;     /* [n][3] or NULL (ABI 8): rigidbody_def::center_of_mass in the shape's frame; `pos` is then the ORIGIN - the
                                        stepper moves position / linear velocity to the centre of mass and shifts a shape-derived inertia
                                        (util/rigidbody.cpp:56-87,517-548); edynhip_get_state returns the centre of mass, as the reference's position */
} edynhip_bodies;

typedef struct {
    const int32_t *type;             /* EDYNHIP_JOINT_* */
    const uint32_t *body;            /* [n][2] */
    const float *pivot;              /* [n][2][3] object-space pivots */
    const float *axis;               /* [n][2][3] hinge axes in object space (ignored for point joints) */
    const float *params;             /* [n][10] or NULL (all zero). hinge_constraint (hinge_constraint.hpp:30-62): angle_min, angle_max,
                                        limit_restitution, bump_stop_angle, bump_stop_stiffness, torque, speed, rest_angle, stiffness,
                                        damping - limits are active when angle_min < angle_max, the spring when stiffness > 0, the
                                        torque row when torque > 0 or damping > 0. point_constraint (point_constraint.hpp:25):
                                        [0] = friction_torque. */
} edynhip_joints;

/* settings that may change on a running world (include/edyn/context/settings.hpp:22-30) */
typedef struct {
    float fixed_dt;
    uint32_t num_velocity_iterations;
    uint32_t num_position_iterations;
    float gravity[3];
    uint32_t num_restitution_iterations;             /* default 8; 0 turns the restitution solver off */
    uint32_t num_individual_restitution_iterations;  /* default 3 */
} edynhip_params;

/* One contact point; mirrors contact_point + contact_point_geometry + _material + _impulse. */
typedef struct {
    float pivotA[3], pivotB[3], normal[3], local_normal[3];
    float distance, friction, restitution;
    int32_t attachment;
    uint32_t lifetime;
    float normal_impulse, friction_impulse[2];
} edynhip_point;

/* One contact manifold (body pair) with its <= 4 points in the reference's list order (newest first). */
typedef struct {
    uint32_t body[2];
    uint32_t num_points;
    uint32_t colour;                 /* solver colour of this pair (0xFF = none) */
    edynhip_point pt[4];
} edynhip_manifold;

/* Stage selector for edynhip_run_stages: the reference's stage names (profile.hpp:8-18). */
enum {
    EDYNHIP_STAGE_BROADPHASE = 1u,
    EDYNHIP_STAGE_NARROWPHASE = 2u,
    EDYNHIP_STAGE_ISLANDS = 4u,
    EDYNHIP_STAGE_SOLVE = 8u,
    EDYNHIP_STAGE_ALL = 15u
};

typedef struct {
    /* milliseconds, accumulated over the steps of the last edynhip_step call (EDYNHIP_FLAG_TIMING) */
    float broadphase_ms, narrowphase_ms, islands_ms, colouring_ms, prepare_ms, solve_velocity_ms,
          integrate_ms, solve_position_ms, finish_ms, step_ms;
    uint32_t solve_velocity_launches;  /* kernel launches inside solve_velocity_ms */
    uint32_t steps;
} edynhip_timings;

typedef struct {
    uint32_t num_bodies, num_manifolds, num_points, num_active_manifolds, num_islands, num_colours,
             num_joint_colours, colour_rounds, num_joints, num_joint_rows;   /* colour_rounds: rounds the last step's contact colouring took (the one-workgroup rounds + the multi-block ones) */
    uint32_t solve_schedule;         /* EDYNHIP_SCHEDULE_*: which velocity-solve kernels the last step launched */
    uint32_t colour_size[64];        /* manifolds per solver colour in the last step */
    uint32_t lean_rows;              /* 1: the last step's velocity solve ran on lean contact rows */
} edynhip_stats;

/* Velocity-solve schedules (edynhip_stats::solve_schedule). The results are bit-identical across them. */
enum {
    EDYNHIP_SCHEDULE_NONE = 0,          /* nothing to solve */
    EDYNHIP_SCHEDULE_DATAFLOW2 = 1,     /* k_contact_solve_df2: one launch per step, two lanes per manifold */
    EDYNHIP_SCHEDULE_DATAFLOW1 = 2,     /* k_contact_solve_df: one launch per step, one lane per manifold */
    EDYNHIP_SCHEDULE_ISLAND_FUSED = 3,  /* k_island_velocity: one wave per island (scenes with joints / contact_extras rows) */
    EDYNHIP_SCHEDULE_MIXED = 4,         /* dataflow launch for the islands without joints + k_island_velocity for the others */
    EDYNHIP_SCHEDULE_PER_COLOUR = 5,    /* k_contact_solve / k_joint_solve: one launch per colour and sweep */
    EDYNHIP_SCHEDULE_DATAFLOW4 = 6      /* k_contact_solve_df4: one launch per step, four lanes per manifold */
};

edynhip_ctx *edynhip_create(const edynhip_config *cfg, int *status_out);
void edynhip_destroy(edynhip_ctx *ctx);
const char *edynhip_last_error(const edynhip_ctx *ctx);   /* ctx may be NULL: error of the last failed create */

/* Optional: run on a caller-owned hipStream_t (e.g. torch's current stream). NULL = the ctx's own stream. */
int edynhip_set_stream(edynhip_ctx *ctx, void *hip_stream);

int edynhip_set_bodies(edynhip_ctx *ctx, uint32_t n, const edynhip_bodies *bodies);
int edynhip_set_joints(edynhip_ctx *ctx, uint32_t n, const edynhip_joints *joints);
/* Append `n` bodies after the existing ones (indices num_bodies .. num_bodies+n-1). Existing bodies, their contact
 * manifolds (cached impulses, colours) and joints are untouched: this is registry.create + make_rigidbody on a running
 * world (src/edyn/util/rigidbody.cpp:18-161; the reference's island worker receives the new entities through
 * registry_operation insertions, src/edyn/simulation/simulation_worker.cpp). To remove bodies: edynhip_remove_bodies, which keeps
 * every other index by leaving a tombstone. */
int edynhip_add_bodies(edynhip_ctx *ctx, uint32_t n, const edynhip_bodies *bodies);

/* Joints on a running world: make_constraint / registry.destroy(constraint entity) (include/edyn/util/constraint_util.hpp:38-54,
 * island_manager.cpp:68-97). Joint indices are the order of creation and stay valid for the life of the world (a removed joint
 * keeps its index); applied impulses and hinge angles of the other joints are carried over. *first_index = index of the first
 * joint added. edynhip_set_joint_params = registry.patch<hinge|point_constraint> followed by reset_angle.
 * Island sleeping: a new joint wakes the islands of its two bodies (insert_to_island, island_manager.cpp:282-294), a removed joint
 * the islands it touched (on_destroy_island_resident, :74-97). Such a wake takes the sleeping tags off and nothing else
 * (wake_up_island, util/island_util.cpp:61-66): the sleep timer of an island that was awake goes on running, and only an island that
 * the removal really splits starts its timers again. In the step's merge rule a joint counts towards an island's size from the step
 * after the one that first saw it (merge_islands sizes the islands before it inserts the new edges). */
int edynhip_add_joints(edynhip_ctx *ctx, uint32_t n, const edynhip_joints *joints, uint32_t *first_index);
int edynhip_remove_joints(edynhip_ctx *ctx, uint32_t n, const uint32_t *joint_indices);
int edynhip_set_joint_params(edynhip_ctx *ctx, uint32_t joint_index, const float *params10);
/* registry.destroy(rigid body) on a running world (src/edyn/edyn.cpp:148-197 hooks, island_manager.cpp:47-115): the body's
 * manifolds and contact points disappear with the next step, joints attached to it are removed, the islands it touched wake
 * up. The body INDEX stays reserved (the slot reads back as a shapeless static body); every other index, manifold, warm-start
 * impulse and sleep timer is untouched. The wake only takes the sleeping tags off: what is left of the body's own island keeps the
 * island's sleep timer if it is still in one piece - also when the removed body had the island's lowest index, i.e. was its label:
 * label and timer move to the lowest body left - and starts again if the removal split it. */
int edynhip_remove_bodies(edynhip_ctx *ctx, uint32_t n, const uint32_t *body_indices);
/* Bodies of a running world edited in place: set_rigidbody_mass / _inertia / _friction, rigidbody_set_shape, rigidbody_set_kind
 * (src/edyn/util/rigidbody.cpp:300-362, :471-495, :579-606) without a fresh upload. values holds n entries parallel to indices; only the
 * arrays of the groups named in `fields` are read. Each group changes what the reference call changes and nothing derived across groups:
 *   MASS      mass: the inverse mass (:300-305).
 *   INERTIA   inertia, has_inertia: the local inverse inertia as edynhip_set_bodies computes it, and the world inverse inertia from the
 *             body's current orientation (:307-312). has_inertia[i] == 0 (or a NULL has_inertia): derived from the body's shape, the
 *             mass given in this call and its centre-of-mass offset, as edynhip_set_bodies does - MASS must then be named too.
 *             (Inverse mass and inertias are kept on the device for dynamic bodies only: on a body that is not dynamic after the call
 *             both groups change nothing.)
 *   MATERIAL  friction, restitution: the body's material. Every living contact point of the body's manifolds takes the friction a
 *             point created now would get, except in a pair the mix table combines - those keep theirs (:314-362). Restitution
 *             reaches new points only; a value above 0 turns the restitution solver on, as in edynhip_set_bodies.
 *   SHAPE     shape_type (box .. polyhedron), shape_param: shape, flags and the AABB from the current pose; mass and inertia are left
 *             alone; every manifold of the body is dropped (:471-495). A polyhedron gets a slice of the rotated-mesh buffer of its own;
 *             a slice the body held before stays unused until the context is destroyed.
 *   KIND      kind, gravity (NULL = the context's): to static or kinematic, inverse mass, inertias and gravity become 0, to static the
 *             velocities too; to dynamic, MASS and INERTIA must be named in the same call. Every manifold of the body is dropped - the
 *             reference keeps those against procedural partners (:591-605); see INTEGRATION.md section 3.
 * A dropped manifold leaves the manifold array as if its pair had left the pair set: with EDYNHIP_FLAG_CONTACT_EVENTS a POINT_DESTROYED
 * event per living point and a MANIFOLD_DESTROYED event are appended to the event list of the last step call; if the pair still overlaps
 * the next step creates it anew. SHAPE and KIND wake the islands of the edited bodies, of every body that shared a dropped manifold with
 * them and of every body that shares a joint with them, as edynhip_remove_bodies does; MASS, INERTIA and MATERIAL wake nobody and keep
 * the candidate lists, the island labels and the solve schedule.
 * Everything is checked before anything changes: EDYNHIP_ERR_INVALID for an index out of range, of a removed body or listed twice, for a
 * polyhedron whose shape_param[0] is not a mesh id, for a missing array; EDYNHIP_ERR_UNSUPPORTED for a shape type outside box ..
 * polyhedron and for a shard of a multi-device world. n == 0 is valid. */
enum { EDYNHIP_EDIT_MASS = 1, EDYNHIP_EDIT_INERTIA = 2, EDYNHIP_EDIT_MATERIAL = 4, EDYNHIP_EDIT_SHAPE = 8, EDYNHIP_EDIT_KIND = 16 };
int edynhip_edit_bodies(edynhip_ctx *ctx, uint32_t n, const uint32_t *indices, const edynhip_bodies *values, uint32_t fields);
/* settings on a running world WITHOUT losing state: set_fixed_dt, set_solver_velocity/position_iterations, set_gravity
 * (src/edyn/edyn.cpp:203-207, src/edyn/config/solver_iteration_config.cpp:9-75, src/edyn/util/gravity_util.cpp:12-20 - like the
 * reference, set_gravity also replaces the gravity of every dynamic body). */
int edynhip_get_params(edynhip_ctx *ctx, edynhip_params *out);
int edynhip_set_params(edynhip_ctx *ctx, const edynhip_params *params);

/* Advance `nsteps` fixed-dt steps. Returns after the work is enqueued and error flags were checked. */
int edynhip_step(edynhip_ctx *ctx, uint32_t nsteps);
/* The same with explicit step time stamps: step i runs at first_step_time + i * step_dt. The stamps only feed the island
 * sleep timers; integration always uses fixed_dt. This is stepper_sequential::update's behaviour when more steps are due
 * than max_steps_per_update allows: the steps that do run get stretched stamps (stepper_sequential.cpp:60-75). */
int edynhip_step_timed(edynhip_ctx *ctx, uint32_t nsteps, double first_step_time, double step_dt);
/* Run a subset of one step's stages (parity tests). */
int edynhip_run_stages(edynhip_ctx *ctx, uint32_t stage_mask);
/* Block until all enqueued work of this ctx has finished. */
int edynhip_synchronize(edynhip_ctx *ctx);

int edynhip_get_state(edynhip_ctx *ctx, float *pos, float *orn, float *linvel, float *angvel);
int edynhip_set_state(edynhip_ctx *ctx, const float *pos, const float *orn, const float *linvel, const float *angvel);
/* collision_exclusion lists (include/edyn/util/exclude_collision.hpp:20-47, src/edyn/util/exclude_collision.cpp:9-71;
 * evaluated by should_collide_default, src/edyn/collision/should_collide.cpp:11-57): no NEW manifold is created for an
 * excluded pair (symmetric; at most 16 partners per body, EDYNHIP_ERR_CAPACITY beyond). A manifold that already exists
 * lives on until its AABBs separate, as in the reference. */
int edynhip_exclude_collision(edynhip_ctx *ctx, uint32_t body_a, uint32_t body_b);
int edynhip_remove_collision_exclusion(edynhip_ctx *ctx, uint32_t body_a, uint32_t body_b);
/* settings.should_collide_func / edyn::set_should_collide (include/edyn/collision/should_collide.hpp:8-18, include/edyn/context/settings.hpp:43):
 * the user's predicate that REPLACES should_collide_default - the reference calls it for every candidate of a body's tree query
 * (src/edyn/collision/broadphase.cpp:143-153) and creates a manifold only when it says yes. A host callback cannot run inside the
 * device broadphase, so a context with a filter takes a slow path in every step that has candidates for NEW manifolds: the device
 * broadphase runs WITHOUT its group / mask / exclusion test, the new candidate pairs (AABBs already found overlapping, no manifold yet)
 * travel to the host, `filter(user, body, other)` is asked once per pair - body = the querying (procedural) body, body[0] of the
 * manifold that would be made - the rejected pairs are taken out of the step's pair list, and the step goes on. A rejected pair is
 * asked about again in every step in which it is still a candidate, an existing manifold lives on until its AABBs separate - both as
 * in the reference. The predicate must be a function of the pair (the reference asks more often - also for pairs that have a
 * manifold or whose boxes then do not overlap - and in another order). edynhip_default_should_collide evaluates what the device would
 * have (collision groups / masks, exclusion lists) for callbacks that extend the default. filter = NULL restores the device test.
 * Costs one device-to-host copy and a stream synchronisation per step that has new candidates. Worlds over several devices:
 * edynhip_world_set_pair_filter (global body indices). */
typedef int (*edynhip_pair_filter)(void *user, uint32_t body, uint32_t other);
int edynhip_set_pair_filter(edynhip_ctx *ctx, edynhip_pair_filter filter, void *user);
int edynhip_default_should_collide(edynhip_ctx *ctx, uint32_t body_a, uint32_t body_b);   /* 1 / 0, negative = error */
/* Recompute every awake body's AABB and world-space inverse inertia from its current transform: the reference's public
 * update_aabbs(registry) / update_inertias(registry) (include/edyn/sys/update_aabbs.hpp:18-25, update_inertias.hpp:18-28).
 * A step does this at its end (solver.cpp:456-465); after edynhip_set_state the derived state is stale until then -
 * exactly as in the reference, where the broadphase of the next step still sees the old AABB - unless this is called. */
int edynhip_refresh_derived(edynhip_ctx *ctx);
/* Pack (pos3, orn4, linvel3, angvel3) = 13 floats per body into DEVICE memory `dst` (for RCCL gathers). */
int edynhip_pack_state_device(edynhip_ctx *ctx, void *dst_device, uint32_t first_body, uint32_t count);
/* Derived per-body state: aabb[n][6] (min,max), inertia_world_inv[n][9], island label[n]; any may be NULL. */
int edynhip_get_derived(edynhip_ctx *ctx, float *aabb, float *inertia_world_inv, uint32_t *island);

/* edyn::raycast (include/edyn/collision/raycast.hpp:139-151, src/edyn/collision/raycast.cpp:20-56) for a batch of rays p0 -> p1.
 * Candidates: every body that has a shape, is not removed and is not in `ignore` - sleeping, static and kinematic bodies and planes
 * included - whose current AABB grown by 0.1 (dynamic_tree.hpp:24) the segment crosses (intersect_segment_aabb, geom.cpp:1185-1223).
 * Each candidate is tested with the reference's shape_raycast for its shape (raycast.cpp:58-380) in the frame of its origin (its
 * position when it has no centre-of-mass offset); the hit is the smallest fraction, an exact tie goes to the lowest body index. The
 * reference's quirks are kept: box and plane fractions are not clipped to [0, 1]. A zero-length ray inside a box or polyhedron is
 * undefined in the reference: the record then carries the reference's fraction, a zero normal and feature_index ~0u.
 * The rays see the context's current state (the last step, or edynhip_set_state / edynhip_add_bodies ... since); the query tree is
 * the context's own, rebuilt at the first raycast after a change, and a raycast changes nothing a later step computes. */
enum { EDYNHIP_RAYCAST_FEATURE_NONE = 0,              /* sphere, plane, miss */
       EDYNHIP_RAYCAST_FEATURE_BOX_FACE = 1,          /* box_raycast_info::face_index */
       EDYNHIP_RAYCAST_FEATURE_CYLINDER_FACE = 2,     /* cylinder_raycast_info{cylinder_feature::face, face_index} */
       EDYNHIP_RAYCAST_FEATURE_CYLINDER_SIDE_EDGE = 3,/* cylinder_raycast_info{cylinder_feature::side_edge} */
       EDYNHIP_RAYCAST_FEATURE_CAPSULE_HEMISPHERE = 4,/* capsule_raycast_info{capsule_feature::hemisphere, hemisphere_index} */
       EDYNHIP_RAYCAST_FEATURE_CAPSULE_SIDE = 5,      /* capsule_raycast_info{capsule_feature::side} */
       EDYNHIP_RAYCAST_FEATURE_POLYHEDRON_FACE = 6 }; /* polyhedron_raycast_info::face_index */
/* flags: EDYNHIP_RAYCAST_BRUTE_FORCE (test aid): every ray tests every body with the same candidate predicate, no tree. Other flag
 * bits: EDYNHIP_ERR_INVALID. A shard context of a multi-device world (edynhip_world_context): EDYNHIP_ERR_UNSUPPORTED. */
enum { EDYNHIP_RAYCAST_BRUTE_FORCE = 1 };
typedef struct {
    uint32_t body;           /* ~0u: nothing hit (raycast_result::entity == entt::null) */
    float fraction;          /* FLT_MAX on a miss; the point hit is lerp(p0, p1, fraction) */
    float normal[3];         /* world-space normal */
    int32_t feature;         /* EDYNHIP_RAYCAST_FEATURE_* */
    uint32_t feature_index;  /* face / hemisphere index of the feature, 0 where it has none */
    uint32_t reserved;
} edynhip_raycast_hit;       /* 32 B */
/* Host arrays p0[n][3], p1[n][3], ignore[num_ignore] (body indices); returns when out[n] holds the results. n = 0 is valid. */
int edynhip_raycast(edynhip_ctx *ctx, uint32_t n, const float *p0, const float *p1, uint32_t num_ignore, const uint32_t *ignore,
                    uint32_t flags, edynhip_raycast_hit *out);
/* The same with DEVICE arrays: p0 / p1 hold one float4 per ray (w unused), out n records; enqueued on the context's stream,
 * no host synchronisation (ignore is a host list, copied before the call returns). */
int edynhip_raycast_device(edynhip_ctx *ctx, uint32_t n, const void *p0_f4, const void *p1_f4, uint32_t num_ignore, const uint32_t *ignore,
                           uint32_t flags, void *out);

/* edyn::query_procedural_aabb / query_non_procedural_aabb / query_island_aabb (include/edyn/collision/query_aabb.hpp:10-26,
 * include/edyn/collision/broadphase.hpp:81-100, src/edyn/collision/dynamic_tree.cpp query) for a batch of boxes q = (min, max).
 * Candidates by category:
 *   EDYNHIP_QUERY_PROCEDURAL      every body that has a shape, is not removed and is dynamic (the holders of procedural_tag);
 *   EDYNHIP_QUERY_NON_PROCEDURAL  every shaped, not removed body that is static or kinematic, planes (with their half-space box) included;
 *   EDYNHIP_QUERY_ISLANDS         every island (label = its lowest body index, as edynhip_get_derived returns it) with the union of the
 *                                 boxes of its shaped dynamic bodies.
 * A candidate is reported iff intersect_aabb(q.min, q.max, box.min - 0.1, box.max + 0.1) (include/edyn/comp/aabb.hpp:45-47,
 * src/edyn/math/geom.cpp:762-770: six <= / >= comparisons on closed intervals; 0.1 is dynamic_tree::aabb_inset, dynamic_tree.hpp:24,
 * dynamic_tree.cpp:45) - the box a freshly created leaf of the reference's tree holds. (The reference's fat boxes depend on the history
 * of dynamic_tree::move; on leaves just created the two coincide exactly.) Sleeping bodies are reported; amorphous and removed bodies
 * never are. The six comparisons are evaluated as written and nothing else: a box that only touches is a hit, a NaN in the query reports
 * nothing, and an inverted query (min > max on an axis) is not special - it reports what the formula passes, as the reference's tree does.
 * The one intended difference: the reference reports in tree-visit order, here each query's hits are in ASCENDING body index (island
 * label). The queries see the context's current state (the last step, or edynhip_set_state / edynhip_add_bodies ... since) through the
 * raycast's query tree, rebuilt at the first query after a change; a query changes nothing a later step computes.
 * Result (CSR): offsets[n + 1] (offsets[0] = 0, offsets[n] = *total), ids[offsets[i] .. offsets[i + 1]) the hits of query i. offsets and
 * *total are always complete (saturated at 0xFFFFFFFF). flags: EDYNHIP_QUERY_BRUTE_FORCE (test aid): every query tests every body /
 * island with the same predicate, no tree. Unknown category or flag bits: EDYNHIP_ERR_INVALID. A shard context of a multi-device world
 * (edynhip_world_context): EDYNHIP_ERR_UNSUPPORTED. n = 0 is valid. */
enum { EDYNHIP_QUERY_PROCEDURAL = 0, EDYNHIP_QUERY_NON_PROCEDURAL = 1, EDYNHIP_QUERY_ISLANDS = 2 };
enum { EDYNHIP_QUERY_BRUTE_FORCE = 1 };
/* Host arrays: boxes6[n][6] (min, max); offsets[n + 1]; ids[capacity], may be NULL (count only). *total > capacity: returns
 * EDYNHIP_ERR_CAPACITY with offsets / *total valid and ids unspecified (size ids by *total and ask again). */
int edynhip_query_aabb(edynhip_ctx *ctx, int category, uint32_t n, const float *boxes6, uint32_t flags,
                       uint32_t *offsets, uint32_t *ids, uint32_t capacity, uint32_t *total);
/* The same with DEVICE arrays: boxes as 2 float4 per query (min, max; w unused), offsets n + 1 uint32, ids capacity uint32 (may be NULL),
 * total 1 uint32; enqueued on the context's stream, no host synchronisation. No id is written at or beyond `capacity`: when
 * *total > capacity the ids of the queries that did not fit are incomplete, offsets and *total are still right. */
int edynhip_query_aabb_device(edynhip_ctx *ctx, int category, uint32_t n, const void *boxes_f4, uint32_t flags,
                              void *offsets, void *ids, uint32_t capacity, void *total);
/* Statistics since the context was created, counted by the fill kernels: segments one wave sorted in LDS, and queries whose hits one
 * wave packed from the body range (the second fill path of large results); every other query was filled and sorted by its own lane.
 * Calls that only count (ids = NULL, or EDYNHIP_ERR_CAPACITY) add nothing. Either pointer may be NULL.
 * Debug knob: the environment variable EDYNHIP_QUERY_SCAN_RATIO = r (read when the context is created) moves the switch to
 * the second fill path to "more than num_bodies / r hits" (default 64). It changes the cost only, never a result; it exists for
 * scripts/bench_query_aabb.py --ratios and for tests that steer queries onto one path. */
int edynhip_query_aabb_stats(edynhip_ctx *ctx, uint64_t *wave_sorted, uint64_t *wave_filled);

/* Queries as TICKETS (additive to ABI 15): what edyn::raycast_async (include/edyn/collision/raycast.hpp:170-182), edyn::query_aabb_async
 * and edyn::query_aabb_of_interest_async (include/edyn/collision/query_aabb.hpp:37-44) need - the reference's worker answers them between
 * steps (src/edyn/simulation/simulation_worker.cpp:600-692) and the caller picks the answer up later. A submit enqueues the query on the
 * context's stream and returns a ticket without waiting for the device: the ticket answers from the state after everything enqueued on
 * the context before the submit (steps, edynhip_set_state, edits) and nothing enqueued after it. The inputs are copied before submit
 * returns. edynhip_query_poll never waits; a collect waits until the ticket is done. Results live in pinned memory the context owns,
 * valid until edynhip_query_release (or edynhip_destroy, which frees outstanding tickets). At most EDYNHIP_QUERY_TICKETS_MAX tickets are
 * outstanding: one more submit returns EDYNHIP_ERR_CAPACITY and disturbs none of them. Ticket values are never reused; a released or
 * unknown ticket, or one of the other kind, is EDYNHIP_ERR_INVALID. Tickets may be collected in any order, more than once, and share no
 * buffer with the synchronous entry points, which may be called between submit and collect. A shard context of a multi-device world:
 * EDYNHIP_ERR_UNSUPPORTED. */
enum { EDYNHIP_QUERY_TICKETS_MAX = 8 };
enum { EDYNHIP_WANT_PROCEDURAL = 1, EDYNHIP_WANT_NON_PROCEDURAL = 2, EDYNHIP_WANT_ISLANDS = 4, EDYNHIP_WANT_OF_INTEREST = 8 };
/* edyn::raycast_async (raycast.hpp:170-182; the worker: simulation_worker.cpp:600-624): n rays p0[n][3] -> p1[n][3], each with an ignore
 * list of its own: ray i ignores ignore_ids[ignore_offsets[i] .. ignore_offsets[i + 1]) (NULL offsets: no list). Ray i gets the record
 * edynhip_raycast(ctx, 1, p0_i, p1_i, its list, flags) would return: indices beyond the body count are skipped, duplicates are allowed.
 * flags as edynhip_raycast. Offsets that descend, or unknown flag bits: EDYNHIP_ERR_INVALID. */
int edynhip_raycast_submit(edynhip_ctx *ctx, uint32_t n, const float *p0, const float *p1,
                           const uint32_t *ignore_offsets, const uint32_t *ignore_ids, uint32_t flags, uint64_t *ticket);
/* edyn::query_aabb_async / query_aabb_of_interest_async (query_aabb.hpp:37-44; the worker: simulation_worker.cpp:626-692): n boxes
 * boxes6[n][6] = (min, max), want[n] = EDYNHIP_WANT_* bits per box. Box i has four lists, 4 i + k: k = 0 procedural, 1 non-procedural,
 * 2 islands - each what edynhip_query_aabb returns for the box in that category - and 3 "of interest": every dynamic body that has a
 * shape and is not removed whose island (the label edynhip_get_derived returns) is one the islands category reports for the box, in
 * ascending body index (the entities the worker collects from the islands it finds, simulation_worker.cpp:652-660). A list that was
 * not wanted is empty. ids_capacity: the ids the ticket may hold. flags as edynhip_query_aabb. Unknown want or flag bits:
 * EDYNHIP_ERR_INVALID. */
int edynhip_query_aabb_submit(edynhip_ctx *ctx, uint32_t n, const float *boxes6, const uint8_t *want,
                              uint32_t ids_capacity, uint32_t flags, uint64_t *ticket);
/* *done = 1 once the ticket's results are in place (the worker's reply has arrived, simulation_worker.cpp:600-692). Never waits. */
int edynhip_query_poll(edynhip_ctx *ctx, uint64_t ticket, int *done);
/* The records of a raycast ticket (raycast.hpp:170-182: what the delegate receives), (*hits)[*n]; waits until they are there. */
int edynhip_raycast_collect(edynhip_ctx *ctx, uint64_t ticket, const edynhip_raycast_hit **hits, uint32_t *n);
typedef struct {
    uint32_t n;               /* boxes of the ticket */
    const uint32_t *offsets;  /* [4 n + 1]: list 4 i + k is ids[offsets[4 i + k] .. offsets[4 i + k + 1]); saturated at 0xFFFFFFFF */
    const uint32_t *ids;      /* NULL when total > the ticket's ids_capacity */
    uint64_t total;           /* ids of all lists together */
} edynhip_query_aabb_view;
/* The lists of a box ticket (query_aabb.hpp:37-44: what the delegate receives); waits until they are there. total > ids_capacity:
 * returns EDYNHIP_ERR_CAPACITY with offsets and total valid and ids = NULL (submit again with ids_capacity = total): no list is ever
 * cut short. */
int edynhip_query_aabb_collect(edynhip_ctx *ctx, uint64_t ticket, edynhip_query_aabb_view *view);
/* Gives the ticket's slot back (done or not: the slot's buffers are reused only by work enqueued later on the same stream); the
 * pointers a collect returned for it are no longer valid (simulation_worker.cpp:600-692: the request is answered once). */
int edynhip_query_release(edynhip_ctx *ctx, uint64_t ticket);

/* Manifolds are kept (and returned) in ascending canonical order: key = (owner << 32) | other, where the owner is the
 * pair's procedural (dynamic) body - the one with the higher index when both are dynamic. edynhip_set_manifolds expects
 * records in that order. (EnTT's pool order is not reproducible; the solver visits manifolds in this order.) */
int edynhip_num_manifolds(edynhip_ctx *ctx, uint32_t *n);
int edynhip_get_manifolds(edynhip_ctx *ctx, edynhip_manifold *out, uint32_t capacity, uint32_t *n);
int edynhip_set_manifolds(edynhip_ctx *ctx, const edynhip_manifold *in, uint32_t n);
/* Canonical broadphase pairs: keys[i] = (max(body)<<32 | min(body)), ascending. */
int edynhip_get_pairs(edynhip_ctx *ctx, uint64_t *keys, uint32_t capacity, uint32_t *n);
/* Per joint (by caller index, removed joints read 0) 10 floats: the applied impulses by slot - hinge: linear[3], hinge[2], limit,
 * bump_stop, spring, torque; point: applied[3], friction - and the tracked hinge angle (hinge_constraint.hpp:62-71). */
int edynhip_get_joint_impulses(edynhip_ctx *ctx, float *impulses10);

/* Frames (row-major 3x3, first COLUMN = the cone direction / the twist axis) and the parameter block of a cone or cvjoint
 * constraint (created with identity frames by edynhip_set_joints / add_joints); resets the cvjoint's twist angle.
 *   cone   : span_tan[0], span_tan[1], restitution, bump_stop_stiffness, bump_stop_length (cone_constraint.hpp:19-49);
 *            impulse slots: 0 limit, 1 bump stop. frame_b is ignored.
 *   cvjoint: twist_min, twist_max, twist_restitution, twist_bump_stop_angle, twist_bump_stop_stiffness, twist_friction_torque,
 *            twist_rest_angle, twist_stiffness, twist_damping, rest_direction[3], bend_stiffness, bend_friction_torque,
 *            bend_damping (cvjoint_constraint.hpp:20-102); impulse slots: 0..2 linear, 3 twist limit, 4 twist bump stop,
 *            5 twist spring, 6 twist friction / damping, 7 bend friction / damping, 8 bend spring; [9] of
 *            edynhip_get_joint_impulses = the tracked twist angle. */
int edynhip_set_joint_definition(edynhip_ctx *ctx, uint32_t joint, const float *frame_a9, const float *frame_b9, const float *params16);

/* generic_constraint: frames (row-major 3x3) and, per degree of freedom d (0..2 translation along frame_a's columns, 3..5 rotation:
 * twist about x, then the two bending angles), 10 floats dof[10 d + ..]: limit_enabled, min, max, limit_restitution,
 * bump_stop_length (angle), bump_stop_stiffness, friction force (torque), rest offset (angle), spring_stiffness, damping
 * (generic_constraint.hpp:23-70). Created by edynhip_set_joints / add_joints with identity frames and every degree of freedom
 * free. edynhip_get_joint_slot_impulses: out[n][24], slot 4 d + {0 limit, 1 bump stop, 2 spring, 3 friction / damping} for
 * generic constraints, the first 9 slots as documented above for the other types. */
int edynhip_set_generic_definition(edynhip_ctx *ctx, uint32_t joint, const float *frame_a9, const float *frame_b9, const float *dof60);
int edynhip_get_joint_slot_impulses(edynhip_ctx *ctx, float *impulses24);

/* contact_extras materials: material::{spin_friction, roll_friction, stiffness, damping} of bodies [first, first + n)
 * (comp/material.hpp:15-22; any array may be NULL = the default 0, 0, large_scalar, large_scalar). Contact points created
 * from then on mix them (material_mixing.hpp:20-34) and, where a mixed value is not the default, get the rolling-friction
 * pair, the spinning-friction row and / or the force-limited ("soft") normal row of contact_extras_constraint
 * (contact_extras_constraint.cpp:12-110, constraint_row_spin_friction.cpp:5-36); soft contacts take no position
 * correction. A world with such materials solves on the per-colour schedule. material::roll_direction is modelled: the tangent axes of
 * the rolling pair of a dynamic capsule or cylinder are scaled by the projection of its axis (contact_extras_constraint.cpp:44-55).
 * edynhip_get_point_extras: out[4 * i + k][7] = rolling impulse[2], spin impulse, mixed roll / spin coefficient, stiffness,
 * damping of point k of manifold i in edynhip_get_manifolds order. */
int edynhip_set_material_extras(edynhip_ctx *ctx, uint32_t first, uint32_t n, const float *spin_friction, const float *roll_friction,
                                const float *stiffness, const float *damping);
int edynhip_get_point_extras(edynhip_ctx *ctx, float *out7, uint32_t capacity_manifolds, uint32_t *n);

/* Material ids and the material mix table (material::id, comp/material.hpp:27-31; material_mix_table, dynamics/material_mixing.hpp:36-82;
 * edyn::insert_material_mixing, util/insert_material_mixing.hpp:17): an entry for a pair of ids replaces every mixing rule for
 * contact points created from then on - material6 = restitution, friction, spin_friction, roll_friction, stiffness, damping.
 * ids: 16 bits, 0xFFFF = unassigned. Faithful to the reference down to its lookup: the table is keyed by the ids of
 * (manifold body[0], body[1]) in a std::map under unordered_pair's comparator, so an entry inserted as (a, b) is not always found
 * for a pair that meets as (b, a) - insert both orders if in doubt (core/unordered_pair.hpp:32-40). */
int edynhip_set_material_ids(edynhip_ctx *ctx, uint32_t first, uint32_t n, const uint32_t *ids);
int edynhip_insert_material_mixing(edynhip_ctx *ctx, uint32_t id0, uint32_t id1, const float *material6);

/* Contact events (EDYNHIP_FLAG_CONTACT_EVENTS): what an application observes in the reference through
 * registry.on_construct / on_destroy<contact_manifold> (make_contact_manifold, constraint_util.cpp:60-102;
 * broadphase::destroy_separated_manifolds, broadphase.cpp:99-134) and <contact_point> (create_contact_point,
 * collision_util.cpp:311-388; destroy_contact_point, :390-430; contact_started_tag, narrowphase.cpp:111-130).
 * The events of all steps of the last edynhip_step / edynhip_step_timed call, in no particular order within a step.
 * A point keeps its id from creation to destruction: id = (step of creation + 1) << 32 | manifold index << 2 | slot
 * (points injected with edynhip_set_manifolds: high word 0). If more events occurred than the context can hold
 * (5 x max_manifolds), `n` is capped and EDYNHIP_ERR_CAPACITY is returned: resynchronise from edynhip_get_manifolds. */
enum { EDYNHIP_EVENT_MANIFOLD_CREATED = 1, EDYNHIP_EVENT_MANIFOLD_DESTROYED = 2, EDYNHIP_EVENT_POINT_CREATED = 3, EDYNHIP_EVENT_POINT_DESTROYED = 4 };
typedef struct {
    uint32_t type;       /* EDYNHIP_EVENT_* */
    uint32_t step;       /* step index (steps since edynhip_create / edynhip_set_bodies) in which it happened */
    uint32_t body[2];    /* the manifold's bodies, as in edynhip_manifold.body */
    uint64_t point_id;   /* point events; 0 for manifold events */
} edynhip_contact_event;
int edynhip_get_contact_events(edynhip_ctx *ctx, edynhip_contact_event *out, uint32_t capacity, uint32_t *n);
/* ids[4 * i + k] = id of point k of manifold i in edynhip_get_manifolds order (0 where there is no point). */
int edynhip_get_point_ids(edynhip_ctx *ctx, uint64_t *ids, uint32_t capacity_manifolds, uint32_t *n);

/* Double-buffered state read-back - the analogue of the asynchronous stepper handing finished steps to the main thread
 * (simulation_worker.cpp:406-444): edynhip_snapshot enqueues, behind the steps issued so far, a copy of the packed state
 * (13 floats / body) into one of two pinned host buffers and returns at once; edynhip_snapshot_read waits for THAT copy
 * only (not for steps enqueued after it) and unpacks it. step -> snapshot -> step -> snapshot_read hands the host the
 * first step's result while the second one runs. `step_index` (may be NULL) = steps completed when the snapshot was taken. */
int edynhip_snapshot(edynhip_ctx *ctx);
int edynhip_snapshot_read(edynhip_ctx *ctx, float *pos, float *orn, float *linvel, float *angvel, uint32_t *step_index);

/* The registry write-back, read in place (ABI 15). The reference has no write-back - the registry IS its storage
 * (stepper_sequential.cpp:28-119) - so what a registry-facing caller pays per update beyond the step is this copy. One packed
 * 96-byte record per body, written by the device into pinned host memory the context owns (two slots, alternating): no
 * per-call staging arrays, no second scatter, and everything a per-body host loop would otherwise compute or fetch separately:
 *   pos orn linvel angvel   the simulated state (what solver::update leaves in the components, solver.cpp:331-339)
 *   present_pos/orn         update_presentation.cpp:56-84 evaluated at `present_dt` from that state: pos + linvel * dt and
 *                           integrate(orn, angvel, dt) (math/quaternion.cpp:7-22) with the stepper's own integrate()
 *   origin                  update_origins.cpp:13-15 (meaningful when EDYNHIP_RECORD_HAS_ORIGIN is set)
 *   flags                   EDYNHIP_RECORD_*: dynamic body / sleeping_tag (island_manager.cpp:541-565) / has a centre-of-mass offset / removed
 * and the contact events of the last step call (edynhip_get_contact_events' list), the first `max_events` of them.
 * edynhip_snapshot_records enqueues, behind the steps issued so far, the pack and the copy (on a side stream) and returns at once;
 * edynhip_snapshot_map waits for THAT copy only and hands out pointers into the pinned slot, valid until the next-but-one
 * edynhip_snapshot_records call. step -> snapshot_records -> step -> snapshot_map hands over the first step's result while the
 * second one runs (simulation_worker.cpp:406-444). `total_events` > `num_events`: the list was cut - in a synchronous caller
 * edynhip_get_contact_events still returns all of them (until the next step call), otherwise resynchronise from the manifolds. */
enum { EDYNHIP_RECORD_DYNAMIC = 1u, EDYNHIP_RECORD_ASLEEP = 2u, EDYNHIP_RECORD_HAS_ORIGIN = 4u, EDYNHIP_RECORD_REMOVED = 8u };
typedef struct {
    float pos[3], orn[4], linvel[3], angvel[3];
    float present_pos[3], present_orn[4];
    float origin[3];
    uint32_t flags;
} edynhip_body_record;
typedef struct {
    const edynhip_body_record *records;    /* [num_bodies], index = body id */
    uint32_t num_bodies;
    uint32_t step_index;                   /* steps completed when the snapshot was taken */
    const edynhip_contact_event *events;   /* [num_events]; NULL when the context records no events */
    uint32_t num_events, total_events;
} edynhip_record_view;
/* flags: EDYNHIP_SNAPSHOT_DIRECT - the caller is going to wait for THIS snapshot right away (a synchronous write-back): the pack kernels store
 * straight into the pinned slot on the stepper's stream instead of handing a device buffer to the copy engine on the side stream (no
 * second stream, no event between the two: ~0.04 ms sooner on the headline pile); without it the copy overlaps whatever is enqueued next. */
enum { EDYNHIP_SNAPSHOT_DIRECT = 1u };
int edynhip_snapshot_records(edynhip_ctx *ctx, float present_dt, uint32_t max_events, uint32_t flags);
int edynhip_snapshot_map(edynhip_ctx *ctx, edynhip_record_view *view);
/* Contact-event prefetch (ABI 15). In the reference contact points become registry entities INSIDE the step, during the narrowphase
 * (create_contact_point collision_util.cpp:311-388, destroy_contact_point :390-430, narrowphase.cpp:21-40) - before the solver moves
 * anything. Every event of a step is emitted by its broadphase and narrowphase, so with the prefetch enabled (max_events > 0) a step
 * call copies its event list (the count and the first max_events events) to pinned memory as soon as the LAST step's narrowphase has
 * run, on a side stream; edynhip_prefetched_events waits for that copy only, so the caller creates / destroys the contact entities
 * while the islands, solve and finish stages of that step are still running. `total_events` > `num_events`: the list was cut -
 * edynhip_get_contact_events returns all of it (and waits for the step). The pointers stay valid until the next step call. */
int edynhip_set_event_prefetch(edynhip_ctx *ctx, uint32_t max_events);
int edynhip_prefetched_events(edynhip_ctx *ctx, const edynhip_contact_event **events, uint32_t *num_events, uint32_t *total_events);

/* Test hook: run the device closest-feature routine on `n` independent shape pairs (no world state involved).
 * shape_type[n][2], shape_param[n][2][4], pos[n][2][3], orn[n][2][4]; out_points[n][4][11] =
 * (pivotA3, pivotB3, normal3, distance, attachment) per point, out_count[n]. Replaces nothing in the reference: it
 * exposes edyn::collide(shA, shB, ctx, result) (include/edyn/collision/collide.hpp) for parity tests. */
int edynhip_debug_collide(edynhip_ctx *ctx, uint32_t n, const int32_t *shape_type, const float *shape_param, const float *pos,
                          const float *orn, float threshold, float *out_points, uint32_t *out_count);

/* Test hook (additive to ABI 15): which of the library's alternative code paths this context has taken. *mask = the OR, since the context
 * was created, of one bit per HOST-side branch actually taken - set at the branch itself, once the launch it selects was accepted - so a parity
 * test that switches a path on through a development knob (scripts/README.md) or through the scene's size can show that the path ran.
 * No kernel reads or writes it. Replaces nothing in the reference. */
#define EDYNHIP_PATH_COMPACT_DIRECT     (1ull << 0)   /* pair compaction: k_bp_compact<true>, its own scan */
#define EDYNHIP_PATH_COMPACT_LIBRARY    (1ull << 1)   /* pair compaction: scan_u32 + k_bp_compact<false> */
#define EDYNHIP_PATH_SORT_DIRECT        (1ull << 2)   /* colour sort: k_cs_hist<true> + k_cs_scatter<true> */
#define EDYNHIP_PATH_SORT_LIBRARY       (1ull << 3)   /* colour sort: k_cs_hist<false> + scan_u32 + k_cs_scatter<false> + k_col_offsets */
#define EDYNHIP_PATH_SPECULATE          (1ull << 4)   /* the manifold build was launched before the pair count reached the host */
#define EDYNHIP_PATH_INPLACE            (1ull << 5)   /* a step kept the previous step's manifold array (unchanged pair set) */
#define EDYNHIP_PATH_LISTS_FORCED       (1ull << 6)   /* the tree was walked in a step in which the candidate lists were still valid (EDYNHIP_BP_LISTS=0) */
#define EDYNHIP_PATH_LOOKAHEAD_CHANGED  (1ull << 7)   /* the candidate lists' look-ahead was halved or doubled */
#define EDYNHIP_PATH_RELABEL_COMPRESS0  (1ull << 8)   /* a step found its label certificate broken and relabelled the islands in full (the forced relabel after a scene edit does not count), with no pointer-jumping pass */
#define EDYNHIP_PATH_RELABEL_COMPRESS1  (1ull << 9)   /*   ... with one */
#define EDYNHIP_PATH_RELABEL_COMPRESSN  (1ull << 10)  /*   ... with more than one */
#define EDYNHIP_PATH_VEL_XCD            (1ull << 11)  /* dataflow velocity launch with XCD-local task lists */
#define EDYNHIP_PATH_POS_XCD            (1ull << 12)  /* dataflow position launch with XCD-local task lists */
#define EDYNHIP_PATH_VEL_LANES1         (1ull << 13)  /* k_contact_solve_df */
#define EDYNHIP_PATH_VEL_LANES2         (1ull << 14)  /* k_contact_solve_df2 */
#define EDYNHIP_PATH_VEL_LANES4         (1ull << 15)  /* k_contact_solve_df4 */
#define EDYNHIP_PATH_VEL_MULTI_ROUND    (1ull << 16)  /* a dataflow velocity launch whose waves take more than one task per sweep */
#define EDYNHIP_PATH_POS_MULTI_ROUND    (1ull << 17)  /* the same for a dataflow position launch */
#define EDYNHIP_PATH_POS_COLOUR_PUSH    (1ull << 18)  /* position solve per colour behind a dataflow (push) velocity solve */
#define EDYNHIP_PATH_MIXED              (1ull << 19)  /* mixed schedule */
#define EDYNHIP_PATH_ISLAND_FUSED       (1ull << 20)  /* island-fused schedule */
#define EDYNHIP_PATH_PER_COLOUR         (1ull << 21)  /* velocity solve per colour */
#define EDYNHIP_PATH_POLY_ONE_LANE      (1ull << 22)  /* polyhedron pairs: one lane per pair in k_np_detect_poly */
#define EDYNHIP_PATH_POLY_AXES8         (1ull << 23)  /* k_np_pp_axes<8> */
#define EDYNHIP_PATH_POLY_AXES16        (1ull << 24)  /* k_np_pp_axes<16> */
#define EDYNHIP_PATH_POLY_CONTACTS4     (1ull << 25)  /* k_np_pp_contacts<4> */
#define EDYNHIP_PATH_POLY_CONTACTS8     (1ull << 26)  /* k_np_pp_contacts<8> */
#define EDYNHIP_PATH_POLY_CONTACTS16    (1ull << 27)  /* k_np_pp_contacts<16> */
#define EDYNHIP_PATH_POLY_HINTS         (1ull << 28)  /* separating-axis hints used */
#define EDYNHIP_PATH_RECORDS_DIRECT     (1ull << 29)  /* edynhip_snapshot_records packed straight into the pinned slot */
#define EDYNHIP_PATH_RECORDS_COPY       (1ull << 30)  /* ... through a device block and the copy engine */
#define EDYNHIP_PATH_WORLD_SERIAL       (1ull << 31)  /* multi-device world only: the shards were stepped on the caller's thread */
#define EDYNHIP_PATH_VEL_NAP            (1ull << 32)  /* k_contact_solve_df2 launched with a pause between polls other than the default (EDYNHIP_DF_NAP) */
#define EDYNHIP_PATH_LISTS_KEPT         (1ull << 33)  /* a full step ran the exact predicates over candidate lists built in an earlier step */
#define EDYNHIP_PATH_LISTS_MOVED        (1ull << 34)  /* a full step rebuilt the candidate lists on the device's own flag (a body left its slack) */
#define EDYNHIP_PATH_PAIR_SURPLUS       (1ull << 35)  /* some owner reported pairs through the unsorted surplus (more than 64 partners, or a sleeping owner): the surplus sort ran */
int edynhip_debug_paths(edynhip_ctx *ctx, uint64_t *mask);
/* Test hook beside edynhip_debug_paths (additive to ABI 15): how many steps since creation brought the island labels up to date with
 * a full relabel (scene edits and forced relabels included) and how many by hooking only the step's new manifolds onto last step's
 * labels. A step in which neither number moved was skipped (an unchanged pair set) or had nothing to relabel. Host counters: no kernel
 * touches them. */
int edynhip_debug_relabel_steps(edynhip_ctx *ctx, uint64_t *full, uint64_t *incremental);

/* Island sleeping (EDYNHIP_FLAG_SLEEPING): asleep[n] = 1 where the body carries sleeping_tag; wake_all = wake_up_entity on
 * everything (also implied by edynhip_set_state). island_manager.cpp:541-565, util/island_util.cpp:61-66. */
int edynhip_get_asleep(edynhip_ctx *ctx, uint8_t *asleep);
int edynhip_wake_all(edynhip_ctx *ctx);
/* wake_up_entity (util/rigidbody.cpp:409-415 -> wake_up_island, util/island_util.cpp:61-66): wakes the islands of the listed bodies.
 * The sleeping tags come off; the sleep timer of an island that was awake already is not restarted. */
int edynhip_wake_bodies(edynhip_ctx *ctx, uint32_t n, const uint32_t *indices);
/* edyn::set_center_of_mass on a running world (util/rigidbody.cpp:364-370, apply_center_of_mass :517-548): the body's position and linear
 * velocity move to the new centre of mass (given in the shape's frame; zero removes the offset), its origin - shape, contact and joint
 * pivots - stays where it is, its inertia is not changed. */
int edynhip_set_center_of_mass(edynhip_ctx *ctx, uint32_t body, const float *com3);

int edynhip_get_timings(edynhip_ctx *ctx, edynhip_timings *out);
int edynhip_get_stats(edynhip_ctx *ctx, edynhip_stats *out);
/* State a caller carries from one context into another (the C++ shim re-creates a context to grow it): the joints' applied
 * impulses - all 24 slots per joint, the layout of edynhip_get_joint_slot_impulses - and tracked angles (the 10th value of
 * edynhip_get_joint_impulses; NULL keeps the angles), by caller joint index; and the sleeping tags of the bodies (as
 * edynhip_get_asleep returns them; sleeping bodies get zero velocities, island timers of awake islands restart). */
int edynhip_set_joint_warm_start(edynhip_ctx *ctx, const float *impulses24, const float *angles);
int edynhip_set_asleep(edynhip_ctx *ctx, const uint8_t *asleep);
/* ... and the island sleep TIMERS (island::sleep_timestamp, island_manager.cpp:605-623; ABI 14): island_label[n] = every body's island (the
 * lowest body index of the island, as edynhip_get_derived returns it), since[n] = by island label, the time stamp at which the island first
 * met the sleep thresholds (negative or NaN: no timer running; entries that are not labels are ignored), clock = the stamp of the last step.
 * A context that receives them (after its bodies, manifolds and sleeping tags) continues the timers where the other context left them - its
 * first step relabels from the given labels, so an island that merges or splits in that very step follows the rules of a running world -
 * instead of starting every timer again. A no-op without EDYNHIP_FLAG_SLEEPING. */
int edynhip_get_sleep_timers(edynhip_ctx *ctx, uint32_t *island_label, double *since, double *clock);
int edynhip_set_sleep_timers(edynhip_ctx *ctx, const uint32_t *island_label, const double *since, double clock);

/* The version changes when a caller built against the previous header would misbehave: a struct's layout or size, a function's signature,
 * the meaning of an argument, a flag or a result. A new entry point beside the existing ones ("additive to ABI n" where it is declared)
 * leaves it alone: nothing an older caller uses has moved, and a newer caller looks the symbol up. */
uint32_t edynhip_abi_version(void);

/* polyhedron_shape's convex_mesh (include/edyn/shapes/convex_mesh.hpp:17-70): vertices[num_vertices][3], the faces' vertex indices
 * (counter-clockwise seen from outside) and faces[num_faces][2] = (first index, vertex count). Does what convex_mesh::initialize does
 * (src/edyn/shapes/convex_mesh.cpp:10-30): moves the vertices so that the centroid is the origin, derives face normals, unique edges,
 * vertex adjacency and the relevant (direction-unique) faces and edges. The mesh belongs to the context and is shared by every body
 * whose shape is EDYNHIP_SHAPE_POLYHEDRON with shape_param[0] = *mesh_id (the shared_ptr<convex_mesh> of the reference); meshes are
 * created before the bodies that use them. flags: EDYNHIP_MESH_INITIALIZED = the vertices come from a convex_mesh on which
 * initialize() already ran (they are relative to the centroid): they are taken as they are and only the derived arrays are built.
 * Limits: closed mesh of positive volume, at most 32 vertices per face (support polygons are held in fixed storage on the device). */
enum { EDYNHIP_MESH_INITIALIZED = 1u };
int edynhip_create_convex_mesh(edynhip_ctx *ctx, uint32_t num_vertices, const float *vertices, uint32_t num_indices, const uint32_t *indices,
                               uint32_t num_faces, const uint32_t *faces, uint32_t flags, uint32_t *mesh_id);
/* The derived arrays of a mesh (parity tests; out == NULL returns the element count): float fields [count][3], index fields uint32. */
enum { EDYNHIP_MESH_VERTICES = 0, EDYNHIP_MESH_NORMALS = 1, EDYNHIP_MESH_RELEVANT_NORMALS = 2, EDYNHIP_MESH_EDGE_VERTICES = 3,
       EDYNHIP_MESH_EDGE_NORMALS = 4, EDYNHIP_MESH_EDGES = 5, EDYNHIP_MESH_EDGE_FACES = 6, EDYNHIP_MESH_RELEVANT_FACES = 7,
       EDYNHIP_MESH_RELEVANT_EDGES = 8, EDYNHIP_MESH_NEIGHBORS_START = 9, EDYNHIP_MESH_NEIGHBOR_INDICES = 10,
       EDYNHIP_MESH_INERTIA_SUMS = 11 /* 7 floats: the face sums of moment_of_inertia_polyhedron (volume, xx, yy, zz, yz, zx, xy) */ };
int edynhip_get_convex_mesh(edynhip_ctx *ctx, uint32_t mesh_id, int field, void *out, uint32_t capacity, uint32_t *count);

/* Measurement aid for the roofline report (bench.py): streams `bytes` of device memory with 16-byte loads from every CU (read_gbs)
 * and copies them device-to-device (copy_gbs, read + write bytes counted), best of five runs each, on the context's stream.
 * Not part of the step path. */
int edynhip_measure_bandwidth(edynhip_ctx *ctx, uint64_t bytes, float *read_gbs, float *copy_gbs);

/* ------------------------------------------------------------------------------------------------ Multi-GPU world (ABI 12)
 * ONE simulation over several GPUs of a node at island granularity - the reference's own unit of parallelism
 * (src/edyn/dynamics/solver.cpp:408-428 runs every island as its own task; islands share only non-procedural bodies, which a
 * step never writes: include/edyn/comp/island.hpp:34-41). An application reaches it through edyn::attach with
 * init_config::devices (include/edyn/edyn.hpp of this repository; the reference's attach: include/edyn/edyn.hpp:66-70).
 * Every device gets one edynhip_ctx (a "shard") that owns the dynamic bodies of its islands plus a replica of every non-dynamic
 * body; shards step concurrently (one private host thread each) with NO exchange inside a step; after each step the integrated
 * state of every shard is copied into pinned host memory and from there into the world's arrays (edynhip_world_get_state); the
 * registry write-back reads edynhip_world_snapshot_records' records in place (below). Islands of different shards that approach each other are noticed from island bounding boxes reduced ON
 * THE DEVICE (edyn_amd/csrc/multi_partition.hip), and the world re-partitions, carrying contact manifolds (warm-start impulses, colours),
 * joint impulses / angles, sleeping tags, exclusions, joint definitions and meshes to the islands' new owners. A shard computes
 * for its islands bit for bit what one context computes for the whole world (tests/cpp/multi.cpp).
 * Body / joint indices of this interface are GLOBAL (the caller's order). `devices` may name a device more than once (several
 * shards on one GPU: functional tests). Scene description calls (meshes, bodies, joints, definitions, exclusions - in this order)
 * come before the first step; a later edynhip_world_set_bodies starts a new world. */
typedef struct edynhip_world edynhip_world;
typedef struct {
    uint32_t num_shards, num_bodies;
    uint32_t steps;                  /* steps taken since creation */
    uint32_t approach_checks;        /* island-box sweeps (device reduction + host sweep) */
    uint32_t repartitions;           /* times the shards were rebuilt because islands of different shards met (or on request) */
    uint32_t bodies_per_shard[16];   /* bodies whose state each shard reports (shard 0 also reports the replicated ones) */
    uint32_t rebalances;             /* meetings that took the full, load-balanced re-partition because the heaviest shard exceeded 1.5 x the mean (ABI 15) */
    uint32_t extras_carries;         /* re-partitions that carried the points' extras (materials, below); always 0 in a world without materials.
                                        Appended at the end of the struct with edynhip_world_set_material_extras: no earlier field has moved */
} edynhip_world_stats;
edynhip_world *edynhip_world_create(const edynhip_config *cfg /* .device is ignored; capacities 0 = sized per shard */,
                                    const int32_t *devices, uint32_t num_devices, int *status_out);
void edynhip_world_destroy(edynhip_world *w);
const char *edynhip_world_last_error(const edynhip_world *w);   /* w may be NULL: error of the last failed create */
int edynhip_world_create_convex_mesh(edynhip_world *w, uint32_t num_vertices, const float *vertices, uint32_t num_indices, const uint32_t *indices,
                                     uint32_t num_faces, const uint32_t *faces, uint32_t flags, uint32_t *mesh_id);
int edynhip_world_set_bodies(edynhip_world *w, uint32_t n, const edynhip_bodies *bodies);
/* The scene description (joints, joint definitions, exclusions) is what the shards are (re)built from, with the state of
 * edynhip_world_set_bodies: these three calls come before the first step. On a world that has been stepped they return EDYNHIP_ERR_UNSUPPORTED
 * (a rebuild would reset the simulation to its initial state); describe the scene again - edynhip_world_set_bodies with the current state -
 * to edit a running world. The initial island probe loads the whole scene onto devices[0]: a scene must fit one GPU's memory once. */
int edynhip_world_set_joints(edynhip_world *w, uint32_t n, const edynhip_joints *joints);
/* edynhip_set_joint_definition (generic = 0: params[16]) / edynhip_set_generic_definition (generic = 1: params[60]) by global joint index */
int edynhip_world_set_joint_definition(edynhip_world *w, uint32_t joint, const float *frame_a9, const float *frame_b9, const float *params, int generic);
int edynhip_world_exclude_collision(edynhip_world *w, uint32_t body_a, uint32_t body_b);
/* settings.should_collide_func on a world over several devices (ABI 14): `filter(user, body, other)` is asked with GLOBAL body indices by
 * whichever shard holds the candidate pair (see edynhip_set_pair_filter for when and how often); the shards step on their own host
 * threads, the calls are serialised. May be set before or after the shards exist; filter = NULL restores the device test.
 * edynhip_world_default_should_collide: collision groups / masks and exclusion lists of the scene, in global indices. */
int edynhip_world_set_pair_filter(edynhip_world *w, edynhip_pair_filter filter, void *user);
int edynhip_world_default_should_collide(edynhip_world *w, uint32_t body_a, uint32_t body_b);
/* edyn::step_simulation on every shard, then the gather, the approach test and - when islands of different shards have met - the
 * re-partition. Returns when the state of the last step is in the world's arrays. */
int edynhip_world_step(edynhip_world *w, uint32_t nsteps);
int edynhip_world_get_state(edynhip_world *w, float *pos, float *orn, float *linvel, float *angvel);   /* any may be NULL */
int edynhip_world_get_partition(edynhip_world *w, int32_t *shard_of_body);   /* -1 = replicated (not dynamic) */
int edynhip_world_repartition(edynhip_world *w);                             /* re-partition now (load balance / tests) */
int edynhip_world_get_manifolds(edynhip_world *w, edynhip_manifold *out, uint32_t capacity, uint32_t *n);   /* global indices, canonical order */
int edynhip_world_get_stats(edynhip_world *w, edynhip_world_stats *out);
edynhip_ctx *edynhip_world_context(edynhip_world *w, uint32_t shard);        /* a shard's context (read-only use: statistics, timings).
    Since the world has materials of its own (edynhip_world_set_material_extras, below) the four single-context material calls -
    edynhip_set_material_extras / _set_material_ids / _insert_material_mixing / _get_point_extras - return EDYNHIP_ERR_UNSUPPORTED on it,
    like the queries: read a world's point extras through edynhip_world_get_point_extras */

/* edynhip_raycast / edynhip_query_aabb on a multi-device world (additive to ABI 15). Arguments, result layout, flags, capacity rules and
 * error codes are those of the single-context calls; every body index - the ignore list, hit.body, ids, island labels - is GLOBAL. The
 * answer is bit for bit what ONE context holding the whole scene returns for the same call: every body is answered by exactly one
 * shard (shard 0: the replicated non-dynamic bodies and its own dynamic ones; any other shard: the dynamic bodies it owns) with the
 * single context's kernels, local indices are translated on the shard's device, and the answers are merged on the home device,
 * devices[0] (smallest fraction, ties to the lowest global index; hit lists in ascending global index) - edyn_amd/csrc/world_query.hip.
 * A world that has been described but not stepped builds its shards first, as edynhip_world_step does, and is seen in the described
 * state; after a step the queries see the state edynhip_world_get_state returns. A query changes nothing a later step computes.
 * The public single-context calls keep refusing a shard context (edynhip_world_context) with EDYNHIP_ERR_UNSUPPORTED.
 * The _device variants take pointers on devices[0]. Unlike the single-context ones they BLOCK the calling thread until every shard has
 * answered and the merge has run: the inputs must be complete when the call is made (synchronise the stream that wrote them) and the
 * results are complete when it returns. Rays, boxes, hits and ids travel device to device, never through pageable host memory.
 * edynhip_world_query_aabb_device with ids: every shard's own total must be below 2^32 - 1 (EDYNHIP_ERR_CAPACITY otherwise). */
int edynhip_world_raycast(edynhip_world *w, uint32_t n, const float *p0, const float *p1,
                          uint32_t num_ignore, const uint32_t *ignore, uint32_t flags, edynhip_raycast_hit *out);
int edynhip_world_raycast_device(edynhip_world *w, uint32_t n, const void *p0_f4, const void *p1_f4,
                          uint32_t num_ignore, const uint32_t *ignore, uint32_t flags, void *out);
int edynhip_world_query_aabb(edynhip_world *w, int category, uint32_t n, const float *boxes6, uint32_t flags,
                          uint32_t *offsets, uint32_t *ids, uint32_t capacity, uint32_t *total);
int edynhip_world_query_aabb_device(edynhip_world *w, int category, uint32_t n, const void *boxes_f4, uint32_t flags,
                          void *offsets, void *ids, uint32_t capacity, void *total);
/* edynhip_get_contact_events / edynhip_get_point_ids on a multi-device world (additive to ABI 15), for a world created with
 * EDYNHIP_FLAG_CONTACT_EVENTS (without it: EDYNHIP_ERR_UNSUPPORTED). The application sees the event stream and the point identities of
 * ONE context holding the whole scene; only the VALUES of the point ids differ.
 *   events: those of all steps of the last edynhip_world_step call (also of the steps before a re-partition inside that call), in no
 *     particular order within a step; body[] = GLOBAL indices in the order edynhip_world_get_manifolds reports the pair; step = the world's
 *     steps since edynhip_world_set_bodies. With point_id left out, the multiset of (type, step, body[0], body[1]) is the single
 *     context's. out == NULL counts; capacity < *n: EDYNHIP_ERR_CAPACITY. A world that is described but not yet stepped has 0 events. If
 *     one shard recorded more events than its context holds, `n` is capped and EDYNHIP_ERR_CAPACITY is returned (after `out` is filled):
 *     resynchronise from edynhip_world_get_manifolds + edynhip_world_get_point_ids.
 *   point ids: ids[4 * i + k] = id of point k of manifold i in edynhip_world_get_manifolds order, 0 where there is no point. An id is
 *     unique among the living points of the world and stays the same from POINT_CREATED to POINT_DESTROYED, whichever shards the point
 *     lives on in between: a re-partition - sticky or full, by itself or through edynhip_world_repartition, rebuilt and kept contexts alike -
 *     emits no event and changes no id. id = (world step of creation + 1) << 32 | shard of creation << 28 | manifold index there << 2 | slot;
 *     hence at most 16 shards and 2^26 manifolds per shard with this flag (edynhip_world_step: EDYNHIP_ERR_CAPACITY otherwise).
 * Every shard translates its step's events to global indices on its own device and the blocks are appended, device to device, to one list
 * on devices[0] (edyn_amd/csrc/world_events.hip); reading the events is one copy from there. A world without the flag runs none of this.
 * A shard context (edynhip_world_context) stays read-only: its own edynhip_get_contact_events speaks local indices. */
int edynhip_world_get_contact_events(edynhip_world *w, edynhip_contact_event *out, uint32_t capacity, uint32_t *n);
int edynhip_world_get_point_ids(edynhip_world *w, uint64_t *ids, uint32_t capacity_manifolds, uint32_t *n);
/* Edits of a RUNNING multi-device world (additive to ABI 15): what edynhip_add_bodies / _remove_bodies / _add_joints / _remove_joints /
 * _set_joint_params / _set_joint_definition / _set_generic_definition / _exclude_collision / _remove_collision_exclusion / _set_state /
 * _get_params / _set_params do on one context, in GLOBAL indices - registry.create + make_rigidbody and registry.destroy on a running
 * world (src/edyn/util/rigidbody.cpp:18-161, src/edyn/edyn.cpp:148-197, island_manager.cpp:47-115), make_constraint / destroy of a
 * constraint (include/edyn/util/constraint_util.hpp:38-54, island_manager.cpp:68-97), registry.patch of a constraint, exclude_collision
 * (src/edyn/util/exclude_collision.cpp:9-71), edyn::refresh of the state pools, set_fixed_dt / set_solver_*_iterations / set_gravity
 * (src/edyn/edyn.cpp:203-207). After any sequence of these and steps the world returns, bit for bit, what ONE context holding the whole
 * scene returns after the same edits and steps.
 *   indices   new bodies take num_bodies .., new joints the next joint indices (*first_index, may be NULL); a removed body's index stays
 *             reserved (the slot is a shapeless static body, edynhip_world_get_partition reports -1 for it), its joints go with it and the
 *             islands it touched wake up; a removed joint keeps its index. Removing what is already removed is accepted and does nothing.
 *   placement a new body that is not dynamic is replicated on every shard (shard 0 reports it); a new dynamic body goes to the shard that
 *             owns the fewest live dynamic bodies at that moment (the bodies of one call are placed one after the other in index order;
 *             ties: the lowest shard) and takes with it every later body of the same call that it touches, directly or through others
 *             (the boxes of their bounding spheres within the manifold-creation margin): a pile spawned in one call lands on one shard.
 *   safety    before the next step no body of one shard is within the manifold-creation margin of an island of another and no joint spans
 *             two shards: after a shaped dynamic body was added the world runs its approach check (new bodies are islands of their own)
 *             and, if that says "close", the sticky re-partition; a joint between two shards re-partitions first (its islands move
 *             together by the sticky rule) and is then made in place; edynhip_world_set_state makes the check due after the next step,
 *             which is when a context's broadphase first sees the moved boxes.
 *   in place  every edit is forwarded to the shard context(s) that hold the bodies / the joint and the world's tables follow: no shard is
 *             rebuilt and nothing is re-partitioned unless the safety rule asks for it. An add that exceeds a shard's body or joint
 *             capacity first rebuilds THAT shard with head-room through what a re-partition carries (manifolds with impulses and point
 *             ids, joint impulses and angles, sleep state) and then runs in place; edynhip_world_edit_stats counts each path.
 *   described On a world that is described but whose shards are not built yet the calls extend or alter the description.
 *   errors    out-of-range indices, missing arrays, a joint to a removed body: EDYNHIP_ERR_INVALID (edynhip_world_last_error); the world
 *             is left as it was.
 * The three scene-description calls above keep refusing a stepped world and edynhip_world_set_bodies still starts a new world.
 * edynhip_world_edit_joint: generic = -1: params[10] (edynhip_set_joint_params; frames ignored, may be NULL), 0: params[16]
 * (edynhip_set_joint_definition), 1: params[60] (edynhip_set_generic_definition). edynhip_world_edit_exclusion: exclude = 1
 * edynhip_exclude_collision, 0 edynhip_remove_collision_exclusion. */
typedef struct {
    uint32_t edits;                   /* edit calls that changed a built world */
    uint32_t in_place;                /* ... of which ran without rebuilding a shard and without a re-partition */
    uint32_t shard_rebuilds;          /* shards rebuilt with head-room because an add did not fit, or because a body's kind crossed between dynamic and not */
    uint32_t repartitions_by_edit;    /* sticky re-partitions an edit caused (close islands, a joint between two shards) */
    uint32_t approach_checks_by_edit; /* approach checks run right after an edit */
} edynhip_world_edit_stats;
int edynhip_world_add_bodies(edynhip_world *w, uint32_t n, const edynhip_bodies *bodies, uint32_t *first_index);
int edynhip_world_remove_bodies(edynhip_world *w, uint32_t n, const uint32_t *body_indices);
int edynhip_world_add_joints(edynhip_world *w, uint32_t n, const edynhip_joints *joints, uint32_t *first_index);
int edynhip_world_remove_joints(edynhip_world *w, uint32_t n, const uint32_t *joint_indices);
int edynhip_world_edit_joint(edynhip_world *w, uint32_t joint, const float *frame_a9, const float *frame_b9, const float *params, int generic);
int edynhip_world_edit_exclusion(edynhip_world *w, uint32_t body_a, uint32_t body_b, int exclude);
int edynhip_world_set_state(edynhip_world *w, const float *pos, const float *orn, const float *linvel, const float *angvel);
int edynhip_world_get_params(edynhip_world *w, edynhip_params *out);
int edynhip_world_set_params(edynhip_world *w, const edynhip_params *params);
int edynhip_world_get_edit_stats(edynhip_world *w, edynhip_world_edit_stats *out);
/* edynhip_edit_bodies / edynhip_wake_bodies on a multi-device world (additive to ABI 15): same arguments, field groups
 * (EDYNHIP_EDIT_MASS .. _KIND) and per-group semantics, GLOBAL body indices. After any sequence of these calls, the other world edits and
 * steps the world returns, bit for bit, what ONE context holding the whole scene returns - state, manifolds, sleeping tags, the multiset of
 * contact events, point ids up to the known renaming, queries, records - right after the call and after every later step.
 *   where     an edit of a dynamic body goes to the shard that owns it, an edit of a replicated (static or kinematic) body to every
 *             shard, each in that shard's local indices on the shard's own thread; a polyhedron edit first creates the mesh on a shard
 *             that lacks it. The scene stays the truth: every edited member lands in the world's description, so whatever rebuilds a
 *             shard later produces the edited body. A body made static has zero velocities in edynhip_world_get_state at once.
 *   in place  MASS, INERTIA, MATERIAL, SHAPE, KIND between kinematic and static, KIND on a body that stays dynamic: no shard is rebuilt,
 *             nothing is re-partitioned (unless the safety rule below asks), nothing sized by a shard is read back or uploaded
 *             (edynhip_world_edit_stats: edits + 1, in_place + 1). With one shard every edit is in place.
 *   crossing  KIND between dynamic and not dynamic changes who holds the body. Local indices ascend with the global ones, so the body cannot
 *             be appended to another shard's context. Dynamic to static / kinematic: the owner is edited in place (the drop, the events, the
 *             wakes), the body becomes replicated, and the OTHER shards are rebuilt, with the replica, through what a sticky re-partition
 *             carries. Static / kinematic to dynamic: every shard edits its replica in place (each drops its own manifolds of the body, emits
 *             their events, wakes the partners: the union is what one context does), the body goes to the shard that owns the fewest live
 *             dynamic bodies (ties: the lowest shard) and the other shards are rebuilt without it; joints of the body to islands of other
 *             shards move those islands together as edynhip_world_add_joints does. Warm starts, joint impulses and angles, sleep tags and
 *             timers, point ids and the step count survive. Counted in shard_rebuilds / repartitions_by_edit, not in in_place.
 *   safety    a SHAPE edit of a dynamic body, or a KIND edit to dynamic, can bring islands of two shards within the creation margin before
 *             the next step: the world runs the approach check at once (which also refreshes the growth monitor's reference boxes) and the
 *             sticky re-partition if it says "close". Edits of replicated bodies need no check.
 *   events    with EDYNHIP_FLAG_CONTACT_EVENTS the POINT_DESTROYED / MANIFOLD_DESTROYED records of a SHAPE or KIND edit are translated on
 *             the shard's device (the tail of its list only) and appended to the world's list: edynhip_world_get_contact_events then
 *             returns the last step call's events plus the edit's, as one context does. Without the flag none of this runs.
 *   described on a world that is described but not built the call alters the description only.
 *   errors    what edynhip_edit_bodies refuses (index out of range, a removed body, an index listed twice, a bad mesh id, dynamic without
 *             MASS + INERTIA, an unknown group ...), decided before anything changes on any shard: the world is left as it was.
 * edynhip_world_wake_bodies: out-of-range indices are refused, removed bodies accepted and ignored; forwarded to the shards that hold the
 * bodies (a body's island lives on one shard); counts as an in-place edit; does nothing without EDYNHIP_FLAG_SLEEPING or on an unbuilt world. */
int edynhip_world_edit_bodies(edynhip_world *w, uint32_t n, const uint32_t *indices, const edynhip_bodies *values, uint32_t fields);
int edynhip_world_wake_bodies(edynhip_world *w, uint32_t n, const uint32_t *indices);
/* edynhip_set_material_extras / _set_material_ids / _insert_material_mixing / _get_point_extras on a multi-device world (additive to ABI 15):
 * same arguments, same rules, GLOBAL body indices, before the first step or on a running world. The world returns, bit for bit, what ONE
 * context holding the whole scene returns after the same calls and steps.
 *   where     a body's material goes to the shard that owns it, a replicated (non-dynamic) body's to every shard, the mix table - the
 *             insertions in the order they were made - to every shard; whatever builds or rebuilds a shard applies them again.
 *   in place  on a running world the calls are forwarded to the shard contexts; no shard is rebuilt and nothing is re-partitioned
 *             (edynhip_world_edit_stats counts them as in-place edits). As on one context only points created from then on see a change.
 *   carry     a point's material as mixed at its creation and the impulses of its rolling pair and spinning row go with it through every
 *             re-partition (sticky or full, rebuilt and kept contexts alike), gathered and put back on the shards' devices
 *             (edyn_amd/csrc/world_extras.hip), once the world holds any such material or mix-table entry; edynhip_world_stats.extras_carries
 *             counts these. A world without materials gathers, copies and allocates nothing for it.
 *   schedule  a shard none of whose bodies has a contact_extras material keeps its fast solve schedule (every schedule computes the same bits).
 *   reading   edynhip_world_get_point_extras: out7[4 * i + k][7] of point k of manifold i in edynhip_world_get_manifolds order; out7 == NULL
 *             counts; capacity_manifolds < *n: EDYNHIP_ERR_CAPACITY (*n is set). edynhip_world_set_bodies resets the bodies' materials and
 *             ids; the mix table stays, as on one context.
 *   errors    a body range beyond num_bodies, ids above 0xFFFF, an unassigned id in a mix entry, negative friction or non-positive stiffness /
 *             damping, a missing array: EDYNHIP_ERR_INVALID (edynhip_world_last_error); the world is left as it was.
 * The public single-context calls refuse a shard context (edynhip_world_context) with EDYNHIP_ERR_UNSUPPORTED. */
int edynhip_world_set_material_extras(edynhip_world *w, uint32_t first, uint32_t n, const float *spin_friction, const float *roll_friction,
                                      const float *stiffness, const float *damping);
int edynhip_world_set_material_ids(edynhip_world *w, uint32_t first, uint32_t n, const uint32_t *ids);
int edynhip_world_insert_material_mixing(edynhip_world *w, uint32_t id0, uint32_t id1, const float *material6);
int edynhip_world_get_point_extras(edynhip_world *w, float *out7, uint32_t capacity_manifolds, uint32_t *n);
/* edynhip_get_asleep on the whole world (additive to ABI 15): asleep[num_bodies], every body's sleeping_tag from the shard that reports
 * its state; all 0 without EDYNHIP_FLAG_SLEEPING. (With tombstones in the world the partition no longer tells which bodies a shard holds.) */
int edynhip_world_get_asleep(edynhip_world *w, uint8_t *asleep);
/* edynhip_snapshot_records / edynhip_snapshot_map on a multi-device world (additive to ABI 15): the registry write-back read in place.
 * Same edynhip_record_view, same contract, and - record for record, byte for byte - what ONE context holding the whole scene hands over:
 *   records[num_bodies]  by GLOBAL body index. Every shard packs the bodies it reports (its own dynamic bodies; shard 0 also the replicated
 *                        ones) with the single context's record arithmetic and stores them straight into the world's pinned slot, which
 *                        is allocated portable and mapped so that every shard's device writes into it (edyn_amd/csrc/world_records.hip);
 *                        a removed body keeps its tombstone record (EDYNHIP_RECORD_REMOVED) whichever shard holds the slot.
 *   step_index           the world's steps since edynhip_world_set_bodies.
 *   events               the first min(max_events, n) records of edynhip_world_get_contact_events' list for the last edynhip_world_step call,
 *                        same order, same bytes, copied from devices[0] after the shards' appends; NULL on a world created without
 *                        EDYNHIP_FLAG_CONTACT_EVENTS. total_events = the events that occurred - the sum of what the shards counted, also
 *                        where a shard's own list overflowed - so total_events > num_events exactly when the list was cut anywhere:
 *                        resynchronise from edynhip_world_get_manifolds + edynhip_world_get_point_ids then.
 * edynhip_world_snapshot_records enqueues the packs behind the steps issued so far (edynhip_world_step returns with the shards idle) and
 * returns; edynhip_world_snapshot_map waits for THAT snapshot only. The world owns two slots, used alternately: the pointers stay valid
 * until the next-but-one edynhip_world_snapshot_records call; a slot grows (and may move) when it is reused for more bodies or events.
 * flags: 0 or EDYNHIP_SNAPSHOT_DIRECT - both store directly into the pinned slot; anything else: EDYNHIP_ERR_INVALID. A map before any
 * snapshot: EDYNHIP_ERR_INVALID. A world that is described but not stepped builds its shards first and hands over the described state. */
int edynhip_world_snapshot_records(edynhip_world *w, float present_dt, uint32_t max_events, uint32_t flags);
int edynhip_world_snapshot_map(edynhip_world *w, edynhip_record_view *view);
/* edynhip_debug_paths of a multi-device world (additive to ABI 15): the OR over every shard context the world has had, plus
 * EDYNHIP_PATH_WORLD_SERIAL when the shards were stepped one after the other on the caller's thread. */
int edynhip_world_debug_paths(edynhip_world *w, uint64_t *mask);

/* The pieces of the above that processes owning ONE GPU each use (edyn_amd/parallel.py ShardedWorld over torch.distributed / RCCL):
 * the island partitioner - longest-processing-time-first over the summed weights, deterministic (islands by descending weight, ties
 * by ascending label, each to the lightest rank, ties to the lowest rank); rank_of[i] = -1 for non-dynamic bodies. weights may be
 * NULL (1 per body). Host only: no GPU needed. */
int edynhip_partition_islands(uint32_t n, const uint32_t *island_label, const int32_t *kind, const double *weights, uint32_t world_size, int32_t *rank_of);
/* island boxes [num][6] (min, max) grown by `margin` on every side that overlap: pairs (label_a < label_b), sorted, without
 * duplicates; any_owner = 0: only pairs of different owners. pairs may be NULL (count only). Host only. */
int edynhip_island_boxes_overlap(uint32_t num_islands, const float *boxes6, const uint32_t *labels, const int32_t *owner, float margin, int any_owner,
                                 uint32_t *pairs, uint32_t capacity, uint32_t *num_pairs);
/* per island of the context (label = its lowest body index, as edynhip_get_derived returns them) the union of the AABBs of its
 * shaped dynamic bodies, reduced on the device after the last step. labels / boxes6 may be NULL (count only). */
int edynhip_get_island_boxes(edynhip_ctx *ctx, uint32_t *labels, float *boxes6, uint32_t capacity, uint32_t *num_islands);

#ifdef __cplusplus
}
#endif
#endif /* EDYNHIP_H */
