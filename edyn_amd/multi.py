"""MultiWorld: thin binding of the library's multi-GPU world (include/edynhip.h "Multi-GPU world", edyn_amd/csrc/multi*.hip).

One simulation, several GPUs of one node, one process: every device steps the islands it owns (solver.cpp:408-428: the island is
the reference's own unit of parallelism), the library gathers the state after every step, watches island bounding boxes reduced on
the devices and re-partitions when islands of different shards meet. Everything happens behind the C-ABI; this class only
marshals arrays. (Processes that own one GPU each - torch.distributed ranks over RCCL - use edyn_amd.parallel.ShardedWorld, which
shares the library's partitioner and box sweep.)"""
import ctypes as C
import numpy as np
from . import _capi
from ._capi import EdynHipError, MANIFOLD_DTYPE
from .world import World, init_config, _ptr, _edit_arrays


class MultiWorld:
    def __init__(self, config=None, devices=(0,)):
        self.cfg = config or init_config()
        self._L = _capi.lib()
        cfg = _capi.Config()
        cfg.device = 0
        cfg.max_bodies = 0; cfg.max_manifolds = int(self.cfg.max_manifolds); cfg.max_joints = 0
        cfg.fixed_dt = self.cfg.fixed_dt
        cfg.num_velocity_iterations = self.cfg.num_solver_velocity_iterations
        cfg.num_position_iterations = self.cfg.num_solver_position_iterations
        cfg.gravity = (C.c_float * 3)(*[float(x) for x in self.cfg.gravity])
        cfg.flags = ((_capi.FLAG_SLEEPING if self.cfg.sleeping else 0) | (_capi.FLAG_EXCLUSIVE_DEVICE if self.cfg.exclusive_device else 0)
                     | (_capi.FLAG_TIMING_SOLVE if self.cfg.timing_solve else 0)
                     | (_capi.FLAG_CONTACT_EVENTS if self.cfg.contact_events else 0)
                     | (_capi.FLAG_FUSED_VELOCITY_ROWS if self.cfg.fused_velocity_rows else 0) | (_capi.FLAG_BLOCK_POSITION if self.cfg.block_position else 0))
        dev = np.ascontiguousarray(devices, np.int32)
        st = C.c_int(0)
        h = self._L.edynhip_world_create(C.byref(cfg), dev.ctypes.data, len(dev), C.byref(st))
        if not h:
            raise EdynHipError(st.value, self._L.edynhip_world_last_error(None).decode())
        self._h = C.c_void_p(h)
        self.num_shards = len(dev)
        self.n = 0
        self.nj = 0

    def close(self):
        if self._h:
            self._L.edynhip_world_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise EdynHipError(rc, self._L.edynhip_world_last_error(self._h).decode())

    def set_scene(self, scene):
        """The whole scene in global indices: meshes, bodies, joints (with their optional-row parameters), cone / cvjoint
        definitions, collision exclusions - what World.set_scene + scenes.apply_figure_settings upload to one context."""
        for mesh in scene.get("meshes") or []:
            v = np.ascontiguousarray(mesh["vertices"], np.float32).reshape(-1, 3)
            idx = np.ascontiguousarray(mesh["indices"], np.uint32); faces = np.ascontiguousarray(mesh["faces"], np.uint32).reshape(-1, 2)
            mid = C.c_uint32(0)
            self._check(self._L.edynhip_world_create_convex_mesh(self._h, len(v), _ptr(v), len(idx), _ptr(idx), len(faces), _ptr(faces), 0, C.byref(mid)))
        n, keep, b = World._body_arrays(None, scene)
        self._check(self._L.edynhip_world_set_bodies(self._h, n, C.byref(b)))
        self.n = n
        self._mat = [keep["friction"].copy(), keep["restitution"].copy()]   # host copy of the materials (edit_bodies: the coefficient not given)
        joints = scene.get("joints") or []
        self.nj = len(joints)
        if joints:
            (jt, jb, jp, ja, jq), js = World._joint_arrays(joints)
            for j, p in scene.get("hinge_params", []):
                jq[j, :len(p)] = p
            self._check(self._L.edynhip_world_set_joints(self._h, len(joints), C.byref(js)))
        for j, fa, fb, p in scene.get("joint_defs", []):
            q = np.zeros(16, np.float32); q[:len(p)] = p
            fa = np.ascontiguousarray(np.asarray(fa, np.float32).reshape(9)); fb = np.ascontiguousarray(np.asarray(fb, np.float32).reshape(9))
            self._check(self._L.edynhip_world_set_joint_definition(self._h, int(j), _ptr(fa), _ptr(fb), _ptr(q), 0))
        for a, bb in scene.get("exclusions", []):
            self._check(self._L.edynhip_world_exclude_collision(self._h, int(a), int(bb)))

    # ---- edits of a running world: what World.add_scene / remove_bodies / add_joints ... do on one context, in global indices
    def add_scene(self, scene):
        """Append the bodies, joints (with `hinge_params`), `joint_defs` and `exclusions` of `scene` - indices relative to the scene - to
        the world, running or not; everybody else's manifolds, impulses, timers and point ids are kept. Returns (first_body, first_joint)."""
        n, keep, b = World._body_arrays(None, scene)
        first = C.c_uint32(0)
        self._check(self._L.edynhip_world_add_bodies(self._h, n, C.byref(b), C.byref(first)))
        self.n += n
        self._mat = [np.concatenate([m, keep[k]]) for m, k in zip(self._mat, ("friction", "restitution"))]
        fb = first.value
        fj = self.nj
        joints = scene.get("joints") or []
        if joints:
            joints = [(j[0], j[1] + fb, j[2] + fb) + tuple(j[3:]) for j in joints]
            fj = self.add_joints(joints, hinge_params=scene.get("hinge_params", []))
        for j, fa, fbm, p in scene.get("joint_defs", []):
            self.set_joint_definition(fj + int(j), fa, fbm, p)
        for a, bb in scene.get("exclusions", []):
            self.exclude_collision(fb + int(a), fb + int(bb))
        return fb, fj

    def remove_bodies(self, indices):
        """registry.destroy(rigid body): the indices stay reserved, the bodies' joints go with them (edynhip_world_remove_bodies)."""
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        self._check(self._L.edynhip_world_remove_bodies(self._h, len(idx), _ptr(idx)))

    def add_joints(self, joints, hinge_params=()):
        """Append joints (World.add_joints' tuples, global body indices; hinge_params: (index in `joints`, params) rows). Returns the first new index."""
        (jt, jb, jp, ja, jq), js = World._joint_arrays(joints)
        for j, p in hinge_params:
            jq[j, :len(p)] = p
        first = C.c_uint32(0)
        self._check(self._L.edynhip_world_add_joints(self._h, len(joints), C.byref(js), C.byref(first)))
        self.nj += len(joints)
        return first.value

    def remove_joints(self, indices):
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        self._check(self._L.edynhip_world_remove_joints(self._h, len(idx), _ptr(idx)))

    def set_joint_params(self, joint, params):
        p = np.zeros(10, np.float32); p[:len(params)] = params
        self._check(self._L.edynhip_world_edit_joint(self._h, int(joint), None, None, _ptr(p), -1))

    def set_joint_definition(self, joint, frameA, frameB, params):
        p = np.zeros(16, np.float32); p[:len(params)] = params
        fa = np.ascontiguousarray(np.asarray(frameA, np.float32).reshape(9)); fb = np.ascontiguousarray(np.asarray(frameB, np.float32).reshape(9))
        self._check(self._L.edynhip_world_edit_joint(self._h, int(joint), _ptr(fa), _ptr(fb), _ptr(p), 0))

    def set_generic_definition(self, joint, frameA, frameB, dofs):
        p = np.ascontiguousarray(np.asarray(dofs, np.float32).reshape(60))
        fa = np.ascontiguousarray(np.asarray(frameA, np.float32).reshape(9)); fb = np.ascontiguousarray(np.asarray(frameB, np.float32).reshape(9))
        self._check(self._L.edynhip_world_edit_joint(self._h, int(joint), _ptr(fa), _ptr(fb), _ptr(p), 1))

    def exclude_collision(self, a, b):
        self._check(self._L.edynhip_world_edit_exclusion(self._h, int(a), int(b), 1))

    def remove_collision_exclusion(self, a, b):
        self._check(self._L.edynhip_world_edit_exclusion(self._h, int(a), int(b), 0))

    def set_state(self, pos, orn, lv, av):
        p = np.ascontiguousarray(pos, np.float32); q = np.ascontiguousarray(orn, np.float32)
        v = np.ascontiguousarray(lv, np.float32); o = np.ascontiguousarray(av, np.float32)
        if (p.size, q.size, v.size, o.size) != (3 * self.n, 4 * self.n, 3 * self.n, 3 * self.n):
            raise ValueError("set_state takes the state of every body of the world")
        self._check(self._L.edynhip_world_set_state(self._h, _ptr(p), _ptr(q), _ptr(v), _ptr(o)))

    def edit_bodies(self, indices, mass=None, inertia=None, friction=None, restitution=None, shape_type=None, shape_param=None,
                    kind=None, gravity=None):
        """World.edit_bodies on the whole world, global indices, in place (edynhip_world_edit_bodies): same arguments, same defaulting -
        of friction and restitution the one not given keeps the value last uploaded. A kind that crosses between dynamic and not
        dynamic rebuilds the shards that gain or lose the body's replica; get_edit_stats() tells the paths apart."""
        idx, a, b, fields = _edit_arrays(self._mat, indices, mass, inertia, friction, restitution, shape_type, shape_param, kind, gravity)
        self._check(self._L.edynhip_world_edit_bodies(self._h, len(idx), _ptr(idx), C.byref(b), fields))
        if fields & _capi.EDIT_MATERIAL:   # (after the call: a refused edit changes nothing)
            self._mat[0][idx] = a["friction"]; self._mat[1][idx] = a["restitution"]

    def wake_bodies(self, indices):
        """World.wake_bodies on the whole world: the islands of these bodies wake (edynhip_world_wake_bodies)."""
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        self._check(self._L.edynhip_world_wake_bodies(self._h, len(idx), _ptr(idx)))

    def get_params(self):
        p = _capi.Params()
        self._check(self._L.edynhip_world_get_params(self._h, C.byref(p)))
        return {"fixed_dt": p.fixed_dt, "velocity_iterations": p.num_velocity_iterations, "position_iterations": p.num_position_iterations,
                "gravity": tuple(p.gravity), "restitution_iterations": p.num_restitution_iterations,
                "individual_restitution_iterations": p.num_individual_restitution_iterations}

    def set_params(self, fixed_dt=None, velocity_iterations=None, position_iterations=None, gravity=None,
                   restitution_iterations=None, individual_restitution_iterations=None):
        """World.set_params on the whole world: no contact state is lost (edynhip_world_set_params)."""
        p = _capi.Params()
        self._check(self._L.edynhip_world_get_params(self._h, C.byref(p)))
        if fixed_dt is not None:
            p.fixed_dt = fixed_dt
        if velocity_iterations is not None:
            p.num_velocity_iterations = velocity_iterations
        if position_iterations is not None:
            p.num_position_iterations = position_iterations
        if gravity is not None:
            p.gravity = (C.c_float * 3)(*[float(x) for x in gravity])
        if restitution_iterations is not None:
            p.num_restitution_iterations = restitution_iterations
        if individual_restitution_iterations is not None:
            p.num_individual_restitution_iterations = individual_restitution_iterations
        self._check(self._L.edynhip_world_set_params(self._h, C.byref(p)))

    def get_asleep(self):
        """World.get_asleep on the whole world: one flag per body, global order (edynhip_world_get_asleep)."""
        out = np.zeros(self.n, np.uint8)
        self._check(self._L.edynhip_world_get_asleep(self._h, _ptr(out)))
        return out

    def get_edit_stats(self):
        """Which path the edits took (edynhip_world_edit_stats): edits, in_place, shard_rebuilds, repartitions_by_edit, approach_checks_by_edit."""
        st = _capi.WorldEditStats()
        self._check(self._L.edynhip_world_get_edit_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _capi.WorldEditStats._fields_}

    def set_should_collide(self, func):
        """edyn::set_should_collide on a world over several devices: func(body, other) -> bool with GLOBAL body indices replaces
        should_collide_default for new manifolds (None restores the device test); edynhip_world_set_pair_filter."""
        self._filter_cb = _capi.PAIR_FILTER(lambda user, a, b: 1 if func(int(a), int(b)) else 0) if func else None
        self._check(self._L.edynhip_world_set_pair_filter(self._h, C.cast(self._filter_cb, C.c_void_p) if func else None, None))

    def default_should_collide(self, a, b):
        return self._L.edynhip_world_default_should_collide(self._h, int(a), int(b)) == 1

    def step_simulation(self, n=1):
        self._check(self._L.edynhip_world_step(self._h, int(n)))

    def get_state(self):
        pos = np.zeros((self.n, 3), np.float32); orn = np.zeros((self.n, 4), np.float32)
        lv = np.zeros((self.n, 3), np.float32); av = np.zeros((self.n, 3), np.float32)
        self._check(self._L.edynhip_world_get_state(self._h, _ptr(pos), _ptr(orn), _ptr(lv), _ptr(av)))
        return pos, orn, lv, av

    def get_partition(self):
        out = np.zeros(self.n, np.int32)
        self._check(self._L.edynhip_world_get_partition(self._h, _ptr(out)))
        return out

    def repartition(self):
        self._check(self._L.edynhip_world_repartition(self._h))

    def get_manifolds(self):
        n = C.c_uint32(0)
        self._check(self._L.edynhip_world_get_manifolds(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), MANIFOLD_DTYPE)
        self._check(self._L.edynhip_world_get_manifolds(self._h, _ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    # ---- materials: World.set_material_extras / .set_material_ids / .insert_material_mixing / .get_point_extras on the whole world
    def set_material_extras(self, first, spin=None, roll=None, stiffness=None, damping=None):
        """material::{spin_friction, roll_friction, stiffness, damping} of bodies [first, first + n), global indices, before the first step
        or on a running world (edynhip_world_set_material_extras). Arrays of equal length; None = the reference's default."""
        arrs = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (spin, roll, stiffness, damping)]
        n = max(len(a) for a in arrs if a is not None)
        self._check(self._L.edynhip_world_set_material_extras(self._h, int(first), n, *[None if a is None else _ptr(a) for a in arrs]))

    def set_material_ids(self, first, ids):
        """material::id of bodies [first, first + len(ids)) (0xFFFF = unassigned): keys into the material mix table."""
        a = np.ascontiguousarray(ids, np.uint32)
        self._check(self._L.edynhip_world_set_material_ids(self._h, int(first), len(a), _ptr(a)))

    def insert_material_mixing(self, id0, id1, restitution=0.0, friction=0.5, spin=0.0, roll=0.0, stiffness=1e18, damping=1e18):
        """edyn::insert_material_mixing on every shard: the material of contact points between bodies with these material ids."""
        m = np.array([restitution, friction, spin, roll, stiffness, damping], np.float32)
        self._check(self._L.edynhip_world_insert_material_mixing(self._h, int(id0), int(id1), _ptr(m)))

    def get_point_extras(self):
        """[num_manifolds, 4, 7]: rolling impulse 0/1, spin impulse, roll mu, spin mu, stiffness, damping (get_manifolds order)."""
        m = C.c_uint32(0)
        self._check(self._L.edynhip_world_get_point_extras(self._h, None, 0, C.byref(m)))
        out = np.zeros((m.value, 4, 7), np.float32)
        if m.value:
            self._check(self._L.edynhip_world_get_point_extras(self._h, _ptr(out), m.value, C.byref(m)))
        return out[:m.value]

    # ---- contact events: World.get_contact_events / .get_point_ids on the whole world (init_config(contact_events=True))
    def get_contact_events(self):
        """Events of the steps of the last step_simulation() call: structured array (type, step, body[2], point_id) as World returns it -
        global body indices, the world's step count, ids that survive re-partitions (edynhip_world_get_contact_events)."""
        n = C.c_uint32(0)
        self._check(self._L.edynhip_world_get_contact_events(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, _capi.EVENT_DTYPE)
        if n.value:
            self._check(self._L.edynhip_world_get_contact_events(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def get_point_ids(self):
        """[num_manifolds, 4] point ids in get_manifolds() order (0 = no point); edynhip_world_get_point_ids."""
        m = C.c_uint32(0)
        self._check(self._L.edynhip_world_get_point_ids(self._h, None, 0, C.byref(m)))
        out = np.zeros((m.value, 4), np.uint64)
        if m.value:
            self._check(self._L.edynhip_world_get_point_ids(self._h, _ptr(out), m.value, C.byref(m)))
        return out[:m.value]

    # ---- record hand-over: World.snapshot_records / .snapshot_map on the whole world (edynhip_world_snapshot_records / _map)
    def snapshot_records(self, present_dt=0.0, max_events=4096):
        """One 96-byte record per body (global order) and the last step call's contact events into one of the world's two pinned slots;
        every shard's device stores its own bodies' records there."""
        self._check(self._L.edynhip_world_snapshot_records(self._h, float(present_dt), int(max_events), 0))

    def snapshot_view(self):
        """The raw edynhip_record_view of the last snapshot (pointers into the pinned slot, valid until the next-but-one snapshot_records)."""
        v = _capi.RecordView()
        self._check(self._L.edynhip_world_snapshot_map(self._h, C.byref(v)))
        return v

    def snapshot_map(self):
        """(records, events, total_events, step_index): structured COPIES of the pinned slot, as World.snapshot_map returns them."""
        v = self.snapshot_view()
        rec = np.ctypeslib.as_array((C.c_uint8 * (v.num_bodies * _capi.RECORD_DTYPE.itemsize)).from_address(v.records)).view(_capi.RECORD_DTYPE).copy() \
            if v.num_bodies else np.zeros(0, _capi.RECORD_DTYPE)
        ev = np.zeros(0, _capi.EVENT_DTYPE)
        if v.events and v.num_events:
            ev = np.ctypeslib.as_array((C.c_uint8 * (v.num_events * _capi.EVENT_DTYPE.itemsize)).from_address(v.events)).view(_capi.EVENT_DTYPE).copy()
        return rec, ev, int(v.total_events), int(v.step_index)

    # ---- queries: World.raycast / World.query_aabb on the whole world, global body indices (edynhip_world_raycast / _query_aabb)
    def raycast(self, p0, p1, ignore=(), brute_force=False):
        """Rays p0[i] -> p1[i] (arrays of shape (n, 3), or one ray of shape (3,)); returns a RAYCAST_HIT_DTYPE array of n records, bit for
        bit what World.raycast returns on one context holding the whole scene. ignore: global body indices left out."""
        a = np.ascontiguousarray(np.asarray(p0, np.float32).reshape(-1, 3))
        b = np.ascontiguousarray(np.asarray(p1, np.float32).reshape(-1, 3))
        if a.shape != b.shape:
            raise ValueError("p0 and p1 must hold the same number of points")
        ign = np.ascontiguousarray(np.asarray(ignore, np.uint32).reshape(-1))
        out = np.zeros(len(a), _capi.RAYCAST_HIT_DTYPE)
        flags = _capi.RAYCAST_BRUTE_FORCE if brute_force else 0
        self._check(self._L.edynhip_world_raycast(self._h, len(a), _ptr(a), _ptr(b), len(ign), _ptr(ign) if len(ign) else None, flags, _ptr(out)))
        return out

    def raycast_device(self, n, p0_ptr, p1_ptr, out_ptr, ignore=(), brute_force=False):
        """Pointers on devices[0]: p0 / p1 hold n float4 (w unused), out receives n 32-byte records. Blocks until the result is complete;
        the inputs must be complete when it is called."""
        ign = np.ascontiguousarray(np.asarray(ignore, np.uint32).reshape(-1))
        flags = _capi.RAYCAST_BRUTE_FORCE if brute_force else 0
        self._check(self._L.edynhip_world_raycast_device(self._h, int(n), C.c_void_p(p0_ptr), C.c_void_p(p1_ptr), len(ign),
                                                         _ptr(ign) if len(ign) else None, flags, C.c_void_p(out_ptr)))

    def query_aabb(self, boxes, category="procedural", brute_force=False):
        """Boxes (n, 6) = (min, max), or one box of shape (6,). Returns (offsets[n + 1], ids) as World.query_aabb does: global body indices
        (island labels for "islands") in ascending order per box."""
        b = np.ascontiguousarray(np.asarray(boxes, np.float32).reshape(-1, 6))
        cat = _capi.QUERY_CATEGORIES[category] if isinstance(category, str) else int(category)
        flags = _capi.QUERY_BRUTE_FORCE if brute_force else 0
        offsets = np.zeros(len(b) + 1, np.uint32)
        total = C.c_uint32(0)
        self._check(self._L.edynhip_world_query_aabb(self._h, cat, len(b), _ptr(b), flags, _ptr(offsets), None, 0, C.byref(total)))
        ids = np.zeros(total.value, np.uint32)
        if total.value:   # (sized by the count: a second call, which cannot run out of capacity)
            self._check(self._L.edynhip_world_query_aabb(self._h, cat, len(b), _ptr(b), flags, _ptr(offsets), _ptr(ids), len(ids), C.byref(total)))
        return offsets, ids

    def query_aabb_device(self, n, boxes_ptr, offsets_ptr, ids_ptr, capacity, total_ptr, category="procedural", brute_force=False):
        """Pointers on devices[0]: boxes hold 2 n float4 (min, max; w unused), offsets n + 1 uint32, ids `capacity` uint32 (0 / None: count
        only), total one uint32. Nothing is written at or beyond `capacity`. Blocks until the result is complete."""
        cat = _capi.QUERY_CATEGORIES[category] if isinstance(category, str) else int(category)
        flags = _capi.QUERY_BRUTE_FORCE if brute_force else 0
        self._check(self._L.edynhip_world_query_aabb_device(self._h, cat, int(n), C.c_void_p(boxes_ptr), flags, C.c_void_p(offsets_ptr),
                                                            C.c_void_p(ids_ptr) if ids_ptr else None, int(capacity), C.c_void_p(total_ptr)))

    def debug_paths(self):
        """World.debug_paths over every shard the world has had, plus "WORLD_SERIAL" (edynhip_world_debug_paths)."""
        mask = C.c_uint64(0)
        self._check(self._L.edynhip_world_debug_paths(self._h, C.byref(mask)))
        return {name for name, bit in _capi.PATH_BITS.items() if mask.value & bit}

    def get_stats(self):
        st = _capi.WorldStats()
        self._check(self._L.edynhip_world_get_stats(self._h, C.byref(st)))
        d = {f: getattr(st, f) for f, _ in _capi.WorldStats._fields_ if f != "bodies_per_shard"}
        d["bodies_per_shard"] = list(st.bodies_per_shard)[:self.num_shards]
        return d
