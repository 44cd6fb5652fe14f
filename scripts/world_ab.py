"""Does a multi-device world decide the same with two builds of the library? The bit-equality tests cannot see a partition decision that
changed (physics does not depend on the partition), so this one-off tool runs a few small scenarios once per build - each build in a
fresh child process, selected by EDYNHIP_LIB - and compares, after every step and every edit, bit for bit: get_partition, get_state,
get_manifolds, get_asleep, edynhip_world_stats and edynhip_world_edit_stats. It first runs the parent's build against itself: what that
run does not hold steady is left out of the comparison, and said so.
usage: python scripts/world_ab.py <parent libedynhip.so> [<this tree's libedynhip.so>] [--out profiles/<name>_ab.json]"""
import hashlib, json, os, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("partition", "state", "manifolds", "asleep", "stats", "edit_stats")
DEVICE_LISTS = ([0, 0], [0, 0, 0])


# ---------------------------------------------------------------------------------------------------------------- child: one build
def child(out_path):
    sys.path.insert(0, ROOT)
    import numpy as np
    import edyn_amd
    from edyn_amd import scenes
    from edyn_amd.multi import MultiWorld

    log = []

    def bodies(rows):
        s = scenes._empty(len(rows))
        for i, r in enumerate(rows):
            s["kind"][i] = r.get("kind", scenes.KIND_DYNAMIC)
            s["pos"][i] = r["pos"]; s["linvel"][i] = r.get("linvel", (0, 0, 0))
            s["shape_type"][i] = r["shape"]; s["shape_param"][i, :len(r["param"])] = r["param"]
        return s

    class Run:
        def __init__(self, name, devices, scene):
            self.name, self.devices = name, devices
            self.mw = MultiWorld(edyn_amd.init_config(num_solver_velocity_iterations=10, sleeping=True), devices=devices)
            self.mw.set_scene(scene)

        def mark(self, tag):
            mw = self.mw
            sha = lambda *arrays: hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()
            stats, edits = mw.get_stats(), mw.get_edit_stats()
            log.append({"scenario": self.name, "devices": self.devices, "tag": tag, "partition": sha(mw.get_partition()), "state": sha(*mw.get_state()),
                        "manifolds": sha(mw.get_manifolds()), "asleep": sha(mw.get_asleep()), "stats": stats, "edit_stats": edits})

        def step(self, k, tag):
            for i in range(k):
                self.mw.step_simulation(1)
                self.mark(f"{tag} step {i + 1}")

    def site(sx, sz, nx, nz):
        return np.array([(sx - (nx - 1) / 2.0) * 8.0, 0.0, (sz - (nz - 1) / 2.0) * 8.0], np.float32)

    def slider(scene, centre, direction):
        """A box on the ground 1 cm beside the pile at `centre` (inside the creation margin: one island with it), sliding along x."""
        edge = centre[0] + direction * (2.53 if direction > 0 else 2.03)
        box = bodies([dict(pos=(edge + direction * 0.51, 0.505, centre[2]), linvel=(direction * 8.0, 0, 0), shape=scenes.SHAPE_BOX, param=(0.5, 0.5, 0.5))])
        box["friction"][:] = 0.5
        return scenes.merge(scene, box)

    for devices in DEVICE_LISTS:
        W = len(devices)
        # 1. nine piles, a body slides from one into its neighbour on another shard: an approach-triggered sticky re-partition
        # (the slider leaves its pile and is an island of its own when it arrives: the first start from which the partition puts it on
        # another shard than the pile it runs into)
        pick = (0, 0, 1)
        for cand in [(sx, sz, d) for sz in range(3) for sx in range(3) for d in (1, -1) if 0 <= sx + d < 3]:
            probe = MultiWorld(edyn_amd.init_config(num_solver_velocity_iterations=10), devices=devices)
            probe.set_scene(slider(scenes.mini_piles(3, 3), site(cand[0], cand[1], 3, 3), cand[2]))
            part = probe.get_partition(); probe.close()
            if part[-1] != part[1 + 64 * (cand[1] * 3 + cand[0] + cand[2])]:
                pick = cand
                break
        r = Run("slide", devices, slider(scenes.mini_piles(3, 3), site(pick[0], pick[1], 3, 3), pick[2]))
        r.mark(f"built, slider at site {pick[:2]} heading {pick[2]:+d}")
        r.step(90, "slide")
        # 2. a forced re-partition, twice
        r = Run("forced", devices, scenes.mini_piles(2, 1))
        r.step(30, "settle"); r.mw.repartition(); r.mark("repartition 1")
        r.step(30, "between"); r.mw.repartition(); r.mark("repartition 2")
        r.step(10, "after")
        # 3. the edits of tests/test_world_edits.py: spawn in place, spawn beyond capacity, a joint across two shards, remove, set_state
        r = Run("edits", devices, scenes.mini_piles(2, 1))
        r.step(20, "settle")
        n0 = r.mw.n
        s0, s1 = site(0, 0, 2, 1), site(1, 0, 2, 1)
        r.mw.add_scene(bodies([dict(pos=(s0[0], 0.505 + 3 * 1.005 + 2.0, s0[2]), shape=scenes.SHAPE_BOX, param=(0.5, 0.5, 0.5)),
                               dict(pos=(0.0, 1.0, 40.0), shape=scenes.SHAPE_SPHERE, param=(0.5,)),
                               dict(kind=scenes.KIND_STATIC, pos=(s1[0] + 2.05 + 0.5, 0.5, s1[2]), shape=scenes.SHAPE_BOX, param=(0.5, 0.5, 0.5))]))
        r.mark("spawn in place"); r.step(10, "after the spawn")
        n1 = r.mw.n
        r.mw.add_scene(bodies([dict(pos=(-19.0 + 2.0 * (k % 20), 0.3, 30.0 + 2.0 * (k // 20)), shape=scenes.SHAPE_SPHERE, param=(0.25,)) for k in range(400)]))
        r.mark("spawn beyond capacity"); r.step(10, "after the grid")
        part, pos = r.mw.get_partition(), r.mw.get_state()[0]
        a = n1
        b = next((n1 + k for k in range(1, 400) if part[n1 + k] != part[a]), n1 + 1)
        d = pos[a] - pos[b]
        r.mw.add_joints([(scenes.JOINT_POINT, int(a), int(b), (0.0, 0.0, 0.0), (float(d[0]), float(d[1]), float(d[2])), (0.0, 0.0, 1.0), (0.0, 0.0, 1.0))])
        r.mark(f"joint {a}-{b}"); r.step(10, "after the joint")
        r.mw.remove_bodies([5, n0 + 1, n1 + 7])
        r.mark("remove"); r.step(10, "after the removal")
        pos, orn, lv, av = r.mw.get_state()
        pos[n1 + 30, 1] += 1.0; pos[70] += (0.0, 3.0, 0.0)
        r.mw.set_state(pos, orn, lv, av)
        r.mark("set_state"); r.step(10, "after set_state")
        # 4. 8 W boxes on a floor: a row of 12 at x = 0 (shard 0 by the curve along x), a lone box 3 m beside it on another shard, rows of the
        # rest further out. The lone box slides into the row: its group of 13 goes to shard 0, which then holds more than 1.5 x the mean
        # (13 W > 12 W) of 8 W bodies - the sticky move is given up for the full, balanced re-partition (stats: rebalances = 1)
        row = lambda x, m: [dict(pos=(x, 0.505, (k - (m - 1) / 2.0) * 1.01), shape=scenes.SHAPE_BOX, param=(0.5, 0.5, 0.5)) for k in range(m)]
        rest = 8 * W - 13
        rows = [dict(kind=scenes.KIND_STATIC, pos=(0, 0, 0), shape=scenes.SHAPE_PLANE, param=(0, 1, 0, 0))] + row(0.0, 12)
        rows += [dict(pos=(4.0, 0.505, 0.0), linvel=(-8.0, 0, 0), shape=scenes.SHAPE_BOX, param=(0.5, 0.5, 0.5))]
        for q in range(W - 1):
            rows += row(20.0 * (q + 1), rest // (W - 1) + (1 if q < rest % (W - 1) else 0))
        r = Run("rebalance", devices, bodies(rows))
        r.mark("built"); r.step(90, "slide")
    json.dump(log, open(out_path, "w"))


# ---------------------------------------------------------------------------------------------------------------- parent: compare
def run(lib, path):
    env = dict(os.environ, EDYNHIP_LIB=os.path.abspath(lib))
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env, check=True, timeout=900)
    return json.load(open(path))


def compare(a, b, fields):
    """per scenario and device list: checkpoints, and per field how many differ and where first"""
    out = {}
    if [(x["scenario"], x["devices"], x["tag"]) for x in a] != [(x["scenario"], x["devices"], x["tag"]) for x in b]:
        return {"checkpoints": "the two runs took different checkpoints", "differences": -1}
    total = 0
    for x, y in zip(a, b):
        row = out.setdefault(f'{x["scenario"]} {x["devices"]}', {"checkpoints": 0, "differing": {}})
        row["checkpoints"] += 1
        for f in fields:
            if x[f] != y[f]:
                total += 1
                d = row["differing"].setdefault(f, {"count": 0, "first": x["tag"]})
                d["count"] += 1
    out["differences"] = total
    return out


def main():
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        return child(args[1])
    out_path = os.path.join(ROOT, "profiles", "world_ab.json")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
        del args[args.index("--out"):args.index("--out") + 2]
    parent = args[0]
    mine = args[1] if len(args) > 1 else os.path.join(ROOT, "edyn_amd", "libedynhip.so")
    with tempfile.TemporaryDirectory() as tmp:
        p1, p2, m = (run(lib, os.path.join(tmp, name)) for lib, name in ((parent, "p1.json"), (parent, "p2.json"), (mine, "m.json")))
    steady = compare(p1, p2, FIELDS)
    unsteady = sorted({f for row in steady.values() if isinstance(row, dict) for f in row.get("differing", {})})
    held = [f for f in FIELDS if f not in unsteady]
    result = {"what": "scripts/world_ab.py: a multi-device world under two builds of the library, compared bit for bit after every step and edit",
              "fields": list(FIELDS), "parent_against_parent": steady, "not_steady_left_out": unsteady,
              "parent_against_this_tree": compare(p1, m, held),
              "final_stats": {f'{x["scenario"]} {x["devices"]}': {"parent": x["stats"], "this_tree": y["stats"], "parent_edits": x["edit_stats"], "this_tree_edits": y["edit_stats"]}
                              for x, y in zip(p1, m)}}
    json.dump(result, open(out_path, "w"), indent=1)
    print(json.dumps({k: result[k] for k in ("parent_against_parent", "not_steady_left_out", "parent_against_this_tree")}, indent=1))
    return 1 if result["parent_against_this_tree"]["differences"] else 0


if __name__ == "__main__":
    sys.exit(main())
