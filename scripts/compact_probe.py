"""esc_nodes_compact beside esc_nodes_rebuild and the full reload, at BASELINE config #4's node
side (1 M nodes, 10 k groups) and config #5's (10 M nodes), a placement loaded with every pod on a
random node: per call, best of --reps, in one run on one context.  Before every repetition 2 000
live nodes are deleted, so that every compaction closes 2 000 holes and unbinds their pods.

  - esc_nodes_compact, split into host plan, buffers and upload, gather + run move (to the
    wait), host mirror remap (the O(pods) pass over the pods' node and run position included)
    and the rebuild part (esc_nodes_rebuild's own six parts, summed and listed); the split
    comes from the measurement library (ESC_LIB_PATH =
    escalator_amd/libescalator_hip_measure.so), on the product library only totals are reported,
  - esc_nodes_rebuild of the same table (holes and all), right before each compaction,
  - the full reload (esc_load_pods + esc_load_nodes + esc_load_placement) at --pods pods.

    python scripts/compact_probe.py [--pods 2000000] [--reps 3] [--configs 4,5]
                                    [--out profiles/r11_compact/probe.json]

The audit must be clean after the last compaction and the free slots what the capacity rule
says; the script exits 1 otherwise.  Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

INT64_MIN = np.iinfo(np.int64).min
SPARE = 0.02
SIZES = {4: (1_000_000, 10_000), 5: (10_000_000, 10_000)}
SPLIT = ["host_plan", "buffers_upload", "gather_run_move", "host_mirror_remap", "pod_remap_alone"]
REBUILD_SPLIT = ["host_layout", "upload", "list_sort_place", "mirror_download", "occupancy_recount", "age_index"]
CHECKS = ["ENTRY", "FIRST", "REGION", "OCC", "TRACKER", "MIRROR"]


def times(lib, name, n):
    if not hasattr(lib, name):
        return None
    ms = (C.c_double * n)()
    getattr(lib, name)(ms, n)
    return [float(x) for x in ms]


def probe(esc, lib, config, pods, reps):
    n_nodes, n_groups = SIZES[config]
    s = esc.Synth(pods, n_nodes, n_groups, config=config, seed=0xE5CA1A7E00000000 + config, threads=16)
    P, N = s.pods(), s.nodes()
    ctx = esc.Context(s)
    ctx.set_spare(SPARE)
    ctx.load(P, N)
    rng = np.random.default_rng(31)
    pod_node = rng.integers(0, n_nodes, size=pods, dtype=np.uint32)
    tainted = (N["flags"] & 2) != 0
    taint_s = np.where(tainted, 1_800_000_000 - rng.integers(0, 1200, size=n_nodes), INT64_MIN).astype(np.int64)
    no_delete = np.zeros(n_nodes, np.uint8)
    ctx.load_placement(pod_node, taint_s, no_delete)
    ctx.set_state(s.states)
    ctx.run()
    ctx.sync()
    out = {"nodes": n_nodes, "node_groups": n_groups, "pods": pods, "spare": SPARE, "deleted_per_rep": 2000}
    live = n_nodes
    best = None
    rebuilds = []
    for _ in range(reps):
        ctx.nodes_delete(np.sort(rng.choice(live, 2000, replace=False)).astype(np.int64))
        t = time.perf_counter()
        ctx.nodes_rebuild()
        rebuilds.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        m = ctx.nodes_compact()
        ms = (time.perf_counter() - t) * 1e3
        live -= 2000
        assert len(m) == live + 2000 and int((m < 0).sum()) == 2000 and int(m.max()) == live - 1
        if best is None or ms < best[0]:
            best = (ms, times(lib, "esc_debug_compact_times", len(SPLIT)), times(lib, "esc_debug_rebuild_times", len(REBUILD_SPLIT)))
    out["ms_nodes_compact"] = best[0]
    if best[1] is not None:
        out["ms_nodes_compact_split"] = dict(zip(SPLIT[:4], best[1]), rebuild_part=sum(best[2]))
        out["ms_pod_remap_alone"] = best[1][4]                 # part of host_mirror_remap: O(pods)
        out["ms_rebuild_part_split"] = dict(zip(REBUILD_SPLIT, best[2]))
    out["ms_nodes_rebuild"] = min(rebuilds)
    rep = ctx.audit(CHECKS)
    out["clean"] = not rep["skipped"] and all(rep[k]["n_bad"] == 0 for k in CHECKS) and \
        ctx.nodes_room()[0] == int(math.ceil(live * SPARE)) + 64
    ctx.run()
    ctx.sync()

    def reload():
        ctx.load(P, N)
        ctx.load_placement(pod_node, taint_s, no_delete)

    t = []
    for _ in range(reps):
        a = time.perf_counter()
        reload()
        t.append((time.perf_counter() - a) * 1e3)
    out["ms_full_reload"] = min(t)
    out["compact_over_rebuild"] = out["ms_nodes_compact"] / out["ms_nodes_rebuild"]
    out["compact_over_full_reload"] = out["ms_nodes_compact"] / out["ms_full_reload"]
    ctx.close()
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="4,5")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import escalator_amd as esc
    from escalator_amd import _lib as L
    lib = L.load()
    for name in ("esc_debug_rebuild_times", "esc_debug_compact_times"):
        if hasattr(lib, name):
            getattr(lib, name).argtypes = [C.POINTER(C.c_double), C.c_int32]
            getattr(lib, name).restype = C.c_int32
    res = {"metric": "esc_nodes_compact beside esc_nodes_rebuild and the full reload, one context, best of reps",
           "library": os.path.basename(L.LIB_PATH), "reps": args.reps, "configs": {},
           "data": "synthetic (esc_synth.cpp; every pod on a random node; 2 000 live nodes deleted before every repetition)"}
    ok = True
    for c in [int(x) for x in args.configs.split(",")]:
        r = probe(esc, lib, c, args.pods, args.reps)
        print("config %d" % c, json.dumps(r), flush=True)
        res["configs"][str(c)] = r
        ok = ok and r["clean"]
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
