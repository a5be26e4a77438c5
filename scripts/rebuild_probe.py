"""esc_nodes_rebuild beside what it replaces, at BASELINE config #4's node side (1 M nodes,
10 k groups) and config #5's (10 M nodes), a placement loaded: per call, best of --reps, in one
run on one context

  - esc_nodes_rebuild, split into host layout, upload, list + sort + place, mirror download
    (with allNodes[0]), occupancy recount and age-index build (the split comes from the
    measurement library, ESC_LIB_PATH = escalator_amd/libescalator_hip_measure.so; on the
    product library only the total is reported),
  - esc_load_nodes of the same table,
  - the full reload (esc_load_pods + esc_load_nodes + esc_load_placement) at --pods pods.

    python scripts/rebuild_probe.py [--pods 2000000] [--reps 3] [--configs 4,5]
                                    [--out profiles/r10_rebuild/probe.json]

The audit of the rebuilt state (ENTRY, FIRST, REGION, OCC, TRACKER) must be clean after the
last rebuild; the script exits 1 otherwise.  Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

INT64_MIN = np.iinfo(np.int64).min
SPARE = 0.02
SIZES = {4: (1_000_000, 10_000), 5: (10_000_000, 10_000)}
SPLIT = ["host_layout", "upload", "list_sort_place", "mirror_download", "occupancy_recount", "age_index"]
REBUILT = ["ENTRY", "FIRST", "REGION", "OCC", "TRACKER"]


def best(fn, reps):
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return min(ms)


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
    # some churn first, so that the rebuild has holes to close: deletes and relabel-free updates
    gone = np.sort(rng.choice(n_nodes, 2000, replace=False)).astype(np.int64)
    ctx.nodes_delete(gone)
    out = {"nodes": n_nodes, "node_groups": n_groups, "pods": pods, "spare": SPARE}
    split = None
    total = []
    for _ in range(reps):
        t = time.perf_counter()
        ctx.nodes_rebuild()
        total.append((time.perf_counter() - t) * 1e3)
        if hasattr(lib, "esc_debug_rebuild_times"):
            ms = (C.c_double * len(SPLIT))()
            lib.esc_debug_rebuild_times(ms, len(SPLIT))
            if split is None or total[-1] == min(total):
                split = dict(zip(SPLIT, [float(x) for x in ms]))
    out["ms_nodes_rebuild"] = min(total)
    out["ms_nodes_rebuild_split"] = split
    rep = ctx.audit(REBUILT)
    out["clean"] = not rep["skipped"] and all(rep[k]["n_bad"] == 0 for k in REBUILT)
    out["entry_incidences"] = rep["ENTRY"]["n_checked"]
    ctx.run()
    ctx.sync()

    def reload():
        ctx.load(P, N)
        ctx.load_placement(pod_node, taint_s, no_delete)

    out["ms_full_reload"] = best(reload, reps)
    out["ms_load_nodes"] = best(lambda: ctx.load_nodes(N), reps)
    out["rebuild_over_load_nodes"] = out["ms_nodes_rebuild"] / out["ms_load_nodes"]
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
    if hasattr(lib, "esc_debug_rebuild_times"):
        lib.esc_debug_rebuild_times.argtypes = [C.POINTER(C.c_double), C.c_int32]
        lib.esc_debug_rebuild_times.restype = C.c_int32
    res = {"metric": "esc_nodes_rebuild beside esc_load_nodes and the full reload, one context, best of reps",
           "library": os.path.basename(L.LIB_PATH), "reps": args.reps, "configs": {},
           "data": "synthetic (esc_synth.cpp; every pod on a random node; 2 000 nodes deleted before the rebuilds)"}
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
