"""esc_nodes_verify beside what it replaces, at BASELINE config #4's node side (1 M nodes, 10 k
groups) and config #5's (10 M nodes), a placement loaded: per call, best of --reps, on one context

  - esc_nodes_verify of the whole store in one call, with the three fact arrays: the Python
    binding's call (it builds the SoA struct) and the C call alone, timed by the host clock;
  - one changed node per call (its cpu), at the batch's first, middle and last index: found alone;
  - esc_nodes_rebuild on the same context;
  - esc_load_nodes + esc_load_placement of the same table, and esc_load_nodes alone.

    python scripts/nodes_verify_probe.py [--pods 2000000] [--reps 3] [--configs 4,5] [--verify-only]
                                         [--out profiles/r20_node_verify/probe.json]

The snapshot is clean and must be reported clean; the script exits 1 otherwise.  --verify-only runs
the verify calls alone (for a kernel trace of its own: rocprofv3 --kernel-trace --stats -- python
scripts/nodes_verify_probe.py --verify-only; no counters are mixed with tracing).  "staged_bytes"
is computed (65 B per node and 4 B per extra label word, what one call copies to the device and
back), not measured.  Prints one JSON line (and writes it to --out)."""
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
SIZES = {4: (1_000_000, 10_000), 5: (10_000_000, 10_000), 2: (10_000, 100)}


def best(fn, reps):
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return min(ms)


def probe(esc, L, config, pods, reps, verify_only):
    from escalator_amd.context import node_soa
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
    no_delete = (rng.integers(0, 50, size=n_nodes) == 0).astype(np.uint8)
    ctx.load_placement(pod_node, taint_s, no_delete)
    inst = np.where(rng.integers(0, 4, size=n_nodes) == 0, 1_700_000_000 * 10**9 - rng.integers(0, 10**12, size=n_nodes),
                    INT64_MIN).astype(np.int64)
    known = np.flatnonzero(inst != INT64_MIN).astype(np.int64)
    ctx.nodes_instantiated(known, inst[known])
    ctx.set_state(s.states)
    ctx.run()
    ctx.sync()
    ids = np.arange(n_nodes, dtype=np.int64)
    V = {k: N[k] for k in ("flags", "label0", "cpu", "mem", "created_ns", "xl_pair")}
    V["flags"] = N["flags"] & ~np.uint32(4)                    # (the tracker is the context's; n_trk = 0 in a batch)
    V["trk_node"], V["trk_group"] = np.zeros(0, np.int32), np.zeros(0, np.int32)
    out = {"nodes": n_nodes, "node_groups": n_groups, "pods": pods, "spare": SPARE, "xl_words": int(len(V["xl_pair"])),
           "staged_bytes": int(65 * n_nodes + 4 * len(V["xl_pair"]))}
    bad = []

    def whole():
        st, r = ctx.nodes_verify(ids, V, taint_s, no_delete, inst)
        bad.append(int(np.count_nonzero(st)) + (r["first_bad"] != -1) + (r["n_checked"] != n_nodes))
    whole()                                                    # the first call also makes the staging buffer
    out["ms_verify_binding"] = best(whole, reps)
    ns, keep = node_soa(V)
    status = np.zeros(n_nodes, np.uint8)
    rep = L.NodesVerifyReport()
    p64, p8 = C.POINTER(C.c_int64), C.POINTER(C.c_uint8)

    def c_call(stat=status):
        rc = ctx.lib.esc_nodes_verify(ctx.handle, ids.ctypes.data_as(p64), C.byref(ns), taint_s.ctypes.data_as(p64),
                                      no_delete.ctypes.data_as(p8), inst.ctypes.data_as(p64),
                                      None if stat is None else stat.ctypes.data_as(p8), C.byref(rep))
        bad.append(int(rc != 0) + int(rep.first_bad != -1))
    out["ms_verify"] = best(c_call, reps)
    out["ms_verify_no_status_out"] = best(lambda: c_call(None), reps)
    out["verify_nodes_per_s"] = n_nodes / (out["ms_verify"] * 1e-3)
    out["staged_gb_per_s"] = out["staged_bytes"] / (out["ms_verify"] * 1e-3) / 1e9
    del keep
    found = 0
    for k in (0, n_nodes // 2, n_nodes - 1):                   # one changed node per call, found alone
        Q = dict(V, cpu=V["cpu"].copy())
        Q["cpu"][k] += 1
        st, r = ctx.nodes_verify(ids, Q, taint_s, no_delete, inst)
        found += int(np.count_nonzero(st)) == 1 and int(st[k]) == L.NV_STATUS and r["first_bad"] == k and r["n_status"] == 1
    out["changed_nodes_found"] = found
    out["clean"] = not any(bad) and found == 3
    if not verify_only:
        out["ms_nodes_rebuild"] = best(ctx.nodes_rebuild, reps)
        whole()
        out["clean"] = out["clean"] and not bad[-1]            # the same answer after a rebuild

        def reload_nodes():
            ctx.load_nodes(N)
            ctx.load_placement(pod_node, taint_s, no_delete)
        out["ms_load_nodes_and_placement"] = best(reload_nodes, reps)
        out["ms_load_nodes"] = best(lambda: ctx.load_nodes(N), reps)
        out["load_over_verify"] = out["ms_load_nodes_and_placement"] / out["ms_verify"]
        out["rebuild_over_verify"] = out["ms_nodes_rebuild"] / out["ms_verify"]
    ctx.close()
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="4,5")
    ap.add_argument("--verify-only", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import escalator_amd as esc
    from escalator_amd import _lib as L
    L.load()
    res = {"metric": "esc_nodes_verify of the whole store in one call beside esc_nodes_rebuild and esc_load_nodes + "
                     "esc_load_placement, one context, host clock, best of reps",
           "library": os.path.basename(L.LIB_PATH), "reps": args.reps, "verify_only": bool(args.verify_only), "configs": {},
           "data": "synthetic (esc_synth.cpp; every pod on a random node; a quarter of the nodes with an instantiation time)"}
    ok = True
    for c in [int(x) for x in args.configs.split(",")]:
        r = probe(esc, L, c, args.pods, args.reps, args.verify_only)
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
