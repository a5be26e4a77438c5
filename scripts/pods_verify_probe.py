"""esc_pods_verify at BASELINE config #3's pod side (10 M pods, 100 groups, spare 0.02, 2
replicas): the whole store compared with the resident pods in calls of --batch pods (1 M), and
beside it, interleaved on the same context, the two things it replaces: esc_pods_upsert of the
same batches (every pod rewritten with the values it has) and, at the end, the full reload.  No
placement is loaded (bindings are not compared: BIND is a host-side compare of two mirrors).  The
snapshot is clean and must be reported clean; the script exits 1 otherwise.

    python scripts/pods_verify_probe.py [--config 3] [--batch 1000000] [--reps 2] [--verify-only]
                                        [--out profiles/r18_pod_verify/probe.json]

--verify-only runs the verify passes alone (for a kernel trace of its own: rocprofv3
--kernel-trace --stats -- python scripts/pods_verify_probe.py --verify-only; no counters are mixed
with tracing).  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SPARE = 0.02
SIZES = {4: (100_000_000, 1_000_000, 10_000), 3: (10_000_000, 100_000, 100), 2: (1_000_000, 10_000, 100)}
REPLICAS = 2


def batches(pods, size):
    """The packed store cut into batches of `size` pods: (ids, SoA views)."""
    f = pods["flags"].astype(np.uint64)
    nrec = (((f >> 8) & 0xFF) + ((f >> 16) & 0xFF) + ((f >> 4) & 1)).astype(np.int64)
    nxp = ((f >> 24) & 0x3F).astype(np.int64)
    ro, po = np.r_[0, np.cumsum(nrec)], np.r_[0, np.cumsum(nxp)]
    n = len(f)
    for a in range(0, n, size):
        b = min(n, a + size)
        yield np.arange(a, b, dtype=np.int64), {
            "flags": pods["flags"][a:b], "cpu0": pods["cpu0"][a:b], "mem0": pods["mem0"][a:b], "pair0": pods["pair0"][a:b],
            "xc_cpu": pods["xc_cpu"][ro[a]:ro[b]], "xc_mem": pods["xc_mem"][ro[a]:ro[b]], "xp_pair": pods["xp_pair"][po[a]:po[b]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--verify-only", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import escalator_amd as esc
    P, N, G = SIZES[args.config]
    t0 = time.perf_counter()
    s = esc.Synth(P, N, G, config=args.config, seed=0xE5CA1A7E00000000 + args.config, threads=16)
    pods, nodes = s.pods(), s.nodes()
    ctx = esc.Context(s)
    ctx.set_spare(SPARE)
    ctx.load(pods, nodes, replicas=REPLICAS)
    setup_s = time.perf_counter() - t0
    print("setup %.1f s" % setup_s, flush=True)
    cut = list(batches(pods, args.batch))
    ctx.pods_verify(*cut[0])                                   # the first call also makes the staging buffer
    verify_ms, upsert_ms, bad = [], [], 0
    for rep in range(args.reps):
        v = u = 0.0
        for ids, B in cut:                                     # interleaved: a verify, then the upsert of the same batch
            t = time.perf_counter()
            st, r = ctx.pods_verify(ids, B)
            v += time.perf_counter() - t
            bad += int(np.count_nonzero(st)) + (r["first_bad"] != -1)
            if not args.verify_only:
                t = time.perf_counter()
                rc = ctx.pods_upsert(ids, B)
                u += time.perf_counter() - t
                bad += rc != 0
        verify_ms.append(v * 1e3)
        upsert_ms.append(u * 1e3)
        print("pass %d: verify %.1f ms, upsert %.1f ms" % (rep, v * 1e3, u * 1e3), flush=True)
    # a changed pod per batch is found, and only it
    found = 0
    for ids, B in cut:
        Q = dict(B, cpu0=B["cpu0"].copy())
        Q["cpu0"][len(ids) // 2] += 1
        st, r = ctx.pods_verify(ids, Q)
        found += int(np.count_nonzero(st)) == 1 and st[len(ids) // 2] in (2, 4) and r["first_bad"] == len(ids) // 2
    reload_ms = 0.0
    if not args.verify_only:
        t = time.perf_counter()
        ctx.load(pods, nodes, replicas=REPLICAS)
        reload_ms = (time.perf_counter() - t) * 1e3
    ok = bad == 0 and found == len(cut)
    vm = min(verify_ms)
    out = {
        "metric": "esc_pods_verify of the whole store beside esc_pods_upsert of the same batches and the full reload",
        "config": {"pods": P, "nodes": N, "node_groups": G, "spare": SPARE, "replicas": REPLICAS, "synth_config": args.config,
                   "batch": args.batch, "calls": len(cut)},
        "ms_verify_whole_store": vm, "verify_pods_per_s": P / (vm * 1e-3),
        "ms_upsert_whole_store": min(upsert_ms), "upsert_pods_per_s": P / (min(upsert_ms) * 1e-3) if min(upsert_ms) else None,
        "ms_full_reload": reload_ms,
        "upsert_over_verify": min(upsert_ms) / vm, "reload_over_verify": reload_ms / vm,
        "ms_verify_passes": verify_ms, "ms_upsert_passes": upsert_ms,
        "changed_pods_found": found, "reps": args.reps, "setup_s": setup_s, "verify_only": bool(args.verify_only), "clean": ok,
        "data": "synthetic (esc_synth.cpp config %d; no placement)" % args.config,
    }
    ctx.close()
    s.close()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
