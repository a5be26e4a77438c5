"""esc_audit_pods at BASELINE config #3's pod side (10 M pods, 100 k nodes, 100 groups, spare
0.02, every pod on a random node, 2 replicas): the time of one pod audit, of each check alone,
REPLICA's achieved bandwidth and, for scale, the same context's decision and its full reload
(pods and placement) in the same run.  Nothing is poked: the snapshot is clean and must be
reported clean, with nothing skipped; the script exits 1 otherwise.

    python scripts/pod_audit_probe.py [--config 3] [--reps 3] [--steps 20]
                                      [--out profiles/r17_pod_audit/probe.json]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

INT64_MIN = np.iinfo(np.int64).min
SPARE = 0.02
SIZES = {4: (100_000_000, 1_000_000, 10_000), 3: (10_000_000, 100_000, 100), 2: (1_000_000, 10_000, 100)}
REPLICAS = 2


def clean(rep):
    return not rep["skipped"] and all(v["n_bad"] == 0 for k, v in rep.items() if k != "skipped")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import escalator_amd as esc
    from escalator_amd import _lib as L
    P, N, G = SIZES[args.config]
    t0 = time.perf_counter()
    s = esc.Synth(P, N, G, config=args.config, seed=0xE5CA1A7E00000000 + args.config, threads=16)
    pods, nodes = s.pods(), s.nodes()
    ctx = esc.Context(s)
    ctx.set_spare(SPARE)
    rng = np.random.default_rng(37)
    pod_node = rng.integers(0, N, size=P, dtype=np.uint32)
    tainted = (nodes["flags"] & 2) != 0
    taint_s = np.where(tainted, 1_800_000_000 - rng.integers(0, 1200, size=N), INT64_MIN).astype(np.int64)
    no_delete = np.zeros(N, np.uint8)

    def load():
        ctx.load(pods, nodes, replicas=REPLICAS)
        ctx.load_placement(pod_node, taint_s, no_delete)
    load()
    ctx.set_state(s.states)
    ctx.use_graph(True)
    for _ in range(3):
        ctx.run()
    ctx.sync()
    setup_s = time.perf_counter() - t0
    print("setup %.1f s" % setup_s, flush=True)

    def timed(checks=None):
        ms = []
        for _ in range(args.reps):
            t = time.perf_counter()
            rep = ctx.audit_pods(checks)
            ms.append((time.perf_counter() - t) * 1e3)
        return min(ms), rep

    first_t = time.perf_counter()
    first = ctx.audit_pods()                                   # the first call also makes the staging buffer
    first_ms = (time.perf_counter() - first_t) * 1e3
    all_ms, rep = timed()
    print("all %.2f ms" % all_ms, json.dumps(rep), flush=True)
    per_check = {}
    for name in L.POD_AUDIT_CHECKS:
        per_check[name], _ = timed([name])
        print(name, "%.2f ms" % per_check[name], flush=True)
    t = time.perf_counter()
    for _ in range(args.steps):
        ctx.run()
    ctx.sync()
    decision_ms = (time.perf_counter() - t) / args.steps * 1e3
    after = ctx.audit_pods()
    t = time.perf_counter()
    load()
    reload_ms = (time.perf_counter() - t) * 1e3
    room = ctx.pods_room()
    pod_bytes, _ = ctx.stream_bytes()
    elems = rep["REPLICA"]["n_checked"]
    c_slots = rep["CSLOT"]["n_checked"]
    ok = clean(first) and clean(rep) and clean(after)
    out = {
        "metric": "esc_audit_pods on one context beside its decision and its reload",
        "config": {"pods": P, "nodes": N, "node_groups": G, "spare": SPARE, "replicas": REPLICAS, "synth_config": args.config,
                   "k_capacity": int(room["k_capacity"]), "c_slots": c_slots},
        "ms_first_call": first_ms, "ms_audit_all_checks": all_ms, "ms_per_check": per_check,
        "ms_per_decision": decision_ms, "ms_full_reload": reload_ms,
        "audit_over_decision": all_ms / decision_ms, "reload_over_audit": reload_ms / all_ms,
        "slowest_check": max(per_check, key=per_check.get),
        "replica_elements": elems, "k1_stream_bytes_per_decision": int(pod_bytes),
        "reps": args.reps, "steps": args.steps, "setup_s": setup_s,
        "n_checked": {k: v["n_checked"] for k, v in rep.items() if k != "skipped"},
        "clean": ok,
        "data": "synthetic (esc_synth.cpp config %d; every pod on a random node)" % args.config,
    }
    lib = ctx.lib
    if hasattr(lib, "esc_debug_pod_audit_bytes"):              # measurement library: the bytes REPLICA compared
        import ctypes as C
        lib.esc_debug_pod_audit_bytes.restype = C.c_int64
        b = int(lib.esc_debug_pod_audit_bytes())
        out["replica_bytes_read"] = 2 * b                      # every compared byte, from both replicas
        out["replica_gb_per_s_of_call"] = 2 * b / (per_check["REPLICA"] * 1e-3) / 1e9    # over the whole call's wall time
        lib.esc_debug_pod_audit_replica_ms.restype = C.c_double
        k_ms = []
        for _ in range(args.reps):                             # events around the compare launches alone
            ctx.audit_pods(["REPLICA"])
            k_ms.append(float(lib.esc_debug_pod_audit_replica_ms()))
        out["replica_launches_ms"] = min(k_ms)
        out["replica_gb_per_s_of_launches"] = 2 * b / (min(k_ms) * 1e-3) / 1e9
    if not ok:
        out["reports"] = {"first": first, "timed": rep, "after_decisions": after}
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
