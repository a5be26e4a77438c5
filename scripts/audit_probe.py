"""esc_audit at BASELINE config #4's sizes (100 M pods, 1 M nodes, 10 k groups), a placement
loaded and K1's shares calibrated: the time of one audit, of each check alone, the bytes each
check reads (algorithmic, from the snapshot's counts) and, for scale, the same context's
decision time in the same run.

    python scripts/audit_probe.py [--pods 100000000] [--nodes 1000000] [--groups 10000]
                                  [--reps 3] [--steps 20] [--out profiles/r09_audit/probe.json]

The report must be clean (no mismatch in any check, none skipped) after the load, after the
calibration and after one round of events applied in place; the script exits 1 otherwise.
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

INT64_MIN = np.iinfo(np.int64).min
NONE = 0xFFFFFFFF
SPARE = 0.02


def clean(rep):
    return not rep["skipped"] and all(v["n_bad"] == 0 for k, v in rep.items() if k != "skipped")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=100_000_000)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--groups", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import escalator_amd as esc
    from escalator_amd import _lib as L
    from oracle import soa
    P, N, G = args.pods, args.nodes, args.groups
    t0 = time.perf_counter()
    s = esc.Synth(P, N, G, config=4, seed=0xE5CA1A7E00000004, threads=16)
    nodes = s.nodes()
    ctx = esc.Context(s)
    ctx.set_spare(SPARE)                                       # room for the event round
    ctx.load_synth(s)
    rng = np.random.default_rng(29)
    pod_node = rng.integers(0, N, size=P, dtype=np.uint32)
    tainted = (nodes["flags"] & 2) != 0
    taint_s = np.where(tainted, 1_800_000_000 - rng.integers(0, 1200, size=N), INT64_MIN).astype(np.int64)
    ctx.load_placement(pod_node, taint_s, np.zeros(N, np.uint8))
    ctx.set_state(s.states)
    ctx.use_graph(True)
    for _ in range(3):
        ctx.run()
    ctx.sync()
    setup_s = time.perf_counter() - t0
    print("setup %.1f s" % setup_s, flush=True)

    def timed_audit(checks=None):
        ms = []
        for _ in range(args.reps):
            t = time.perf_counter()
            rep = ctx.audit(checks)
            ms.append((time.perf_counter() - t) * 1e3)
        return min(ms), rep

    reports = {}
    _, reports["after_load"] = timed_audit()
    print("after load", json.dumps(reports["after_load"]), flush=True)
    ctx.k1_calibrate(2)
    for _ in range(2):
        ctx.run()
    ctx.sync()
    all_ms, reports["after_calibration"] = timed_audit()
    per_check = {}
    for name in L.AUDIT_CHECKS:
        per_check[name], _ = timed_audit([name])
        print(name, "%.2f ms" % per_check[name], flush=True)
    t = time.perf_counter()
    for _ in range(args.steps):
        ctx.run()
    ctx.sync()
    decision_ms = (time.perf_counter() - t) / args.steps * 1e3

    # one event round in place: node updates (taint flips, allocatable), node deletes, pod
    # deletes, pod moves (a move that does not fit its node's run is left out and counted)
    events = {}
    ids = np.sort(rng.choice(N, 2000, replace=False)).astype(np.int64)
    upd, dele = ids[:1900], ids[1900:]
    ctx.nodes_update(upd, nodes["flags"][upd] ^ np.uint32(2), nodes["cpu"][upd] + 1000, nodes["mem"][upd])
    ctx.nodes_delete(dele)
    events["nodes_update"], events["nodes_delete"] = len(upd), len(dele)
    gone = np.sort(rng.choice(P, 2000, replace=False)).astype(np.int64)
    ctx.pods_delete(gone[:1000])
    events["pods_delete"] = 1000
    live_nodes = np.setdiff1d(np.arange(N), dele)
    try:
        ctx.pods_bind(gone[1000:], rng.choice(live_nodes, 1000).astype(np.uint32))
        events["pods_bind"] = 1000
    except L.EscError as e:
        if e.code != L.ESC_E_LIMIT:
            raise
        events["pods_bind"] = 0
    ctx.run()
    ctx.sync()
    events_ms, reports["after_events"] = timed_audit()

    # algorithmic bytes per check, from the snapshot's counts
    tb = soa.group_tables(s.groups)
    n_gp = tb["n_gp"]
    inc = int((nodes["label0"] < n_gp).sum() + (nodes["xl_pair"] < n_gp).sum())     # live (node, group pair) incidences
    n_cap = N + int(math.ceil(N * SPARE)) + 64
    spare_e = sum(int(math.ceil(c * SPARE)) + 4 for c in np.bincount(
        np.concatenate([nodes["label0"][nodes["label0"] < n_gp], nodes["xl_pair"][nodes["xl_pair"] < n_gp]]).astype(np.int64),
        minlength=n_gp))
    entries = inc + spare_e
    memb = reports["after_calibration"]["REGION"]["n_checked"]
    pod_bytes, _ = ctx.stream_bytes()
    n_trk = len(nodes["trk_node"])
    bytes_read = {
        # per entry: flags, node, cpu, mem, the packed record, its pair; per live entry its node's flags, cpu, mem,
        # label0; the reverse walk: per slot flags + two map offsets, per incidence a map word, the entry's node, its range
        "ENTRY": entries * (4 + 4 + 8 + 8 + 16 + 4) + inc * (4 + 8 + 8 + 4) + n_cap * 12 + inc * (4 + 4 + 16),
        "FIRST": entries * 4 + inc * 4 + G * 40,
        "REGION": memb * (4 + 4 + 4 + 4 + 16) + G * 8,
        # the recount: per entry flags, pair, node; per live entry its node's run bounds and every PodRef of the run
        # (20 B; a node of k group pairs has its run read k times); the compare: four words per entry
        "OCC": entries * 12 + inc * 8 + int(P * inc / max(N, 1)) * 20 + entries * 16,
        # k_touch walks every K pod's head and pair words: K1's pod stream is the upper bound; then the downloads
        "TOUCH": pod_bytes,
        "TRACKER": n_cap * (8 + 4 * max(1, int(math.log2(max(n_trk, 2))))) + n_trk * 16,
        "MIRROR": n_cap * 24,
    }
    ok = all(clean(r) for r in reports.values())
    slowest = max(per_check, key=per_check.get)
    out = {
        "metric": "esc_audit on one context beside its decision",
        "config": {"pods": P, "nodes": N, "node_groups": G, "spare": SPARE, "node_slots": n_cap,
                   "group_pair_incidences": inc, "entries_with_spare": entries, "memberships": memb, "tracker_entries": n_trk},
        "ms_audit_all_checks": all_ms, "ms_audit_all_checks_after_events": events_ms, "ms_per_check": per_check,
        "ms_per_decision": decision_ms, "audit_over_decision": all_ms / decision_ms,
        "slowest_check": slowest, "bytes_read_per_check": bytes_read,
        "reps": args.reps, "steps": args.steps, "setup_s": setup_s, "events": events,
        "n_checked": {k: v["n_checked"] for k, v in reports["after_events"].items() if k != "skipped"},
        "clean": {k: clean(r) for k, r in reports.items()},
        "data": "synthetic (esc_synth.cpp config 4; every pod on a random node)",
    }
    if not ok:
        out["reports"] = reports
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
