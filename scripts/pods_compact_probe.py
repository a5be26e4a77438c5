"""esc_pods_compact beside the full reload, at BASELINE config #3's pod side (10 M pods, spare
0.02): one context, one compaction.

The setup follows scripts/pods_grow_probe.py: the base pods are loaded, a burst of 10 % new pods
goes in through esc_pods_grow + esc_pods_upsert, then as many pods are deleted, spread over every
id, so there are holes everywhere and not just a free tail.  Recorded:

  - esc_pods_compact and its stages (candidates + classify, plan + buffers + upload, keys + sort
    with its launches, the move kernel, the map download, the host check + remap, C slots + other
    replicas, re-plan + touch); the split needs the measurement library (ESC_LIB_PATH =
    escalator_amd/libescalator_hip_measure.so), the product library reports the total;
  - the full reload (load + load_placement) of the same live pods in the same run: the yardstick,
    and the ratio;
  - the move kernel's bytes per second (bytes written) beside hipMemcpy device to device of as
    many bytes of the old K array in the same call;
  - ms_per_step, 5 interleaved runs of 20 steps, of the uncompacted context, the compacted one and
    a context freshly loaded with the same pods, with the K-block bytes K1 streams and
    esc_k1_flush_entries of each;
  - the decision before and after the call: byte-equal.

    python scripts/pods_compact_probe.py [--out profiles/r16_pods_compact/probe.json]

The decision after the call must equal the one before and the fresh load's bit for bit and the
audit be clean; the script exits 1 otherwise.  Prints one JSON line (and writes it to --out)."""
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
SIZES = {3: (10_000_000, 100_000, 100), 2: (1_000_000, 10_000, 100)}
SPLIT = ["candidates_classify", "plan_buffers_upload", "keys_sort", "move_kernel", "map_download_wait", "host_check_remap",
         "c_slots_other_replicas", "replan_touch_podrefs"]
CHECKS = ["ENTRY", "FIRST", "REGION", "OCC", "TOUCH", "TRACKER", "MIRROR"]
STEPS = 20


def step_ms(ctx):
    ctx.run()
    ctx.sync()
    t = time.perf_counter()
    for _ in range(STEPS):
        ctx.run()
    ctx.sync()
    return (time.perf_counter() - t) * 1e3 / STEPS


def subset(P, keep):
    """The packed records of the pods under the boolean mask `keep`, in order."""
    f = P["flags"].astype(np.uint64)
    nxc = (((f >> 8) & 0xFF) + ((f >> 16) & 0xFF) + ((f >> 4) & 1)).astype(np.int64)
    nxp = ((f >> 24) & 0x3F).astype(np.int64)
    out = {k: np.ascontiguousarray(P[k][keep]) for k in ("flags", "cpu0", "mem0", "pair0")}
    kc, kp = np.repeat(keep, nxc), np.repeat(keep, nxp)
    out["xc_cpu"] = np.ascontiguousarray(P["xc_cpu"][:len(kc)][kc])
    out["xc_mem"] = np.ascontiguousarray(P["xc_mem"][:len(kc)][kc])
    out["xp_pair"] = np.ascontiguousarray(P["xp_pair"][:len(kp)][kp])
    return out


def probe(esc, lib, config):
    from escalator_amd import _lib as L
    n_pods, n_nodes, n_groups = SIZES[config]
    n_burst = n_pods // 10
    seed = 0xE5CA1A7E00000000 + config
    base = esc.Synth(n_pods + n_burst, n_nodes, n_groups, config=config, seed=seed, p_hi=n_pods, threads=16)
    burst = esc.Synth(n_pods + n_burst, n_nodes, n_groups, config=config, seed=seed, p_lo=n_pods, threads=16)
    full = esc.Synth(n_pods + n_burst, n_nodes, n_groups, config=config, seed=seed, threads=16)
    P, N, B, PF = base.pods(), base.nodes(), burst.pods(), full.pods()
    ids = np.arange(n_pods, n_pods + n_burst, dtype=np.int64)
    rng = np.random.default_rng(31)
    pod_node = rng.integers(0, n_nodes, size=n_pods + n_burst, dtype=np.uint32)
    pod_node[n_pods:] = 0xFFFFFFFF                             # the burst's pods are not bound yet (the runs' room)
    tainted = (N["flags"] & 2) != 0
    taint_s = np.where(tainted, 1_800_000_000 - rng.integers(0, 1200, size=n_nodes), INT64_MIN).astype(np.int64)
    no_delete = np.zeros(n_nodes, np.uint8)
    out = {"pods": n_pods, "burst": n_burst, "deleted": n_burst, "nodes": n_nodes, "node_groups": n_groups, "spare": SPARE}

    def drained():
        c = esc.Context(base)
        c.set_spare(SPARE)
        c.set_state(base.states)
        c.load(P, N)
        c.load_placement(pod_node[:n_pods], taint_s, no_delete)
        c.run()
        c.sync()
        assert c.pods_upsert(ids, B) == L.ESC_E_LIMIT
        c.pods_grow(ids, B)
        assert c.pods_upsert(ids, B) == 0
        c.pods_delete(gone)
        return c
    gone = np.sort(rng.choice(n_pods + n_burst, size=n_burst, replace=False)).astype(np.int64)
    keep = np.ones(n_pods + n_burst, bool)
    keep[gone] = False
    live = subset(PF, keep)
    ctx, loose = drained(), drained()                          # one to compact, one left as it is
    before = ctx.decide_all(base.states)
    out["slack"] = ctx.pods_slack()
    t = time.perf_counter()
    rep = ctx.pods_compact()
    out["ms_pods_compact"] = (time.perf_counter() - t) * 1e3
    out["report"] = rep
    if hasattr(lib, "esc_debug_pods_compact_times"):
        ms = (C.c_double * 12)()
        lib.esc_debug_pods_compact_times(ms, 12)
        ms = [float(x) for x in ms]
        out["ms_pods_compact_split"] = dict(zip(SPLIT, ms[:8]))
        out["order_pass_launches"] = {"k_pc_keys": 1, "lsd_passes": int((ms[10] - 1) / 3),
                                      "per_pass": ["k_rs_hist", "k_rs_scan_rows", "k_rs_scatter"], "total": int(ms[10])}
        out["move_kernel"] = {"bytes_written": ms[8], "ms": ms[3], "gb_per_s_written": ms[8] / ms[3] / 1e6 if ms[3] else None,
                              "memcpy_dtod_bytes": ms[11], "memcpy_dtod_ms": ms[9],
                              "memcpy_gb_per_s": ms[11] / ms[9] / 1e6 if ms[9] else None}
    after = ctx.decide_all(base.states)
    out["equal_before_after"] = before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    a = ctx.audit(CHECKS)
    out["clean"] = not a["skipped"] and all(a[k]["n_bad"] == 0 for k in CHECKS)
    # ---- the full reload of the same live pods, in the same run
    fresh = esc.Context(full)
    fresh.set_spare(SPARE)
    fresh.set_state(full.states)
    reloads = []
    for _ in range(2):
        t = time.perf_counter()
        fresh.load(live, N)
        fresh.load_placement(pod_node[keep], taint_s, no_delete)
        reloads.append((time.perf_counter() - t) * 1e3)
    out["ms_full_reload"] = min(reloads)
    out["ms_full_reload_all"] = reloads
    out["compact_over_full_reload"] = out["ms_pods_compact"] / out["ms_full_reload"]
    b = fresh.decide_all(full.states)
    out["equal_to_fresh"] = after[0].tobytes() == b[0].tobytes() and after[1].tobytes() == b[1].tobytes()
    runs = {"uncompacted": [], "compacted": [], "fresh": []}
    for _ in range(5):
        runs["uncompacted"].append(step_ms(loose))
        runs["compacted"].append(step_ms(ctx))
        runs["fresh"].append(step_ms(fresh))
    out["ms_per_step"] = {k: {"runs": v, "min": min(v), "max": max(v)} for k, v in runs.items()}
    out["compacted_fresh_ranges_overlap"] = (min(runs["compacted"]) <= max(runs["fresh"]) and
                                             min(runs["fresh"]) <= max(runs["compacted"]))
    out["k1_flush_entries"] = {"uncompacted": list(loose.k1_flush_entries()), "compacted": list(ctx.k1_flush_entries()),
                               "fresh": list(fresh.k1_flush_entries())}
    out["k1_kblock_bytes"] = {"uncompacted": rep["k1_bytes_before"], "compacted": rep["k1_bytes_after"],
                              "fresh": fresh.pods_compact()["k1_bytes_before"]}
    out["stream_bytes"] = {"uncompacted": list(loose.stream_bytes()), "compacted": list(ctx.stream_bytes()),
                           "fresh": list(fresh.stream_bytes())}
    out["k_capacity"] = {"uncompacted": loose.pods_room()["k_capacity"], "compacted": ctx.pods_room()["k_capacity"],
                         "fresh": fresh.pods_room()["k_capacity"]}
    for x in (ctx, loose, fresh, base, burst, full):
        x.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import escalator_amd as esc
    from escalator_amd import _lib as L
    lib = L.load()
    if hasattr(lib, "esc_debug_pods_compact_times"):
        lib.esc_debug_pods_compact_times.argtypes = [C.POINTER(C.c_double), C.c_int32]
        lib.esc_debug_pods_compact_times.restype = C.c_int32
    res = {"metric": "esc_pods_compact after a 10 % burst and as many deletes spread over every id, beside the full "
                     "reload of the same live pods, one context, one call",
           "library": os.path.basename(L.LIB_PATH), "steps_per_run": STEPS, "config": args.config,
           "data": "synthetic (esc_synth.cpp; every pod on a random node; the burst is the next 10 % of the same generator)",
           "not_measured": "config 4 (100 M pods): its host remap and 400 MB map download are not measured here"}
    r = probe(esc, lib, args.config)
    res["result"] = r
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if r["clean"] and r["equal_before_after"] and r["equal_to_fresh"] else 1


if __name__ == "__main__":
    sys.exit(main())
