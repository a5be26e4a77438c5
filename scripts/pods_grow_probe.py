"""esc_pods_grow beside the full reload, at BASELINE config #3's pod side (10 M pods) and, with
--configs 3,4, config #4's (100 M): one context, best of --reps.

Per repetition the context is reloaded with the base pods (that reload — esc_load_pods +
esc_load_nodes + esc_load_placement — is the figure the grow stands beside), a burst of 10 % new
pods is refused by esc_pods_upsert (ESC_E_LIMIT), esc_pods_grow is timed with that batch and the
upsert must then fit.  Recorded:

  - esc_pods_grow and its parts (host plan, buffers + staged upload, k_kb_regrow to its wait, the
    C copies, other replicas, work re-plan + touch); the split needs the measurement library
    (ESC_LIB_PATH = escalator_amd/libescalator_hip_measure.so), the product library reports totals;
  - k_kb_regrow's bytes per second (bytes written; as many are read) beside hipMemcpy device to
    device of the old K array in the same call;
  - ms_per_step of the grown context against a context freshly loaded with the same pods and the
    same spare, 5 runs each, interleaved, with esc_k1_flush_entries of both.

    python scripts/pods_grow_probe.py [--configs 3] [--reps 3] [--out profiles/r14_pods_grow/probe.json]

The decision of the grown context must equal the fresh one's bit for bit and the audit be clean;
the script exits 1 otherwise.  Prints one JSON line (and writes it to --out)."""
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
SIZES = {3: (10_000_000, 100_000, 100), 4: (100_000_000, 1_000_000, 10_000)}
SPLIT = ["host_plan", "buffers_upload", "kb_regrow_to_wait", "c_copies", "other_replicas", "replan_touch"]
CHECKS = ["ENTRY", "FIRST", "REGION", "OCC", "TOUCH", "TRACKER", "MIRROR"]
STEPS = 20


def times(lib, n):
    if not hasattr(lib, "esc_debug_grow_times"):
        return None
    ms = (C.c_double * n)()
    lib.esc_debug_grow_times(ms, n)
    return [float(x) for x in ms]


def step_ms(ctx):
    ctx.run()
    ctx.sync()
    t = time.perf_counter()
    for _ in range(STEPS):
        ctx.run()
    ctx.sync()
    return (time.perf_counter() - t) * 1e3 / STEPS


def probe(esc, lib, config, reps):
    from escalator_amd import _lib as L
    n_pods, n_nodes, n_groups = SIZES[config]
    n_burst = n_pods // 10
    seed = 0xE5CA1A7E00000000 + config
    base = esc.Synth(n_pods + n_burst, n_nodes, n_groups, config=config, seed=seed, p_hi=n_pods, threads=16)
    burst = esc.Synth(n_pods + n_burst, n_nodes, n_groups, config=config, seed=seed, p_lo=n_pods, threads=16)
    P, N, B = base.pods(), base.nodes(), burst.pods()
    ids = np.arange(n_pods, n_pods + n_burst, dtype=np.int64)
    rng = np.random.default_rng(31)
    pod_node = rng.integers(0, n_nodes, size=n_pods, dtype=np.uint32)
    tainted = (N["flags"] & 2) != 0
    taint_s = np.where(tainted, 1_800_000_000 - rng.integers(0, 1200, size=n_nodes), INT64_MIN).astype(np.int64)
    no_delete = np.zeros(n_nodes, np.uint8)
    ctx = esc.Context(base)
    ctx.set_spare(SPARE)
    ctx.set_state(base.states)
    out = {"pods": n_pods, "burst": n_burst, "nodes": n_nodes, "node_groups": n_groups, "spare": SPARE}
    best, reloads = None, []
    for _ in range(reps):
        t = time.perf_counter()
        ctx.load(P, N)
        ctx.load_placement(pod_node, taint_s, no_delete)
        reloads.append((time.perf_counter() - t) * 1e3)
        ctx.run()
        ctx.sync()
        assert ctx.pods_upsert(ids, B) == L.ESC_E_LIMIT
        t = time.perf_counter()
        ctx.pods_grow(ids, B)
        ms = (time.perf_counter() - t) * 1e3
        if best is None or ms < best[0]:
            best = (ms, times(lib, 8))
        t = time.perf_counter()
        assert ctx.pods_upsert(ids, B) == 0
        out["ms_pods_upsert_after"] = (time.perf_counter() - t) * 1e3
    out["ms_pods_grow"] = best[0]
    if best[1] is not None:
        out["ms_pods_grow_split"] = dict(zip(SPLIT, best[1][:6]))
        kb_bytes, ms_kernel, ms_memcpy = best[1][6], best[1][2], best[1][7]
        out["kb_regrow"] = {"bytes_written": kb_bytes, "ms_to_wait": ms_kernel,
                            "gb_per_s_written": kb_bytes / ms_kernel / 1e6 if ms_kernel else None,
                            "memcpy_dtod_old_array_ms": ms_memcpy}
    out["ms_full_reload"] = min(reloads)
    out["ms_full_reload_all"] = reloads
    out["grow_over_full_reload"] = out["ms_pods_grow"] / out["ms_full_reload"]
    rep = ctx.audit(CHECKS)
    out["clean"] = not rep["skipped"] and all(rep[k]["n_bad"] == 0 for k in CHECKS)
    # ---- the grown context against a fresh load of the same pods at the same spare
    full = esc.Synth(n_pods + n_burst, n_nodes, n_groups, config=config, seed=seed, threads=16)
    fresh = esc.Context(full)
    fresh.set_spare(SPARE)
    fresh.set_state(full.states)
    fresh.load(full.pods(), N)
    a, b = ctx.decide_all(base.states), fresh.decide_all(full.states)
    out["equal_to_fresh"] = a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    runs = {"grown": [], "fresh": []}
    for _ in range(5):
        runs["grown"].append(step_ms(ctx))
        runs["fresh"].append(step_ms(fresh))
    out["ms_per_step"] = {k: {"runs": v, "min": min(v), "max": max(v)} for k, v in runs.items()}
    out["ranges_overlap"] = min(runs["grown"]) <= max(runs["fresh"]) and min(runs["fresh"]) <= max(runs["grown"])
    out["k1_flush_entries"] = {"grown": list(ctx.k1_flush_entries()), "fresh": list(fresh.k1_flush_entries())}
    out["stream_bytes"] = {"grown": list(ctx.stream_bytes()), "fresh": list(fresh.stream_bytes())}
    r1, r2 = ctx.pods_room(), fresh.pods_room()
    out["k_capacity"] = {"grown": r1["k_capacity"], "fresh": r2["k_capacity"]}
    for x in (ctx, fresh, base, burst, full):
        x.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="3")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import escalator_amd as esc
    from escalator_amd import _lib as L
    lib = L.load()
    if hasattr(lib, "esc_debug_grow_times"):
        lib.esc_debug_grow_times.argtypes = [C.POINTER(C.c_double), C.c_int32]
        lib.esc_debug_grow_times.restype = C.c_int32
    res = {"metric": "esc_pods_grow for a burst of 10 % new pods beside the full reload, one context, best of reps",
           "library": os.path.basename(L.LIB_PATH), "reps": args.reps, "steps_per_run": STEPS, "configs": {},
           "data": "synthetic (esc_synth.cpp; every pod on a random node; the burst is the next 10 % of the same generator)"}
    ok = True
    for c in [int(x) for x in args.configs.split(",")]:
        r = probe(esc, lib, c, args.reps)
        print("config %d" % c, json.dumps(r), flush=True)
        res["configs"][str(c)] = r
        ok = ok and r["clean"] and r["equal_to_fresh"]
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
