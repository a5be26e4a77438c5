"""Child process of tests/test_gpu_k1_width.py on the MEASUREMENT library (ESC_LIB_PATH =
escalator_amd/libescalator_hip_measure.so), whose ESC_K1_THREADS knob forces K1's workgroup
width (the product library reads none and runs 512 threads).  The knob is read when a context
is created.  Prints one JSON line:
  widths: "<slots>@<threads>" -> the pod mix of tests/test_gpu_k1_width.py on each side of
          SWITCH_S with that width forced: exact against the C oracle, and byte-equal to the
          first width's totals and decisions at the same slot count;
  mix_full_window: the pod mix over a full window at 1024 threads;
  paths:  slot count -> the test's paths (the same functions) at 1024 threads;
  noplan: ESC_K1_VARIANT=7 at 1024 threads (null plan: the weight-range walk, full-row flush)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import escalator_amd as esc  # noqa: E402
from escalator_amd import _lib as L  # noqa: E402
from oracle import soa  # noqa: E402

soa.build()


def exact(ctx, w):
    tot, dec = ctx.results()
    ok = all(np.array_equal(tot[n], w["otot"][:, k]) for k, n in enumerate(soa.TOT_FIELDS[:12]))
    ok &= np.array_equal(dec["cpu_pct"].view(np.uint64), w["odf"][:, 0].view(np.uint64))
    ok &= np.array_equal(dec["mem_pct"].view(np.uint64), w["odf"][:, 1].view(np.uint64))
    ok &= np.array_equal(dec["delta"], w["odi"][:, 0]) and np.array_equal(dec["n_to_taint"], w["odi"][:, 1])
    return bool(ok), tot.tobytes() + dec.tobytes()


def force(threads, variant=0):
    os.environ["ESC_K1_THREADS"], os.environ["ESC_K1_VARIANT"] = str(threads), str(variant)


def run_mix(T, S, threads, variant=0):
    force(threads, variant)
    w = T.world(esc, S)
    ctx = esc.Context(w["groups"])
    ctx.load(w["P"], w["N"])
    ctx.set_state(w["states"])
    ok, raw = True, None
    for _ in range(2):
        ctx.run()
        e, raw = exact(ctx, w)
        ok &= e
    tr = ctx.k1_trace()
    entries, full = ctx.k1_flush_entries()
    out = {"slots": L.load().esc_ctx_num_group_pairs(ctx.handle) + 1, "exact": ok, "workgroups": int(tr.shape[0]),
           "entries": entries, "full": full, "plan_words_zero": bool(np.all(tr[:, 6:8] == 0))}
    ctx.close()
    return out, raw


def main():
    assert hasattr(L.load(), "esc_debug_lookback_fail"), "not the measurement library: %s" % L.LIB_PATH
    import test_gpu_k1_width as T
    widths = {}
    for S in (T.SWITCH_S, T.SWITCH_S + 1):
        first = None
        for threads in (512, 1024):
            out, raw = run_mix(T, S, threads)
            first = raw if first is None else first
            out["same_as_first"] = raw == first
            widths["%d@%d" % (S, threads)] = out
    full, _ = run_mix(T, T.WINDOW, 1024)
    force(1024)
    paths = {}
    for S in T.PATH_S:
        paths[str(S)] = {}
        for name, fn in T.PATHS.items():
            fn(esc, S)                                   # asserts exactness itself
            paths[str(S)][name] = True
    noplan, _ = run_mix(T, T.WINDOW + 1, 1024, variant=7)
    print(json.dumps({"widths": widths, "mix_full_window": {"slots": full["slots"], "exact": full["exact"]},
                      "paths": paths, "noplan": noplan}), flush=True)


if __name__ == "__main__":
    main()
