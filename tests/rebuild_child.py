"""Child process of tests/test_gpu_rebuild.py, on the MEASUREMENT library (ESC_LIB_PATH =
escalator_amd/libescalator_hip_measure.so).  One JSON line per run.

  repair <target>   tests/audit_child.py's poke of <target> on its small context (the same word,
                    found the same way: its mode_poke runs unchanged), the audit's report of it,
                    esc_nodes_rebuild, the audit again and the decision against the C oracle
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import audit_child as A  # noqa: E402


def _bad(rep):
    return [k for k, v in rep.items() if k != "skipped" and v["n_bad"] > 0]


def mode_repair(lib, esc, target):
    from oracle import soa
    soa.build()
    held = {}
    load_small = A.load_small

    def keep(esc_, trackers=True):                             # mode_poke's context, kept for what follows
        held["world"] = load_small(esc_, trackers)
        return held["world"]

    A.load_small = keep
    try:
        poked = A.mode_poke(lib, esc, target)
    finally:
        A.load_small = load_small
    ctx, groups, states, pods, nodes, P, N = held["world"]
    ctx.nodes_rebuild()
    after = ctx.audit()
    otot = soa.totals(P, N, groups)
    odf, odi = soa.decide(groups, states, otot)
    equal = False
    if target != "host_ncpu":                                  # (a wrong mirror is not decided on)
        tot, dec = ctx.decide_all(states)
        equal = all(np.array_equal(tot[name], otot[:, k]) for k, name in enumerate(soa.TOT_FIELDS) if name != "flags")
        equal = equal and np.array_equal(dec["cpu_pct"].view(np.uint64), odf[:, 0].view(np.uint64))
        equal = equal and np.array_equal(dec["mem_pct"].view(np.uint64), odf[:, 1].view(np.uint64))
        equal = equal and np.array_equal(dec["delta"].astype(np.int64), odi[:, 0])
        equal = equal and np.array_equal(dec["branch"].astype(np.int64), odi[:, 5])
    return {"id": poked["id"], "bad_before": _bad(poked["report"]), "bad_after": _bad(after),
            "skipped_after": after["skipped"], "decision_equal": bool(equal)}


if __name__ == "__main__":
    import escalator_amd as esc
    from escalator_amd import _lib as L
    lib = L.load()
    assert hasattr(lib, "esc_debug_poke"), "not the measurement library: %s" % L.LIB_PATH
    lib.esc_debug_poke.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64]
    lib.esc_debug_poke.restype = C.c_int32
    assert sys.argv[1] == "repair"
    print(json.dumps(mode_repair(lib, esc, sys.argv[2])), flush=True)
