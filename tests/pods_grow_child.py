"""Child process of tests/test_gpu_pods_grow.py, on the MEASUREMENT library (ESC_LIB_PATH =
escalator_amd/libescalator_hip_measure.so).  One JSON line per run.

  refuse   tests/audit_child.py's small context; esc_debug_fail_grow makes the next esc_pods_grow
           fail on the host after its buffers are built and before they are swapped in (a
           returned ESC_E_HIP, no device fault).  Nothing is swapped: the audit, the room and
           every answer are what they were, and the next grow of the same batch succeeds and
           the batch then fits.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import audit_child as A  # noqa: E402
from compact_child import _answers  # noqa: E402


def _room(ctx):
    r = ctx.pods_room()
    return [r["k_capacity"], r["k_free"], r["c_free"], r["per_class"].tolist()]


def mode_refuse(lib, esc):
    from escalator_amd import _lib as L
    ctx, groups, states, pods, nodes, P, N = A.load_small(esc)
    ctx.set_order_in_step(True)
    n0 = len(pods)
    room = ctx.pods_room()
    # one-container pods without a selector: the packed small class without extra pairs (id 256);
    # one more of them than its free positions and the free C slots together
    n_new = int(room["per_class"][256]) + int(room["c_free"]) + 1
    assert 0 < n_new < 20_000, n_new
    new = [{"name": "burst-%d" % i, "owner_kinds": [], "annotations": {}, "node_selector": None, "affinity": None,
            "containers": [{"cpu": 100 + i % 7, "mem": 1 << 20}], "init_containers": [], "overhead": None,
            "node_name": ""} for i in range(n_new)]
    ids = list(range(n0, n0 + n_new))
    B, _ = ctx.pack(new, [])
    limit = ctx.pods_upsert(ids, B)
    before, room, ans = ctx.audit(), _room(ctx), _answers(ctx, states, len(groups))
    assert lib.esc_debug_fail_grow(ctx.handle, 1) == 0
    code = 0
    try:
        ctx.pods_grow(ids, B)
    except L.EscError as e:
        code = e.code
    out = {"limit": limit, "e_limit": L.ESC_E_LIMIT, "code": code, "hip": L.ESC_E_HIP,
           "audit_equal": ctx.audit() == before, "room_equal": _room(ctx) == room,
           "answers_equal": _answers(ctx, states, len(groups)) == ans,
           "still_limit": ctx.pods_upsert(ids, B)}
    ctx.pods_grow(ids, B)                                      # the injection is used up
    out["upsert"] = ctx.pods_upsert(ids, B)
    rep = ctx.audit()
    out["bad_after"] = [k for k in rep if k != "skipped" and rep[k]["n_bad"]]
    out["skipped_after"] = rep["skipped"]
    tot, _ = ctx.decide_all(states)
    out["n_pods"] = int(tot["n_pods"].sum())
    ms = (C.c_double * 6)()
    assert lib.esc_debug_grow_times(ms, 6) == 0
    out["ms"] = list(ms)
    return out


if __name__ == "__main__":
    import escalator_amd as esc
    from escalator_amd import _lib as L
    lib = L.load()
    assert hasattr(lib, "esc_debug_fail_grow"), "not the measurement library: %s" % L.LIB_PATH
    lib.esc_debug_fail_grow.argtypes = [C.c_void_p, C.c_int32]
    lib.esc_debug_fail_grow.restype = C.c_int32
    lib.esc_debug_grow_times.argtypes = [C.POINTER(C.c_double), C.c_int32]
    lib.esc_debug_grow_times.restype = C.c_int32
    assert sys.argv[1] == "refuse"
    print(json.dumps(mode_refuse(lib, esc)), flush=True)
