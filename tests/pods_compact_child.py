"""Child process of tests/test_gpu_pods_compact.py, on the MEASUREMENT library (ESC_LIB_PATH =
escalator_amd/libescalator_hip_measure.so).  One JSON line.

tests/audit_child.py's small context with every third pod deleted.  esc_debug_fail_compact makes
the next esc_pods_compact fail on the host after its new K section is built and before it is
swapped in (a returned ESC_E_HIP, no device fault): the audit, the room, every pod's place and
every answer are what they were.  The next compaction succeeds, moves pods and changes no answer.
Then a pod event that fails after its host-side writes (esc_debug_fail_patches) leaves the context
stale, and esc_pods_compact refuses it with ESC_E_STATE."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import audit_child as A  # noqa: E402
from compact_child import _answers  # noqa: E402
from pods_grow_child import _room  # noqa: E402


def run(lib, esc):
    from escalator_amd import _lib as L
    ctx, groups, states, pods, nodes, P, N = A.load_small(esc)
    ctx.set_order_in_step(True)
    n0 = len(pods)
    ctx.pods_delete(list(range(0, n0, 3)))
    where = lambda: [ctx.pod_where(i) for i in range(n0)]  # noqa: E731
    before, room, ans, at = ctx.audit(), _room(ctx), _answers(ctx, states, len(groups)), where()
    assert lib.esc_debug_fail_compact(ctx.handle, 1) == 0
    code = 0
    try:
        ctx.pods_compact()
    except L.EscError as e:
        code = e.code
    out = {"code": code, "hip": L.ESC_E_HIP, "e_state": L.ESC_E_STATE,
           "audit_equal": ctx.audit() == before, "room_equal": _room(ctx) == room, "where_equal": where() == at,
           "answers_equal": _answers(ctx, states, len(groups)) == ans}
    rep = ctx.pods_compact()                                   # the injection is used up
    out["moved_after"] = rep["moved"]
    out["report"] = rep
    aud = ctx.audit()
    out["bad_after"] = [k for k in aud if k != "skipped" and aud[k]["n_bad"]]
    out["answers_after_equal"] = _answers(ctx, states, len(groups)) == ans
    ms = (C.c_double * 12)()
    assert lib.esc_debug_pods_compact_times(ms, 12) == 0
    out["ms"] = list(ms)
    # a stale context
    assert lib.esc_debug_fail_patches(ctx.handle, 1) == 0
    try:
        ctx.pods_delete([1])
        out["delete_code"] = 0
    except L.EscError as e:
        out["delete_code"] = e.code
    try:
        ctx.pods_compact()
        out["stale_code"] = 0
    except L.EscError as e:
        out["stale_code"] = e.code
    return out


if __name__ == "__main__":
    import escalator_amd as esc
    from escalator_amd import _lib as L
    lib = L.load()
    assert hasattr(lib, "esc_debug_fail_compact"), "not the measurement library: %s" % L.LIB_PATH
    for name in ("esc_debug_fail_compact", "esc_debug_fail_patches"):
        getattr(lib, name).argtypes = [C.c_void_p, C.c_int32]
        getattr(lib, name).restype = C.c_int32
    lib.esc_debug_pods_compact_times.argtypes = [C.POINTER(C.c_double), C.c_int32]
    lib.esc_debug_pods_compact_times.restype = C.c_int32
    print(json.dumps(run(lib, esc)), flush=True)
