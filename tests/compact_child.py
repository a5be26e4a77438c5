"""Child process of tests/test_gpu_compact.py, on the MEASUREMENT library (ESC_LIB_PATH =
escalator_amd/libescalator_hip_measure.so).  One JSON line per run.

  refuse   tests/audit_child.py's small context with three nodes deleted; esc_debug_poke 8 makes
           the mirror h_ncpu of a live node disagree with the table, poke 9 clears a deleted
           slot's absent bit in the mirror h_nflags only.  esc_nodes_compact then plans a source
           the table calls absent: k_node_gather reports it, the call answers ESC_E_HIP and
           nothing is swapped — the audit (MIRROR's report of the two pokes included), the
           room and every answer are what they were.  Both pokes are value words: no kernel
           indexes with them unchecked.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import audit_child as A  # noqa: E402

NOW = 1_700_000_000 * 10**9 + 10**12


def _answers(ctx, states, n_groups):
    tot, dec = ctx.decide_all(states)
    rm = ctx.try_remove(NOW, 300 * 10**9, 3600 * 10**9)
    return {"tot": tot.tobytes().hex(), "dec": dec.tobytes().hex(), "rm": rm.tobytes().hex(),
            "rm_list": [[int(j) for j in ctx.removal_nodes(g)] for g in range(n_groups)],
            "order": [[int(j) for j in ctx.group_order(g, w)] for g in range(n_groups) for w in (0, 1)],
            "trk": [[int(j) for j in ctx.tracker_list(g)] for g in range(n_groups)]}


def mode_refuse(lib, esc):
    from escalator_amd import _lib as L
    ctx, groups, states, pods, nodes, P, N = A.load_small(esc)
    ctx.set_order_in_step(True)
    ctx.nodes_delete([3, 150, 299])
    assert lib.esc_debug_poke(ctx.handle, 9, 4, 0) == L.ESC_E_INVAL      # a live slot: refused
    assert lib.esc_debug_poke(ctx.handle, 8, 7, 123_457) == 0
    assert lib.esc_debug_poke(ctx.handle, 9, 150, 0) == 0
    before, room = ctx.audit(), ctx.nodes_room()
    ans = _answers(ctx, states, len(groups))
    code = 0
    try:
        ctx.nodes_compact()
    except L.EscError as e:
        code = e.code
    after = ctx.audit()
    return {"code": code, "hip": L.ESC_E_HIP, "audit_equal": after == before, "mirror_bad": before["MIRROR"]["n_bad"],
            "other_bad": [k for k in before if k not in ("skipped", "MIRROR") and before[k]["n_bad"]],
            "room_equal": ctx.nodes_room() == room, "answers_equal": _answers(ctx, states, len(groups)) == ans}


if __name__ == "__main__":
    import escalator_amd as esc
    from escalator_amd import _lib as L
    lib = L.load()
    assert hasattr(lib, "esc_debug_poke"), "not the measurement library: %s" % L.LIB_PATH
    lib.esc_debug_poke.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64]
    lib.esc_debug_poke.restype = C.c_int32
    assert sys.argv[1] == "refuse"
    print(json.dumps(mode_refuse(lib, esc)), flush=True)
