"""The small cluster of tests/test_gpu_nodes_verify.py, and — run as a program on the measurement
library (ESC_LIB_PATH = escalator_amd/libescalator_hip_measure.so) — the one case that library is
needed for: its esc_debug_multi_sub hands out one device's context of a two-shard context, so a
node event can reach ONE shard's copy of the node table alone.  esc_nodes_verify on the two-shard
context must report that node although the other shard's copy matches.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

KEYS = ["k0", "k1", "k2"]
TAINT = "atlassian.com/escalator"
T0 = 1_700_000_000 * 10**9
N_GROUPS, N_NODES, N_PODS = 40, 600, 400


def group(g):
    return {"name": "g%d" % g, "label_key": KEYS[g % 3], "label_value": "v%d" % (g // 3), "min_nodes": 0, "max_nodes": 5000,
            "taint_lower_pct": 20, "taint_upper_pct": 40, "scale_up_pct": 70, "slow_removal_rate": 1, "fast_removal_rate": 2,
            "dry_mode": False, "soft_delete_grace_ns": 60 * 10**9, "hard_delete_grace_ns": 600 * 10**9}


def node(i, name=None):
    """Node i: 0 to 3 labels on the groups' keys (so 0 to 2 extra label pairs; k2's v13 and v14 are
    no group's), every seventh tainted with a time, every eleventh cordoned, every thirteenth safe
    from deletion."""
    labels = {}
    if i % 25 != 24:
        labels["k0"] = "v%d" % (i % 14)
    if i % 3 >= 1:
        labels["k1"] = "v%d" % (i % 13)
    if i % 3 == 2:
        labels["k2"] = "v%d" % ((i * 7) % 15)
    x = {"name": name or "n%d" % i, "labels": labels, "unschedulable": i % 11 == 0, "taints": [], "cpu": 4000 + i % 7,
         "mem": (8 << 30) + i, "created_ns": T0 + (i * 7919 % 600) * 1000, "annotations": {}}
    if i % 7 == 0:
        x["taints"], x["taint_value"] = [TAINT], str(T0 // 10**9 - 30 * (i % 50))
    if i % 13 == 0:
        x["annotations"] = {"atlassian.com/no-delete": "true"}
    return x


def pod(i):
    g = i % N_GROUPS
    return {"name": "p%d" % i, "owner_kinds": [], "annotations": {}, "node_selector": {KEYS[g % 3]: "v%d" % (g // 3)},
            "affinity": None, "containers": [{"cpu": 100 + i % 40, "mem": (1 << 20) + i}], "init_containers": [],
            "overhead": None, "node_name": "n%d" % (i * 3 % N_NODES) if i % 4 else ""}


def cluster(n_nodes=N_NODES, n_pods=N_PODS):
    return [group(g) for g in range(N_GROUPS)], [node(i) for i in range(n_nodes)], [pod(i) for i in range(n_pods)]


def main():
    from escalator_amd import _lib as L
    from escalator_amd.context import Context
    from escalator_amd.objects import placement
    lib = L.load()
    assert hasattr(lib, "esc_debug_multi_sub"), "not the measurement library: %s" % L.LIB_PATH
    lib.esc_debug_multi_sub.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    lib.esc_debug_multi_sub.restype = C.c_int32
    groups, nodes, pods = cluster()
    ctx = Context(groups, devices=[0, 0])
    ctx.set_spare(0.5)
    P, N = ctx.pack(pods, nodes)
    ctx.load(P, N)
    pn, t, d = placement(pods, nodes)
    ctx.load_placement(pn, t, d)
    ids = np.arange(len(nodes), dtype=np.int64)
    inst = np.full(len(nodes), -(1 << 63), np.int64)
    st, rep = ctx.nodes_verify(ids, N, t, d, inst)
    out = {"clean": int(np.count_nonzero(st)), "clean_rep": rep}

    def send(shard, j, flags, cpu, mem):
        sub = C.c_void_p()
        assert lib.esc_debug_multi_sub(ctx.handle, shard, C.byref(sub)) == 0
        a, f = np.array([j], np.int64), np.array([flags], np.uint32)
        c_, m = np.array([cpu], np.int64), np.array([mem], np.int64)
        rc = lib.esc_nodes_update(sub, a.ctypes.data_as(C.POINTER(C.c_int64)), 1, f.ctypes.data_as(C.POINTER(C.c_uint32)),
                                  c_.ctypes.data_as(C.POINTER(C.c_int64)), m.ctypes.data_as(C.POINTER(C.c_int64)))
        assert rc == 0, rc
    sub = C.c_void_p()
    out["bad_shard"] = lib.esc_debug_multi_sub(ctx.handle, 2, C.byref(sub))
    # node 40 on shard 1 alone (its taint), node 300 on shard 0 alone (its cpu), node 500 on both
    send(1, 40, int(N["flags"][40]) ^ 2, int(N["cpu"][40]), int(N["mem"][40]))
    send(0, 300, int(N["flags"][300]), int(N["cpu"][300]) + 1, int(N["mem"][300]))
    for s in (0, 1):
        send(s, 500, int(N["flags"][500]), int(N["cpu"][500]), int(N["mem"][500]) + 5)
    st, rep = ctx.nodes_verify(ids, N, t, d, inst)
    out["found"] = {int(i): int(st[i]) for i in np.flatnonzero(st)}
    out["rep"] = rep
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    sys.exit(main())
