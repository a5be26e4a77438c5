"""Child process of tests/test_gpu_pod_audit.py, on the MEASUREMENT library (ESC_LIB_PATH =
escalator_amd/libescalator_hip_measure.so): its esc_debug_poke_pods makes one word of the
resident pod side wrong, which the product library cannot do.  One JSON line per run.

  poke <target>   the small pod context (3 replicas, placed), one poke, esc_audit_pods only (no
                  decision, reaping pass, event or compaction runs on the poked state), the
                  report, the poked id and the refused pokes' codes
  heal            ResidentController(pod_audit_every=1) beside the reloading Controller on the
                  seeded history of tests/test_gpu_resident.py, a free K position poked before
                  the third pod audit
  state           ESC_E_STATE before esc_load_pods and on a context a failed pod event left stale

The small context's builders are imported by the parent too (they load no library)."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from audit_child import SPARE, small_cluster  # noqa: E402

POKES = {"free_k": 0, "free_k12": 0, "ds_bits": 1, "inert_pair": 2, "count": 3, "map": 4, "cflags": 5, "parked_pair": 6, "podref": 7,
         "replica": 8}
OWNER = {"free_k": "KSLOT", "free_k12": "KSLOT", "ds_bits": "KSLOT", "inert_pair": "KSLOT", "count": "COUNT", "map": "MAP", "cflags": "CSLOT",
         "parked_pair": "CSLOT", "podref": "PODREF", "replica": "REPLICA"}
REPLICAS = 3
N_INERT, N_WIDE, N_P12 = 3, 2, 2


def pod_cluster():
    """audit_child's small cluster (40 groups, 300 nodes, 4 000 pods, node-0 with 70 pods, node-1
    with none) and, behind its pods, unbound: N_INERT pods whose selector names no group's pair
    (default-blocking, in an inert class), N_WIDE pods of 6 pairs (the C section, indirect
    PodRefs once bound) and N_P12 pods that request 17 GiB (past the packed small range: the
    12-byte packed class without extra pairs)."""
    from test_gpu_pods_grow import c_pod
    rng, groups, states, pods, nodes = small_cluster()
    first = len(pods)
    for k in range(N_INERT):
        pods.append({"name": "inert%d" % k, "owner_kinds": [], "annotations": {}, "node_selector": {"no-such-key": "v%d" % k},
                     "affinity": None, "containers": [{"cpu": 100 + k, "mem": 1 << 20}], "init_containers": [],
                     "overhead": None, "node_name": ""})
    pools = ["zz%d" % k for k in range(9)]
    for k in range(N_WIDE):
        pods.append(c_pod("wide%d" % k, k, pools, "", containers=1, pairs=6))
    for k in range(N_P12):
        pods.append({"name": "p12-%d" % k, "owner_kinds": [], "annotations": {}, "node_selector": {}, "affinity": None,
                     "containers": [{"cpu": 300 + k, "mem": (17 << 30) + k}], "init_containers": [], "overhead": None,
                     "node_name": ""})
    return rng, groups, states, pods, nodes, first


def load_pods_small(esc, replicas=REPLICAS):
    from escalator_amd.objects import placement
    rng, groups, states, pods, nodes, first = pod_cluster()
    ctx = esc.Context(groups)
    ctx.set_spare(SPARE)
    P, N = ctx.pack(pods, nodes)
    ctx.load(P, N, replicas=replicas)
    ctx.load_placement(*placement(pods, nodes))
    return ctx, groups, states, pods, nodes, first, P, N


def bound(pods, nodes):
    names = {x["name"] for x in nodes}
    return sum(1 for p in pods if p.get("node_name") in names)


def is_clean(rep):
    return all(v["n_bad"] == 0 and v["first_bad"] == -1 for k, v in rep.items() if k != "skipped")


def _poke(lib, ctx, what, index, value):
    return lib.esc_debug_poke_pods(ctx.handle, what, index, value)


def _first_ok(lib, ctx, what, value, limit):
    for i in range(limit):
        if _poke(lib, ctx, what, i, value) == 0:
            return i
    raise AssertionError("no index accepted for poke %d" % what)


def mode_poke(lib, esc, target):
    from test_gpu_pods_grow import c_pod
    ctx, groups, states, pods, nodes, first, P, N = load_pods_small(esc)
    what = POKES[target]
    slot = lambda i: int(lib.esc_debug_pod_slot(ctx.handle, i))          # noqa: E731
    unbound_k = [i for i, p in enumerate(pods) if not p["node_name"] and ctx.pod_where(i)[0] >= 0]
    i8 = next(i for i in unbound_k if 256 <= ctx.pod_where(i)[0] < 260)     # a live pod of a packed small class
    if target == "parked_pair":
        # a spare-room slot: the 6-pair pod's slot re-used in place by a 5-pair pod
        small = c_pod("wide0", 0, ["zz%d" % k for k in range(9)], "", containers=1, pairs=5)
        where = ctx.pod_where(first + N_INERT)
        assert ctx.pods_upsert([first + N_INERT], ctx.pack([small], [])[0]) == 0
        assert ctx.pod_where(first + N_INERT) == where and where[0] == -1
    before = ctx.audit_pods()
    assert is_clean(before) and not before["skipped"], before
    cap = ctx.pods_room()["k_capacity"]
    aux = {}
    if target == "free_k":                                     # the lowest free position: a packed small class's
        ident = _first_ok(lib, ctx, what, 77, cap)
        aux["format"] = 8
    elif target == "free_k12":
        # the 12-byte format: the first free position behind a pod of the 12-byte class (its
        # class's tiles follow it, with spare positions at their end)
        p12 = first + N_INERT + N_WIDE
        assert ctx.pod_where(p12)[0] == 128, ctx.pod_where(p12)
        ident = next(i for i in range(slot(p12) + 1, cap) if _poke(lib, ctx, what, i, 77) == 0)
        assert ident - slot(p12) < 256 * 3, (ident, slot(p12))          # still that class's tiles (2 pods, spare 2.0)
        aux["format"] = 12
    elif target == "ds_bits":
        ident = slot(i8)
        assert _poke(lib, ctx, what, ident, 0) == 0
    elif target == "inert_pair":
        assert ctx.pod_where(first)[0] == 384, ctx.pod_where(first)
        ident = slot(first)
        assert _poke(lib, ctx, what, ident, 0) == 0
    elif target == "count":
        ident = 5
        assert _poke(lib, ctx, what, 0, 3) == 0
    elif target == "map":
        ident = slot(unbound_k[7])
        assert _poke(lib, ctx, what, unbound_k[7], 0) == 0
    elif target == "cflags":
        i = next(i for i in range(len(pods)) if ctx.pod_where(i)[0] == -1)
        ident = ctx.pod_where(i)[1]
        aux["bound"] = bool(pods[i]["node_name"])
        assert _poke(lib, ctx, what, ident, 0) == 0
    elif target == "parked_pair":
        ident = ctx.pod_where(first + N_INERT)[1]
        assert _poke(lib, ctx, what, ident, 12345) == 0
    elif target == "podref":
        ident = _first_ok(lib, ctx, what, 0x0FFFFFF0, 1 << 16)
    elif target == "replica":
        assert _poke(lib, ctx, what, slot(i8), int(P["cpu0"][i8]) ^ 1) == 0
        ident = (1 << 56) | (0 << 48) | int(lib.esc_debug_k_word(ctx.handle, slot(i8)))
    # everything outside the table of targets is refused
    big = 1 << 40
    refused = [_poke(lib, ctx, 9, 0, 0), _poke(lib, ctx, -1, 0, 0), _poke(lib, ctx, 0, -1, 1), _poke(lib, ctx, 0, big, 1),
               _poke(lib, ctx, 0, slot(i8), 1), _poke(lib, ctx, 1, big, 0), _poke(lib, ctx, 2, slot(i8), 0),
               _poke(lib, ctx, 3, 0, 0), _poke(lib, ctx, 4, big, 0), _poke(lib, ctx, 5, big, 0), _poke(lib, ctx, 6, big, 1),
               _poke(lib, ctx, 7, big, 1), _poke(lib, ctx, 8, big, 1)]
    return {"id": int(ident), "report": ctx.audit_pods(), "aux": aux, "refused": refused}


def mode_heal(lib, esc):
    import test_gpu_resident as R
    from escalator_amd.controller import ResidentController

    class Poked(ResidentController):
        poked = None

        def _pod_audit(self):
            if self.pod_audits == 2:                           # flushed, not yet audited: the third scan
                Poked.poked = _first_ok(lib, self.ctx, POKES["free_k"], 55, self.ctx.pods_room()["k_capacity"])
            super()._pod_audit()

    def resident(groups, clock, actuator, spare):
        return Poked(groups, clock=clock, actuator=actuator, spare=spare, pod_audit_every=1)

    # drive() asserts on every scan that the two controllers' records, states and trackers are
    # equal and equal the literal oracle: the healing scan and every later one included
    ra, rb, seen, reloads = R.drive(1, 2.0, resident, R._reload, burst=True)
    return {"reload_causes": ra.events.reload_causes, "reloads": reloads, "pod_audits": ra.pod_audits,
            "pod_audit_failures": ra.pod_audit_failures, "scans": R.SCANS, "poked": Poked.poked,
            "last_clean": is_clean(ra.last_pod_audit)}


def mode_state(lib, esc):
    from escalator_amd import _lib as L
    rng, groups, states, pods, nodes, first = pod_cluster()
    ctx = esc.Context(groups)
    ctx.set_spare(SPARE)
    P, N = ctx.pack(pods, nodes)
    out = {"unloaded_rc": lib.esc_audit_pods(ctx.handle, 0, C.byref(L.PodAuditReport()))}
    ctx.load(P, N)
    out["loaded_clean"] = is_clean(ctx.audit_pods())
    assert lib.esc_debug_fail_patches(ctx.handle, 1) == 0
    try:
        ctx.pods_delete([1])
        out["delete_code"] = 0
    except L.EscError as e:
        out["delete_code"] = e.code
    out["stale_rc"] = lib.esc_audit_pods(ctx.handle, 0, C.byref(L.PodAuditReport()))
    ctx.load(P, N)
    out["reloaded_clean"] = is_clean(ctx.audit_pods())
    return out


if __name__ == "__main__":
    import escalator_amd as esc
    from escalator_amd import _lib as L
    lib = L.load()
    assert hasattr(lib, "esc_debug_poke_pods"), "not the measurement library: %s" % L.LIB_PATH
    lib.esc_debug_poke_pods.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64]
    lib.esc_debug_poke_pods.restype = C.c_int32
    lib.esc_debug_pod_slot.argtypes = [C.c_void_p, C.c_int64]
    lib.esc_debug_pod_slot.restype = C.c_int64
    lib.esc_debug_k_word.argtypes = [C.c_void_p, C.c_int64]
    lib.esc_debug_k_word.restype = C.c_int64
    lib.esc_debug_fail_patches.argtypes = [C.c_void_p, C.c_int32]
    if sys.argv[1] == "poke":
        res = mode_poke(lib, esc, sys.argv[2])
    else:
        res = {"heal": mode_heal, "state": mode_state}[sys.argv[1]](lib, esc)
    print(json.dumps(res), flush=True)
