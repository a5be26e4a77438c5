"""Child process of tests/test_gpu_audit.py, on the MEASUREMENT library (ESC_LIB_PATH =
escalator_amd/libescalator_hip_measure.so): its esc_debug_poke makes one derived word of a
resident snapshot wrong, which the product library cannot do.  One JSON line per run.

  poke <target>   the small context, one poke, esc_audit only (no decision, reaping pass or
                  ordering runs on the poked state), the report and the poked id
  heal            ResidentController(audit_every=1) beside the reloading Controller on the seeded
                  history of tests/test_gpu_resident.py, an occupancy word poked before the
                  third audit
  skips           which checks are skipped before a plan, a placement and a valid age index

The small context's builders are imported by the parent too (they load no library)."""
import ctypes as C
import json
import math
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

SPARE = 2.0
POKES = {"entry_flags": 0, "entry_cpu": 1, "region_flags": 2, "region_swap": 3, "occ": 4, "touch": 5,
         "node_tracked": 6, "first_cpu": 7, "host_ncpu": 8}


def small_cluster(seed=4242):
    """About 40 groups (one of them surely dry), 300 nodes, 4 000 pods of random objects; node-0
    holds 70 pods (more than one wave of PodRefs), node-1 none."""
    from randobj import make_groups, make_nodes, make_pods, make_states
    rng = random.Random(seed)
    groups = make_groups(rng, 40)
    groups[2]["dry_mode"] = True
    nodes = make_nodes(rng, 300, groups)
    pods = make_pods(rng, 4000, groups)
    for i, p in enumerate(pods):
        r = rng.random()
        p["node_name"] = "node-0" if i < 70 else ("" if r < 0.15 else "node-%d" % rng.randrange(2, 300))
    return rng, groups, make_states(rng, len(groups)), pods, nodes


def node_cap(n_loaded, spare=SPARE):
    """The node table's capacity after a load of n nodes (esc_set_spare; include/escalator_hip.h)."""
    return n_loaded + (int(math.ceil(n_loaded * spare)) + 64 if spare > 0 else 0)


def pair_counts(N, n_gp):
    """Live (node, group pair) incidences per pair, from a packed node SoA."""
    f = N["flags"].astype(np.int64)
    cnt = np.zeros(n_gp, np.int64)
    l0 = N["label0"].astype(np.int64)
    np.add.at(cnt, l0[l0 < n_gp], 1)
    xl = N["xl_pair"].astype(np.int64)
    np.add.at(cnt, xl[xl < n_gp], 1)
    assert ((f >> 8) & 0xFF).sum() == len(xl)
    return cnt


def expected_counts(N, groups, n_cap, ranks=1):
    """esc_audit's n_checked per check, computed from the SoA arrays alone."""
    from oracle import soa
    t = soa.group_tables(groups)
    cnt = pair_counts(N, t["n_gp"])
    inc = int(cnt.sum())
    return {"ENTRY": ranks * inc, "OCC": ranks * inc, "REGION": int(cnt[t["gpair"].astype(np.int64)].sum()),
            "FIRST": t["G"], "TRACKER": ranks * n_cap, "MIRROR": ranks * n_cap}


def load_small(esc, trackers=True):
    """The small context, resident: loaded, placed, one decision taken (the K1 plan and with it
    the touch tables exist from the first step on)."""
    from escalator_amd.objects import placement
    from randobj import make_trackers
    rng, groups, states, pods, nodes = small_cluster()
    trk = make_trackers(rng, groups, nodes) if trackers else {}
    ctx = esc.Context(groups)
    ctx.set_spare(SPARE)
    P, N = ctx.pack(pods, nodes, trk)
    ctx.load(P, N)
    ctx.load_placement(*placement(pods, nodes))
    ctx.decide_all(states)
    return ctx, groups, states, pods, nodes, P, N


def _poke(lib, ctx, what, index, value):
    return lib.esc_debug_poke(ctx.handle, what, index, value)


def _first_ok(lib, ctx, what, value, limit=1 << 20):
    """The lowest index the poke accepts (it refuses everything that is not a live target)."""
    for i in range(limit):
        if _poke(lib, ctx, what, i, value(i) if callable(value) else value) == 0:
            return i
    raise AssertionError("no index accepted for poke %d" % what)


def mode_poke(lib, esc, target):
    from oracle import soa
    ctx, groups, states, pods, nodes, P, N = load_small(esc)
    t = soa.group_tables(groups)
    before = ctx.audit()
    assert all(v["n_bad"] == 0 for k, v in before.items() if k != "skipped") and not before["skipped"], before
    what, aux = POKES[target], {}
    if target == "entry_flags":
        ident = _first_ok(lib, ctx, what, 1)
    elif target == "entry_cpu":
        ident = _first_ok(lib, ctx, what, 123457)
    elif target == "region_flags":
        ident = _first_ok(lib, ctx, what, 2)
    elif target == "region_swap":
        ident = _first_ok(lib, ctx, what, 0) + 1            # the second word now sorts before the first
    elif target == "occ":
        words = ctx.reap_download()
        ident = _first_ok(lib, ctx, what, lambda i: int(words[i]) + 1, limit=len(words) // 2)
    elif target == "touch":
        for col in range(t["n_gp"] // 32 + 2):               # workgroup 0's first touched column
            if _poke(lib, ctx, what, 0, col) == 0:
                break
        else:
            raise AssertionError("workgroup 0 touches no column")
        ident = (0 << 32) | col
    elif target == "node_tracked":
        # an untracked live node of at least one group pair: its bit flipped ON in the table
        f = N["flags"].astype(np.int64)
        own = np.repeat(np.arange(len(f)), (f >> 8) & 0xFF)
        xl = N["xl_pair"].astype(np.int64)
        ident = next(j for j in range(len(f)) if not f[j] & 4 and
                     (N["label0"][j] < t["n_gp"] or (xl[own == j] < t["n_gp"]).any()))
        pairs = [int(q) for q in [N["label0"][ident]] + list(xl[own == ident]) if q < t["n_gp"]]
        aux["incidences"] = len(pairs)
        aux["wet_memberships"] = sum(1 for g in range(t["G"]) if int(t["gpair"][g]) in pairs and not t["dry"][g])
        assert _poke(lib, ctx, what, ident, 0) == 0
    elif target == "first_cpu":
        cnt = pair_counts(N, t["n_gp"])
        ident = next(g for g in range(t["G"]) if cnt[int(t["gpair"][g])] > 0)
        assert _poke(lib, ctx, what, ident, 777) == 0
    elif target == "host_ncpu":
        ident = 7
        assert _poke(lib, ctx, what, ident, 999983) == 0
    # everything outside the table of targets is refused
    refused = [_poke(lib, ctx, 9, 0, 0), _poke(lib, ctx, -1, 0, 0), _poke(lib, ctx, 0, -1, 1), _poke(lib, ctx, 0, 1 << 40, 1),
               _poke(lib, ctx, 3, 1 << 40, 0), _poke(lib, ctx, 6, 1 << 40, 0), _poke(lib, ctx, 7, t["G"], 1)]
    return {"id": int(ident), "report": ctx.audit(), "aux": aux, "refused": refused}


def mode_heal(lib, esc):
    import test_gpu_resident as R
    from escalator_amd.controller import ResidentController

    class Poked(ResidentController):
        poked = None

        def _audit(self):
            if self.audits == 2:                               # flushed, not yet audited: the third scan
                words = self.ctx.reap_download()
                Poked.poked = _first_ok(lib, self.ctx, POKES["occ"], lambda i: int(words[i]) + 1, limit=len(words) // 2)
            super()._audit()

    def resident(groups, clock, actuator, spare):
        return Poked(groups, clock=clock, actuator=actuator, spare=spare, audit_every=1)

    # drive() asserts on every scan that the two controllers' records, states and trackers are
    # equal and equal the literal oracle: the healing scan and every later one included
    ra, rb, seen, reloads = R.drive(1, 2.0, resident, R._reload, burst=True)
    return {"reload_causes": ra.events.reload_causes, "reloads": reloads, "audits": ra.audits,
            "audit_failures": ra.audit_failures, "scans": R.SCANS, "poked": Poked.poked,
            "last_clean": all(v["n_bad"] == 0 for k, v in ra.last_audit.items() if k != "skipped")}


def mode_skips(lib, esc):
    from escalator_amd.objects import placement
    rng, groups, states, pods, nodes = small_cluster()
    ctx = esc.Context(groups)
    ctx.set_spare(SPARE)
    P, N = ctx.pack(pods, nodes)
    out = {"unloaded_rc": lib.esc_audit(ctx.handle, 0, C.byref(esc._lib.AuditReport()))}
    ctx.load(P, N)
    out["loaded"] = ctx.audit()["skipped"]                     # no plan, no placement
    out["asked_tracker_only"] = ctx.audit(["TRACKER"])
    # no valid age index: the listing's look-back is made to give up (it has one only with
    # several tiles of nodes, hence the larger snapshot)
    s = esc.Synth(100_000, 300_000, 30, config=5, seed=0xE5CA1A7E00000005)
    big = esc.Context(s)
    big.load_synth(s)
    esc._lib.check(lib.esc_debug_lookback_fail(big.handle, 0, 1))
    out["build_rc"] = lib.esc_build_age_index(big.handle)
    out["no_index"] = big.audit()["skipped"]
    big.build_age_index()
    out["index_again"] = big.audit()["skipped"]
    big.close()
    ctx.load_placement(*placement(pods, nodes))
    out["placed"] = ctx.audit()["skipped"]
    ctx.decide_all(states)
    rep = ctx.audit()
    out["resident"] = rep["skipped"]
    out["resident_clean"] = all(v["n_bad"] == 0 for k, v in rep.items() if k != "skipped")
    return out


if __name__ == "__main__":
    import escalator_amd as esc
    from escalator_amd import _lib as L
    lib = L.load()
    assert hasattr(lib, "esc_debug_poke"), "not the measurement library: %s" % L.LIB_PATH
    lib.esc_debug_poke.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64]
    lib.esc_debug_poke.restype = C.c_int32
    lib.esc_debug_lookback_fail.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    if sys.argv[1] == "poke":
        res = mode_poke(lib, esc, sys.argv[2])
    else:
        res = {"heal": mode_heal, "skips": mode_skips}[sys.argv[1]](lib, esc)
    print(json.dumps(res), flush=True)
