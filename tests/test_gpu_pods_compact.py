"""GPU: esc_pods_compact — the pod side of the resident snapshot re-homed, re-cut and re-sorted on
the device.

Each pod sits under its own group pair (tests/test_gpu_pods_grow.py's ``fmt_pod``) or a few pods
under known pairs (``PodWorld``), and pod requests are pairwise distinct, so a misplaced or lost
pod changes a total and a delete or upsert aimed through a wrong position shows in the sums.
After the call every case is compared with the C oracle, the literal oracle (every group of the
small worlds, a sample of the large ones) and a fresh load of the same live pods at the same
spare: totals and decisions bit for bit, esc_stream_bytes equal to the fresh load's and to
layout.pod_bytes, esc_pods_room equal to the fresh load's, a clean esc_audit.

The injected failure before the swap and the stale context run in a child process on the
measurement library (tests/pods_compact_child.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from escalator_amd import layout
from oracle import oracle as O
from oracle import soa
from test_gpu_audit import assert_decision
from test_gpu_pods_grow import (CLASS_ID, E_LIMIT, KEY, MEASURE, PodWorld, _in, c_pod, code_of, fmt_pod, four_pools,
                                room, small_pods, tiles)
from test_gpu_rebuild import group, node, pod

pytestmark = pytest.mark.gpu
soa.build()

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NONE = 0xFFFFFFFF
SMALL0, INERT0 = 256, 384
# class id = signature | packed << 7, signature = regular * 32 + init * 8 + overhead * 4 + extra pairs
PLAIN = ["k%d%d" % (r, x) for r in (1, 2, 3) for x in range(4)]               # plain, r records x 0..3 extra pairs
CLS = dict(CLASS_ID, ds=INERT0, p12x1=129, p12x2=130, p12x3=131, **{k: int(k[1]) * 32 + int(k[2]) for k in PLAIN})
AUDIT = ["ENTRY", "FIRST", "REGION", "TOUCH", "TRACKER", "MIRROR"]          # (OCC needs a placement)


@pytest.fixture(scope="module")
def esc():
    import escalator_amd
    return escalator_amd


def mk(kind, i, n_groups):
    """fmt_pod and more kinds: the 12-B packed block with 1..3 extra pairs (p12x<pairs>), every
    plain class of 1..3 records and 0..3 extra pairs (k<records><pairs>), a daemonset pod (the
    inert class)."""
    if kind.startswith("p12x"):
        p = fmt_pod("s" + kind[4], i, n_groups)
        return dict(p, containers=[{"cpu": 200 + i % 900, "mem": (17 << 30) + i}])
    if kind in PLAIN and kind not in ("k11", "k33"):
        p = fmt_pod("s" + kind[2], i, n_groups)               # its pairs; a first container outside the packed ranges
        return dict(p, containers=[{"cpu": (1 << 20) + i, "mem": 5}] +
                    [{"cpu": 3 + k, "mem": 7 + i + k} for k in range(int(kind[1]))])
    if kind == "ds":
        return dict(fmt_pod("s0", i, n_groups), owner_kinds=["DaemonSet"])
    return fmt_pod(kind, i, n_groups)


def check_literal(esc, groups, pods, nodes, tot, dec, sample):
    for g in sample:
        L = O.scale_node_group(groups[g], {}, pods, nodes, tracker=[])
        assert (int(tot["n_pods"][g]), int(tot["n_nodes"][g])) == (L["n_pods"], L["n_nodes"]), g
        if L["pod_cpu_m"] is not None:
            assert (int(tot["pod_cpu_m"][g]), int(tot["pod_mem_b"][g])) == (L["pod_cpu_m"], L["pod_mem_b"]), g
        assert esc._lib.BRANCHES[int(dec["branch"][g])] == L["branch"], g


def clean_audit(ctx, checks=AUDIT):
    rep = ctx.audit(checks)
    assert rep["skipped"] == [] and all(rep[k]["n_bad"] == 0 for k in rep if k != "skipped"), rep


def same_as_fresh(esc, ctx, groups, P, N, spare, flush=False, vacated=0):
    """A fresh context loaded with the same live pods at the same spare: the same decision bytes,
    stream bytes (layout.pod_bytes too), room (capacity, free, free per class; the C section keeps
    its size, so the `vacated` C slots are free ones a fresh load does not have); returns the fresh
    context's k1_flush_entries."""
    fresh = esc.Context(groups)
    fresh.set_spare(spare)
    fresh.load(P, N)
    a, b = ctx.decide_all(None), fresh.decide_all(None)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert ctx.stream_bytes() == fresh.stream_bytes()
    n_gp = soa.group_tables(groups)["n_gp"]
    assert ctx.stream_bytes()[0] == layout.pod_bytes(P, n_gp)
    ours, theirs = room(ctx), room(fresh)
    assert ours[:2] == theirs[:2] and ours[3] == theirs[3] and ours[2] == theirs[2] + vacated
    fl = fresh.k1_flush_entries() if flush else None
    fresh.close()
    return fl


# ------------------------------------------------------------------ burst and drain
# (kind, pods loaded, the class-relative positions deleted): every pod under its own pair, in
# pair order, so a class's k-th pod sits at position k after the load
DRAIN = [
    ("s0", 769, list(range(256))),                                  # a whole free first tile -> 513
    ("s1", 512, list(range(255, 512))),                             # a whole free last tile and a tile's end -> 255
    ("s2", 300, list(range(100, 144))),                             # a tile's middle -> 256
    ("s3", 287, list(range(30))),                                   # a tile's start -> 257: two tiles stay
    ("p12", 600, list(range(3, 600, 6))[:87]),                      # holes everywhere -> 513: three tiles stay
    ("p12x2", 260, [0, 100, 255, 256, 259]),                        # -> 255
    ("k00", 257, []),                                               # untouched: two tiles stay
    ("k11", 300, list(range(212, 256))),                            # a tile's end -> 256
    ("k21", 258, [1]),                                              # -> 257
    ("k33", 270, list(range(0, 30, 2))),                            # -> 255
    ("ds", 300, list(range(257, 300))),                             # the inert class -> 257
]
# the rest of the matrix (12-B packed with 1 and 3 pairs, plain with 1..3 records x 0..3 pairs), by
# turns 260 -> 255 pods (a tile goes) and 258 -> 257 (two tiles stay)
REST = ["p12x1", "p12x3"] + [k for k in PLAIN if k not in ("k11", "k21", "k33")]
DRAIN += [(k, 260, [0, 100, 255, 256, 259]) if j % 2 == 0 else (k, 258, [1]) for j, k in enumerate(REST)]
LIVE = {"s0": 513, "s1": 255, "s2": 256, "s3": 257, "p12": 513, "p12x2": 255, "k00": 257, "k11": 256, "k21": 257,
        "k33": 255, "ds": 257}
LIVE.update({k: 255 if j % 2 == 0 else 257 for j, k in enumerate(REST)})


@pytest.fixture(scope="module")
def drain(esc):
    # (three groups without a pod behind the last one: the last pods' extra pairs do not wrap round
    # to pair 0, so every pod's first pair is its own group's and pair order is pod order)
    n_total = sum(n for _, n, _ in DRAIN) + 3
    groups = [dict(group("g%d" % i, key=KEY, value="c%d" % i)) for i in range(n_total)]
    pods, gone, first = [], [], {}
    for kind, n, holes in DRAIN:
        first[kind] = len(pods)
        gone += [len(pods) + q for q in holes]
        pods += [mk(kind, len(pods) + k, n_total) for k in range(n)]
    nodes = [node("n%d" % j, {KEY: "c%d" % (j * 37 % n_total)}, j) for j in range(64)]
    dead = set(gone)
    live = [p for i, p in enumerate(pods) if i not in dead]
    ctx = esc.Context(groups, device=-1)
    P0, N = ctx.pack(pods, nodes)
    P1, _ = ctx.pack(live, nodes)
    ctx.close()
    assert [len(h) for _, _, h in DRAIN] == [n - LIVE[k] for k, n, _ in DRAIN]
    return {"groups": groups, "pods": pods, "live": live, "nodes": nodes, "gone": gone, "first": first, "P0": P0,
            "P1": P1, "N": N}


@pytest.mark.parametrize("variant", ["plain", "force_wide", "graph_replicas", "calibrated"])
def test_burst_and_drain_every_format(esc, drain, variant):
    D = drain
    groups = D["groups"]
    reps = 3 if variant == "graph_replicas" else 1
    ctx = esc.Context(groups)
    ctx.set_spare(0.0)
    ctx.load(D["P0"], D["N"], replicas=reps)
    if variant == "force_wide":
        ctx.force_wide(True)
    if variant == "graph_replicas":
        ctx.use_graph(True)
    if variant == "calibrated":
        ctx.k1_calibrate(2)
    assert_decision(ctx, None, D["P0"], D["N"], groups)
    for kind, n, _ in DRAIN:                                   # the load put a class's k-th pod at position k
        assert ctx.pod_where(D["first"][kind] + n - 1) == (CLS[kind], n - 1), kind
    ctx.pods_delete(D["gone"])
    s = ctx.pods_slack()
    assert s == {"k_tiles": sum(tiles(n) for _, n, _ in DRAIN), "k_tiles_rule": sum(tiles(v) for v in LIVE.values()),
                 "parked": 0}
    before = ctx.decide_all(None)
    where0 = {i: ctx.pod_where(i) for i in range(len(D["pods"]))}
    rep = ctx.pods_compact()
    # tiles by the rule: they fell where a tile emptied and nowhere else
    r = ctx.pods_room()
    for kind, n, _ in DRAIN:
        assert r["per_class"][CLS[kind]] == tiles(LIVE[kind]) * 256 - LIVE[kind], kind
    assert rep["k_tiles_before"] == s["k_tiles"] and rep["k_tiles_after"] == s["k_tiles_rule"] == r["k_capacity"] // 256
    assert [tiles(n) - tiles(LIVE[k]) for k, n, _ in DRAIN] == [1, 1, 1, 0, 0, 1, 0, 1, 0, 1, 0] + [1, 0] * 5 + [1]
    assert rep["rehomed"] == 0 and rep["classes_created"] == 0 and rep["c_free_before"] == rep["c_free_after"] == 0
    assert rep["k1_bytes_after"] < rep["k1_bytes_before"]
    assert ctx.pods_slack() == {"k_tiles": s["k_tiles_rule"], "k_tiles_rule": s["k_tiles_rule"], "parked": 0}
    # every pod's position is the rule's: the live pods of a class close up in old-position order
    # (their buckets ascend with the old positions here)
    ids = [i for i in range(len(D["pods"])) if i not in set(D["gone"])]
    dead = set(D["gone"])
    moved = 0
    for kind, n, holes in DRAIN:
        nxt = 0
        for k in range(n):
            i = D["first"][kind] + k
            if i in dead:
                assert ctx.pod_where(i) == (-2, -1)
                continue
            assert ctx.pod_where(i) == (CLS[kind], nxt), (kind, k)
            moved += where0[i] != (CLS[kind], nxt)
            nxt += 1
    assert rep["moved"] == moved > 0
    for _ in range(reps):                                      # every replica
        assert_decision(ctx, None, D["P1"], D["N"], groups)
    after = ctx.decide_all(None)
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    check_literal(esc, groups, D["live"], D["nodes"], after[0], after[1],
                  [D["first"][k] for k, _, _ in DRAIN] + [D["first"][k] + n - 1 for k, n, _ in DRAIN])
    clean_audit(ctx)
    same_as_fresh(esc, ctx, groups, D["P1"], D["N"], 0.0)
    # a second compaction right after the first moves nothing and changes no byte of the answer
    rep2 = ctx.pods_compact()
    assert rep2["moved"] == 0 and rep2["rehomed"] == 0 and rep2["k_tiles_before"] == rep2["k_tiles_after"]
    again = ctx.decide_all(None)
    assert again[0].tobytes() == after[0].tobytes() and again[1].tobytes() == after[1].tobytes()
    # events go on through the new positions: a moved pod deleted, one upserted into another class
    # across a tile edge (s0's last pod, position 512 of 513, becomes a 12-B packed pod), a new id
    last_s0 = D["first"]["s0"] + 768
    assert ctx.pod_where(last_s0) == (CLS["s0"], 512)
    live = {i: D["pods"][i] for i in ids}
    victim = D["first"]["s2"] + 299
    ctx.pods_delete([victim])
    del live[victim]
    live[last_s0] = mk("p12", last_s0, len(groups))
    live[len(D["pods"])] = mk("s1", D["first"]["s1"] + 300, len(groups))
    B, _ = ctx.pack([live[last_s0], live[len(D["pods"])]], [])
    assert ctx.pods_upsert([last_s0, len(D["pods"])], B) == 0
    assert ctx.pod_where(last_s0) == (CLS["p12"], 513) and ctx.pod_where(len(D["pods"])) == (CLS["s1"], 255)
    P2, _ = ctx.pack([live[i] for i in sorted(live)], D["nodes"])
    for _ in range(reps):
        assert_decision(ctx, None, P2, D["N"], groups)
    clean_audit(ctx)
    ctx.close()


def test_a_class_drops_to_no_tile_at_spare_zero_and_keeps_its_index(esc, drain):
    D = drain
    groups = D["groups"]
    ctx = esc.Context(groups)
    ctx.set_spare(0.0)
    ctx.load(D["P0"], D["N"])
    lo = D["first"]["s2"]
    gone = list(range(lo, lo + 300))                           # every pod of the 2-pair packed small class
    ctx.pods_delete(gone)
    t0 = ctx.pods_room()["k_capacity"] // 256
    rep = ctx.pods_compact()
    assert rep["k_tiles_after"] == t0 - 2 and ctx.pods_room()["per_class"][CLS["s2"]] == 0   # a class, no position
    live = [p for i, p in enumerate(D["pods"]) if not lo <= i < lo + 300]
    P, _ = ctx.pack(live, D["nodes"])
    assert_decision(ctx, None, P, D["N"], groups)
    clean_audit(ctx)
    # a pod of the class again: no room in place, esc_pods_grow gives the class a tile
    B, _ = ctx.pack([D["pods"][lo]], [])
    assert ctx.pods_upsert([lo], B) == E_LIMIT
    ctx.pods_grow([lo], B)
    assert ctx.pods_upsert([lo], B) == 0 and ctx.pod_where(lo) == (CLS["s2"], 0)
    P, _ = ctx.pack([D["pods"][lo]] + live, D["nodes"])
    assert_decision(ctx, None, P, D["N"], groups)
    clean_audit(ctx)
    ctx.close()


# ------------------------------------------------------------------ parked pods
def ds_pod(name, pool, i):
    return dict(pod(name, pool, "n%d" % (i % 12), cpu=700 + i), owner_kinds=["DaemonSet"])


def run_parked(esc, devices=None):
    """300 packed-small pods at spare 0.25 (212 free positions, 16 spare C slots) and 70 pods that
    need a C slot (5 or 6 containers).  220 more small pods: 8 of them park in spare C slots; 3 daemonset pods park
    too (the load had no inert pod: no inert class).  No pods_grow before the compaction."""
    groups, nodes = four_pools()
    pools = ["one", "some", "dry"]
    base = small_pods(300) + [c_pod("wide%d" % i, i, pools, "n%d" % (i % 12), containers=5 + i % 2, pairs=1 + i % 3)
                              for i in range(70)]
    w = PodWorld(esc, groups, base, nodes, 0.25, devices=devices)
    k = len(devices) if devices else 1
    # (two devices: the new ids are the last device's, whose class holds 115 pods and 141 free positions)
    n_more = 220 if k == 1 else 149
    more = small_pods(n_more, 1000, bound=lambda i: i % 11 == 3)   # few bound (the runs' spare room); p1213 parks bound
    ids = list(range(370, 370 + n_more))
    assert w.upsert(ids, more) == 0
    ds = [ds_pod("ds%d" % i, pools[i % 3], i) for i in range(3)]
    d0 = 370 + n_more
    assert w.upsert([d0, d0 + 1, d0 + 2], ds) == 0
    # the same numbers on one device and on two (there every parked pod is the last device's: its
    # class held 115 pods and 141 free positions, the first device's shard has nothing parked)
    assert w.ctx.pods_slack()["parked"] == 11
    assert [w.ctx.pod_where(i)[0] for i in (d0 - 9, d0 - 8, d0 - 1, d0, d0 + 2)] == [SMALL0, -1, -1, -1, -1]
    c_free = w.ctx.pods_room()["c_free"]
    assert c_free == (32 if k == 1 else 16 + 32) - 11          # max(16, ceil(70 * 0.25)) -> two spare tiles; 16 beside no C pod
    wide = {i: w.ctx.pod_where(i) for i in range(300, 370)}
    assert all(v[0] == -1 for v in wide.values())
    w.check("parked")
    rep = w.ctx.pods_compact()
    assert w.ctx.pods_slack()["parked"] == 0
    assert rep["rehomed"] == 11 and rep["classes_created"] == 1 and rep["moved"] >= 11
    assert rep["c_free_after"] == rep["c_free_before"] + 11 == w.ctx.pods_room()["c_free"] == c_free + 11
    # the classes the layout predicts; the re-homed pods follow the residents of their bucket
    # (every pod here has pair 0, 1, 2 or none: bucket 0 or the last)
    P, _ = w.ctx.pack([w.pods[i] for i in range(d0 + 3)], [])
    want = layout.class_ids(P, soa.group_tables(groups)["n_gp"])
    for i in (0, 299, 370, d0 - 9, d0 - 8, d0 - 1, d0, d0 + 1, d0 + 2):
        assert w.ctx.pod_where(i)[0] == want[i], i
    assert [int(want[i]) for i in (d0 - 8, d0)] == [SMALL0, INERT0]
    assert [w.ctx.pod_where(i)[1] for i in (d0, d0 + 1, d0 + 2)] == [0, 1, 2]
    # a pod that needs its C slot stays (the parked pods' PodRefs were indirect: a spare slot has
    # room for 6 pairs; check() compares esc_try_remove with the oracle before and after)
    assert {i: w.ctx.pod_where(i) for i in range(300, 370)} == wide
    w.check("compacted")
    rep2 = w.ctx.pods_compact()
    assert (rep2["moved"], rep2["rehomed"], rep2["classes_created"]) == (0, 0, 0)
    w.check("compacted twice", fresh=False)
    # events after the move: pods that were re-homed, pods that stayed, a C pod; binds
    w.delete([d0 - 8, d0, 5, 301])
    assert w.upsert([d0 - 7, 6, d0 + 3], small_pods(3, 5000)) == 0
    w.bind([d0 - 6, d0 + 1, 7, 302], ["n3", "n4", "", "n5"])
    w.check("events after")
    return w


def test_parked_pods_go_home(esc):
    run_parked(esc)


def test_multi_device_context(esc):
    """devices=[0, 0]: every device's shard is compacted; the ids above the load belong to the
    last device's shard."""
    run_parked(esc, devices=[0, 0])


def test_rehomed_pods_create_their_classes_at_spare_zero(esc):
    """Loaded at spare 0: classes only for the formats present.  76 C pods; six of them are
    upserted with K shapes whose classes the context lacks, so each stays in its own C slot
    (its records and pairs first in the slot's room, the rest neutral).  The compaction creates
    the five classes in ascending class id and writes each pod in its format."""
    n_groups = 400
    groups = [dict(group("g%d" % i, key=KEY, value="c%d" % i)) for i in range(n_groups)]
    nodes = [node("n%d" % j, {KEY: "c%d" % (j * 37 % n_groups)}, j) for j in range(32)]

    def big(i):
        p = fmt_pod("s0", i, n_groups)
        return dict(p, containers=[{"cpu": 10 + i + k, "mem": (1 << 20) + k} for k in range(5)],
                    affinity=_in(KEY, ["c%d" % ((i + 1 + k) % n_groups) for k in range(5)]))
    pods = [mk("s0", i, n_groups) for i in range(300)] + [big(i) for i in range(300, 376)]
    ctx = esc.Context(groups)
    ctx.set_spare(0.0)
    P0, N = ctx.pack(pods, nodes)
    ctx.load(P0, N)
    kinds = {300: "s2", 310: "p12", 320: "k11", 330: "k33", 340: "ds", 375: "s0"}
    for i, kind in kinds.items():
        pods[i] = mk(kind, i, n_groups)
    B, _ = ctx.pack([pods[i] for i in kinds], [])
    assert ctx.pods_upsert(list(kinds), B) == 0
    where = {i: ctx.pod_where(i) for i in kinds}
    assert where[375][0] == SMALL0 and all(where[i] == (-1, i - 300) for i in kinds if i != 375)   # s0 had room
    assert ctx.pods_slack()["parked"] == 5
    P1, _ = ctx.pack(pods, nodes)
    assert_decision(ctx, None, P1, N, groups)
    rep = ctx.pods_compact()
    # (one C slot was free already: pod 375 left its own for the packed small class at the upsert)
    assert (rep["rehomed"], rep["classes_created"], rep["c_free_before"], rep["c_free_after"]) == (5, 5, 1, 6)
    want = layout.class_ids(P1, n_groups)
    for i, kind in kinds.items():
        assert ctx.pod_where(i)[0] == want[i] == CLS[kind], (i, kind)
        if i != 375:
            assert ctx.pod_where(i)[1] == 0
    assert ctx.pod_where(301) == (-1, 1)                       # the others keep their slots
    assert ctx.pods_slack()["parked"] == 0
    tot, dec = ctx.decide_all(None)
    assert_decision(ctx, None, P1, N, groups)
    check_literal(esc, groups, pods, nodes, tot, dec, list(kinds) + [301, 302, 0])
    clean_audit(ctx)
    same_as_fresh(esc, ctx, groups, P1, N, 0.0, vacated=6)
    # a freed slot takes a C pod again, a re-homed pod changes class, another is deleted
    pods.append(big(376))
    B, _ = ctx.pack([pods[376]], [])
    assert ctx.pods_upsert([376], B) == 0 and ctx.pod_where(376) == (-1, 0)      # the lowest freed slot first
    pods[310] = mk("k11", 310, n_groups)                      # a re-homed pod changes class: beside the other one
    B, _ = ctx.pack([pods[310]], [])
    assert ctx.pods_upsert([310], B) == 0 and ctx.pod_where(310) == (CLS["k11"], 1)
    ctx.pods_delete([330])
    live = [p for i, p in enumerate(pods) if i != 330]
    P2, _ = ctx.pack(live, nodes)
    assert_decision(ctx, None, P2, N, groups)
    clean_audit(ctx)
    ctx.close()


# ------------------------------------------------------------------ the order
def order_case(esc, n_groups, n_pods, pairs):
    groups = [dict(group("g%d" % i, key=KEY, value="c%d" % i)) for i in range(n_groups)]
    nodes = [node("n%d" % j, {KEY: "c%d" % (j * 37 % n_groups)}, j) for j in range(16)]
    kind = "s%d" % pairs

    def under(i, g):                                           # pod i under group g's pair, its request its own
        return dict(mk(kind, g, n_groups), name="o%d" % i, containers=[{"cpu": 100 + i % 900, "mem": (1 << 20) + i}])
    seed = [under(0, 0), under(1, n_groups - 1)]
    ctx = esc.Context(groups)
    ctx.set_spare(4.0)
    P0, N = ctx.pack(seed, nodes)
    ctx.load(P0, N)
    # filled by upserts in descending pair order: positions in arrival order, the buckets upside down
    step = max(1, n_groups // n_pods)
    late = [under(2 + i, (n_groups - 2 - step * i) % n_groups) for i in range(n_pods)]
    pods = seed + late
    ids = list(range(2, 2 + len(late)))
    B, _ = ctx.pack(late, [])
    if ctx.pods_upsert(ids, B) == E_LIMIT:
        ctx.pods_grow(ids, B)
        assert ctx.pods_upsert(ids, B) == 0
    P1, _ = ctx.pack(pods, nodes)
    n_gp = soa.group_tables(groups)["n_gp"]
    where0 = [ctx.pod_where(i) for i in range(len(pods))]
    assert len(set(c for c, _ in where0)) == 1 and where0[0][0] >= 0
    rep = ctx.pods_compact()
    want = layout.compact_positions([c for c, _ in where0], [q for _, q in where0], P1["pair0"], [1] * len(pods),
                                    [0] * len(pods), n_gp)
    got = [ctx.pod_where(i) for i in range(len(pods))]
    assert [q for _, q in got] == want.tolist() and [c for c, _ in got] == [c for c, _ in where0]
    assert rep["moved"] == sum(a != b for a, b in zip(got, where0)) > len(pods) // 2
    assert_decision(ctx, None, P1, N, groups)
    clean_audit(ctx)
    return ctx, groups, P1, N


@pytest.mark.parametrize("pairs", [0, 2])
def test_order_after_descending_upserts(esc, pairs):
    """72 groups: buckets 0, 1, 2 and the last.  Without extra pairs a pod touches one column, so
    the re-sorted tiles flush what a fresh load's do."""
    ctx, groups, P1, N = order_case(esc, 72, 600, pairs)
    fl = same_as_fresh_sorted(esc, ctx, groups, P1, N)
    if pairs == 0:
        assert ctx.k1_flush_entries() == fl
    ctx.close()


def same_as_fresh_sorted(esc, ctx, groups, P, N):
    fresh = esc.Context(groups)
    fresh.set_spare(4.0)
    fresh.load(P, N)
    a, b = ctx.decide_all(None), fresh.decide_all(None)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert ctx.stream_bytes() == fresh.stream_bytes() and room(ctx) == room(fresh)
    fl = fresh.k1_flush_entries()
    fresh.close()
    return fl


def test_order_over_two_k1_windows(esc):
    """20 480 group pairs: 641 buckets, two K1 windows, no packed small class; 320 pods."""
    ctx, groups, P1, N = order_case(esc, 20480, 320, 0)
    same_as_fresh_sorted(esc, ctx, groups, P1, N)
    ctx.close()


# ------------------------------------------------------------------ shards
def test_two_shards_only_one_compacts(esc):
    """Two sharded contexts (world 2) with the host exchange: rank 1 drains and compacts, rank 0
    does nothing.  No collective.  The merged decision equals the C oracle over every live pod."""
    from escalator_amd.dist import merge_owned
    from test_gpu import _packed_subset, check_against_c_oracle
    groups, nodes = four_pools()
    base = small_pods(1200)
    ctxs = []
    for r in range(2):
        c = esc.Context(groups, rank=r, world=2)
        c.set_spare(0.25)
        P, N = c.pack(base, nodes)
        c.load(_packed_subset(P, list(range(600 * r, 600 * r + 600))), N, pod_offset=600 * r)
        ctxs.append(c)
    c0, c1 = ctxs
    r0 = room(c0)
    gone = list(range(0, 600, 2)) + list(range(301, 400, 2))   # 350 of rank 1's 600 pods (shard-local ids)
    c1.pods_delete(gone)
    rep = c1.pods_compact()
    assert rep["k_tiles_after"] < rep["k_tiles_before"] and rep["moved"] > 0 and room(c0) == r0
    assert c1.pods_room()["per_class"][SMALL0] == tiles(250 + 62) * 256 - 250
    words, firsts = [], []
    for c in ctxs:
        c.set_state(None)
        c.reduce()
        w, f = c.exchange_download()
        words.append(w)
        firsts.append(f)
    W, F = np.sum(words, axis=0), np.min(firsts, axis=0)
    parts = []
    for c in ctxs:
        c.exchange_upload(W, F)
        c.decide()
        parts.append(c.results())
    tot, dec = merge_owned(parts)
    dead = set(600 + i for i in gone)
    P, N = c0.pack([p for i, p in enumerate(base) if i not in dead], nodes)
    otot = soa.totals(P, N, groups)
    odf, odi = soa.decide(groups, None, otot)
    check_against_c_oracle(tot, dec, otot, odf, odi)
    for c in ctxs:
        clean_audit(c)
        c.close()


# ------------------------------------------------------------------ refusals
def test_refusals(esc):
    L = esc._lib
    groups, nodes = four_pools()
    ctx = esc.Context(groups)
    assert code_of(esc, ctx.pods_compact) == L.ESC_E_STATE     # before a load
    assert code_of(esc, ctx.pods_slack) == L.ESC_E_STATE
    assert code_of(esc, ctx.pod_where, 0) == L.ESC_E_STATE
    ctx.set_spare(0.25)
    P, N = ctx.pack(small_pods(20), nodes)
    ctx.load(P, N)
    assert ctx.pod_where(19) == (SMALL0, 19) and ctx.pod_where(20) == (-2, -1) and ctx.pod_where(1 << 40) == (-2, -1)
    assert code_of(esc, ctx.pod_where, -1) == L.ESC_E_INVAL
    r0 = room(ctx)
    rep = ctx.pods_compact()                                   # a fresh load: nothing to do
    assert rep["moved"] == 0 and rep["k_tiles_before"] == rep["k_tiles_after"] and room(ctx) == r0
    ctx.close()
    nodev = esc.Context(groups, device=-1)
    assert code_of(esc, nodev.pods_compact) == L.ESC_E_NODEV
    assert code_of(esc, nodev.pods_slack) == L.ESC_E_NODEV
    nodev.close()


def test_a_failure_before_the_swap_changes_nothing_and_a_stale_context_refuses():
    assert os.path.exists(MEASURE), "build the measurement library: make -C escalator_amd/csrc ABLATIONS=1"
    env = dict(os.environ, ESC_LIB_PATH=MEASURE)
    try:
        r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "pods_compact_child.py")], capture_output=True,
                           text=True, timeout=240, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired:
        pytest.exit("pods_compact_child.py hung: nothing more is started on this GPU", 1)
    if r.returncode in (134, 139, -6, -11):                    # an abort or a fault: the session ends here
        pytest.exit("pods_compact_child.py died (%d): %s" % (r.returncode, r.stderr[-2000:]), 1)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    print(json.dumps(out))
    assert out["code"] == out["hip"], out
    assert out["audit_equal"] and out["room_equal"] and out["where_equal"] and out["answers_equal"], out
    assert out["moved_after"] > 0 and out["bad_after"] == [] and out["answers_after_equal"], out
    assert out["stale_code"] == out["e_state"], out


# ------------------------------------------------------------------ the controller
def _burst_then_drain(base, at, until, n):
    """tests/test_gpu_resident.py's FakeCluster whose history has n more pods from scan `at` to
    scan `until`."""
    class Bursty(base):
        def churn(self, scan, tracked):
            super().churn(scan, tracked)
            grp = self.rnd_groups[0]
            if scan == at:
                for i in range(n):
                    self.put_pod({"name": "pb%d" % i, "owner_kinds": [], "annotations": {},
                                  "node_selector": {grp["label_key"]: grp["label_value"]}, "affinity": None,
                                  "containers": [{"cpu": 50 + i % 20, "mem": 1 << 20}], "init_containers": [],
                                  "overhead": None, "node_name": ""})
            if scan == until:
                for i in range(n):
                    self.del_pod("pb%d" % i)
    return Bursty


def test_resident_controller_over_a_burst_then_drain_history(monkeypatch):
    """1 500 pods arrive at scan 2 (one pods_grow) and finish at scan 4: the classes shrink again
    by one pods_compact, no reload after the first load, every scan's records equal to the
    reloading Controller's and the literal oracle's (drive asserts both scan by scan)."""
    import test_gpu_resident as R
    from escalator_amd.controller import ResidentController
    monkeypatch.setattr(R, "FakeCluster", _burst_then_drain(R.FakeCluster, 2, 4, 1500))

    def resident(groups, clock, actuator, spare):
        return ResidentController(groups, clock=clock, actuator=actuator, spare=spare, pod_grow=True, pod_compact=0.25)
    ra, rb, seen, reloads = R.drive(1, 2.0, resident, R._reload, burst=False)
    ev = ra.events
    assert reloads == [1] * R.SCANS, (reloads, ev.reload_causes)
    assert ev.pod_grows == 1 and ev.pod_compacts >= 1 and ev.pod_compact_failures == 0, (ev.pod_grows, ev.pod_compacts)
    assert "slack" in ev.pod_compact_causes
    s = ra.ctx.pods_slack()
    assert s["parked"] == 0
