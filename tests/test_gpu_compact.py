"""GPU: esc_nodes_compact — the node table compacted and grown on the device.

``CWorld`` is tests/test_gpu_rebuild.py's ``World`` with a ``compact()`` that applies the returned
map to its name -> index table, so ``check`` compares everything the context answers with the
oracles on the live objects and with a fresh context on the live nodes, and requires a clean
audit, exactly as after a rebuild.  After a compaction ``check_compacted`` also asserts that the
context's raw indices are the fresh context's (0 .. L-1 in snapshot order, no name mapping) and
that every group's tracker list holds the tracked names' new indices.

The refusal with nothing swapped runs in a child process on the measurement library
(tests/compact_child.py)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import soa
from test_gpu_audit import CHECKS, assert_decision
from test_gpu_rebuild import E_LIMIT, MEASURE, T0, World, group, limit, node, pod, tainted

pytestmark = pytest.mark.gpu
soa.build()

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NO_DELETE = "atlassian.com/no-delete"


@pytest.fixture(scope="module")
def esc():
    import escalator_amd
    assert escalator_amd._lib.ESC_E_LIMIT == E_LIMIT
    return escalator_amd


def table_slots(n, f):
    return n + (int(math.ceil(n * f)) + 64 if f > 0 else 0)


class CWorld(World):
    def compact(self, min_free_slots=0, min_free_xl_words=0):
        """One esc_nodes_compact; the map is -1 for exactly the deleted slots, dense and
        ascending over the others, and is applied to the names."""
        old = dict(self.idx)
        m = self.ctx.nodes_compact(min_free_slots, min_free_xl_words)
        live = sorted(old.values())
        assert [j for j in range(len(m)) if m[j] >= 0] == live, (m, live)
        assert [int(m[j]) for j in live] == list(range(len(live)))
        self.idx = {name: int(m[j]) for name, j in old.items()}
        for i, p in enumerate(self.pods):                    # pods of deleted nodes' runs came out unbound
            if p is not None and p["node_name"] and p["node_name"] not in self.idx:
                self.pods[i] = dict(p, node_name="")
        return m

    def bind(self, ids, names):
        self.ctx.pods_bind(ids, [self.idx[m] if m else 0xFFFFFFFF for m in names])
        for i, m in zip(ids, names):
            self.pods[i] = dict(self.pods[i], node_name=m)

    def check_compacted(self, tag, **kw):
        names = [x["name"] for x in self.live()]
        assert self.idx == {m: j for j, m in enumerate(names)}, tag     # raw indices: a fresh load's
        got, rep = self.check(tag, **kw)
        for g in range(len(self.groups)):
            want = sorted(self.idx[m] for m in self.trk.get(g, []) if m in self.idx)
            assert self.ctx.tracker_list(g).tolist() == want, (tag, g)
        return got, rep


# ------------------------------------------------------------------ slot exhaustion by turnover
def turnover_world(esc, devices=None, graph=False):
    groups = [group("a"), group("b"), group("dry", dry_mode=True), group("default", key="", value="")]
    nodes = [node("n0", {"pool": "a"}, 0), tainted("n1", {"pool": "b"}, 1), tainted("n2", {"pool": "dry"}, 2),
             node("n3", {"pool": "a"}, 3), tainted("n4", {"pool": "dry"}, 4), node("n5", {"pool": "b"}, 5)]
    pods = [pod("p%d" % i, ["a", "b", "dry", ""][i % 4], ["n0", "n1", "n4", "", "n5"][i % 5]) for i in range(40)]
    return CWorld(esc, groups, pods, nodes, 0.25, devices=devices, trackers={2: ["n2", "n4"]}, graph=graph)


def run_turnover(esc, devices=None, graph=False, checks=True):
    w = turnover_world(esc, devices, graph)
    chk = (lambda tag: w.check(tag)) if checks else (lambda tag: None)
    assert w.ctx.nodes_room()[0] == 6 + 2 + 64 - 6 == 66
    w.check("load")
    k, rebuilds = 0, 0
    while w.ctx.nodes_room()[0] > 0:                           # one node comes, one goes: the size holds
        x = (tainted if k % 4 == 1 else node)("t%d" % k, {"pool": ["a", "b", "dry"][k % 3]}, 100 + k)
        try:
            w.add([x])
        except esc._lib.EscError as e:                         # a pair's spare entries ran out: a rebuild answers
            assert e.code == E_LIMIT and w.ctx.nodes_room()[0] > 0
            w.rebuild()
            rebuilds += 1
            w.add([x])
        if k >= 1:
            w.delete(["t%d" % (k - 1)])
        if k == 3:
            w.bind([3, 7], ["t3", "t3"])                      # t3's run holds pods when t3 is deleted
        k += 1
    assert k == 66 and rebuilds > 0
    chk("slots used up")
    last = node("t%d" % k, {"pool": "a"}, 100 + k)
    before = w.ctx.audit()
    limit(esc, w.add, [last])
    assert w.ctx.audit() == before                             # refused: the snapshot is untouched
    w.rebuild()                                                # a rebuild does not grow the table
    assert w.ctx.nodes_room()[0] == 0
    limit(esc, w.add, [last])
    w.check("refused after the rebuild")
    m = w.compact()
    assert len(m) == 72 and int((m < 0).sum()) == 65
    L = 7
    assert w.ctx.nodes_room()[0] == table_slots(L, 0.25) - L
    w.check_compacted("compacted")
    assert w.add([last]) == [L]
    w.check("the add after the compaction")
    return w


def test_turnover_runs_the_table_dry_and_compaction_refills_it(esc):
    """Four groups, 6 nodes, spare 0.25: 66 free slots, used up by 66 adds of which 65 are
    deleted again; the next add is refused, a rebuild does not help, the compaction gives
    table_slots(7, 0.25) - 7 free slots and the add takes index 7.  A captured graph is on:
    every check decides twice."""
    run_turnover(esc, graph=True)


@pytest.mark.parametrize("shards", [2, 3])
def test_turnover_multi_device(esc, shards):
    run_turnover(esc, devices=[0] * shards, checks=False)


# ------------------------------------------------------------------ growth
def test_growth_without_spare(esc):
    """f = 0: a load leaves no free slot and no spare word.  compact(5, 8) admits five nodes
    that carry extra labels (values of the groups' keys that no group selects: at f = 0 no group
    pair has a spare entry)."""
    groups = [group("a"), group("b"), group("hot", key="tier", value="hot"), group("default", key="", value="")]
    nodes = [node("n%d" % i, {"pool": "ab"[i % 2], "tier": "hot" if i % 3 == 0 else "warm"}, i) for i in range(9)]
    pods = [pod("p%d" % i, "ab"[i % 2], "n%d" % (i % 9)) for i in range(30)]
    w = CWorld(esc, groups, pods, nodes, 0.0)
    assert w.ctx.nodes_room() == (0, 0)
    new = [node("x%d" % i, {"pool": "zz%d" % i, "tier": "cold"}, 50 + i) for i in range(5)]
    limit(esc, w.add, new)
    w.delete(["n4"])
    m = w.compact(min_free_slots=5, min_free_xl_words=8)
    assert m.tolist() == [0, 1, 2, 3, -1, 4, 5, 6, 7]
    assert w.ctx.nodes_room() == (5, 8)
    w.check_compacted("grown")
    assert w.add(new) == [8, 9, 10, 11, 12]
    assert w.ctx.nodes_room() == (0, 3)                        # one extra-label word per new node
    w.check("five added")


# ------------------------------------------------------------------ edges of the gather
@pytest.mark.parametrize("cap", [255, 256, 257, 600])
@pytest.mark.parametrize("absent", ["first", "last", "alternating"])
def test_gather_capacity_edges(esc, cap, absent):
    """New capacity one below, at and one above one workgroup of the gather, and several."""
    groups = [group("a"), group("b", dry_mode=True)]
    n = 40
    nodes = [(tainted if i % 3 == 0 else node)("n%d" % i, {"pool": "ab"[i % 2]}, i) for i in range(n)]
    pods = [pod("p%d" % i, "ab"[i % 2], "n%d" % (i * 7 % n)) for i in range(60)]
    w = CWorld(esc, groups, pods, nodes, 0.0, trackers={1: ["n1", "n3", "n39"]})
    gone = {"first": range(0, 12), "last": range(28, 40), "alternating": range(0, 40, 2)}[absent]
    w.delete(["n%d" % i for i in gone])
    L = n - len(gone)
    w.compact(min_free_slots=cap - L)
    assert w.ctx.nodes_room()[0] == cap - L
    w.check_compacted("cap %d %s" % (cap, absent))


def test_live_nodes_behind_300_absent_slots(esc):
    groups = [group("a"), group("b")]
    nodes = [node("n%d" % i, {"pool": "ab"[i % 2]}, i) for i in range(306)]
    pods = [pod("p%d" % i, "ab"[i % 2], "n%d" % (300 + i % 6)) for i in range(24)]
    w = CWorld(esc, groups, pods, nodes, 0.5)
    w.delete(["n%d" % i for i in range(300)])
    m = w.compact()
    assert m[:300].tolist() == [-1] * 300 and m[300:].tolist() == list(range(6))
    assert w.ctx.nodes_room()[0] == table_slots(6, 0.5) - 6
    w.check_compacted("behind 300")


def test_empty_table_and_every_node_deleted(esc):
    groups = [group("a"), group("b")]
    w = CWorld(esc, groups, [pod("p0", "a")], [], 0.5)
    assert len(w.compact()) == 0
    w.check_compacted("empty")
    assert w.add([node("n0", {"pool": "a"}, 0), node("n1", {"pool": "b"}, 1)]) == [0, 1]
    w.bind([0], ["n1"])
    w.delete(["n0", "n1"])
    assert w.compact().tolist() == [-1, -1]
    got, rep = w.check_compacted("all deleted")
    assert rep["ENTRY"]["n_checked"] == 0 and got["first"] == [None, None]
    assert w.ctx.nodes_room()[0] == 64
    assert w.add([node("n2", {"pool": "a"}, 2)]) == [0]        # the numbering starts again
    w.bind([0], ["n2"])
    w.check("after")


# ------------------------------------------------------------------ edges of the run move
def test_run_lengths_dead_runs_and_a_full_run(esc):
    """Runs of 0, 1, 63, 64, 65 and 300 PodRefs (one wave's stride below, at and above it), a
    dead run between live ones whose pods come out unbound, pods on the nodes at both ends of
    the table, and a run filled to its capacity: a bind into it is refused before the compaction
    and succeeds after it."""
    groups = [group("a"), group("b"), group("default", key="", value="")]
    lens = [300, 0, 1, 63, 10, 64, 65, 5]
    nodes = [(tainted if i in (1, 4, 6) else node)("n%d" % i, {"pool": "ab"[i % 2]}, i) for i in range(8)]
    pods = []
    for j, k in enumerate(lens):
        pods += [pod("p%d-%d" % (j, i), ["a", "b", ""][i % 3], "n%d" % j) for i in range(k)]
    bound = len(pods)
    pods += [pod("u%d" % i, ["a", "b", ""][i % 3]) for i in range(100)]
    w = CWorld(esc, groups, pods, nodes, 0.25)
    cap = int(math.ceil(bound / 8 * 1.25)) + 4               # what the empty run of n1 got at the load
    free = list(range(bound, bound + cap))
    w.bind(free, ["n1"] * cap)
    limit(esc, w.ctx.pods_bind, [bound + cap], [w.idx["n1"]])
    w.check("n1 full")
    w.delete(["n4"])                                          # its ten pods wait in the dead run
    dead = [i for i, p in enumerate(w.pods) if p["node_name"] == "n4"]
    assert len(dead) == 10
    m = w.compact()
    assert m.tolist() == [0, 1, 2, 3, -1, 4, 5, 6]
    assert all(w.pods[i]["node_name"] == "" for i in dead)
    w.check_compacted("moved")
    w.bind([bound + cap], ["n1"])                             # the re-cut run has room: len + ceil(len f) + 2
    w.bind(dead[:2], ["n7", "n0"])                            # the unbound pods bind again, at both ends
    w.check("bound after")


# ------------------------------------------------------------------ what outlives it
def test_state_outlives_the_compaction(esc):
    """Tracked nodes on both sides of a deleted slot, instantiation times, taint times and
    no-delete bytes around the gaps, a node with no label, one carrying 70 group pairs, two
    groups on one pair, the default group; the K1 flush entries are equal; a second compaction
    is the identity with an equal audit and equal answers."""
    groups = [group("k%d" % i, key="k%d" % i, value="v") for i in range(70)] + \
             [group("x"), group("x2", value="x"), group("default", key="", value=""), group("y", dry_mode=True)]
    wide = node("wide", {"k%d" % i: "v" for i in range(70)}, 3)
    keep = {"annotations": {NO_DELETE: "true"}}
    nodes = [node("bare", {}, 0), node("low", {"pool": "y"}, 1), wide] + \
            [(tainted if i % 2 else node)("x%d" % i, {"pool": "x"}, 10 + i, **(keep if i == 3 else {})) for i in range(6)] + \
            [tainted("y%d" % i, {"pool": "y"}, 40 + i, **(keep if i == 2 else {})) for i in range(5)]
    pods = [pod("p%d" % i, ["x", "y", ""][i % 3], ["x1", "y1", "low", "", "x3", "y3"][i % 6]) for i in range(36)]
    w = CWorld(esc, groups, pods, nodes, 0.5, trackers={73: ["y0", "y2", "y4"]})
    w.instantiated(["x1", "x3", "y1", "y3", "wide"], [T0 - 10**9 * (i + 1) for i in range(5)])
    w.delete(["x2", "y1", "y3"])                               # y1 and y3 sit between the tracked nodes
    got, _ = w.check("before")
    flush = w.ctx.k1_flush_entries()
    owners = [w.ctx.group_owner(g) for g in range(0, 74, 9)]
    w.compact()
    got2, rep = w.check_compacted("after")
    assert got2 == got                                         # by name: every answer is what it was
    assert w.ctx.k1_flush_entries() == flush and [w.ctx.group_owner(g) for g in range(0, 74, 9)] == owners
    assert got2["first"][0] == "wide" and got2["first"][70] == "x0" and got2["first"][71] == "x0"
    assert w.ctx.tracker_list(73).tolist() == [w.idx["y0"], w.idx["y2"], w.idx["y4"]]
    m = w.compact()                                            # determinism: the identity, the same report
    assert m.tolist() == list(range(len(m)))
    got3, rep3 = w.check_compacted("again")
    assert got3 == got2 and rep3 == rep
    # node and pod events go on against the new numbering
    w.instantiated(["x5"], [T0 - 5])
    w.relabel([dict(w.rec["low"], labels={"pool": "x"})])
    w.bind([0, 1], ["x5", "low"])
    w.check("events after")


# ------------------------------------------------------------------ all or nothing (child process)
def test_a_table_that_disagrees_with_the_plan_is_refused_whole():
    assert os.path.exists(MEASURE), "build the measurement library: make -C escalator_amd/csrc ABLATIONS=1"
    env = dict(os.environ, ESC_LIB_PATH=MEASURE)
    try:
        r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "compact_child.py"), "refuse"], capture_output=True,
                           text=True, timeout=240, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired:
        pytest.exit("compact_child.py hung: nothing more is started on this GPU", 1)
    if r.returncode in (134, 139, -6, -11):                    # an abort or a fault: the session ends here
        pytest.exit("compact_child.py died (%d): %s" % (r.returncode, r.stderr[-2000:]), 1)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    print(json.dumps(out))
    assert out["code"] == out["hip"], out
    assert out["mirror_bad"] == 2 and out["other_bad"] == [], out      # the two pokes, reported before and after
    assert out["audit_equal"] and out["room_equal"] and out["answers_equal"], out


# ------------------------------------------------------------------ the queue and the controller
def _history(q, scan):
    """One scan's events: node t<scan> comes with a pod that names it, node t<scan - 1> goes."""
    q.node_add((tainted if scan % 5 == 0 else node)("t%d" % scan, {"pool": ["one", "some"][scan % 2]}, 100 + scan))
    q.pod_add(pod("late%d" % scan, ["one", "some"][scan % 2], "t%d" % scan))
    if scan:
        q.node_delete("t%d" % (scan - 1))
        q.pod_delete("late%d" % (scan - 1))


@pytest.mark.parametrize("compact", [True, False])
def test_event_queue_compacts_instead_of_reloading(esc, compact):
    """70 nodes turned over in a cluster of 6, every new node named by a pod: with compact on the
    queue reloads once (the first load), compacts when the slots run out and binds the late
    pods; with compact off the same history reloads."""
    from escalator_amd.events import EventQueue
    groups = [group("one"), group("some")]
    q, ctx = EventQueue(spare=0.25, rebuild=True, compact=compact), esc.Context(groups)
    for i in range(6):
        q.node_add(node("s%d" % i, {"pool": ["one", "some"][i % 2]}, i))
    for i in range(12):
        q.pod_add(pod("p%d" % i, ["one", "some"][i % 2], ["s0", "s1", ""][i % 3]))
    q.flush(ctx)
    for scan in range(70):
        _history(q, scan)
        q.flush(ctx)
        if scan % 23 == 0 or scan == 69:
            live = q.live_nodes()
            P, N = ctx.pack(q.live_pods(), live)
            assert_decision(ctx, None, P, N, groups, q.node_name, [x["name"] for x in live])
            rep = ctx.audit()
            assert rep["skipped"] == [] and all(rep[k]["n_bad"] == 0 for k in CHECKS), rep
    assert q.node_index("t69") is not None and q.pod_id("late69") is not None
    if compact:
        assert q.reloads == 1 and q.reload_causes == ["first"], q.reload_causes
        assert q.compactions >= 1 and set(q.compact_causes) == {"nodes_add"}, q.compact_causes
        assert max(q.node_index(m) for m in q.nodes) < 7 + 66   # the indices started again at a compaction
    else:
        assert q.compactions == 0 and q.reloads >= 2 and "nodes_add" in q.reload_causes
    ctx.close()


class _Turnover:
    """tests/test_gpu_resident.py's FakeCluster with another history: five nodes come on every
    scan, each named by a pod, and the five of the scan before go with their pods."""

    def __new__(cls, *a):
        import test_gpu_resident as R

        class T(R.FakeCluster):
            def churn(self, scan, tracked):
                now = self.clock()
                for g, n in self.pending:                      # the cloud's nodes register
                    grp = self.groups[g]
                    for _ in range(n):
                        self.serial += 1
                        self.put_node({"name": "cloud-%d" % self.serial, "labels": {grp["label_key"]: grp["label_value"]},
                                       "unschedulable": False, "taints": [], "cpu": 4000, "mem": 8 << 30, "created_ns": now})
                self.pending = []
                for i in range(5):
                    k = scan * 5 + i
                    pool = ["one", "some", "dry"][k % 3]
                    self.put_node(node("t%d" % k, {"pool": pool}, 100 + k))
                    self.put_pod(pod("late%d" % k, pool, "t%d" % k, cpu=1500))
                    self.del_node("t%d" % (k - 5))
                    self.del_pod("late%d" % (k - 5))
        return T(*a)


@pytest.mark.parametrize("compact", [True, False])
def test_resident_controller_compacts_instead_of_reloading(compact):
    """ResidentController(node_compact=True) in lock-step with the reloading Controller over a
    history that turns over 70 nodes of a 6-node cluster: equal records on every scan, one
    reload (the first load), a compaction when the slots run out, the trackers in place after
    it; with node_compact off (node_rebuild on) the same history reloads."""
    import copy
    import test_gpu_resident as R
    from escalator_amd.controller import Controller, ResidentController
    groups = [dict(group(n, dry_mode=(n == "dry"), max_nodes=12), scale_up_cool_down_ns=0,
                   soft_delete_grace_ns=R.SCAN_NS, hard_delete_grace_ns=3 * R.SCAN_NS + 1) for n in ("one", "some", "dry")]
    nodes = [(tainted if i == 4 else node)("s%d" % i, {"pool": ["one", "some", "dry"][i % 3]}, i) for i in range(6)]
    pods = [pod("p%d" % i, ["one", "some", "dry"][i % 3], ["s0", "s1", "s2", ""][i % 4], cpu=900) for i in range(12)]
    clock = [R.T0]
    A, B = (_Turnover(7, groups, groups, lambda: clock[0], False) for _ in range(2))
    ra = ResidentController(groups, clock=lambda: clock[0], actuator=A, spare=0.25, node_rebuild=True, node_compact=compact)
    rb = Controller(groups, clock=lambda: clock[0], actuator=B)
    A.sink, A.resolve = ra.events, ra.events.node_name
    B.resolve = lambda j: B.listed[j]
    for c in (A, B):
        for x in nodes:
            c.put_node(x)
        for p in pods:
            c.put_pod(p)
    for scan in range(15):                                     # the first five come with the first load
        A.churn(scan, [])
        B.churn(scan, [])
        assert list(A.nodes) == list(B.nodes) and A.pods == B.pods and A.nodes == B.nodes, scan
        rb._lock_states(clock[0])
        states, trackers = copy.deepcopy(rb.state), {g: list(t) for g, t in rb.taint_tracker.items()}
        cur_pods, cur_nodes = B.list_pods(), B.list_nodes()
        out_a = [R._record(r, A.resolve) for r in ra.run_once()]
        out_b = [R._record(r, B.resolve) for r in rb.run_once(B.list_pods, B.list_nodes)]
        assert [x["name"] for x in ra.events.live_nodes()] == [x["name"] for x in cur_nodes], scan
        for g in range(len(groups)):
            assert out_a[g] == out_b[g], (scan, g, out_a[g], out_b[g])
        assert ra.state == rb.state and ra.taint_tracker == rb.taint_tracker and ra.lock_time == rb.lock_time, scan
        R._check_literal(groups, states, trackers, cur_pods, cur_nodes, out_a, scan)
        for g, names in ra.taint_tracker.items():              # the device tracks every tracked live name
            want = {ra.events.node_index(m) for m in names} - {None}
            assert want <= set(int(j) for j in ra.ctx.tracker_list(g)), (scan, g)
        clock[0] += R.SCAN_NS
    ev = ra.events
    print(ev.reload_causes, ev.compact_causes, ev.rebuild_causes, ev.applied)
    if compact:
        assert ev.applied["nodes_add"] >= 70 and ev.applied["pods_bind"] >= 70
        assert ev.reloads == 1 and ev.reload_causes == ["first"], ev.reload_causes
        assert ev.compactions >= 1 and set(ev.compact_causes) == {"nodes_add"}, ev.compact_causes
    else:
        assert ev.compactions == 0 and ev.reload_causes[0] == "first" and "nodes_add" in ev.reload_causes[1:]
    rep = ra.ctx.audit()
    assert rep["skipped"] == [] and all(rep[k]["n_bad"] == 0 for k in CHECKS), rep


# ------------------------------------------------------------------ two ranks (two processes)
def _compact_worker(rank, world, port, out, seed):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import random
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import escalator_amd as esc
    from escalator_amd.dist import shard_range, try_remove
    from escalator_amd.objects import placement
    from randobj import make_reaping_cluster, make_trackers
    rng = random.Random(seed)
    groups, pods, nodes, now_ns = make_reaping_cluster(rng, 8, 1500, 120)
    trackers = make_trackers(rng, groups, nodes)
    pn, ts, nd = placement(pods, nodes)
    lo, hi = shard_range(len(pods), rank, world)
    c = esc.Context(groups, device=0, rank=rank, world=world)
    c.set_spare(0.25)
    Pr, Nr = c.pack(pods[lo:hi], nodes, trackers)
    c.load(Pr, Nr, pod_offset=lo)
    c.load_placement(pn[lo:hi], ts, nd)
    c.nodes_delete(list(range(5, 120, 7)))
    m = c.nodes_compact(min_free_slots=3)                      # every rank, the same arguments: no collective
    soft, hard = np.full(8, 60 * 10**9, np.int64), np.full(8, 4000 * 10**9, np.int64)
    res = try_remove(c, now_ns, soft, hard, device_collective=False)
    rem = [list(c.removal_nodes(g)) for g in range(8)]
    out.put((rank, (m.tolist(), res.tolist(), rem, c.nodes_room()[0], [c.tracker_list(g).tolist() for g in range(8)])))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_compact_to_the_same_map(esc):
    """World 2, one process per rank, each with its pod shard and the whole node table: both
    compact with the same arguments, their maps are equal, and the reaping over the exchanged
    occupancy words equals a one-rank context's on the live nodes, index for index."""
    import random
    from escalator_amd.objects import placement
    from randobj import make_reaping_cluster, make_trackers
    from test_gpu_dist import _run_ranks
    got = _run_ranks(_compact_worker, 2, 9400)
    gone = set(range(5, 120, 7))
    want_map, k = [], 0
    for j in range(120):
        want_map.append(-1 if j in gone else k)
        k += j not in gone
    assert got[0][0] == got[1][0] == want_map
    assert got[0][1:] == got[1][1:]
    rng = random.Random(9400)
    groups, pods, nodes, now_ns = make_reaping_cluster(rng, 8, 1500, 120)
    trackers = make_trackers(rng, groups, nodes)
    live = [x for j, x in enumerate(nodes) if j not in gone]
    names = {x["name"] for x in live}
    trackers = {g: [m for m in t if m in names] for g, t in trackers.items()}    # (a deleted node's entry is dropped)
    c = esc.Context(groups)
    c.set_spare(0.25)
    c.load(*c.pack(pods, live, trackers))
    c.load_placement(*placement(pods, live))
    res = c.try_remove(now_ns, 60 * 10**9, 4000 * 10**9)
    assert got[0][1] == res.tolist()
    assert got[0][2] == [list(c.removal_nodes(g)) for g in range(8)]
    assert got[0][3] == table_slots(len(live), 0.25) - len(live) and len(names) == len(live)
    assert got[0][4] == [c.tracker_list(g).tolist() for g in range(8)]
    c.close()
