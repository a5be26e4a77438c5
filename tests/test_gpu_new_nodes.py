"""GPU: esc_new_nodes_eval / esc_new_nodes_list / esc_nodes_instantiated — calculateNewNodeMetrics
(controller.go:157-189) for every group on the device — against the literal restatement in
tests/newnode_literal.py: random clusters, the wave and chunk edges of the per-group walk, the
lag and bucket edges, two groups on one label pair, the fact's life under node events, the
error contract, a multi-device context and the two controllers in lock-step."""
import random

import numpy as np
import pytest

import newnode_literal as NL
from randobj import make_reaping_cluster, make_trackers

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
S = 1_000_000_000
T0 = 1_700_000_000 * S
# lags at and beside the bucket bounds, negative, zero, mid-bucket, beyond every bound
LAG_EDGES = [60 * S, 60 * S + 1, 1740 * S, 1740 * S + 1, -5 * S, 0, 1, 30 * S, 600 * S, 601 * S, 10**13, 59 * S + 999_999_999]
SEEDS = [(0, None), (1, None), (2, None), (3, None), (4, 700)]


@pytest.fixture(scope="module")
def esc():
    import escalator_amd
    return escalator_amd


# ------------------------------------------------------------------------- helpers
def _upload(ctx, live, inst):
    """The known instantiation times of the live nodes, in one call."""
    ids = [j for j in sorted(live) if inst.get(live[j]["name"]) is not None]
    ctx.nodes_instantiated(ids, [inst[live[j]["name"]] for j in ids])


def _lists(ctx, G):
    return [tuple(map(list, ctx.new_nodes_list(g))) for g in range(G)]


def _compare(ctx, groups, live, since, inst, tag=""):
    """One eval against the literal helper on the live list: every field of every record and
    every list with its known bytes.  Returns the records."""
    idx = sorted(live)
    lst = [live[j] for j in idx]
    rec = ctx.new_nodes(since)
    for g, grp in enumerate(groups):
        want = NL.calculate_new_node_metrics(grp, lst, int(since[g]), inst)
        r = rec[g]
        assert int(r["n_new"]) == want["n_new"], (tag, g)
        assert int(r["n_observed"]) == want["n_observed"], (tag, g)
        assert int(r["lag_sum_ns"]) == want["lag_sum_ns"], (tag, g)
        assert int(r["flags"]) == want["flags"], (tag, g)
        assert [int(x) for x in r["bucket"]] == want["bucket"], (tag, g)
        got_idx, got_known = ctx.new_nodes_list(g)
        assert sorted(zip((int(j) for j in got_idx), (int(k) for k in got_known))) == \
            sorted((idx[i], k) for i, k in want["list"]), (tag, g)
    return rec


def scenario(seed, n_nodes=None):
    """A random cluster with per-group `since` words of every kind and instantiation times
    unknown for about a third of the nodes (shared with the CPU check of the seeds)."""
    rng = random.Random(7300 + seed)
    G = rng.choice([3, 6, 12])
    groups, pods, nodes, _ = make_reaping_cluster(rng, G, 60, n_nodes or rng.choice([40, 90, 120]))
    trackers = make_trackers(rng, groups, nodes)
    since = []
    for g, grp in enumerate(groups):
        members = NL.group_nodes(grp, nodes)
        kind = rng.choice(["zero", "off", "own", "own-1", "past"]) if members else rng.choice(["zero", "off"])
        own = nodes[rng.choice(members)]["created_ns"] if members else 0
        since.append({"zero": I64_MIN, "off": I64_MAX, "own": own, "own-1": own - 1,
                      "past": max([nodes[i]["created_ns"] for i in members], default=0)}[kind])
    inst = {}
    for x in nodes:
        if rng.random() >= 1 / 3:
            inst[x["name"]] = x["created_ns"] - rng.choice(LAG_EDGES)
    return groups, pods, nodes, trackers, np.array(since, np.int64), inst


def _loaded(esc, groups, pods, nodes, trackers=None, spare=None, devices=None):
    ctx = esc.Context(groups, devices=devices) if devices else esc.Context(groups)
    if spare:
        ctx.set_spare(spare)
    P, N = ctx.pack(pods, nodes, trackers)
    ctx.load(P, N)
    return ctx


def _node(name, labels, created, **kw):
    return dict({"name": name, "labels": labels, "unschedulable": False, "taints": [], "cpu": 4000, "mem": 8 << 30,
                 "created_ns": created}, **kw)


def _group(name, key, value, **kw):
    return dict({"name": name, "label_key": key, "label_value": value, "min_nodes": 0, "max_nodes": 1000,
                 "taint_lower_pct": 20, "taint_upper_pct": 40, "scale_up_pct": 70, "slow_removal_rate": 1,
                 "fast_removal_rate": 2, "dry_mode": False}, **kw)


# ------------------------------------------------------- 1. random clusters vs literal
@pytest.mark.parametrize("seed, n_nodes", SEEDS)
def test_random_clusters_equal_the_literal_helper(esc, seed, n_nodes):
    groups, pods, nodes, trackers, since, inst = scenario(seed, n_nodes)
    ctx = _loaded(esc, groups, pods, nodes, trackers)
    live = dict(enumerate(nodes))
    _compare(ctx, groups, live, since, {}, "nothing known")        # before any upload: nothing observed
    _upload(ctx, live, inst)
    _compare(ctx, groups, live, since, inst, "known")


# ------------------------------------------------------------ 2. wave and chunk edges
def test_wave_and_chunk_edges(esc):
    sizes = [0, 1, 63, 64, 65, 127, 128, 129, 193]
    groups = [_group("g%d" % i, "pool", "g%d" % i) for i in range(len(sizes))]
    order = [g for g, n in enumerate(sizes) for _ in range(n)]
    random.Random(5).shuffle(order)                                # the groups' nodes interleave in the table
    nodes, inst, pos = [], {}, [0] * len(sizes)
    for j, g in enumerate(order):
        x = _node("n%d" % j, {"pool": "g%d" % g}, T0 + j * 1000)   # distinct creation times
        if pos[g] % 2 == 0:                                        # known and unknown alternate
            inst[x["name"]] = x["created_ns"] - (pos[g] % 31) * 60 * S - 1
        pos[g] += 1
        nodes.append(x)
    ctx = _loaded(esc, groups, [], nodes)
    live = dict(enumerate(nodes))
    _upload(ctx, live, inst)
    rec = _compare(ctx, groups, live, np.full(len(sizes), I64_MIN, np.int64), inst, "all new")
    assert [int(x) for x in rec["n_new"]] == sizes
    assert [int(x) for x in rec["n_observed"]] == [(n + 1) // 2 for n in sizes]
    assert [int(r["bucket"].sum()) for r in rec] == [(n + 1) // 2 for n in sizes]
    # only each group's last node new: its position is the count of every chunk before it
    last = [max((j for j, g in enumerate(order) if g == k), default=None) for k in range(len(sizes))]
    since = np.array([0 if j is None else nodes[j]["created_ns"] - 1 for j in last], np.int64)
    rec = _compare(ctx, groups, live, since, inst, "last new")
    assert [int(x) for x in rec["n_new"]] == [min(n, 1) for n in sizes]
    for g, j in enumerate(last):
        idx, known = ctx.new_nodes_list(g)
        assert list(idx) == ([] if j is None else [j])
        assert [int(k) for k in known] == ([] if j is None else [1 if nodes[j]["name"] in inst else 0])


# --------------------------------------------------------------------- 3. lag edges
def test_lag_and_bucket_edges_and_sum_overflow(esc):
    groups = [_group("a", "pool", "a"), _group("b", "team", "b"), _group("c", "pool", "c")]
    big = (1 << 62) - 1000 * S                                     # two of them stay within int64, alone
    lags = [60 * S, 60 * S + 1, 1740 * S, 1740 * S + 1, -5 * S, None]
    nodes, inst = [], {}
    for k, lag in enumerate(lags):
        nodes.append(_node("e%d" % k, {"pool": "a"}, T0 + k))
        if lag is not None:
            inst["e%d" % k] = T0 + k - lag
    for k in range(2):                                             # in a (with the others) and alone in b
        nodes.append(_node("big%d" % k, {"pool": "a", "team": "b"}, T0 + 100 + k))
        inst["big%d" % k] = T0 + 100 + k - big
    nodes.append(_node("sat", {"pool": "c"}, T0 + 200))            # a lag past int64 saturates like Time.Sub
    inst["sat"] = I64_MIN + 1
    ctx = _loaded(esc, groups, [], nodes)
    live = dict(enumerate(nodes))
    _upload(ctx, live, inst)
    rec = _compare(ctx, groups, live, np.full(3, I64_MIN, np.int64), inst)
    a, b, c = rec[0], rec[1], rec[2]
    want = [0] * 30
    want[0], want[1], want[28], want[29] = 2, 1, 1, 1 + 2          # 60 s and the negative lag; ...; +Inf and the two big
    assert [int(x) for x in a["bucket"]] == want
    assert (int(a["n_new"]), int(a["n_observed"])) == (8, 7)
    total = 60 * S + 60 * S + 1 + 1740 * S + 1740 * S + 1 - 5 * S + 2 * big
    assert total > I64_MAX and int(a["flags"]) == NL.LAG_OVERFLOW
    assert int(a["lag_sum_ns"]) == total - (1 << 64)               # the low 64 bits
    assert (int(b["n_new"]), int(b["n_observed"]), int(b["lag_sum_ns"]), int(b["flags"])) == (2, 2, 2 * big, 0)
    assert int(b["bucket"][29]) == 2
    assert (int(c["n_observed"]), int(c["lag_sum_ns"]), int(c["flags"]), int(c["bucket"][29])) == (1, I64_MAX, 0, 1)


# ------------------------------------------------------ 4. two groups on one label pair
def test_two_groups_on_one_pair_get_their_own_records(esc):
    groups = [_group("a", "pool", "a"), _group("b", "pool", "b"), _group("default", "pool", "a")]
    nodes = [_node("n%d" % j, {"pool": "ab"[j % 2]}, T0 + j * S) for j in range(150)]
    inst = {x["name"]: x["created_ns"] - 90 * S for j, x in enumerate(nodes) if j % 3}
    ctx = _loaded(esc, groups, [], nodes)
    live = dict(enumerate(nodes))
    _upload(ctx, live, inst)
    since = np.array([T0 + 100 * S, I64_MAX, T0 + 20 * S], np.int64)
    rec = _compare(ctx, groups, live, since, inst)
    assert (int(rec[0]["n_new"]), int(rec[1]["n_new"]), int(rec[2]["n_new"])) == (24, 0, 64)
    ia, id_ = ctx.new_nodes_list(0)[0], ctx.new_nodes_list(2)[0]
    assert set(ia) < set(id_) and len(ctx.new_nodes_list(1)[0]) == 0


# --------------------------------------------------------------------------- 5. events
def test_fact_lifecycle_under_node_events(esc):
    groups = [_group("a", "pool", "a"), _group("b", "pool", "b"), _group("c", "team", "c", dry_mode=True)]
    rng = random.Random(17)
    nodes = [_node("n%d" % j, dict({"pool": "ab"[j % 2]}, **({"team": "c"} if j % 5 == 0 else {})), T0 + j * 1000,
                   unschedulable=j % 7 == 0, taints=["atlassian.com/escalator"] if j % 4 == 0 else [])
             for j in range(70)]
    inst = {x["name"]: x["created_ns"] - rng.choice(LAG_EDGES) for x in nodes if rng.random() < 0.6}
    since = np.array([I64_MIN, T0 + 30 * 1000, T0 - 1], np.int64)

    def fresh(live_nodes, known):
        f = _loaded(esc, groups, [], live_nodes, spare=2.0)
        _upload(f, dict(enumerate(live_nodes)), known)
        return f

    ctx = _loaded(esc, groups, [], nodes, spare=2.0)
    live = dict(enumerate(nodes))
    _upload(ctx, live, inst)
    _compare(ctx, groups, live, since, inst, "loaded")
    # nodes_add: the new slots are unknown, then known
    new = [_node("late%d" % k, {"pool": "a", "team": "c"} if k else {"pool": "b"}, T0 + 10**6 + k) for k in range(3)]
    ids = [int(j) for j in ctx.nodes_add(ctx.pack([], new)[1])]
    assert ids == [70, 71, 72]
    live.update(zip(ids, new))
    rec = _compare(ctx, groups, live, since, inst, "added")
    assert int(rec[0]["n_new"]) - int(rec[0]["n_observed"]) >= 2
    for x in new:
        inst[x["name"]] = x["created_ns"] - 75 * S
    ctx.nodes_instantiated(ids, [inst[x["name"]] for x in new])
    rec = _compare(ctx, groups, live, since, inst, "added, known")
    f = fresh([live[j] for j in sorted(live)], inst)
    assert f.new_nodes(since).tobytes() == rec.tobytes() and _lists(f, 3) == _lists(ctx, 3)
    # nodes_relabel moves a known node between groups and keeps its time
    mover = next(j for j in range(1, 70, 2) if live[j]["name"] in inst and j % 5)      # in b only
    live[mover] = dict(live[mover], labels={"pool": "a"})
    ctx.nodes_relabel([mover], ctx.pack([], [live[mover]])[1])
    rec = _compare(ctx, groups, live, since, inst, "relabelled")
    assert mover in ctx.new_nodes_list(0)[0]
    f = fresh([live[j] for j in sorted(live)], inst)
    assert f.new_nodes(since).tobytes() == rec.tobytes()
    assert [sorted(zip(*x)) for x in _lists(f, 3)] == [sorted(zip(*x)) for x in _lists(ctx, 3)]
    # nodes_update keeps it too
    live[mover] = dict(live[mover], unschedulable=True)
    packed = ctx.pack([], [live[mover]])[1]
    ctx.nodes_update([mover], packed["flags"], packed["cpu"], packed["mem"])
    _compare(ctx, groups, live, since, inst, "updated")
    # nodes_delete: gone from counts and list
    gone = ids[1]
    before = int(ctx.new_nodes(since)[0]["n_new"])
    ctx.nodes_delete([gone])
    del inst[live.pop(gone)["name"]]
    rec = _compare(ctx, groups, live, since, inst, "deleted")
    assert int(rec[0]["n_new"]) == before - 1 and gone not in ctx.new_nodes_list(0)[0]
    # a node back under the name takes the next index and starts unknown
    back = dict(new[1], created_ns=T0 + 2 * 10**6)
    (j,) = [int(j) for j in ctx.nodes_add(ctx.pack([], [back])[1])]
    assert j == 73
    live[j] = back
    _compare(ctx, groups, live, since, inst, "back")
    idx, known = ctx.new_nodes_list(0)
    assert int(known[list(idx).index(j)]) == 0
    # load_nodes alone resets every time to unknown
    lst = [live[k] for k in sorted(live)]
    ctx.load_nodes(ctx.pack([], lst)[1])
    rec = _compare(ctx, groups, dict(enumerate(lst)), since, {}, "reloaded")
    assert int(rec["n_observed"].sum()) == 0 and int(rec["n_new"].sum()) > 0


# ----------------------------------------------------------------------- 6. errors
def test_errors_apply_nothing(esc):
    import ctypes as C
    from escalator_amd._lib import ESC_E_INVAL, ESC_E_LIMIT, ESC_E_STATE, EscError, NewNodes
    groups, pods, nodes, trackers, since, inst = scenario(1)
    since[:] = I64_MIN
    bare = esc.Context(groups)
    for call in (lambda: bare.new_nodes(since), lambda: bare.nodes_instantiated([0], [5]),
                 lambda: bare.new_nodes_list(0)):
        with pytest.raises(EscError) as e:                         # before esc_load_nodes
            call()
        assert e.value.code == ESC_E_STATE
    ctx = _loaded(esc, groups, pods, nodes, trackers, spare=1.0)
    live = dict(enumerate(nodes))
    with pytest.raises(EscError) as e:                             # loaded, but no eval yet
        ctx.new_nodes_list(0)
    assert e.value.code == ESC_E_STATE
    _upload(ctx, live, inst)
    ctx.nodes_delete([3])
    del live[3]
    before = _compare(ctx, groups, live, since, {k: v for k, v in inst.items() if k != "node-3"}, "before")
    lists = _lists(ctx, len(groups))
    hw = len(nodes)
    unknown = sorted({int(j) for idx, known in lists for j, k in zip(idx, known) if not k})[:4]
    assert len(unknown) == 4                                       # listed for a lookup by some group
    for bad in ([hw], [-1], [3], [unknown[0]], [hw + 1000]):       # outside the table, absent, repeated
        ids = unknown + bad
        with pytest.raises(EscError) as e:
            ctx.nodes_instantiated(ids, [T0] * len(ids))
        assert e.value.code == ESC_E_INVAL, ids
        assert ctx.new_nodes(since).tobytes() == before.tobytes(), ids
        assert _lists(ctx, len(groups)) == lists, ids
    one = (C.c_int64 * 1)(1)
    assert ctx.lib.esc_nodes_instantiated(ctx.handle, None, 1, one) == ESC_E_INVAL
    assert ctx.lib.esc_nodes_instantiated(ctx.handle, one, 1, None) == ESC_E_INVAL
    assert ctx.lib.esc_nodes_instantiated(ctx.handle, None, 0, None) == 0          # n == 0
    assert ctx.lib.esc_new_nodes_eval(ctx.handle, None, (NewNodes * len(groups))()) == ESC_E_INVAL
    assert ctx.new_nodes(since).tobytes() == before.tobytes()
    # a short cap
    g = int(np.argmax(before["n_new"]))
    n_new = int(before[g]["n_new"])
    assert n_new >= 2
    n = C.c_int64()
    idx, known = (C.c_int64 * n_new)(), (C.c_uint8 * n_new)()
    assert ctx.lib.esc_new_nodes_list(ctx.handle, g, idx, known, n_new - 1, C.byref(n)) == ESC_E_LIMIT
    assert n.value == n_new
    assert ctx.lib.esc_new_nodes_list(ctx.handle, g, idx, known, n_new, C.byref(n)) == 0
    assert ctx.lib.esc_new_nodes_list(ctx.handle, len(groups), idx, known, n_new, C.byref(n)) == ESC_E_INVAL
    # the same ids in a valid batch: the eval is no longer current after the call, and the new
    # one differs (a refused batch that had written anything would have shown above)
    ctx.nodes_instantiated(unknown, [T0] * 4)
    with pytest.raises(EscError) as e:
        ctx.new_nodes_list(g)
    assert e.value.code == ESC_E_STATE
    after = ctx.new_nodes(since)
    assert int(after["n_observed"].sum()) > int(before["n_observed"].sum())
    # every node event makes the eval not current
    packed = ctx.pack([], [live[0]])[1]
    for event in (lambda: ctx.nodes_update([0], packed["flags"], packed["cpu"], packed["mem"]),
                  lambda: ctx.nodes_delete([5]),
                  lambda: ctx.nodes_add(ctx.pack([], [dict(nodes[5], name="again")])[1]),
                  lambda: ctx.nodes_relabel([0], packed)):
        ctx.new_nodes(since)
        ctx.new_nodes_list(0)
        event()
        with pytest.raises(EscError) as e:
            ctx.new_nodes_list(0)
        assert e.value.code == ESC_E_STATE


# ------------------------------------------------------------------ 7. multi-device
def test_multi_device_equals_single(esc):
    groups, pods, nodes, trackers, since, inst = scenario(2)
    one = _loaded(esc, groups, pods, nodes, trackers)
    multi = _loaded(esc, groups, pods, nodes, trackers, devices=[0, 0])
    live = dict(enumerate(nodes))
    _upload(one, live, inst)
    _upload(multi, live, inst)
    want = _compare(one, groups, live, since, inst, "single")
    got = _compare(multi, groups, live, since, inst, "multi")
    assert got.tobytes() == want.tobytes() and _lists(multi, len(groups)) == _lists(one, len(groups))


# ----------------------------------------------------- 8. the controllers in lock-step
SCAN_NS = 60 * S
SKEW = 3 * SCAN_NS      # the API server's clock runs ahead of the controller's: a registered node
                        # stays newer than the next scale-out stamp, so a failed lookup is retried


def _history():
    """Two groups over capacity.  `lock` (cool-down two scans): scan 0 scales up by the 3 nodes
    its maximum allows and locks, scan 1 is locked, scan 2 is unlocked and armed.  `fast`
    (no cool-down): scan 0 adds 2, scans 1 and 2 are armed; one of its nodes' lookups fails
    once.  registrations[s] = the nodes that register after scan s."""
    common = dict(label_key="pool", taint_lower_pct=20, taint_upper_pct=40, scale_up_pct=70, slow_removal_rate=1,
                  fast_removal_rate=2, dry_mode=False, min_nodes=1, soft_delete_grace_ns=10**15,
                  hard_delete_grace_ns=10**15)
    groups = [dict(common, name="lock", label_value="lock", max_nodes=7, scale_up_cool_down_ns=2 * SCAN_NS),
              dict(common, name="fast", label_value="fast", max_nodes=6, scale_up_cool_down_ns=0)]
    nodes = [_node("%s-%d" % (g["name"], i), {"pool": g["name"]}, T0 - 10**12 + i) for g in groups for i in range(4)]
    pods = [{"name": "%s-pod-%d" % (g["name"], i), "owner_kinds": [], "annotations": {},
             "node_selector": {"pool": g["name"]}, "affinity": None, "containers": [{"cpu": 1500, "mem": 1 << 28}],
             "init_containers": [], "overhead": None, "node_name": ""} for g in groups for i in range(20)]
    reg = {0: [_node("cloud-lock-%d" % i, {"pool": "lock"}, T0 + SCAN_NS // 2 + i) for i in range(3)] +
              [_node("cloud-fast-%d" % i, {"pool": "fast"}, T0 + SCAN_NS // 2 + SKEW + i) for i in range(2)],
           # after scan 2 a node goes away and registers again under its name: a new instance
           2: [_node("cloud-fast-0", {"pool": "fast"}, T0 + 2 * SCAN_NS + SCAN_NS // 2 + SKEW)]}
    return groups, pods, nodes, reg


def _since_restated(prev_delta, branch, last_scale_out):
    """The arming rule read off the reference, not off the controller: the loop runs when the
    previous scaleDelta was positive (controller.go:165) and scaleNodeGroup gets to :325 — it
    returns before that for no pods and nodes (:233), the min / max gate (:238-255), fewer
    untainted nodes than the minimum (:281-294), a percent error (:299-303) and the lock
    (:317-323)."""
    returned_early = branch in ("empty", "gate", "below_min", "pct_err", "locked")
    if prev_delta <= 0 or returned_early:
        return I64_MAX
    return I64_MIN if last_scale_out is None else last_scale_out


class _Store:
    """The API server of one controller: the objects in arrival order, optionally mirrored
    into an event queue."""

    def __init__(self, sink=None):
        self.nodes, self.pods, self.sink = {}, {}, sink

    def put_node(self, x):
        if self.nodes.pop(x["name"], None) is not None and self.sink is not None:
            self.sink.node_delete(x["name"])                   # registered again: deleted first
        self.nodes[x["name"]] = x
        if self.sink is not None:
            self.sink.node_add(x)

    def put_pod(self, p):
        self.pods[p["name"]] = p
        if self.sink is not None:
            self.sink.pod_add(p)


def _cloud(esc_controller, groups, resolve, fail_once):
    class Cloud(esc_controller.SimulatedCloud):
        """SimulatedCloud plus GetInstance: launched 90 s before registration; the names in
        `fail_once` fail their first lookup."""

        def __init__(self):
            super().__init__(groups)
            self.asked, self.answered, self.failing = [], {}, set(fail_once)

        def instantiation_time(self, g, j):
            name = resolve(j)
            self.asked.append(name)
            if name in self.failing:
                self.failing.discard(name)
                raise RuntimeError("GetInstance: throttled")
            self.answered[name] = self.created[name] - 90 * S
            return self.answered[name]
    return Cloud()


def _run_history(esc, with_lookup, scans=6):
    """Both controllers over the history; per scan (results of Controller, results of
    ResidentController, what each literal record should be)."""
    from escalator_amd import controller as EC
    groups, pods, nodes, reg = _history()
    now = [T0]
    out = []
    listed = []
    c1_store = _Store()
    act1 = _cloud(EC, groups, lambda j: listed[j], {"cloud-fast-1"}) if with_lookup else None
    c1 = EC.Controller(groups, clock=lambda: now[0], actuator=act1)
    c2 = EC.ResidentController(groups, clock=lambda: now[0], actuator=None)
    act2 = _cloud(EC, groups, c2.events.node_name, {"cloud-fast-1"}) if with_lookup else None
    if with_lookup:
        c2.actuator = act2
    c2_store = _Store(c2.events)
    calls = {"n": 0}
    for c in (c1, c2):
        def counted(since, _f=c.ctx.new_nodes):
            calls["n"] += 1
            return _f(since)
        c.ctx.new_nodes = counted
    for st in (c1_store, c2_store):
        for x in nodes:
            st.put_node(x)
        for p in pods:
            st.put_pod(p)

    def list_nodes():
        listed[:] = list(c1_store.nodes)
        return list(c1_store.nodes.values())

    for scan in range(scans):
        now[0] = T0 + scan * SCAN_NS
        for act in (act1, act2):
            if act is not None:
                act.created = {m: x["created_ns"] for m, x in c1_store.nodes.items()}
        prev = (list(c1.scale_delta), list(c1.last_scale_out))
        r1 = c1.run_once(lambda: list(c1_store.pods.values()), list_nodes)
        r2 = c2.run_once()
        want = []
        for g, grp in enumerate(groups):
            since = _since_restated(prev[0][g], r1[g]["branch"], prev[1][g])
            if not with_lookup or since == I64_MAX:
                want.append(None)
                continue
            lit = NL.calculate_new_node_metrics(grp, list(c1_store.nodes.values()), since, act1.answered)
            want.append({"n_new": lit["n_new"], "n_observed": lit["n_observed"],
                         "n_unknown": lit["n_new"] - lit["n_observed"], "lag_sum_ns": lit["lag_sum_ns"],
                         "buckets": lit["bucket"], "expected": prev[0][g]})
        out.append((r1, r2, want))
        assert c1.scale_delta == c2.scale_delta and c1.last_scale_out == c2.last_scale_out, scan
        for x in reg.get(scan, []):
            c1_store.put_node(x)
            c2_store.put_node(x)
    return out, calls["n"], (act1, act2)


def test_controllers_in_lock_step_with_the_literal_helper(esc):
    out, n_calls, (act1, act2) = _run_history(esc, with_lookup=True)
    assert len(out) >= 6
    seen = []
    for scan, (r1, r2, want) in enumerate(out):
        for g in range(2):
            assert r1[g].get("new_nodes") == r2[g].get("new_nodes") == want[g], (scan, g)
            assert (r1[g]["branch"], r1[g]["delta"], r1[g]["added"]) == (r2[g]["branch"], r2[g]["delta"], r2[g]["added"])
            if want[g] is not None:
                seen.append(want[g])
    # the history did what it is for: a scale-up that locks, the cool-down expiring, nodes
    # registering after the scale-out, a lookup that fails once
    assert [out[s][0][0]["branch"] for s in range(3)] == ["scale_up", "locked", "scale_up"]
    assert out[0][0][0]["added"] == 3 and out[0][0][1]["added"] == 2
    assert out[1][0][0].get("new_nodes") is None                      # locked: not reached (controller.go:317-325)
    assert out[2][0][0]["new_nodes"]["n_observed"] == 3 == out[2][0][0]["new_nodes"]["expected"]
    fast1, fast2 = out[1][0][1]["new_nodes"], out[2][0][1]["new_nodes"]
    assert (fast1["n_new"], fast1["n_observed"], fast1["n_unknown"]) == (2, 1, 1)
    assert (fast2["n_new"], fast2["n_observed"], fast2["n_unknown"]) == (2, 2, 0)
    assert fast1["buckets"][1] == 1 and fast2["buckets"][1] == 2 and fast2["lag_sum_ns"] == 180 * S
    assert any(w["n_observed"] > 0 for w in seen) and any(w["n_unknown"] > 0 for w in seen)
    assert any(w["expected"] != w["n_observed"] for w in seen)
    # an instance is asked about until it answers, and never again: the reloading controller
    # re-uploads what it learned, the resident snapshot keeps it; the node that registered again
    # under its name is a new instance to both
    for act in (act1, act2):
        assert sorted(act.asked) == sorted(["cloud-lock-0", "cloud-lock-1", "cloud-lock-2", "cloud-fast-0",
                                            "cloud-fast-1", "cloud-fast-1", "cloud-fast-0"])
    fast3 = out[3][0][1]["new_nodes"]
    assert (fast3["n_new"], fast3["n_observed"], fast3["n_unknown"]) == (2, 2, 0)
    assert n_calls > 0


def test_without_the_actuator_method_nothing_is_called(esc):
    out, n_calls, _ = _run_history(esc, with_lookup=False)
    assert n_calls == 0
    assert all("new_nodes" not in r for r1, r2, _ in out for r in r1 + r2)
    assert [out[s][0][0]["branch"] for s in range(3)] == ["scale_up", "locked", "scale_up"]
