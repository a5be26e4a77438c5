"""CPU: the host side of the new-node pass (calculateNewNodeMetrics, controller.go:157-189):
the ABI's new entries, the arming rule, the scaleDelta / lastScaleOut bookkeeping of the
controllers, the event queue's instantiation-time cache and the literal checker's two
bucket rules."""
import ctypes as C

import numpy as np
import pytest

import newnode_literal as NL
from escalator_amd import _lib as L
from test_event_queue import Rec, node, pod

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
S = 1_000_000_000


# ------------------------------------------------------------------------------ ABI
def test_new_symbols_resolve_and_record_size():
    lib = L.load()
    for name in ("esc_nodes_instantiated", "esc_new_nodes_eval", "esc_new_nodes_list"):
        assert hasattr(lib, name), name
        assert name in L._SIGS and name in L.header_functions(), name
    assert C.sizeof(L.NewNodes) == 152
    from escalator_amd.context import NEW_NODES_DTYPE
    assert NEW_NODES_DTYPE.itemsize == 152 and NEW_NODES_DTYPE["bucket"].shape == (30,)
    assert (L.ESC_NN_BUCKETS, L.ESC_NN_LAG_OVERFLOW) == (30, 1)
    assert lib.esc_abi_version() == 6                        # entries were only added
    hdr = open(L.HEADER).read()
    assert "#define ESC_NN_BUCKETS 30" in hdr and "#define ESC_NN_LAG_OVERFLOW 1" in hdr


def test_host_only_context_reports_no_device():
    from escalator_amd.context import Context
    ctx = Context([{"name": "a", "label_key": "k", "label_value": "v"}], device=-1)
    one = (C.c_int64 * 1)(0)
    rec = (L.NewNodes * 1)()
    n = C.c_int64()
    assert ctx.lib.esc_nodes_instantiated(ctx.handle, one, 1, one) == L.ESC_E_NODEV
    assert ctx.lib.esc_new_nodes_eval(ctx.handle, one, rec) == L.ESC_E_NODEV
    assert ctx.lib.esc_new_nodes_list(ctx.handle, 0, None, None, 0, C.byref(n)) == L.ESC_E_NODEV
    assert ctx.lib.esc_new_nodes_eval(ctx.handle, None, rec) == L.ESC_E_INVAL
    assert ctx.lib.esc_new_nodes_list(ctx.handle, 5, None, None, 0, C.byref(n)) == L.ESC_E_INVAL


# --------------------------------------------------------------------------- arming
def test_arming_truth_table():
    from escalator_amd.controller import ARMED_BRANCHES, new_node_since
    assert len(L.BRANCHES) == 9
    armed = {"fast_down", "slow_down", "scale_up", "none"}
    assert set(ARMED_BRANCHES) == armed
    for branch in L.BRANCHES:
        for prev in (-1, 0, 3):
            for status in (L.ESC_ST_OK, L.ESC_ST_ERR_NEG_DELTA):
                for last in (None, 1_700_000_000 * S):
                    got = new_node_since(prev, branch, status, last)
                    if prev > 0 and branch in armed:         # controller.go:165 and :325 both reached
                        assert got == (I64_MIN if last is None else last), (branch, prev, status, last)
                    else:
                        assert got == I64_MAX, (branch, prev, status, last)
    # an errored scale_up is armed: calcScaleUpDelta fails at :346, after :325
    assert new_node_since(3, "scale_up", L.ESC_ST_ERR_NEG_DELTA, 7) == 7
    for branch in ("empty", "gate", "below_min", "pct_err", "locked"):
        assert new_node_since(3, branch, L.ESC_ST_OK, 7) == I64_MAX


# ---------------------------------------------------------------------- bookkeeping
class _Ctx:
    """What _act reads of the context when no walk has anything to walk."""

    def removal_nodes(self, g):
        return np.zeros(0, np.int64)

    def group_order(self, g, which):
        return np.zeros(0, np.int64)


def _bare_controller(groups, clock):
    from escalator_amd.controller import Controller, SimulatedCloud
    from escalator_amd.context import REMOVAL_DTYPE
    c = object.__new__(Controller)                           # no device: the action switch alone
    c.groups = [dict(g, dry_mode=False) for g in groups]
    c.ctx, c._sel, c._new_nodes = _Ctx(), None, None
    c.state = [{"locked": False, "requested_nodes": 0, "cached_cpu_m": 0, "cached_mem_b": 0} for _ in groups]
    c.lock_time = [None] * len(groups)
    c.scale_delta = [0] * len(groups)
    c.last_scale_out = [None] * len(groups)
    c.inst_ns = {}
    c.taint_tracker = {g: [] for g in range(len(groups))}
    c.clock = clock
    c.actuator = SimulatedCloud(c.groups)
    c._removal = np.zeros(len(groups), REMOVAL_DTYPE)
    return c


def _decision(rows):
    from escalator_amd.context import DECISION_DTYPE, TOTALS_DTYPE
    dec = np.zeros(len(rows), DECISION_DTYPE)
    tot = np.zeros(len(rows), TOTALS_DTYPE)
    for g, (branch, delta, status) in enumerate(rows):
        dec[g]["branch"], dec[g]["delta"], dec[g]["status"] = L.BRANCHES.index(branch), delta, status
        tot[g]["n_nodes"] = tot[g]["n_untainted"] = 10
    return tot, dec


def test_scale_delta_and_last_scale_out_bookkeeping():
    groups = [{"name": "g%d" % i, "label_key": "k", "label_value": "v%d" % i, "max_nodes": 100} for i in range(4)]
    now = [1000]
    c = _bare_controller(groups, lambda: now[0])
    assert c.scale_delta == [0] * 4 and c.last_scale_out == [None] * 4
    # scan 1: below_min scales up without the stamp (controller.go:281-294 returns before :376);
    # a scale-up stamps; an errored scale-up stores its delta and does not act; no change
    out = c._act(*_decision([("below_min", 2, 0), ("scale_up", 3, 0), ("scale_up", -4, L.ESC_ST_ERR_NEG_DELTA),
                             ("none", 0, 0)]), names=[])
    assert [r["delta"] for r in out] == [2, 3, -4, 0]
    assert c.scale_delta == [2, 3, -4, 0]
    assert c.last_scale_out == [None, 1000, None, None]
    assert out[2]["err"] == "negative scale up delta" and out[2]["added"] == 0
    assert all("new_nodes" not in r for r in out)
    # scan 2: locked returns requestedNodes (stored, no stamp); a gate error stores 0; scale-down
    now[0] = 2000
    out = c._act(*_decision([("locked", 5, 0), ("gate", 0, L.ESC_ST_ERR_MIN_NODES), ("slow_down", -1, 0),
                             ("scale_up", 1, 0)]), names=[])
    assert c.scale_delta == [5, 0, -1, 1]
    assert c.last_scale_out == [None, 1000, None, 2000]
    # a lister error is scaleNodeGroup's (0, err) for every group (controller.go:195-205, :434)
    def boom():
        raise RuntimeError("list failed")
    out = c.run_once(boom, lambda: [])
    assert [r["delta"] for r in out] == [0] * 4 and c.scale_delta == [0] * 4
    assert c.last_scale_out == [None, 1000, None, 2000]
    # a record of the pass made before the switch lands in the armed group's result only
    c._new_nodes = {3: {"n_new": 1}}
    out = c._act(*_decision([("none", 0, 0)] * 4), names=[])
    assert [("new_nodes" in r) for r in out] == [False, False, False, True]


# ---------------------------------------------------------------------- event queue
class RecInst(Rec):
    def nodes_instantiated(self, ids, inst_ns):
        self.calls.append(("nodes_instantiated", [int(j) for j in ids], [int(t) for t in inst_ns]))


def test_event_queue_cache_dropped_on_delete_and_resent_once_after_reload():
    from escalator_amd.events import EventQueue
    q, ctx = EventQueue(spare=0.5), RecInst()
    for j in range(4):
        q.node_add(node("n%d" % j))
    q.pod_add(pod("p0", "n0"))
    q.flush(ctx)                                             # the first load: nothing known, nothing sent
    assert "nodes_instantiated" not in ctx.names()
    q.inst_ns["n1"] = 111                                    # (the controller's pass learned these)
    q.inst_ns["n3"] = 333
    ctx.calls.clear()
    q.node_update(node("n2", unschedulable=True))            # an ordinary flush does not send the cache
    q.flush(ctx)
    assert ctx.names() == ["nodes_update"]
    # node_delete drops the name at once; the node back under it is a new instance
    q.node_delete("n1")
    assert q.inst_ns == {"n3": 333}
    q.node_add(node("n1"))
    ctx.calls.clear()
    q.flush(ctx)
    assert "nodes_instantiated" not in ctx.names() and q.inst_ns == {"n3": 333}
    # a reload (ESC_E_LIMIT on the add) re-sends what is known, once, after the load
    q.inst_ns["n1"] = 112
    ctx.calls.clear()
    ctx.fail_at = ctx.events + 1
    q.node_add(node("n9"))
    q.flush(ctx)
    assert q.reloads == 2 and q.reload_causes[-1] == "nodes_add"
    assert ctx.names() == ["nodes_add!", "load", "load_placement", "nodes_instantiated"]
    sent = ctx.calls[-1]
    assert dict(zip(sent[1], sent[2])) == {q.node_index("n3"): 333, q.node_index("n1"): 112}
    ctx.calls.clear()
    q.pod_add(pod("p1", "n9"))
    q.flush(ctx)                                             # and not again
    assert "nodes_instantiated" not in ctx.names()


def test_event_queue_without_cache_never_calls_the_context():
    from escalator_amd.events import EventQueue
    q, ctx = EventQueue(), Rec()                             # the stand-in has no nodes_instantiated
    q.node_add(node("a"))
    q.flush(ctx)
    q.node_delete("a")
    q.flush(ctx)
    assert q.inst_ns == {}


# ------------------------------------------------------------ the GPU test's scenarios
def test_random_scenarios_cover_new_unknown_and_unevaluated_groups():
    """The seeds tests/test_gpu_new_nodes.py compares on the device, judged with the literal
    helper alone: at least half of the evaluated groups have new nodes, and at least one has
    some but not all of them observed."""
    from test_gpu_new_nodes import SEEDS, scenario
    evaluated = with_new = partial = 0
    for seed, n_nodes in SEEDS:
        groups, _, nodes, _, since, inst = scenario(seed, n_nodes)
        assert 3 <= len(groups) <= 12 and len(nodes) in (40, 90, 120, 700)
        for g, grp in enumerate(groups):
            if int(since[g]) == I64_MAX:
                continue
            r = NL.calculate_new_node_metrics(grp, nodes, int(since[g]), inst)
            evaluated += 1
            with_new += r["n_new"] > 0
            partial += 0 < r["n_observed"] < r["n_new"]
    assert evaluated >= 10 and 2 * with_new >= evaluated and partial >= 1, (evaluated, with_new, partial)


# ------------------------------------------------------------------ literal checker
@pytest.mark.parametrize("lag_ns, bucket", [(-5 * S, 0), (0, 0), (60 * S, 0), (60 * S + 1, 1), (1740 * S, 28),
                                            (1740 * S + 1, 29)])
def test_float_bucket_rule_equals_integer_rule_at_the_edges(lag_ns, bucket):
    assert NL.bucket_of_float(NL.duration_seconds(lag_ns)) == bucket
    assert NL.bucket_of_int(lag_ns) == bucket


def test_float_and_integer_bucket_rules_agree_around_every_bound():
    assert NL.BUCKETS == [60.0 * (k + 1) for k in range(29)] and NL.N_BUCKETS == L.ESC_NN_BUCKETS
    lags = [I64_MIN, I64_MAX, -1, 1]
    for k in range(29):
        lags += [60 * S * (k + 1) + d for d in (-S, -1, 0, 1, S)]
    for lag in lags:
        assert NL.bucket_of_float(NL.duration_seconds(lag)) == NL.bucket_of_int(lag), lag


def test_literal_skips_unknown_instances_without_counting_them():
    g = {"name": "a", "label_key": "pool", "label_value": "a"}
    nodes = [{"name": "x", "labels": {"pool": "a"}, "created_ns": 100 * S},
             {"name": "y", "labels": {"pool": "a"}, "created_ns": 200 * S, "unschedulable": True},
             {"name": "z", "labels": {"pool": "b"}, "created_ns": 300 * S},
             {"name": "w", "labels": {"pool": "a"}, "created_ns": 100 * S + 1,
              "taints": ["atlassian.com/escalator"]}]
    r = NL.calculate_new_node_metrics(g, nodes, 100 * S, {"y": 200 * S - 61 * S, "w": None})
    assert (r["n_new"], r["n_observed"], r["lag_sum_ns"], r["flags"]) == (2, 1, 61 * S, 0)
    assert r["list"] == [(1, 1), (3, 0)] and r["bucket"][1] == 1 and sum(r["bucket"]) == 1
    assert NL.calculate_new_node_metrics(g, nodes, I64_MAX, {})["n_new"] == 0
    assert NL.calculate_new_node_metrics(g, nodes, I64_MIN, {})["n_new"] == 3
    r = NL.calculate_new_node_metrics(g, nodes, 0, {"x": I64_MIN + 5, "y": I64_MIN + 5})
    assert r["flags"] == NL.LAG_OVERFLOW and r["bucket"][29] == 2      # two saturated lags sum past int64
