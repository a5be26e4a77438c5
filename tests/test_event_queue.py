"""CPU: escalator_amd.events.EventQueue against a recording stand-in context — the flush
order, coalescing, pod id assignment, the classification of node updates, late and repeated
binding, and the single reload on ESC_E_LIMIT."""
import numpy as np
import pytest

from escalator_amd._lib import ESC_E_INVAL, ESC_E_LIMIT
from escalator_amd.events import KINDS, NONE, EventQueue

TAINT = "atlassian.com/escalator"


class Refused(RuntimeError):
    def __init__(self, code):
        super().__init__("refused %d" % code)
        self.code = code


class Rec:
    """Records every call; packs to name lists; answers `code` to the fail_at-th event call."""

    def __init__(self, fail_at=None, code=ESC_E_LIMIT):
        self.calls, self.hw, self.events, self.fail_at, self.code = [], 0, 0, fail_at, code

    def names(self):
        return [c[0] for c in self.calls]

    def _event(self, name, *args):
        self.events += 1
        if self.fail_at == self.events:
            self.calls.append((name + "!",) + args)
            if name == "pods_upsert":
                return self.code
            raise Refused(self.code)
        self.calls.append((name,) + args)
        return 0

    def pack(self, pods, nodes, trackers=None):
        assert not trackers
        return ({"keys": [p["name"] for p in pods]},
                {"names": [n["name"] for n in nodes],
                 "flags": np.array([int(bool(n.get("unschedulable"))) | 2 * (TAINT in (n.get("taints") or []))
                                    for n in nodes], np.uint32),
                 "cpu": np.array([n.get("cpu") or 0 for n in nodes], np.int64),
                 "mem": np.array([n.get("mem") or 0 for n in nodes], np.int64)})

    def set_spare(self, f):
        self.calls.append(("set_spare", f))

    def load(self, P, N):
        self.hw = len(N["names"])
        self.calls.append(("load", list(P["keys"]), list(N["names"])))

    def load_placement(self, pod_node, taint_s, no_delete):
        self.calls.append(("load_placement", [int(x) for x in pod_node], [int(x) for x in taint_s],
                           [int(x) for x in no_delete]))

    def nodes_delete(self, ids):
        self._event("nodes_delete", [int(j) for j in ids])

    def nodes_add(self, N):
        self._event("nodes_add", list(N["names"]))
        out = np.arange(self.hw, self.hw + len(N["names"]), dtype=np.int64)
        self.hw += len(out)
        return out

    def nodes_relabel(self, ids, N):
        self._event("nodes_relabel", [int(j) for j in ids], list(N["names"]))

    def nodes_update(self, ids, flags, cpu, mem):
        self._event("nodes_update", [int(j) for j in ids], [int(x) for x in flags], [int(x) for x in cpu],
                    [int(x) for x in mem])

    def nodes_facts(self, ids, taint_s, no_delete):
        self._event("nodes_facts", [int(j) for j in ids], [int(x) for x in taint_s], [int(x) for x in no_delete])

    def pods_delete(self, ids):
        self._event("pods_delete", [int(i) for i in ids])

    def pods_upsert(self, ids, P):
        return self._event("pods_upsert", [int(i) for i in ids], list(P["keys"]))

    def pods_bind(self, ids, to):
        self._event("pods_bind", [int(i) for i in ids], [int(j) for j in to])


def node(name, **kw):
    return dict({"name": name, "labels": {"pool": "a"}, "unschedulable": False, "taints": [], "cpu": 4000,
                 "mem": 8 << 30, "created_ns": 1000}, **kw)


def pod(name, node_name="", cpu=100, **kw):
    return dict({"name": name, "containers": [{"cpu": cpu, "mem": 1 << 20}], "node_name": node_name}, **kw)


def loaded(n_nodes=3, n_pods=4, spare=0.5):
    q, ctx = EventQueue(spare=spare), Rec()
    for j in range(n_nodes):
        q.node_add(node("n%d" % j))
    for i in range(n_pods):
        q.pod_add(pod("p%d" % i, "n%d" % (i % n_nodes) if n_nodes else ""))
    q.flush(ctx)
    ctx.calls.clear()
    return q, ctx


def test_first_flush_sets_spare_then_loads():
    q, ctx = EventQueue(spare=1.5), Rec()
    q.node_add(node("a"))
    q.node_add(node("b", taints=[TAINT], taint_value="77", annotations={"atlassian.com/no-delete": "true"}))
    q.pod_add(pod("x", "b"))
    q.pod_add(pod("y", "ghost"))
    q.pod_add(pod("z", namespace="kube"))
    q.flush(ctx)
    assert ctx.names() == ["set_spare", "load", "load_placement"]
    assert ctx.calls[0] == ("set_spare", 1.5)
    assert ctx.calls[1] == ("load", ["x", "y", "z"], ["a", "b"])
    assert ctx.calls[2] == ("load_placement", [1, NONE, NONE], [-(1 << 63), 77], [0, 1])
    assert (q.reloads, q.flushes) == (1, 1) and sum(q.applied.values()) == 0
    assert [q.node_index("a"), q.node_index("b"), q.node_index("c")] == [0, 1, None]
    assert [q.pod_id("x"), q.pod_id("y"), q.pod_id("kube/z"), q.pod_id("z")] == [0, 1, 2, None]
    assert q.node_name(1) == "b" and q.node_name(5) is None
    assert [n["name"] for n in q.live_nodes()] == ["a", "b"] and [p["name"] for p in q.live_pods()] == ["x", "y", "z"]
    q.flush(ctx)                                        # nothing ingested: no call at all
    assert len(ctx.calls) == 3 and q.reloads == 1 and q.flushes == 2


def test_flush_call_order():
    q, ctx = loaded(n_nodes=6, n_pods=6)
    q.pod_update(pod("p1", "n1", cpu=250))              # upsert only
    q.pod_update(pod("p2", "n0"))                       # bind only
    q.pod_delete("p3")
    q.pod_add(pod("new", "fresh"))
    q.node_update(node("n1", unschedulable=True))
    q.node_update(node("n2", labels={"pool": "b"}))
    q.node_update(node("n3", taints=[TAINT], taint_value="5"))        # update + facts
    q.node_update(node("n4", annotations={"atlassian.com/no-delete": "y"}))
    q.node_delete("n5")
    q.node_add(node("fresh"))
    q.flush(ctx)
    assert tuple(ctx.names()) == KINDS
    c = dict((x[0], x[1:]) for x in ctx.calls)
    assert c["nodes_delete"] == ([5],)
    assert c["nodes_add"] == (["fresh"],) and q.node_index("fresh") == 6 and q.node_name(6) == "fresh"
    assert c["nodes_relabel"] == ([2], ["n2"])
    assert c["nodes_update"] == ([1, 3], [1, 2], [4000, 4000], [8 << 30, 8 << 30])
    assert c["nodes_facts"] == ([6, 3, 4], [-(1 << 63), 5, -(1 << 63)], [0, 0, 1])
    assert c["pods_delete"] == ([3],)
    assert c["pods_upsert"] == ([3, 1], ["new", "p1"])            # the freed id goes to the new pod
    assert c["pods_bind"] == ([3, 2], [6, 0])
    assert q.applied == {"nodes_delete": 1, "nodes_add": 1, "nodes_relabel": 1, "nodes_update": 2, "nodes_facts": 3,
                         "pods_delete": 1, "pods_upsert": 2, "pods_bind": 2}
    assert q.reloads == 1
    assert [n["name"] for n in q.live_nodes()] == ["n0", "n1", "n2", "n3", "n4", "fresh"]


def test_coalescing():
    q, ctx = loaded()
    q.pod_update(pod("p0", "n0", cpu=1))
    q.pod_update(pod("p0", "n0", cpu=2))                # update, update: one record, the last
    q.node_update(node("n0", cpu=1))
    q.node_update(node("n0", cpu=2))
    q.pod_add(pod("ghost"))                             # add, delete of a key never flushed: nothing
    q.pod_delete("ghost")
    q.node_add(node("phantom"))
    q.node_delete("phantom")
    q.flush(ctx)
    assert ctx.calls == [("nodes_update", [0], [0], [2], [8 << 30]), ("pods_upsert", [0], ["p0"])]
    assert q.live_pods()[0]["containers"][0]["cpu"] == 2
    ctx.calls.clear()
    q.node_delete("n1")                                 # delete, add: a delete plus a fresh add
    q.node_add(node("n1"))
    q.pod_delete("p2")
    q.pod_add(pod("p2", "n2"))
    q.flush(ctx)
    assert ctx.calls == [("nodes_delete", [1]), ("nodes_add", ["n1"]), ("nodes_facts", [3], [-(1 << 63)], [0]),
                         ("pods_delete", [2]), ("pods_upsert", [2], ["p2"]),
                         ("pods_bind", [2, 1], [2, 3])]       # p1 named n1: bound to its new index
    assert q.node_index("n1") == 3 and q.node_name(1) is None
    assert [n["name"] for n in q.live_nodes()] == ["n0", "n2", "n1"]
    ctx.calls.clear()
    q.pod_update(pod("p1", "n1", cpu=100))              # an update that changes nothing: no call
    q.flush(ctx)
    assert ctx.calls == []


def test_pod_ids_fresh_then_lowest_freed_first():
    q, ctx = loaded(n_nodes=1, n_pods=6)
    q.pod_add(pod("a"))
    q.flush(ctx)
    assert q.pod_id("a") == 6                           # next unused
    for k in ("p4", "p1", "p3"):
        q.pod_delete(k)
    q.flush(ctx)
    assert ctx.calls[-1] == ("pods_delete", [4, 1, 3])
    for k in ("b", "c", "d", "e"):
        q.pod_add(pod(k))
    q.flush(ctx)
    assert [q.pod_id(k) for k in ("b", "c", "d", "e")] == [1, 3, 4, 7]
    assert ctx.calls[-2] == ("pods_upsert", [1, 3, 4, 7], ["b", "c", "d", "e"])
    assert [p["name"] for p in q.live_pods()] == ["p0", "b", "p2", "c", "d", "p5", "a", "e"]


@pytest.mark.parametrize("change, want", [
    (dict(labels={"pool": "b"}), ["nodes_relabel"]),
    (dict(created_ns=2000), ["nodes_relabel"]),
    (dict(labels={"pool": "b"}, unschedulable=True, cpu=1), ["nodes_relabel"]),
    (dict(unschedulable=True), ["nodes_update"]),
    (dict(taints=["other", TAINT]), ["nodes_update"]),           # taint_value absent: no time
    (dict(cpu=8000), ["nodes_update"]),
    (dict(mem=None), ["nodes_update"]),
    (dict(taints=[TAINT], taint_value="9"), ["nodes_update", "nodes_facts"]),
    (dict(annotations={"atlassian.com/no-delete": "true"}), ["nodes_facts"]),
    (dict(annotations={"atlassian.com/no-delete": ""}), []),     # empty: not safe from deletion
    (dict(annotations={"team": "x"}), []),
    (dict(taints=["other"]), []),
    (dict(taint_value="12"), []),                                # no escalator taint: no time
])
def test_node_update_classification(change, want):
    q, ctx = loaded()
    q.node_update(node("n1", **change))
    q.flush(ctx)
    assert ctx.names() == want
    for c in ctx.calls:
        assert c[1] == [1]
    q2, ctx2 = EventQueue(), Rec()                      # a value-only change of a tainted node
    q2.node_add(node("t", taints=[TAINT], taint_value="100"))
    q2.flush(ctx2)
    ctx2.calls.clear()
    q2.node_update(node("t", taints=[TAINT], taint_value="200"))
    q2.flush(ctx2)
    assert ctx2.calls == [("nodes_facts", [0], [200], [0])]


def test_late_binding():
    q, ctx = loaded(n_nodes=2, n_pods=2)
    q.pod_add(pod("early", "later"))                    # names a node not yet known
    q.flush(ctx)
    assert ctx.calls[-1] == ("pods_bind", [2], [NONE])
    ctx.calls.clear()
    q.flush(ctx)
    assert ctx.calls == []
    q.node_add(node("later"))
    q.flush(ctx)
    assert ctx.calls == [("nodes_add", ["later"]), ("nodes_facts", [2], [-(1 << 63)], [0]), ("pods_bind", [2], [2])]
    ctx.calls.clear()
    q.pod_update(pod("early", ""))                      # unbound again
    q.flush(ctx)
    assert ctx.calls == [("pods_bind", [2], [NONE])]


def test_same_name_readd_rebinds_to_new_index():
    q, ctx = loaded(n_nodes=2, n_pods=4)                # p0, p2 on n0; p1, p3 on n1
    q.node_delete("n0")
    q.flush(ctx)
    assert ctx.calls == [("nodes_delete", [0])]         # its pods stay as the library leaves them
    ctx.calls.clear()
    q.pod_delete("p2")
    q.node_add(node("n0"))
    q.flush(ctx)
    assert ctx.calls == [("nodes_add", ["n0"]), ("nodes_facts", [2], [-(1 << 63)], [0]), ("pods_delete", [2]),
                         ("pods_bind", [0], [2])]
    assert q.node_index("n0") == 2


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 8])
def test_limit_causes_exactly_one_reload(k):
    q, ctx = loaded(n_nodes=4, n_pods=5)
    ctx.fail_at = k
    q.node_delete("n1")
    q.node_add(node("m0"))
    q.node_update(node("n2", labels={"pool": "z"}))
    q.node_update(node("n3", cpu=1))
    q.pod_delete("p0")
    q.pod_add(pod("fresh", "m0"))
    q.pod_update(pod("p4", "n2"))
    q.node_delete("n0")                                 # gone and back: a new node, listed last
    q.node_add(node("n0"))
    q.flush(ctx)
    order = ["nodes_delete", "nodes_add", "nodes_relabel", "nodes_update", "nodes_facts", "pods_delete",
             "pods_upsert", "pods_bind"]
    want = order[:k - 1] + [order[k - 1] + "!", "load", "load_placement"]      # the rest is skipped
    assert ctx.names() == want
    nodes_now = ["n2", "n3", "m0", "n0"]                # compacted in snapshot order, new ones after
    bound = {"p1": NONE, "p2": 0, "p3": 1, "p4": 0, "fresh": 2}      # p1 named n1 (gone), fresh m0
    # pods in id order, then the ones without an id (from the upsert on, "fresh" holds p0's)
    pods_now = ["p1", "p2", "p3", "p4", "fresh"] if k < 7 else ["fresh", "p1", "p2", "p3", "p4"]
    assert ctx.calls[-2] == ("load", pods_now, nodes_now)
    assert ctx.calls[-1][1] == [bound[p] for p in pods_now]
    assert q.reloads == 2 and "set_spare" not in ctx.names() and q.reload_causes == ["first", order[k - 1]]
    assert [q.node_index(m) for m in nodes_now] == [0, 1, 2, 3] and q.node_index("n1") is None
    assert [q.node_name(j) for j in range(5)] == nodes_now + [None]
    assert [q.pod_id(p) for p in pods_now] == [0, 1, 2, 3, 4] and q.pod_id("p0") is None
    ctx.calls.clear()
    ctx.fail_at = None
    q.pod_add(pod("after"))                             # the free list was rebuilt: next unused
    q.flush(ctx)
    assert q.pod_id("after") == 5 and ctx.names() == ["pods_upsert", "pods_bind"] and q.reloads == 2


def test_other_errors_propagate():
    q, ctx = loaded()
    ctx.fail_at, ctx.code = 1, ESC_E_INVAL
    q.node_delete("n0")
    with pytest.raises(Refused):
        q.flush(ctx)
    assert q.reloads == 1 and "load" not in ctx.names()
