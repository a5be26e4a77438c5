"""CPU: EventQueue.resync_nodes against the recording stand-in context of tests/test_event_queue.py
with a scripted nodes_verify: the flush comes first, the object store's nodes are verified with the
ids of the identity map, their facts and the instantiation times the queue holds, the repairs are
one call per kind in the flush's order with the right indices, a clean verify issues none, an
ESC_E_LIMIT from a repair takes the flush's rebuild, compact or reload path, and EventQueue.resync
neither calls nor needs any of it."""
import logging

import numpy as np

from escalator_amd._lib import NV_ABSENT, NV_FACTS, NV_INST, NV_SHAPE, NV_STATUS
from escalator_amd.events import KINDS, NONE, EventQueue
from test_event_queue import TAINT, Rec, node, pod
from test_event_queue_resync import VerifyRec

UNKNOWN = -(1 << 63)
ZERO = {"checked": 0, "absent": 0, "shape": 0, "status": 0, "facts": 0, "inst": 0, "orphans": 0, "reloaded": False}


class NodeVerifyRec(Rec):
    """Rec with a scripted node verify: `status` maps a node's name to its status byte, `extra`
    are slots the device holds beyond the ones it was given."""

    def __init__(self, status=None, extra=(), room=(0, 0)):
        super().__init__()
        self.status, self.extra, self.live, self.room = dict(status or {}), list(extra), set(), room

    def load(self, P, N):
        super().load(P, N)
        self.live = set(range(len(N["names"])))

    def nodes_add(self, N):
        out = super().nodes_add(N)
        self.live |= {int(j) for j in out}
        return out

    def nodes_delete(self, ids):
        super().nodes_delete(ids)
        self.live -= {int(j) for j in ids}

    def nodes_verify(self, ids, N, taint_s=None, no_delete=None, inst_ns=None):
        self.calls.append(("nodes_verify", [int(j) for j in ids], list(N["names"]), [int(x) for x in taint_s],
                           [int(x) for x in no_delete], [int(x) for x in inst_ns]))
        st = np.array([self.status.get(m, 0) for m in N["names"]], np.uint8)
        return st, {"n_checked": len(st)}

    def nodes_live_ids(self):
        self.calls.append(("nodes_live_ids",))
        return np.array(sorted(self.live | set(self.extra)), np.int64)

    def nodes_instantiated(self, ids, inst_ns):
        self._event("nodes_instantiated", [int(j) for j in ids], [int(x) for x in inst_ns])

    def nodes_rebuild(self):
        self.calls.append(("nodes_rebuild",))

    def nodes_room(self):
        return self.room

    def nodes_compact(self, min_free_slots=0, min_free_xl_words=0):
        self.calls.append(("nodes_compact", min_free_slots, min_free_xl_words))
        old = sorted(self.live)
        new = np.full(self.hw, -1, np.int64)
        new[old] = np.arange(len(old))
        self.live, self.hw = set(range(len(old))), len(old)
        return new


def loaded(status=None, extra=(), room=(0, 0), **kw):
    q, ctx = EventQueue(spare=0.5, **kw), NodeVerifyRec(status, extra, room)
    for j in range(6):
        q.node_add(node("n%d" % j))
    for i in range(6):
        q.pod_add(pod("p%d" % i, "n%d" % (i % 3)))
    q.flush(ctx)
    ctx.calls.clear()
    ctx.events = 0
    return q, ctx


def test_a_clean_store_makes_no_calls_and_returns_zeros():
    q, ctx = loaded()
    q.inst_ns["n2"] = 555
    out = q.resync_nodes(ctx)
    assert ctx.names() == ["nodes_verify", "nodes_live_ids"]
    assert ctx.calls[0][1:] == (list(range(6)), ["n%d" % j for j in range(6)], [UNKNOWN] * 6, [0] * 6,
                                [UNKNOWN, UNKNOWN, 555, UNKNOWN, UNKNOWN, UNKNOWN])
    assert out == dict(ZERO, checked=6)
    assert (q.node_resyncs, q.reloads, q.flushes) == (1, 1, 2)
    assert q.node_resync_repairs == {"absent": 0, "shape": 0, "status": 0, "facts": 0, "inst": 0, "orphans": 0}
    assert sum(q.applied.values()) == 0 and tuple(q.applied) == KINDS


def test_it_flushes_first_and_verifies_in_chunks_with_the_facts():
    q, ctx = loaded()
    q.node_update(node("n1", taints=[TAINT], taint_value="77", annotations={"atlassian.com/no-delete": "true"}))
    q.node_delete("n0")
    q.node_add(node("n6"))
    out = q.resync_nodes(ctx, chunk=4)
    assert ctx.names() == ["nodes_delete", "nodes_add", "nodes_update", "nodes_facts", "nodes_verify", "nodes_verify",
                           "nodes_live_ids"]
    assert ctx.calls[4][1:] == ([1, 2, 3, 4], ["n1", "n2", "n3", "n4"], [77, UNKNOWN, UNKNOWN, UNKNOWN], [1, 0, 0, 0],
                                [UNKNOWN] * 4)
    assert ctx.calls[5][1:3] == ([5, 6], ["n5", "n6"])
    assert out == dict(ZERO, checked=6)


def test_one_node_per_kind_gives_the_four_repair_calls_in_order(caplog):
    status = {"n1": NV_SHAPE, "n2": NV_STATUS, "n3": NV_FACTS, "n4": NV_INST}
    q, ctx = loaded(status)
    q.inst_ns["n4"] = 999
    before = dict(q.applied)
    with caplog.at_level(logging.WARNING, logger="escalator_amd.events"):
        out = q.resync_nodes(ctx)
    assert ctx.names() == ["nodes_verify", "nodes_live_ids", "nodes_relabel", "nodes_update", "nodes_facts",
                           "nodes_instantiated"]
    assert ctx.calls[2][1:] == ([1], ["n1"])
    assert ctx.calls[3][1:] == ([2], [0], [4000], [8 << 30])
    assert ctx.calls[4][1:] == ([3], [UNKNOWN], [0])
    assert ctx.calls[5][1:] == ([4], [999])
    assert out == dict(ZERO, checked=6, shape=1, status=1, facts=1, inst=1)
    assert q.node_resync_repairs == {"absent": 0, "shape": 1, "status": 1, "facts": 1, "inst": 1, "orphans": 0}
    got = {k: q.applied[k] - before[k] for k in KINDS}
    assert got == dict({k: 0 for k in KINDS}, nodes_relabel=1, nodes_update=1, nodes_facts=1)   # inst is not counted
    warned = [r.getMessage() for r in caplog.records if r.name == "escalator_amd.events"]
    assert len(warned) == 4 and all(m.startswith("resync: 1 nodes ") for m in warned)
    assert q.reloads == 1 and q.node_resyncs == 1
    # a second pass over a clean device reports nothing
    ctx.status = {}
    ctx.calls.clear()
    assert q.resync_nodes(ctx) == dict(ZERO, checked=6)
    assert ctx.names() == ["nodes_verify", "nodes_live_ids"]


def test_shape_with_status_goes_to_relabel_only_and_every_kind_or_ed():
    status = {"n0": NV_SHAPE | NV_STATUS, "n2": NV_STATUS | NV_FACTS | NV_INST, "n5": NV_SHAPE | NV_FACTS}
    q, ctx = loaded(status)
    out = q.resync_nodes(ctx)
    assert ctx.names() == ["nodes_verify", "nodes_live_ids", "nodes_relabel", "nodes_update", "nodes_facts",
                           "nodes_instantiated"]
    assert ctx.calls[2][1:] == ([0, 5], ["n0", "n5"])
    assert ctx.calls[3][1] == [2]                                      # n0's status went with its relabel
    assert ctx.calls[4][1] == [2, 5]
    assert ctx.calls[5][1:] == ([2], [UNKNOWN])
    assert out == dict(ZERO, checked=6, shape=2, status=2, facts=2, inst=1)


def test_orphans_go_to_one_nodes_delete():
    q, ctx = loaded(extra=[9, 11])
    out = q.resync_nodes(ctx)
    assert ctx.names() == ["nodes_verify", "nodes_live_ids", "nodes_delete"]
    assert ctx.calls[2][1:] == ([9, 11],)
    assert out == dict(ZERO, checked=6, orphans=2) and q.node_resync_repairs["orphans"] == 2
    assert q.applied["nodes_delete"] == 2


def test_an_absent_node_is_added_again_and_its_pods_rebound():
    q, ctx = loaded({"n1": NV_ABSENT})
    ctx.live.discard(1)
    q.inst_ns["n1"] = 321
    out = q.resync_nodes(ctx)
    assert ctx.names() == ["nodes_verify", "nodes_live_ids", "nodes_add", "nodes_facts", "nodes_instantiated", "pods_bind"]
    assert ctx.calls[2][1:] == (["n1"],)
    assert q.node_index("n1") == 6 and q.node_name(6) == "n1" and q.node_name(1) is None
    assert ctx.calls[3][1:] == ([6], [UNKNOWN], [0])
    assert ctx.calls[4][1:] == ([6], [321])
    assert ctx.calls[5][1:] == ([1, 4], [6, 6])                         # p1 and p4 name n1
    assert out == dict(ZERO, checked=6, absent=1) and q.touched_nodes
    assert [n["name"] for n in q.live_nodes()] == ["n0", "n2", "n3", "n4", "n5", "n1"]
    ctx.status = {}
    ctx.calls.clear()
    assert q.resync_nodes(ctx) == dict(ZERO, checked=6)
    assert ctx.calls[0][1] == [0, 6, 2, 3, 4, 5]                        # the store's order, the new index


def test_limit_from_the_repair_relabel_rebuilds_when_enabled():
    q, ctx = loaded({"n3": NV_SHAPE}, rebuild=True)
    ctx.fail_at = 1                                                    # events: nodes_relabel!
    out = q.resync_nodes(ctx)
    assert ctx.names() == ["nodes_verify", "nodes_live_ids", "nodes_relabel!", "nodes_rebuild", "nodes_relabel"]
    assert ctx.calls[2][1:] == ctx.calls[4][1:] == ([3], ["n3"])
    assert (q.rebuilds, q.rebuild_causes, q.reloads) == (1, ["nodes_relabel"], 1)
    assert out == dict(ZERO, checked=6, shape=1)


def test_limit_from_the_repair_add_compacts_when_enabled():
    q, ctx = loaded({"n4": NV_ABSENT, "n5": NV_STATUS}, compact=True, room=(0, 0))
    ctx.live.discard(4)
    ctx.fail_at = 1                                                    # events: nodes_add!
    out = q.resync_nodes(ctx)
    assert ctx.names() == ["nodes_verify", "nodes_live_ids", "nodes_add!", "nodes_compact", "nodes_add", "nodes_update",
                           "nodes_facts"]
    assert ctx.calls[3][1:] == (1, 0)
    assert (q.compactions, q.compact_causes, q.reloads) == (1, ["nodes_add"], 1)
    # the compaction renumbered n5 from slot 5 to 4; the node added again follows it
    assert ctx.calls[5][1] == [4] and q.node_index("n4") == 5 and ctx.calls[6][1] == [5]
    assert out == dict(ZERO, checked=6, absent=1, status=1)


def test_limit_from_a_repair_reloads_otherwise():
    q, ctx = loaded({"n3": NV_SHAPE, "n4": NV_FACTS}, extra=[8])
    q.inst_ns["n0"] = 5
    ctx.fail_at = 2                                                    # events: nodes_delete, nodes_relabel!
    out = q.resync_nodes(ctx)
    assert ctx.names() == ["nodes_verify", "nodes_live_ids", "nodes_delete", "nodes_relabel!", "load", "load_placement",
                           "nodes_instantiated"]
    assert ctx.calls[4][2] == ["n%d" % j for j in range(6)]            # the whole store, in index order
    assert out == dict(ZERO, checked=6, shape=1, facts=1, orphans=1, reloaded=True)
    assert (q.reloads, q.reload_causes) == (2, ["first", "resync_nodes:nodes_relabel"])


def test_the_pod_resync_still_works_on_a_context_without_node_calls():
    q, ctx = EventQueue(spare=0.5), VerifyRec()
    for j in range(2):
        q.node_add(node("n%d" % j))
    for i in range(3):
        q.pod_add(pod("p%d" % i, "n%d" % (i % 2)))
    q.flush(ctx)
    ctx.calls.clear()
    assert not hasattr(ctx, "nodes_verify") and not hasattr(ctx, "nodes_live_ids")
    out = q.resync(ctx)
    assert ctx.names() == ["pods_verify", "pods_live_ids"]
    assert ctx.calls[0][3] == [0, 1, 0] and NONE not in ctx.calls[0][3]
    assert out == {"checked": 3, "absent": 0, "class": 0, "value": 0, "bind": 0, "orphans": 0, "reloaded": False}
    assert q.node_resyncs == 0 and q.resyncs == 1


def test_the_controller_resyncs_the_nodes_every_kth_scan_before_the_decision():
    import test_audit_host as H

    c = H._ctl(0)
    seen = []

    def resync_nodes(ctx):
        seen.append((c.scans, "decide" in c.ctx.calls[mark[0]:]))
        return {"checked": 0}
    mark = [0]
    c.events.resync_nodes = resync_nodes
    c.node_resync_every, c.node_resyncs, c.last_node_resync = 3, 0, None
    for _ in range(7):
        mark[0] = len(c.ctx.calls)
        c.run_once()
    assert seen == [(3, False), (6, False)]                            # the 3rd and the 6th scan, before their decision
    assert c.node_resyncs == 2 and c.last_node_resync == {"checked": 0}
    c2 = H._ctl(0)
    c2.events.resync_nodes = lambda ctx: (_ for _ in ()).throw(AssertionError("off by default"))
    for _ in range(4):
        c2.run_once()
    assert c2.node_resyncs == 0 and c2.node_resync_every is None
