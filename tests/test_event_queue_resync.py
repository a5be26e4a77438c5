"""CPU: EventQueue.resync against the recording stand-in context of tests/test_event_queue.py with a
scripted pods_verify: the flush comes first, the object store is verified in chunks with the ids
of the identity map and the targets of the binding, the repairs are exactly one pods_upsert, one
pods_bind and one pods_delete in that order with the right ids, a clean verify issues none, and
an ESC_E_LIMIT from the repair upsert takes the flush's grow or reload path."""
import logging

import numpy as np

from escalator_amd._lib import PV_ABSENT, PV_BIND, PV_CLASS, PV_VALUE
from escalator_amd.events import NONE, EventQueue
from test_event_queue import Rec, node, pod


class VerifyRec(Rec):
    """Rec with a scripted verify: `status` maps a pod's key to its status byte, `extra` are
    ids the device holds beyond the ones it was given."""

    def __init__(self, status=None, extra=()):
        super().__init__()
        self.status, self.extra, self.live = dict(status or {}), list(extra), set()

    def load(self, P, N):
        super().load(P, N)
        self.live = set(range(len(P["keys"])))

    def pods_upsert(self, ids, P):
        rc = super().pods_upsert(ids, P)
        if rc == 0:
            self.live |= {int(i) for i in ids}
        return rc

    def pods_delete(self, ids):
        super().pods_delete(ids)
        self.live -= {int(i) for i in ids}

    def pods_grow(self, ids, P):
        self._event("pods_grow", [int(i) for i in ids], list(P["keys"]))

    def pods_verify(self, ids, P, pod_node=None):
        self.calls.append(("pods_verify", [int(i) for i in ids], list(P["keys"]), [int(j) for j in pod_node]))
        st = np.array([self.status.get(k, 0) for k in P["keys"]], np.uint8)
        return st, {"n_checked": len(st)}

    def pods_live_ids(self):
        self.calls.append(("pods_live_ids",))
        return np.array(sorted(self.live | set(self.extra)), np.int64)


def loaded(status=None, extra=(), **kw):
    q, ctx = EventQueue(spare=0.5, **kw), VerifyRec(status, extra)
    for j in range(2):
        q.node_add(node("n%d" % j))
    for i in range(6):
        q.pod_add(pod("p%d" % i, "n%d" % (i % 2) if i < 4 else ""))
    q.flush(ctx)
    ctx.calls.clear()
    ctx.events = 0
    return q, ctx


def test_a_clean_verify_repairs_nothing():
    q, ctx = loaded()
    out = q.resync(ctx)
    assert ctx.names() == ["pods_verify", "pods_live_ids"]
    assert ctx.calls[0][1:] == ([0, 1, 2, 3, 4, 5], ["p%d" % i for i in range(6)], [0, 1, 0, 1, NONE, NONE])
    assert out == {"checked": 6, "absent": 0, "class": 0, "value": 0, "bind": 0, "orphans": 0, "reloaded": False}
    assert (q.resyncs, q.reloads, q.flushes) == (1, 1, 2)
    assert q.resync_repairs == {"absent": 0, "class": 0, "value": 0, "bind": 0, "orphans": 0}


def test_it_flushes_first_and_verifies_in_chunks():
    q, ctx = loaded()
    q.pod_add(pod("p6", "n1"))
    q.pod_delete("p0")
    out = q.resync(ctx, chunk=4)
    assert ctx.names() == ["pods_delete", "pods_upsert", "pods_bind", "pods_verify", "pods_verify", "pods_live_ids"]
    assert ctx.calls[3][1:] == ([1, 2, 3, 4], ["p1", "p2", "p3", "p4"], [1, 0, 1, NONE])
    assert ctx.calls[4][1:] == ([5, 0], ["p5", "p6"], [NONE, 1])       # the freed id went to the new pod
    assert out["checked"] == 6 and not any(out[k] for k in ("absent", "class", "value", "bind", "orphans"))


def test_one_call_per_kind_with_the_right_ids_in_order(caplog):
    status = {"p1": PV_VALUE, "p2": PV_BIND, "p3": PV_CLASS | PV_BIND, "p5": PV_ABSENT}
    q, ctx = loaded(status, extra=[9, 11])
    ctx.live.discard(5)
    with caplog.at_level(logging.WARNING, logger="escalator_amd.events"):
        out = q.resync(ctx)
    assert ctx.names() == ["pods_verify", "pods_live_ids", "pods_upsert", "pods_bind", "pods_delete"]
    assert ctx.calls[2][1:] == ([1, 3, 5], ["p1", "p3", "p5"])
    assert ctx.calls[3][1:] == ([2, 3], [0, 1])
    assert ctx.calls[4][1:] == ([9, 11],)
    assert out == {"checked": 6, "absent": 1, "class": 1, "value": 1, "bind": 2, "orphans": 2, "reloaded": False}
    assert q.resync_repairs == {"absent": 1, "class": 1, "value": 1, "bind": 2, "orphans": 2}
    warned = [r.getMessage() for r in caplog.records if r.name == "escalator_amd.events"]
    assert len(warned) == 5 and all(m.startswith("resync: ") for m in warned)     # one per kind, with its count
    assert q.reloads == 1 and q.resyncs == 1
    # the device's view follows: a second pass over a clean device reports nothing
    ctx.status, ctx.extra = {}, []
    ctx.calls.clear()
    again = q.resync(ctx)
    assert ctx.names() == ["pods_verify", "pods_live_ids"]
    assert not any(again[k] for k in ("absent", "class", "value", "bind", "orphans"))
    assert q.resync_repairs["bind"] == 2 and q.resyncs == 2


def test_limit_from_the_repair_upsert_grows_when_enabled():
    q, ctx = loaded({"p1": PV_VALUE, "p4": PV_ABSENT}, pod_grow=True)
    ctx.fail_at = 1                                     # events: pods_upsert!
    out = q.resync(ctx)
    assert ctx.names() == ["pods_verify", "pods_live_ids", "pods_upsert!", "pods_grow", "pods_upsert"]
    assert ctx.calls[2][1:] == ctx.calls[3][1:] == ctx.calls[4][1:] == ([1, 4], ["p1", "p4"])
    assert (q.pod_grows, q.pod_grow_causes, q.reloads) == (1, ["pods_upsert"], 1)
    assert out["reloaded"] is False and (out["value"], out["absent"]) == (1, 1)


def test_limit_from_the_repair_upsert_reloads_otherwise():
    q, ctx = loaded({"p1": PV_VALUE, "p2": PV_BIND}, extra=[8])
    ctx.fail_at = 1
    out = q.resync(ctx)
    assert ctx.names() == ["pods_verify", "pods_live_ids", "pods_upsert!", "load", "load_placement"]
    assert ctx.calls[3][1] == ["p%d" % i for i in range(6)]            # the whole store, in pod-id order
    assert out["reloaded"] is True and (out["value"], out["bind"], out["orphans"]) == (1, 1, 1)
    assert (q.reloads, q.reload_causes) == (2, ["first", "resync:pods_upsert"])
    assert q.pod_grows == 0


def test_the_controller_resyncs_every_kth_scan_in_place_of_the_flush():
    import test_audit_host as H

    c = H._ctl(0)
    seen = []
    c.events.resync = lambda ctx: seen.append(c.scans) or {"checked": 0}
    c.resync_every, c.resyncs, c.last_resync = 3, 0, None
    for _ in range(7):
        c.run_once()
    assert seen == [2, 5] and c.resyncs == 2 and c.last_resync == {"checked": 0}      # the 3rd and the 6th scan
    c2 = H._ctl(0)
    c2.events.resync = lambda ctx: (_ for _ in ()).throw(AssertionError("off by default"))
    for _ in range(4):
        c2.run_once()
    assert c2.resyncs == 0 and c2.resync_every is None
