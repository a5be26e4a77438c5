"""CPU: EventQueue(pod_grow=True) against the recording stand-in context of
tests/test_event_queue.py — a pods_upsert that answers ESC_E_LIMIT is answered by one pods_grow
with the same ids and packed batch and one retry, a second limit reloads, and the counters
stand beside rebuilds / compactions."""
import pytest

from escalator_amd._lib import ESC_E_INVAL, ESC_E_LIMIT
from escalator_amd.events import EventQueue
from test_event_queue import Rec, Refused, node, pod


class GrowRec(Rec):
    def pods_grow(self, ids, P):
        self._event("pods_grow", [int(i) for i in ids], list(P["keys"]))


def loaded(pod_grow, fail_at=None, code=ESC_E_LIMIT):
    q, ctx = EventQueue(spare=0.5, pod_grow=pod_grow), GrowRec()
    for j in range(2):
        q.node_add(node("n%d" % j))
    for i in range(3):
        q.pod_add(pod("p%d" % i, "n%d" % (i % 2)))
    q.flush(ctx)
    ctx.calls.clear()
    ctx.events, ctx.fail_at, ctx.code = 0, fail_at, code
    return q, ctx


def burst(q):
    q.pod_delete("p1")
    q.pod_add(pod("b0", "n0"))
    q.pod_add(pod("b1"))
    q.pod_add(pod("p0", "n0", cpu=900))                 # a changed spec: in the same upsert


def test_limit_is_answered_by_one_grow_and_one_retry():
    q, ctx = loaded(True, fail_at=2)                    # events: pods_delete, pods_upsert!, ...
    burst(q)
    q.flush(ctx)
    assert ctx.names() == ["pods_delete", "pods_upsert!", "pods_grow", "pods_upsert", "pods_bind"]
    refused, grow, retry = ctx.calls[1], ctx.calls[2], ctx.calls[3]
    assert grow[1:] == refused[1:] == retry[1:]         # the same ids and the same packed batch
    assert grow[1] == [1, 3, 0] and grow[2] == ["b0", "b1", "p0"]      # the freed id is reused first
    assert (q.pod_grows, q.pod_grow_causes, q.reloads) == (1, ["pods_upsert"], 1)
    assert (q.rebuilds, q.compactions) == (0, 0)
    assert q.applied["pods_upsert"] == 3 and q.applied["pods_bind"] == 2
    assert q.reload_causes == ["first"]
    # the next scan's upsert goes straight through
    q.pod_add(pod("b2"))
    q.flush(ctx)
    assert ctx.names()[5:] == ["pods_upsert", "pods_bind"] and q.pod_grows == 1


def test_second_limit_reloads():
    q, ctx = loaded(True, fail_at=2)
    orig = ctx._event

    def event(name, *args):                             # the retry is refused too
        if name == "pods_upsert" and any(c[0] == "pods_grow" for c in ctx.calls):
            ctx.calls.append(("pods_upsert!",) + args)
            return ESC_E_LIMIT
        return orig(name, *args)
    ctx._event = event
    burst(q)
    q.flush(ctx)
    assert ctx.names() == ["pods_delete", "pods_upsert!", "pods_grow", "pods_upsert!", "load", "load_placement"]
    assert (q.pod_grows, q.reloads, q.reload_causes) == (1, 2, ["first", "pods_upsert"])
    assert ctx.calls[4][1] == ["p0", "b0", "p2", "b1"]  # the reload carries the whole store, in pod-id order
    assert q.applied["pods_upsert"] == 0


def test_a_grow_that_answers_limit_reloads_without_a_retry():
    q, ctx = loaded(True, fail_at=2)
    orig = ctx._event

    def event(name, *args):                             # a pod no spare C slot holds
        if name == "pods_grow":
            ctx.calls.append(("pods_grow!",) + args)
            raise Refused(ESC_E_LIMIT)
        return orig(name, *args)
    ctx._event = event
    burst(q)
    q.flush(ctx)
    assert ctx.names() == ["pods_delete", "pods_upsert!", "pods_grow!", "load", "load_placement"]
    assert (q.pod_grows, q.pod_grow_causes, q.reloads) == (0, [], 2)


def test_switch_off_reloads_as_before():
    q, ctx = loaded(False, fail_at=2)
    burst(q)
    q.flush(ctx)
    assert ctx.names() == ["pods_delete", "pods_upsert!", "load", "load_placement"]
    assert (q.pod_grows, q.pod_grow_causes, q.reloads) == (0, [], 2)
    assert EventQueue().pod_grow is False


def test_other_errors_pass_through():
    q, ctx = loaded(True)
    orig = ctx._event

    def event(name, *args):
        if name == "pods_grow":
            raise Refused(ESC_E_INVAL)
        if name == "pods_upsert":
            return ESC_E_LIMIT
        return orig(name, *args)
    ctx._event = event
    burst(q)
    with pytest.raises(Refused):
        q.flush(ctx)
    assert q.pod_grows == 0


def test_resident_controller_passes_the_switch_on():
    import inspect

    from escalator_amd.controller import ResidentController
    sig = inspect.signature(ResidentController.__init__)
    assert sig.parameters["pod_grow"].default is False
    src = inspect.getsource(ResidentController.__init__)
    assert "pod_grow=self.pod_grow" in src
