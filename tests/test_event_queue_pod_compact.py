"""CPU: EventQueue(pod_compact=frac) against the recording stand-in context of
tests/test_event_queue.py — after a flush that applied cleanly, one pods_compact when
(k_tiles - k_tiles_rule) * 256 + parked >= frac * live pods; the counters; off by default; a
failed compaction does not abort the flush."""
import pytest

from escalator_amd._lib import ESC_E_HIP, ESC_E_STATE
from escalator_amd.events import EventQueue
from test_event_queue import Rec, Refused, node, pod


class SlackRec(Rec):
    """Answers pods_slack with what the test sets; pods_compact clears it (or fails)."""

    slack = {"k_tiles": 0, "k_tiles_rule": 0, "parked": 0}
    fail = None
    swapped = False                                     # the failure comes after the swap: the context is stale
    stale = False

    def pods_slack(self):
        if self.stale:
            self.calls.append(("pods_slack!",))
            raise Refused(ESC_E_STATE)
        self.calls.append(("pods_slack",))
        return dict(self.slack)

    def load(self, P, N):
        self.stale = False
        super().load(P, N)

    def pods_compact(self):
        if self.fail is not None:
            self.calls.append(("pods_compact!",))
            self.stale = self.swapped
            raise Refused(self.fail)
        self.calls.append(("pods_compact",))
        self.slack = dict(self.slack, k_tiles=self.slack["k_tiles_rule"], parked=0)
        return {"moved": 1}


def loaded(pod_compact, n_pods=1024):
    q, ctx = EventQueue(spare=0.5, pod_compact=pod_compact), SlackRec()
    q.node_add(node("n0"))
    for i in range(n_pods):
        q.pod_add(pod("p%d" % i))
    q.flush(ctx)                                        # the first load: no slack question
    assert ctx.names() == ["set_spare", "load", "load_placement"]
    ctx.calls.clear()
    return q, ctx


def touch(q, i=0):
    q.pod_add(pod("p%d" % i, cpu=900 + i))              # one changed spec: a flush with one upsert


def test_off_by_default():
    q, ctx = loaded(None)
    assert q.pod_compact is None
    ctx.slack = {"k_tiles": 100, "k_tiles_rule": 1, "parked": 500}
    touch(q)
    q.flush(ctx)
    assert ctx.names() == ["pods_upsert"] and q.pod_compacts == 0


@pytest.mark.parametrize("slack, parked, fires, cause", [
    ({"k_tiles": 5, "k_tiles_rule": 4}, 0, True, "slack"),        # 256 = 0.25 * 1024: at the threshold
    ({"k_tiles": 5, "k_tiles_rule": 4}, -1, False, None),         # (a count the device never gives: one below)
    ({"k_tiles": 4, "k_tiles_rule": 4}, 256, True, "parked"),
    ({"k_tiles": 4, "k_tiles_rule": 4}, 255, False, None),        # one below
    ({"k_tiles": 4, "k_tiles_rule": 4}, 0, False, None),
    ({"k_tiles": 5, "k_tiles_rule": 5}, 300, True, "parked"),
    ({"k_tiles": 4, "k_tiles_rule": 5}, 512, True, "parked"),     # a class short of its rule: 512 - 256 = 256
    ({"k_tiles": 4, "k_tiles_rule": 5}, 511, False, None),
])
def test_trigger_arithmetic(slack, parked, fires, cause):
    q, ctx = loaded(0.25)
    ctx.slack = dict(slack, parked=parked)
    touch(q)
    q.flush(ctx)
    assert ctx.names() == ["pods_upsert", "pods_slack"] + (["pods_compact"] if fires else [])
    assert q.pod_compacts == int(fires) and q.pod_compact_causes == ([cause] if fires else [])
    assert q.reloads == 1 and q.pod_compact_failures == 0


def test_threshold_follows_the_live_pods():
    q, ctx = loaded(0.25)
    ctx.slack = {"k_tiles": 5, "k_tiles_rule": 4, "parked": 0}
    q.pod_add(pod("extra"))                             # 1025 live pods: 256 < 256.25
    q.flush(ctx)
    assert "pods_compact" not in ctx.names() and q.pod_compacts == 0
    q.pod_delete("extra")
    q.flush(ctx)
    assert ctx.names()[-2:] == ["pods_slack", "pods_compact"] and q.pod_compact_causes == ["slack"]
    # compacted: the next flush asks and finds nothing
    touch(q, 1)
    q.flush(ctx)
    assert ctx.names()[-2:] == ["pods_upsert", "pods_slack"] and q.pod_compacts == 1


def test_zero_fraction_needs_some_slack():
    q, ctx = loaded(0.0)
    touch(q)
    q.flush(ctx)
    assert ctx.names() == ["pods_upsert", "pods_slack"] and q.pod_compacts == 0


def test_a_failed_compaction_does_not_abort_the_flush():
    q, ctx = loaded(0.25)
    ctx.slack = {"k_tiles": 9, "k_tiles_rule": 4, "parked": 3}
    ctx.fail = ESC_E_HIP
    touch(q)
    q.pod_add(pod("late", "n0"))
    q.flush(ctx)                                        # no exception
    assert ctx.names() == ["pods_upsert", "pods_bind", "pods_slack", "pods_compact!", "pods_slack"]
    assert (q.pod_compacts, q.pod_compact_causes, q.pod_compact_failures, q.reloads) == (0, [], 1, 1)
    assert q.applied["pods_upsert"] == 2 and q.pod_id("late") == 1024
    ctx.fail = None                                     # the next flush tries again
    touch(q, 2)
    q.flush(ctx)
    assert ctx.names()[-1] == "pods_compact" and (q.pod_compacts, q.pod_compact_causes) == (1, ["slack"])


def test_no_compaction_after_a_reload():
    q, ctx = loaded(0.25)
    ctx.slack = {"k_tiles": 9, "k_tiles_rule": 4, "parked": 0}
    ctx.events, ctx.fail_at = 0, 1                      # the upsert answers ESC_E_LIMIT: one reload
    touch(q)
    q.flush(ctx)
    assert ctx.names() == ["pods_upsert!", "load", "load_placement"] and q.reloads == 2 and q.pod_compacts == 0


def test_a_compaction_that_fails_after_its_swap_reloads_at_once():
    q, ctx = loaded(0.25)
    ctx.slack = {"k_tiles": 9, "k_tiles_rule": 4, "parked": 0}
    ctx.fail, ctx.swapped = ESC_E_HIP, True
    touch(q)
    q.pod_add(pod("late", "n0"))
    q.flush(ctx)                                        # no exception: the stale snapshot is reloaded
    assert ctx.names() == ["pods_upsert", "pods_bind", "pods_slack", "pods_compact!", "pods_slack!", "load",
                           "load_placement"]
    assert (q.pod_compacts, q.pod_compact_failures, q.reloads) == (0, 1, 2)
    assert q.reload_causes == ["first", "pods_compact"]
    assert "late" in ctx.calls[-2][1] and q.pod_id("late") is not None     # the reload holds what the flush applied
    ctx.fail = None
    touch(q, 3)
    q.flush(ctx)                                        # and the loop goes on
    assert ctx.names()[-3:] == ["pods_upsert", "pods_slack", "pods_compact"] and q.pod_compacts == 1
