"""CPU: ResidentController's dry-mode tracker mirror with stand-ins — after a flush that
added nodes or reloaded, every tracked name with a live node is tracked on the device again
(a reload drops the device's tracker; a node back under a tracked name has a new index); a
tracked name whose node is gone stays in the list and asks for nothing."""
import numpy as np

from escalator_amd.controller import ResidentController


class _Events:
    def __init__(self, index):
        self.index = index

    def node_index(self, name):
        return self.index.get(name)


class _Ctx:
    def __init__(self, tracked):
        self.tracked, self.calls = tracked, []

    def tracker_list(self, g):
        return np.array(sorted(self.tracked.get(g, [])), np.int64)

    def tracker_update(self, g, add=(), remove=()):
        self.calls.append((g, list(add), list(remove)))


def _ctl(trackers, index, tracked):
    c = ResidentController.__new__(ResidentController)
    c.taint_tracker, c.events, c.ctx = trackers, _Events(index), _Ctx(tracked)
    return c


def test_missing_tracked_names_are_re_added():
    c = _ctl({0: [], 1: ["a", "gone", "b", "c"], 2: ["d"], 3: ["gone"]},
             {"a": 4, "b": 9, "c": 2, "d": 7}, {1: [9], 2: [7]})
    c._sync_trackers()
    assert c.ctx.calls == [(1, [2, 4], [])]            # b is tracked already, "gone" has no node
    assert c.taint_tracker[1] == ["a", "gone", "b", "c"] and c.taint_tracker[3] == ["gone"]


def test_nothing_missing_issues_no_call():
    c = _ctl({0: ["a"], 1: []}, {"a": 0}, {0: [0]})
    c._sync_trackers()
    assert c.ctx.calls == []
