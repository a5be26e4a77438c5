"""CPU: esc_nodes_compact's ABI surface and EventQueue's compact-then-retry rule against a
recording stand-in context.

The library exports the symbol with the header's signature and the ABI stays at 6; NULL is
ESC_E_INVAL, a context without a device ESC_E_NODEV, a negative minimum ESC_E_INVAL.  With
``compact=True`` a nodes_add that answers ESC_E_LIMIT while nodes_room shows too few slots is
followed by one nodes_compact with the batch's slots, the same call again and the rest of the
flush, the queue's index maps following the returned map; a pods_bind that answers ESC_E_LIMIT
is answered the same way; a second ESC_E_LIMIT reloads; with ``compact=False`` the calls are
today's, with ``rebuild`` on and off."""
import ctypes as C
import os
import re

import numpy as np

from escalator_amd import _lib as L
from escalator_amd.context import Context
from escalator_amd.controller import ResidentController
from escalator_amd.events import EventQueue
from test_event_queue import node, pod
from test_rebuild_host import RecR, _churn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the ABI
def test_library_exports_the_symbol_with_the_headers_signature():
    lib = L.load()
    assert hasattr(lib, "esc_nodes_compact")
    assert lib.esc_abi_version() == 6                       # additive: the version stays
    assert "esc_nodes_compact" in L.header_functions()
    i64 = C.c_int64
    assert L._SIGS["esc_nodes_compact"] == (C.c_int32, [C.c_void_p, i64, i64, C.POINTER(i64), i64])
    header = open(os.path.join(ROOT, "include", "escalator_hip.h")).read()
    assert re.search(r"int32_t esc_nodes_compact\(esc_ctx\* ctx, int64_t min_free_slots, int64_t min_free_xl_words,\s*"
                     r"int64_t\* new_index, int64_t cap\);", header)


def test_null_no_device_and_negative_minima():
    lib = L.load()
    out = (C.c_int64 * 4)(7, 7, 7, 7)
    assert lib.esc_nodes_compact(None, 0, 0, out, 4) == L.ESC_E_INVAL
    ctx = Context([{"name": "a", "label_key": "k", "label_value": "v"}], device=-1)
    assert ctx.lib.esc_nodes_compact(ctx.handle, 0, 0, out, 4) == L.ESC_E_NODEV
    assert ctx.lib.esc_nodes_compact(ctx.handle, 0, 0, None, 0) == L.ESC_E_NODEV
    assert ctx.lib.esc_nodes_compact(ctx.handle, -1, 0, out, 4) == L.ESC_E_INVAL
    assert ctx.lib.esc_nodes_compact(ctx.handle, 0, -1, out, 4) == L.ESC_E_INVAL
    assert ctx.lib.esc_nodes_compact(ctx.handle, 0, 0, None, 4) == L.ESC_E_INVAL
    assert list(out) == [7, 7, 7, 7]
    try:
        ctx.nodes_compact()
    except L.EscError as e:
        assert e.code == L.ESC_E_NODEV
    else:
        raise AssertionError("nodes_compact on device=-1 did not raise")


# ------------------------------------------------------------------ EventQueue
class RecC(RecR):
    """RecR with nodes_compact: the live indices (those never deleted) renumbered densely."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.dead = set()

    def load(self, P, N):
        self.dead = set()
        return super().load(P, N)

    def nodes_delete(self, ids):
        super().nodes_delete(ids)
        self.dead |= {int(j) for j in ids}

    def nodes_compact(self, min_free_slots=0, min_free_xl_words=0):
        self.calls.append(("nodes_compact", int(min_free_slots), int(min_free_xl_words)))
        out, k = np.full(self.hw, -1, np.int64), 0
        for j in range(self.hw):
            if j not in self.dead:
                out[j], k = k, k + 1
        self.hw, self.dead = k, set()
        self.room = max(self.room, min_free_slots)
        return out


def _loaded(ctx, **kw):
    q = EventQueue(spare=0.5, **kw)
    for j in range(3):
        q.node_add(node("n%d" % j))
    for i in range(4):
        q.pod_add(pod("p%d" % i, "n%d" % (i % 3)))
    q.flush(ctx)
    ctx.calls.clear()
    ctx.events = 0
    return q


def test_add_without_slots_compacts_remaps_and_retries():
    ctx = RecC(fail={2}, room=1)                               # event 1: nodes_delete, 2: nodes_add; two adds, one slot
    q = _loaded(ctx, compact=True)
    assert q.rebuild                                           # compact=True implies the rebuild rule
    _churn(q)                                                  # deletes n0 (index 0), adds new0 and new1
    q.flush(ctx)
    assert ctx.names() == ["nodes_delete", "nodes_add!", "nodes_room", "nodes_compact", "nodes_add", "nodes_relabel",
                           "nodes_update", "nodes_facts", "pods_upsert", "pods_bind"]
    assert ctx.calls[3] == ("nodes_compact", 2, 0)             # the batch's slots
    assert (q.reloads, q.rebuilds, q.compactions, q.compact_causes) == (1, 0, 1, ["nodes_add"])
    assert q.touched_nodes
    # n1, n2 moved down over the deleted slot; the new nodes follow them
    assert [q.node_index(m) for m in ("n0", "n1", "n2", "new0", "new1")] == [None, 0, 1, 2, 3]
    assert [q.node_name(j) for j in range(5)] == ["n1", "n2", "new0", "new1", None]
    # the calls after the compaction carry the new indices
    by = {c[0]: c for c in ctx.calls}
    assert by["nodes_relabel"][1] == [0] and by["nodes_update"][1] == [1]
    assert sorted(by["nodes_facts"][1]) == [2, 3]
    assert by["pods_bind"][2][by["pods_bind"][1].index(q.pod_id("late"))] == 3


def test_add_with_slots_rebuilds_as_before():
    ctx = RecC(fail={2}, room=100)
    q = _loaded(ctx, compact=True)
    _churn(q)
    q.flush(ctx)
    assert ctx.names()[:5] == ["nodes_delete", "nodes_add!", "nodes_room", "nodes_rebuild", "nodes_add"]
    assert (q.rebuilds, q.compactions, q.rebuild_causes) == (1, 0, ["nodes_add"])


def test_relabel_limit_rebuilds_never_compacts():
    ctx = RecC(fail={3}, room=0)
    q = _loaded(ctx, compact=True)
    _churn(q)
    q.flush(ctx)
    assert ctx.names()[:5] == ["nodes_delete", "nodes_add", "nodes_relabel!", "nodes_rebuild", "nodes_relabel"]
    assert (q.rebuilds, q.compactions) == (1, 0)


def test_second_limit_after_the_compaction_reloads():
    ctx = RecC(fail={2, 3}, room=0)
    q = _loaded(ctx, compact=True)
    _churn(q)
    q.flush(ctx)
    assert ctx.names() == ["nodes_delete", "nodes_add!", "nodes_room", "nodes_compact", "nodes_add!", "load",
                           "load_placement"]
    assert q.reloads == 2 and q.reload_causes == ["first", "nodes_add"] and q.compactions == 1
    assert [q.node_index(m) for m in ("n1", "n2", "new0", "new1")] == [0, 1, 2, 3]


def test_bind_limit_compacts_once_and_retries():
    ctx = RecC(fail={7})                                       # pods_bind
    q = _loaded(ctx, compact=True)
    _churn(q)
    q.flush(ctx)
    assert ctx.names()[-4:] == ["pods_upsert", "pods_bind!", "nodes_compact", "pods_bind"]
    assert ctx.calls[-2] == ("nodes_compact", 0, 0)
    assert (q.reloads, q.compactions, q.compact_causes) == (1, 1, ["pods_bind"])
    first, again = ctx.calls[-3], ctx.calls[-1]
    assert first[1] == again[1]                                # the same pods,
    assert first[2][first[1].index(q.pod_id("late"))] == 4     # bound to new1 at its old index, then
    assert again[2][again[1].index(q.pod_id("late"))] == 3     # at its new one
    # a second limit reloads
    ctx = RecC(fail={7, 8})
    q = _loaded(ctx, compact=True)
    _churn(q)
    q.flush(ctx)
    assert ctx.names()[-5:] == ["pods_bind!", "nodes_compact", "pods_bind!", "load", "load_placement"]
    assert q.reload_causes == ["first", "pods_bind"] and q.compactions == 1


def test_compact_off_is_todays_sequence():
    """compact=False (and the default), with rebuild on and off: the recorded calls are the
    ones today's queue makes — nodes_compact is never called, whichever call is refused."""
    for rebuild in (False, True):
        for fail, room in (({2}, 1), ({2}, 100), ({3}, 100), ({7}, 100), ({2, 3}, 100)):
            seen = []
            for kw in ({"rebuild": rebuild}, {"rebuild": rebuild, "compact": False}):
                ctx = RecC(fail=fail, room=room)
                q = _loaded(ctx, **kw)
                _churn(q)
                q.flush(ctx)
                seen.append(repr(ctx.calls))
                assert "nodes_compact" not in ctx.names() and q.compactions == 0 and q.compact_causes == []
                if not rebuild:
                    assert "nodes_room" not in ctx.names() and "nodes_rebuild" not in ctx.names()
                    assert q.reloads == 2
                if fail == {7}:
                    assert ctx.names()[-3:] == ["pods_bind!", "load", "load_placement"]
                if rebuild and fail == {2} and room == 1:
                    assert ctx.names() == ["nodes_delete", "nodes_add!", "nodes_room", "load", "load_placement"]
            assert seen[0] == seen[1]


def test_both_switches_are_off_by_default():
    import inspect
    assert inspect.signature(EventQueue.__init__).parameters["compact"].default is False
    assert inspect.signature(ResidentController.__init__).parameters["node_compact"].default is False
    q = EventQueue()
    assert not q.compact and not q.rebuild and (q.compactions, q.compact_causes) == (0, [])
    assert not EventQueue(rebuild=True).compact
