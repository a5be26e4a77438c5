"""CPU: esc_nodes_rebuild / esc_nodes_room's ABI surface, EventQueue's rebuild-then-retry rule
and ResidentController's answer to an audit mismatch, against stand-in contexts.

The library exports the two symbols with the header's signatures and the ABI stays at 6; NULL is
ESC_E_INVAL and a context without a device ESC_E_NODEV.  With ``rebuild=True`` a nodes_add or
nodes_relabel that answers ESC_E_LIMIT is followed by nodes_room (adds only), nodes_rebuild and
the same call again, then the rest of the flush; a second ESC_E_LIMIT, or too few free slots,
reloads as before; with ``rebuild=False`` the calls are today's."""
import ctypes as C
import os
import re

from escalator_amd import _lib as L
from escalator_amd.context import Context
from escalator_amd.controller import ResidentController
from escalator_amd.events import EventQueue
from test_audit_host import CLEAN, _Ctx
from test_event_queue import Rec, node, pod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the ABI
def test_library_exports_the_two_symbols_with_the_headers_signatures():
    lib = L.load()
    assert hasattr(lib, "esc_nodes_rebuild") and hasattr(lib, "esc_nodes_room")
    assert lib.esc_abi_version() == 6                       # additive: the version stays
    fns = L.header_functions()
    assert "esc_nodes_rebuild" in fns and "esc_nodes_room" in fns
    i32, i64p = C.c_int32, C.POINTER(C.c_int64)
    assert L._SIGS["esc_nodes_rebuild"] == (i32, [C.c_void_p])
    assert L._SIGS["esc_nodes_room"] == (i32, [C.c_void_p, i64p, i64p])
    header = open(os.path.join(ROOT, "include", "escalator_hip.h")).read()
    assert re.search(r"int32_t esc_nodes_rebuild\(esc_ctx\* ctx\);", header)
    assert re.search(r"int32_t esc_nodes_room\(const esc_ctx\* ctx, int64_t\* free_slots, int64_t\* free_xl_words\);", header)


def test_null_and_no_device():
    lib = L.load()
    a, b = C.c_int64(-1), C.c_int64(-1)
    assert lib.esc_nodes_rebuild(None) == L.ESC_E_INVAL
    assert lib.esc_nodes_room(None, C.byref(a), C.byref(b)) == L.ESC_E_INVAL
    ctx = Context([{"name": "a", "label_key": "k", "label_value": "v"}], device=-1)
    assert ctx.lib.esc_nodes_rebuild(ctx.handle) == L.ESC_E_NODEV
    assert ctx.lib.esc_nodes_room(ctx.handle, C.byref(a), C.byref(b)) == L.ESC_E_NODEV
    assert (a.value, b.value) == (-1, -1)
    for call in (ctx.nodes_rebuild, ctx.nodes_room):
        try:
            call()
        except L.EscError as e:
            assert e.code == L.ESC_E_NODEV
        else:
            raise AssertionError("%s on device=-1 did not raise" % call.__name__)


# ------------------------------------------------------------------ EventQueue
class RecR(Rec):
    """Rec with the two new calls: `room` free table slots; ESC_E_LIMIT at every event call
    whose number is in `fail`."""

    def __init__(self, fail=(), room=100):
        super().__init__()
        self.fail, self.room = set(fail), room

    def _event(self, name, *args):
        self.fail_at = self.events + 1 if self.events + 1 in self.fail else None
        return super()._event(name, *args)

    def nodes_room(self):
        self.calls.append(("nodes_room",))
        return self.room, 1000

    def nodes_rebuild(self):
        self.calls.append(("nodes_rebuild",))


def _loaded(rebuild, **kw):
    q, ctx = EventQueue(spare=0.5, rebuild=rebuild), RecR(**kw)
    for j in range(3):
        q.node_add(node("n%d" % j))
    for i in range(4):
        q.pod_add(pod("p%d" % i, "n%d" % (i % 3)))
    q.flush(ctx)
    ctx.calls.clear()
    ctx.events = 0
    return q, ctx


def _churn(q):
    q.node_delete("n0")
    q.node_add(node("new0"))
    q.node_add(node("new1"))
    q.node_update(node("n1", labels={"pool": "b"}))
    q.node_update(node("n2", unschedulable=True))
    q.pod_add(pod("late", "new1"))


def test_add_limit_rebuilds_and_retries():
    q, ctx = _loaded(True, fail={2})                           # event 1: nodes_delete, 2: nodes_add
    _churn(q)
    q.flush(ctx)
    assert ctx.names() == ["nodes_delete", "nodes_add!", "nodes_room", "nodes_rebuild", "nodes_add", "nodes_relabel",
                           "nodes_update", "nodes_facts", "pods_upsert", "pods_bind"]
    assert q.reloads == 1 and q.reload_causes == ["first"]
    assert q.rebuilds == 1 and q.rebuild_causes == ["nodes_add"]
    assert q.applied["nodes_add"] == 2 and q.node_index("new1") == 4


def test_relabel_limit_rebuilds_without_asking_for_room():
    q, ctx = _loaded(True, fail={3})
    _churn(q)
    q.flush(ctx)
    assert ctx.names()[:6] == ["nodes_delete", "nodes_add", "nodes_relabel!", "nodes_rebuild", "nodes_relabel",
                               "nodes_update"]
    assert q.reloads == 1 and q.rebuild_causes == ["nodes_relabel"]


def test_second_limit_after_the_rebuild_reloads():
    q, ctx = _loaded(True, fail={2, 3})
    _churn(q)
    q.flush(ctx)
    assert ctx.names() == ["nodes_delete", "nodes_add!", "nodes_room", "nodes_rebuild", "nodes_add!", "load",
                           "load_placement"]
    assert q.reloads == 2 and q.reload_causes == ["first", "nodes_add"]
    assert q.rebuilds == 1 and q.rebuild_causes == ["nodes_add"]


def test_too_few_slots_means_no_rebuild():
    q, ctx = _loaded(True, fail={2}, room=1)                   # two adds, one free slot
    _churn(q)
    q.flush(ctx)
    assert ctx.names() == ["nodes_delete", "nodes_add!", "nodes_room", "load", "load_placement"]
    assert q.reloads == 2 and q.reload_causes == ["first", "nodes_add"] and q.rebuilds == 0


def test_pod_side_limit_reloads_as_before():
    q, ctx = _loaded(True, fail={6})                           # pods_upsert
    _churn(q)
    q.flush(ctx)
    assert ctx.names()[-3:] == ["pods_upsert!", "load", "load_placement"]
    assert q.reload_causes == ["first", "pods_upsert"] and q.rebuilds == 0


def test_rebuild_off_is_todays_sequence():
    """rebuild=False (and the default): the calls are the ones a plain Rec sees — neither new
    call is ever made."""
    for make in (lambda: EventQueue(spare=0.5), lambda: EventQueue(spare=0.5, rebuild=False)):
        seen = []
        for ctx in (Rec(), RecR()):
            q = make()
            for j in range(3):
                q.node_add(node("n%d" % j))
            for i in range(4):
                q.pod_add(pod("p%d" % i, "n%d" % (i % 3)))
            q.flush(ctx)
            first = len(ctx.calls)
            ctx.events, ctx.fail_at = 0, 2
            if isinstance(ctx, RecR):
                ctx.fail = {2}
            _churn(q)
            q.flush(ctx)
            seen.append(repr(ctx.calls[first:]))
            assert q.reload_causes == ["first", "nodes_add"] and q.rebuilds == 0 and q.rebuild_causes == []
        assert seen[0] == seen[1]
        assert "nodes_room" not in seen[1] and "nodes_rebuild" not in seen[1]


# ------------------------------------------------------------------ ResidentController
class _CtxR(_Ctx):
    def nodes_rebuild(self):
        self.calls.append("nodes_rebuild")

    def audit(self, checks=None):
        self.calls.append("audit" if checks is None else "audit:" + ",".join(checks))
        rep = dict(self.reports.pop(0) if self.reports else CLEAN)
        rep.setdefault("skipped", [])
        return rep


def _ctl(reports, node_rebuild=True):
    c = ResidentController.__new__(ResidentController)
    c.groups, c.state, c.lock_time, c.scale_delta, c.last_scale_out = [], [], [], [], []
    c.taint_tracker, c.clock, c.actuator, c._sel = {}, (lambda: 0), object(), None
    c.node_rebuild = node_rebuild
    c.events, c.ctx = EventQueue(spare=0.5, rebuild=node_rebuild), _CtxR(reports)
    c.audit_every, c.scans, c.audits, c.audit_failures, c.last_audit = 1, 0, 0, 0, None
    return c


def _bad(name):
    return dict(CLEAN, **{name: {"n_checked": 5, "n_bad": 1, "first_bad": 3}})


def test_audit_entry_rebuilds():
    c = _ctl([CLEAN, _bad("ENTRY"), CLEAN])
    c.run_once()
    before = len(c.ctx.calls)
    c.run_once()
    assert c.ctx.calls[before:] == ["audit", "nodes_rebuild", "audit:ENTRY,FIRST,REGION,OCC,TRACKER", "decide"]
    assert c.events.rebuild_causes == ["audit:ENTRY"] and c.events.reload_causes == ["first"]
    assert (c.events.reloads, c.events.rebuilds, c.audit_failures) == (1, 1, 1)


def test_audit_mirror_reloads():
    for bad in (_bad("MIRROR"), _bad("TOUCH"), dict(_bad("ENTRY"), **{"MIRROR": _bad("MIRROR")["MIRROR"]})):
        c = _ctl([bad])
        c.run_once()
        assert "nodes_rebuild" not in c.ctx.calls
        assert c.events.reloads == 2 and c.events.rebuilds == 0
        assert c.events.reload_causes[1] in ("audit:MIRROR", "audit:TOUCH", "audit:ENTRY")


def test_audit_mismatch_that_survives_the_rebuild_reloads():
    c = _ctl([_bad("OCC"), _bad("OCC")])
    c.run_once()
    assert c.ctx.calls[-6:] == ["audit", "nodes_rebuild", "audit:ENTRY,FIRST,REGION,OCC,TRACKER", "load", "load_placement",
                               "decide"]
    assert c.events.rebuild_causes == ["audit:OCC"] and c.events.reload_causes == ["first", "audit:OCC"]


def test_node_rebuild_off_reloads_on_entry():
    c = _ctl([_bad("ENTRY")], node_rebuild=False)
    c.run_once()
    assert "nodes_rebuild" not in c.ctx.calls and c.events.reload_causes == ["first", "audit:ENTRY"]
