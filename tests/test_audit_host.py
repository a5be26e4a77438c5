"""CPU: esc_audit's ABI surface and ResidentController's audit schedule with a stand-in context.

The library exports esc_audit and the binding knows it; a context without a device answers
ESC_E_NODEV; the corruption entry point esc_debug_poke exists in the measurement library only.
The controller audits on every audit_every-th scan, after the flush; a report with a mismatch
makes the queue reload exactly once with the cause "audit:<check>"; audit_every=0 never audits."""
import ctypes as C
import os

import numpy as np

from escalator_amd import _lib as L
from escalator_amd.context import Context
from escalator_amd.controller import ResidentController
from escalator_amd.events import EventQueue

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_esc_audit():
    lib = L.load()
    assert hasattr(lib, "esc_audit")
    assert "esc_audit" in L._SIGS and "esc_audit" in L.header_functions()
    assert C.sizeof(L.AuditReport) == 8 + 24 * len(L.AUDIT_CHECKS)
    assert L.AUDIT_CHECKS == ["ENTRY", "FIRST", "REGION", "OCC", "TOUCH", "TRACKER", "MIRROR"]
    assert lib.esc_abi_version() == 6                       # additive: the version stays


def test_audit_without_a_device_is_nodev():
    ctx = Context([{"name": "a", "label_key": "k", "label_value": "v"}], device=-1)
    rep = L.AuditReport()
    assert ctx.lib.esc_audit(ctx.handle, 0, C.byref(rep)) == L.ESC_E_NODEV
    assert ctx.lib.esc_audit(ctx.handle, 0, None) == L.ESC_E_INVAL
    assert ctx.lib.esc_audit(ctx.handle, 1 << len(L.AUDIT_CHECKS), C.byref(rep)) == L.ESC_E_INVAL
    try:
        ctx.audit()
    except L.EscError as e:
        assert e.code == L.ESC_E_NODEV
    else:
        raise AssertionError("Context.audit on device=-1 did not raise")


def test_product_library_has_no_poke():
    lib = L.load()
    assert os.path.basename(L.LIB_PATH) == "libescalator_hip.so"
    assert not hasattr(lib, "esc_debug_poke")
    measure = os.path.join(ROOT, "escalator_amd", "libescalator_hip_measure.so")
    assert os.path.exists(measure), "build the measurement library: make -C escalator_amd/csrc ABLATIONS=1"
    with open(measure, "rb") as f:                           # (not loaded: one library per process)
        assert b"esc_debug_poke" in f.read()


CLEAN = {n: {"n_checked": 5, "n_bad": 0, "first_bad": -1} for n in L.AUDIT_CHECKS}


class _Ctx:
    """What ResidentController.run_once and EventQueue's load path call, for zero groups."""

    def __init__(self, reports):
        self.reports, self.calls = list(reports), []

    def audit(self, checks=None):
        self.calls.append("audit")
        rep = dict(self.reports.pop(0) if self.reports else CLEAN)
        rep.setdefault("skipped", [])
        return rep

    def set_spare(self, f):
        self.calls.append("set_spare")

    def pack(self, pods, nodes, trackers=None):
        return {}, {}

    def load(self, P, N):
        self.calls.append("load")

    def load_placement(self, *a):
        self.calls.append("load_placement")

    def decide_all(self, states):
        self.calls.append("decide")
        return np.zeros(0), np.zeros(0)

    def selections(self):
        return None

    def try_remove(self, now, soft, hard):
        return []


def _ctl(audit_every, reports=()):
    c = ResidentController.__new__(ResidentController)
    c.groups, c.state, c.lock_time, c.scale_delta, c.last_scale_out = [], [], [], [], []
    c.taint_tracker, c.clock, c.actuator, c._sel = {}, (lambda: 0), object(), None
    c.events, c.ctx = EventQueue(spare=0.5), _Ctx(reports)
    c.audit_every, c.scans, c.audits, c.audit_failures, c.last_audit = audit_every, 0, 0, 0, None
    return c


def test_audit_every_third_scan_after_the_flush():
    c = _ctl(3)
    audited = []
    for scan in range(1, 8):
        before = len(c.ctx.calls)
        assert c.run_once() == []
        calls = c.ctx.calls[before:]
        if "audit" in calls:
            audited.append(scan)
            assert calls.index("audit") < calls.index("decide")          # before the decision
            assert "load" not in calls[calls.index("audit"):]            # clean: no reload
    assert audited == [3, 6]
    assert (c.audits, c.audit_failures, c.scans) == (2, 0, 7)
    assert c.events.reload_causes == ["first"] and c.events.reloads == 1


def test_a_mismatch_reloads_once_with_its_cause():
    bad = dict(CLEAN, OCC={"n_checked": 5, "n_bad": 2, "first_bad": 17})
    c = _ctl(1, [CLEAN, bad, CLEAN])
    for _ in range(4):
        c.run_once()
    assert c.events.reload_causes == ["first", "audit:OCC"]
    assert c.events.reloads == 2
    assert (c.audits, c.audit_failures) == (4, 1)
    # the reload happened inside the failing scan, between its audit and its decision
    k = [i for i, x in enumerate(c.ctx.calls) if x == "audit"][1]
    assert c.ctx.calls[k + 1:k + 4] == ["load", "load_placement", "decide"]
    assert c.last_audit["OCC"]["n_bad"] == 0


def test_two_failing_checks_name_the_first_in_check_order():
    bad = dict(CLEAN, TRACKER={"n_checked": 5, "n_bad": 1, "first_bad": 3}, ENTRY={"n_checked": 5, "n_bad": 1, "first_bad": 9})
    c = _ctl(1, [bad])
    c.run_once()
    assert c.events.reload_causes == ["first", "audit:ENTRY"] and c.audit_failures == 1


def test_audit_every_zero_never_audits():
    c = _ctl(0)
    for _ in range(5):
        c.run_once()
    assert "audit" not in c.ctx.calls and c.audits == 0
    assert c.events.reload_causes == ["first"]
    assert ResidentController.__init__.__defaults__[-1] == 0            # the default: off
