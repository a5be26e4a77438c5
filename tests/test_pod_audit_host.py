"""CPU: esc_audit_pods' ABI surface, the class re-derivation its KSLOT check runs on the device
(tests/pod_audit_check.cpp, built with the host compiler under AddressSanitizer and UBSan) and
ResidentController's pod audit schedule with a stand-in context.

Both libraries export esc_audit_pods and the binding knows it; a context without a device
answers ESC_E_NODEV; the injection entry point esc_debug_poke_pods exists in the measurement
library only.  The controller runs the pod audit on every pod_audit_every-th scan, after the
flush and after audit_every's pass; a mismatch reloads exactly once with the cause
"pod_audit:<check>"; 0 (the default) never calls it."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

from escalator_amd import _lib as L
from escalator_amd.context import Context
from escalator_amd.controller import ResidentController

import test_audit_host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURE = os.path.join(ROOT, "escalator_amd", "libescalator_hip_measure.so")


def test_class_rederivation_round_trip(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pod_audit_check")
    # the sanitizer runtimes are linked into the executable (clang's default; g++ is told to)
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = ["-static-libasan", "-static-libubsan"] if "Free Software Foundation" in version else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static + [
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "escalator_amd", "csrc"),
                    os.path.join(ROOT, "tests", "pod_audit_check.cpp"), "-o", exe], check=True, cwd=ROOT)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "checks held, 0 failed" in r.stdout
    assert "over 76 classes" in r.stdout


def test_both_libraries_export_esc_audit_pods():
    lib = L.load()
    assert hasattr(lib, "esc_audit_pods")
    assert "esc_audit_pods" in L._SIGS and "esc_audit_pods" in L.header_functions()
    assert C.sizeof(L.PodAuditReport) == 8 + 24 * 6
    assert L.POD_AUDIT_CHECKS == ["MAP", "KSLOT", "CSLOT", "COUNT", "PODREF", "REPLICA"]
    assert lib.esc_abi_version() == 6                       # additive: the version stays
    assert os.path.exists(MEASURE), "build the measurement library: make -C escalator_amd/csrc ABLATIONS=1"
    with open(MEASURE, "rb") as f:                           # (not loaded: one library per process)
        assert b"esc_audit_pods" in f.read()


def test_without_a_device_is_nodev_and_bad_arguments_inval():
    ctx = Context([{"name": "a", "label_key": "k", "label_value": "v"}], device=-1)
    rep = L.PodAuditReport()
    assert ctx.lib.esc_audit_pods(ctx.handle, 0, C.byref(rep)) == L.ESC_E_NODEV
    assert ctx.lib.esc_audit_pods(ctx.handle, 0, None) == L.ESC_E_INVAL
    assert ctx.lib.esc_audit_pods(None, 0, C.byref(rep)) == L.ESC_E_INVAL
    assert ctx.lib.esc_audit_pods(ctx.handle, 1 << len(L.POD_AUDIT_CHECKS), C.byref(rep)) == L.ESC_E_INVAL
    assert ctx.lib.esc_audit_pods(ctx.handle, (1 << len(L.POD_AUDIT_CHECKS)) - 1, C.byref(rep)) == L.ESC_E_NODEV
    try:
        ctx.audit_pods()
    except L.EscError as e:
        assert e.code == L.ESC_E_NODEV
    else:
        raise AssertionError("Context.audit_pods on device=-1 did not raise")


def test_product_library_has_no_pod_poke():
    lib = L.load()
    assert os.path.basename(L.LIB_PATH) == "libescalator_hip.so"
    assert not hasattr(lib, "esc_debug_poke_pods")
    with open(L.LIB_PATH, "rb") as f:
        assert b"esc_debug_poke_pods" not in f.read()
    with open(MEASURE, "rb") as f:
        assert b"esc_debug_poke_pods" in f.read()


PCLEAN = {n: {"n_checked": 5, "n_bad": 0, "first_bad": -1} for n in L.POD_AUDIT_CHECKS}


class _Ctx(H._Ctx):
    """test_audit_host's stand-in context with a pod audit beside the node one."""

    def __init__(self, pod_reports=(), reports=()):
        super().__init__(reports)
        self.pod_reports = list(pod_reports)

    def audit_pods(self, checks=None):
        self.calls.append("audit_pods")
        rep = dict(self.pod_reports.pop(0) if self.pod_reports else PCLEAN)
        rep.setdefault("skipped", [])
        return rep


def _ctl(pod_audit_every, pod_reports=(), audit_every=0):
    c = H._ctl(audit_every)
    c.ctx = _Ctx(pod_reports)
    c.pod_audit_every, c.pod_audits, c.pod_audit_failures, c.last_pod_audit = pod_audit_every, 0, 0, None
    return c


def test_every_kth_scan_after_the_flush_and_the_node_audit():
    c = _ctl(3, audit_every=2)
    seen = {}
    for scan in range(1, 8):
        before = len(c.ctx.calls)
        assert c.run_once() == []
        calls = c.ctx.calls[before:]
        seen[scan] = [x for x in calls if x in ("audit", "audit_pods")]
        if "audit_pods" in calls:
            assert calls.index("audit_pods") < calls.index("decide")
            assert "load" not in calls[calls.index("audit_pods"):]     # clean: no reload
    assert seen == {1: [], 2: ["audit"], 3: ["audit_pods"], 4: ["audit"], 5: [], 6: ["audit", "audit_pods"], 7: []}
    assert (c.pod_audits, c.pod_audit_failures, c.audits, c.scans) == (2, 0, 3, 7)
    assert c.events.reload_causes == ["first"] and c.events.reloads == 1
    assert c.last_pod_audit["KSLOT"]["n_bad"] == 0


def test_a_pod_mismatch_reloads_once_with_its_cause():
    bad = dict(PCLEAN, KSLOT={"n_checked": 5, "n_bad": 1, "first_bad": 17}, PODREF={"n_checked": 5, "n_bad": 3, "first_bad": 2})
    c = _ctl(1, [PCLEAN, bad, PCLEAN])
    for _ in range(4):
        c.run_once()
    assert c.events.reload_causes == ["first", "pod_audit:KSLOT"]      # the first failing check, in check order
    assert c.events.reloads == 2
    assert (c.pod_audits, c.pod_audit_failures) == (4, 1)
    k = [i for i, x in enumerate(c.ctx.calls) if x == "audit_pods"][1]
    assert c.ctx.calls[k + 1:k + 4] == ["load", "load_placement", "decide"]
    assert "audit" not in c.ctx.calls and c.audits == 0                # audit_every stayed 0


def test_zero_never_calls_it_and_is_the_default():
    c = _ctl(0)
    for _ in range(5):
        c.run_once()
    assert "audit_pods" not in c.ctx.calls and c.pod_audits == 0
    assert c.events.reload_causes == ["first"]
    p = inspect.signature(ResidentController.__init__).parameters["pod_audit_every"]
    assert p.default == 0 and p.kind is inspect.Parameter.KEYWORD_ONLY
