"""CPU: esc_pods_verify's compare (tests/pod_verify_check.cpp, built with the host compiler under
AddressSanitizer and UBSan: kb_pod_same / c_pod_same against kb_write_pod / c_write_pod for every
holdable class and several C rooms) and the ABI surface of esc_pods_verify / esc_pods_live_ids on
a context without a device."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np

from escalator_amd import _lib as L
from escalator_amd.context import Context, pod_soa
from escalator_amd.controller import ResidentController

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURE = os.path.join(ROOT, "escalator_amd", "libescalator_hip_measure.so")


def test_compare_against_the_writers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pod_verify_check")
    # the sanitizer runtimes are linked into the executable (clang's default; g++ is told to)
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = ["-static-libasan", "-static-libubsan"] if "Free Software Foundation" in version else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static + [
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "escalator_amd", "csrc"),
                    os.path.join(ROOT, "tests", "pod_verify_check.cpp"), "-o", exe], check=True, cwd=ROOT)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "checks held, 0 failed" in r.stdout
    assert "76 classes, 5 rooms" in r.stdout


def test_both_libraries_export_the_two_calls():
    lib = L.load()
    for name in ("esc_pods_verify", "esc_pods_live_ids"):
        assert hasattr(lib, name)
        assert name in L._SIGS and name in L.header_functions()
    assert C.sizeof(L.PodsVerifyReport) == 48
    assert (L.PV_ABSENT, L.PV_CLASS, L.PV_VALUE, L.PV_BIND) == (1, 2, 4, 8)
    assert lib.esc_abi_version() == 6                       # additive: the version stays
    with open(os.path.join(ROOT, "include", "escalator_hip.h")) as f:
        text = f.read()
    for name, v in (("ESC_PV_ABSENT", 1), ("ESC_PV_CLASS", 2), ("ESC_PV_VALUE", 4), ("ESC_PV_BIND", 8)):
        assert re.search(r"#define %s +%d " % (name, v), text)
    assert os.path.exists(MEASURE), "build the measurement library: make -C escalator_amd/csrc ABLATIONS=1"
    with open(MEASURE, "rb") as f:                           # (not loaded: one library per process)
        blob = f.read()
    assert b"esc_pods_verify" in blob and b"esc_pods_live_ids" in blob


def _one_pod():
    pods = {"flags": np.zeros(1, np.uint32), "cpu0": np.array([100], np.uint32), "mem0": np.array([1 << 20], np.int64),
            "pair0": np.array([0xFFFFFFFF], np.uint32),
            "xc_cpu": np.zeros(0, np.int64), "xc_mem": np.zeros(0, np.int64), "xp_pair": np.zeros(0, np.uint32)}
    return np.zeros(1, np.int64), pods


def test_without_a_device_is_nodev_and_bad_arguments_inval():
    ctx = Context([{"name": "a", "label_key": "k", "label_value": "v"}], device=-1)
    ids, pods = _one_pod()
    ps, keep = pod_soa(pods)
    idp = ids.ctypes.data_as(C.POINTER(C.c_int64))
    rep = L.PodsVerifyReport()
    stat = np.zeros(1, np.uint8)
    sp = stat.ctypes.data_as(C.POINTER(C.c_uint8))
    lib = ctx.lib
    assert lib.esc_pods_verify(ctx.handle, idp, C.byref(ps), None, sp, C.byref(rep)) == L.ESC_E_NODEV
    assert lib.esc_pods_verify(ctx.handle, idp, C.byref(ps), None, None, C.byref(rep)) == L.ESC_E_NODEV
    assert lib.esc_pods_verify(ctx.handle, idp, C.byref(ps), None, sp, None) == L.ESC_E_INVAL      # a NULL report
    assert lib.esc_pods_verify(None, idp, C.byref(ps), None, sp, C.byref(rep)) == L.ESC_E_INVAL
    assert lib.esc_pods_verify(ctx.handle, idp, None, None, sp, C.byref(rep)) == L.ESC_E_INVAL
    assert lib.esc_pods_verify(ctx.handle, None, C.byref(ps), None, sp, C.byref(rep)) == L.ESC_E_INVAL   # n_pods > 0, no ids
    n = C.c_int64(-1)
    assert lib.esc_pods_live_ids(ctx.handle, None, 0, C.byref(n)) == L.ESC_E_NODEV
    assert lib.esc_pods_live_ids(ctx.handle, None, 0, None) == L.ESC_E_INVAL
    assert lib.esc_pods_live_ids(ctx.handle, None, 4, C.byref(n)) == L.ESC_E_INVAL                 # room claimed, no array
    assert lib.esc_pods_live_ids(None, None, 0, C.byref(n)) == L.ESC_E_INVAL
    for call in (lambda: ctx.pods_verify(ids, pods), ctx.pods_live_ids):
        try:
            call()
        except L.EscError as e:
            assert e.code == L.ESC_E_NODEV
        else:
            raise AssertionError("the call on device=-1 did not raise")
    del keep


def test_the_binding_takes_an_optional_pod_node():
    sig = inspect.signature(Context.pods_verify)
    assert list(sig.parameters) == ["self", "ids", "pods", "pod_node"] and sig.parameters["pod_node"].default is None


def test_resync_every_is_off_by_default_and_keyword_only():
    p = inspect.signature(ResidentController.__init__).parameters["resync_every"]
    assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert ResidentController.resync_every is None
