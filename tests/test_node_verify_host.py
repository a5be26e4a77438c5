"""CPU: esc_nodes_verify's compare (tests/node_verify_check.cpp, built with the host compiler under
AddressSanitizer and UBSan: nv_compare of esc_node_verify.h, the function the kernel runs, over a
table the program fills itself) and the ABI surface of esc_nodes_verify / esc_nodes_live_ids on a
context without a device."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np

from escalator_amd import _lib as L
from escalator_amd.context import Context, node_soa
from escalator_amd.controller import ResidentController
from escalator_amd.events import EventQueue

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURE = os.path.join(ROOT, "escalator_amd", "libescalator_hip_measure.so")


def test_the_compare_rule_over_a_table_of_its_own(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "node_verify_check")
    # the sanitizer runtimes are linked into the executable (clang's default; g++ is told to)
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = ["-static-libasan", "-static-libubsan"] if "Free Software Foundation" in version else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static + [
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "escalator_amd", "csrc"),
                    os.path.join(ROOT, "tests", "node_verify_check.cpp"), "-o", exe], check=True, cwd=ROOT)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "checks held, 0 failed" in r.stdout
    assert "label counts 0 1 2 255" in r.stdout
    held = int(r.stdout.split(" checks held")[0].split()[-1])
    assert held > 300                                        # four nodes, every field, both sides


def test_the_kernel_runs_the_header_the_check_builds():
    with open(os.path.join(ROOT, "escalator_amd", "csrc", "esc_node_verify.hip")) as f:
        hip = f.read()
    assert '#include "esc_node_verify.h"' in hip and "nv_compare(" in hip
    with open(os.path.join(ROOT, "tests", "node_verify_check.cpp")) as f:
        assert '#include "esc_node_verify.h"' in f.read()


def test_both_libraries_export_the_two_calls():
    lib = L.load()
    for name in ("esc_nodes_verify", "esc_nodes_live_ids"):
        assert hasattr(lib, name)
        assert name in L._SIGS and name in L.header_functions()
    assert C.sizeof(L.NodesVerifyReport) == 64
    assert (L.NV_ABSENT, L.NV_SHAPE, L.NV_STATUS, L.NV_FACTS, L.NV_INST) == (1, 2, 4, 8, 16)
    assert lib.esc_abi_version() == 6                       # additive: the version stays
    with open(os.path.join(ROOT, "include", "escalator_hip.h")) as f:
        text = f.read()
    for name, v in (("ESC_NV_ABSENT", 1), ("ESC_NV_SHAPE", 2), ("ESC_NV_STATUS", 4), ("ESC_NV_FACTS", 8), ("ESC_NV_INST", 16)):
        assert re.search(r"#define %s +%d " % (name, v), text)
    assert os.path.exists(MEASURE), "build the measurement library: make -C escalator_amd/csrc ABLATIONS=1"
    with open(MEASURE, "rb") as f:                           # (not loaded: one library per process)
        blob = f.read()
    assert b"esc_nodes_verify" in blob and b"esc_nodes_live_ids" in blob
    # one shard's context of a multi-device context is handed out by the measurement library only
    assert not hasattr(lib, "esc_debug_multi_sub") and b"esc_debug_multi_sub" in blob
    with open(L.LIB_PATH, "rb") as f:
        assert b"esc_debug_multi_sub" not in f.read()


def _one_node():
    nodes = {"flags": np.zeros(1, np.uint32), "label0": np.zeros(1, np.uint32), "cpu": np.array([4000], np.int64),
             "mem": np.array([8 << 30], np.int64), "created_ns": np.array([1000], np.int64),
             "xl_pair": np.zeros(0, np.uint32), "trk_node": np.zeros(0, np.int32), "trk_group": np.zeros(0, np.int32)}
    return np.zeros(1, np.int64), nodes


def test_without_a_device_is_nodev_and_bad_arguments_inval():
    ctx = Context([{"name": "a", "label_key": "k", "label_value": "v"}], device=-1)
    ids, nodes = _one_node()
    ns, keep = node_soa(nodes)
    idp = ids.ctypes.data_as(C.POINTER(C.c_int64))
    rep = L.NodesVerifyReport()
    rep.n_checked = 77
    stat = np.zeros(1, np.uint8)
    sp = stat.ctypes.data_as(C.POINTER(C.c_uint8))
    t = np.zeros(1, np.int64)
    tp = t.ctypes.data_as(C.POINTER(C.c_int64))
    lib = ctx.lib
    assert lib.esc_nodes_verify(ctx.handle, idp, C.byref(ns), None, None, None, sp, C.byref(rep)) == L.ESC_E_NODEV
    assert lib.esc_nodes_verify(ctx.handle, idp, C.byref(ns), tp, sp, tp, None, C.byref(rep)) == L.ESC_E_NODEV
    assert lib.esc_nodes_verify(ctx.handle, idp, C.byref(ns), None, None, None, sp, None) == L.ESC_E_INVAL     # a NULL report
    assert lib.esc_nodes_verify(None, idp, C.byref(ns), None, None, None, sp, C.byref(rep)) == L.ESC_E_INVAL
    assert lib.esc_nodes_verify(ctx.handle, idp, None, None, None, None, sp, C.byref(rep)) == L.ESC_E_INVAL
    assert lib.esc_nodes_verify(ctx.handle, None, C.byref(ns), None, None, None, sp, C.byref(rep)) == L.ESC_E_INVAL   # no ids
    for name in ("flags", "label0", "cpu", "mem", "created_ns"):                   # a NULL array with n_nodes > 0
        bad, keep2 = node_soa(nodes)
        setattr(bad, name, None)
        assert lib.esc_nodes_verify(ctx.handle, idp, C.byref(bad), None, None, None, sp, C.byref(rep)) == L.ESC_E_INVAL, name
        del keep2
    bad, keep2 = node_soa(nodes)
    bad.n_xl = 3                                                                    # label words claimed, no array
    bad.xl_pair = None
    assert lib.esc_nodes_verify(ctx.handle, idp, C.byref(bad), None, None, None, sp, C.byref(rep)) == L.ESC_E_INVAL
    assert rep.n_checked == 77                                                      # nothing reported
    n = C.c_int64(-1)
    assert lib.esc_nodes_live_ids(ctx.handle, None, 0, C.byref(n)) == L.ESC_E_STATE                # before a load
    assert lib.esc_nodes_live_ids(ctx.handle, None, 0, None) == L.ESC_E_INVAL
    assert lib.esc_nodes_live_ids(ctx.handle, None, 4, C.byref(n)) == L.ESC_E_INVAL                # room claimed, no array
    assert lib.esc_nodes_live_ids(None, None, 0, C.byref(n)) == L.ESC_E_INVAL
    for call, code in ((lambda: ctx.nodes_verify(ids, nodes), L.ESC_E_NODEV), (ctx.nodes_live_ids, L.ESC_E_STATE)):
        try:
            call()
        except L.EscError as e:
            assert e.code == code
        else:
            raise AssertionError("the call on device=-1 did not raise")
    del keep, keep2


def test_the_binding_takes_three_optional_fact_arrays():
    sig = inspect.signature(Context.nodes_verify)
    assert list(sig.parameters) == ["self", "ids", "nodes", "taint_s", "no_delete", "inst_ns"]
    assert all(sig.parameters[k].default is None for k in ("taint_s", "no_delete", "inst_ns"))
    ctx = Context([{"name": "a", "label_key": "k", "label_value": "v"}], device=-1)
    ids, nodes = _one_node()
    for kw in ({"taint_s": [1, 2]}, {"no_delete": []}, {"inst_ns": [1, 2, 3]}):
        try:
            ctx.nodes_verify(ids, nodes, **kw)
        except ValueError:
            pass
        else:
            raise AssertionError("a fact array of another length was accepted")


def test_node_resync_every_is_off_by_default_and_keyword_only():
    p = inspect.signature(ResidentController.__init__).parameters["node_resync_every"]
    assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert (ResidentController.node_resync_every, ResidentController.node_resyncs, ResidentController.last_node_resync) == (None, 0, None)
    q = EventQueue()
    assert q.node_resyncs == 0
    assert q.node_resync_repairs == {"absent": 0, "shape": 0, "status": 0, "facts": 0, "inst": 0, "orphans": 0}
