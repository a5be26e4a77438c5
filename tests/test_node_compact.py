"""CPU: the node-table compaction plan (plan_node_compact, plan_runs in
escalator_amd/csrc/esc_node_layout.h) against a naive recomputation, in a stand-alone program
(tests/node_compact_check.cpp) built with the host compiler under AddressSanitizer and UBSan.
esc_nodes_compact takes every table it uploads from the plan and esc_load_placement cuts its
runs with the same function, so this is where the renumbering, the capacities, the run moves,
the unbound pods and the limits are checked field by field; the GPU suite
(tests/test_gpu_compact.py) compares a compacted context with a fresh load from outside."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_agrees_with_a_naive_recomputation(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "node_compact_check")
    # the sanitizer runtimes are linked into the executable (clang's default; g++ is told to),
    # so it runs in the environment as it is and nothing has to come first among the libraries
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = ["-static-libasan", "-static-libubsan"] if "Free Software Foundation" in version else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static + [
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "escalator_amd", "csrc"),
                    os.path.join(ROOT, "tests", "node_compact_check.cpp"), "-o", exe], check=True, cwd=ROOT)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "checks held, 0 failed" in r.stdout
