"""CPU: the plan of esc_pods_compact (plan_pod_compact in escalator_amd/csrc/esc_pod_layout.h) against
a naive recomputation, in a stand-alone program (tests/pod_compact_check.cpp) built with the host
compiler under AddressSanitizer and UBSan.  esc_pods_compact takes every table it uploads from
the plan — the re-cut class table, k_pc_move's per-class starts and live counts, the free tiles it
copies into the positions past them — so this is where the tile counts (shrink, growth by
re-homed pods, no tile at spare 0), the kept indices, the created classes, the free ranges and
the 32-bit limit are checked field by field.  The program also pins the class rule the device now
shares with the host (pod_class_id / pod_inert) over the edges of tests/inert_class_check.cpp."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_agrees_with_a_naive_recomputation(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pod_compact_check")
    # the sanitizer runtimes are linked into the executable (clang's default; g++ is told to),
    # so it runs in the environment as it is and nothing has to come first among the libraries
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = ["-static-libasan", "-static-libubsan"] if "Free Software Foundation" in version else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static + [
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "escalator_amd", "csrc"),
                    os.path.join(ROOT, "tests", "pod_compact_check.cpp"), "-o", exe], check=True, cwd=ROOT)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "checks held, 0 failed" in r.stdout
