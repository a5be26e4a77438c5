"""CPU: the inert classes of the pod layout (escalator_amd/csrc/esc_pod_layout.h) in a
stand-alone program (tests/inert_class_check.cpp) built with the host compiler under
AddressSanitizer and UBSan: ``pod_inert`` and ``pod_class_id`` at every edge of the definition,
the class cut (inert classes last, with real tiles and no K1 weight, every other class's range as
in a cut of the same pods without the inert ones) and ``plan_pod_grow`` growing and creating an
inert class by the load's rule."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_inert_classes_on_the_host(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "inert_class_check")
    # the sanitizer runtimes are linked into the executable (clang's default; g++ is told to)
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = ["-static-libasan", "-static-libubsan"] if "Free Software Foundation" in version else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static + [
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "escalator_amd", "csrc"),
                    os.path.join(ROOT, "tests", "inert_class_check.cpp"), "-o", exe], check=True, cwd=ROOT)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "checks held, 0 failed" in r.stdout
