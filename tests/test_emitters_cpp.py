"""The trace emitters' host arithmetic as a stand-alone C++ program (tests/cpp/test_emitters.cpp): scn_host.hip and the program
compiled by plain g++ as C++17 -- no HIP header on the include path, nothing of HIP linked, nothing loaded into Python -- and run
plain and under ASan + UBSan, which must report nothing."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("san", ["address,undefined", ""])
def test_emitters_stand_alone(tmp_path, san):
    csrc = os.path.join(ROOT, "scanner_amd", "csrc")
    exe = tmp_path / "test_emitters"
    cmd = ["g++", "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"] + ([f"-fsanitize={san}"] if san else []) + [
        "-Wall", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "test_emitters.cpp"), os.path.join(csrc, "scn_host.hip"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "emitters tests ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr[-3000:]
