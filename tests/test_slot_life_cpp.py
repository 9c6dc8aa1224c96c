"""A slot's life cycle as a stand-alone C++ program (tests/cpp/test_slot_life.cpp): scn_host.hip and the program compiled by plain g++
as C++17 -- no HIP header on the include path, nothing of HIP linked, nothing loaded into Python -- and run plain and under
ASan + UBSan, which must report nothing."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_program(out_dir, san=""):
    """compiles the program into out_dir; returns its path"""
    csrc = os.path.join(ROOT, "scanner_amd", "csrc")
    exe = os.path.join(str(out_dir), "test_slot_life")
    cmd = ["g++", "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"] + ([f"-fsanitize={san}"] if san else []) + [
        "-Wall", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "test_slot_life.cpp"), os.path.join(csrc, "scn_host.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("san", ["address,undefined", ""])
def test_slot_life_stand_alone(tmp_path, san):
    exe = build_program(tmp_path, san)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "slot life tests ok (1049 states, 28846 cells)" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr[-3000:]
    # the table the program holds the header to is the one tests/test_slot_life_gpu.py holds the library to
    printed = subprocess.run([exe, "--print"], capture_output=True, text=True, timeout=300, env=env)
    with open(os.path.join(ROOT, "tests", "golden", "slot_life_table.txt")) as fh:
        assert printed.returncode == 0 and printed.stdout == fh.read()
