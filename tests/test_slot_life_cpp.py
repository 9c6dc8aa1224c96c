"""A slot's life cycle as a stand-alone C++ program (tests/cpp/test_slot_life.cpp): scn_host.hip and the program compiled by plain g++
as C++17 -- no HIP header on the include path, nothing of HIP linked, nothing loaded into Python -- and run plain and under
ASan + UBSan, which must report nothing."""
import os
import re
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
    assert out.returncode == 0 and "slot life tests ok (1049 states, 38071 cells)" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr[-3000:]
    # the table the program holds the header to is the one tests/test_slot_life_gpu.py holds the library to
    printed = subprocess.run([exe, "--print"], capture_output=True, text=True, timeout=300, env=env)
    with open(os.path.join(ROOT, "tests", "golden", "slot_life_table.txt")) as fh:
        assert printed.returncode == 0 and printed.stdout == fh.read()


def test_the_table_names_every_entry_point_that_takes_a_plan():
    """The header against the table: every SCN_API function of include/scanner_hip.h with a parameter of type `scn_plan *` or `const
    scn_plan *` (`scn_plan **`, scn_plan_create's output, does not count) has a row, and no row names anything else.  The names are the
    golden table's, which test_slot_life_stand_alone holds to the program and the program to slot_life_table(), row for row."""
    with open(os.path.join(ROOT, "include", "scanner_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
    declared = re.findall(r"\bSCN_API\b[^;(]*?\b(\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert len(declared) > 60 and {"scn_plan_create", "scn_trace_merge"} <= {name for name, _ in declared}
    takes_a_plan = {name for name, params in declared if any(re.fullmatch(r"(const\s+)?scn_plan\s*\*\s*\w*", p.strip()) for p in params.split(","))}
    assert "scn_plan_create" not in takes_a_plan and "scn_plan_average_parts" in takes_a_plan
    with open(os.path.join(ROOT, "tests", "golden", "slot_life_table.txt")) as fh:
        rows = {line.split()[0] for line in fh if line.strip()}
    assert rows - {"scn_collect/refused"} == takes_a_plan, (sorted(takes_a_plan - rows), sorted(rows - takes_a_plan))
