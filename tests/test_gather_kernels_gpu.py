"""The steady-state gather's pack and compaction kernels (scanner_amd/csrc/scn_gather_kernels.h) at world sizes 1, 2, 3 and 8 on
one GPU.  tests/cpp/test_gather_kernels_gpu.cpp -- HIP with its own main, no libscanner_hip.so, no RCCL -- fills the root's ring
with what `world` ranks would have sent, through the production launchers and address functions, and holds the list, the headers,
the ring and every message byte for byte to a host model whose definition of the list is scn_stream_outcome, the function
scn_gather_wait reports to the caller.  Compiled once per module with the library's own flags, run once as a child process; one
result line per case, so that a failure names its case.

Mutation check (each a one-line edit of a COPY of scn_gather_kernels.h kept outside the tree, the program compiled against it and
run on an MI355X; none is committed).  mutant -> cases that fail, of the 316:
  * the offset loop starts at q = 1                  -> 209 cases: every one with records on rank 0 and a second rank, e.g.
                                                        cap_1_w2_allcap_root1, pattern_w8_mix_rootmiddle, ring_w3_cap300_round0_post0
  * `h.sent <= cap` dropped from the predicate       -> bad_sentcapplus1_w3_middle.  The only case this mutant was run on: there the
                                                        one record too many that it reads is the next rank's header and what it writes
                                                        stays inside the list; at the last rank it would read past the ring.
  * `h.seq == seq` dropped                           -> 51 cases: every bad_seq{minus1,plus1,minustickets,highword}_*, bad_several_w8_*
                                                        and ring_*_round1_post1 / _post3 (the message that did not arrive)
  * 3u -> 2u in the compaction's word count          -> 297 cases: every one whose list is not empty, e.g. cap_1_w1_allcap_root0
  * pack stride gridDim.x * 256u -> 256u * 64u       -> packgrid_1_sent86, packgrid_1_sent5462, packgrid_3_sent5462.
    Through scn_launch_gather_pack this mutant is EQUIVALENT: below the cap of 64 the launcher asks for ceil(words / 256) workgroups,
    so every thread's loop body runs at most once and the stride is never used; at the cap the two strides are the same number.  No
    sent_* case can tell them apart (sent_5462_* and sent_11000_* re-enter the loop, with the same stride either way).  The packgrid_*
    cases launch the kernel directly with grids of 1, 3, 64 and 65 workgroups: the kernel's own contract is that it strides by
    whatever grid it is given.
"""
import os
import re
import subprocess
import time

import pytest

from scanner_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# the families of the cases, each with the fewest names it must contribute
FAMILIES = {"cap_": 64, "sent_": 28, "packgrid_": 8, "pattern_": 48, "truncated_w": 18, "failed_": 9, "marked_with_records_": 9,
            "truncated_upstream_": 9, "bad_": 70, "ring_": 48}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """The program, compiled once and run once: {case name: (ok, rest of its line)}, plus the timings."""
    exe = tmp_path_factory.mktemp("gather_kernels") / "test_gather_kernels_gpu"
    cmd = [build.hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "-fno-slp-vectorize", *build.EXTRA_FLAGS, "-Wall",
           "-I", build.CSRC, os.path.join(ROOT, "tests", "cpp", "test_gather_kernels_gpu.cpp"), "-o", str(exe)]
    t0 = time.time()
    c = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    t_compile = time.time() - t0
    assert c.returncode == 0, c.stderr[-4000:]
    t0 = time.time()
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    t_run = time.time() - t0
    cases = {}
    for ln in out.stdout.splitlines():
        m = re.match(r"case (\S+) (ok|FAIL)\b ?(.*)", ln)
        if m:
            assert m.group(1) not in cases, f"case name used twice: {m.group(1)}"
            cases[m.group(1)] = (m.group(2) == "ok", m.group(3))
    print(f"gather kernels: {len(cases)} cases, compile {t_compile:.1f} s, run {t_run:.2f} s")
    return {"cases": cases, "returncode": out.returncode, "stdout": out.stdout, "stderr": out.stderr, "compile_s": t_compile, "run_s": t_run}


def test_no_hip_error_and_every_case_reported(run):
    tail = run["stdout"][-1500:] + run["stderr"][-1500:]
    assert "hip-error" not in run["stdout"] and "program-bug" not in run["stdout"], tail
    assert run["returncode"] in (0, 1), tail                       # 1: a mismatch, named by test_every_case_matches_the_host_model
    m = re.search(r"summary cases=(\d+) failed=(\d+)", run["stdout"])
    assert m, tail
    assert int(m.group(1)) == len(run["cases"]) and int(m.group(2)) == sum(not ok for ok, _ in run["cases"].values())
    for prefix, at_least in FAMILIES.items():
        n = sum(name.startswith(prefix) for name in run["cases"])
        assert n >= at_least, f"{n} cases named {prefix}*, expected at least {at_least}"


def test_every_case_matches_the_host_model(run):
    failed = {name: rest for name, (ok, rest) in run["cases"].items() if not ok}
    assert not failed, "\n".join(f"{name}: {rest}" for name, rest in sorted(failed.items()))
    assert run["returncode"] == 0


def test_the_cases_reach_every_edge_the_grids_have(run):
    """World sizes, root positions, both sides of every grid threshold, and every defect at every position: by name."""
    names = set(run["cases"])
    for cap in (1, 85, 86, 682, 683, 10922, 10923, 11000):
        for world in (1, 2, 3, 8):
            assert any(n.startswith(f"cap_{cap}_w{world}_") for n in names), (cap, world)
    for sent in (0, 1, 85, 86, 5461, 5462, 11000):
        assert {f"sent_{sent}_w1", f"sent_{sent}_w2_root0", f"sent_{sent}_w2_root1", f"sent_{sent}_w3_last_root1"} <= names, sent
    for world in (3, 8):
        for pat in ("allcap", "allzero", "firstonly", "lastonly", "zerosbetween", "mix"):
            for where in ("first", "middle", "last"):
                assert f"pattern_w{world}_{pat}_root{where}" in names
        for defect in ("magic", "seqminus1", "seqplus1", "seqminustickets", "seqhighword", "sentcapplus1", "sentabovecount", "sentmax"):
            for where in ("first", "middle", "last"):
                assert f"bad_{defect}_w{world}_{where}" in names
        for where in ("first", "middle", "last"):
            assert {f"failed_w{world}_{where}", f"truncated_w{world}_{where}_count301"} <= names
        for rnd in (0, 1):
            for k in range(4):
                assert f"ring_w{world}_cap300_round{rnd}_post{k}" in names
    # the roots the cases used: first, middle and last rank of a world of 8
    roots = {re.search(r"root=(\d+)", rest).group(1) for n, (ok, rest) in run["cases"].items() if ok and "world=8 " in rest}
    assert roots >= {"0", "4", "7"}, roots
