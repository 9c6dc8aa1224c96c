"""The trace emitters' host form (scn_trace_emitters: scn_host.hip) against tests/emitters_ref.py, the numpy model written from the
definition: whole record arrays, byte for byte, on seeded traces and on a list of corners.  No device is needed.

The corners are named, because the model must tell five deliberate errors apart on them (test_the_cases_tell_each_mutant_apart): `>=`
for `>`, a gap rule off by one, empty cells on under a threshold of -inf, a peak tie to the highest cell, count summed over the
span's off cells too."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from scanner_amd import capi
from tests import emitters_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINES = (capi.TRACE_LINE_MAX, capi.TRACE_LINE_MIN, capi.TRACE_LINE_SPREAD)
INF = np.float32(np.inf)


def window(cells, **at):
    """an empty trace with cells put in: c=(max, min, count)"""
    mx, mn, ct = np.full(cells, -INF, np.float32), np.full(cells, INF, np.float32), np.zeros(cells, np.uint64)
    for c, (a, b, k) in at.items():
        mx[int(c[1:])], mn[int(c[1:])], ct[int(c[1:])] = a, b, k
    return mx, mn, ct


def corners():
    """name -> (trace, line, threshold_db, max_gap)"""
    flat = lambda n, v=1.0: (np.full(n, v, np.float32), np.full(n, v - 1, np.float32), np.full(n, 3, np.uint64))  # noqa: E731
    alt = flat(64)
    alt[0][1::2] = -5.0
    gaps = window(40, c3=(1, 0, 1), c5=(1, 0, 2), c8=(1, 0, 3), c12=(1, 0, 4), c30=(1, 0, 5))  # distances 2, 3, 4, 18
    ties = window(9, c2=(7, 1, 1), c3=(9, 1, 1), c4=(-5, -6, 99), c5=(9, 1, 1), c6=(7, 1, 1))
    quiet = flat(10)
    quiet[0][3:6] = 0.5  # off cells with large counts inside a span
    quiet[2][3:6] = 1000
    denorm = window(4, c0=(np.uint32(0x00C00000).view(np.float32), np.uint32(0x00800000).view(np.float32), 2), c1=(2, 2, 1), c2=(INF, INF, 2), c3=(3, 1, 2))
    zeros = window(6, c0=(-0.0, -0.0, 1), c1=(0.0, -0.0, 2), c2=(0.0, 0.0, 1), c4=(-INF, -INF, 5), c5=(INF, -INF, 1 << 40))
    big = flat(7)
    big[2][:] = np.uint64(1 << 40) + np.arange(7, dtype=np.uint64)
    return {
        "equal_to_threshold": (flat(5), capi.TRACE_LINE_MAX, 1.0, 0),
        "one_ulp_below": (flat(5), capi.TRACE_LINE_MAX, np.nextafter(np.float32(1.0), np.float32(0.0)), 0),
        "alternating_gap0": (alt, capi.TRACE_LINE_MAX, 0.0, 0),
        "alternating_gap1": (alt, capi.TRACE_LINE_MAX, 0.0, 1),
        "gaps_1": (gaps, capi.TRACE_LINE_MAX, 0.5, 1), "gaps_2": (gaps, capi.TRACE_LINE_MAX, 0.5, 2), "gaps_3": (gaps, capi.TRACE_LINE_MAX, 0.5, 3),
        "gaps_17": (gaps, capi.TRACE_LINE_MAX, 0.5, 17), "gaps_all": (gaps, capi.TRACE_LINE_MAX, 0.5, 0xFFFFFFFF),
        "empty_under_minus_inf": (gaps, capi.TRACE_LINE_MAX, -INF, 0),
        "empty_under_minus_inf_min": (gaps, capi.TRACE_LINE_MIN, -INF, 0),
        "plus_inf": (flat(5), capi.TRACE_LINE_MAX, INF, 0),
        "peak_tie": (ties, capi.TRACE_LINE_MAX, 0.0, 1),
        "peak_tie_spread": (ties, capi.TRACE_LINE_SPREAD, 5.5, 1),
        "count_inside_span": (quiet, capi.TRACE_LINE_MAX, 0.75, 3),
        "spread_denormal": (denorm, capi.TRACE_LINE_SPREAD, 0.0, 0),
        "zeros_max": (zeros, capi.TRACE_LINE_MAX, -1.0, 0), "zeros_min": (zeros, capi.TRACE_LINE_MIN, -1.0, 0),
        "zeros_at_zero": (zeros, capi.TRACE_LINE_MAX, -0.0, 0), "zeros_spread": (zeros, capi.TRACE_LINE_SPREAD, -INF, 0),
        "counts_beyond_32_bits": (big, capi.TRACE_LINE_MIN, -1.0, 0),
    }


def host(trace, line, thr, gap, f0=88000000, cell_hz=12500, first_cell=0):
    return capi.trace_emitters(trace, f0, cell_hz, line, thr, gap, first_cell)


def model(trace, line, thr, gap, f0=88000000, cell_hz=12500, first_cell=0, mutant=None):
    return ref.emitters(trace, f0, cell_hz, line, thr, gap, first_cell, mutant=mutant)


@pytest.mark.parametrize("name", sorted(corners()))
def test_corners_equal_the_model(built_lib, name):
    trace, line, thr, gap = corners()[name]
    got, want = host(trace, line, thr, gap), model(trace, line, thr, gap)
    assert ref.same(got, want), (name, ref.describe(got, want))
    got, want = host(trace, line, thr, gap, first_cell=1000003), model(trace, line, thr, gap, first_cell=1000003)
    assert ref.same(got, want), (name, "windowed", ref.describe(got, want))


def test_corner_answers_by_hand(built_lib):
    """a few of the corners' records written out, so that the model and the host form cannot be wrong together"""
    c = corners()
    assert host(*c["equal_to_threshold"]).size == 0 and host(*c["plus_inf"]).size == 0
    r = host(*c["one_ulp_below"])
    assert r.size == 1 and (r[0]["first_cell"], r[0]["last_cell"], r[0]["n_cells"], r[0]["count"], r[0]["peak_cell"]) == (0, 4, 5, 15, 0)
    assert (r[0]["start_hz"], r[0]["stop_hz"], r[0]["peak_hz"]) == (88000000, 88000000 + 5 * 12500, 88000000)
    assert host(*c["alternating_gap0"]).size == 32 and host(*c["alternating_gap1"]).size == 1
    assert [host(*c[k]).size for k in ("gaps_1", "gaps_2", "gaps_3", "gaps_17", "gaps_all")] == [4, 3, 2, 1, 1]
    r = host(*c["empty_under_minus_inf"])
    assert r["first_cell"].tolist() == [3, 5, 8, 12, 30] and r["count"].tolist() == [1, 2, 3, 4, 5]
    r = host(*c["peak_tie"])
    assert r.size == 1 and (r[0]["peak_cell"], r[0]["peak_db"], r[0]["peak_other_db"], r[0]["n_cells"], r[0]["count"]) == (3, 9.0, 1.0, 4, 4)
    r = host(*c["peak_tie_spread"])  # spreads 6 8 1 8 6
    assert r.size == 1 and (r[0]["peak_cell"], r[0]["peak_db"], r[0]["peak_other_db"], r[0]["n_cells"]) == (3, 8.0, 9.0, 4)
    r = host(*c["count_inside_span"])
    assert r.size == 1 and (r[0]["first_cell"], r[0]["last_cell"], r[0]["n_cells"], r[0]["count"]) == (0, 9, 7, 21)
    r = host(*c["spread_denormal"])  # 2^-127 is on above 0; 0.0 (one value) and inf - inf are not
    assert r["first_cell"].tolist() == [0, 3] and r["peak_db"].view(np.uint32).tolist() == [0x00400000, 0x40000000]
    r = host(*c["zeros_max"])  # -0.0 < +0.0 in key order: the peak is cell 1, the first +0.0
    assert r.size == 2 and r[0]["peak_cell"] == 1 and r["peak_db"].view(np.uint32).tolist() == [0x00000000, 0x7F800000] and r[0]["n_cells"] == 3
    r = host(*c["zeros_min"])
    assert r.size == 1 and r[0]["peak_cell"] == 2 and r[0]["last_cell"] == 2
    assert host(*c["zeros_at_zero"]).size == 1 and host(*c["zeros_at_zero"])[0]["first_cell"] == 5  # +-0.0 are not above -0.0
    r = host(*c["zeros_spread"])  # 0 0 0 . NaN +inf
    assert r["first_cell"].tolist() == [0, 5] and r[1]["count"] == 1 << 40
    r = host(*c["counts_beyond_32_bits"])
    assert r.size == 1 and r[0]["count"] == 7 * (1 << 40) + 21


@pytest.mark.parametrize("cells", [1, 2, 63, 64, 65, 1000, 40000])
def test_seeded_traces_equal_the_model(built_lib, cells):
    for seed in range(3):
        trace = ref.seeded_trace(cells, 100 * cells + seed, p_empty=(0.05, 0.3, 0.9)[seed])
        for line in LINES:
            v = ref.values(trace, line)
            finite = v[np.isfinite(v) & (trace[2] != 0)]
            cuts = [-INF, INF, 0.0] + ([float(np.median(finite)), float(finite.max()), float(np.nextafter(finite.max(), -INF))] if finite.size else [])
            for thr in cuts:
                for gap in (0, 1, 2, 7, cells, 0xFFFFFFFF):
                    got, want = host(trace, line, thr, gap, first_cell=seed * 77), model(trace, line, thr, gap, first_cell=seed * 77)
                    assert ref.same(got, want), (cells, seed, line, thr, gap, ref.describe(got, want))


def test_the_largest_window(built_lib):
    cells = capi.TRACE_CELLS_MAX
    trace = ref.seeded_trace(cells, 5)
    for line, thr, gap in ((capi.TRACE_LINE_MAX, -55.0, 0), (capi.TRACE_LINE_SPREAD, 6.0, 2)):
        got, want = host(trace, line, thr, gap, f0=(1 << 64) - 5, cell_hz=0xFFFFFFFF), model(trace, line, thr, gap, f0=(1 << 64) - 5, cell_hz=0xFFFFFFFF)
        assert want.size > cells // 16 and ref.same(got, want), ref.describe(got, want)


@pytest.mark.parametrize("mutant,names", [("ge", ["equal_to_threshold"]), ("gap", ["gaps_2", "alternating_gap1"]), ("empty_on", ["empty_under_minus_inf"]),
                                          ("peak_high", ["peak_tie", "peak_tie_spread"]), ("count_span", ["count_inside_span"])])
def test_the_cases_tell_each_mutant_apart(mutant, names):
    """the model with one deliberate error differs from the definition on the corner named for it -- so the equalities above are not vacuous"""
    assert mutant in ref.MUTANTS and len(ref.MUTANTS) == 5
    c = corners()
    for name in names:
        assert not ref.same(model(*c[name], mutant=mutant), model(*c[name])), (mutant, name)
    assert sum(not ref.same(model(*c[k], mutant=mutant), model(*c[k])) for k in c) >= len(names)


def test_refusals_and_paging(built_lib):
    L = capi.lib()
    trace = window(6, c0=(1, 1, 1), c2=(1, 1, 1), c3=(1, 1, 1), c5=(1, 1, 1))
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    total = C.c_uint64(99)

    def call(mx=trace[0], mn=trace[1], ct=trace[2], cell_hz=10, cells=6, first=0, line=0, thr=0.0, gap=0, out=None, cap=0):
        return L.scn_trace_emitters(vp(mx), vp(mn), vp(ct), 500, cell_hz, cells, first, line, thr, gap, vp(out), cap, C.byref(total))

    out = np.zeros(4, capi.EMITTER_DTYPE)
    want = model(trace, 0, 0.0, 0, f0=500, cell_hz=10)
    assert want.size == 3
    assert call(out=out, cap=4) == capi.OK and total.value == 3 and ref.same(out[:3], want)
    assert call(out=out, cap=3) == capi.OK
    out[:] = 0
    assert call(out=out, cap=2) == capi.E_TRUNCATED and total.value == 3 and ref.same(out[:2], want[:2]) and out[2]["n_cells"] == 0
    assert b"3 emitters" in L.scn_last_error()
    assert call() == capi.E_TRUNCATED and total.value == 3  # NULL out with cap 0: the total
    assert call(thr=2.0) == capi.OK and total.value == 0
    for bad in (dict(mx=None), dict(mn=None), dict(ct=None), dict(cap=1), dict(cell_hz=0), dict(cells=0), dict(cells=capi.TRACE_CELLS_MAX + 1),
                dict(first=capi.TRACE_CELLS_MAX - 5), dict(line=3), dict(line=0xFFFFFFFF), dict(thr=float("nan")), dict(thr=-float("nan"))):
        total.value = 99
        assert call(**bad) == capi.E_INVALID and total.value == 0, bad
    assert call(first=capi.TRACE_CELLS_MAX - 6) == capi.E_TRUNCATED
    assert L.scn_trace_emitters(vp(trace[0]), vp(trace[1]), vp(trace[2]), 500, 10, 6, 0, 0, 0.0, 0, None, 0, None) == capi.E_INVALID
    # the plan's two entry points refuse a null plan before they touch a device
    n = C.c_uint32()
    assert L.scn_plan_trace_emitters(None, 0, 0, 0, 0.0, 0, 0, None, 0, C.byref(n)) == capi.E_INVALID and b"null plan" in L.scn_last_error()
    assert L.scn_plan_merge_trace(None, 0, 0, None, None, None) == capi.E_INVALID


def test_record_layout_in_c_cxx_and_ctypes(tmp_path):
    fields = [("start_hz", 0), ("stop_hz", 8), ("peak_hz", 16), ("count", 24), ("first_cell", 32), ("last_cell", 36), ("peak_cell", 40), ("n_cells", 44),
              ("peak_db", 48), ("peak_other_db", 52)]
    assert C.sizeof(capi.Emitter) == 56 == capi.EMITTER_DTYPE.itemsize
    assert [(n, getattr(capi.Emitter, n).offset) for n, _ in capi.Emitter._fields_] == fields
    assert [(n, capi.EMITTER_DTYPE.fields[n][1]) for n in capi.EMITTER_DTYPE.names] == fields
    checks = " + ".join(f"(int)(offsetof(scn_emitter, {n}) != {o})" for n, o in fields)
    for comp, std, ext in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")):
        f = tmp_path / f"t.{ext}"
        f.write_text('#include <stddef.h>\n#include "scanner_hip.h"\nint main(void){ return (int)(sizeof(scn_emitter) != 56) + %s'
                     ' + (int)(SCN_TRACE_LINE_MAX != 0) + (int)(SCN_TRACE_LINE_MIN != 1) + (int)(SCN_TRACE_LINE_SPREAD != 2); }\n' % checks)
        exe = tmp_path / f"t_{ext}"
        subprocess.check_call([comp, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(f), "-o", str(exe)])
        assert subprocess.run([str(exe)]).returncode == 0, comp
    assert (capi.TRACE_LINE_MAX, capi.TRACE_LINE_MIN, capi.TRACE_LINE_SPREAD) == (0, 1, 2)


def test_launch_shape_follows_the_launcher():
    """tests/emitters_ref.py's tile and grid against the lines of scn_emitters.hip and scn_kernels.h they were read from"""
    csrc = os.path.join(ROOT, "scanner_amd", "csrc")
    src, hdr = open(os.path.join(csrc, "scn_emitters.hip")).read(), open(os.path.join(csrc, "scn_kernels.h")).read()
    assert int(re.search(r"constexpr uint32_t kEmitTile = (\d+);", hdr).group(1)) == ref.TILE
    assert "constexpr uint32_t kEmitTilesMax = (1u << 22) / kEmitTile;" in hdr and (1 << 22) == capi.TRACE_CELLS_MAX
    assert int(re.search(r"constexpr uint32_t kEmitBlock = (\d+);", src).group(1)) == ref.BLOCK
    m = re.search(r"constexpr uint32_t kEmitScanBlock = (\d+), kEmitScanPerThread = (\d+);", src)
    assert (int(m.group(1)), int(m.group(2))) == (ref.SCAN_BLOCK, ref.SCAN_PER_THREAD)
    assert ref.SCAN_BLOCK * ref.SCAN_PER_THREAD == ref.tiles(capi.TRACE_CELLS_MAX)
    assert "constexpr uint32_t kEmitTilesPerBlock = kEmitBlock / 64u;" in src
    assert src.count("const dim3 grid((tiles + kEmitTilesPerBlock - 1u) / kEmitTilesPerBlock), block(kEmitBlock);") == 2  # no grid loop: a tile per wave
    assert "tile = blockIdx.x * kEmitTilesPerBlock + (threadIdx.x >> 6);" in src and "gridDim" not in src
    assert "hipLaunchKernelGGL(scn_emitters_scan_kernel, dim3(1), dim3(kEmitScanBlock), 0, stream, a, tiles);" in src
    assert "hipOccupancy" not in src and "getenv" not in src
    assert "atomicAdd(float" not in src and "atomicAdd((float" not in src
    assert [ref.tiles(c) for c in (1, 1024, 1025, 1 << 22)] == [1, 1, 2, 4096] and [ref.grid(c) for c in (1, 4096, 4097, 1 << 22)] == [1, 1, 2, 1024]
