"""The sweep trace's host forms (scn_trace_fold_spectrum, scn_trace_init, scn_trace_merge: scn_host.hip) against tests/trace_ref.py,
the numpy model written from the definition, on seeded spectra: every cell of every case, as bits.  No device is needed.

Spectra are seeded float32 values with +-inf, NaN (both signs) and +-0.0 put on evaluated bins.  The sample rate is 8 MHz, so
bin_step = sample_rate // n is 500000 at n = 16 and truncated at n = 18 (444444), 1001 (7992) and 4096 (1953).  The geometries, per
n: cell_hz in {1, bin_step, bin_step + 1, 64 bin_step + 7, 3 sample rates (several units in one cell)}, each with f0 inside the
first unit's band and the last cell ending inside the last unit's band (the 1 Hz cells: 2^20 of them inside the first unit's band).  The scenes: units 6 MHz apart (adjacent bands touch), 5 MHz
apart (they overlap), two units on one centre, a centre below sample_rate / 2 (a negative start frequency: the first bins wrap to
frequencies near 2^64 and fold nowhere)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from scanner_amd import capi
from tests import trace_caps, trace_ref

FS = 8000000
SIZES = [16, 18, 1001, 4096]


def spectra(n, units, seed):
    """float32 [units, n] in natural bin order; units 0 and 1 carry the special values on evaluated bins"""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal((units, n)) * 20.0 - 30.0).astype(np.float32)
    ev_j = (np.flatnonzero(trace_ref.evaluated(n)) + n // 2) % n  # natural bins that are evaluated, in fftshift order
    specials = np.array([np.inf, -np.inf, 0.0, -0.0, np.nan], np.float32)
    specials = np.concatenate([specials, np.array([0xFFC00001], np.uint32).view(np.float32)])  # (a NaN with its sign set)
    for u in range(units):
        where = ev_j[(np.arange(specials.size) * 7 + 3 * u) % ev_j.size] if u < 2 else ev_j[:0]
        p[u, where] = specials[: where.size]
    # -0.0 and +0.0 side by side, so that one cell of a wide geometry holds both: the key order decides
    p[-1, ev_j[0]], p[-1, ev_j[1]] = np.float32(-0.0), np.float32(0.0)
    return p


def scenes(n):
    """(name, centres)"""
    return [("touching", 100e6 + 0.5 + 6e6 * np.arange(3)), ("overlapping", 100e6 + 5e6 * np.arange(3)), ("repeated", np.array([100e6, 100e6, 106e6])),
            ("negative_start", np.array([1e6, 3e6, 9e6]))]


def geometries(n, centres):
    """(f0_hz, cell_hz, cells): f0 inside the first unit's band (never below 0), the last cell ending inside the last unit's"""
    bs = FS // n
    f0 = max(0, int(centres[0] - FS / 2 + 0.3 * FS))
    end = int(centres[-1] - FS / 2 + 0.6 * FS)
    out = []
    for cell_hz in (bs, bs + 1, 64 * bs + 7, 3 * FS):
        out.append((f0, cell_hz, max(1, (end - f0) // cell_hz)))
    # 1 Hz cells cannot span a band: 2^20 of them from 3 Hz below unit 0's lowest evaluated bin that did not wrap
    f = trace_ref.bin_freqs(n, FS, centres[0])[trace_ref.evaluated(n)]
    out.append((int(f[f < (1 << 63)].min()) - 3, 1, 1 << 20))
    return out


def host_fold(trace, f0, cell_hz, p, centres, **kw):
    capi.trace_fold_spectrum(trace, f0, cell_hz, p, FS, centres, **kw)
    return trace


@pytest.mark.parametrize("n", SIZES)
def test_host_fold_equals_the_model(built_lib, n):
    p = spectra(n, 3, seed=n)
    assert np.isnan(p).sum() == 4 and np.isinf(p).sum() == 4
    for name, centres in scenes(n):
        for f0, cell_hz, cells in geometries(n, centres):
            want = trace_ref.fold(trace_ref.new(cells), f0, cell_hz, p, FS, centres)
            got = host_fold(capi.trace_init(cells), f0, cell_hz, p, centres)
            assert trace_ref.same(got, want), (name, f0, cell_hz, cells, trace_ref.describe(got, want))
            assert int(want[2].sum()) > 0, (name, cell_hz, "the case folds nothing")
            empty = want[2] == 0  # empty cells read (-inf, +inf, 0)
            assert np.all(np.isneginf(got[0][empty])) and np.all(np.isposinf(got[1][empty]))
            # in/out: two calls accumulate, and merge(A, B) is the trace of both
            a = host_fold(capi.trace_init(cells), f0, cell_hz, p[:2], centres[:2])
            b = host_fold(capi.trace_init(cells), f0, cell_hz, p[2:], centres[2:])
            two = host_fold(tuple(x.copy() for x in a), f0, cell_hz, p[2:], centres[2:])
            assert trace_ref.same(two, want), (name, cell_hz)
            capi.trace_merge(a, b)
            assert trace_ref.same(a, want) and trace_ref.same(trace_ref.merge(b, trace_ref.fold(trace_ref.new(cells), f0, cell_hz, p[:2], FS, centres[:2])), want)


def test_negative_start_wraps_and_is_skipped(built_lib):
    n, centres = 16, np.array([1e6])
    f = trace_ref.bin_freqs(n, FS, centres[0])
    assert f[0] == (1 << 64) - 3000000 and f[5] == (1 << 64) - 500000 and f[6] == 0 and f[7] == 500000
    p = np.arange(n, dtype=np.float32).reshape(1, n)
    got = host_fold(capi.trace_init(4), 0, 1 << 31, p, centres)  # evaluated i in {2, 3, 4} wrap, {12, 13, 14} are 3 ... 4 MHz
    assert got[2].tolist() == [3, 0, 0, 0]


def test_key_order_and_specials(built_lib):
    """one wide cell: -0.0 is below +0.0, +-inf fold, NaN does not; a second fold of the same unit counts twice and changes nothing else"""
    n = 16
    ev_j = (np.flatnonzero(trace_ref.evaluated(n)) + n // 2) % n
    assert np.flatnonzero(trace_ref.evaluated(n)).tolist() == [2, 3, 4, 12, 13, 14]
    p = np.full((1, n), 99.0, np.float32)  # (the bins the mask removes would win every maximum)
    p[0, ev_j] = [-0.0, 0.0, np.nan, -0.0, 0.0, -0.0]
    t = host_fold(capi.trace_init(1), 0, 1 << 31, p, [100e6])
    assert t[2][0] == 5 and t[0].view(np.uint32)[0] == 0x00000000 and t[1].view(np.uint32)[0] == 0x80000000
    host_fold(t, 0, 1 << 31, p, [100e6])
    assert t[2][0] == 10 and t[0].view(np.uint32)[0] == 0x00000000 and t[1].view(np.uint32)[0] == 0x80000000
    p[0, ev_j] = [np.inf, -np.inf, np.nan, 1.0, 2.0, 3.0]
    t = host_fold(capi.trace_init(1), 0, 1 << 31, p, [100e6])
    assert t[2][0] == 5 and np.isposinf(t[0][0]) and np.isneginf(t[1][0])
    p[0, ev_j] = np.nan
    t = host_fold(capi.trace_init(1), 0, 1 << 31, p, [100e6])
    assert trace_ref.same(t, trace_ref.new(1))


def test_mask_arguments(built_lib):
    """dc_ignore_bins and use_bandwidth as the descriptor takes them"""
    n, centres = 64, [100e6]
    p = spectra(n, 1, seed=9)
    for kw in (dict(dc_ignore_bins=0), dict(dc_ignore_bins=9), dict(use_bandwidth=0.5), dict(use_bandwidth=1.0, dc_ignore_bins=1)):
        want = trace_ref.fold(trace_ref.new(40), 96000000, FS // n + 1, p, FS, centres, **kw)
        got = host_fold(capi.trace_init(40), 96000000, FS // n + 1, p, centres, **kw)
        assert trace_ref.same(got, want), (kw, trace_ref.describe(got, want))


@pytest.mark.parametrize("mutant", trace_ref.MUTANTS)
def test_the_cases_tell_each_mutant_apart(mutant):
    """the model with one deliberate error differs from the definition on these very cases -- so the equality above is not vacuous"""
    differing = 0
    for n in SIZES:
        p = spectra(n, 3, seed=n)
        for name, centres in scenes(n):
            for f0, cell_hz, cells in geometries(n, centres):
                want = trace_ref.fold(trace_ref.new(cells), f0, cell_hz, p, FS, centres)
                differing += not trace_ref.same(trace_ref.fold(trace_ref.new(cells), f0, cell_hz, p, FS, centres, mutant=mutant), want)
    assert differing >= 4, (mutant, differing)


def test_rejections(built_lib):
    L = capi.lib()
    mx, mn, ct = capi.trace_init(8)
    p, fc = np.zeros((1, 16), np.float32), np.array([100e6])
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def fold(mx=mx, mn=mn, ct=ct, cell_hz=1000, cells=8, p=p, units=1, n=16, fs=FS, fc=fc):
        return L.scn_trace_fold_spectrum(vp(mx), vp(mn), vp(ct), 0, cell_hz, cells, vp(p), units, n, fs, 0, 0.0, vp(fc))

    assert fold() == capi.OK
    assert fold(units=0, p=None, fc=None) == capi.OK
    before = (mx.copy(), mn.copy(), ct.copy())
    for bad in (dict(mx=None), dict(mn=None), dict(ct=None), dict(p=None), dict(fc=None), dict(cell_hz=0), dict(cells=0),
                dict(cells=capi.TRACE_CELLS_MAX + 1), dict(n=0), dict(n=(1 << 24) + 1), dict(fs=0)):
        assert fold(**bad) == capi.E_INVALID, bad
    assert trace_ref.same((mx, mn, ct), before)
    assert L.scn_trace_init(vp(mx), vp(mn), vp(ct), 0) == capi.E_INVALID
    assert L.scn_trace_init(vp(mx), vp(mn), vp(ct), capi.TRACE_CELLS_MAX + 1) == capi.E_INVALID
    assert L.scn_trace_init(None, vp(mn), vp(ct), 8) == capi.E_INVALID
    assert L.scn_trace_merge(vp(mx), vp(mn), vp(ct), vp(mx), vp(mn), None, 8) == capi.E_INVALID
    assert L.scn_trace_merge(vp(mx), vp(mn), vp(ct), vp(mx), vp(mn), vp(ct), 0) == capi.E_INVALID
    # the plan's three entry points refuse a null plan before they touch a device
    assert L.scn_plan_set_trace(None, 0, 1, 1) == capi.E_INVALID and b"null plan" in L.scn_last_error()
    assert L.scn_plan_update_trace(None, 0) == capi.E_INVALID
    assert L.scn_plan_get_trace(None, 0, 0, None, None, None) == capi.E_INVALID
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "scanner_hip.h")) as fh:
        assert f"#define SCN_TRACE_CELLS_MAX (1u << {capi.TRACE_CELLS_MAX.bit_length() - 1})" in fh.read()


def test_cap_formula_follows_the_launcher():
    """tests/trace_caps.py against the lines of scn_trace.hip, scn_detect.h and scn_mask.h it was read from: a changed grid fails here
    instead of silently turning the GPU suite's two-trip batch into a single-trip one"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scanner_amd", "csrc")
    src = open(os.path.join(csrc, "scn_trace.hip")).read()
    m = re.search(r"constexpr int kTraceBlocksPerCu256 = (\d+), kTraceBlocksPerCu1024 = (\d+);", src)
    assert m and {256: int(m.group(1)), 1024: int(m.group(2))} == trace_caps.TRACE_BLOCKS_PER_CU
    assert "const int per_cu = G::BLOCK == 256u ? kTraceBlocksPerCu256 : kTraceBlocksPerCu1024;" in src
    assert "dim3(scn_team_grid(a.n_units, G::TEAMS, num_cus, per_cu)), dim3(G::BLOCK), 0, stream, a);" in src
    assert "hipOccupancy" not in src
    assert "if (a.n <= 512u) return launch_team<64, VEC>" in src and "if (a.n <= 4096u) return launch_team<256, VEC>" in src
    assert "return launch_team<1024, VEC>" in src
    assert "for (uint32_t u0 = blockIdx.x * G::TEAMS + team; u0 < a.n_units; u0 += gridDim.x * G::TEAMS)" in src
    detect = open(os.path.join(csrc, "scn_detect.h")).read()
    assert "BLOCK = T == 64 ? 256u : (uint32_t)T, TEAMS = BLOCK / (uint32_t)T;" in detect
    mask = open(os.path.join(csrc, "scn_mask.h")).read()
    assert "const uint32_t resident = (uint32_t)(num_cus > 0 ? num_cus : 256) * (uint32_t)per_cu;" in mask
    assert "return blocks < resident ? blocks : resident;" in mask
    assert [trace_caps.trace_team(n) for n in (16, 512, 513, 4096, 4097, 65536)] == [64, 64, 256, 256, 1024, 1024]
    assert [trace_caps.trace_cap(256, n) for n in (16, 1024, 8192)] == [256 * 32, 256 * 8, 256 * 2]
