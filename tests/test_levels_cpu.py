"""The level histogram's host forms (scn_levels_fold_spectrum, scn_levels_merge, scn_levels_summary: scn_host.hip) against
tests/levels_ref.py, the numpy model written from the definition: every counter of every case, as integers.  No device is needed.

The spectra, the scenes and the geometries are those of tests/test_trace_cpu.py (seeded float32 values with +-inf, NaN of both
signs and +-0.0 on evaluated bins; cell_hz in {bin_step, bin_step + 1, 64 bin_step + 7, three sample rates, 1}).  A geometry whose
cells times the table's levels exceed SCN_LEVELS_WORDS_MAX keeps its f0_hz and cell_hz and as many cells as that limit allows (the 1
Hz grid of 2^20 cells under 63 and 255 edges).  The tables: 1, 2, 7, 63 and 255 edges, among them -inf and +inf as end edges, the
adjacent pair -0.0, +0.0, and edges taken from the spectrum's own values, so that a value equal to an edge occurs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from scanner_amd import capi
from tests import levels_caps, levels_ref, trace_ref
from tests.test_trace_cpu import FS, SIZES, geometries, scenes, spectra

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scanner_amd", "csrc")


def own_values(p):
    """the finite values on evaluated bins of the spectra p, sorted, unique as bits"""
    n = p.shape[1]
    ev_j = (np.flatnonzero(trace_ref.evaluated(n)) + n // 2) % n
    v = p[:, ev_j].reshape(-1)
    v = v[np.isfinite(v) & (v != 0)]
    return np.unique(v)


def tables(p):
    """{n_edges: edges float32}, each strictly increasing in key order"""
    own = own_values(p)
    out = {1: own[own.size // 2: own.size // 2 + 1],
           2: np.array([-0.0, 0.0], np.float32),
           7: np.array([-np.inf, -60.0, float(own[own.size // 3]), -0.0, 0.0, 10.0, np.inf], np.float32)}
    steps = np.arange(-61, 2, dtype=np.float32)  # 63 edges one unit apart; every eighth gives way to the own value next above it
    for k in range(0, 63, 8):
        above = own[(own > steps[k]) & (own < steps[k] + 1)]
        if above.size:
            steps[k] = above[0]
    out[63] = steps
    picked = own[np.linspace(0, own.size - 1, min(own.size, 100)).astype(int)]
    rest = np.linspace(-120.0, 60.0, 400).astype(np.float32)
    e = np.unique(np.concatenate([picked, rest[~np.isin(rest, picked)][: 255 - np.unique(picked).size]]))
    out[255] = e
    for k, e in out.items():
        assert e.dtype == np.float32 and e.size == k and levels_ref.edges_valid(e), k
    return out


def on_an_edge(p, edges):
    """evaluated bins whose value is, bit for bit, an edge"""
    n = p.shape[1]
    ev_j = (np.flatnonzero(trace_ref.evaluated(n)) + n // 2) % n
    return int(np.isin(p[:, ev_j].view(np.uint32), np.ascontiguousarray(edges, np.float32).view(np.uint32)).sum())


def clip(cells, n_edges):
    return min(cells, capi.LEVELS_WORDS_MAX // (n_edges + 1))


def host_fold(hist, f0, cell_hz, edges, p, centres, **kw):
    capi.levels_fold_spectrum(hist, f0, cell_hz, edges, p, FS, centres, **kw)
    return hist


def cases(n, p):
    """(scene, centres, f0_hz, cell_hz, cells, n_edges, edges): every table on two scenes, 7 and 63 edges on all four"""
    tabs = tables(p)
    for name, centres in scenes(n):
        for k, edges in tabs.items():
            if k in (7, 63) or name in ("touching", "negative_start"):
                for f0, cell_hz, cells in geometries(n, centres):
                    yield name, centres, f0, cell_hz, clip(cells, k), k, edges


@pytest.mark.parametrize("n", SIZES)
def test_host_fold_equals_the_model(built_lib, n):
    p = spectra(n, 3, seed=n)
    assert np.isnan(p).sum() == 4 and np.isinf(p).sum() == 4 and (np.signbit(p) & (p == 0)).sum() >= 2
    tabs = tables(p)
    assert all(on_an_edge(p, tabs[k]) > 0 for k in (1, 2, 7, 63, 255)), "no value equals an edge"
    for name, centres, f0, cell_hz, cells, k, edges in cases(n, p):
        want = levels_ref.fold(levels_ref.new(cells, k), f0, cell_hz, edges, p, FS, centres)
        got = host_fold(levels_ref.new(cells, k), f0, cell_hz, edges, p, centres)
        assert levels_ref.same(got, want), (name, f0, cell_hz, cells, k, levels_ref.describe(got, want))
        assert int(want.sum()) > 0, (name, cell_hz, "the case folds nothing")
        if cell_hz == 1:
            continue
        # in/out: two calls accumulate, and merge(A, B) is the histogram of both
        a = host_fold(levels_ref.new(cells, k), f0, cell_hz, edges, p[:2], centres[:2])
        b = host_fold(levels_ref.new(cells, k), f0, cell_hz, edges, p[2:], centres[2:])
        two = host_fold(a.copy(), f0, cell_hz, edges, p[2:], centres[2:])
        assert levels_ref.same(two, want), (name, cell_hz, k)
        capi.levels_merge(a, b)
        assert levels_ref.same(a, want), (name, cell_hz, k)


def test_levels_by_hand(built_lib):
    """one wide cell, n = 16 (evaluated i = 2, 3, 4, 12, 13, 14): a value equal to an edge belongs to the level above it; -0.0 is
    below the edge +0.0 and at the edge -0.0; +-inf count, also where they are edges; NaN does not"""
    n = 16
    ev_j = (np.flatnonzero(trace_ref.evaluated(n)) + n // 2) % n
    assert np.flatnonzero(trace_ref.evaluated(n)).tolist() == [2, 3, 4, 12, 13, 14]
    p = np.full((1, n), 5.0, np.float32)  # (the bins the mask removes would all land in one level)
    p[0, ev_j] = [-0.0, 0.0, np.nan, -1.0, 1.0, 0.5]
    h = host_fold(levels_ref.new(1, 3), 0, 1 << 31, [-0.0, 0.0, 1.0], p, [100e6])
    assert h.tolist() == [[1, 1, 2, 1]]  # -1 | -0.0 | +0.0, 0.5 | 1.0
    p[0, ev_j] = [np.inf, -np.inf, np.array([0xFFC00001], np.uint32).view(np.float32)[0], -3.0e38, 3.0e38, 0.0]
    h = host_fold(levels_ref.new(1, 2), 0, 1 << 31, [-np.inf, np.inf], p, [100e6])
    assert h.tolist() == [[0, 4, 1]]  # nothing is below -inf; +inf is at the edge +inf
    h = host_fold(h, 0, 1 << 31, [-np.inf, np.inf], p, [100e6])
    assert h.tolist() == [[0, 8, 2]]
    p[0, ev_j] = np.nan
    assert host_fold(levels_ref.new(1, 1), 0, 1 << 31, [0.0], p, [100e6]).sum() == 0


def test_mask_arguments(built_lib):
    n, centres = 64, [100e6]
    p = spectra(n, 1, seed=9)
    edges = tables(p)[7]
    for kw in (dict(dc_ignore_bins=0), dict(dc_ignore_bins=9), dict(use_bandwidth=0.5), dict(use_bandwidth=1.0, dc_ignore_bins=1)):
        want = levels_ref.fold(levels_ref.new(40, 7), 96000000, FS // n + 1, edges, p, FS, centres, **kw)
        got = host_fold(levels_ref.new(40, 7), 96000000, FS // n + 1, edges, p, centres, **kw)
        assert levels_ref.same(got, want), (kw, levels_ref.describe(got, want))


@pytest.mark.parametrize("mutant", levels_ref.MUTANTS)
def test_the_cases_tell_each_mutant_apart(mutant):
    """the model with one deliberate error differs from the definition on these very cases -- so the equality above is not vacuous"""
    differing = 0
    for n in SIZES:
        p = spectra(n, 3, seed=n)
        for name, centres, f0, cell_hz, cells, k, edges in cases(n, p):
            if cell_hz == 1 or name != "touching":
                continue
            want = levels_ref.fold(levels_ref.new(cells, k), f0, cell_hz, edges, p, FS, centres)
            differing += not levels_ref.same(levels_ref.fold(levels_ref.new(cells, k), f0, cell_hz, edges, p, FS, centres, mutant=mutant), want)
    assert differing >= 4, (mutant, differing)


def summary_histograms(n_levels, seed):
    """uint64 [cells, n_levels]: an empty cell, cells of one count (first, a middle, the last level), seeded small counts, a cell of
    equal counts, and cells whose counts exceed 2^32 and whose total nears 2^64 -- built with scn_levels_merge, by doubling"""
    rng = np.random.default_rng(seed)
    h = np.zeros((12, n_levels), np.uint64)
    h[1, 0] = h[2, n_levels // 2] = h[3, n_levels - 1] = 1
    h[4] = rng.integers(0, 5, n_levels)
    h[5] = rng.integers(0, 1000, n_levels)
    h[6] = 3
    h[7, rng.integers(0, n_levels, 3)] = 2  # (few occupied levels: long runs of equal cumulative counts)
    big = np.zeros((4, n_levels), np.uint64)
    big[0] = rng.integers(1, (1 << 23) // n_levels, n_levels)  # (total below 2^23, times 2^40: below 2^63)
    big[1, :2] = [3, 5]
    big[2, n_levels - 1] = 1
    big[3, rng.integers(0, n_levels, 2)] = 7
    for _ in range(40):  # times 2^40
        capi.levels_merge(big, big.copy())
    assert big.max() > (1 << 32) and sum(int(x) for x in big[0]) < (1 << 64)
    assert any(1000 * sum(int(x) for x in row) >= (1 << 64) for row in big), "no cell where permille * (total - 1) overflows 64 bits"
    h[8:12] = big
    return h


@pytest.mark.parametrize("n_levels", [2, 3, 8, 64, 256])
def test_summary_equals_the_model(built_lib, n_levels):
    h = summary_histograms(n_levels, seed=n_levels)
    for level in range(n_levels):
        for permille in (0, 1, 500, 999, 1000):
            got = capi.levels_summary(h, permille, level)
            want = levels_ref.summary(h, permille, level)
            for name, g, w in zip(("rank_level", "above", "total"), got, want):
                assert levels_ref.same(g, w), (n_levels, permille, level, name, g.tolist(), w.tolist())
    rank, above, total = capi.levels_summary(h, 500, n_levels - 1)
    assert rank[0] == capi.LEVELS_NO_RANK and above[0] == 0 and total[0] == 0
    assert rank[1:4].tolist() == [0, n_levels // 2, n_levels - 1] and total[1:4].tolist() == [1, 1, 1] and above[1:4].tolist() == [0, int(n_levels == 2), 1]


def test_summary_of_a_folded_histogram_and_null_outputs(built_lib):
    n = 1001
    p = spectra(n, 3, seed=n)
    name, centres = scenes(n)[0]
    f0, cell_hz, cells = geometries(n, centres)[2]
    edges = tables(p)[63]
    h = host_fold(levels_ref.new(cells, 63), f0, cell_hz, edges, p, centres)
    for permille, level in ((0, 0), (500, 30), (1000, 63)):
        got, want = capi.levels_summary(h, permille, level), levels_ref.summary(h, permille, level)
        assert all(levels_ref.same(g, w) for g, w in zip(got, want)), (permille, level)
    only = np.zeros(cells, np.uint64)  # any output may be NULL
    vp = only.ctypes.data_as(C.c_void_p)
    assert capi.lib().scn_levels_summary(h.ctypes.data_as(C.c_void_p), cells, 64, 500, 0, None, None, vp) == capi.OK
    assert np.array_equal(only, h.sum(axis=1))
    assert capi.lib().scn_levels_summary(h.ctypes.data_as(C.c_void_p), cells, 64, 500, 0, None, None, None) == capi.OK


def test_rejections(built_lib):
    L = capi.lib()
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    hist = np.zeros((8, 4), np.uint64)
    hist[2, 1] = 5
    good = np.array([-1.0, 0.0, 1.0], np.float32)
    p, fc = np.zeros((1, 16), np.float32), np.array([100e6])
    big = np.zeros(256, np.float32)

    def fold(hist=hist, cell_hz=1000, cells=8, edges=good, n_edges=3, p=p, units=1, n=16, fs=FS, fc=fc):
        return L.scn_levels_fold_spectrum(vp(hist), 0, cell_hz, cells, vp(edges), n_edges, vp(p), units, n, fs, 0, 0.0, vp(fc))

    before = hist.copy()
    assert fold(units=0, p=None, fc=None) == capi.OK and np.array_equal(hist, before)
    nan = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
    bad_edges = [np.array(e, np.float32) for e in ([0.0, -1.0, 1.0], [-1.0, 0.0, 0.0], [-1.0, 1.0, 1.0], [0.0, -0.0, 1.0], [-1.0, np.nan, 1.0],
                                                   [-1.0, 0.0, nan], [np.inf, np.inf, np.inf], [np.nan, 0.0, 1.0])]
    for bad in ([dict(hist=None), dict(edges=None), dict(p=None), dict(fc=None), dict(cell_hz=0), dict(cells=0), dict(n_edges=0),
                 dict(edges=big, n_edges=256), dict(cells=capi.TRACE_CELLS_MAX + 1), dict(cells=capi.LEVELS_WORDS_MAX // 4 + 1), dict(n=0),
                 dict(n=(1 << 24) + 1), dict(fs=0)] + [dict(edges=e) for e in bad_edges]):
        assert fold(**bad) == capi.E_INVALID, bad
        assert np.array_equal(hist, before), bad
    assert fold(edges=np.array([-0.0, 0.0, 1.0], np.float32)) == capi.OK  # (-0.0 and +0.0 are two edges)
    assert fold(edges=np.array([-np.inf, 0.0, np.inf], np.float32)) == capi.OK
    hist[:] = before
    # merge
    src = np.ones((8, 4), np.uint64)
    for args in ((None, vp(src), 8, 4), (vp(hist), None, 8, 4), (vp(hist), vp(src), 0, 4), (vp(hist), vp(src), 8, 1), (vp(hist), vp(src), 8, 0),
                 (vp(hist), vp(src), 8, 257), (vp(hist), vp(src), capi.LEVELS_WORDS_MAX // 4 + 1, 4)):
        assert L.scn_levels_merge(*args) == capi.E_INVALID, args
    assert np.array_equal(hist, before)
    # summary
    rank, above, total = np.full(8, 77, np.uint32), np.full(8, 77, np.uint64), np.full(8, 77, np.uint64)

    def summary(hist=hist, cells=8, n_levels=4, permille=500, level=0):
        return L.scn_levels_summary(vp(hist), cells, n_levels, permille, level, vp(rank), vp(above), vp(total))

    for bad in (dict(hist=None), dict(cells=0), dict(n_levels=1), dict(n_levels=257), dict(permille=1001), dict(level=4), dict(level=0xFFFFFFFF),
                dict(cells=capi.LEVELS_WORDS_MAX // 4 + 1)):
        assert summary(**bad) == capi.E_INVALID, bad
    assert (rank == 77).all() and (above == 77).all() and (total == 77).all()
    assert summary(permille=1000, level=3) == capi.OK and total[2] == 5 and rank[2] == 1
    # the plan's four entry points refuse a null plan before they touch a device
    assert L.scn_plan_set_levels(None, 0, 1, 1, vp(good), 3) == capi.E_INVALID and b"null plan" in L.scn_last_error()
    assert L.scn_plan_update_levels(None, 0) == capi.E_INVALID and b"null plan" in L.scn_last_error()
    assert L.scn_plan_get_levels(None, 0, 0, None) == capi.E_INVALID and b"null plan" in L.scn_last_error()
    assert L.scn_plan_levels_summary(None, 0, 0, 500, 0, None, None, None) == capi.E_INVALID and b"null plan" in L.scn_last_error()
    with open(os.path.join(os.path.dirname(CSRC), "..", "include", "scanner_hip.h")) as fh:
        header = fh.read()
    assert f"#define SCN_LEVELS_EDGES_MAX {capi.LEVELS_EDGES_MAX}u" in header
    assert f"#define SCN_LEVELS_WORDS_MAX (1u << {capi.LEVELS_WORDS_MAX.bit_length() - 1})" in header


def test_cap_formula_follows_the_launcher():
    """tests/levels_caps.py against the lines of scn_levels.hip, scn_levels.h, scn_detect.h and scn_mask.h it was read from: a
    changed grid or tile fails here instead of silently turning the GPU suite's two-trip batch into a single-trip one, or its
    fits-the-tile grid into one that does not"""
    src = open(os.path.join(CSRC, "scn_levels.hip")).read()
    m = re.search(r"constexpr int kLevelsBlocksPerCu256 = (\d+), kLevelsBlocksPerCu1024 = (\d+);", src)
    assert m and {256: int(m.group(1)), 1024: int(m.group(2))} == levels_caps.LEVELS_BLOCKS_PER_CU
    m = re.search(r"constexpr int kLevelsTileWords256 = (\d+), kLevelsTileWords1024 = (\d+);", src)
    assert m and {256: int(m.group(1)), 1024: int(m.group(2))} == levels_caps.LEVELS_TILE_WORDS
    assert "const int per_cu = G::BLOCK == 256u ? kLevelsBlocksPerCu256 : kLevelsBlocksPerCu1024;" in src
    assert "dim3(scn_team_grid(a.n_units, G::TEAMS, num_cus, per_cu)), dim3(G::BLOCK), 0, stream, a);" in src
    assert "hipOccupancy" not in src
    assert "if (a.n <= 512u) return launch_team<64, VEC>" in src and "if (a.n <= 4096u) return launch_team<256, VEC>" in src
    assert "return launch_team<1024, VEC>" in src
    assert "for (uint32_t u0 = blockIdx.x * G::TEAMS + team; u0 < a.n_units; u0 += gridDim.x * G::TEAMS)" in src
    assert "BLOCK_TILE = T == 1024 ? (uint32_t)kLevelsTileWords1024 : (uint32_t)kLevelsTileWords256, TILE = BLOCK_TILE / G::TEAMS;" in src
    assert "tile_cells = TILE / n_levels;" in src
    assert "__shared__ uint32_t s_keys[kLevelsKeys];" in src and "__shared__ uint32_t s_tile[BLOCK_TILE];" in src
    assert f"constexpr uint32_t kLevelsKeys = {levels_caps.KEYS}u;" in open(os.path.join(CSRC, "scn_levels.h")).read()
    detect = open(os.path.join(CSRC, "scn_detect.h")).read()
    assert "BLOCK = T == 64 ? 256u : (uint32_t)T, TEAMS = BLOCK / (uint32_t)T;" in detect
    mask = open(os.path.join(CSRC, "scn_mask.h")).read()
    assert "const uint32_t resident = (uint32_t)(num_cus > 0 ? num_cus : 256) * (uint32_t)per_cu;" in mask
    # the stated workgroups per CU fit a CU's LDS with their tile and keys
    for block, per_cu in levels_caps.LEVELS_BLOCKS_PER_CU.items():
        assert (levels_caps.LEVELS_TILE_WORDS[block] + levels_caps.KEYS) * 4 * per_cu <= levels_caps.LDS_BYTES_PER_CU
    assert [levels_caps.levels_team(n) for n in (16, 512, 513, 4096, 4097, 65536)] == [64, 64, 256, 256, 1024, 1024]
    assert [levels_caps.levels_cap(256, n) for n in (16, 1024, 8192)] == [256 * 32, 256 * 8, 256 * 2]
    assert [levels_caps.tile_cells(n, e) for n, e in ((16, 63), (16, 255), (4096, 63), (4096, 255), (8192, 63))] == [16, 4, 64, 16, 128]
