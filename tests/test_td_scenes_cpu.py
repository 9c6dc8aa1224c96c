"""The time-domain scenes of tests/td_scenes.py, pinned on the host (no GPU) on the REFERENCE ALONE: what tests/test_time_domain_gpu.py
holds the two time-domain kernels to has to be true of the inputs first.  These are conditions on the inputs, not measurements: an
input that misses one is changed, not the condition.

For every scene and format the GPU module submits:
  * the planted maximum and the planted (nonzero) minimum are the buffer's extremes by at least 1 dB, every other sample lies
    above 0 dB, and the reference's maximum is not the clamp constant numeric_limits<float>::min() -- except where no buffer can
    do that: DC removal at n = 1 (a sample less its own mean is zero: the reference returns (FLT_MIN, -inf), asserted) and at
    n = 2 (two samples less their mean are +-half their difference, one count apart where the integer mean rounds: at 49 counts or more that is 0.09 dB; maximum and
    minimum within 0.1 dB of each other, asserted);
  * the plain numpy reference and oracle.time_domain agree: exactly on +-inf, FLT_MIN and FLT_MAX, within 1e-4 dB elsewhere;
  * the levels of the launch-shape scene: two levels of a format are at least 1e-3 dB apart (ten times the bar on the maximum), and
    the pairs of buffers a stride or indexing error could swap (b +- 1, b +- 4, b +- grid, b +- 4 grid) carry different levels of
    both extremes -- at the grid of an MI355X (256 CUs) and of other CU counts;
  * the threshold the GPU module takes (the middle level of the launch) leaves both above == 1 and above == 0 among the buffers,
    and the buffers AT that level are above (process.cpp:226, >=);
  * the special rows: the oracle's values (all NaN: (FLT_MIN, FLT_MAX); all +inf: (inf, FLT_MAX); |x| = 1e-20: a minimum of
    -200 dB within 1e-4 dB) and the rest of what the rows are for."""
import numpy as np
import pytest

from tests import td_scenes as sc

WAVE_SIZES = [8, 16, 24, 64, 512, 520, 1024, 1032, 2048, 2056]
SAMPLE_SIZES = [1, 2, 7, 9, 63, 65, 255, 257, 1001]
FMT_IDS = [f.replace("/", "-") for f in sc.FORMATS]
CUS = 256   # MI355X


def launch_cases(cus):
    """(n, nb, grid) of the launch-shape test on a device of `cus` compute units: scn_launch_time_domain caps the grid at 8 blocks
    per CU; the wave form runs 4 buffers per block, the per-sample form 1"""
    grid = 8 * cus
    return [(8, 2 * 4 * grid + 3, grid), (520, 2 * 4 * grid + 3, grid), (9, 2 * grid + 3, grid), (257, 2 * grid + 3, grid),
            (8, 1, grid), (8, 3, grid), (8, 5, grid)]


def _check_scene(oracle_mod, fmt, n, raw, pos_max, pos_min):
    mx, mn, p = sc.reference(oracle_mod, fmt, n, raw)
    mx2, mn2, _ = sc.second_opinion(oracle_mod, fmt, n, raw)
    sc.agree(mx2, mx, 1e-4)
    sc.agree(mn2, mn, 1e-4)
    rows = np.arange(len(raw))
    if sc.CLEAR(fmt, n):
        up, down, low = sc.margins(p, pos_max, pos_min)
        assert (mx != sc.FLT_MIN).all() and np.isfinite(mx).all() and np.isfinite(mn).all()
        assert np.array_equal(mx, np.maximum(sc.db_of_power(p[rows, pos_max]), sc.FLT_MIN)), "the planted sample is the maximum"
        if n > 1:
            assert (p[rows, pos_min] > 0).all() and np.array_equal(mn, sc.db_of_power(p[rows, pos_min])), "the planted sample is the minimum"
            assert up >= sc.CLEAR_DB and down >= sc.CLEAR_DB and low > 0.0, (fmt, n, up, down, low)
    elif n == 1:
        assert (mx == sc.FLT_MIN).all() and np.isneginf(mn).all()
    else:
        assert n == 2 and np.isfinite(mx).all() and (mx > 0).all() and (np.abs(mx - mn) < 0.1).all()
    return mx, mn, mx2


def _check_flags(oracle_mod, fmt, n, raw, mx2):
    """the oracle's flags at the threshold the GPU module takes: the middle level of the launch"""
    thr = np.float32(sc.middle_threshold(mx2))
    ab = sc.second_opinion(oracle_mod, fmt, n, raw, float(thr))[2]
    assert np.array_equal(ab, (mx2 >= thr).astype(np.uint8))
    assert (mx2 == thr).any() and ab[mx2 == thr].all(), "the buffers at the threshold are above (>=)"
    if len(raw) >= 3:
        assert ab.min() == 0 and ab.max() == 1, "both outcomes occur"


@pytest.mark.parametrize("fmt", sc.FORMATS, ids=FMT_IDS)
def test_position_scenes(oracle_mod, fmt):
    for n in WAVE_SIZES + SAMPLE_SIZES:
        raw, pos_max, pos_min = sc.position(fmt, n)
        assert len(raw) == len(pos_max) == len(pos_min) == n + (n > 1 and n % 2) and np.array_equal(pos_max[:n], np.arange(n))
        keep = np.ones(len(raw), bool)
        keep[n // 2] = n == 1 or n % 2 == 0          # (an odd n: buffer (n - 1) / 2 has its minimum one sample on, buffer n has it there)
        assert sorted(pos_min[keep]) == list(range(n)), "every sample is the maximum of one buffer and the minimum of one"
        if n > 1:
            assert (pos_max != pos_min).all()
        mx, mn, _ = _check_scene(oracle_mod, fmt, n, raw, pos_max, pos_min)
        assert len(np.unique(mx)) == 1 and len(np.unique(mn)) == 1, "every buffer of a position scene holds the same values"


@pytest.mark.parametrize("fmt", sc.FORMATS, ids=FMT_IDS)
def test_levels_are_apart(oracle_mod, fmt):
    """the planted levels THROUGH THE CONVERTER, one buffer per level (the wave form's smallest size)"""
    n, nb = 8, sc.N_MAX_LEVELS
    lv = np.arange(nb)
    raw = sc._assemble(fmt, n, np.zeros(nb, np.int64), np.full(nb, n - 1), lv, lv % sc.N_MIN_LEVELS, seed=5)
    mx, mn, _ = sc.reference(oracle_mod, fmt, n, raw)
    assert np.diff(mx).max() <= -sc.LEVEL_DB, (fmt, np.diff(mx).max())             # strongest first
    assert np.diff(mn[:sc.N_MIN_LEVELS]).min() >= sc.LEVEL_DB, (fmt, np.diff(mn[:sc.N_MIN_LEVELS]).min())


@pytest.mark.parametrize("cus", [256, 304, 64, 8])
def test_level_indices_separate_what_a_stride_error_swaps(cus):
    grid = 8 * cus
    nb = 2 * 4 * grid + 3
    lmax, lmin = sc.level_indices(nb, grid)
    assert lmax.max() < sc.N_MAX_LEVELS and lmin.max() < sc.N_MIN_LEVELS
    for d in (1, 4, grid, 4 * grid):
        assert (lmax[d:] != lmax[:-d]).all() and (lmin[d:] != lmin[:-d]).all(), d


@pytest.mark.parametrize("fmt", sc.FORMATS, ids=FMT_IDS)
def test_launch_shape_scenes(oracle_mod, fmt):
    for n, nb, grid in launch_cases(CUS):
        raw, pos_max, pos_min = sc.launch_shape(fmt, n, nb, grid)
        assert len(raw) == nb
        mx, mn, mx2 = _check_scene(oracle_mod, fmt, n, raw, pos_max, pos_min)
        _check_flags(oracle_mod, fmt, n, raw, mx2)
        for d in (1, 4, grid, 4 * grid):
            if d < nb:
                assert np.abs(mx[d:] - mx[:-d]).min() >= sc.LEVEL_DB and np.abs(mn[d:] - mn[:-d]).min() >= sc.LEVEL_DB, (fmt, n, nb, d)


@pytest.mark.parametrize("fmt", sc.FORMATS, ids=FMT_IDS)
def test_long_buffer_scenes(oracle_mod, fmt):
    cases = [(1 << 20, 3)] + ([(1 << 24, 2)] if fmt == "int8" else [])
    for n, nb in cases:
        raw, pos_max, pos_min = sc.long_buffers(fmt, n, nb)
        assert (pos_max == n - 1).all() and (pos_min == n - 2).all()
        m, mean = sc.offset_and_mean(fmt, n)
        if fmt.startswith("int16") and sc.FORMATS[fmt][2]:
            assert (m, mean) == (8192, 0), "2^20 samples of mean 8192 sum to 2^33: the int32 sum wraps to 0"
            w = raw.astype(np.int64)
            sums = w.sum(axis=2 if sc.FORMATS[fmt][0] == sc.KIND_SHORT else 1)
            assert (sums == 1 << 33).all()
            conv = sc.convert(oracle_mod, fmt, n, raw[:1])
            assert conv[0, n - 1] == np.complex64(complex(*(sc.max_levels(fmt)[0] / 2048.0))), "the converter took nothing out"
        mx, mn, mx2 = _check_scene(oracle_mod, fmt, n, raw, pos_max, pos_min)
        _check_flags(oracle_mod, fmt, n, raw, mx2)
        assert np.abs(np.diff(mx)).min() >= sc.LEVEL_DB and np.abs(np.diff(mn)).min() >= sc.LEVEL_DB


@pytest.mark.parametrize("n", [16, 1001])
def test_special_rows(oracle_mod, n):
    x = sc.special_rows(n)
    assert len(x) == len(sc.SPECIAL)
    mx, mn = sc.extremes(sc.powers(x))
    o = oracle_mod.Oracle(n)
    ref = [o.time_domain(x[r], threshold=0.0) for r in range(len(x))]
    omx, omn = np.array([r[1] for r in ref], np.float32), np.array([r[2] for r in ref], np.float32)
    sc.agree(omx, mx, 1e-4)
    sc.agree(omn, mn, 1e-4)
    row = {name: r for r, name in enumerate(sc.SPECIAL)}
    inf, F32 = np.float32(np.inf), np.float32
    assert (omx[row["all NaN"]], omn[row["all NaN"]]) == (F32(sc.FLT_MIN), F32(sc.FLT_MAX))
    assert (omx[row["all +inf"]], omn[row["all +inf"]]) == (inf, F32(sc.FLT_MAX))
    assert omx[row["all 1e-20"]] == F32(sc.FLT_MIN) and abs(float(omn[row["all 1e-20"]]) + 200.0) < 1e-4
    assert abs(float(omn[row["one 1e-20 sample"]]) + 200.0) < 1e-4
    plain = (omx[row["plain"]], omn[row["plain"]])
    assert np.isfinite(plain).all() and plain[0] > plain[1] > 0
    for name in ("NaN in sample 0", "NaN in the last sample"):       # a NaN is never taken
        assert (omx[row[name]], omn[row[name]]) == plain, name
    assert (omx[row["one +inf"]], omn[row["one +inf"]]) == (inf, plain[1])
    assert (omx[row["one zero and one -0.0"]], omn[row["one zero and one -0.0"]]) == (plain[0], -inf)
    assert (omx[row["one power overflows"]], omn[row["one power overflows"]]) == (inf, plain[1])
    p = sc.powers(x[row["one power near FLT_MAX"]][None])[0]
    assert np.isfinite(p).all() and p.max() > 0.99 * sc.FLT_MAX
    assert abs(float(omx[row["one power near FLT_MAX"]]) - 5.0 * np.log10(float(p.max()))) < 1e-4 and omn[row["one power near FLT_MAX"]] == plain[1]
    assert np.isinf(sc.powers(x[row["one power overflows"]][None])).sum() == 1


def test_the_reference_takes_what_the_oracle_takes():
    """extremes() on hand-made powers: the comparisons of process.cpp:222-223"""
    nan, inf = np.nan, np.inf
    p = np.array([[nan, nan], [inf, inf], [nan, 4.0], [0.0, 4.0], [inf, 4.0], [sc.FLT_MAX, sc.FLT_MAX], [0.25, 0.5]], np.float32)
    mx, mn = sc.extremes(p)
    d4 = 5.0 * np.log10(4.0)
    assert mx.tolist() == [sc.FLT_MIN, inf, d4, d4, inf, 5.0 * np.log10(sc.FLT_MAX), sc.FLT_MIN]
    assert mn.tolist() == [sc.FLT_MAX, sc.FLT_MAX, d4, -inf, d4, 5.0 * np.log10(sc.FLT_MAX), 5.0 * np.log10(0.25)]
