"""Time-domain scenes and a plain reference of process.cpp:203-237, shared by tests/test_td_scenes_cpu.py (which pins what the scenes
are, on the reference alone) and tests/test_time_domain_gpu.py (which holds scn_time_domain_kernel and scn_time_domain_wave_kernel
to them).  No GPU and no pytest in here.

THE REFERENCE (reference()): the wire buffers through oracle.Oracle(...).convert (bit-pinned to the reference's utility.cpp),
p = re * re + im * im in numpy float32 (two roundings and a third: unfused, as process.cpp:220), the largest p that is no NaN and the
smallest p the reference's `magnitude < minMagnitude` can take (finite or zero: NaN and +inf never replace FLT_MAX), then
5 log10(p) in float64 under the reference's clamps: max >= numeric_limits<float>::min(), a minimum nothing replaced stays FLT_MAX.
oracle.time_domain (float, sample by sample) is the second opinion; the CPU module holds the two together.

WHAT A SCENE IS.  Everything is laid out in COUNTS of the wire format and, for cfloat, divided by 2048 at the end (int16 at ENOB 12
and cfloat carry the same numbers).  0 dB is |x| = 1: 2048 counts of int16 at ENOB 12, 8 counts of int8 at ENOB 4.
  * background: |re|, |im| in 4096 ... 8192 counts (int8: 24 ... 48), random signs, drawn in (v, -v) pairs -- every background
    magnitude lies above 0 dB, so a buffer's maximum is never the clamp constant;
  * a planted maximum at one of 25 levels near (-32000, 32000) (int8: (-128, 127)) and a planted minimum at one of 9 levels of a
    few counts ((1, 0) ... (3, 3)); each stands at least 1 dB clear of every other sample of its buffer, and two levels are at least
    1e-3 dB apart (both asserted by the CPU module; 1 dB is a factor 1.58 in p, 1e-3 dB is 4.6e-4 of p);
  * DC removal: the values above are what the converter is to LEAVE; the wire carries them plus a positive offset m (8192 / 16),
    and the background is shifted so that the buffer's values sum to zero, which makes the integer mean m exactly and the sums
    positive (the negative-sum quirk of utility.cpp:77-78 has tests/test_parity_gpu.py test_dc_quirk_negative_mean_time_domain).
    Up to 15 background samples (int8: 7) the background is the balancing share of the planted pair plus a small jitter, beyond
    that the pairs plus the share.  With n = 1 and n = 2 no such buffer exists -- one sample less its own mean is zero, two are
    +-half their difference -- and the scene is what it is (sums still positive): the reference says what comes out, and CLEAR()
    says where the margins hold;
  * n m >= 2^31 (int16 at 2^20 samples: 2^33): the int32 sum wraps to exactly 0, the mean is 0 and the converter leaves the offset
    in.  The scene is then laid out around m (background m +- 1024 ... 4096) so that the margins hold on what the reference sees.

position(): nb = n buffers that hold the same values: buffer b has the maximum at sample b and the minimum at sample n - 1 - b, the
background in the free places in one order (n = 1: the one sample is both; odd n > 1: in buffer (n - 1) / 2 the two meet, its minimum
moves on one sample and buffer n has the minimum in the middle, so that every sample is the maximum once and the minimum once).  launch_shape(): levels that are functions of the buffer index -- see level_indices().  long_buffers(): the maximum in
the last sample, the minimum in the one before.  special_rows(): cfloat rows of special values."""
import numpy as np

FLT_MIN = float(np.float32(1.17549435e-38))
FLT_MAX = float(np.float32(3.40282347e+38))
MAX_BAR, MIN_BAR = 1e-4, 2e-3      # dB: the bars of tests/test_parity_gpu.py test_time_domain_mode
CLEAR_DB, LEVEL_DB = 1.0, 1e-3     # a planted extreme over every other sample; two neighbouring levels
N_MAX_LEVELS, N_MIN_LEVELS = 25, 9

KIND_BYTE_COMPLEX, KIND_SHORT, KIND_SHORT_COMPLEX, KIND_FLOAT_COMPLEX = 1, 2, 3, 4   # scanner_amd.capi / oracle.oracle

# name -> (kind, enob, correct_dc)
FORMATS = {
    "cfloat": (KIND_FLOAT_COMPLEX, 12, False),
    "int16": (KIND_SHORT_COMPLEX, 12, False),
    "int16/dc": (KIND_SHORT_COMPLEX, 12, True),
    "int16planar": (KIND_SHORT, 12, False),
    "int16planar/dc": (KIND_SHORT, 12, True),
    "int8": (KIND_BYTE_COMPLEX, 4, False),
    "int8/dc": (KIND_BYTE_COMPLEX, 4, True),
}
_MIN_LEVELS = np.array([(1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (3, 2), (3, 3)], np.int64)   # p = 1 2 4 5 8 9 10 13 18


def _family(fmt):
    """the count-space constants of a format: background range, offset m, jitter and the largest background count laid out as a
    balancing share"""
    kind, _, dc = FORMATS[fmt]
    if kind == KIND_BYTE_COMPLEX:
        return dict(lo=24, hi=48, m=16 if dc else 0, jitter=2, share_upto=7, wrap_lo=4, wrap_hi=8, int8=True)
    return dict(lo=4096, hi=8192, m=8192 if dc else 0, jitter=50, share_upto=15, wrap_lo=1024, wrap_hi=4096, int8=False)


def max_levels(fmt):
    """int64 [25, 2]: the planted maxima, strongest first"""
    f, dc = _family(fmt), FORMATS[fmt][2]
    l = np.arange(N_MAX_LEVELS, dtype=np.int64)
    if f["int8"]:
        return np.stack([-100 + l, 100 - l // 5], 1) if dc else np.stack([-128 + 2 * l, 127 - l], 1)
    M = 24000 if dc else 32000       # with DC removal the wire carries the value plus 8192
    return np.stack([-M + 300 * l, M - 200 * l], 1)


def min_levels(fmt):
    return _MIN_LEVELS


def level_indices(nb, grid):
    """(max level, min level) of buffer b in a launch whose grid-stride loops step by `grid` or 4 * grid buffers: the pairs a stride or
    indexing error could swap -- b +- 1, b +- 4, b +- grid, b +- 4 grid -- differ in both.  (b % 5, (b // grid) % 5) and
    (b % 3, (b // grid) % 3): 1 and 4 are nonzero modulo 5 and modulo 3, so the first component differs for b +- 1 and b +- 4 and
    the second for b +- grid and b +- 4 grid.)"""
    b = np.arange(nb, dtype=np.int64)
    return b % 5 + 5 * ((b // grid) % 5), b % 3 + 3 * ((b // grid) % 3)


def offset_and_mean(fmt, n):
    """(m, mean): the offset the wire carries and the mean the converter takes out of a buffer whose other values sum to zero --
    int32(uint32(n m) / n), the sum wrapped as utility.cpp:77-78 computes it"""
    m = _family(fmt)["m"]
    return m, ((n * m) & 0xFFFFFFFF) // n


def CLEAR(fmt, n):
    """whether the scene of n samples can hold its margins (module docstring): always without DC removal"""
    return not FORMATS[fmt][2] or n >= 4


_BLOCK = 65536


def _pairs(rng, k, lo, hi):
    """int64 [k, 2] of sum zero: (v, -v) pairs with |re|, |im| in lo ... hi and random signs, shuffled; an odd one out is three
    samples (lo, lo, -2 lo) in each component (2 lo <= hi)"""
    if k == 0:
        return np.zeros((0, 2), np.int64)
    if k == 1:
        return np.array([[lo, -lo]], np.int64)       # (a single background sample cannot sum to zero; only n = 2, 3 get here)
    if k > 3 * _BLOCK:                              # a long buffer: a block of 65536 drawn once and repeated, the rest drawn
        reps = (k - 2) // _BLOCK
        return np.concatenate([np.tile(_pairs(rng, _BLOCK, lo, hi), (reps, 1)), _pairs(rng, k - reps * _BLOCK, lo, hi)])
    h = (k - 3) // 2 if k % 2 else k // 2
    v = rng.integers(lo, hi + 1, (h, 2)) * rng.choice([-1, 1], (h, 2))
    z = np.concatenate([v, -v])
    if k % 2:
        s = rng.choice([-1, 1], 2)
        z = np.concatenate([z, np.array([[lo, lo], [lo, lo], [-2 * lo, -2 * lo]]) * s])
    return rng.permutation(z, axis=0).astype(np.int64)


def _backgrounds(rng, fmt, n, cmax, cmin):
    """int64 [B, k, 2]: the k = n - 2 (n = 1: 0) background samples, in counts as the converter is to leave them, of B buffers whose
    planted values are cmax, cmin [B, 2]"""
    f, dc = _family(fmt), FORMATS[fmt][2]
    B, k = len(cmax), max(0, n - 2)
    m, mean = offset_and_mean(fmt, n)
    centre = m - mean                        # what the converter leaves of the offset: 0, or m where the sum wraps
    if not dc or k == 0:
        return np.broadcast_to(_pairs(rng, k, f["lo"], f["hi"])[None], (B, k, 2)).copy()
    # the buffer's values are to sum to n * centre
    need = n * centre - cmax - cmin                                   # [B, 2]: the background's sum
    if centre:
        z = _pairs(rng, k, f["wrap_lo"], f["wrap_hi"])
    elif k <= f["share_upto"]:
        j = rng.integers(0, f["jitter"] + 1, (k // 2, 2))
        z = np.concatenate([j, -j, np.zeros((k % 2, 2), np.int64)])
    else:
        z = _pairs(rng, k, f["lo"], f["hi"])
    q, r = np.divmod(need, k)                                         # floor share and what is left: 0 <= r < k
    return z[None] + q[:, None, :] + (np.arange(k)[None, :, None] < r[:, None, :])


def _to_wire(fmt, c, n):
    """counts as the converter is to leave them, int64 [B, n, 2] -> the wire array: complex64 [B, n], int16 [B, n, 2], planar
    int16 [B, 2, n], int8 [B, n, 2]"""
    kind, _, dc = FORMATS[fmt]
    if kind == KIND_FLOAT_COMPLEX:
        x = (c / 2048.0).astype(np.float32)
        return np.ascontiguousarray(x).view(np.complex64)[..., 0]
    w = c + offset_and_mean(fmt, n)[1]
    dt = np.int8 if kind == KIND_BYTE_COMPLEX else np.int16
    assert w.min() >= np.iinfo(dt).min and w.max() <= np.iinfo(dt).max, (fmt, int(w.min()), int(w.max()))
    w = w.astype(dt)
    return np.ascontiguousarray(w.transpose(0, 2, 1)) if kind == KIND_SHORT else np.ascontiguousarray(w)


def _assemble(fmt, n, pos_max, pos_min, lmax, lmin, seed):
    """the wire array of B buffers: buffer b holds max level lmax[b] at sample pos_max[b], min level lmin[b] at pos_min[b] and its
    background in the free places, in order"""
    rng = np.random.default_rng([seed, n, sorted(FORMATS).index(fmt)])
    B = len(pos_max)
    cmax, cmin = max_levels(fmt)[lmax], min_levels(fmt)[lmin]
    if FORMATS[fmt][2] and n < 4:
        cmax = np.abs(cmax)      # (nothing balances these buffers: both components positive keeps their sums positive)
    c = np.empty((B, n, 2), np.int32)
    free = np.ones((B, n), bool)
    rows = np.arange(B)
    free[rows, pos_max] = False
    if n > 1:
        assert (pos_max != pos_min).all()
        free[rows, pos_min] = False
        c[rows, pos_min] = cmin
    c[rows, pos_max] = cmax
    c[free] = _backgrounds(rng, fmt, n, cmax, cmin).reshape(-1, 2)
    if FORMATS[fmt][2] and n >= 4:   # the mean the converter takes out is the one the layout assumed
        assert (c.sum(axis=1, dtype=np.int64) == n * (offset_and_mean(fmt, n)[0] - offset_and_mean(fmt, n)[1])).all()
    return _to_wire(fmt, c, n)


def position(fmt, n):
    """(wire array, pos_max [nb], pos_min [nb]) of the position scene: n buffers of n samples, and for an odd n > 1 one more"""
    b = np.arange(n)
    pos_min = n - 1 - b
    if n > 1 and n % 2:      # buffer (n - 1) / 2: the two meet.  Its minimum moves on one sample, and a buffer more has it there
        pos_min = np.concatenate([np.where(pos_min == b, b + 1, pos_min), [n // 2]])
        b = np.concatenate([b, [0]])
    z = np.zeros(len(b), np.int64)
    return _assemble(fmt, n, b, pos_min, z, z, seed=1), b, pos_min


def launch_shape(fmt, n, nb, grid):
    """(wire array, pos_max [nb], pos_min [nb]) of the launch-shape scene: levels by level_indices(nb, grid), positions that walk
    through the buffer with b"""
    assert n >= 4
    b = np.arange(nb)
    pos_max = (7 * b) % n
    pos_min = (pos_max + 1 + b % (n - 1)) % n
    lmax, lmin = level_indices(nb, grid)
    return _assemble(fmt, n, pos_max, pos_min, lmax, lmin, seed=2), pos_max, pos_min


def long_buffers(fmt, n, nb):
    """(wire array, pos_max, pos_min): the maximum in the last sample, the minimum in the one before; levels b, b"""
    b = np.arange(nb)
    return _assemble(fmt, n, np.full(nb, n - 1), np.full(nb, n - 2), b, b, seed=3), np.full(nb, n - 1), np.full(nb, n - 2)


SPECIAL = ["all NaN", "all +inf", "NaN in sample 0", "NaN in the last sample", "one +inf", "one zero and one -0.0", "all 1e-20",
           "one 1e-20 sample", "one power overflows", "one power near FLT_MAX", "plain"]


def special_rows(n):
    """complex64 [11, n], row r as SPECIAL[r] says, on the cfloat background (no planted levels)"""
    assert n >= 8
    rng = np.random.default_rng([4, n])
    bg = (_pairs(rng, n, 4096, 8192) / 2048.0).astype(np.float32)
    x = np.broadcast_to(bg[None], (len(SPECIAL), n, 2)).copy()
    mid = n // 2
    x[0] = np.nan
    x[1, :, 0] = np.inf
    x[2, 0, 1] = np.nan
    x[3, n - 1, 0] = np.nan
    x[4, mid] = (np.inf, 1.0)
    x[5, 1], x[5, mid] = (0.0, 0.0), (-0.0, -0.0)
    x[6] = (1e-20, 0.0)
    x[7, mid] = (0.0, 1e-20)
    x[8, n - 2] = (3e19, 1.0)            # re * re = 9e38 > FLT_MAX
    x[9, 3] = (1.3e19, 1.3e19)           # p = 3.38e38 < FLT_MAX = 3.4028e38
    return np.ascontiguousarray(x).view(np.complex64)[..., 0]


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def convert(oracle_mod, fmt, n, raw):
    """complex64 [B, n]: the wire buffers through the oracle's converter"""
    kind, enob, dc = FORMATS[fmt]
    o = oracle_mod.Oracle(n, kind=kind, enob=enob, correct_dc=dc)
    return np.stack([o.convert(raw[b]) for b in range(len(raw))])


def powers(conv):
    """float32 [B, n]: re * re + im * im, each operation rounded to float (process.cpp:220)"""
    re, im = np.ascontiguousarray(conv.real), np.ascontiguousarray(conv.imag)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return re * re + im * im


def db_of_power(p):
    with np.errstate(divide="ignore"):
        return 5.0 * np.log10(np.asarray(p, np.float64))


def extremes(p):
    """(max_db, min_db) float64 [B] of powers p [B, n] under the reference's comparisons and clamps"""
    p = np.asarray(p, np.float32)
    with np.errstate(invalid="ignore"):
        pmax = np.fmax.reduce(np.where(np.isnan(p), np.float32(-1.0), p), axis=1)                 # NaN is never taken; -1: nothing was
        takes = np.isfinite(p)                                                                    # dB < FLT_MAX: finite p, or 0 (-inf)
        pmin = np.min(np.where(takes, p, np.float32(np.inf)), axis=1)
    mx = np.where(pmax > 0, db_of_power(np.maximum(pmax, 0)), -np.inf)
    mx = np.maximum(mx, FLT_MIN)
    mn = np.where(np.isinf(pmin), FLT_MAX, db_of_power(np.where(np.isinf(pmin), 1.0, pmin)))
    return mx, mn


def reference(oracle_mod, fmt, n, raw):
    """(max_db, min_db, p): the plain reference of the wire buffers `raw`; p float32 [B, n]"""
    p = powers(convert(oracle_mod, fmt, n, raw))
    return (*extremes(p), p)


def second_opinion(oracle_mod, fmt, n, raw, threshold=0.0):
    """(max_db, min_db, above) float32, float32, uint8 [B]: oracle.time_domain, buffer by buffer"""
    kind, enob, dc = FORMATS[fmt]
    o = oracle_mod.Oracle(n, kind=kind, enob=enob, correct_dc=dc)
    r = [o.time_domain(o.convert(raw[b]), threshold=threshold) for b in range(len(raw))]
    return (np.array([t[1] for t in r], np.float32), np.array([t[2] for t in r], np.float32), np.array([t[0] for t in r], np.uint8))


def is_exact(v):
    """the values that compare exactly: +-inf and the two clamp constants"""
    v = np.asarray(v, np.float64)
    return np.isinf(v) | (v == FLT_MIN) | (v == FLT_MAX)


def agree(got, want, bar):
    """largest |got - want| over the finite values, after asserting that +-inf, FLT_MIN and FLT_MAX sit at the same places with
    the same value and that nothing is NaN"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert not np.isnan(got).any() and not np.isnan(want).any()
    ex = is_exact(want) | is_exact(got)
    assert np.array_equal(got[ex], want[ex]), \
        f"+-inf / clamp constants differ at {np.flatnonzero(ex & (got != want))[:8].tolist()}: got {got[ex & (got != want)][:8]}, want {want[ex & (got != want)][:8]}"
    err = np.where(ex, 0.0, np.abs(got - np.where(ex, 0.0, want)))
    worst = int(np.argmax(err)) if err.size else 0
    assert err.max(initial=0.0) <= bar, f"largest error {err.max():.3e} dB > {bar} dB at buffer {worst}: got {got[worst]!r}, want {want[worst]!r}"
    return float(err.max(initial=0.0))


def middle_threshold(max_db):
    """the float32 level in the middle of a launch's maxima: the buffers at that very level are above (process.cpp:226, >=), the
    levels under it are not"""
    return float(np.sort(np.asarray(max_db, np.float32))[len(max_db) // 2])


def margins(p, pos_max, pos_min):
    """(max margin, min margin, lowest background) in dB over the buffers of p [B, n]: how far the planted maximum stands over
    every other sample, how far the planted minimum under, and the smallest dB value of any sample that is not the planted minimum"""
    B, n = p.shape
    if n == 1:
        return np.inf, np.inf, np.inf
    rows = np.arange(B)
    pm, pn = p[rows, pos_max].copy(), p[rows, pos_min].copy()
    q = p.copy()
    q[rows, pos_max] = 0
    up = db_of_power(pm) - db_of_power(q.max(axis=1))
    q[rows, pos_max] = pm
    q[rows, pos_min] = np.inf
    rest = db_of_power(q.min(axis=1))
    return float(up.min()), float((rest - db_of_power(pn)).min()), float(rest.min())
