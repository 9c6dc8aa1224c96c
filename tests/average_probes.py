"""Averaged-plan groups whose every bin power is known EXACTLY, shared by tests/test_average_probes_cpu.py (which pins this
generator and shows that the model sees the faults it is there for) and tests/test_average_exact_gpu.py (which holds the group mean
of scn_average.hip to the bit on them).  Built on tests/db_probes.py; rectangular window, DC removal off unless stated.

* Flat group: member b of group g is a_{g,b} * delta[n] in cfloat (db_probes' flat probe): every bin of the member holds the exact
  power db_probes.exact_power(a).  The amplitudes are real float32 with full mantissas spread over six binades of power inside a
  group, so every addition of the group's sum rounds; each group is scaled by a power of two (exact) so that its mean lands in
  [0.5, 0.89] or [1.12, 2.0], where one ulp of the mean is several ulps of 5 log10(mean) and the map's region around 1.0 (where an
  ulp of the value vanishes) is avoided.
* Pair group, all four wire formats: member b is a * delta[n] + c * delta[n - N/2] with small positive integer quanta: even bins
  hold a + c, odd bins a - c.  WHY THE TRANSFORM IS EXACT (the argument of tests/welch_probes.py, for scn_avg_power_kernel): a
  thread t owns samples T a' + t, a' = 0 .. 15, T = N / 16; samples 0 and N/2 = 8 T are thread 0's fft16 inputs 0 and 8.  They
  meet the +-1 paths of the radix-4 steps only, thread 0's pass-1 twiddles are W^0, the later passes add exact zeros under W^0
  twiddles.  At 8192 points (two 4096-point halves of the even and the odd samples) sample N/2 = 4096 is even: it is sample 2048 =
  8 * 256 of the even half, again input 8 of thread 0; the odd half is all zeros and the radix-2 step in double adds W * 0.  The
  powers are integers under 2^24 quanta^2 and so is K times the largest: the group's sum is exact in ANY order and only the
  division rounds.  With correct_dc = 1 the integer mean (a + c) / N is 0 (a + c < 1024): the bytes must equal the correct_dc = 0 run.

THE FLOAT THE MAP IS APPLIED TO (mean_float), restated from scanner_amd/csrc/scn_average.hip:
  * a work item is (group, part q); AvgCursor::start_item gives it the members k = q K / P .. (q + 1) K / P - 1 (integer division),
    buffer() maps member k of group g to buffer g K + k (SCN_AVG_DWELL) or g + k G (SCN_AVG_SWEEPS);
  * scn_avg_power_kernel starts every item from `acc[o] = 0.0f` and adds member by member, `acc[o] = acc[o] + power_of(...)`;
  * P == 1: the item is the group, `const float q = acc[16 * hh + o] / kf;` with kf = (float)args.k -- a float division;
  * P > 1: scn_avg_combine_kernel runs W = min(P, 16) waves (scn_launch_average: `waves = a.parts < 16u ? a.parts : 16u`); wave x
    adds parts x, x + W, x + 2 W, ... to `float s = 0.0f` in that order (the four-loads-in-flight loop and its tail add in the same
    order); wave 0 then forms `s = part_sum[0][lane]; s = s + part_sum[x][lane]` for x = 1 .. W - 1, and
    `const float p = s / (float)args.k;`.
Denormals are kept as numpy keeps them, an overflowing sum is +inf, NaN propagates."""
import numpy as np

from tests import db_probes as pr

F32 = np.float32
AVG_DWELL, AVG_SWEEPS = 0, 1   # SCN_AVG_* (scanner_hip.h)
WG_PER_CU = {1024: 12, 2048: 6, 4096: 3, 8192: 2}   # resident workgroups per CU of scn_avg_power_kernel (AvgGeo::WG_PER_CU)
MEAN_RANGES = ((0.5, 0.89), (1.12, 2.0))


# ---- the partition and the model ------------------------------------------------------------------------------------------------
def parts_of(n, G, K, cus=256):
    """scn_avg_parts restated: the parts a group of K buffers is split into in a submit of G groups on a device of `cus` CUs"""
    slots = cus * WG_PER_CU[n]
    if K <= 1 or G >= slots:
        return 1
    return min(-(-slots // G), (K + 1) // 2)


def part_bounds(K, parts):
    """[(first member, end)] of every part"""
    return [((q * K) // parts, ((q + 1) * K) // parts) for q in range(parts)]


def _running(p, members):
    acc = np.zeros(p.shape[:-1], F32)
    for k in members:
        acc = (acc + p[..., k]).astype(F32)
    return acc


def _combine(sums, waves):
    """the part sums added as the combine kernel adds them with `waves` waves (waves = 1: plain part order)"""
    per_wave = [_running(np.stack(sums, axis=-1), range(x, len(sums), waves)) for x in range(waves)]
    total = per_wave[0]
    for s in per_wave[1:]:
        total = (total + s).astype(F32)
    return total


def group_sum(powers, K, parts, bounds=None, waves=None):
    """float32: the sum of the float powers [..., K] (member axis last, member order) as the kernels form it.  `bounds` and `waves`
    replace the partition and the combine kernel's wave count: the faults tests/test_average_probes_cpu.py asks the model to see."""
    p = np.asarray(powers, F32)
    assert p.shape[-1] == K and 1 <= parts <= max(K, 1)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if parts == 1 and bounds is None:
            return _running(p, range(K))
        sums = [_running(p, range(lo, hi)) for lo, hi in (bounds or part_bounds(K, parts))]
        return _combine(sums, waves or min(len(sums), 16))


def mean_float(powers, K, parts):
    """float32: the mean of the float powers [..., K] as the kernels form it -- see the module docstring"""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return (group_sum(powers, K, parts) / F32(K)).astype(F32)


# ---- member order ---------------------------------------------------------------------------------------------------------------
def member_buffers(G, K, layout):
    """int64 [G, K]: the submit's buffer index of member k of group g"""
    g, k = np.arange(G, dtype=np.int64)[:, None], np.arange(K, dtype=np.int64)[None, :]
    return g + k * G if layout == AVG_SWEEPS else g * K + k


def arrange(members, layout):
    """members [G, K, ...] -> the submit's buffers [G K, ...] in the layout's order (the sweeps input is a permutation of the dwell one)"""
    members = np.asarray(members)
    G, K = members.shape[:2]
    out = np.empty((G * K,) + members.shape[2:], members.dtype)
    out[member_buffers(G, K, layout).reshape(-1)] = members.reshape((G * K,) + members.shape[2:])
    return out


def first_buffer(G, K, layout):
    """int64 [G]: the buffer whose seq_id a group's records carry"""
    return member_buffers(G, K, layout)[:, 0]


# ---- amplitudes of a prescribed power -------------------------------------------------------------------------------------------
def amp_of_power(p):
    """complex64 [...]: amplitudes whose flat probes hold exactly the (normal, finite, positive) float powers p.  As
    db_probes.power_ladder: x = the 12-bit float just under 0.98 sqrt(p) (x * x is exact), y aimed at the middle of p's rounding
    interval and nudged by a few ulps until the correctly rounded x^2 + y^2 is p, clear of a rounding boundary."""
    p = np.asarray(p, F32)
    flat = p.reshape(-1)
    assert (np.isfinite(flat) & (flat >= np.finfo(F32).tiny)).all(), "amp_of_power: normal finite powers only"
    p64 = flat.astype(np.float64)
    e = np.exp2(np.floor(np.log2(np.sqrt(p64))))
    x = (np.floor(np.sqrt(p64) * 0.98 / e * 2048.0) / 2048.0 * e).astype(F32)
    x64 = x.astype(np.float64)
    y0 = np.sqrt(p64 - x64 * x64).astype(F32)
    y, found = y0.copy(), np.zeros(flat.shape, bool)
    ulp = np.spacing(flat).astype(np.float64)
    for step in (0, 1, -1, 2, -2, 3, -3, 4, -4, 5, -5, 6, -6):
        c = y0.copy()
        for _ in range(abs(step)):
            c = np.nextafter(c, F32(np.inf if step > 0 else 0))
        s = x64 * x64 + c.astype(np.float64) ** 2          # (a double rounds this at 2^-29 ulp of p: a screen, verified below)
        ok = ~found & (s.astype(F32) == flat) & (np.abs(s - p64) < 0.45 * ulp)
        y[ok], found = c[ok], found | ok
    assert found.all(), f"amp_of_power: no amplitude for {flat[~found][:4].tolist()}"
    amps = (x.astype(np.complex64) + 1j * y.astype(np.complex64)).astype(np.complex64)
    assert np.array_equal(pr.exact_power(amps), flat), "amp_of_power misses a power"
    return amps.reshape(p.shape)


def neighbours(m):
    """(the float below, the float above) of every float in m"""
    m = np.asarray(m, F32)
    return np.nextafter(m, F32(-np.inf)), np.nextafter(m, F32(np.inf))


# ---- flat groups ----------------------------------------------------------------------------------------------------------------
def in_ranges(m):
    m = np.asarray(m)
    return ((m >= MEAN_RANGES[0][0]) & (m <= MEAN_RANGES[0][1])) | ((m >= MEAN_RANGES[1][0]) & (m <= MEAN_RANGES[1][1]))


def reciprocal_differs(K):
    """whether the float 1 / K is far enough from 1 / K (2^-28 relative: a thirtieth of an ulp) for the reciprocal-product mean to differ from the
    division in a fair share of sums.  False for the powers of two (exact) and for K = 130: 1/65 = 0.000000111111 000000111111 ...
    in binary, the float of 1/130 is 2^-30 relative from it, and the two forms agree in all but one sum in 64."""
    r = float(F32(1.0) / F32(K))
    return abs(r * K - 1.0) > 2.0 ** -28


def faulty_means(powers, K, parts):
    """{name: float32 [...]}: the mean under the faults this module exists for, where the shape has that fault at all --
    "reciprocal": sum * (1.0f / K); "single": one running sum where the kernels add parts; "plain": the parts added in plain part
    order where the combine kernel's 16 waves interleave them; "reversed": the members in reverse order"""
    p = np.asarray(powers, F32)
    k = F32(K)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        out = {"reversed": mean_float(p[..., ::-1], K, parts)}
        if reciprocal_differs(K):
            out["reciprocal"] = (group_sum(p, K, parts) * (F32(1.0) / k)).astype(F32)
        if parts > 1:
            out["single"] = (group_sum(p, K, 1) / k).astype(F32)
        if parts > 16:
            out["plain"] = (group_sum(p, K, parts, waves=1) / k).astype(F32)
    return out


SELECT = ("reciprocal", "reversed", "single")


def flat_amplitudes(G, K, parts, seed):
    """float32 [G, K]: real amplitudes with full mantissas, the powers of a group spread over six binades, every group scaled by a
    power of two so that its mean (any partition: they differ by ulps) lies well inside MEAN_RANGES; a draw that lands in the gap
    around 1.0 is drawn again.  A draw is also drawn again unless the model mean under `parts` differs in bits from ONE faulty
    form, taken in turn by group index from SELECT (a form the shape does not have: the reversed order instead): left to chance a
    K = 3 group tells the reversed order apart in one draw of five, a K = 5 group the reciprocal product in one of five."""
    a = np.zeros((G, K), F32)
    todo = np.ones(G, bool)
    turn = (np.arange(G) + int(np.sum(np.atleast_1d(seed)))) % len(SELECT)
    for attempt in range(2000):
        if not todo.any():
            break
        rng = np.random.default_rng(list(np.atleast_1d(seed)) + [G, K, parts, attempt])
        c = (np.exp2(rng.uniform(-3.0, 0.0, (G, K))) * rng.choice([-1.0, 1.0], (G, K))).astype(F32)
        p = pr.exact_power(c.astype(np.complex64).reshape(-1)).reshape(G, K)
        m = mean_float(p, K, parts)
        shift = np.ceil((-1.0 - np.log2(m.astype(np.float64))) / 2.0)          # m 4^shift in [0.5, 2)
        ms = m.astype(np.float64) * np.exp2(2.0 * shift)
        faulty = faulty_means(p, K, parts)
        seen = np.zeros(G, bool)
        for i, name in enumerate(SELECT):
            f = faulty.get(name, faulty["reversed"])
            seen |= (turn == i) & (f.view(np.uint32) != m.view(np.uint32))
        if attempt >= 100:   # (a shape on which the form in turn cannot differ, as the reversed order at K = 4, P = 2: any other form)
            for f in faulty.values():
                seen |= f.view(np.uint32) != m.view(np.uint32)
        ok = todo & seen & (((ms >= 0.52) & (ms <= 0.87)) | ((ms >= 1.15) & (ms <= 1.95)))
        a[ok] = (c[ok] * np.exp2(shift[ok])[:, None]).astype(F32)
        todo &= ~ok
    assert not todo.any(), "no admissible draw"
    return a


def powers(amps):
    """float32, the shape of amps: db_probes.exact_power, with NaN where an amplitude holds a NaN"""
    a = np.asarray(amps).astype(np.complex64)
    flat = a.reshape(-1)
    bad = np.isnan(flat.real) | np.isnan(flat.imag)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        p = pr.exact_power(np.where(bad, np.complex64(0), flat))
    p[bad] = np.nan
    return p.reshape(a.shape)


class FlatGroups:
    """G flat groups of K members: amps [G, K] (float32, or complex64 when given), power float32 [G, K] (exact), and what every
    partition owes.  parts: the partition the draw is selected for (flat_amplitudes); amps: given amplitudes instead of a draw"""

    def __init__(self, G, K, parts=1, seed=0, amps=None):
        self.G, self.K = G, K
        self.amps = flat_amplitudes(G, K, parts, seed) if amps is None else np.asarray(amps, np.complex64 if np.iscomplexobj(amps) else F32)
        assert self.amps.shape == (G, K)
        self.power = powers(self.amps)

    def means(self, parts):
        return mean_float(self.power, self.K, parts)

    def raw(self, n, layout):
        """complex64 [G K, n] in the layout's buffer order"""
        return arrange(pr.flat_raw(n, self.amps.reshape(-1)).reshape(self.G, self.K, n), layout)


# ---- pair groups ----------------------------------------------------------------------------------------------------------------
# (ENOB, range of a + c in quanta, cap of (a - c) / 2): the even bins' mean (a + c)^2 scale^2 lands in MEAN_RANGES
PAIR = {pr.KIND_FLOAT_COMPLEX: (None, (730, 960), 300), pr.KIND_SHORT_COMPLEX: (11, (730, 960), 300), pr.KIND_SHORT: (11, (730, 960), 300),
        pr.KIND_BYTE_COMPLEX: (8, (137, 180), 30)}
PAIR_CFLOAT_SHIFT = 2.0 ** -4   # db_probes.pack writes cfloat quanta of 2^-6: times this, the scale of ENOB 11


def pair_enob(kind):
    return 12 if kind == pr.KIND_FLOAT_COMPLEX else PAIR[kind][0]


def pair_scale(kind):
    return pr.CFLOAT_QUANTUM * PAIR_CFLOAT_SHIFT if kind == pr.KIND_FLOAT_COMPLEX else 2.0 ** -(PAIR[kind][0] - 1)


class PairGroups:
    """G pair groups of K members in one wire format: ia, ic int64 [G, K] (quanta, positive, a > c), power {"even", "odd"} float32
    [G, K] (exact, and exact as sums)"""

    def __init__(self, kind, G, K, seed):
        _, (lo, hi), dmax = PAIR[kind]
        rng = np.random.default_rng(list(np.atleast_1d(seed)) + [kind, G, K])
        q = rng.integers(lo, hi + 1, (G, K))
        d = rng.integers(1, dmax + 1, (G, K))
        self.kind, self.G, self.K = kind, G, K
        self.ia, self.ic = (q + 1) // 2 + d, q - (q + 1) // 2 - d
        ev, od = self.ia + self.ic, self.ia - self.ic
        assert (self.ic > 0).all() and (od > 0).all() and ev.max() < 1024, "positive amplitudes whose integer mean is 0 from 1024 points up"
        assert K * int((ev * ev).max()) < 1 << 24, "K times the largest power reaches 2^24 quanta^2"
        if kind != pr.KIND_FLOAT_COMPLEX:
            assert self.ia.max() <= pr.INT_MAX[kind]
        s2 = pair_scale(kind) ** 2
        self.power = {"even": (ev * ev * s2).astype(F32), "odd": (od * od * s2).astype(F32)}
        for name, v in (("even", ev), ("odd", od)):   # exact as rationals, and exact as sums
            assert np.array_equal(self.power[name].astype(np.float64), v * v * s2)
            assert np.array_equal(self.power[name].astype(np.float64).sum(axis=1).astype(F32).astype(np.float64), (v * v).sum(axis=1) * s2)

    def means(self, parts=1):
        """{"even", "odd"} -> float32 [G]: one rounding, the division's (the sums are exact in any order)"""
        return {k: mean_float(p, self.K, parts) for k, p in self.power.items()}

    def raw(self, n, layout):
        """the wire format's raw array [G K, ...] in the layout's buffer order"""
        q = np.zeros((self.G * self.K, n, 2), np.int64)
        q[:, 0, 0], q[:, n // 2, 0] = self.ia.reshape(-1), self.ic.reshape(-1)
        x = pr.pack(self.kind, q)
        if self.kind == pr.KIND_FLOAT_COMPLEX:
            x = (x * F32(PAIR_CFLOAT_SHIFT)).astype(np.complex64)
        return arrange(x.reshape((self.G, self.K) + x.shape[1:]), layout)


# ---- the shapes tests/test_average_exact_gpu.py runs (tests/test_average_probes_cpu.py shows the model sensitive at each) -------
SIZES = (1024, 2048, 4096, 8192)
LAYOUTS = (AVG_DWELL, AVG_SWEEPS)
SMALL_G = (1, 5)
# (K, P on a 256-CU device): with G <= 5 the cap P = (K + 1) // 2 decides at every size
SMALL_SHAPES = ((3, 2), (5, 3), (7, 4), (13, 7), (33, 17), (64, 32), (130, 65))
BIG_K = 3   # the P = 1 shape: G = slots + 5 groups of three, two items on some persistent workgroups


def big_groups(n, cus=256):
    return cus * WG_PER_CU[n] + 5


def flat_case(n, layout, K, G, parts):
    """the flat groups of one launch of the GPU module (a seed of its own per launch), drawn for the partition `parts`"""
    return FlatGroups(G, K, parts, [20260, n, layout])


def pair_case(kind, n, K, G, dc):
    """the pair groups of one launch of the GPU module"""
    return PairGroups(kind, G, K, [20261, n, dc])


# ---- special values -------------------------------------------------------------------------------------------------------------
SPECIALS = ("nan_re", "nan_im", "big", "zero", "overflow", "den_mean", "den_members")


def special_row(base, name, k):
    """complex64 [K]: the amplitudes of a group whose ordinary members are `base` [K], with the special value `name` at member k
    (the whole group for "zero", "overflow", "den_mean" and "den_members", where k is the member that differs from the rest)"""
    K = len(base)
    row = np.asarray(base).astype(np.complex64)
    if name == "nan_re":
        row[k] = np.nan
    elif name == "nan_im":
        row[k] = complex(1.0, np.nan)
    elif name == "big":
        row[k] = 2.0 ** 64                                       # P_b = +inf on its own
    elif name == "zero":
        row[:] = 0.0
    elif name == "overflow":                                     # three finite members of about 2^126.8 each: the SUM overflows
        for j, f in zip(sorted({0, K // 2, K - 1}) if K > 3 else (0, 1, 2), (1.0, -1.01, 0.99)):
            row[j] = F32(f * 2.0 ** 63.4)
    elif name == "den_mean":                                     # one normal member, a denormal mean
        row[:] = 0.0
        row[k] = amp_of_power(F32(1.5 * 2.0 ** -126))
    elif name == "den_members":                                  # denormal powers of 2^-128 ... 0.81 * 2^-126 around one normal member
        row[:] = (2.0 ** -64 * (1.0 + 0.8 * ((np.arange(K) * 0.6180339887) % 1.0))).astype(F32)
        row[k] = F32(1.2345 * 2.0 ** -61)
    else:
        raise KeyError(name)
    return row
