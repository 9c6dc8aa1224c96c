"""The averaged-plan probe groups of tests/average_probes.py, pinned on the host before any GPU is involved, and the proof that the
model of the group mean SEES the faults tests/test_average_exact_gpu.py exists for.

Asserted:
  * mean_float against fractions.Fraction arithmetic rounded step by step, written out a second time from the kernels' description
    (parts, waves, wave order, division), on every (K, P) shape of the GPU module and a few more;
  * amp_of_power: exact_power(amp_of_power(p)) == p for every partner the GPU module asks for -- the model mean of every flat and
    pair group of every launch and its two neighbouring floats (asserted inside amp_of_power, which this module calls on all of them);
  * member order: the sweeps input is a permutation of the dwell input, member k of group g at buffer g + k G against g K + k;
  * pair groups against numpy's float64 FFT in all four wire formats: even bins a + c, odd bins a - c, exactly; sums exact in any
    partition; the integer mean that correct_dc removes is 0;
  * FAULT SENSITIVITY, per (K, P) shape of the GPU module over the very groups it launches (4 sizes x 2 layouts x (1 + 5) groups = 48
    per small shape; all 11846 groups of the P = 1 shape): the model mean differs in bits, in at least a quarter of the groups, from
    (a) the reciprocal-product mean, (b) a single running sum (P > 1), (c) parts added in plain part order (P > 16), (d) the
    reversed member order, (e) a member dropped / doubled (every member in turn, the worst one counted), (f) every part boundary
    moved by one, up or down.  Left to chance a K = 3 group tells (b) and (d) apart in one draw of five, a K = 5 group (a) in one of
    five (the random-draw figures below), so the generator draws a group again until the model tells ONE form apart, taken in turn
    by group index (average_probes.flat_amplitudes): the quarter is a property of the groups the GPU module runs, asserted here.
    (a) has two controls where the forms agree: K = 64 (a power of two), and K = 130, whose float reciprocal is 2^-30 relative from
    1/130 -- asserted below: at most one group in sixteen differs there, which the GPU module cannot rely on.
    A single boundary moved by one in a P = 65 partition changes few sums (0 ... 34 of 64 random groups, by boundary): not asserted.
  * a distinguishable map: for every flat group mean m of the GPU module (and every pair group's even-bin mean) the correctly rounded
    float32 of 5 log10 at m and at its two neighbouring floats are three different floats;
  * special values: the model gives +inf for three members of 2^126.8, keeps denormal members, and a denormal mean stays denormal.

Random draws without the selection, 4000 groups per shape, share of groups that differ (measured while writing this module):
(a) K = 3: 0.33, K = 5: 0.19, K = 7: 0.53, K = 13: 0.45, K = 130: 0.016; (d) K = 3: 0.20, K = 5: 0.25, K = 7: 0.34, K = 13: 0.44."""
from fractions import Fraction

import numpy as np
import pytest

from tests import average_probes as ap
from tests import db_probes as pr

F32 = np.float32
KINDS = [pr.KIND_FLOAT_COMPLEX, pr.KIND_SHORT_COMPLEX, pr.KIND_SHORT, pr.KIND_BYTE_COMPLEX]
NAMES = {pr.KIND_FLOAT_COMPLEX: "cfloat", pr.KIND_SHORT_COMPLEX: "int16", pr.KIND_SHORT: "int16planar", pr.KIND_BYTE_COMPLEX: "int8"}
SHAPES = list(ap.SMALL_SHAPES) + [(ap.BIG_K, 1)]


def _launches(K, P):
    """the flat groups of every launch of the GPU module at the shape (K, P), with P as a 256-CU device gives it"""
    for n in ap.SIZES:
        for layout in ap.LAYOUTS:
            for G in (ap.SMALL_G if P > 1 else (ap.big_groups(n),)):
                assert ap.parts_of(n, G, K) == P, (n, G, K, P)
                yield n, layout, G, ap.flat_case(n, layout, K, G, P)


# ---- against exact arithmetic ---------------------------------------------------------------------------------------------------
def _fl(fr):
    """the Fraction fr >= 0 rounded to the nearest float32, ties to even, denormals kept (below 2^128: no case here overflows)"""
    if fr == 0:
        return Fraction(0)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    e -= Fraction(2) ** e > fr                  # 2^e <= fr < 2^(e + 1)
    ulp = Fraction(2) ** (max(e, -126) - 23)
    q = fr / ulp
    n = q.numerator // q.denominator
    rem = q - n
    n += rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1)
    out = n * ulp
    assert out < Fraction(2) ** 128 and float(F32(float(out))) == float(out)
    return out


def _mean_fractions(p, K, P):
    """the kernels' mean of the floats p [K] in rational arithmetic, rounded to float32 after every operation"""
    p = [Fraction(float(v)) for v in p]
    if P == 1:
        s = Fraction(0)
        for v in p:
            s = _fl(s + v)
        return _fl(s / K)
    part = []
    for q in range(P):
        s = Fraction(0)
        for k in range(q * K // P, (q + 1) * K // P):
            s = _fl(s + p[k])
        part.append(s)
    W = min(P, 16)
    wave = []
    for x in range(W):
        s, q = Fraction(0), x
        while q < P:
            s = _fl(s + part[q])
            q += W
        wave.append(s)
    s = wave[0]
    for x in range(1, W):
        s = _fl(s + wave[x])
    return _fl(s / K)


@pytest.mark.parametrize("K,P", SHAPES + [(4, 1), (4, 2), (7, 1), (16, 8), (40, 20), (100, 49), (101, 50)])
def test_mean_float_against_fractions(K, P):
    fg = ap.FlatGroups(4, K, P, [7, K, P])
    m = ap.mean_float(fg.power, K, P)
    for g in range(fg.G):
        assert Fraction(float(m[g])) == _mean_fractions(fg.power[g], K, P), (K, P, g)
    if P > 1:   # the partition covers every member once, in order
        b = ap.part_bounds(K, P)
        assert b[0][0] == 0 and b[-1][1] == K and all(b[i][1] == b[i + 1][0] for i in range(P - 1)) and all(hi > lo for lo, hi in b)


def test_partition_classes():
    """what the shapes are there for (scn_avg_combine_kernel: W = min(P, 16) waves, four loads in flight while q + 3 W < P)"""
    assert [hi - lo for lo, hi in ap.part_bounds(7, 4)] == [1, 2, 2, 2]                       # ragged parts
    assert list(range(0, 17, 16)) == [0, 16]                                                   # P = 17: wave 0 adds parts 0 and 16
    for x in range(16):                                                                        # P = 65: every wave runs the loop once,
        q = x
        assert q + 48 < 65                                                                     # (parts x, x + 16, x + 32, x + 48)
        assert (q + 64 < 65) == (x == 0)                                                       # and wave 0 alone the tail (part 64)
    assert not 0 + 48 < 32 and 0 + 48 < 49                                                     # the loop first runs at P = 49
    for n in ap.SIZES:
        assert ap.parts_of(n, ap.big_groups(n), ap.BIG_K) == 1 and ap.big_groups(n) > 256 * ap.WG_PER_CU[n]
        for K, P in ap.SMALL_SHAPES:
            assert all(ap.parts_of(n, G, K) == P == (K + 1) // 2 for G in ap.SMALL_G)
    assert [ap.big_groups(n) - 5 for n in ap.SIZES] == [3072, 1536, 768, 512]


def test_amp_of_power_reaches_every_partner():
    rng = np.random.default_rng(3)
    p = np.concatenate([rng.uniform(0.4, 2.5, 300), np.exp2(rng.uniform(-125.0, 120.0, 300))]).astype(F32)
    assert np.array_equal(pr.exact_power(ap.amp_of_power(p)), p)
    count = 0
    for K, P in SHAPES:
        for n, layout, G, fg in _launches(K, P):
            m = fg.means(P)
            lo, hi = ap.neighbours(m)
            ap.amp_of_power(np.concatenate([lo, m, hi]))   # (asserts exact_power(...) == p itself)
            count += 3 * G
    for kind in KINDS:
        for K in (3, 5, 7):
            for dc in (0, 1):
                m = ap.pair_case(kind, 1024, K, 5, dc).means()
                for v in m.values():
                    lo, hi = ap.neighbours(v)
                    ap.amp_of_power(np.concatenate([lo, v, hi]))
    assert count == 3 * (7 * 48 + 2 * sum(ap.big_groups(n) for n in ap.SIZES))


# ---- member order ---------------------------------------------------------------------------------------------------------------
def test_member_order():
    G, K = 5, 7
    x = np.arange(G * K * 3).reshape(G, K, 3)
    d, s = ap.arrange(x, ap.AVG_DWELL), ap.arrange(x, ap.AVG_SWEEPS)
    assert np.array_equal(d, x.reshape(G * K, 3))
    for g in range(G):
        for k in range(K):
            assert np.array_equal(d[g * K + k], x[g, k]) and np.array_equal(s[g + k * G], x[g, k])
    perm = np.array([g * K + k for k in range(K) for g in range(G)])   # (tests/test_average_gpu.py: sweeps position g + k G holds dwell buffer g K + k)
    assert np.array_equal(s, d[perm]) and sorted(perm.tolist()) == list(range(G * K))
    assert np.array_equal(ap.first_buffer(G, K, ap.AVG_DWELL), np.arange(G) * K) and np.array_equal(ap.first_buffer(G, K, ap.AVG_SWEEPS), np.arange(G))


# ---- pair groups ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=[NAMES[k] for k in KINDS])
def test_pair_groups_against_float64(kind):
    n, G, K = 1024, 5, 7
    pg = ap.pair_case(kind, n, K, G, 1)
    raw = pg.raw(n, ap.AVG_DWELL)
    if kind == pr.KIND_FLOAT_COMPLEX:
        x = raw.astype(np.complex128)
    elif kind == pr.KIND_SHORT:
        assert raw.shape == (G * K, 2, n) and raw.dtype == np.int16
        x = (raw[:, 0].astype(np.float64) + 1j * raw[:, 1]) * ap.pair_scale(kind)
    else:
        assert raw.shape == (G * K, n, 2)
        x = (raw[..., 0].astype(np.float64) + 1j * raw[..., 1]) * ap.pair_scale(kind)
        isum = raw[..., 0].astype(np.int64).sum(axis=1)
        assert (isum > 0).all() and (isum // n == 0).all(), "the integer mean that correct_dc removes is 0"
    X = np.fft.fft(x, axis=1)
    P = (X.real ** 2 + X.imag ** 2).reshape(G, K, n)
    assert np.abs(P[:, :, 0::2] - pg.power["even"].astype(np.float64)[:, :, None]).max() <= 1e-12 * pg.power["even"].max()
    assert np.abs(P[:, :, 1::2] - pg.power["odd"].astype(np.float64)[:, :, None]).max() <= 1e-12 * pg.power["even"].max()
    one = pg.means(1)
    for parts in (2, 3, 4):
        assert all(pg.means(parts)[k].tobytes() == one[k].tobytes() for k in one), "exact sums: any partition gives one float"
    for k in one:   # one rounding: the division of the exact sum
        S = pg.power[k].astype(np.float64).sum(axis=1)
        assert np.array_equal(one[k], (S.astype(F32) / F32(K)).astype(F32))
    assert ap.in_ranges(one["even"]).all(), "the even bins' mean lies where the map tells neighbouring floats apart"
    sw = pg.raw(n, ap.AVG_SWEEPS)
    assert np.array_equal(sw[ap.member_buffers(G, K, ap.AVG_SWEEPS).reshape(-1)], raw)
    for bad in (dict(lo=1100, hi=1200), ):   # the preconditions are asserted, not hoped for
        old = ap.PAIR[kind]
        ap.PAIR[kind] = (old[0], (bad["lo"], bad["hi"]), old[2])
        try:
            with pytest.raises(AssertionError):
                ap.PairGroups(kind, G, K, 1)
        finally:
            ap.PAIR[kind] = old


# ---- the model sees the faults --------------------------------------------------------------------------------------------------
def _shifted(K, P, d):
    cut = [0] + [min(max(hi + d, 0), K) for _, hi in ap.part_bounds(K, P)[:-1]] + [K]
    return [(cut[i], cut[i + 1]) for i in range(P)]


@pytest.mark.parametrize("K,P", SHAPES)
def test_fault_sensitivity(K, P):
    differ, total = {}, 0
    kf = F32(K)
    for n, layout, G, fg in _launches(K, P):
        m = fg.means(P)
        assert ap.in_ranges(m).all()
        forms = ap.faulty_means(fg.power, K, P)
        if P > 1:
            for d in (-1, 1):
                forms[f"boundaries {d:+d}"] = (ap.group_sum(fg.power, K, P, bounds=_shifted(K, P, d)) / kf).astype(F32)
        if not ap.reciprocal_differs(K):
            forms["(control) reciprocal"] = (ap.group_sum(fg.power, K, P) * (F32(1.0) / kf)).astype(F32)
        # a member dropped / doubled, as a wrong boundary or a wrong buffer index would: the member it matters least for
        for k in sorted({0, K // 2, K - 1}):
            for name, mult in (("dropped", 0.0), ("doubled", 2.0)):
                p = fg.power.copy()
                p[:, k] *= F32(mult)
                f = ap.mean_float(p, K, P)
                differ[f"member {k} {name}"] = differ.get(f"member {k} {name}", 0) + int((f.view(np.uint32) != m.view(np.uint32)).sum())
        for name, f in forms.items():
            differ[name] = differ.get(name, 0) + int((f.view(np.uint32) != m.view(np.uint32)).sum())
        total += G
    print(f"K={K} P={P}: {total} groups; differing: {differ}")
    assert total == (48 if P > 1 else sum(ap.big_groups(n) for n in ap.SIZES) * 2)
    want = {"reversed"} | ({"reciprocal"} if ap.reciprocal_differs(K) else set()) | ({"single", "boundaries -1", "boundaries +1"} if P > 1 else set()) \
        | ({"plain"} if P > 16 else set())
    assert want <= set(differ), (want, set(differ))
    for name, cnt in differ.items():
        if name.startswith("(control)"):
            assert 16 * cnt <= total, f"K={K}: the reciprocal product is expected to agree with the division here ({cnt} of {total} differ)"
        else:
            assert 4 * cnt >= total, f"K={K} P={P}: the model tells '{name}' apart in {cnt} of {total} groups only"


def test_reciprocal_controls():
    assert [K for K in (3, 5, 7, 13, 33, 64, 130) if not ap.reciprocal_differs(K)] == [64, 130]
    assert F32(1.0) / F32(64) == 2.0 ** -6
    assert abs(float(F32(1.0) / F32(130)) * 130 - 1.0) < 2.0 ** -29
    rng = np.random.default_rng(1)
    S = rng.uniform(1.0, 2.0, 200000).astype(F32)
    for K in (3, 5, 7, 13, 33):
        ulps = np.abs((S * (F32(1.0) / F32(K))).view(np.int32).astype(np.int64) - (S / F32(K)).view(np.int32).astype(np.int64))
        assert ulps.max() == 1 and (ulps == 1).mean() > 0.15, K


# ---- a distinguishable map ------------------------------------------------------------------------------------------------------
def _three_floats(m):
    lo, hi = ap.neighbours(m)
    d = [pr.db64(v).astype(F32) for v in (lo, m, hi)]
    return (d[0] < d[1]) & (d[1] < d[2])


def test_the_ideal_map_tells_neighbouring_means_apart():
    rng = np.random.default_rng(9)
    draw = np.concatenate([rng.uniform(*r, 150) for r in ap.MEAN_RANGES]).astype(F32)
    assert _three_floats(draw).all()
    for K, P in SHAPES:
        for n, layout, G, fg in _launches(K, P):
            m = fg.means(P)
            assert ap.in_ranges(m).all() and _three_floats(m).all(), (K, P, n, layout)
            d = np.abs(pr.db64(m))
            assert d.min() >= 0.24 and d.max() <= 1.51
    for kind in KINDS:
        for K in (3, 5, 7):
            m = ap.pair_case(kind, 1024, K, 5, 0).means()["even"]
            assert ap.in_ranges(m).all() and _three_floats(m).all(), (kind, K)


# ---- special values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,P", [(3, 1), (7, 4)])
def test_special_members_in_the_model(K, P):
    base = ap.FlatGroups(1, K, P, [11, K]).amps[0]
    tiny = np.finfo(F32).tiny
    for k in sorted({0, K // 2, K - 1}):
        for name in ap.SPECIALS:
            row = ap.special_row(base, name, k)
            p = ap.powers(row)
            m = ap.mean_float(p[None, :], K, P)[0]
            if name in ("nan_re", "nan_im"):
                assert np.isnan(p[k]) and np.isnan(m) and np.isfinite(np.delete(p, k)).all()
            elif name == "big":
                assert np.isposinf(p[k]) and np.isposinf(m)
            elif name == "zero":
                assert (p == 0).all() and m == 0
            elif name == "overflow":
                assert np.isfinite(p).all() and (p > 2.0 ** 126.5).sum() == 3 and np.isposinf(m), "three members of 2^126.8, none special on its own"
                assert np.isposinf(ap.mean_float(p[None, :], K, 1)[0]), "on both epilogues alike"
            elif name == "den_mean":
                assert p[k] == F32(1.5 * 2.0 ** -126) and (np.delete(p, k) == 0).all() and 0 < m < tiny
            elif name == "den_members":
                den = (p > 0) & (p < tiny)
                assert den.sum() == K - 1 and not den[k] and p[k] >= tiny and m >= tiny, "denormal members, one normal one, a normal mean"
                flushed = np.where(den, F32(0), p)
                assert ap.mean_float(flushed[None, :], K, P)[0] != m, "a kernel that flushed denormal powers would report another float"
                assert Fraction(float(m)) == _mean_fractions(p, K, P), "denormals kept, as IEEE arithmetic keeps them"


def test_documents_name_this_suite():
    import os

    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for doc in ("README.md", os.path.join("profiles", "README.md")):   # (DESIGN.md is within two bytes of its 40 KB limit)
        assert "test_average_exact_gpu.py" in open(os.path.join(root, doc)).read(), doc
    assert os.path.exists(os.path.join(here, "test_average_exact_gpu.py")) and os.path.exists(os.path.join(root, "profiles", "average_exact.md"))
