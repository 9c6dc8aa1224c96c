"""Probe inputs whose bin powers are known EXACTLY (rectangular window, DC removal off), shared by tests/test_db_probes_cpu.py
(which pins this generator against float64 mathematics and the oracle) and tests/test_db_map_gpu.py (which holds the device's dB
map and hit decision to the bit on them).

* Flat probe: buffer b is a_b * delta[n].  The only nonzero datum of every pass of every FFT decomposition sits at index 0 of the
  remaining dimensions, its twiddle is W^0 = (1, 0), and the butterflies add exact zeros to it: every bin equals a_b, and its power
  is the float re*re (+ im*im).  A REAL a_b may be any float: P = fl(a^2), one float multiply however the kernel forms it.  A COMPLEX
  a_b = (x, y) is admitted where x has at most 12 significant bits (x*x is then exact) and x^2 + y^2 is not within 2^-20 ulp of a
  rounding boundary: fma(y, y, x*x) in float and (float)(x*x + y*y) in double then give the same float, the correctly rounded sum.
  Real probes cannot reach every float power (fl(a^2) skips more than half of them, SCN_P_EXACT_FROM among them); complex ones can.
* Line probe: x[n] = A1 i^n + A3 i^(3n) + a delta[n] with A1, A3, a small integers times one power of two (the wire format's
  scale).  The samples are (+-(A1 + A3), 0) and (0, +-(A1 - A3)); the spectrum holds exactly N A1 + a at bin N/4, N A3 + a at bin
  3N/4 and a everywhere else, as long as N A + a stays below 2^24 quanta."""
from fractions import Fraction

import numpy as np

F32 = np.float32
KIND_BYTE_COMPLEX, KIND_SHORT, KIND_SHORT_COMPLEX, KIND_FLOAT_COMPLEX = 1, 2, 3, 4   # SCN_KIND_* (scanner_hip.h)
# (wire format, ENOB): the integer scale is 2^-(ENOB - 1) (utility.cpp:64-65); chosen so that a 16-point line still reaches 16 dB
ENOB = {KIND_FLOAT_COMPLEX: 12, KIND_SHORT_COMPLEX: 12, KIND_SHORT: 10, KIND_BYTE_COMPLEX: 4}
INT_MAX = {KIND_SHORT_COMPLEX: 32767, KIND_SHORT: 32767, KIND_BYTE_COMPLEX: 127}
CFLOAT_QUANTUM = 2.0 ** -6   # the float probes' "scale": line probes in cfloat are integers times this


def scale_of(kind):
    return CFLOAT_QUANTUM if kind == KIND_FLOAT_COMPLEX else 2.0 ** -(ENOB[kind] - 1)


# ---- exact float powers ---------------------------------------------------------------------------------------------------------
def _round_f32(fr):
    """the float nearest to the Fraction fr (> 0, normal range), and its distance to the nearer rounding boundary in ulp"""
    c = F32(float(fr))
    best = min((np.nextafter(c, F32(0)), c, np.nextafter(c, F32(np.inf))), key=lambda f: abs(Fraction(float(f)) - fr))
    ulp = Fraction(float(np.spacing(best)))
    return best, float(Fraction(1, 2) - abs(Fraction(float(best)) - fr) / ulp)


def exact_power(amps):
    """float32 [B]: the power of every bin of the flat probes of complex64 amplitudes `amps`, as every kernel forms it."""
    amps = np.asarray(amps, np.complex64)
    re, im = amps.real.astype(F32), amps.imag.astype(F32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        p = re * re   # numpy's float32 product: correctly rounded, denormal results kept
    for b in np.flatnonzero(im != 0):
        m = abs(int(np.frexp(re[b])[0] * (1 << 24)))
        assert m % (1 << 12) == 0, "a complex flat probe needs a real part of at most 12 significant bits"
        p[b], margin = _round_f32(Fraction(float(re[b])) ** 2 + Fraction(float(im[b])) ** 2)
        assert margin > 2.0 ** -20, "x^2 + y^2 sits on a rounding boundary"
    return p


def power_ladder(centre, below, above):
    """complex64 amplitudes whose exact powers are the `below` floats under `centre`, centre itself and the `above` floats over it,
    in order: x = the 12-bit float just under sqrt(centre) * 0.98, y aimed at the middle of each power's rounding interval."""
    centre = F32(centre)
    e = 2.0 ** np.floor(np.log2(np.sqrt(float(centre))))
    x = F32(np.floor(np.sqrt(float(centre)) * 0.98 / e * 2048.0) / 2048.0 * e)   # mantissa in [1, 2) to 11 fraction bits
    p = centre
    for _ in range(below):
        p = np.nextafter(p, F32(0))
    amps, want = [], []
    for _ in range(below + above + 1):
        y = F32(np.sqrt(float(p) - float(x) ** 2))
        amps.append(complex(x, y))
        want.append(p)
        p = np.nextafter(p, F32(np.inf))
    amps = np.array(amps, np.complex64)
    got = exact_power(amps)
    assert np.array_equal(got, np.array(want, F32)), "the ladder misses a power"
    return amps


def float_ladder(centre, below, above):
    """real float32 amplitudes: consecutive floats around `centre`"""
    c = F32(centre)
    lo, hi = [], []
    f = c
    for _ in range(below):
        f = np.nextafter(f, F32(0))
        lo.append(f)
    f = c
    for _ in range(above):
        f = np.nextafter(f, F32(np.inf))
        hi.append(f)
    return np.array(lo[::-1] + [c] + hi, F32)


def db64(p):
    """5 log10 P in float64 of exact float powers (the value the map owes); -inf at 0"""
    with np.errstate(divide="ignore"):
        return 5.0 * np.log10(np.asarray(p, F32).astype(np.float64))


# ---- raw buffers ----------------------------------------------------------------------------------------------------------------
def flat_raw(n, amps):
    """complex64 [B, n]: a_b * delta[n]"""
    amps = np.asarray(amps, np.complex64)
    x = np.zeros((len(amps), n), np.complex64)
    x[:, 0] = amps
    return x


def line_ints(n, i1, i3, ia):
    """int64 [B, n, 2] (re, im) in quanta: I1 i^n + I3 i^(3n) + ia delta[n] for integer arrays i1, i3, ia [B]"""
    i1, i3, ia = (np.asarray(v, np.int64).reshape(-1) for v in (i1, i3, ia))
    assert n % 4 == 0 and len(i1) == len(i3) == len(ia)
    s, d = i1 + i3, i1 - i3
    q = np.zeros((len(i1), n, 2), np.int64)
    q[:, 0::4, 0] = s[:, None]
    q[:, 1::4, 1] = d[:, None]
    q[:, 2::4, 0] = -s[:, None]
    q[:, 3::4, 1] = -d[:, None]
    q[:, 0, 0] += ia
    assert (n * np.maximum(np.abs(i1), np.abs(i3)) + np.abs(ia)).max() < 1 << 24, "a partial sum would not be a float"
    return q


def pack(kind, q):
    """integer samples [B, n, 2] in quanta -> the wire format's raw array"""
    if kind == KIND_FLOAT_COMPLEX:
        v = (q.astype(np.float64) * CFLOAT_QUANTUM).astype(F32)
        return np.ascontiguousarray(v).view(np.complex64).reshape(q.shape[0], q.shape[1])
    assert np.abs(q).max() <= INT_MAX[kind], (kind, int(np.abs(q).max()))
    if kind == KIND_SHORT:
        return np.ascontiguousarray(q.transpose(0, 2, 1)).astype(np.int16)   # planar: I[n] then Q[n]
    return np.ascontiguousarray(q).astype(np.int8 if kind == KIND_BYTE_COMPLEX else np.int16)


def line_values(kind, n, i1, i3, ia):
    """(line at N/4, line at 3N/4, floor): the exact float32 bin values of the line probes"""
    i1, i3, ia = (np.asarray(v, np.int64).reshape(-1) for v in (i1, i3, ia))
    s = scale_of(kind)
    return tuple(((n * a + ia).astype(np.float64) * s).astype(F32) for a in (i1, i3)) + ((ia.astype(np.float64) * s).astype(F32),)


def line_spectrum(kind, n, i1, i3, ia):
    """float32 [B, n]: the stated spectrum (real; the imaginary parts are zero) of the line probes"""
    h1, h3, fl = line_values(kind, n, i1, i3, ia)
    x = np.repeat(fl[:, None], n, axis=1)
    x[:, n // 4], x[:, 3 * n // 4] = h1, h3
    return x


def line_params(kind, n, count, seed=0):
    """`count` line probes for (kind, n): I1 as large as the format and 2^23 / n allow (so that the line reaches the exact half of
    the map at 16 points too), I3 about half of it (the two lines within 4 dB of each other, in 32 ... 64 dB from 1000 points up),
    and floors ia > 0 walking up in single quanta from a seeded start"""
    rng = np.random.default_rng(1000 * n + 10 * kind + seed)
    top = 8000 if kind != KIND_BYTE_COMPLEX else 40
    big = max(2, min(top, (1 << 23) // n))
    i1 = big - rng.integers(0, max(1, big // 8), count)
    i3 = i1 // 2 + rng.integers(0, max(1, big // 16), count)
    room = (INT_MAX[kind] if kind != KIND_FLOAT_COMPLEX else 32767) - (i1 + i3).max()
    ia = 1 + (rng.integers(0, 8) + np.arange(count)) % min(room, 2000)
    return i1, i3, ia
