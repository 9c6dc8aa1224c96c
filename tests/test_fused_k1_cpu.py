"""The premise of tests/test_fused_k1_gpu.py, on the host.

Every transform family forms a sample as conv(raw, dc, 1.0f) * (w[i] * scale): float(d) times the window tap with onebymax folded in
(scale = onebymax = +-2^-k, utility.cpp:16-17, 40-41, 64-65; d = int32(s - dc), utility.cpp:81-82).  A FLOAT_COMPLEX plan of the same
size and window, fed scn_convert_raw's output float(d) * scale, forms (float(d) * scale) * (w[i] * 1.0f).  The GPU module demands
bit-identical outputs of the two; that is a fair demand only if, in float32 and for every d, tap and scale that can occur,

    (float32(d) * scale) * w[i]  ==  float32(d) * (w[i] * scale)

bit for bit -- and equally where the compiler contracts the product into an FMA with whatever the first butterfly adds to it.  Both
hold if the two EXACT (unrounded) products are the same real number, since a rounded product and an FMA are functions of the exact
product (and the addend) alone.  The exact product of two float32 values fits a float64 (48 significant bits, exponents far inside the
range), so the test compares float64 products of the float32 factors with ==, then shows the float32 product and an FMA emulation on
them for the record.  The one way the fold can fail is a tap whose product with the scale is SUBNORMAL (w[i] * scale then rounds,
float32(d) * scale cannot): asserted absent for every window type, size and ENOB below; were one present the GPU module would have to
exempt that window.

ENOB: convert_scale (scn_host.hip) computes max = intN_t(1 << (enob - 1)); from enob = width + 1 up the narrowing leaves max = 0 and
the scale is 1 / 0 = inf -- no conversion at all -- so the values with a finite scale are 1 ... 16 for the int16 kinds and 1 ... 8 for
int8, and those are walked, the wrapping extremes (enob = width: a NEGATIVE scale) included.

d: the full range of s - dc for the width (both in range: |d| <= 2^width - 1), and what the negative-sum quirk of utility.cpp:77-78
makes of it: a negative sum divided as uint32 gives dc = (2^32 - |sum|) / n, about 2^32 / n, and d = int32(s - dc) wraps to
-(2^32 / n) + small -- beyond 2^24 at n <= 128, where float(int) itself rounds (that rounding is the same on both sides: it precedes
the product)."""
import numpy as np
import pytest

from scanner_amd import capi

# (name -> the plan's window type; the oracle numbers them as GNU Radio does, Hamming = 0, and is asked by name)
WINDOWS = {"HANN": capi.WIN_HANN, "BLACKMAN": capi.WIN_BLACKMAN, "RECTANGULAR": capi.WIN_RECTANGULAR, "KAISER": capi.WIN_KAISER,
           "BLACKMAN_HARRIS": capi.WIN_BLACKMAN_HARRIS, "BARTLETT": capi.WIN_BARTLETT, "FLATTOP": capi.WIN_FLATTOP, "HAMMING": capi.WIN_HAMMING}
SIZES = [16, 1000, 4096, 65536]
TINY = np.float32(np.finfo(np.float32).tiny)


def scale_of(width, enob):
    """convert_scale of scn_host.hip / scale_for_i16, scale_for_i8 of the oracle, restated: float(1.0 / intN_t(1 << (enob - 1)))"""
    one = (1 << ((enob - 1) & 31)) & ((1 << width) - 1)
    mx = one - (1 << width) if one >> (width - 1) else one
    assert mx != 0, "enob beyond the width: max wraps to 0, the scale is infinite"
    return np.float32(1.0 / mx)


def d_values(width, n, rng):
    """int32 d = s - dc: every value of the plain range, and the quirk's: dc = (2^32 - m) / n for sums -m just below zero, at -n (the
    last sum whose quotient is 2^32 / n - 1), and at the most negative sum n * min, each against samples over the whole range"""
    top = (1 << width) - 1
    plain = np.arange(-top, top + 1, dtype=np.int64)
    lo, hi = -(1 << (width - 1)), (1 << (width - 1)) - 1
    s = np.unique(np.concatenate([[lo, lo + 1, -1, 0, 1, hi - 1, hi], rng.integers(lo, hi + 1, 300)])).astype(np.int64)
    quirk = []
    for m in (1, 2, n - 1, n, n + 1, 2 * n + 1, -lo * n // 2, -lo * n):
        dc = ((1 << 32) - m) // n                       # uint32 division
        dc = dc - (1 << 32) if dc >> 31 else dc         # ... stored to the int32 sum (utility.cpp:77-78)
        quirk.append(((s - dc + (1 << 31)) % (1 << 32)) - (1 << 31))   # wrapping int32 subtraction
    quirk = np.concatenate(quirk)
    assert np.abs(quirk).max() > ((1 << 24) if n <= 128 else 0)
    return plain, quirk


def exact_products(d, w, scale):
    """the exact products of both forms, as float64 (products of two float32 values are exact there), shape [len(d), len(w)]"""
    fd = d.astype(np.float32)                              # float(int): rounds beyond 2^24, before either product
    left = (fd * scale).astype(np.float64)[:, None] * w.astype(np.float64)[None, :]       # (float(d) * scale) * w
    right = fd.astype(np.float64)[:, None] * (w * scale).astype(np.float64)[None, :]       # float(d) * (w * scale)
    return left, right


@pytest.fixture(scope="module")
def windows(oracle_mod):
    assert sorted(WINDOWS.values()) == list(range(1, 9)), "every window type scn_plan_create accepts (scanner_hip.h)"
    return {(name, n): oracle_mod.window(getattr(oracle_mod, "WIN_" + name), n) for name in WINDOWS for n in SIZES}


def test_the_scales_are_signed_powers_of_two():
    for width in (16, 8):
        for enob in range(1, width + 1):
            s = scale_of(width, enob)
            m, e = np.frexp(s)
            assert abs(m) == 0.5 and e == 2 - enob, (width, enob, s)
            assert (s < 0) == (enob == width), "only enob = width wraps max to the negative"
        with pytest.raises(AssertionError):
            scale_of(width, width + 1)


@pytest.mark.parametrize("name", list(WINDOWS))
def test_no_tap_times_scale_is_subnormal(windows, name):
    for n in SIZES:
        w = windows[(name, n)]
        assert np.isfinite(w).all()
        for width in (16, 8):
            for enob in range(1, width + 1):
                ws = w * scale_of(width, enob)
                assert ((ws == 0) | (np.abs(ws) >= TINY)).all(), (name, n, width, enob)
                assert ((ws == 0) == (w == 0)).all(), "a tap that vanishes only with the scale"
                assert np.array_equal(ws.astype(np.float64), w.astype(np.float64) * float(scale_of(width, enob))), "w * scale is exact"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(WINDOWS))
def test_the_fold_is_exact(windows, name, n):
    rng = np.random.default_rng(n)
    w = np.unique(windows[(name, n)])                      # (the windows are symmetric, two of them constant)
    nz = w[w != 0]
    some_w = np.unique(np.concatenate([[w.min(), w.max(), nz[np.abs(nz).argmin()]], rng.choice(w, min(5, len(w)))])).astype(np.float32)
    addends = np.float64(rng.standard_normal(3).astype(np.float32)) * np.array([1e-6, 1, 1e9])
    for width in (16, 8):
        plain, quirk = d_values(width, n, rng)
        some_d = np.unique(np.concatenate([[plain[0], -1, 0, 1, plain[-1], quirk.min(), quirk.max()], rng.choice(quirk, 5)]))
        for enob in range(1, width + 1):
            scale = scale_of(width, enob)
            for d, taps in ((plain, some_w), (quirk, some_w), (some_d, w)):     # every d on some taps, every tap on some d
                left, right = exact_products(d, taps, scale)
                assert np.array_equal(left, right), (name, n, width, enob)
                assert np.isfinite(left).all()
                # the float32 product, and the product contracted into an FMA with an addend: functions of the exact product
                assert np.array_equal(left.astype(np.float32), right.astype(np.float32))
                for c in addends:
                    assert np.array_equal((left + c).astype(np.float32), (right + c).astype(np.float32))
                # and the float32 arithmetic itself, as numpy rounds it
                fd = d.astype(np.float32)
                assert np.array_equal((fd * scale)[:, None] * taps[None, :], fd[:, None] * (taps * scale)[None, :])
