"""The Welch probe streams of tests/welch_probes.py, pinned on the host before any GPU is involved.

Asserted:
  * the stated segment powers agree with a float64 FFT of the very float32 stream (every segment, every bin): flat bins to 1e-12
    relative, the line bin too (the stated float is its one rounding), the floor under a line to the float64 FFT's own rounding of
    the line (64 eps N A); as rationals the flat powers and their sums over a PSD are exact (asserted inside the generator, which every test here constructs);
  * oracle.welch / oracle.welch_raw under the rectangular window stay inside compare_spectra of the stated means, in all four wire
    formats -- which also pins the delivery-block layout of the packed streams (planar int16: I[hop] then Q[hop] per block);
  * mean_float: on flat bins every split into parts gives one float (the sums are exact); the product with the float 1/K and the
    oracle's division differ by at most one ulp of the mean, at most 2.6e-7 dB, and do differ for K = 3, 5, 7;
  * the probe sets have means on both sides of SCN_P_EXACT_FROM in every wire format;
  * the pins of (b): a K = 3 / 5 / 7 stream and its K = 4 partner owe the map the same float under the product form only;
  * every exactness precondition is refused by the generator when it is broken."""
import os

import numpy as np
import pytest

from tests import db_probes as pr
from tests import tolerances as tol
from tests import welch_probes as wp

F32 = np.float32
N, HOP = wp.N, wp.HOP
KINDS = [pr.KIND_FLOAT_COMPLEX, pr.KIND_SHORT_COMPLEX, pr.KIND_SHORT, pr.KIND_BYTE_COMPLEX]
NAMES = {pr.KIND_FLOAT_COMPLEX: "cfloat", pr.KIND_SHORT_COMPLEX: "int16", pr.KIND_SHORT: "int16planar", pr.KIND_BYTE_COMPLEX: "int8"}


def _stated_segment_powers(s):
    """float64 [segments, N] from the generator's own statement"""
    out = np.empty((s.n_psd * s.K, N))
    out[:, 0::2] = s.power["even"].reshape(-1, 1)
    out[:, 1::2] = s.power["odd"].reshape(-1, 1)
    if s.line:
        out[:, N // 4] = s.power["line"].reshape(-1)
    return out


@pytest.mark.parametrize("kind", KINDS, ids=[NAMES[k] for k in KINDS])
def test_stated_powers_against_float64(kind):
    """the formula X_s[k] = a_s + (-1)^k a_{s+1} (+ N A at N/4), K = 3 and two PSDs, against numpy's float64 FFT"""
    for s in (wp.flat(kind, 3, 2), wp.line(kind, 3, 2)):
        x = s.complex64().astype(np.complex128)
        want = _stated_segment_powers(s)
        top = float(np.sqrt(want.max()))
        for seg in range(s.n_psd * s.K):
            X = np.fft.fft(x[seg * HOP: seg * HOP + N])
            P = X.real ** 2 + X.imag ** 2
            if not s.line:
                assert np.abs(P - want[seg]).max() <= 1e-12 * want[seg].min(), (NAMES[kind], seg)
            else:
                exact = (float(s.seg_quanta["line"][seg]) * s.scale) ** 2   # (under 2^48 quanta^2: a double holds it)
                assert abs(P[N // 4] - exact) <= 1e-12 * exact and F32(P[N // 4]) == F32(exact) == F32(want[seg, N // 4])
                floor = np.arange(N) != N // 4
                assert np.abs(np.abs(X) - np.sqrt(want[seg]))[floor].max() <= 64 * np.finfo(np.float64).eps * top, (NAMES[kind], seg)


@pytest.mark.parametrize("kind", KINDS, ids=[NAMES[k] for k in KINDS])
def test_oracle_welch_holds_the_stated_means(oracle_mod, kind):
    for s in (wp.flat(kind, 3, 2), wp.line(kind, 3, 2), wp.flat(kind, 4, 1)):
        want = pr.db64(s.stated_means(1))
        with oracle_mod.window_type(oracle_mod.WIN_RECTANGULAR):
            got = oracle_mod.welch(s.complex64(), N, s.K, s.n_psd)
            raw = s.raw()
            if kind != pr.KIND_FLOAT_COMPLEX:
                raw = raw.view(np.int8 if kind == pr.KIND_BYTE_COMPLEX else np.int16)
                conv = oracle_mod.welch_convert(raw, kind, pr.ENOB[kind], False, HOP)
                assert np.array_equal(conv, s.complex64()), "the packed stream is the stated one, block by block"
                assert np.array_equal(oracle_mod.welch_raw(raw, kind, pr.ENOB[kind], False, N, s.K, s.n_psd), got)
        fig = tol.compare_spectra(got, want)
        assert fig["max_db_err_all_bins"] < 1e-5, fig   # (a mean's ulp and the dB map's, nothing else: the transform is exact here)


def test_mean_float_parts_and_the_two_forms():
    for K in (1, 2, 3, 4, 5, 7, 16):
        s = wp.flat(pr.KIND_FLOAT_COMPLEX, K, 4)
        one = s.means(1)
        for parts in (2, 4):
            if parts <= K:
                m = s.means(parts)
                assert all(m[k].tobytes() == one[k].tobytes() for k in ("even", "odd")), "exact sums: any order gives one float"
        for k in ("even", "odd"):   # against the rational mean: one rounding of the product with the float 1/K
            S = s.power[k].astype(np.float64).sum(axis=1)
            assert np.array_equal(one[k], (S.astype(F32) * (F32(1.0) / F32(K))).astype(F32))
            assert (np.abs(one[k].astype(np.float64) - S / K) <= np.spacing(one[k]).astype(np.float64)).all()
    rng = np.random.default_rng(11)
    S = rng.integers(1, 1 << 24, 200000).astype(F32)
    for K in (3, 5, 7):
        prod, div = S * (F32(1.0) / F32(K)), S / F32(K)
        ulps = np.abs(prod.view(np.int32).astype(np.int64) - div.view(np.int32).astype(np.int64))
        assert ulps.max() == 1, "the two forms differ, by one ulp of the mean at most"
        assert np.abs(pr.db64(prod) - pr.db64(div)).max() <= 2.6e-7
        assert 2.6e-7 < tol.DB_MAP_ABS
    for K in (2, 4, 16):
        assert np.array_equal(S * (F32(1.0) / F32(K)), S / F32(K))
    # a line bin's sum rounds at every add: the split into parts is part of the statement
    ln = wp.line(pr.KIND_FLOAT_COMPLEX, 7, 40)
    assert ln.means(1)["line"].tobytes() != ln.means(4)["line"].tobytes()


@pytest.mark.parametrize("kind", KINDS, ids=[NAMES[k] for k in KINDS])
def test_both_halves_of_the_map(kind):
    for K in (1, 2, 3, 4, 5, 7, 16):
        s = wp.line(kind, K, 2)
        m = s.means(1)
        assert (m["line"] >= tol.P_EXACT_FROM).all() and (m["odd"] < tol.P_EXACT_FROM).all(), (NAMES[kind], K)
        assert (m["odd"] >= np.finfo(F32).tiny).all() and (m["even"] >= np.finfo(F32).tiny).all()


@pytest.mark.parametrize("K", [3, 5, 7])
def test_product_form_pins(K):
    a, b, pins = wp.pin_streams(K, 8)
    assert a.K == K and b.K == 4 and a.n_psd == b.n_psd == 8
    q2 = F32(pr.CFLOAT_QUANTUM ** 2)
    want = np.array([m for m, _, _ in pins], F32) * q2
    for parts in (1, 2):
        assert a.means(parts)["even"].tobytes() == want.tobytes() and b.means(parts)["even"].tobytes() == want.tobytes()
    S = a.power["even"].astype(np.float64).sum(axis=1).astype(F32)
    div = S / F32(K)
    assert (div != want).all(), "the division gives the neighbouring float in every pinned PSD"
    assert (pr.db64(div).astype(F32) != pr.db64(want).astype(F32)).all(), "... whose correctly rounded dB value is another float"
    assert np.array_equal(b.power["even"].astype(np.float64).sum(axis=1) / 4.0, want.astype(np.float64)), "the partner's mean is exact"


def test_zero_bins_on_purpose():
    s = wp.Stream(pr.KIND_FLOAT_COMPLEX, 2, [300, -300, 300, 17, 90], zeros=True)
    m = s.means(1)
    assert m["even"][0] == 0.0 and m["odd"][0] > 0 and (m["even"][1] > 0)
    with np.errstate(divide="ignore"):
        assert np.isneginf(pr.db64(s.stated_means(1))[0, 0::2]).all()


def test_preconditions_are_refused():
    K = pr.KIND_FLOAT_COMPLEX
    for ia, k, why in (([2048, 2048 + 1], 1, "sum reaches 2^12"), ([2000, -2000], 1, "difference reaches 2^12"),
                       ([600, 500, 600, 450, 610], 4, "K times the largest power"), ([5, 5], 1, "equal neighbours"),
                       ([5, -5], 1, "opposite neighbours"), ([5, 7, 5], 2, "a repeated amplitude")):
        with pytest.raises(AssertionError):
            wp.Stream(K, k, ia)
    with pytest.raises(AssertionError):
        wp.Stream(pr.KIND_BYTE_COMPLEX, 1, [100, 20], line=64)        # 164 > 127
    with pytest.raises(AssertionError):
        wp.Stream(K, 1, [100, 20], line=256)                          # N A = 2^24
    with pytest.raises(AssertionError):
        wp.mean_float(np.ones((3, 4), F32), 3, 1)


def test_documents_name_this_suite():
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for doc in ("DESIGN.md", "README.md"):
        txt = open(os.path.join(root, doc)).read()
        assert "test_welch_exact_gpu.py" in txt and os.path.exists(os.path.join(here, "test_welch_exact_gpu.py")), doc
    assert "welch_probes.py" in open(os.path.join(root, "DESIGN.md")).read()
    assert "test_welch_exact_gpu.py" in open(os.path.join(here, "test_db_map_gpu.py")).read()
