"""Signals on the GPU (scn_collect_signals, scn_hits.hip): in every case Plan.collect_signals equals scn_signals_from_hits on
the same slot's full hit list and the numpy restatement of tests/signals_ref.py, record for record and bit for bit; the planted
scenes add signal lists written out from what was planted."""
import ctypes as C

import numpy as np
import pytest
import torch

from scanner_amd import Plan, capi
from tests import signals_ref

pytestmark = pytest.mark.gpu

FS = 8000000


def _noise(n, nb, seed, sigma=0.05):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((nb, n, 2), dtype=np.float32) * np.float32(sigma)).view(np.complex64).reshape(nb, n)


def _submit(plan, slot, x, **kw):
    d_raw = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()
    plan.submit_device(slot, d_raw, x.shape[0], **kw)


def _run(plan, x, slot=0, **kw):
    """submit + collect: the slot's FULL hit list (the part beyond max_hits walked with collect_more)"""
    _submit(plan, slot, x, **kw)
    return plan.collect(slot, want_power=False)[1]


def _median_threshold(n, x):
    """the median of the plan's own spectrum over x"""
    with Plan(n, FS, 1e9, max_batch=x.shape[0], flags=capi.OUT_SPECTRUM) as plan:
        _submit(plan, 0, x)
        p = plan.collect(0)[0]
    return float(np.median(p))


def _check(plan, slot, hits, n, gaps, fs=FS):
    """the GPU's signals against both host forms; returns the reference lists by gap"""
    out = {}
    for g in gaps:
        got = plan.collect_signals(slot, g)
        want = signals_ref.signals(hits, n, fs, g)
        signals_ref.assert_same(got, capi.signals_from_hits(hits, n, fs, g), f"n {n} max_gap {g}: GPU against scn_signals_from_hits")
        signals_ref.assert_same(got, want, f"n {n} max_gap {g}: GPU against the numpy reference")
        assert int(got["n_hits"].sum()) == len(hits)
        out[g] = want
    return out


# 16: one bitmap word; 64: a run crossing the word boundary at i = 32, and units outnumbering a workgroup's waves many times; 1000:
# mixed radix; 1001: Bluestein; 4096; 32768: four-step, the largest bitmap exercised (two waves per workgroup)
@pytest.mark.parametrize("n,nb", [(16, 5), (64, 300), (1000, 5), (1001, 5), (4096, 5), (32768, 2)])
def test_noise_at_the_median(built_lib, n, nb):
    x = _noise(n, nb, seed=n)
    thr = _median_threshold(n, x)
    with Plan(n, FS, thr, max_batch=nb, dc_ignore_bins=0 if n == 64 else 4) as plan:
        hits = _run(plan, x)
        assert len(hits) > nb
        ref = _check(plan, 0, hits, n, (0, 1, 7, 31, 32, 63, 64, n))
    if n == 64:  # (no DC mask here, so that runs can cross the word boundary)
        assert np.any((ref[0]["first_i"] < 32) & (ref[0]["last_i"] >= 32)), "no run crosses the word boundary at i = 32"
    if n == 4096:  # the regimes this input is here for
        assert np.bincount(ref[0]["seq_id"].astype(np.int64)).max() > 64, "no unit with more than 64 signals"
        assert max(r["n_hits"].max() for r in ref.values()) > 64, "no signal of more than 64 hits"
        assert max((r["last_i"] - r["first_i"] + 1).max() for r in ref.values()) > 64, "no signal wider than 64 bins"
    assert len(ref[n]) == len(np.unique(hits["seq_id"]))  # max_gap = n: one signal per unit that has hits


@pytest.mark.parametrize("n", [16, 64, 1000, 4096])
def test_every_evaluated_bin_a_hit(built_lib, n):
    """threshold -200 dB: two signals per buffer around the DC mask's 7 bins up to max_gap 6, one from 7"""
    nb, half, use_window, dcw = 3, n // 2, int(0.75 * n / 2.0), 4
    x = _noise(n, nb, seed=3)
    with Plan(n, FS, -200.0, max_batch=nb) as plan:
        hits = _run(plan, x)
        assert len(hits) == nb * (2 * use_window + 1 - (2 * dcw - 1))
        ref = _check(plan, 0, hits, n, (0, 6, 7))
    for g in (0, 6):
        assert [(int(s["seq_id"]), int(s["first_i"]), int(s["last_i"])) for s in ref[g]] == [
            t for b in range(nb) for t in ((b, half - use_window, half - dcw), (b, half + dcw, half + use_window))]
        assert np.all(ref[g]["n_hits"] == use_window - dcw + 1)
    assert [(int(s["seq_id"]), int(s["first_i"]), int(s["last_i"]), int(s["n_hits"])) for s in ref[7]] == [
        (b, half - use_window, half + use_window, 2 * (use_window - dcw + 1)) for b in range(nb)]


# ---- planted scenes: a spectrum with chosen strong bins, through the inverse FFT -----------------------------------------------
def _amp(i):
    """the planted amplitude of bin i: 30 .. 32.3 dB, distinct inside any run used here (asserted where it matters)"""
    return 1000.0 + 7.0 * ((i * 37) % 101)


def _planted(n, buffers, amp=_amp):
    """buffers: per buffer a list of (first_i, last_i) runs -> complex64 [B, n] whose n-point FFT has amplitude amp(i) in the
    planted bins (natural bin j = (i + n/2) % n) and nothing elsewhere: numpy's inverse FFT in float64, cast once"""
    S = np.zeros((len(buffers), n), np.complex128)
    for b, runs in enumerate(buffers):
        for lo, hi in runs:
            for i in range(lo, hi + 1):
                S[b, (i + n // 2) % n] = amp(i)
    return np.fft.ifft(S, axis=1).astype(np.complex64)


def _expected(hits, buffers, merged, n, fs=FS, amp=_amp):
    """The signal list written from the planted pattern: merged[b] lists, per signal, the indices of buffer b's runs it is made
    of.  The peak is the planted bin of the largest amplitude; its power_db and freq_hz are its hit record's own."""
    rows = []
    for b, groups in enumerate(merged):
        for idx in groups:
            bins = [i for r in idx for i in range(buffers[b][r][0], buffers[b][r][1] + 1)]
            amps = [amp(i) for i in bins]
            assert len(set(amps)) == len(amps), "the scene has an unplanned tie"
            peak = bins[int(np.argmax(amps))]
            h = hits[(hits["seq_id"] == b) & (hits["i"] == peak)]
            assert len(h) == 1
            rows.append((b, h["freq_hz"][0], bins[0], bins[-1], peak, len(bins), h["power_db"][0], (bins[-1] - bins[0] + 1) * (fs // n)))
    return np.array(rows, capi.SIGNAL_DTYPE)


# g = the gap the scene is built around: runs 0 and 1 of buffer 0 lie exactly g empty bins apart, runs 1 and 2 g + 1
SCENES = {
    # no DC mask (dc_ignore_bins = 0), evaluated bins 8 .. 56, one word boundary at 32
    64: dict(g=2, dc=0, buffers=[
        [(8, 10), (13, 14), (18, 19), (29, 31), (40, 41), (55, 56)],  # first evaluated bin; g and g + 1 apart; ends at bit 31; last evaluated bin
        [],                                                          # a buffer with no hits between two that have some
        [(20, 22), (32, 34), (45, 45)],                              # starts at bit 32 (31 empty)
        [(30, 33), (50, 52)],                                        # crosses the word boundary
    ], merged_g=[[[0, 1], [2], [3], [4], [5]], [], [[0], [1], [2]], [[0], [1]]]),
    # the defaults: evaluated bins 512 .. 3584 without 2045 .. 2051
    4096: dict(g=5, dc=4, buffers=[
        [(512, 514), (520, 521), (528, 530), (1021, 1023), (1056, 1060), (1086, 1091), (2040, 2044), (2052, 2060), (3580, 3584)],
        [],
        [(1024, 1030), (3000, 3000), (3584, 3584)],
    ], merged_g=[[[0, 1], [2], [3], [4], [5], [6], [7], [8]], [], [[0], [1], [2]]]),
}


@pytest.mark.parametrize("n", sorted(SCENES))
def test_planted_scenes(built_lib, n):
    sc = SCENES[n]
    buffers, g = sc["buffers"], sc["g"]
    x = _planted(n, buffers)
    # planted bins are at 30 dB or more, the others hold rounding residue far below -30 dB: the threshold is midway
    with Plan(n, FS, 0.0, max_batch=len(buffers), window_type=capi.WIN_RECTANGULAR, dc_ignore_bins=sc["dc"]) as plan:
        hits = _run(plan, x)
        planted = [(b, i) for b, runs in enumerate(buffers) for lo, hi in runs for i in range(lo, hi + 1)]
        assert [(int(h["seq_id"]), int(h["i"])) for h in hits] == planted, "the hit list is not exactly the planted bins"
        assert np.all(hits["power_db"] >= 29.9) and np.all(hits["power_db"] <= 32.5)
        every_run = [[[r] for r in range(len(runs))] for runs in buffers]
        for gap, merged in ((0, every_run), (g - 1, every_run), (g, sc["merged_g"])):
            got = plan.collect_signals(0, gap)
            signals_ref.assert_same(got, _expected(hits, buffers, merged, n), f"max_gap {gap}: against the planted pattern")
        _check(plan, 0, hits, n, (0, g - 1, g, g + 1, 7, 31, 32, n))


def test_tie_inside_a_run(built_lib):
    """two planted bins of identical amplitude in one run: the peak is the lower i if their power_db come out bit-equal, and
    whichever the reference says otherwise"""
    n = 4096
    tie = {700: 1000.0, 701: 1500.0, 702: 1500.0, 703: 1200.0, 900: 1300.0, 901: 1300.0}
    x = _planted(n, [[(700, 703), (900, 901)]], amp=lambda i: tie[i])
    with Plan(n, FS, 0.0, max_batch=1, window_type=capi.WIN_RECTANGULAR) as plan:
        hits = _run(plan, x)
        assert list(hits["i"]) == sorted(tie)
        ref = _check(plan, 0, hits, n, (0, 1000))
    p = {int(h["i"]): h["power_db"] for h in hits}
    assert [int(s["peak_i"]) for s in ref[0]] == [701 if p[701] >= p[702] else 702, 900 if p[900] >= p[901] else 901]
    assert len(ref[1000]) == 1 and int(ref[1000]["peak_i"][0]) in (701, 702)


@pytest.fixture(scope="module")
def dense():
    """5 x 4096 points of noise and the median threshold: thousands of hits, hundreds of signals per buffer"""
    x = _noise(4096, 5, seed=11)
    return x, _median_threshold(4096, x)


def test_max_hits_far_below_the_total(built_lib, dense):
    x, thr = dense
    with Plan(4096, FS, thr, max_batch=5, max_hits=64) as plan:
        hits = _run(plan, x)  # (collect walks the list beyond max_hits with collect_more)
        assert len(hits) > 5000 and plan.last_n_hits == len(hits)
        ref = _check(plan, 0, hits, 4096, (0, 3))
    assert set(ref[0]["seq_id"]) == set(range(5)) and len(ref[0]) > 1000


def test_windows(built_lib, dense):
    x, thr = dense
    with Plan(4096, FS, thr, max_batch=5) as plan:
        hits = _run(plan, x)
        want = _check(plan, 0, hits, 4096, (1,))[1]
        total = len(want)
        per_unit = np.bincount(want["seq_id"].astype(np.int64))
        assert per_unit.min() > 100
        a, b = int(per_unit[0]) // 2, int(per_unit[0] + per_unit[1] + per_unit[2] // 3)  # both in the middle of a unit
        signals_ref.assert_same(plan.collect_signals(0, 1, first=a), want[a:], "from the middle of unit 0 to the end")
        assert plan.last_n_signals == total
        with pytest.raises(capi.ScannerError) as e:
            plan.collect_signals(0, 1, first=a, cap=b - a)
        assert e.value.status == capi.E_TRUNCATED
        out = np.zeros(b - a + 2, capi.SIGNAL_DTYPE)
        out["n_hits"] = 0xDEADBEEF
        n_sig = C.c_uint32()
        L = capi.lib()
        st = L.scn_collect_signals(plan.handle, 0, 1, a, out.ctypes.data_as(C.c_void_p), b - a, C.byref(n_sig))
        assert (st, n_sig.value) == (capi.E_TRUNCATED, total)          # the records stored are valid, nothing beyond them is touched
        signals_ref.assert_same(out[: b - a], want[a:b], "a window from the middle of unit 0 to the middle of unit 2")
        assert np.all(out["n_hits"][b - a:] == 0xDEADBEEF)
        st = L.scn_collect_signals(plan.handle, 0, 1, 0, None, 0, C.byref(n_sig))  # the total alone
        assert (st, n_sig.value) == (capi.E_TRUNCATED, total)
        signals_ref.assert_same(plan.collect_signals(0, 1, first=total - 3, cap=10), want[total - 3:], "a window past the end")
        assert len(plan.collect_signals(0, 1, first=total)) == 0 and len(plan.collect_signals(0, 1, first=total + 5, cap=4)) == 0
        st = L.scn_collect_signals(plan.handle, 0, 1, 0, None, 4, C.byref(n_sig))
        assert st == capi.E_INVALID


def test_hits_only_plan_gives_the_same_signals(built_lib, dense):
    x, thr = dense
    got = []
    for flags in (capi.OUT_HITS, capi.OUT_SPECTRUM | capi.OUT_HITS):
        with Plan(4096, FS, thr, max_batch=5, flags=flags) as plan:
            hits = _run(plan, x)
            got.append(_check(plan, 0, hits, 4096, (0, 7)))
    for g in (0, 7):
        signals_ref.assert_same(got[0][g], got[1][g], f"hits-only against spectrum + hits, max_gap {g}")


def test_averaged_plan(built_lib):
    """units are the groups; seq_id is the group's first buffer's"""
    n, K, G = 1024, 2, 3
    x = _noise(n, K * G, seed=5)
    with Plan(n, FS, 1e9, max_batch=K * G, average=K, flags=capi.OUT_SPECTRUM) as plan:
        _submit(plan, 0, x)
        thr = float(np.median(plan.collect(0)[0]))
    seq = np.arange(500, 500 + K * G, dtype=np.uint64)
    with Plan(n, FS, thr, max_batch=K * G, average=K) as plan:
        hits = _run(plan, x, seq_ids=seq, center_freqs=np.repeat(1e9 + 6e6 * np.arange(G), K))
        ref = _check(plan, 0, hits, n, (0, 2, n))
    assert sorted(set(int(s) for s in ref[0]["seq_id"])) == [500, 502, 504]
    assert [int(s) for s in ref[n]["seq_id"]] == [500, 502, 504]


def test_table_indexed_submit(built_lib, dense):
    x, thr = dense
    table = 88e6 + 6e6 * np.arange(7)
    first_index = 5  # buffers 0 .. 4 carry entries 5, 6, 0, 1, 2
    with Plan(4096, FS, thr, max_batch=5) as plan:
        plan.set_table(table)
        hits = _run(plan, x, first_index=first_index)
        ref = _check(plan, 0, hits, 4096, (0, 7))
    for s in ref[7][:: max(1, len(ref[7]) // 50)]:  # the peak's frequency in the reference's arithmetic, from the table's entry
        fc = table[(first_index + int(s["seq_id"])) % len(table)]
        assert int(s["peak_freq_hz"]) == int(fc - float(FS // 2) + float(int(s["peak_i"]) * (FS // 4096)))
    assert len(set(ref[7]["seq_id"])) == 5


def test_pending_slot_is_undisturbed(built_lib, dense):
    x, thr = dense
    y = _noise(4096, 5, seed=12)
    with Plan(4096, FS, thr, max_batch=5) as plan:
        _submit(plan, 0, y)
        p_plain, h_plain, t_plain = plan.collect(0)   # the plain run of y
        hits = _run(plan, x, slot=0)
        _submit(plan, 1, y)                       # pending while slot 0's signals are built
        _check(plan, 0, hits, 4096, (0, 7))
        p1, h1, t1 = plan.collect(1)
        assert np.array_equal(p1, p_plain) and np.array_equal(h1, h_plain) and np.array_equal(t1, t_plain)
        _check(plan, 1, h1, 4096, (0,))


def test_status_paths(built_lib, dense):
    x, thr = dense
    L = capi.lib()
    n_sig = C.c_uint32(77)
    with Plan(4096, FS, thr, max_batch=5) as plan:
        assert L.scn_collect_signals(plan.handle, 0, 0, 0, None, 0, C.byref(n_sig)) == capi.E_STATE      # nothing collected yet
        assert L.scn_collect_signals(plan.handle, capi.NUM_SLOTS, 0, 0, None, 0, C.byref(n_sig)) == capi.E_INVALID
        assert L.scn_collect_signals(plan.handle, 0, 0, 0, None, 0, None) == capi.E_INVALID
        _submit(plan, 0, x)
        assert L.scn_collect_signals(plan.handle, 0, 0, 0, None, 0, C.byref(n_sig)) == capi.E_STATE      # pending
        hits = plan.collect(0, want_power=False)[1]
        _check(plan, 0, hits, 4096, (0,))
        _submit(plan, 0, x)                                                                              # the slot's next submit:
        assert L.scn_collect_signals(plan.handle, 0, 0, 0, None, 0, C.byref(n_sig)) == capi.E_STATE      # the old list is gone
        hits = plan.collect(0, want_power=False)[1]
        _check(plan, 0, hits, 4096, (0,))                                                                # until it is collected
    with Plan(4096, FS, 1e9, max_batch=5) as plan:                                                       # no hits at all
        assert len(_run(plan, x)) == 0
        got = plan.collect_signals(0, 3)
        assert got.dtype == capi.SIGNAL_DTYPE and len(got) == 0 and plan.last_n_signals == 0
    with Plan(4096, FS, thr, max_batch=5, flags=capi.OUT_SPECTRUM) as plan:                              # a plan without hits
        _submit(plan, 0, x)
        plan.collect(0)
        assert L.scn_collect_signals(plan.handle, 0, 0, 0, None, 0, C.byref(n_sig)) == capi.E_INVALID
    with Plan(4096, FS, 0.0, max_batch=5, mode=capi.MODE_TIME_DOMAIN) as plan:
        _submit(plan, 0, x)
        plan.collect_time_domain(0)
        assert L.scn_collect_signals(plan.handle, 0, 0, 0, None, 0, C.byref(n_sig)) == capi.E_INVALID
