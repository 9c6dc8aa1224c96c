"""Every grid-capped kernel past its grid.

Many launchers cap their grid at a fixed size or at a multiple of the CU count, and their kernels walk the rest of the work in a
`for (...; x += stride)` loop.  The second trip through such a loop is where a persistent kernel goes wrong: the next buffer's
prefetch descriptor, LDS reused behind a barrier, a per-buffer counter that must be zeroed again, a sum scratch that must be free
again, an index that must advance by exactly the grid.  The fused kernels, the buffer queue, the floor, time-domain, averaged and list
kernels have such tests (test_dispatch_gpu.py, test_parity_gpu.py, test_floor_gpu.py, test_time_domain_gpu.py, test_welch.py,
test_sweep_gpu.py); here are the four families no deterministic test took round their loop:

  four-step columns   scn_big_cols_kernel at 32768 / 65536 points: G buffers per trip            test_four_step_columns_*
  Bluestein           scn_gen_load_kernel: 8 CUs buffers per trip                                 test_bluestein_load_kernel_*
                      scn_gen_stage_kernel<2 / 4 / 16>, _pointwise, _finish: 8192 CUs items       test_bluestein_stages_pointwise_and_finish
  signals             scn_signal_count / _build_kernel: 8192 x waves units per trip; the scan     test_signals_beyond_the_block_cap
                      of the signal counts over 33 blocks of 2048
  convert             scn_convert_kernel: 2048 buffers per trip                                   test_convert_beyond_the_block_cap

Every batch comes from tests/launch_caps.py as TWICE the cap plus a small odd remainder, from the CU count of the device the test
runs on: some workgroups make three trips, the rest two, on any partition (asserted: nb > 2 * cap; tests/test_launch_caps_cpu.py holds
the caps to the launchers' source).  Every buffer has its own content (its own noise and its own tones, level or offset), so a
skipped, repeated or swapped buffer differs by whole dB.  Run with -s for the shapes, the caps and the largest errors.

The bars are those of tests/tolerances.py: spectra to compare_spectra; hit lists exact (bin, buffer id, frequency, order) outside
the guard band of the threshold on the oracle's spectrum, the band's population bounding the rest; against float64, exact wherever
the spectrum bar itself could not move the bin across the threshold (flip_unsafe), with at most 2 % of the reference's records
exempt."""
import ctypes as C

import numpy as np
import pytest

from scanner_amd import Plan, capi, synth
from tests import launch_caps as caps
from tests import signals_ref
from tests import tolerances as tol
from tests.test_parity_gpu import _assert_hits_equal

pytestmark = pytest.mark.gpu
FS = 8000000
CF, I16, I16P, I8 = capi.KIND_FLOAT_COMPLEX, capi.KIND_SHORT_COMPLEX, capi.KIND_SHORT, capi.KIND_BYTE_COMPLEX
NAMES = {CF: "cfloat", I16: "int16", I16P: "int16planar", I8: "int8"}


@pytest.fixture(scope="module")
def gpu(built_lib):
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need a GPU; refusing to skip silently"
    return torch


@pytest.fixture(scope="module")
def cus(gpu):
    return gpu.cuda.get_device_properties(0).multi_processor_count


def _to_dev(torch, raw):
    return torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).reshape(-1)).cuda()


def _offset(raw, off):
    """a positive offset for the integer DC removal to take out, clipped, not wrapped; every I and Q sum stays positive (the
    negative-sum quirk of utility.cpp:77-78 has its own tests, and rides along in test_convert_beyond_the_block_cap)"""
    info = np.iinfo(raw.dtype)
    raw = np.clip(raw.astype(np.int32) + off, info.min, info.max).astype(raw.dtype)
    sums = raw.astype(np.int64).sum(axis=2 if raw.shape[1] == 2 else 1)   # planar [B, 2, n] or interleaved [B, n, 2]
    assert (sums > 0).all()
    return raw


def _in_range(h, seq0, nb, n):
    """every record names a buffer of the launch and a bin of the transform (an unwritten record of a list too long does not)"""
    assert np.all((h["seq_id"] >= np.uint64(seq0)) & (h["seq_id"] < np.uint64(seq0 + nb))), "a record's seq_id is not one of the launch's"
    assert np.all(h["i"] < n), "a record's bin is beyond the transform"


def _counts(h, seq0, nb):
    return np.bincount((h["seq_id"] - np.uint64(seq0)).astype(np.int64), minlength=nb)


def _exact_outside_guard(h, h_ref, p_ref, n, thr, seq0, ev=None):
    """The scheme of test_every_fused_specialisation_vs_oracle: every record whose bin is NOT within tol.GUARD_DB of the threshold on
    the oracle's spectrum must be there, bit for bit and in order; the band's population bounds what may differ inside it.  Returns
    the band [B, n]."""
    ev = tol.evaluated_mask(n) if ev is None else ev
    _in_range(h, seq0, len(p_ref), n)
    near = np.zeros(p_ref.shape, bool)
    near[:, ev] = np.abs(p_ref[:, ev].astype(np.float64) - thr) < tol.GUARD_DB

    def outside(a):
        return a[~near[(a["seq_id"] - np.uint64(seq0)).astype(np.int64), (a["i"].astype(np.int64) + n // 2) % n]]

    g, r = outside(h), outside(h_ref)
    assert len(g) == len(r), (len(g), len(r))
    for f in ("seq_id", "i", "freq_hz"):
        assert np.array_equal(g[f], r[f]), f
    assert abs(len(h) - len(h_ref)) <= int(near.sum())
    # the powers of those records (aligned one to one by the checks above): the dB bar on bins at or above their buffer's mean
    # power -- the bar compare_spectra holds a spectrum to --, a sanity bound on the others
    err = np.abs(g["power_db"].astype(np.float64) - r["power_db"])
    ok = np.isfinite(p_ref)
    mean = np.where(ok, tol.db_to_power(np.where(ok, p_ref, 0)), 0.0).mean(axis=1)
    big = tol.db_to_power(r["power_db"].astype(np.float64)) >= tol.DB_MIN_POWER_RATIO * mean[(r["seq_id"] - np.uint64(seq0)).astype(np.int64)]
    assert np.all(err[big] <= tol.DB_REL * np.abs(r["power_db"][big].astype(np.float64)) + tol.DB_ABS) and err.max(initial=0) < 0.2
    return near


def _check_against_oracle(p, h, t, p_ref, h_ref, t_ref, n, thr, trig_count, seq0):
    """spectra to the bar; records exact outside the guard band, its population bounding the rest; trigger flags wherever the band
    cannot move the count across trigger_count; a record carries the float the spectrum holds.  Returns the figures."""
    nb = len(p_ref)
    fig = tol.compare_spectra(p, p_ref) if p is not None else None
    near = _exact_outside_guard(h, h_ref, p_ref, n, thr, seq0)
    band = int(near.sum())
    c_ref = _counts(h_ref, seq0, nb)
    trig_safe = (c_ref + near.sum(axis=1) <= trig_count) | (c_ref - near.sum(axis=1) > trig_count)
    assert np.array_equal(t[trig_safe], t_ref[trig_safe]) and trig_safe.mean() > 0.9
    # per-buffer counts: a buffer without a bin in the band has exactly the reference's count
    clean = ~near.any(axis=1)
    assert np.array_equal(_counts(h, seq0, nb)[clean], c_ref[clean])
    if p is not None:
        jj = (h["i"].astype(np.int64) + n // 2) % n
        assert np.array_equal(h["power_db"], p[(h["seq_id"] - np.uint64(seq0)).astype(np.int64), jj]), "a record carries the float the spectrum holds"
    if band == 0:
        _assert_hits_equal(h, h_ref, p_ref, np.arange(nb, dtype=np.uint64) + np.uint64(seq0))
    return fig, band


def _float64_check(p, h, db64, thr, n, seq0, what):
    """against plain float64: the spectrum to the bar; the records exact (buffer, bin, order) wherever the bar itself could not move
    the bin across the threshold; the exempt records at most 2 % of the reference's -- a condition (tests/test_launch_caps_cpu.py
    holds it on a CPU sample of the same generator), not a measurement"""
    fig = tol.compare_spectra(p, db64)
    _in_range(h, seq0, len(db64), n)
    ev = tol.evaluated_mask(n)
    unsafe = tol.flip_unsafe(db64, thr)
    rb, ri = caps.reference_hits(db64, thr, ev, n)
    r_safe = ~unsafe[rb, (ri + n // 2) % n]
    share = 1.0 - float(r_safe.mean())
    gb, gi = (h["seq_id"] - np.uint64(seq0)).astype(np.int64), h["i"].astype(np.int64)
    g_safe = ~unsafe[gb, (gi + n // 2) % n]
    print(f"{what} against float64: {fig}; {len(rb)} reference records, exempt share {100 * share:.3f} % (the condition: under "
          f"{100 * caps.MAX_EXEMPT_SHARE:.0f} %)")
    assert len(rb) > 10 * len(db64) and share < caps.MAX_EXEMPT_SHARE, (len(rb), share)
    assert int(g_safe.sum()) == int(r_safe.sum()), (int(g_safe.sum()), int(r_safe.sum()))
    assert np.array_equal(gb[g_safe], rb[r_safe]) and np.array_equal(gi[g_safe], ri[r_safe])
    return fig, share


# ---- four-step columns ----------------------------------------------------------------------------------------------------------
FOUR_STEP_LOADS = [(CF, 12, False), (I16, 12, True), (I16P, 14, False), (I8, 8, True)]


@pytest.mark.parametrize("kind,enob,dc", FOUR_STEP_LOADS, ids=[f"{NAMES[k]}{'-dc' if dc else ''}" for k, _, dc in FOUR_STEP_LOADS])
@pytest.mark.parametrize("n", [32768, 65536])
def test_four_step_columns_past_the_grid(gpu, cus, oracle_mod, n, kind, enob, dc):
    """scn_big_cols_kernel: workgroup (j, g) owns column tile j of buffers g, g + G, g + 2 G, ...  nb = 2 G + 5: five of the G
    workgroup rows make three trips, the others two (197 / 101 buffers at 256 CUs).  Against the oracle.  The cfloat case of each size
    also runs hits-only, holds 65536 points to float64 as well, and submits a loud batch and then a quiet one to the SAME slot, twice
    over (a slot's counts have two generations): buffers b >= G hold the loud batch's counts unless the loop zeroes
    per_buffer_hits[b] on every trip."""
    G = caps.four_step_cap(cus, n)
    nb = caps.two_trips_and(G, 5)
    assert nb > 2 * G
    print(f"\nfour-step columns: n {n} {NAMES[kind]} dc {dc}: {cus} CUs, G {G}, {nb} buffers (trips {np.bincount([caps.trip_of(b, G) for b in range(nb)]).tolist()})")
    x = caps.scene(n, nb, seed=5000 + n)
    raw = synth.quantize(x, kind)
    if dc:
        raw = _offset(raw, 60 if raw.dtype == np.int16 else 11)
    seq0 = 1 << 33
    fc, seq = 70e6 + 6e6 * np.arange(nb), np.arange(nb, dtype=np.uint64) + np.uint64(seq0)
    ev = tol.evaluated_mask(n)
    p_ref, _, _ = oracle_mod.Oracle(n, FS, 1e9, kind=kind, enob=enob, correct_dc=dc).run(raw, want_hits=False, threads=8)
    thr = caps.noise_tail_threshold(p_ref, ev)
    o = oracle_mod.Oracle(n, FS, thr, kind=kind, enob=enob, correct_dc=dc)
    _, h_ref, _ = o.run(raw, fc, seq, want_power=False, threads=8)
    trig_count = max(1, int(np.median(_counts(h_ref, seq0, nb))))   # about half of the flags set
    o.params.trigger_count = trig_count
    _, h_ref, t_ref = o.run(raw, fc, seq, want_power=False, threads=8)
    c_ref = _counts(h_ref, seq0, nb)
    assert len(np.unique(c_ref)) > 10 and t_ref.any() and not t_ref.all()
    cap = len(h_ref) + 65536
    d_raw = _to_dev(gpu, raw)
    with Plan(n, FS, thr, kind=kind, enob=enob, correct_dc=dc, max_batch=nb, max_hits=cap, trigger_count=trig_count) as plan:
        plan.submit_device(0, d_raw, nb, fc, seq)
        p, h, t = plan.collect(0, hit_cap=cap)
        fig, band = _check_against_oracle(p, h, t, p_ref, h_ref, t_ref, n, thr, trig_count, seq0)
        print(f"  against the oracle: {fig}; thr {thr:.3f} dB, {len(h_ref)} records, {band} bins in the guard band, {int(t_ref.sum())} triggers")
        if kind != CF:
            return
        if n == 65536:
            _float64_check(p, h, caps.float64_db(x, plan.window()), thr, n, seq0, f"  four-step n {n}")
        # loud, then quiet, on the same slot, through both generations of its counts
        quiet = (caps.scene(n, nb, seed=6000 + n) * np.float32(0.25)).astype(np.complex64)   # 6 dB down: tones still report, little noise does
        oq = oracle_mod.Oracle(n, FS, thr, trigger_count=trig_count)
        pq_ref, hq_ref, tq_ref = oq.run(quiet, fc, seq, threads=8)
        cq = _counts(hq_ref, seq0, nb)
        assert 0 < len(hq_ref) < len(h_ref) // 2 and (cq[G:] != c_ref[G:]).mean() > 0.9 and (cq == 0).any() and (cq > 0).any()
        d_quiet = _to_dev(gpu, quiet)
        plan.submit_device(0, d_raw, nb, fc, seq)   # the loud batch in the counts' other generation
        assert plan.collect(0, want_power=False, hit_cap=cap)[1].tobytes() == h.tobytes()
        for generation in range(2):
            plan.submit_device(0, d_quiet, nb, fc, seq)
            pq, hq, tq = plan.collect(0, hit_cap=cap)
            _, bq = _check_against_oracle(pq, hq, tq, pq_ref, hq_ref, tq_ref, n, thr, trig_count, seq0)
            assert abs(len(hq) - len(hq_ref)) <= bq
        print(f"  quiet after loud on one slot: {len(hq_ref)} records after {len(h_ref)}, {bq} bins in the guard band")
    # hits-only: the same records from the kernels without spectrum stores
    with Plan(n, FS, thr, max_batch=nb, max_hits=cap, trigger_count=trig_count, flags=capi.OUT_HITS) as plan:
        plan.submit_device(0, d_raw, nb, fc, seq)
        p0, h0, t0 = plan.collect(0, hit_cap=cap)
        assert p0 is None
        _check_against_oracle(None, h0, t0, p_ref, h_ref, t_ref, n, thr, trig_count, seq0)   # (records' powers included)


# ---- Bluestein ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,enob,dc", [(CF, 12, False), (I16, 12, True), (I16P, 14, True), (I8, 8, True)],
                         ids=["cfloat", "int16-dc", "int16planar-dc", "int8-dc"])
def test_bluestein_load_kernel_past_the_grid(gpu, cus, oracle_mod, kind, enob, dc):
    """scn_gen_load_kernel takes one buffer per workgroup and trip, 8 CUs workgroups: n = 17, nb = 2 * 8 CUs + 37 (the DC sums'
    scratch, s_sum, must be free again on every trip).  Against the oracle's DFT, as test_non_power_of_two_sizes_vs_oracle
    compares: spectra to the bar, the hit list bit for bit at a threshold whose guard band is empty, the trigger flags."""
    n = 17
    cap = caps.bluestein_load_cap(cus)
    nb = caps.two_trips_and(cap, 37)
    assert nb > 2 * cap and capi.size_path(n) == capi.PATH_BLUESTEIN
    print(f"\nBluestein load kernel: n {n} {NAMES[kind]} dc {dc}: {cus} CUs, {cap} workgroups, {nb} buffers")
    # a fifth of the usual level, so that an offset of about half the integer range keeps every I and Q sum of 17 samples positive
    x = (caps.scene(n, nb, seed=5017) * np.float32(0.2)).astype(np.complex64)
    raw = synth.quantize(x, kind)
    if dc:
        raw = _offset(raw, 1000 if raw.dtype == np.int16 else 60)
    fc = 915e6 + 6e6 * np.arange(nb)
    ev = tol.evaluated_mask(n)
    p_ref, _, _ = oracle_mod.Oracle(n, FS, 1e9, kind=kind, enob=enob, correct_dc=dc).run(raw, want_hits=False, threads=8)
    thr = tol.pick_threshold(p_ref, n, start=float(np.quantile(p_ref[:, ev][np.isfinite(p_ref[:, ev])], 0.97)))
    trig_count = 1   # (six evaluated bins: the reference's 1047 would never trigger)
    p_ref, h_ref, t_ref = oracle_mod.Oracle(n, FS, thr, kind=kind, enob=enob, correct_dc=dc, trigger_count=trig_count).run(raw, fc, threads=8)
    assert len(h_ref) > nb // 20 and t_ref.any() and not t_ref.all()
    with Plan(n, FS, thr, kind=kind, enob=enob, correct_dc=dc, max_batch=nb, max_hits=nb * n, trigger_count=trig_count) as plan:
        plan.submit_device(0, _to_dev(gpu, raw), nb, fc)
        p, h, t = plan.collect(0, hit_cap=nb * n)
    fig = tol.compare_spectra(p, p_ref)
    print(f"  against the oracle: {fig}; thr {thr:.3f} dB, {len(h_ref)} records, {int(t_ref.sum())} triggers")
    _assert_hits_equal(h, h_ref, p_ref)
    assert np.array_equal(t, t_ref)


def test_bluestein_stages_pointwise_and_finish_past_the_grid(gpu, cus, oracle_mod):
    """n = 11000: M = 32768 = 2^15, one radix-2, one radix-4 and three radix-16 stages per transform.  The stage, pointwise and
    finish kernels take one item per thread and trip, 8192 CUs threads; the radix-16 stage has the fewest items, M / 16 = 2048 per
    buffer, so 4 CUs buffers fill one trip of it and nb = 2 * 4 CUs + 7 takes every thread of all five kernels round its loop at
    least twice (2055 buffers at 256 CUs: 2.2 GB of double work buffers).  Should the plan refuse that batch, 4 CUs + 7 still loops
    every kernel once (printed).

    The reference is plain float64 (the oracle is too slow for the batch): x * window in float32, numpy's FFT in complex128,
    5 log10 |X|^2, held to compare_spectra; the records exact wherever the bar could not move the bin across the threshold, at most
    2 % of the reference's records exempt.  Six buffers are also held bit for bit, freq_hz included, to the oracle run on them alone:
    buffer b's radix-16 items are g = 2048 b + j, taken on trip g // (8192 CUs) = b // (4 CUs) = b // cap, so 0 and cap - 1 are of the
    first trip, cap and 2 cap - 1 of the second, 2 cap and nb - 1 of the third."""
    n = 11000
    cap = caps.bluestein_stage_cap(cus, n)
    nb = caps.two_trips_and(cap, 7)
    item_cap = caps.bluestein_item_cap(cus)
    assert nb > 2 * cap and all(v > 2 * item_cap for v in caps.bluestein_items(n, nb).values()) and capi.size_path(n) == capi.PATH_BLUESTEIN
    x = caps.scene(n, nb, seed=5000 + n)
    window = oracle_mod.Oracle(n).window()
    db64 = caps.float64_db(x, window)
    ev = tol.evaluated_mask(n)
    six = np.array([0, cap - 1, cap, 2 * cap - 1, 2 * cap, nb - 1])
    assert [caps.trip_of(int(b), cap) for b in six] == [0, 0, 1, 1, 2, 2]
    fc, seq = 433e6 + 6e6 * np.arange(nb), np.arange(nb, dtype=np.uint64)
    held = np.append(six, cap + 6)   # (the fallback batch's last buffer)
    p_held, _, _ = oracle_mod.Oracle(n, FS, 1e9).run(x[held], want_hits=False, threads=7)
    thr = tol.pick_threshold(p_held, n, start=caps.noise_tail_threshold(db64, ev))   # guard-band-free on the buffers held to the oracle
    max_hits = int((db64[:, ev] > thr).sum()) + 65536
    d_x = _to_dev(gpu, x)

    full = nb
    try:
        plan = Plan(n, FS, thr, max_batch=nb, max_hits=max_hits)
    except capi.ScannerError as e:   # plan creation refused the batch: one trip less (a submit that fails is a failure)
        print(f"\nBluestein stages: {nb} buffers refused ({e}); falling back to {cap + 7}")
        nb = cap + 7
        x, db64, fc, seq, six = x[:nb], db64[:nb], fc[:nb], seq[:nb], np.array([0, cap - 1, cap, nb - 1])
        assert all(v > item_cap for v in caps.bluestein_items(n, nb).values())
        plan = Plan(n, FS, thr, max_batch=nb, max_hits=max_hits)
    p6, h6, _ = oracle_mod.Oracle(n, FS, thr).run(x[six], fc[six], seq[six], threads=6)
    with plan:
        plan.submit_device(0, d_x, nb, fc, seq)
        print(f"\nBluestein stages ran at {'the full batch, 2 x 4 CUs + 7' if nb == full else 'the FALLBACK batch, 4 CUs + 7'}")
        print(f"\nBluestein stages, pointwise and finish: n {n} cfloat: {cus} CUs, {item_cap} items per trip, {cap} buffers fill the radix-16 stage's, "
              f"{nb} buffers; trips per kernel { {k: -(-v // item_cap) for k, v in caps.bluestein_items(n, nb).items()} }")
        assert np.array_equal(plan.window(), window)
        p, h, t = plan.collect(0, hit_cap=max_hits)
    _float64_check(p, h, db64, thr, n, 0, f"  Bluestein n {n}")
    counts = _counts(h, 0, nb)
    assert len(np.unique(counts)) > 10
    got6 = h[np.isin(h["seq_id"], six.astype(np.uint64))]
    tol.compare_spectra(p[six], p6)
    _assert_hits_equal(got6, h6, p6, seq[six])
    assert not t.any()   # (the reference's trigger_count, 1047: no buffer comes near)
    print(f"  six buffers {six.tolist()} against the oracle: {len(h6)} records bit for bit; thr {thr:.3f} dB")


# ---- signals --------------------------------------------------------------------------------------------------------------------
def test_signals_beyond_the_block_cap(gpu, cus, oracle_mod):
    """scn_signal_count_kernel and scn_signal_build_kernel take one unit per wave and trip, min(ceil(units / waves), 8192) workgroups
    of `waves` waves (4 at 64 points): 2 * 32768 + 19 units.  Noise with a level of each unit's own, the threshold at the 20 %
    quantile of the units' largest evaluated bins (on the oracle's spectrum), so that about one unit in five has no hit at all: the
    c == 0 path and the window skip on later trips, with the previous unit's maps still in LDS; the scan of the signal counts runs
    over 33 blocks.  (The cap does not depend on the CU count.)"""
    n = 64
    cap = caps.signal_cap(n)
    nb = caps.two_trips_and(cap, 19)
    assert nb > 2 * cap and -(-nb // caps.SCAN_CHUNK) == 33
    print(f"\nsignals: n {n}: {caps.signal_waves(n)} waves per workgroup, {cap} units per trip, {nb} units, {-(-nb // caps.SCAN_CHUNK)} scan blocks")
    rng = np.random.default_rng(64064)
    x = rng.standard_normal((nb, n, 2), dtype=np.float32)
    x *= (0.05 * 10.0 ** rng.uniform(-0.5, 0.5, size=(nb, 1, 1))).astype(np.float32)   # +-10 dB of amplitude, +-5 in the plan's dB = 5 log10 P
    x = x.view(np.complex64).reshape(nb, n)
    ev = tol.evaluated_mask(n, dc_ignore_bins=0)
    p_ref, _, _ = oracle_mod.Oracle(n, FS, 1e9, dc_ignore_bins=0).run(x, want_hits=False, threads=8)
    thr = float(np.float32(np.quantile(p_ref[:, ev].max(axis=1), 0.2)))
    fc = 88e6 + 1e6 * np.arange(nb)
    _, h_ref, _ = oracle_mod.Oracle(n, FS, thr, dc_ignore_bins=0).run(x, fc, want_power=False, threads=8)
    empty = float((np.bincount(h_ref["seq_id"].astype(np.int64), minlength=nb) == 0).mean())
    print(f"  thr {thr:.3f} dB, {len(h_ref)} reference hits, {100 * empty:.1f} % of the units without one")
    assert 0.10 < empty < 0.35
    max_hits = len(h_ref) + 65536
    with Plan(n, FS, thr, max_batch=nb, max_hits=max_hits, dc_ignore_bins=0) as plan:
        plan.submit_device(0, _to_dev(gpu, x), nb, fc)
        _, hits, _ = plan.collect(0, want_power=False, hit_cap=max_hits)
        # the hit list itself: exact outside the guard band
        near = _exact_outside_guard(hits, h_ref, p_ref, n, thr, 0, ev)
        print(f"  {len(hits)} hits, {int(near.sum())} bins in the guard band")
        totals = {}
        for gap in (0, 1, 31, 32, 64):
            got = plan.collect_signals(0, gap)
            want = signals_ref.signals(hits, n, FS, gap)
            signals_ref.assert_same(got, capi.signals_from_hits(hits, n, FS, gap), f"n {n} max_gap {gap}: GPU against scn_signals_from_hits")
            signals_ref.assert_same(got, want, f"n {n} max_gap {gap}: GPU against the numpy reference")
            assert int(got["n_hits"].sum()) == len(hits)
            totals[gap] = len(want)
            if gap not in (1, 64):
                continue
            # a window that starts inside the second trip's units: to the end, and a bounded one that ends inside the third trip's
            a = int(np.searchsorted(want["seq_id"], cap + 1001))
            while gap < n and want["seq_id"][a] != want["seq_id"][a - 1]:   # (in the middle of a unit, where units have several signals)
                a += 1
            b = int(np.searchsorted(want["seq_id"], 2 * cap + 9))
            assert caps.trip_of(int(want["seq_id"][a]), cap) == 1 and caps.trip_of(int(want["seq_id"][b - 1]), cap) == 2 and b - a > cap // 2
            signals_ref.assert_same(plan.collect_signals(0, gap, first=a), want[a:], f"max_gap {gap}: from a unit of the second trip to the end")
            out = np.zeros(b - a + 2, capi.SIGNAL_DTYPE)
            out["n_hits"] = 0xDEADBEEF
            n_sig = C.c_uint32()
            st = capi.lib().scn_collect_signals(plan.handle, 0, gap, a, out.ctypes.data_as(C.c_void_p), b - a, C.byref(n_sig))
            assert (st, n_sig.value) == (capi.E_TRUNCATED, len(want))
            signals_ref.assert_same(out[: b - a], want[a:b], f"max_gap {gap}: a window from the second trip's units into the third's")
            assert np.all(out["n_hits"][b - a:] == 0xDEADBEEF)
        assert totals[64] == len(np.unique(hits["seq_id"])) and totals[0] > totals[1] > totals[31] >= totals[32] >= totals[64]
        print(f"  signals by max_gap: {totals}")


# ---- convert --------------------------------------------------------------------------------------------------------------------
def _convert_batch(n, nb, kind, seed):
    """raw integer buffers, each with an offset of its own on each rail; buffers 3, 13, 23, ... have a negative I sum, 7, 17, 27, ... a
    negative Q sum (with DC removal the `int32 /= uint32` quirk of utility.cpp:77-78 then rides along on every trip)"""
    rng = np.random.default_rng(seed)
    a, lo, hi = (20, 8, 40) if kind == I8 else (100, 40, 400)
    raw = rng.integers(-a, a + 1, size=(nb, n, 2)).astype(np.int32)
    off = rng.integers(lo, hi + 1, size=(nb, 1, 2))
    off[3::10, :, 0] *= -1
    off[7::10, :, 1] *= -1
    raw = (raw + off).astype(np.int8 if kind == I8 else np.int16)
    sums = raw.astype(np.int64).sum(axis=1)
    neg = (sums < 0)
    assert np.array_equal(np.flatnonzero(neg[:, 0]), np.arange(3, nb, 10)) and np.array_equal(np.flatnonzero(neg[:, 1]), np.arange(7, nb, 10))
    assert len(np.unique(sums[:, 0])) > nb // 2
    if kind == I16P:
        raw = np.ascontiguousarray(np.moveaxis(raw, -1, -2))   # planar: I[n] then Q[n]
    return raw


@pytest.mark.parametrize("dc", [False, True], ids=["", "dc"])
@pytest.mark.parametrize("kind,enob", [(I16, 12), (I16P, 14), (I8, 8)], ids=["int16", "int16planar", "int8"])
@pytest.mark.parametrize("n", [100, 4096])
def test_convert_beyond_the_block_cap(gpu, oracle_mod, n, kind, enob, dc):
    """scn_convert_kernel takes one buffer per workgroup and trip, min(nb, 2048) workgroups: 2 * 2048 + 13 buffers, bit for bit against
    the oracle's convert (itself pinned to the reference's utility.cpp).  (The cap does not depend on the CU count.)"""
    cap = caps.convert_cap()
    nb = caps.two_trips_and(cap, 13)
    assert nb > 2 * cap
    raw = _convert_batch(n, nb, kind, seed=n + 10 * kind)
    o = oracle_mod.Oracle(n, FS, 0.0, kind=kind, enob=enob, correct_dc=dc)
    flat = raw.reshape(nb, -1)
    ref = np.stack([o.convert(flat[b]) for b in range(nb)])
    if dc:   # the quirk is in play on the marked buffers, and only there
        big = np.abs(ref.real).min(axis=1) > 30
        assert np.array_equal(np.flatnonzero(big), np.arange(3, nb, 10))
    with Plan(n, FS, 0.0, kind=kind, enob=enob, correct_dc=dc, max_batch=1) as plan:
        got = plan.convert_raw(raw)
    same = got.view(np.uint32) == ref.view(np.uint32)
    bad = np.flatnonzero(~same.all(axis=1))
    print(f"\nconvert: n {n} {NAMES[kind]} dc {dc}: {cap} workgroups, {nb} buffers, {len(bad)} buffers differ (largest |difference| "
          f"{float(np.abs(got - ref).max()):.3g})")
    assert bad.size == 0, (bad[:8].tolist(), [caps.trip_of(int(b), cap) for b in bad[:8]])
