"""Averaged plans on the GPU (scn_plan_desc.average = K > 1, scn_average.hip): a group's spectrum is the mean of its K buffers'
periodograms, and detection runs once per group.  References: float64 (the oracle's converters and window, numpy's FFT in
double, the mean of |X|^2) held to the parity bar of tests/tolerances.py, and a float32 restatement from the oracle's FFT."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from scanner_amd import Plan, capi, synth
from tests import tolerances as tol

pytestmark = pytest.mark.gpu

FS = 8000000
KINDS = [capi.KIND_FLOAT_COMPLEX, capi.KIND_SHORT_COMPLEX, capi.KIND_SHORT, capi.KIND_BYTE_COMPLEX]
WG_PER_CU = {1024: 12, 2048: 6, 4096: 3, 8192: 2}  # resident workgroups per CU of the accumulation kernel (scn_average.hip)


def _enob(kind):
    return 8 if kind == capi.KIND_BYTE_COMPLEX else 12


def _members(g, G, K, layout):
    return g + G * np.arange(K) if layout == capi.AVG_SWEEPS else g * K + np.arange(K)


def _signal(n, G, K, layout, seed, tone_amp=0.3):
    """Buffers with a gain of their own and a tone at a bin of their GROUP: a buffer taken into the wrong group moves whole
    dB.  complex64 [G*K, n]."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((G * K, n, 2), dtype=np.float32) * np.float32(0.05)).view(np.complex64).reshape(G * K, n)
    t = np.arange(n)
    for g in range(G):
        f = 16 + (97 * g + 13) % (n // 4)  # natural bin: in band, away from DC
        for b in _members(g, G, K, layout):
            x[b] += (tone_amp * np.exp(2j * np.pi * (f + 0.25) * t / n)).astype(np.complex64)
            x[b] *= np.float32(rng.uniform(0.4, 1.0))
    return x


def _convert(oracle_mod, n, kind, dc, raw, enob=12):
    o = oracle_mod.Oracle(n, FS, kind=kind, enob=enob, correct_dc=dc)
    return np.stack([o.convert(raw[b]) for b in range(raw.shape[0])]), o


def _ref64(oracle_mod, n, kind, dc, raw, G, K, layout, enob=12):
    """float64 mean power and its dB per group, [G, n]"""
    conv, o = _convert(oracle_mod, n, kind, dc, raw, enob)
    _, P, _ = oracle_mod.ref64_spectrum(conv, o.window())
    Pm = np.stack([P[_members(g, G, K, layout)].mean(axis=0) for g in range(G)])
    with np.errstate(divide="ignore"):
        return Pm, 5.0 * np.log10(Pm)


def _ref32(oracle_mod, n, kind, dc, raw, G, K, layout, enob=12):
    """float32 restatement: the oracle's float32 FFT, |X|^2 in float, summed in the group's order, divided by K"""
    conv, o = _convert(oracle_mod, n, kind, dc, raw, enob)
    w = o.window()
    out = np.empty((G, n), np.float64)
    for g in range(G):
        acc = np.zeros(n, np.float32)
        for b in _members(g, G, K, layout):
            X = o.fft((conv[b] * w).astype(np.complex64))
            acc = acc + (X.real * X.real + X.imag * X.imag).astype(np.float32)
        with np.errstate(divide="ignore"):
            out[g] = 5.0 * np.log10((acc / np.float32(K)).astype(np.float64))
    return out


def _expected_hits(db64, n, threshold, fc_groups, seq_groups, trigger_count=1047):
    """process_fft's mask and threshold over the float64 average, per group (process.cpp:36-64)"""
    mask = tol.evaluated_mask(n)
    evaluated = np.concatenate([db64[g][mask] for g in range(db64.shape[0])])
    assert not np.any(np.abs(evaluated - threshold) < tol.GUARD_DB), "a bin sits within the guard band of the threshold"
    recs, trig = [], []
    bin_step = FS // n
    for g in range(db64.shape[0]):
        i = np.arange(n)
        j = (i + n // 2) % n
        hit = mask[j] & (db64[g][j] > threshold)
        start = fc_groups[g] - float(FS // 2)
        for ii in i[hit]:
            recs.append((int(seq_groups[g]), int(ii), int(start + float(np.uint32(ii * bin_step)))))
        trig.append(int(hit.sum() > trigger_count))
    return recs, np.array(trig, np.uint8)


def _hits_tuples(h):
    return [(int(a), int(b), int(c)) for a, b, c in zip(h["seq_id"], h["i"], h["freq_hz"])]


def _run(plan, raw_np, nb, fc=None, seq=None, d_power=None, first_index=None, slot=0):
    d_raw = torch.from_numpy(np.ascontiguousarray(raw_np).view(np.uint8).reshape(-1)).cuda()
    plan.submit_device(slot, d_raw, nb, center_freqs=fc, seq_ids=seq, d_power_db=d_power, first_index=first_index)
    return plan.collect(slot)


def _threshold(db64, n, start):
    return tol.pick_threshold(db64, n, start=start)


@pytest.mark.parametrize("dc", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1024, 2048, 4096, 8192])
def test_matches_references(oracle_mod, built_lib, n, kind, dc):
    G, K = 3, 4
    x = _signal(n, G, K, capi.AVG_DWELL, seed=n + 10 * kind + dc)
    if dc:
        # a DC offset for the integer kinds to remove, per buffer (positive: a negative sum would take the reference's
        # int32 /= uint32 quirk, whose 2e6-sized offset leaves the bins near DC as cancellation residue)
        x = x + np.complex64(0.07 + 0.05j)
    raw = synth.quantize(x, kind)
    Pm, db64 = _ref64(oracle_mod, n, kind, dc, raw, G, K, capi.AVG_DWELL, enob=_enob(kind))
    thr = _threshold(db64, n, 12.0)
    fc = np.repeat(1e9 + 7e6 * np.arange(G), K)
    seq = np.arange(1000, 1000 + G * K, dtype=np.uint64)
    with Plan(n, FS, thr, kind=kind, enob=_enob(kind), correct_dc=dc, max_batch=G * K, average=K) as plan:
        p, h, t = _run(plan, raw, G * K, fc, seq)
    assert p.shape == (G, n) and t.shape == (G,)
    tol.compare_spectra(p, db64)
    tol.compare_spectra(p, _ref32(oracle_mod, n, kind, dc, raw, G, K, capi.AVG_DWELL, enob=_enob(kind)))
    recs, trig = _expected_hits(db64, n, thr, fc[::K], seq[::K])
    assert len(recs) > 0
    assert _hits_tuples(h) == recs
    assert np.array_equal(t, trig)
    # the tone of each group sits where its group put it: a buffer of another group would add a second peak
    mask = tol.evaluated_mask(n)
    for g in range(G):
        assert np.sum(p[g][mask] > thr) == np.sum(db64[g][mask] > thr)


def test_averaging_reduces_noise_spread(built_lib):
    n, K = 4096, 16
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((K, n, 2), dtype=np.float32) * np.float32(0.05)).view(np.complex64).reshape(K, n)
    mask = tol.evaluated_mask(n)
    with Plan(n, FS, 1e9, max_batch=K) as plain:
        p1, _, _ = _run(plain, x, K)
    with Plan(n, FS, 1e9, max_batch=K, average=K) as avg:
        pk, _, _ = _run(avg, x, K)
    one = float(np.mean([np.std(p1[b][mask]) for b in range(K)]))
    avgd = float(np.std(pk[0][mask]))
    assert 2.3 < one < 3.3, one  # one periodogram: 5.6 dB in 10 log10 P, i.e. 2.8 dB on this map (5 log10 P)
    assert avgd < 0.3 * one, (one, avgd)  # K = 16: ~0.55 dB


def test_dwell_and_sweeps_agree(built_lib):
    n, G, K = 2048, 5, 6
    kind = capi.KIND_SHORT_COMPLEX
    x = synth.quantize(_signal(n, G, K, capi.AVG_DWELL, seed=3), kind)
    perm = np.array([g * K + k for k in range(K) for g in range(G)])  # sweeps position g + k G holds dwell buffer g K + k
    fc = np.repeat(2e9 + 5e6 * np.arange(G), K)
    seq = np.arange(G * K, dtype=np.uint64) * 3 + 11
    with Plan(n, FS, 12.0, kind=kind, max_batch=G * K, average=K) as dwell:
        pd, hd, td = _run(dwell, x, G * K, fc, seq)
    with Plan(n, FS, 12.0, kind=kind, max_batch=G * K, average=K, average_layout=capi.AVG_SWEEPS) as sweeps:
        ps, hs, ts = _run(sweeps, x[perm], G * K, fc[perm], seq[perm])
    assert len(hd) > 0
    assert pd.tobytes() == ps.tobytes()
    assert hd.tobytes() == hs.tobytes()
    assert np.array_equal(td, ts)
    # seq_ids NULL: a group's id is the index of its first buffer (g K for dwell, g for sweeps)
    with Plan(n, FS, 12.0, kind=kind, max_batch=G * K, average=K) as dwell:
        _, h0, _ = _run(dwell, x, G * K, fc)
    with Plan(n, FS, 12.0, kind=kind, max_batch=G * K, average=K, average_layout=capi.AVG_SWEEPS) as sweeps:
        _, h1, _ = _run(sweeps, x[perm], G * K, fc[perm])
    assert set(h0["seq_id"].tolist()) <= {g * K for g in range(G)} and set(h1["seq_id"].tolist()) <= set(range(G))
    assert np.array_equal(h0["seq_id"] // K, h1["seq_id"]) and np.array_equal(h0["i"], h1["i"])


@pytest.mark.parametrize("layout", [capi.AVG_DWELL, capi.AVG_SWEEPS])
def test_indexed_submits_follow_the_table(built_lib, layout):
    n, G, K, count, first = 1024, 4, 3, 5, 3
    x = synth.quantize(_signal(n, G, K, layout, seed=9), capi.KIND_BYTE_COMPLEX)
    table = 1e9 + 11e6 * np.arange(count)
    with Plan(n, FS, 12.0, kind=capi.KIND_BYTE_COMPLEX, enob=8, max_batch=G * K, average=K, average_layout=layout) as plan:
        plan.set_table(table)
        _, hi, ti = _run(plan, x, G * K, first_index=first)
        fc_groups = table[(first + np.arange(G)) % count]  # group 2 and 3 wrap round
        fc = np.empty(G * K)
        for g in range(G):
            fc[_members(g, G, K, layout)] = fc_groups[g]
        _, hf, tf = _run(plan, x, G * K, fc)
    assert len(hi) > 0 and hi.tobytes() == hf.tobytes() and np.array_equal(ti, tf)
    g_of = hi["seq_id"] if layout == capi.AVG_SWEEPS else hi["seq_id"] // K
    expect = (fc_groups[g_of] - FS // 2 + (hi["i"].astype(np.uint64) * (FS // n)).astype(np.float64)).astype(np.uint64)
    assert np.array_equal(hi["freq_hz"], expect)
    assert set(g_of.tolist()) == set(range(G))


@pytest.mark.parametrize("n,kind,G,K", [
    (4096, capi.KIND_SHORT_COMPLEX, 1, 7),
    (4096, capi.KIND_SHORT_COMPLEX, 1, 64),
    (1024, capi.KIND_FLOAT_COMPLEX, 1, 8192),
    (2048, capi.KIND_BYTE_COMPLEX, 3, 5),
    (1024, capi.KIND_SHORT, 2000, 2),
    (8192, capi.KIND_SHORT_COMPLEX, 1, 33),
    (8192, capi.KIND_BYTE_COMPLEX, 700, 2),
])
def test_splits_match_the_references(oracle_mod, built_lib, n, kind, G, K):
    layout = capi.AVG_DWELL
    x = _signal(n, G, K, layout, seed=G * 1000 + K)
    raw = synth.quantize(x, kind)
    Pm, db64 = _ref64(oracle_mod, n, kind, False, raw, G, K, layout, enob=_enob(kind))
    thr = _threshold(db64, n, 12.0)
    fc = np.repeat(3e8 + 1e6 * np.arange(G), K)
    with Plan(n, FS, thr, kind=kind, enob=_enob(kind), max_batch=G * K, average=K,
              max_hits=1 << 20) as plan:
        parts = plan.average_parts(G * K)
        slots = torch.cuda.get_device_properties(0).multi_processor_count * WG_PER_CU[n]
        want = 1 if G >= slots else min(math.ceil(slots / G), (K + 1) // 2)
        assert parts == want, (parts, want)
        p, h, t = _run(plan, raw, G * K, fc)
        p2, h2, t2 = _run(plan, raw, G * K, fc)  # deterministic: the same bits again
    if G == 1:
        assert parts > 1
    assert p.tobytes() == p2.tobytes() and h.tobytes() == h2.tobytes() and np.array_equal(t, t2)
    tol.compare_spectra(p, db64)
    if G * K <= 64:
        tol.compare_spectra(p, _ref32(oracle_mod, n, kind, False, raw, G, K, layout, enob=_enob(kind)))
    recs, trig = _expected_hits(db64, n, thr, fc[::K], np.arange(G) * K)
    assert _hits_tuples(h) == recs and np.array_equal(t, trig)


@pytest.mark.parametrize("n,G,K", [(4096, 1, 64), (4096, 8, 2), (4096, 800, 2), (8192, 1, 64), (8192, 600, 2)])
def test_output_modes_agree(built_lib, n, G, K):
    x = synth.quantize(_signal(n, G, K, capi.AVG_DWELL, seed=77, tone_amp=0.5), capi.KIND_SHORT_COMPLEX)
    fc = np.repeat(1e9 + 1e6 * np.arange(G), K)
    out = {}
    for name, flags in (("both", capi.OUT_SPECTRUM | capi.OUT_HITS), ("spec", capi.OUT_SPECTRUM), ("hits", capi.OUT_HITS)):
        # a threshold near the noise floor: many hits, strong (exact-map) and weak bins among them
        with Plan(n, FS, 1.5, kind=capi.KIND_SHORT_COMPLEX, max_batch=G * K, average=K, flags=flags, max_hits=1 << 20) as plan:
            out[name] = _run(plan, x, G * K, fc)
    assert len(out["both"][1]) > 20
    assert out["spec"][0].tobytes() == out["both"][0].tobytes()
    assert out["hits"][1].tobytes() == out["both"][1].tobytes()
    assert np.array_equal(out["hits"][2], out["both"][2])


def test_pinned_and_device_submits_agree_in_every_slot(built_lib):
    n, G, K = 2048, 6, 4
    kind = capi.KIND_SHORT
    inputs = [synth.quantize(_signal(n, G, K, capi.AVG_SWEEPS, seed=100 + s), kind) for s in range(capi.NUM_SLOTS)]
    fcs = np.tile(5e8 + 2e6 * np.arange(G), K)  # sweeps: buffer b belongs to group b % G
    with Plan(n, FS, 12.0, kind=kind, correct_dc=True, max_batch=G * K, average=K, average_layout=capi.AVG_SWEEPS) as plan:
        for s in range(capi.NUM_SLOTS):  # every slot in flight at once
            hb = plan.host_buffer(s)
            hb[: inputs[s].nbytes] = np.ascontiguousarray(inputs[s]).view(np.uint8).reshape(-1)
            plan.submit(s, G * K, fcs)
        pinned = [plan.collect(s) for s in range(capi.NUM_SLOTS)]
        dev = [_run(plan, inputs[s], G * K, fcs, slot=s) for s in range(capi.NUM_SLOTS)]
    for s in range(capi.NUM_SLOTS):
        assert pinned[s][0].tobytes() == dev[s][0].tobytes()
        assert pinned[s][1].tobytes() == dev[s][1].tobytes() and len(dev[s][1]) > 0
        assert np.array_equal(pinned[s][2], dev[s][2])


def test_wideband_burst_hit_lists(built_lib):
    n, G, K = 2048, 3, 4
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((G * K, n, 2), dtype=np.float32) * np.float32(0.3)).view(np.complex64).reshape(G * K, n)
    fc = np.repeat(1e9 + 1e7 * np.arange(G), K)
    per = int(tol.evaluated_mask(n).sum())
    assert per > 1047
    with Plan(n, FS, -50.0, max_batch=G * K, average=K, max_hits=1000) as plan:
        d_raw = torch.from_numpy(x.view(np.uint8).reshape(-1)).cuda()
        plan.submit_device(0, d_raw, G * K, center_freqs=fc)
        with pytest.raises(capi.ScannerError) as e:
            plan.collect(0, hit_cap=500)
        assert e.value.status == capi.E_TRUNCATED and plan.last_n_hits == G * per
        view = plan.hits_view(0)
        assert len(view) == 1000
        rest = plan.collect_more(0, 0, G * per)
        assert len(rest) == G * per and rest[:1000].tobytes() == view.tobytes()
        plan.submit_device(0, d_raw, G * K, center_freqs=fc)
        _, h, t = plan.collect(0)
    assert h.tobytes() == rest.tobytes()
    assert np.array_equal(t, np.ones(G, np.uint8))
    mask = tol.evaluated_mask(n)
    i_all = np.array([i for i in range(n) if mask[(i + n // 2) % n]])
    for g in range(G):
        sel = h[g * per:(g + 1) * per]
        assert np.all(sel["seq_id"] == g * K) and np.array_equal(sel["i"], i_all)


@pytest.mark.parametrize("n", [64, 512, 4096, 8192, 16384, 1000, 32768, 1001])
def test_average_one_is_the_plain_plan(built_lib, n):
    nb = 4
    x = synth.cfloat_batch(n, nb, seed=n)
    fc = 1e9 + 1e6 * np.arange(nb)
    with Plan(n, FS, 0.0, max_batch=nb) as plain:
        a = _run(plain, x, nb, fc)
    with Plan(n, FS, 0.0, max_batch=nb, average=1, average_layout=capi.AVG_SWEEPS) as one:
        b = _run(one, x, nb, fc)
        assert one.average_parts(nb) == 1
    assert len(a[1]) > 0
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("n,K", [(1024, 3), (4096, 16)])
def test_identical_copies_match_the_plain_plan(built_lib, n, K):
    x = _signal(n, 1, 1, capi.AVG_DWELL, seed=4)
    with Plan(n, FS, 1e9, max_batch=1) as plain:
        p1, _, _ = _run(plain, x, 1)
    thr = tol.pick_threshold(p1, n, start=12.0)
    with Plan(n, FS, thr, max_batch=1) as plain:
        p1, h1, t1 = _run(plain, x, 1, [2e9])
    with Plan(n, FS, thr, max_batch=K, average=K) as avg:
        pk, hk, tk = _run(avg, np.repeat(x, K, axis=0), K, np.full(K, 2e9))
    tol.compare_spectra(pk, p1)
    assert len(h1) > 0 and _hits_tuples(hk) == _hits_tuples(h1) and np.array_equal(tk, t1)


def test_rejected_submits(built_lib):
    n, K = 1024, 4
    x = synth.cfloat_batch(n, 8, seed=2)
    d_raw = torch.from_numpy(x.view(np.uint8).reshape(-1)).cuda()
    L = capi.lib()
    with Plan(n, FS, 10.0, max_batch=8, average=K) as plan:
        with pytest.raises(capi.ScannerError) as e:
            plan.submit_device(0, d_raw, 6, center_freqs=np.zeros(6))
        assert e.value.status == capi.E_INVALID and b"multiple of average" in L.scn_last_error()
        fc = np.zeros(8)
        fc[5] = 1.0
        with pytest.raises(capi.ScannerError) as e:
            plan.submit_device(0, d_raw, 8, center_freqs=fc)
        assert e.value.status == capi.E_INVALID and b"differ inside group 1" in L.scn_last_error()
        plan.submit_device(0, d_raw, 8, center_freqs=np.zeros(8))  # the slot is still usable
        with pytest.raises(capi.ScannerError) as e:
            plan.collect_time_domain(0)
        assert e.value.status == capi.E_INVALID
        p, _, t = plan.collect(0)
        assert p.shape == (2, n) and t.shape == (2,)
        parts = C.c_uint32()
        assert L.scn_plan_average_parts(plan.handle, 6, C.byref(parts)) == capi.E_INVALID
