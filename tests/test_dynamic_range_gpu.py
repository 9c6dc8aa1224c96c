"""Weak bins under a strong signal, in every kernel family, against float64: the floor criterion of tests/tolerances.py floor_errors
on the high-dynamic-range scenes of tests/dr_scenes.py (a 0.5-amplitude blocker, noise 74 dB below it, weak tones in the noise;
pinned on the host by tests/test_dynamic_range_cpu.py).  88 % of such a spectrum at 64 points and more than 99 % from 4096 up lie
below 1e-5 of the buffer's mean power, where compare_spectra allows an error of a hundred times the bin and flip_unsafe drops the bin
from the hit comparison: a fast-sine twiddle table, a float pass where DESIGN.md promises double, a slightly wrong W_3 / W_5 would
pass every other module of the suite while raising the floor by tens of dB.

WHAT A SINGLE TABLE ENTRY DOES (measured on an MI355X with one entry of one table moved ten float ulp, 6e-7; tests/test_parity_gpu.py
passed under every one of these):  an entry that carries the share s of a buffer's energy adds 6e-7 sqrt(s) of the rms level, spread
over the bins it feeds, and Y -- the rounding of a whole float32 transform -- grows with the size.  So the module FAILS for any pass-1
entry at 64 points (three entries tried: ratio 2.13 ... 2.22 against 1.11) and for a pass-2 entry (the W_n table a workgroup shares)
at 512 and 1024 points (2.2 ... 4.4 in every launch of the size), and it does NOT see: a pass-1 entry from 512 points up (one thread's
constant, 1/32 ... 1/512 of the input: ratios unchanged to two digits at 512, 1024, 4096, 8192, 16384); a pass-2 entry at 4096 (four
tried: 1.06 ... 1.55, one of them 2.13 in the averaged K = 16 launches only), 8192 and 16384 points.  There a ten-ulp entry is below
what two correct float32 transforms differ by; no criterion measured against float32 transforms can hold it.  A table that is coarse
THROUGHOUT (every entry a few ulp off) adds up over the entries and is seen at every size.

The figures are maxima over all floor bins of a launch against twice another maximum, on fixed seeds: stable on one build, but wire
formats that carry the same arithmetic range over 1.06 ... 1.89 at 8192 points (32 buffers), so another seed or launch shape can cross
2 there with no kernel changed.  8192 is the largest size whose last pass is float and sits nearest the bar in this criterion as in
the first; a failure there after a change of seed is to be read against the other wire formats of the size.

Per launch (about 2^18 samples; 37 extra buffers up to 512 points so that the last workgroup's buffer slots stay partly empty):
  * the float64 reference: numpy's FFT in complex128 of the FLOAT32 product x * w (x through the oracle's converter, bit-pinned to
    the reference's utility.cpp; w = plan.window(), asserted equal to the oracle's), averaged plans: the mean over the K copies of
    the float64 powers; Welch: oracle.ref64_welch;
  * the yardstick Y of the launch: the larger floor_errors figure, ON THE SAME BUFFERS, of two float32 transforms that are not the
    kernel under test -- the oracle's chain through Oracle.run (default mode) and scipy.fft on complex64 (float32_chain of
    tests/test_oracle_vs_pocketfft.py); at lengths that are not powers of two the oracle computes in double and scipy alone supplies
    it.  (The oracle's default mode accumulates in double: its figure is 0 and Y is pocketfft's -- tests/test_dynamic_range_cpu.py.)
  * asserted: the scene's floor-bin share (dr_scenes.assert_floor_share); floor_errors <= 2 Y (the factor of the tone sweep's eps in
    tests/test_db_map_gpu.py); compare_spectra on the same output, so that the strong bins stay held;
  * hit lists at a threshold of twice the median floor amplitude of the float64 spectrum (6 dB over the floor: the noise tail, the
    weak tones and the blocker's main lobe report): a bin is exempt only where |a64 - a_thr| <= 2 Y rms; everywhere else the
    records' (seq_id, i, freq_hz), their order and the trigger flags are what the float64 spectrum owes; the exempt share of a
    launch's evaluated bins must stay <= 5 % (it FAILS above, it does not skip); spectrum + hits and hits-only plans report
    byte-identical records, and a record carries the float the spectrum holds.

Covered: every fused power of two 16 ... 16384, every mixed-radix size the library runs fused, 32768 / 65536 (four-step), Bluestein at
17 / 1023 / 4097 / 20000 / 65535 in cfloat; int16 interleaved and planar at ENOB 12 and 16, DC removal off and on (a positive mean),
at one size per family (128, 512, 4096, 8192, 16384, 6000, 12000, 65536, 1023); averaged plans at 1024 ... 8192 points with K = 2
and 16 in both layouts (K = 16 takes the split-over-workgroups path: asserted from Plan.average_parts); one Welch submit of four
PSDs in cfloat and int16.  int8 is left out: its quantisation floor is 4e-5 of the mean, which the old bar sees.

MODULE STATE: the figures are a module global filled in test order; test_zz_figures prints the table (run with -rP or -s) and
asserts the totals only where the whole module ran."""
import numpy as np
import pytest

from scanner_amd import Plan, WelchPlan, build, capi
from tests import dr_scenes as sc
from tests import tolerances as tol

pytestmark = pytest.mark.gpu
FS = 8000000
SEQ0 = 1 << 33
BOTH, HITS = capi.OUT_SPECTRUM | capi.OUT_HITS, capi.OUT_HITS
CF, I16, I16P = capi.KIND_FLOAT_COMPLEX, capi.KIND_SHORT_COMPLEX, capi.KIND_SHORT
NAMES = {CF: "cfloat", I16: "int16", I16P: "int16planar"}
MAX_EXEMPT = 0.05

build.build()  # (collection needs scn_size_path; seconds when the library is current, and it needs no GPU)
POW2, MIXED = sc.fused_sizes()
INT_SIZES = [128, 512, 4096, 8192, 16384, 6000, 12000, 65536, 1023]
WIRE = [(k, e, dc) for k in (I16, I16P) for e in (12, 16) for dc in (False, True)]
CASES = [(n, CF, 12, False) for n in sc.spectrum_sizes()] + [(n, *f) for n in INT_SIZES for f in WIRE]
AVG = [(n, k, lay) for n in (1024, 2048, 4096, 8192) for k in (2, 16) for lay in (capi.AVG_DWELL, capi.AVG_SWEEPS)]

_FIG = {}   # (family, wire format) -> list of (label, kernel figure, Y, floor share, exempt share)


def family(n):
    if n in sc.BLUESTEIN_SIZES:
        return "bluestein"
    if n in sc.FOUR_STEP_SIZES:
        return "four-step"
    if n in MIXED:
        return "mixed >= 10240" if n >= 10240 else "mixed < 10240"
    return "16 ... 128" if n <= 128 else "256, 512" if n <= 512 else "1024 ... 4096" if n <= 4096 else str(n)


def _wire_name(kind, enob, dc):
    return NAMES[kind] + ("" if kind == CF else f"/enob{enob}") + ("/dc" if dc else "")


def _dev(raw):
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need a GPU; refusing to skip silently"
    return torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).reshape(-1)).cuda()


def _count(n):
    return max(2, (1 << 18) // n) + (37 if n <= 512 else 0)


def _threshold(a64):
    """twice the median floor amplitude of the float64 spectra of the launch, as the float32 dB value a plan takes; and the amplitude
    that float stands for"""
    P = a64 * a64
    floor = P < tol.REL_POWER * P.mean(axis=1, keepdims=True)
    thr = np.float32(10.0 * np.log10(2.0 * np.median(a64[floor])))
    return float(thr), 10.0 ** (float(thr) / 10.0)


def _owed(a64, n, a_thr, Y):
    """(owes, exempt) boolean [G, n] over natural bins: the evaluated bins the float64 spectrum puts above the threshold, and those
    within 2 Y rms of it"""
    ev = tol.evaluated_mask(n)[None, :]
    rms = np.sqrt((a64 * a64).mean(axis=1, keepdims=True))
    return ev & (a64 > a_thr), ev & (np.abs(a64 - a_thr) <= 2.0 * Y * rms)


def _check_hits(h, t, p, n, owes, exempt, fc_g, seq_g, trig_count, what):
    """the records h and trigger flags t of one launch against what the float64 spectrum owes; returns the exempt share"""
    G = owes.shape[0]
    n_ev = int(tol.evaluated_mask(n).sum())
    share = float(exempt.sum()) / (G * n_ev)
    assert share <= MAX_EXEMPT, f"{what}: {share:.2%} of the evaluated bins lie within 2 Y rms of the threshold"
    g = np.searchsorted(seq_g, h["seq_id"])
    assert (g < G).all() and np.array_equal(seq_g[g], h["seq_id"]), f"{what}: a record's seq_id is no group's"
    i = h["i"].astype(np.int64)
    assert (i < n).all()
    key = g.astype(np.int64) * n + i
    assert (np.diff(key) > 0).all(), f"{what}: the records are not ordered by (buffer, i), each once"
    j = (i + n // 2) % n
    got = np.zeros(owes.shape, bool)
    got[g, j] = True
    assert tol.evaluated_mask(n)[j].all(), f"{what}: a record outside the evaluated band"
    bad = (got != owes) & ~exempt
    assert not bad.any(), (f"{what}: {int(bad.sum())} bins outside the exempt band differ from float64 "
                           f"({int((bad & got).sum())} reported and not owed, {int((bad & owes).sum())} owed and not reported); first (group, j): "
                           f"{np.argwhere(bad)[:6].tolist()}")
    start = fc_g[g] - float(FS // 2)
    want_f = (start + ((i * (FS // n)) & 0xFFFFFFFF).astype(np.float64)).astype(np.uint64)   # process.cpp:38-39, 55-57
    assert np.array_equal(h["freq_hz"], want_f), f"{what}: freq_hz"
    if p is not None:
        assert h["power_db"].tobytes() == p[g, j].tobytes(), f"{what}: a record carries the float the spectrum holds"
    lo = (owes & ~exempt).sum(axis=1)
    hi = lo + exempt.sum(axis=1)
    safe = (lo > trig_count) | (hi <= trig_count)     # the exempt bins cannot move the count across trigger_count
    assert np.array_equal(t[safe], (lo > trig_count).astype(np.uint8)[safe]), f"{what}: trigger flags against float64"
    assert np.array_equal(t, (got.sum(axis=1) > trig_count).astype(np.uint8)), f"{what}: trigger flags follow the counts (process.cpp:62)"
    return share


def _launch_and_check(oracle_mod, n, kind, enob, dc, raw, conv, copies, layout, label, fam):
    """both plans of one launch against the float64 reference of its buffers; notes the figures"""
    sweeps = layout == capi.AVG_SWEEPS
    nb = len(conv)
    G = nb // copies
    fc_g = 70e6 + 6e6 * np.arange(G)
    fc = np.tile(fc_g, copies) if sweeps else np.repeat(fc_g, copies)
    seq = np.arange(nb, dtype=np.uint64) + np.uint64(SEQ0)
    seq_g = seq[:G] if sweeps else seq[::copies]       # a group's id is its first buffer's
    d_raw = _dev(raw)
    common = dict(kind=kind, enob=enob, correct_dc=dc, max_batch=nb, average=copies, average_layout=layout)
    with Plan(n, FS, 1e9, flags=capi.OUT_SPECTRUM, **common) as plan:     # the plan's own window, and its report of the split
        w = plan.window()
        got = {"parts": plan.average_parts(nb) if copies > 1 else 1}
    assert np.array_equal(w, oracle_mod.Oracle(n).window())
    a64 = np.sqrt(sc.group_mean(sc.ref64_power(conv, w), copies, sweeps))
    Y, _ = sc.yardstick(tol, sc.float32_dbs(oracle_mod, n, kind, enob, dc, raw, conv, w), a64, copies, sweeps)
    thr, a_thr = _threshold(a64)
    owes, exempt = _owed(a64, n, a_thr, Y)
    got["trig"] = max(1, int(np.median(owes.sum(axis=1))))    # about half of the flags set
    cap = int(owes.sum() + exempt.sum()) + 4096
    for flags, slot in ((BOTH, 0), (HITS, 1)):
        with Plan(n, FS, thr, flags=flags, max_hits=cap, trigger_count=got["trig"], **common) as plan:
            plan.submit_device(slot, d_raw, nb, fc, seq)
            got[flags] = plan.collect(slot)
    p, h, t = got[BOTH]
    ph, hh, th = got[HITS]
    assert p.shape == a64.shape and ph is None
    fig = tol.floor_errors(p, a64)
    sc.assert_floor_share(n, fig["floor_share"])
    with np.errstate(divide="ignore"):
        cmp = tol.compare_spectra(p, 10.0 * np.log10(a64))
    # (6 dB over the median floor is one noise bin in 16 of a single periodogram -- thousands of records; the mean of 16 periodograms
    #  hardly reaches it, and an averaged launch reports the weak tones and the blocker's main lobe: 66 ... 286 records)
    assert owes.sum() >= (200 if copies == 1 else 50), f"{label}: only {int(owes.sum())} records owed"
    share = _check_hits(h, t, p, n, owes, exempt, fc_g, seq_g, got["trig"], label)
    assert len(hh) == len(h) and hh.tobytes() == h.tobytes(), f"{label}: hits-only records are byte-identical to spectrum + hits records"
    assert np.array_equal(th, t), label
    _FIG.setdefault((fam, _wire_name(kind, enob, dc)), []).append((label, fig["floor_err"], Y, fig["floor_share"], share))
    print(f"{label}: {nb} buffers, floor_err {fig['floor_err']:.2e}, Y {Y:.2e}, ratio {fig['floor_err'] / Y:.2f}, floor share {fig['floor_share']:.4f}, "
          f"strict p99 {fig['strict_p99']:.1e}, -inf {fig['n_minus_inf']}, thr {thr:.2f} dB, {len(h)} records, exempt {share:.2%}, "
          f"max rel power {cmp['max_rel_power_vs_max_bin_mean']:.1e}" + (f", parts {got['parts']}" if copies > 1 else ""))
    assert fig["floor_err"] <= 2.0 * Y, (f"{label}: a floor bin is off by {fig['floor_err']:.2e} of the rms level; two float32 transforms that are not this "
                                         f"kernel stay within Y = {Y:.2e} on the same buffers (ratio {fig['floor_err'] / Y:.2f} > 2)")
    return got


@pytest.mark.parametrize("n,kind,enob,dc", CASES, ids=[f"{n}-{_wire_name(k, e, dc).replace('/', '-')}" for n, k, e, dc in CASES])
def test_floor_under_a_blocker(built_lib, oracle_mod, n, kind, enob, dc):
    x, _ = sc.batch(n, _count(n), seed=100 + kind + enob + dc)
    raw = sc.to_wire(x, kind, enob, dc)
    conv = sc.convert(oracle_mod, n, kind, enob, dc, raw)
    _launch_and_check(oracle_mod, n, kind, enob, dc, raw, conv, 1, capi.AVG_DWELL, f"n={n} {_wire_name(kind, enob, dc)}", family(n))


@pytest.mark.parametrize("n,k,layout", AVG, ids=[f"{n}-K{k}-{'sweeps' if lay == capi.AVG_SWEEPS else 'dwell'}" for n, k, lay in AVG])
def test_floor_under_a_blocker_averaged(built_lib, oracle_mod, n, k, layout):
    G = max(2, (1 << 18) // (n * k))
    x, _ = sc.batch(n, G, seed=200 + k, copies=k)
    if layout == capi.AVG_SWEEPS:
        x, _ = sc.regroup(x, G, k)
    got = _launch_and_check(oracle_mod, n, CF, 12, False, x, x, k, layout,
                            f"n={n} K={k} {'sweeps' if layout == capi.AVG_SWEEPS else 'dwell'}", f"averaged {n}")
    if k == 16:
        assert got["parts"] > 1, "K = 16 at this shape shares a group's buffers among workgroups"


@pytest.mark.parametrize("kind", [CF, I16], ids=["cfloat", "int16"])
def test_floor_under_a_blocker_welch(built_lib, oracle_mod, kind):
    from tests.test_oracle_vs_pocketfft import float32_chain

    N, K, n_psd, enob = 65536, 16, 4, 12
    hop = N // 2
    x, _ = sc.stream(N, (n_psd * K + 1) * hop, seed=300)
    raw = sc.to_wire(x.reshape(-1, hop), kind, enob, False)
    conv = oracle_mod.welch_convert(raw, kind, enob, False, hop)
    with WelchPlan(N, K, max_psd=4, kind=kind, enob=enob if kind != CF else 0) as wp:
        flat = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        assert flat.size == wp.samples(n_psd) * wp.bytes_per_sample
        wp.submit_device(0, _dev(flat), n_psd)
        p = wp.collect(0)
    w = oracle_mod.Oracle(N).window()
    d64 = oracle_mod.ref64_welch(conv, w, N, K, n_psd)
    a64 = 10.0 ** (d64 / 10.0)
    seg = np.stack([conv[s * hop:s * hop + N] for s in range(n_psd * K)])
    dbs = {"oracle": oracle_mod.welch(conv, N, K, n_psd),
           "pocketfft": 5.0 * np.log10(sc.group_mean(10.0 ** (float32_chain(seg, w).astype(np.float64) / 5.0), K))}
    Y = max(tol.floor_errors(d, a64)["floor_err"] for d in dbs.values())
    fig = tol.floor_errors(p, a64)
    sc.assert_floor_share(N, fig["floor_share"])
    tol.compare_spectra(p, d64)
    label = f"welch {NAMES[kind]}"
    _FIG.setdefault(("welch", _wire_name(kind, enob, False)), []).append((label, fig["floor_err"], Y, fig["floor_share"], 0.0))
    print(f"{label}: floor_err {fig['floor_err']:.2e}, Y {Y:.2e}, ratio {fig['floor_err'] / Y:.2f}, floor share {fig['floor_share']:.4f}, strict p99 {fig['strict_p99']:.1e}")
    assert fig["floor_err"] <= 2.0 * Y, (label, fig, Y)


def test_zz_figures(request):
    """prints what the module measured, per family and wire format: the worst launch's kernel figure, its Y, the ratio, the smallest
    floor share and the largest exempt share; where the whole module ran in this process, asserts that every launch was noted"""
    mine = [i for i in request.session.items if i.fspath.basename == "test_dynamic_range_gpu.py"]
    total = len(CASES) + len(AVG) + 2
    whole = not request.config.option.keyword and not hasattr(request.config, "workerinput") and len(mine) == total + 1
    notes = [r for rows in _FIG.values() for r in rows]
    if whole and mine[-1].name == "test_zz_figures":
        assert len(notes) == total, (len(notes), total)
        assert max(r[1] / r[2] for r in notes) <= 2.0 and max(r[4] for r in notes) <= MAX_EXEMPT
    print(f"build {build.source_hash()}: floor criterion, {len(notes)} launches")
    print(f"{'family':<16}{'wire format':<22}{'launches':>8}  {'floor_err':>9}  {'Y':>9}  {'ratio':>5}  {'floor share':>11}  {'exempt':>6}  worst launch")
    for (fam, wire), rows in _FIG.items():
        worst = max(rows, key=lambda r: r[1] / r[2])
        print(f"{fam:<16}{wire:<22}{len(rows):>8}  {worst[1]:>9.2e}  {worst[2]:>9.2e}  {worst[1] / worst[2]:>5.2f}  {min(r[3] for r in rows):>11.4f}  "
              f"{max(r[4] for r in rows):>6.2%}  {worst[0]}")
