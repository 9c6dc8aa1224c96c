"""The Bluestein path (scanner_amd/csrc/scn_generic.hip: every size from 17 to 65535 without a fused or four-step kernel) held to
its own promise -- double between the windowed input and the spectrum, rounded to float once -- at every transform length.

The bar is tests/bluestein_cases.py allowance_db: the dB map's proven bound, the four float roundings of the finish kernel, and 2^-40
of the rms level for the double chain; tests/test_bluestein_cases_cpu.py shows on the CPU that float work buffers, a float chirp and
a float filter transform each miss it by 80 ... 11000 times at every size tried, and that the bins it leaves to floor_errors (below
2^-20 of the rms level) are at most 3.1e-5 of any launch here.  The older bars (tolerances.compare_spectra, floor_errors) are run
on the same output.

Per launch about 2^16 samples, max(3, 65536 // n) + 5 buffers of dr_scenes.batch (a 0.5-amplitude blocker, noise 74 dB below, weak
tones); the reference is numpy's complex128 FFT of the float32 product of the oracle-converted samples and plan.window().  The hit
list is demanded EXACTLY as the float64 spectrum owes it -- (seq_id, i, freq_hz), order, trigger flags -- at a threshold 6 dB over
the floor with an empty guard band (GUARD_DB is three orders above the allowance), and every record carries the float the
spectrum holds.

  test_every_size          SIZES in cfloat: both ends of every transform length 2^6 ... 2^17 (every radix-2 / 4 / 16 stage sequence and
                           both ping-pong parities), seven even sizes
  test_wire_formats        33 / 257 / 8193 / 11000 in int16 interleaved (ENOB 12, 16), int16 planar (14) and int8 (8), DC removal off
                           and on: all seven scn_gen_load_kernel instantiations at odd row strides
  test_output_modes        hits-only and spectrum-only plans byte-identical to the spectrum + hits plan
  test_position_independence   a buffer's row and records do not depend on where it sits, what sits beside it, or the slot
  test_special_values      zero, NaN, overflow and a unit impulse beside ordinary buffers
  test_zz_figures          prints the worst margin per launch and term (run with -rP); profiles/bluestein_exact.md keeps a copy

MODULE STATE: the figures are a module global filled in test order."""
import numpy as np
import pytest

from scanner_amd import Plan, build, capi
from tests import bluestein_cases as bc
from tests import dr_scenes as sc
from tests import launch_caps as caps
from tests import tolerances as tol

pytestmark = pytest.mark.gpu
FS = 8000000
SEQ0 = 1 << 33
BOTH, HITS, SPEC = capi.OUT_SPECTRUM | capi.OUT_HITS, capi.OUT_HITS, capi.OUT_SPECTRUM
CF = capi.KIND_FLOAT_COMPLEX

_FIG = []   # (label, n, buffers, check_spectrum's figures, floor_errors' figures, compare_spectra's figures, records)


def _dev(raw):
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need a GPU; refusing to skip silently"
    return torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).reshape(-1)).cuda()


def _window(oracle_mod, n, **kw):
    with Plan(n, FS, 1e9, flags=SPEC, **kw) as plan:
        w = plan.window()
    if "window_type" not in kw:
        assert np.array_equal(w, oracle_mod.Oracle(n).window())
    return w


def _headers(nb):
    return 70e6 + 6e6 * np.arange(nb), np.arange(nb, dtype=np.uint64) + np.uint64(SEQ0)


def _launch(n, raw, nb, thr, trig, fc, seq, flags=BOTH, slot=0, cap=0, **kw):
    with Plan(n, FS, thr, flags=flags, max_batch=nb, max_hits=cap + 4096, trigger_count=trig, **kw) as plan:
        plan.submit_device(slot, _dev(raw), nb, fc, seq)
        return plan.collect(slot)


def _assert_records(h, t, p, rec, counts, trig, n, what):
    """the records and trigger flags of a launch are exactly what the float64 spectrum owes, and carry the spectrum's floats"""
    assert len(h) == len(rec), f"{what}: {len(h)} records, the float64 spectrum owes {len(rec)}"
    for f in ("seq_id", "i", "freq_hz"):
        assert np.array_equal(h[f], rec[f]), f"{what}: {f} differs from what the float64 spectrum owes"
    assert np.array_equal(t, (counts > trig).astype(np.uint8)), f"{what}: trigger flags"
    if p is not None:
        g = (h["seq_id"] - np.uint64(SEQ0)).astype(np.int64)
        j = (h["i"].astype(np.int64) + n // 2) % n
        assert h["power_db"].tobytes() == p[g, j].tobytes(), f"{what}: a record carries the float the spectrum holds"


def _launch_and_check(oracle_mod, n, kind, enob, dc, label):
    raw, conv = bc.scene(oracle_mod, n, kind, enob, dc)
    nb = len(conv)
    assert nb == bc.count(n)
    common = dict(kind=kind, enob=enob, correct_dc=dc)
    a64, d64 = bc.owed(conv, _window(oracle_mod, n, **common))
    thr = bc.threshold_of(a64, d64, n)
    fc, seq = _headers(nb)
    rec, counts = bc.owed_hits(d64, n, thr, fc, seq, FS)
    trig = bc.trigger_count_of(counts)
    p, h, t = _launch(n, raw, nb, thr, trig, fc, seq, cap=len(rec), **common)
    assert p.shape == a64.shape
    fig = bc.measure_spectrum(p, a64)
    flo = tol.floor_errors(p, a64)
    print(f"{label}: {nb} buffers, stages {caps.bluestein_radices(n)}, excess {fig['excess']:.3f} ({fig['err_db']:.2e} dB; map {fig['terms'][0]:.2e}, "
          f"roundings {fig['terms'][1]:.2e}, chain {fig['terms'][2]:.2e}), excluded {fig['excluded_share']:.1e}, floor_err {flo['floor_err']:.2e} "
          f"(bound {bc.FLOOR_BOUND:.2e}), thr {thr:.2f} dB, {len(rec)} records owed, {len(h)} reported, trigger_count {trig}")
    bc.check_spectrum(p, a64, label)
    cmp = tol.compare_spectra(p, d64)
    bc.floor_bound_check(p, a64, label)
    _assert_records(h, t, p, rec, counts, trig, n, label)
    assert t.any() and not t.all(), f"{label}: trigger flags of one kind only"
    _FIG.append((label, n, nb, fig, flo, cmp, len(h)))


@pytest.mark.parametrize("n", bc.SIZES)
def test_every_size(built_lib, oracle_mod, n):
    assert capi.size_path(n) == capi.PATH_BLUESTEIN
    _launch_and_check(oracle_mod, n, CF, 12, False, f"n={n} cfloat")


assert set(bc.WIRE_SIZES) <= set(bc.SIZES)           # cfloat at the wire-format sizes is test_every_size's
WIRE = [c for c in bc.wire_cases() if c[1] != CF]


@pytest.mark.parametrize("n,kind,enob,dc", WIRE, ids=[bc.wire_id(*c) for c in WIRE])
def test_wire_formats(built_lib, oracle_mod, n, kind, enob, dc):
    _launch_and_check(oracle_mod, n, kind, enob, dc, "n=" + bc.wire_id(n, kind, enob, dc).replace("-", " ", 1))


@pytest.mark.parametrize("n", bc.MODE_SIZES)
def test_output_modes(built_lib, oracle_mod, n):
    """hits-only and spectrum-only plans against the spectrum + hits plan: records with their power_db, trigger flags, spectra"""
    raw, conv = bc.scene(oracle_mod, n, CF, 12, False, seed=520)
    nb = len(conv)
    a64, d64 = bc.owed(conv, _window(oracle_mod, n))
    thr = bc.threshold_of(a64, d64, n)
    fc, seq = _headers(nb)
    rec, counts = bc.owed_hits(d64, n, thr, fc, seq, FS)
    trig = bc.trigger_count_of(counts)
    p, h, t = _launch(n, raw, nb, thr, trig, fc, seq, BOTH, cap=len(rec))
    ph, hh, th = _launch(n, raw, nb, thr, trig, fc, seq, HITS, slot=1, cap=len(rec))
    ps, hs, ts = _launch(n, raw, nb, thr, trig, fc, seq, SPEC, slot=2, cap=len(rec))
    bc.check_spectrum(p, a64, f"n={n}")
    _assert_records(h, t, p, rec, counts, trig, n, f"n={n}")
    assert len(h) > 0 and t.any() and not t.all()
    assert ph is None and hs is None and ts is None
    assert len(hh) == len(h) and hh.tobytes() == h.tobytes(), "hits-only records are byte-identical to spectrum + hits records"
    assert th.tobytes() == t.tobytes()
    assert ps.shape == p.shape and ps.tobytes() == p.tobytes(), "the spectrum-only plan's spectrum is byte-identical"


def _tone_rows(n, rows, amplitude):
    k = np.arange(n, dtype=np.float64)
    tone = amplitude * np.exp(2j * np.pi * (n // 5 + 0.5) * k / n)
    return np.tile(tone.astype(np.complex64), (rows, 1))


@pytest.mark.parametrize("n", bc.POSITION_SIZES)
def test_position_independence(built_lib, oracle_mod, n):
    """No arithmetic crosses buffers: buffer k's spectrum row, records and trigger flag are byte-identical at batch position 0, in
    the middle and last, in a batch of 1 and of nb, in slot 0 and slot 3, and with its neighbours replaced by all-zero and by
    full-scale buffers."""
    nb = bc.count(n)
    x, _ = sc.batch(n, nb, seed=600)
    k = nb // 2
    a64, d64 = bc.owed(x, _window(oracle_mod, n))
    thr = bc.threshold_of(a64, d64, n)
    fc, seq = _headers(nb)
    rec, counts = bc.owed_hits(d64, n, thr, fc, seq, FS)
    trig = bc.trigger_count_of(counts)

    def swapped(a, b):
        perm = np.arange(nb)
        perm[[a, b]] = perm[[b, a]]
        return perm

    zeros, full = np.zeros_like(x), _tone_rows(n, nb, 1.0)
    zeros[k] = full[k] = x[k]
    ident = np.arange(nb)
    variants = {                                  # name: (buffers, their original indices, slot)
        "middle": (x, ident, 0),
        "first": (x[swapped(0, k)], swapped(0, k), 0),
        "last": (x[swapped(nb - 1, k)], swapped(nb - 1, k), 0),
        "alone": (x[k:k + 1], ident[k:k + 1], 0),
        "slot 3": (x, ident, 3),
        "zero neighbours": (zeros, ident, 0),
        "full-scale neighbours": (full, ident, 0),
    }
    got = {}
    with Plan(n, FS, thr, max_batch=nb, max_hits=nb * n, trigger_count=trig) as plan:
        for name, (bufs, idx, slot) in variants.items():
            plan.submit_device(slot, _dev(bufs), len(bufs), fc[idx], seq[idx])
            p, h, t = plan.collect(slot)
            pos = int(np.flatnonzero(idx == k)[0])
            got[name] = (p[pos].tobytes(), h[h["seq_id"] == seq[k]].tobytes(), int(t[pos]), p, h, t)
            if name == "zero neighbours":
                others = np.arange(nb) != k
                assert np.isneginf(p[others]).all() and len(h) == counts[k] and not t[others].any()
    p, h, t = got["middle"][3:]
    bc.check_spectrum(p, a64, f"n={n}")
    _assert_records(h, t, p, rec, counts, trig, n, f"n={n}")
    assert counts[k] > 0
    for name in variants:
        assert got[name][:3] == got["middle"][:3], f"n={n}: buffer {k} reads differently: {name}"


@pytest.mark.parametrize("n", bc.SPECIAL_SIZES)
def test_special_values(built_lib, oracle_mod, n):
    """Under the rectangular window, at a threshold below every finite value and trigger_count 1 (the smallest: 0 is the descriptor's
    default; every buffer with finite bins has at least six evaluated ones): an all-zero buffer is -inf
    everywhere and yields no record; one NaN sample makes the buffer all-NaN, without record or trigger; a buffer scaled by 2^70
    reports +inf, and a record where evaluated, wherever the float32 power of the reference's float-cast components overflows (bins
    within a factor of two of the boundary exempt); a unit impulse of amplitude 0.75 is 10 log10 0.75 in every bin within
    allowance_db; and the ordinary buffers of the launch are byte-identical to the launch without the special ones."""
    thr, fmax = -1e30, float(np.finfo(np.float32).max)
    ordinary, _ = sc.batch(n, 6, seed=700)
    w = _window(oracle_mod, n, window_type=capi.WIN_RECTANGULAR)
    assert np.array_equal(w, np.ones(n, np.float32))
    rng = np.random.default_rng([700, n])
    zero, nan, impulse = (np.zeros(n, np.complex64) for _ in range(3))
    nan[:] = ordinary[0]
    nan[5] = np.complex64(complex(np.nan, 0.25))
    impulse[n // 3] = 0.75
    k = np.arange(n, dtype=np.float64)
    big = 0.01 * np.exp(2j * np.pi * (n // 3 + 0.37) * k / n) + 1e-5 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    big = (big.astype(np.complex64) * np.float32(2.0 ** 70)).astype(np.complex64)
    mixed = np.stack([ordinary[0], zero, ordinary[1], nan, ordinary[2], big, ordinary[3], impulse, ordinary[4], ordinary[5]])
    ORD, ZERO, NAN, BIG, IMP = [0, 2, 4, 6, 8, 9], 1, 3, 5, 7
    fc, seq = _headers(len(mixed))
    kw = dict(window_type=capi.WIN_RECTANGULAR)
    p, h, t = _launch(n, mixed, len(mixed), thr, 1, fc, seq, cap=len(mixed) * n, **kw)
    p0, h0, t0 = _launch(n, ordinary, 6, thr, 1, fc[ORD], seq[ORD], slot=1, cap=6 * n, **kw)
    ev = tol.evaluated_mask(n)

    def records_of(b):
        return h[h["seq_id"] == seq[b]]

    assert np.isneginf(p[ZERO]).all() and len(records_of(ZERO)) == 0 and t[ZERO] == 0
    assert np.isnan(p[NAN]).all() and len(records_of(NAN)) == 0 and t[NAN] == 0
    # the scaled buffer, against the float32 power of the float64 spectrum's float-cast components
    X = np.fft.fft(sc.windowed(big[None, :], w)[0].astype(np.complex128))
    re, im = X.real.astype(np.float32).astype(np.float64), X.imag.astype(np.float32).astype(np.float64)
    P = re * re + im * im
    over, under = P > 2.0 * fmax, P < 0.5 * fmax
    assert over.any() and under.any() and (over & ev).any()
    assert not np.isnan(p[BIG]).any()
    assert (p[BIG][over] == np.inf).all() and np.isfinite(p[BIG][under]).all()
    a_big = np.sqrt(P)[None, :]
    held = under & ~bc.excluded(a_big)[0]
    assert (np.abs(p[BIG].astype(np.float64) - 5.0 * np.log10(P))[held] <= bc.allowance_db(a_big)[0][held]).all()
    r = records_of(BIG)
    j = (r["i"].astype(np.int64) + n // 2) % n
    assert np.array_equal(np.sort(j), np.flatnonzero(ev)), "every evaluated bin of the scaled buffer is above the threshold"
    assert r["power_db"].tobytes() == p[BIG][j].tobytes() and (r["power_db"][over[j]] == np.inf).all() and t[BIG] == 1
    # the impulse: |X| = 0.75 in every bin
    a_imp = np.full((1, n), 0.75)
    assert (np.abs(p[IMP].astype(np.float64) - 10.0 * np.log10(0.75)) <= bc.allowance_db(a_imp)[0]).all(), np.abs(p[IMP] - 10.0 * np.log10(0.75)).max()
    assert len(records_of(IMP)) == ev.sum() and t[IMP] == 1
    # the ordinary buffers: right, and untouched by their neighbours
    a64, _ = bc.owed(ordinary, w)
    bc.check_spectrum(p0, a64, f"n={n} rectangular")
    assert p[ORD].tobytes() == p0.tobytes(), "an ordinary buffer's spectrum changed beside the special buffers"
    assert h[np.isin(h["seq_id"], seq[ORD])].tobytes() == h0.tobytes() and len(h0) == 6 * ev.sum()
    assert t[ORD].tobytes() == t0.tobytes() and t0.all()


def test_zz_figures():
    """prints what the module measured, per launch: the worst |dB - dB64| over its allowance among the held bins, that bin's error and
    the three terms of its allowance, the excluded share, floor_errors' figure, compare_spectra's; a record, not a bound"""
    print(f"build {build.source_hash()}: Bluestein against its double-precision promise, {len(_FIG)} launches")
    print(f"{'launch':<32}{'buffers':>7}  {'stages':<20}{'excess':>7}  {'err dB':>8}  {'map':>8}  {'round.':>8}  {'chain':>8}  {'excluded':>8}  "
          f"{'floor_err':>9}  {'rel power':>9}  {'records':>7}")
    for label, n, nb, fig, flo, cmp, records in _FIG:
        print(f"{label:<32}{nb:>7}  {str(caps.bluestein_radices(n)):<20}{fig['excess']:>7.3f}  {fig['err_db']:>8.2e}  {fig['terms'][0]:>8.2e}  "
              f"{fig['terms'][1]:>8.2e}  {fig['terms'][2]:>8.2e}  {fig['excluded_share']:>8.1e}  {flo['floor_err']:>9.2e}  "
              f"{cmp['max_rel_power_vs_max_bin_mean']:>9.1e}  {records:>7}")
    if _FIG:
        assert max(f[3]["excess"] for f in _FIG) <= 1.0 and max(f[3]["excluded_share"] for f in _FIG) <= bc.MAX_EXCLUDED_SHARE
