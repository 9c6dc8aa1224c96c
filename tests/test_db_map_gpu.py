"""The dB map (db_of_power, scn_device.h) and the decision `dB > threshold` behind the linear-power gate, held TO THE BIT on inputs
whose bin powers are known exactly (tests/db_probes.py, pinned on the host by tests/test_db_probes_cpu.py): rectangular window, DC
removal off, so that the FFT drops out of the picture and a test can say which float the map owes.

Per kernel family of DESIGN.md section 3.1 (16 ... 512, 1024 ... 8192, 16384, the mixed-radix sizes 1000 / 6000 / 12000, the
four-step sizes 32768 / 65536, the averaged plans at 1024 ... 8192 with K = 2 and 4 identical copies; the Welch plan's two
epilogues -- separate code sites that no launch of this module reaches -- are held the same way by tests/test_welch_exact_gpu.py):
  * one float per flat buffer: all N bins of a flat probe hold the same bits (no reference needed);
  * the bound (tests/tolerances.py db_map_bound*): every value within max(4.2e-6 dB, 2.2 ulp) of the float64 value 5 log10 P below
    SCN_P_EXACT_FROM, within 1.0 ulp at and above it -- on a sweep over the whole float range of powers that walks EVERY float
    power from 40 below SCN_P_EXACT_FROM to 40 above it, and against the oracle's magnitude() (bit-pinned to the reference,
    correctly rounded: bound + half an ulp) where the amplitude has at most 12 significant bits;
  * purity: {power bits -> dB bits} is collected over every family, wire format, output mode, slot and record of this module's
    launches; a power that maps to two floats fails and names both launches;
  * special values: P = 0 -> -inf, |a| >= 2^64 -> +inf, a NaN sample -> an all-NaN buffer without record or trigger; the ordinary
    buffers of the same launch are byte-identical to the launch without the special buffers;
  * the knife edge: ladders of consecutive floats (below, across and above SCN_P_EXACT_FROM, and one of line probes per wire
    format); with the threshold T ON a reported value (and one float above / below it) the hit list is exactly the evaluated bins
    whose reported float is > T, in spectrum + hits and hits-only plans alike, byte for byte;
  * every output position: an on-grid tone swept over the bins, its line (32 ... 64 dB) within 1.0 ulp + (5 / ln 10) eps / ulp of
    float64, eps = twice the larger relative power deviation of two float32 transforms that are not the kernel under test (the
    oracle's FFT, scipy.fft on complex64) on the very same lines.  The total must stay <= 1.7 ulp (asserted), or the test could not
    tell the exact form from the product form, which reaches 2.2.  The tones are min(N, 2^24 / N) per amplitude set, one per
    stratum of consecutive bins (every bin up to 4096 points; every 2nd, 4th, 16th, 256th bin at 6000 / 8192, 16384, 12000,
    65536 points, spread over the whole spectrum, every residue mod 16 and 32, mod 256 where there are 4096 tones -- asserted), each with a mantissa of its
    own (an on-grid tone of one amplitude has ONE power at every bin).  An output index of a thread's 16 so sees 3 x 4096 / 16 =
    768 (bin, amplitude) pairs at 4096 points, 192 at 16384 and 48 at 65536; a SINGLE (thread, output) pair sees three or none,
    which is not enough to catch an overlay that misses just that pair.

DENORMAL POWERS (2^-149 <= P < 2^-126): the device's v_log_f32 takes no denormal input, the map returns -inf and no record can
form, whatever the threshold; the reference returns a finite -190 ... -224 dB there (its sqrtf of a denormal is normal).  This is
a stated limit (scn_device.h); test_denormal_powers asserts its exact form so that a change is noticed.

LINE PROBES IN THE MIXED-RADIX KERNELS: a radix-3 / radix-5 pass may see i^n at a stride that is not a multiple of 4, and then
W_3 / W_5 multiply nonzero data.  The test finds out without a reference: the floor bins of a line probe must hold the bits of the
flat probe of the floor's amplitude.  The sizes where they do not are listed in LINE_INEXACT: their line probes are held to the
tone sweep's bound instead of the exact one, their flat probes stay exact.

MODULE STATE: the purity table, the eps cache and the figures are module globals filled in test order, in one process.  Under -k,
xdist or a random order purity compares fewer launches (it is still asserted at every insertion); test_zz_figures asserts the
totals only where the whole module ran.  8192 POINTS: plain plans of every wire format run scn_fft8k_kernel (the dispatch has one
form); the two-halves form is the averaged plans'.  Both get the dense cfloat sweep, the former the integer impulse sweeps too.

Measured on an MI355X (test_zz_figures prints them; run with -rP): product form 1.767 ulp at P = 8.5691e-24 and 3.33e-6 dB at
P = 8.4773e-6 (bounds 2.2 ulp / 4.2e-6 dB); exact form 0.995 ulp at P = 5.5909e24 (bound 1.0); 24957 distinct powers, one dB value
each, over 1608 launches.  eps per size: 64: 4.8e-7, 512: 5.3e-7, 1024: 5.5e-7, 4096: 5.4e-7, 8192: 6.1e-7, 16384: 5.8e-7,
1000: 6.2e-7, 6000: 5.9e-7, 12000: 5.3e-7, 65536: 4.9e-7 (a bound of 1.26 ... 1.35 ulp); worst line of the tone sweep 1.02 ulp.
The whole module takes 22 s (203 tests)."""
import math

import numpy as np
import pytest

from scanner_amd import Plan, build, capi
from tests import db_probes as pr
from tests import tolerances as tol

pytestmark = pytest.mark.gpu
F32 = np.float32
FS = 8000000
FC = 100e6
SEQ0 = 1 << 33
BOTH, HITS, SPEC = capi.OUT_SPECTRUM | capi.OUT_HITS, capi.OUT_HITS, capi.OUT_SPECTRUM
NAMES = {capi.KIND_FLOAT_COMPLEX: "cfloat", capi.KIND_SHORT_COMPLEX: "int16", capi.KIND_SHORT: "int16planar", capi.KIND_BYTE_COMPLEX: "int8"}
KINDS = list(NAMES)

build.build()  # (seconds when the library is current; needs no GPU)
SIZES = [16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 1000, 6000, 12000, 32768, 65536]
AVG = [(n, k) for n in (1024, 2048, 4096, 8192) for k in (2, 4)]
# sizes whose line probes are not exact in the kernel's decomposition (see the module docstring)
LINE_INEXACT = (1000, 6000, 12000)   # measured: every mixed-radix size tried; all powers of two are exact
TONE_SIZES = [64, 512, 1024, 4096, 8192, 16384, 1000, 6000, 12000, 65536]
TONE_CAP_ULP = 1.7

_PURE = {}      # power bits -> (dB bits, the launch that reported them)
_FIG = {"fast": (0.0, None, None), "fast_abs": (0.0, None, None), "exact": (0.0, None, None), "eps": {}, "tone": {}}
_LAUNCH = [0]


# ---- launching ------------------------------------------------------------------------------------------------------------------
def _dev(raw):
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need a GPU; refusing to skip silently"
    return torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).reshape(-1)).cuda()


def _run(n, kind, d_raw, nb, thr, flags, cap=4096, average=1):
    """one launch of nb buffers (nb / average groups) in the next slot; returns (power_db, hits, trigger) of collect"""
    slot = _LAUNCH[0] % capi.NUM_SLOTS
    _LAUNCH[0] += 1
    with Plan(n, FS, thr, kind=kind, enob=pr.ENOB[kind], correct_dc=False, max_batch=nb, max_hits=cap, flags=flags, trigger_count=1,
              window_type=capi.WIN_RECTANGULAR, average=average) as plan:
        plan.submit_device(slot, d_raw, nb, np.full(nb, FC), np.arange(nb, dtype=np.uint64) + SEQ0)
        return plan.collect(slot)


def _expected(p, n, thr):
    """the hit list and trigger flags that the reported spectrum p [G, n] owes at threshold thr: the evaluated bins whose float is
    > thr, strictly (process.cpp:54), ordered by (group, i); trigger = count > 1 (process.cpp:62 with trigger_count = 1)"""
    half = n // 2
    pi = np.roll(p, half, axis=1)                       # pi[:, i] = p[:, (i + half) % n]
    ev = np.roll(tol.evaluated_mask(n), half)
    with np.errstate(invalid="ignore"):
        hm = ev[None, :] & (pi > F32(thr))
    g, i = np.nonzero(hm)
    return g, i, pi[hm], (hm.sum(axis=1) > 1).astype(np.uint8)


def _check_hits(p, h, t, n, thr, average, what):
    g, i, d, trig = _expected(p, n, thr)
    assert len(h) == len(g), f"{what}: {len(h)} records, the reported floats owe {len(g)}"
    assert np.array_equal(h["seq_id"], (g * average).astype(np.uint64) + np.uint64(SEQ0)), what
    assert np.array_equal(h["i"], i.astype(np.uint32)), what
    assert h["power_db"].tobytes() == d.tobytes(), f"{what}: a record carries the float the spectrum holds"
    assert np.array_equal(t, trig), f"{what}: trigger flags follow the counts"
    return len(g)


def _n_hits(p, n, thr):
    return len(_expected(p, n, thr)[0])


def _decide(n, kind, d_raw, nb, p0, thr, what, average=1):
    """spectrum + hits and hits-only plans at threshold thr against the floats p0 a plan of threshold 1e9 reported"""
    cap = _n_hits(p0, n, thr) + 1024
    p, h, t = _run(n, kind, d_raw, nb, thr, BOTH, cap, average)
    assert p.tobytes() == p0.tobytes(), f"{what}: the spectrum does not depend on the threshold"
    cnt = _check_hits(p, h, t, n, thr, average, what)
    ph, hh, th = _run(n, kind, d_raw, nb, thr, HITS, cap, average)
    assert ph is None
    assert len(hh) == len(h), f"{what}: hits-only plan reports {len(hh)} records, spectrum + hits {len(h)}"
    assert hh.tobytes() == h.tobytes(), f"{what}: hits-only records are byte-identical to spectrum + hits records"
    assert np.array_equal(th, t), what
    return cnt


# ---- the map --------------------------------------------------------------------------------------------------------------------
def _note(P, v, label):
    P, v = np.asarray(P, F32).reshape(-1), np.asarray(v, F32).reshape(-1)
    ok = ~np.isnan(P)
    u = np.unique(np.stack([P[ok].view(np.uint32), v[ok].view(np.uint32)], axis=1), axis=0)
    for a, b in u.tolist():
        old = _PURE.setdefault(a, (b, label))
        assert old[0] == b, (f"purity: power {np.array(a, np.uint32).view(F32)!r} ({a:#x}) maps to {np.array(old[0], np.uint32).view(F32)!r} "
                             f"in [{old[1]}] and to {np.array(b, np.uint32).view(F32)!r} in [{label}]")


def _check_map(P, v, label, eps=None):
    """device values v of exact NORMAL float powers P against float64, to the bound of the half of the map P takes"""
    P, v = np.asarray(P, F32).reshape(-1), np.asarray(v, F32).reshape(-1)
    assert ((P >= np.finfo(F32).tiny) & np.isfinite(P)).all()
    d = pr.db64(P)
    ulp = np.spacing(np.abs(d).astype(F32)).astype(np.float64)
    err = np.abs(v.astype(np.float64) - d)
    exact = P >= tol.P_EXACT_FROM
    if eps is None:
        bound = tol.db_map_bound_of_power(P, d)
    else:   # powers known to the relative deviation eps only (the tone sweep's bound)
        bound = tol.DB_MAP_ULP_EXACT * ulp + (5.0 / math.log(10.0)) * eps
        assert exact.all() and (bound / ulp).max() <= TONE_CAP_ULP, (label, eps, float((bound / ulp).max()))
    if eps is None:
        # (the product form's figure in ulp where 2.2 ulp is the bound, i.e. below -16 dB; in dB where the 4.2e-6 floor is)
        floor = tol.DB_MAP_ULP_FAST * ulp < tol.DB_MAP_ABS
        for key, m, e in (("fast", ~exact & ~floor, err / ulp), ("fast_abs", ~exact & floor, err), ("exact", exact, err / ulp)):
            if m.any():
                k = int(np.argmax(np.where(m, e, -1.0)))
                if e[k] > _FIG[key][0]:
                    _FIG[key] = (float(e[k]), float(P[k]), label)
    bad = ~(err <= bound)
    assert not bad.any(), (f"{label}: {int(bad.sum())} of {bad.size} values outside the map's bound; worst "
                           f"{[(float(P[k]), float(v[k]), float(d[k]), round(float(err[k] / ulp[k]), 3)) for k in np.argsort(-err / ulp)[:4]]} "
                           f"(power, device, float64, error in ulp)")


def _one_float(p, label):
    b = p.view(np.uint32)
    bad = np.flatnonzero((b != b[:, :1]).any(axis=1))
    if bad.size:
        k = bad[0]
        j = np.flatnonzero(b[k] != b[k, 0])
        raise AssertionError(f"{label}: {bad.size} flat buffers hold more than one float; buffer {k}: bin 0 = {p[k, 0]!r}, "
                             f"{j.size} bins differ, first j = {j[:8].tolist()} -> {p[k, j[:8]].tolist()}")


def _sweep_amps():
    """the amplitudes of the flat sweep, the same list (a prefix of it) for every family so that purity compares like with like:
    the power ladder across SCN_P_EXACT_FROM, consecutive amplitudes around sqrt of it, values near 1.0 (the 4.2e-6 dB floor),
    12-bit amplitudes (the oracle's magnitude() is exact on them), then random ones over the whole float range of powers (up to
    2^125.8, so that the sum of four copies in an averaged plan stays finite)"""
    rng = np.random.default_rng(20240611)
    lad = pr.power_ladder(tol.P_EXACT_FROM, 40, 40)
    strad = pr.float_ladder(39.81072, 20, 20).astype(np.complex64)
    near1 = np.concatenate([pr.float_ladder(1.0, 8, 8), rng.uniform(0.9, 1.1, 24).astype(F32)]).astype(np.complex64)
    twelve = (rng.integers(2048, 4096, 64) * np.exp2(rng.integers(-70, 50, 64).astype(np.float64)) * rng.choice([-1.0, 1.0], 64)).astype(F32)
    wide = (np.exp2(rng.uniform(-62.9, 62.9, 14000)) * rng.choice([-1.0, 1.0], 14000)).astype(F32)
    strong = np.exp2(rng.uniform(5.3, 21.3, 6000)).astype(F32)          # 16 ... 64 dB
    rest = np.concatenate([wide, strong])
    rng.shuffle(rest)
    first = len(lad) + len(strad) + len(near1)
    return np.concatenate([lad, strad, near1, twelve.astype(np.complex64), rest.astype(np.complex64)]), slice(first, first + len(twelve))


AMPS, TWELVE = _sweep_amps()


def _sweep_count(n):
    return min(len(AMPS), (1 << (24 if n >= 16384 else 23)) // n + 37)   # (+37: the last workgroup's buffer slots stay partly empty)


def _flat_sweep(oracle_mod, n, average):
    nb = _sweep_count(n) // (2 if average > 1 else 1)
    amps = AMPS[:nb]
    P = pr.exact_power(amps)
    label = f"flat n={n} cfloat" + (f" K={average}" if average > 1 else "")
    d_raw = _dev(np.repeat(pr.flat_raw(n, amps), average, axis=0))
    ps, _, _ = _run(n, capi.KIND_FLOAT_COMPLEX, d_raw, nb * average, 1e9, SPEC, average=average)
    p, h, t = _run(n, capi.KIND_FLOAT_COMPLEX, d_raw, nb * average, 1e9, BOTH, average=average)
    assert len(h) == 0 and not t.any()
    _one_float(p, label)
    assert ps.tobytes() == p.tobytes(), f"{label}: spectrum-only and spectrum + hits plans store identical spectra"
    v = p[:, 0].copy()
    _check_map(P, v, label)
    _note(P, v, label)
    m = oracle_mod.Oracle(64).magnitude(amps[TWELVE])
    ulp = np.spacing(np.abs(m)).astype(np.float64)
    assert (np.abs(v[TWELVE].astype(np.float64) - m) <= tol.db_map_bound_of_power(P[TWELVE], m) + 0.5 * ulp).all(), f"{label}: against magnitude()"
    # the records' power_db field, in both hit modes: a low threshold on the leading buffers makes every evaluated bin a record
    lead = min(nb, (1 << 20) // n + 37)
    cnt = _decide(n, capi.KIND_FLOAT_COMPLEX, d_raw, lead * average, p[:lead], -300.0, label + " thr=-300", average)
    assert cnt == lead * int(tol.evaluated_mask(n).sum())
    print(f"{label}: {nb} amplitudes, {cnt} records")


@pytest.mark.parametrize("n", SIZES)
def test_flat_sweep(built_lib, oracle_mod, n):
    _flat_sweep(oracle_mod, n, 1)


@pytest.mark.parametrize("n,k", AVG, ids=[f"{n}-K{k}" for n, k in AVG])
def test_flat_sweep_averaged(built_lib, oracle_mod, n, k):
    """K identical copies per group: the mean of K equal powers is that power exactly (P + P and 4 P / 4 are exact)"""
    _flat_sweep(oracle_mod, n, k)


INT_KINDS = [k for k in KINDS if k != capi.KIND_FLOAT_COMPLEX]


@pytest.mark.parametrize("kind", INT_KINDS, ids=[NAMES[k] for k in INT_KINDS])
@pytest.mark.parametrize("n", SIZES)
def test_flat_sweep_integer(built_lib, n, kind):
    """integer impulses of k quanta (every k the int8 format has, a seeded draw of the int16 ones, both signs): the dense sweep of the
    integer kernels, product form mostly (P <= 256 with ENOB 12; the planar format's ENOB 10 reaches 4096, the int8 one's ENOB 4 252)"""
    rng = np.random.default_rng(10 * n + kind)
    top = pr.INT_MAX[kind]
    k = np.arange(1, top + 1) if top < 1000 else np.unique(np.concatenate([np.arange(1, 65), rng.integers(1, top + 1, 6000)]))
    k = np.concatenate([k, -k])
    rng.shuffle(k)
    k = k[: (1 << 22) // n + 37]
    nb = len(k)
    a = (k.astype(np.float64) * pr.scale_of(kind)).astype(F32)
    P = pr.exact_power(a.astype(np.complex64))
    label = f"flat n={n} {NAMES[kind]}"
    d_raw = _dev(pr.pack(kind, pr.line_ints(n, 0 * k, 0 * k, k)))
    ps, _, _ = _run(n, kind, d_raw, nb, 1e9, SPEC)
    p, h, t = _run(n, kind, d_raw, nb, 1e9, BOTH)
    assert len(h) == 0 and not t.any()
    _one_float(p, label)
    assert ps.tobytes() == p.tobytes(), f"{label}: spectrum-only and spectrum + hits plans store identical spectra"
    _check_map(P, p[:, 0], label)
    _note(P, p[:, 0], label)
    lead = min(nb, (1 << 19) // n + 37)
    cnt = _decide(n, kind, d_raw, lead, p[:lead], -300.0, label + " thr=-300")
    assert cnt == lead * int(tol.evaluated_mask(n).sum())


@pytest.mark.parametrize("kind", KINDS, ids=[NAMES[k] for k in KINDS])
@pytest.mark.parametrize("n", SIZES)
def test_line_probes(built_lib, oracle_mod, n, kind):
    count = 45
    i1, i3, ia = pr.line_params(kind, n, count)
    q = np.concatenate([pr.line_ints(n, i1, i3, ia), pr.line_ints(n, 0 * ia, 0 * ia, ia)])   # the lines, then the flat probes of their floors
    nb = len(q)
    label = f"line n={n} {NAMES[kind]}"
    d_raw = _dev(pr.pack(kind, q))
    p, _, _ = _run(n, kind, d_raw, nb, 1e9, BOTH)
    ps, _, _ = _run(n, kind, d_raw, nb, 1e9, SPEC)
    assert ps.tobytes() == p.tobytes()
    h1, h3, fl = pr.line_values(kind, n, i1, i3, ia)
    P1, P3, Pf = (pr.exact_power(x.astype(np.complex64)) for x in (h1, h3, fl))
    assert (P1 >= tol.P_EXACT_FROM).all() and (Pf < tol.P_EXACT_FROM).all(), "the line takes the exact half of the map, its floor the product form"
    _one_float(p[count:], label + " (flat part)")
    _check_map(Pf, p[count:, 0], label + " (flat part)")
    _note(Pf, p[count:, 0], label + " (flat part)")
    floor = np.ones(n, bool)
    floor[[n // 4, 3 * n // 4]] = False
    same = p[:count][:, floor].view(np.uint32) == p[count:, :1].view(np.uint32)
    if n not in LINE_INEXACT:
        assert same.all(), (f"{label}: the floor of a line probe is not the flat probe of its amplitude in {int((~same).sum())} bins "
                            f"(a pass multiplies nonzero data by a twiddle that is not exact: LINE_INEXACT?)")
    eps = None
    if n in LINE_INEXACT:
        # the tone sweep's bound with the tone sweep's eps at this size (measuring eps on the line probes themselves is void: both
        # comparison transforms are EXACT on small integers -- 7e-16 for int8 at 1000 points), under the tone sweep's condition
        eps = _tone_eps(oracle_mod, n)
        for P in (P1, P3):
            assert (pr.db64(P) > 32.0).all() and (pr.db64(P) < 64.0).all(), "the tone sweep's bound is for lines in 32 ... 64 dB"
        # the floors: a float32 transform's error on ANY bin scales with the buffer's strongest components, so the relative amplitude
        # deviation eps / 2 measured on a line becomes (eps / 2) (L1 + L3) / a on a floor of amplitude a -- loose where the floor is
        # thousands of times weaker than the lines (int16), a few 1e-3 dB in int8; it still fails a floor that is garbage
        delta = 0.5 * eps * (np.abs(h1).astype(np.float64) + np.abs(h3)) / np.abs(fl).astype(np.float64)
        df = pr.db64(Pf)
        hi = df + tol.db_map_bound(df) + 10.0 * np.log10(1.0 + delta)
        with np.errstate(divide="ignore", invalid="ignore"):
            lo = np.where(delta < 1.0, df - tol.db_map_bound(df) + 10.0 * np.log10(np.maximum(1.0 - delta, 1e-300)), -np.inf)
        pf = p[:count][:, floor].astype(np.float64)
        assert ((pf <= hi[:, None]) & (pf >= lo[:, None])).all(), f"{label}: a floor bin outside the map's bound plus the transform's error"
    for P, j in ((P1, n // 4), (P3, 3 * n // 4)):
        _check_map(P, p[:count, j], f"{label} bin {j}", eps)
        if n not in LINE_INEXACT:
            _note(P, p[:count, j], f"{label} bin {j}")
    # records: the lines above 10 dB and whatever floor is (none: Pf < 100 in every format)
    _decide(n, kind, d_raw, nb, p, 12.0, label + " thr=12")


SPECIALS = {1: 0.0, 2: 2.0 ** 64, 17: np.nan, 38: -(2.0 ** 70), 39: complex(1.0, np.nan), 63: 0.0, 64: complex(0.0, 3.0e38), 96: np.nan}


@pytest.mark.parametrize("n", SIZES)
def test_special_values_do_not_leak(built_lib, n):
    """P = 0, P = +inf and NaN buffers among ordinary ones (flat probes on both sides of the threshold and line probes), placed so
    that in the 16 ... 512-point kernels they share a wave -- and the segmented prefix sums of the hit slots -- with ordinary ones"""
    kind = capi.KIND_FLOAT_COMPLEX
    rng = np.random.default_rng(n)
    nb = 101
    x = pr.flat_raw(n, np.exp2(rng.uniform(-2, 9, nb)).astype(F32))
    i1, i3, ia = pr.line_params(kind, n, 20)
    x[5::5] = pr.pack(kind, pr.line_ints(n, i1, i3, ia))[: len(x[5::5])]
    for b in SPECIALS:
        assert b % 5
    y = x.copy()
    for b, a in SPECIALS.items():
        y[b] = pr.flat_raw(n, [a])[0]
    thr = 10.0
    label = f"special n={n}"
    res = {}
    for name, raw in (("plain", x), ("special", y)):
        d_raw = _dev(raw)
        p, _, _ = _run(n, kind, d_raw, nb, 1e9, BOTH)
        cap = _n_hits(p, n, thr) + 1024
        pb, h, t = _run(n, kind, d_raw, nb, thr, BOTH, cap)
        assert pb.tobytes() == p.tobytes()
        _check_hits(p, h, t, n, thr, 1, f"{label} {name}")
        _, hh, th = _run(n, kind, d_raw, nb, thr, HITS, cap)
        assert hh.tobytes() == h.tobytes() and np.array_equal(th, t), f"{label} {name}: hits-only"
        res[name] = (p, h, t)
    (p0, h0, t0), (p1, h1, t1) = res["plain"], res["special"]
    assert len(h0) > 50 and t0.any() and not t0.all()
    ordinary = np.ones(nb, bool)
    ordinary[list(SPECIALS)] = False
    assert p1[ordinary].tobytes() == p0[ordinary].tobytes(), f"{label}: a special buffer changed an ordinary buffer's spectrum"
    keep0 = ordinary[(h0["seq_id"] - np.uint64(SEQ0)).astype(np.int64)]
    keep1 = ordinary[(h1["seq_id"] - np.uint64(SEQ0)).astype(np.int64)]
    assert h1[keep1].tobytes() == h0[keep0].tobytes(), f"{label}: a special buffer changed an ordinary buffer's records"
    assert np.array_equal(t1[ordinary], t0[ordinary])
    bits = p1.view(np.uint32)
    n_ev = int(tol.evaluated_mask(n).sum())
    counts = np.bincount((h1["seq_id"] - np.uint64(SEQ0)).astype(np.int64), minlength=nb)
    for b, a in SPECIALS.items():
        if a == 0.0:
            assert (bits[b] == 0xFF800000).all() and counts[b] == 0 and not t1[b], f"{label}: P = 0 gives -inf and no record (buffer {b})"
        elif np.isnan(a):
            assert np.isnan(p1[b]).all() and counts[b] == 0 and not t1[b], f"{label}: a NaN sample gives an all-NaN buffer, no record, no trigger (buffer {b})"
        else:
            assert (bits[b] == 0x7F800000).all() and counts[b] == n_ev and t1[b], f"{label}: an overflowing power gives +inf, as in the reference (buffer {b})"


@pytest.mark.parametrize("n", SIZES)
def test_denormal_powers(built_lib, n):
    """The stated limit: a power below FLT_MIN -- a denormal float or zero -- maps to -inf and forms no record at any threshold;
    FLT_MIN itself and its neighbours above are ordinary values (-189.65 dB) and are reported."""
    kind = capi.KIND_FLOAT_COMPLEX
    a = np.concatenate([np.exp2(np.linspace(-76.0, -63.02, 48)), [2.0 ** -63, 2.0 ** -63 * 1.0000002, 2.0 ** -62.5, 2.0 ** -75, 2.0 ** -74.5]]).astype(F32)
    P = pr.exact_power(a.astype(np.complex64))
    tiny = np.finfo(F32).tiny
    den = P < tiny
    assert (P[den] > 0).sum() >= 40 and (P == 0).any() and (P == tiny).any() and (~den).sum() >= 3
    nb = len(a)
    d_raw = _dev(pr.flat_raw(n, a))
    p, _, _ = _run(n, kind, d_raw, nb, 1e9, BOTH)
    label = f"denormal n={n}"
    _one_float(p, label)
    assert (p[den].view(np.uint32) == 0xFF800000).all(), (f"{label}: the map of a denormal power is -inf; got "
                                                          f"{[(float(x), float(y)) for x, y in zip(P[den][:6], p[den, 0][:6])]}")
    _check_map(P[~den], p[~den, 0], label)
    _note(P[~den], p[~den, 0], label)
    cnt = _decide(n, kind, d_raw, nb, p, -250.0, label + " thr=-250")
    assert cnt == int((~den).sum()) * int(tol.evaluated_mask(n).sum())
    _, hh, _ = _run(n, kind, d_raw, nb, -np.inf, HITS, cnt + 1024)
    assert len(hh) == cnt, f"{label}: threshold -inf"


# ---- the decision on the knife edge ---------------------------------------------------------------------------------------------
def _ladders(n, kind):
    """(name, raw buffers, index of the representative bin, middle buffer) per ladder"""
    out = []
    if kind == capi.KIND_FLOAT_COMPLEX:
        for name, amps in (("below", pr.float_ladder(20.0, 20, 20).astype(np.complex64)), ("across", pr.power_ladder(tol.P_EXACT_FROM, 40, 40)),
                           ("strong", pr.float_ladder(31623.0, 30, 30).astype(np.complex64))):
            out.append((name, pr.flat_raw(n, amps), 8 % n if n > 16 else 5, len(amps) // 2))
    i1, i3, _ = pr.line_params(kind, n, 1)
    cnt = 41
    ia = 1 + np.arange(cnt)
    out.append(("line", pr.pack(kind, pr.line_ints(n, np.repeat(i1, cnt), np.repeat(i3, cnt), ia)), n // 4, cnt // 2))
    return out


KNIFE = [(n, k, 1) for n in SIZES for k in KINDS] + [(n, capi.KIND_FLOAT_COMPLEX, k) for n, k in AVG]


@pytest.mark.parametrize("n,kind,average", KNIFE, ids=[f"{n}-{NAMES[k]}" + (f"-K{a}" if a > 1 else "") for n, k, a in KNIFE])
def test_knife_edge(built_lib, n, kind, average):
    assert tol.evaluated_mask(n)[[8 % n if n > 16 else 5, n // 4]].all()
    for name, raw, j, mid in _ladders(n, kind):
        label = f"knife n={n} {NAMES[kind]} K={average} ladder {name}"
        nb = len(raw) * average
        d_raw = _dev(np.repeat(raw, average, axis=0))
        p0, h, t = _run(n, kind, d_raw, nb, 1e9, BOTH, average=average)
        assert len(h) == 0 and not t.any()
        v = p0[:, j]
        T = v[mid]
        # the condition every ladder must meet (not a measurement): buffers ON the threshold, above it and below it
        assert (v == T).any() and (v > T).any() and (v < T).any(), f"{label}: {np.unique(v).tolist()} around T = {T!r}"
        got = []
        for thr in (T, np.nextafter(T, F32(np.inf)), np.nextafter(T, F32(-np.inf))):
            got.append(_decide(n, kind, d_raw, nb, p0, float(thr), f"{label} thr={thr!r}", average))
        assert got[2] > got[0] >= got[1], f"{label}: {got}"   # the buffers on T appear only once the threshold is below T
        on_T = int((v == T).sum())
        if name != "line":
            n_ev = int(tol.evaluated_mask(n).sum())
            assert got[2] - got[0] == on_T * n_ev, f"{label}: the {on_T} buffers that report T itself have no record at T and all of theirs below it"


# ---- every output position ------------------------------------------------------------------------------------------------------
TONE_AMPS = (2.0 ** 12, 2.0 ** 15, 2.0 ** 18)   # N A = c 2^m with a seeded mantissa c in [1, 2) per tone: lines at 36.1 ... 57.2 dB, all mantissas


def _tones(n, bins, amp):
    """complex64 [B, n]: amp / n * exp(2 pi i k n' / n) on the grid, from one float64 table; and the float64 line X[k] of the FLOAT samples"""
    tab = np.exp(2j * np.pi * np.arange(n) / n)
    amp = np.broadcast_to(np.asarray(amp, np.float64), (len(bins),))[:, None]
    x, X = np.empty((len(bins), n), np.complex64), np.empty(len(bins), np.complex128)
    for lo in range(0, len(bins), 256):
        idx = (bins[lo:lo + 256, None].astype(np.int64) * np.arange(n, dtype=np.int64)[None, :]) % n
        w = tab[idx]
        x[lo:lo + 256] = ((amp[lo:lo + 256] / n) * w).astype(np.complex64)
        X[lo:lo + 256] = (x[lo:lo + 256].astype(np.complex128) * np.conj(w)).sum(axis=1)
    return x, X


def _power(X):
    X = np.asarray(X)
    return X.real.astype(np.float64) ** 2 + X.imag.astype(np.float64) ** 2


def _tone_inputs(n):
    """(bins, [(N A, samples, float64 lines)] per amplitude set) of the tone sweep at n points"""
    count = min(n, (1 << 24) // n)
    # one tone per stratum of n / count consecutive bins, at a seeded offset inside the stratum: the bins spread over the whole
    # spectrum (gaps below two strata), and bin mod 16 / 32 / 256 takes every value (every bin where count = n)
    b = np.arange(count, dtype=np.int64)
    start = (b * n) // count
    off = 7 * b if n // count >= 64 else np.random.default_rng(7 * n).integers(0, 1 << 30, count)   # (wide strata: walk through them)
    bins = start + off % (((b + 1) * n) // count - start)
    assert len(np.unique(bins)) == count and bins[0] <= n // count and bins[-1] >= n - 1 - n // count
    assert count == 1 or np.diff(bins).max() <= 2 * -(-n // count)
    for m in (16, 32, 256):
        if count >= 4 * m and n % m == 0:
            assert len(np.unique((bins * m) // n)) == m, (n, m)
        if count >= 16 * m and n % m == 0:
            assert len(np.unique(bins % m)) == m, (n, m)
    if n == 65536:   # the four-step rows kernel: k = k1 + 256 k2, a thread's 16 outputs are k2 = pl + 8 h + 16 q
        k2 = bins >> 8
        assert len(np.unique(k2 % 16)) == 16 and len(np.unique(k2 // 16)) == 16 and len(np.unique(bins & 255)) == 256
    rng = np.random.default_rng(n)
    return bins, [(amp,) + _tones(n, bins, amp * rng.uniform(1.0, 2.0, count)) for amp in TONE_AMPS]


_EPS = {}


def _tone_eps(oracle_mod, n, inputs=None):
    """eps of a size: twice the larger relative power deviation from float64 of two float32 transforms that are not the kernel under
    test -- the oracle's FFT and scipy.fft on complex64 --, on 3 x 107 = 321 lines of the tone sweep's own inputs"""
    if n not in _EPS:
        import scipy.fft

        bins, sets = inputs or _tone_inputs(n)
        sub = np.unique(np.linspace(0, len(bins) - 1, min(len(bins), 107)).astype(np.int64))
        fo = oracle_mod.Oracle(n)
        eps = 0.0
        for _, x, X in sets:
            P64 = _power(X)
            for b in sub:
                eps = max(eps, abs(_power(fo.fft(x[b])[bins[b]]) - P64[b]) / P64[b])
            Xs = scipy.fft.fft(x[sub], axis=1)[np.arange(len(sub)), bins[sub]]
            assert Xs.dtype == np.complex64
            eps = max(eps, float((np.abs(_power(Xs) - P64[sub]) / P64[sub]).max()))
        _EPS[n] = 2.0 * float(eps)
    return _EPS[n]


@pytest.mark.parametrize("n", TONE_SIZES)
def test_tone_sweep(built_lib, oracle_mod, n):
    kind = capi.KIND_FLOAT_COMPLEX
    bins, sets = _tone_inputs(n)
    count = len(bins)
    eps = eps_all = _tone_eps(oracle_mod, n, (bins, sets))
    worst = 0.0
    for amp, x, X in sets:
        P64 = _power(X)
        d = 5.0 * np.log10(P64)
        assert (d > 32.0).all() and (d < 64.0).all()
        ulp = np.spacing(d.astype(F32)).astype(np.float64)
        bound_ulp = 1.0 + (5.0 / math.log(10.0)) * eps / ulp
        assert bound_ulp.max() <= TONE_CAP_ULP, f"n={n}: eps {eps:.2e} makes the bound {bound_ulp.max():.2f} ulp: the test could not tell the two forms apart"
        d_raw = _dev(x)
        p, _, _ = _run(n, kind, d_raw, count, 1e9, BOTH)
        v = p[np.arange(count), bins].astype(np.float64)
        err = np.abs(v - d) / ulp
        worst = max(worst, float(err.max()))
        bad = err > bound_ulp
        assert not bad.any(), (f"tone n={n} N A={amp}: {int(bad.sum())} lines outside 1.0 ulp + eps ({bound_ulp.max():.2f} ulp); worst "
                               f"{[(int(bins[k]), round(float(err[k]), 3)) for k in np.argsort(-err)[:6]]} (bin, ulp)")
        # the same lines through the hit path: records of both hit modes carry the float the spectrum holds
        cnt = _decide(n, kind, d_raw, count, p, 30.0, f"tone n={n} N A={amp} thr=30")
        assert cnt >= int(tol.evaluated_mask(n)[bins].sum())
    _FIG["eps"][n], _FIG["tone"][n] = eps_all, worst
    print(f"tone n={n}: {count} bins x {len(TONE_AMPS)} amplitudes, eps {eps_all:.2e}, worst line error {worst:.3f} ulp")


def test_zz_figures(request):
    """prints what the module measured; where the whole module ran in this process (no -k, no deselection by node id, no xdist
    worker), asserts that the purity table and the figures were really filled"""
    mine = [i for i in request.session.items if i.fspath.basename == "test_db_map_gpu.py"]
    whole = not request.config.option.keyword and not hasattr(request.config, "workerinput") and len(mine) >= 250
    if whole and mine[-1].name == "test_zz_figures":
        assert len(_PURE) >= 20000 and _LAUNCH[0] >= 1500 and len(_FIG["eps"]) == len(TONE_SIZES), (len(_PURE), _LAUNCH[0])
        assert _FIG["exact"][1] is not None and _FIG["fast"][1] is not None
    print(f"map error, product form (P < SCN_P_EXACT_FROM): {_FIG['fast'][0]:.3f} ulp at P = {_FIG['fast'][1]!r} [{_FIG['fast'][2]}]")
    print(f"map error, product form where the 4.2e-6 dB floor is the bound: {_FIG['fast_abs'][0]:.3e} dB at P = {_FIG['fast_abs'][1]!r} [{_FIG['fast_abs'][2]}]")
    print(f"map error, exact form (P >= SCN_P_EXACT_FROM): {_FIG['exact'][0]:.3f} ulp at P = {_FIG['exact'][1]!r} [{_FIG['exact'][2]}]")
    print(f"purity: {len(_PURE)} distinct powers, each with one dB value over {_LAUNCH[0]} launches")
    print("eps per size: " + ", ".join(f"{n}: {e:.2e}" for n, e in _FIG["eps"].items()))
    print("worst tone-line error per size (ulp): " + ", ".join(f"{n}: {e:.3f}" for n, e in _FIG["tone"].items()))
