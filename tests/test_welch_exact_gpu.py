"""The Welch PSD path (scn_welch.hip, scn_welch_plan.hip; BASELINE config C5) held the way every other kernel family is held by
tests/test_db_map_gpu.py: TO THE BIT on streams whose every PSD bin is known exactly (tests/welch_probes.py, pinned on the host by
tests/test_welch_probes_cpu.py), on special values, and under every window type.  tests/test_welch.py compares the same path with
the oracle and float64 inside the 1e-5 bar on random streams; what that bar cannot see is asserted here.

(a) The mean and the map.  All four wire formats, K = 1, 2, 3, 4, 5, 7, 16, plans with 1, 2 and 4 row parts (asserted via
    WelchPlan.partition where the device has 256 CUs), among them the shape whose column workgroups carry halves across segments
    (K = 4, 13 PSDs of 16: 26 column groups of 2 segments) and the one whose last column group is ragged (K = 5, 11 PSDs of 16).
    Per launch, before anything else, the structure: all even bins of a PSD hold one bit pattern, all odd bins another (flat
    stream; the line stream leaves bin N/4 out).  Then every reported value within
    tolerances.db_map_bound_of_power(m, 5 log10 m) of float64, m = welch_probes.mean_float(...) -- the float the kernels owe the
    map; purity {mean bits -> dB bits} over every launch of this module, whichever epilogue (the row kernel's parts == 1 one or
    the combine kernel) and submit path wrote it; the same stream gives the same bytes on the parts == 1 plan and on the parts > 1
    plans of one K, and through the device and the pinned / hipGraph submit.
    THE LINE STREAM is found exact in the 256 x 256 decomposition without a reference: its floor bins hold the bits of the flat
    stream of the same block amplitudes (asserted in every case; LINE_EXACT would be the place to say otherwise).
(b) Which float the mean is: the PRODUCT of the sum with the float 1/K (include/scanner_hip.h).  For K = 3, 5, 7 the pins of
    welch_probes.pin_streams owe the map, under the product form only, the very float a K = 4 partner stream owes (where the mean
    is exact under either form): both must report the same bits, from the parts == 1 and the parts == 2 plan.  Under the
    division the K-stream's mean is the neighbouring float, whose correctly rounded dB value is another float.
(c) Special values on the cfloat flat stream, at the carrying shape and at a parts == 4 shape that carries too (K = 16, 4 PSDs
    of 4): a zero stream gives -inf everywhere; a NaN sample / an amplitude of 2^64 in block b makes every bin NaN / +inf in
    exactly the PSDs {(b - 1) // K, b // K} that exist, every other PSD byte-identical to the launch without it -- with b the first
    block, the last, a PSD boundary, a block inside a PSD and the first block of a column group, the sample once in each of the
    column kernel's two prefetch groups (SCN_WELCH_PF_CUT).  The NaN sits at arbitrary samples of the two groups; 2^64 sits at
    samples 0 and 16384 of the block (a8 = 0 and 4 of thread 0): only inputs 0, 4, 8, 12 of fft16 meet no rounded twiddle, and
    (1 - 6e-8) 2^128 would round to FLT_MAX, not to +inf.
(d) Every window type: K = 2, two PSDs of test_welch.py's non-stationary stream against oracle.welch under oracle.window_type(t)
    and against ref64_welch with oracle.window(t, N); the plain plan's window table (same build_window) equals the oracle's bit for
    bit; window type 9 is refused; correct_dc on a cfloat plan changes no byte.
(e) The caller's device destination d_psd_db; (f) device-path and pinned-path slots in flight together, with a graph re-capture
    while the others are pending; (g) refusals that leave the plan usable.

MODULE STATE: the purity table and the figures are module globals filled in test order; test_zz_figures prints them (-rP) and
asserts the totals only where the whole module ran.

MEASURED on an MI355X (test_zz_figures prints them; run with -rP): product form 1.594 ulp at a mean of 8.4256e-11 (bound 2.2) and
1.93e-6 dB at a mean of 662.89 where the 4.2e-6 dB floor is the bound; exact form 0.904 ulp at a mean of 2.7489e11 (bound 1.0);
1285 distinct means, one dB value each, over 539 launches.  The line stream IS exact in this decomposition, in every wire format
and shape tried.  The whole module takes 6 s (47 tests).  No kernel arithmetic was changed for this module.

MUTATION CHECKS (scripts/build_mutant.py on scn_welch.hip, the module run with SCN_LIB=...; each run only produced failing asserts):
  * `db_of_power(acc[q] * args.inv_k)` -> `db_of_power(acc[q] / (float)args.k)` in the row kernel only: 15 failed --
    test_mean_and_map at K = 3, 5, 7 in every wire format but cfloat K = 5 (purity: one mean, two dB floats, parts == 1 against
    parts > 1), test_mean_is_the_product_form at K = 3, 5 and 7 (purity against the K = 4 partner, from the parts == 1 plan alone:
    the pin sees the division without the other epilogue's help), test_zz_figures (totals);
  * `raw[a] = raw[a + 8]` -> `raw[a] = raw[a]` (the carried half goes stale): 12 failed -- test_mean_and_map at K = 4 and K = 5 in
    every wire format (the shapes with two segments per column group: every PSD whole dB outside the bound), both
    test_special_values shapes (at their baseline check), test_mean_is_the_product_form[7] (56 segments), test_zz_figures; the
    shapes with one segment per column group pass, as they must;
  * `db_of_power(sum[c] * args.inv_k)` -> `db_fast(sum[c] * args.inv_k)` in the combine kernel: 21 failed -- test_mean_and_map in
    every wire format at the parts > 1 plans, on the line bin only (the exact half: 1.07 ... 1.73 ulp against the bound 1.0, or
    purity against the parts == 1 plan), test_zz_figures."""
import ctypes as C

import numpy as np
import pytest

from scanner_amd import Plan, WelchPlan, capi
from tests import db_probes as pr
from tests import tolerances as tol
from tests import welch_probes as wp
from tests.test_welch import _nonstationary, _stream

pytestmark = pytest.mark.gpu
F32 = np.float32
N, HOP = wp.N, wp.HOP
CF = capi.KIND_FLOAT_COMPLEX
NAMES = {capi.KIND_FLOAT_COMPLEX: "cfloat", capi.KIND_SHORT_COMPLEX: "int16", capi.KIND_SHORT: "int16planar", capi.KIND_BYTE_COMPLEX: "int8"}
KINDS = list(NAMES)
NEG_INF, POS_INF = 0xFF800000, 0x7F800000
LINE_EXACT = True   # (see the module docstring: asserted, not assumed)

# K -> [(max_psd, n_psd, parts on 256 CUs)]: the parts == 1 plan first
SHAPES = {1: [(16, 5, 1)],
          2: [(16, 7, 1), (8, 7, 2)],
          3: [(16, 5, 1), (8, 5, 2)],
          4: [(16, 13, 1), (2, 2, 4)],      # 52 segments: 26 column groups of 2, the carried half consumed once in each
          5: [(16, 11, 1), (2, 2, 4)],      # 55 segments: 28 column groups of 2, the last one ragged (1)
          7: [(16, 3, 1), (8, 3, 2), (4, 3, 4)],
          16: [(16, 3, 1), (2, 2, 4)]}

_PURE = {}      # mean bits -> (dB bits, the launch that reported them)
_FIG = {"fast": (0.0, None, None), "fast_abs": (0.0, None, None), "exact": (0.0, None, None)}
_LAUNCH = [0]


@pytest.fixture(scope="module")
def torch_cuda(built_lib):
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need a GPU; refusing to skip silently"
    return torch


# ---- launching ------------------------------------------------------------------------------------------------------------------
def _bytes(raw):
    return np.ascontiguousarray(raw).view(np.uint8).reshape(-1)


def _dev(torch, raw):
    return torch.from_numpy(_bytes(raw)).cuda()


def _submit_device(w, slot, d, n_psd, out=None):
    _LAUNCH[0] += 1
    w.submit_device(slot, d, n_psd, d_psd_db=out)


def _submit_pinned(w, slot, raw, n_psd):
    _LAUNCH[0] += 1
    raw = _bytes(raw)
    hb = w.host_buffer(slot).view(np.uint8)
    hb[: raw.size] = raw
    w.submit(slot, n_psd)


def _both_paths(torch, w, raw, n_psd, label):
    """the stream through the device path (slot 0) and the pinned / hipGraph path (slot 1), in flight together: identical bytes"""
    raw = _bytes(raw)[: w.samples(n_psd) * w.bytes_per_sample]
    _submit_device(w, 0, _dev(torch, raw), n_psd)
    _submit_pinned(w, 1, raw, n_psd)
    got, pinned = w.collect(0), w.collect(1)
    assert got.tobytes() == pinned.tobytes(), f"{label}: the pinned / hipGraph submit differs from the device submit"
    return got


def _alone(torch, K, max_psd, raw, n_psd, **kw):
    """the stream alone on a fresh plan, device path"""
    with WelchPlan(N, K, max_psd=max_psd, window_type=capi.WIN_RECTANGULAR, **kw) as w:
        _submit_device(w, 0, _dev(torch, raw), n_psd)
        return w.collect(0)


# ---- the map --------------------------------------------------------------------------------------------------------------------
def _note(m, v, label):
    m, v = np.asarray(m, F32).reshape(-1), np.asarray(v, F32).reshape(-1)
    for a, b in np.unique(np.stack([m.view(np.uint32), v.view(np.uint32)], axis=1), axis=0).tolist():
        old = _PURE.setdefault(a, (b, label))
        assert old[0] == b, (f"purity: mean {np.array(a, np.uint32).view(F32)!r} ({a:#x}) maps to {np.array(old[0], np.uint32).view(F32)!r} "
                             f"in [{old[1]}] and to {np.array(b, np.uint32).view(F32)!r} in [{label}]")


def _check_map(m, v, label):
    """reported values v of the means m (the floats the kernels owe the map) against float64, by the half of the map m takes;
    a mean of zero owes -inf"""
    m, v = np.asarray(m, F32).reshape(-1), np.asarray(v, F32).reshape(-1)
    zero = m == 0
    assert (v[zero].view(np.uint32) == NEG_INF).all(), f"{label}: a mean of zero maps to -inf"
    m, v = m[~zero], v[~zero]
    if not m.size:
        return
    assert ((m >= np.finfo(F32).tiny) & np.isfinite(m)).all()
    d = pr.db64(m)
    ulp = np.spacing(np.abs(d).astype(F32)).astype(np.float64)
    err = np.abs(v.astype(np.float64) - d)
    exact = m >= tol.P_EXACT_FROM
    floor = tol.DB_MAP_ULP_FAST * ulp < tol.DB_MAP_ABS
    for key, sel, e in (("fast", ~exact & ~floor, err / ulp), ("fast_abs", ~exact & floor, err), ("exact", exact, err / ulp)):
        if sel.any():
            k = int(np.argmax(np.where(sel, e, -1.0)))
            if e[k] > _FIG[key][0]:
                _FIG[key] = (float(e[k]), float(m[k]), label)
    bad = ~(err <= tol.db_map_bound_of_power(m, d))
    assert not bad.any(), (f"{label}: {int(bad.sum())} of {bad.size} values outside the map's bound; worst "
                           f"{[(float(m[k]), float(v[k]), float(d[k]), round(float(err[k] / ulp[k]), 3)) for k in np.argsort(-err / ulp)[:4]]} "
                           f"(mean, device, float64, error in ulp)")


_EVEN = np.arange(N) % 2 == 0


def _structure(got, line, label):
    """within a PSD all even bins hold one bit pattern and all odd bins another (bin N/4 apart on a line stream)"""
    bits = got.view(np.uint32)
    keep = np.ones(N, bool)
    if line:
        keep[N // 4] = False
    for name, sel in (("even", keep & _EVEN), ("odd", keep & ~_EVEN)):
        b = bits[:, sel]
        bad = np.flatnonzero((b != b[:, :1]).any(axis=1))
        if bad.size:
            j = np.flatnonzero(sel)[np.flatnonzero(b[bad[0]] != b[bad[0], 0])]
            raise AssertionError(f"{label}: the {name} bins of {bad.size} PSDs hold more than one float; PSD {bad[0]}: first = "
                                 f"{got[bad[0], np.flatnonzero(sel)[0]]!r}, {j.size} bins differ, first {j[:8].tolist()} -> {got[bad[0], j[:8]].tolist()}")


def _check_stream(got, s, parts, label):
    n_psd = got.shape[0]
    _structure(got, bool(s.line), label)
    m = s.means(parts)
    for name, col in (("even", 0), ("odd", 1)) + ((("line", N // 4),) if s.line else ()):
        _check_map(m[name][:n_psd], got[:, col], f"{label} {name}")
        _note(m[name][:n_psd], got[:, col], f"{label} {name}")


# ---- (a) the mean and the map ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", list(SHAPES))
@pytest.mark.parametrize("kind", KINDS, ids=[NAMES[k] for k in KINDS])
def test_mean_and_map(torch_cuda, kind, K):
    torch = torch_cuda
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_max = max(n for _, n, _ in SHAPES[K])
    ln = wp.line(kind, K, n_max, seed=K)
    streams = {"flat": wp.flat(kind, K, n_max, seed=K), "floor": wp.Stream(kind, K, ln.ia), "line": ln}
    if kind == CF:   # flat streams moved by exact powers of two: means of -45 ... -65 dB (where 2.2 ulp is the bound) and of 40 ... 60 dB
        streams.update(small=wp.flat(kind, K, n_max, seed=K + 100, shift=2.0 ** -20), big=wp.flat(kind, K, n_max, seed=K + 200, shift=2.0 ** 9))
    res = {}
    for max_psd, n_psd, want_parts in SHAPES[K]:
        with WelchPlan(N, K, max_psd=max_psd, window_type=capi.WIN_RECTANGULAR, kind=kind, enob=pr.ENOB[kind], correct_dc=False) as w:
            parts, groups, per = w.partition(n_psd)
            if cus == 256:
                assert parts == want_parts, (parts, want_parts)
                if (K, n_psd) in ((4, 13), (5, 11)):
                    assert (groups, per) == (48, 2)                   # halves carried across segments; K = 5: the last group ragged
            for name, s in streams.items():
                label = f"{NAMES[kind]} K={K} max_psd={max_psd} n_psd={n_psd} parts={parts} {name}"
                got = _both_paths(torch, w, s.raw(n_psd), n_psd, label)
                _check_stream(got, s, parts, label)
                res[(max_psd, name)] = got
            if LINE_EXACT:
                floor = np.arange(N) != N // 4
                assert res[(max_psd, "line")][:, floor].tobytes() == res[(max_psd, "floor")][:, floor].tobytes(), \
                    f"{NAMES[kind]} K={K} max_psd={max_psd}: the floor of the line stream is not the flat stream of its amplitudes"
    # one stream, one K: the parts == 1 epilogue and the combine kernel report the same bytes (exact sums: any order, one float)
    first = SHAPES[K][0][0]
    for max_psd, n_psd, _ in SHAPES[K][1:]:
        for name in set(streams) - {"line"}:
            assert res[(max_psd, name)].tobytes() == res[(first, name)][:n_psd].tobytes(), \
                f"{NAMES[kind]} K={K} {name}: max_psd={max_psd} (row parts) and max_psd={first} (one part) report different bytes"
        floor = np.arange(N) != N // 4
        assert res[(max_psd, "line")][:, floor].tobytes() == res[(first, "line")][:n_psd][:, floor].tobytes()


def test_minus_inf_bins_on_purpose(torch_cuda):
    """opposite neighbours cancel in the even bins of PSD 0 (a mean of exactly zero -> -inf), on both epilogues"""
    s = wp.Stream(CF, 2, [300, -300, 300, 17, 90], zeros=True)
    for max_psd in (16, 8):
        with WelchPlan(N, 2, max_psd=max_psd, window_type=capi.WIN_RECTANGULAR) as w:
            got = _both_paths(torch_cuda, w, s.raw(), 2, f"zeros max_psd={max_psd}")
            _check_stream(got, s, w.partition(2)[0], f"zeros max_psd={max_psd}")
            assert (got[0, 0::2].view(np.uint32) == NEG_INF).all() and np.isfinite(got[0, 1::2]).all() and np.isfinite(got[1]).all()


# ---- (b) which float the mean is ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 5, 7])
def test_mean_is_the_product_form(torch_cuda, K):
    a, b, pins = wp.pin_streams(K, 8)
    want = a.means(1)["even"]
    assert want.tobytes() == b.means(1)["even"].tobytes()
    with WelchPlan(N, 4, max_psd=16, window_type=capi.WIN_RECTANGULAR) as w:
        ref = _both_paths(torch_cuda, w, b.raw(), 8, f"pins K=4 partner of K={K}")
        _check_stream(ref, b, w.partition(8)[0], f"pins K=4 partner of K={K}")
    for max_psd in (16, 8):
        with WelchPlan(N, K, max_psd=max_psd, window_type=capi.WIN_RECTANGULAR) as w:
            parts = w.partition(8)[0]
            label = f"pins K={K} max_psd={max_psd} parts={parts}"
            got = _both_paths(torch_cuda, w, a.raw(), 8, label)
            _check_stream(got, a, parts, label)
            assert got[:, 0].tobytes() == ref[:, 0].tobytes(), \
                (f"{label}: the even bins owe the map the float {want.tolist()} under the product form, the very mean of the K = 4 "
                 f"partner; reported {got[:, 0].tolist()} against {ref[:, 0].tolist()}")


# ---- (c) special values ---------------------------------------------------------------------------------------------------------
NAN_AT = ((4096 * 1 + 777, 0), (4096 * 6 + 1234, 1))     # (sample of the block, re / im): a8 = 1 and a8 = 6 of some thread
BIG_AT = ((0, 0), (16384, 0))                            # a8 = 0 and a8 = 4 of thread 0: fft16 inputs 0 / 8 and 4 / 12


@pytest.mark.parametrize("K,max_psd,n_psd,want_parts", [(4, 16, 13, 1), (16, 4, 4, 4)])
def test_special_values(torch_cuda, K, max_psd, n_psd, want_parts):
    torch = torch_cuda
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    s = wp.flat(CF, K, n_psd, seed=50 + K)
    x = np.ascontiguousarray(s.complex64()).view(F32)
    d = torch.from_numpy(x).cuda()
    last = n_psd * K
    with WelchPlan(N, K, max_psd=max_psd, window_type=capi.WIN_RECTANGULAR) as w:
        parts, groups, per = w.partition(n_psd)
        if cus == 256:
            assert parts == want_parts and per >= 2
        label = f"special K={K} n_psd={n_psd} parts={parts}"
        base = _both_paths(torch, w, x, n_psd, label)
        _check_stream(base, s, parts, label)
        zero = _both_paths(torch, w, np.zeros_like(x), n_psd, label + " zero stream")
        assert (zero.view(np.uint32) == NEG_INF).all(), f"{label}: a zero stream gives -inf in every bin of every PSD"
        used = -(-last // per)                                   # column groups that get segments
        blocks = sorted({0, last, K, K + 2, per, per * (used - 1)})   # first, last, PSD boundary, inside PSD 1, first of a column group (x 2)
        assert (K + 2) % K != 0 and blocks[-1] == last and used >= 2
        for b in blocks:
            hit = sorted({seg // K for seg in (b - 1, b) if 0 <= seg < last})   # the PSDs whose segments contain block b
            assert set(hit) == {p for p in ((b - 1) // K, b // K) if 0 <= p < n_psd} and 1 <= len(hit) <= 2
            keep = np.ones(n_psd, bool)
            keep[hit] = False
            for value, places, name in ((np.nan, NAN_AT, "NaN"), (2.0 ** 64, BIG_AT, "2^64")):
                for k, (pos, comp) in enumerate(places):
                    y = d.clone()
                    y[2 * (b * HOP + pos) + comp] = value
                    what = f"{label}: {name} at sample {pos} of block {b}"
                    if b == K and k == 1:   # once per special through the pinned / hipGraph path too
                        got = _both_paths(torch, w, y.cpu().numpy(), n_psd, what)
                    else:
                        _submit_device(w, 2, y, n_psd)
                        got = w.collect(2)
                    assert got[keep].tobytes() == base[keep].tobytes(), f"{what}: a PSD without block {b} changed"
                    if name == "NaN":
                        assert np.isnan(got[hit]).all(), f"{what}: PSDs {hit} are not NaN in every bin ({int(np.isnan(got[hit]).sum())} bins are)"
                    else:
                        assert (got[hit].view(np.uint32) == POS_INF).all(), \
                            f"{what}: PSDs {hit} are not +inf in every bin ({int((got[hit].view(np.uint32) == POS_INF).sum())} bins are)"


# ---- (d) every window type ------------------------------------------------------------------------------------------------------
WINDOWS = ["HAMMING", "HANN", "BLACKMAN", "RECTANGULAR", "KAISER", "BLACKMAN_HARRIS", "BARTLETT", "FLATTOP"]
_RANDOM = {}


def _random_stream():
    if "x" not in _RANDOM:
        _RANDOM["x"] = _nonstationary(_stream(2, seed=77, k=2), 2, seed=3)
    return _RANDOM["x"]


@pytest.mark.parametrize("wt", WINDOWS)
def test_every_window_type(torch_cuda, oracle_mod, wt):
    o_t, p_t = getattr(oracle_mod, "WIN_" + wt), getattr(capi, "WIN_" + wt)
    x = _random_stream()
    win = oracle_mod.window(o_t, N)
    with oracle_mod.window_type(o_t):
        ref = oracle_mod.welch(x, N, 2, 2)
    ref64 = oracle_mod.ref64_welch(x, win, N, 2, 2)
    with WelchPlan(N, 2, max_psd=2, window_type=p_t) as w:
        got = _both_paths(torch_cuda, w, x, 2, f"window {wt}")
    f1, f2 = tol.compare_spectra(got, ref), tol.compare_spectra(got, ref64)
    print(f"welch window {wt}: vs oracle {f1['max_rel_power_vs_max_bin_mean']:.2e}, vs float64 {f2['max_rel_power_vs_max_bin_mean']:.2e}")
    with Plan(N, 8000000, 1e9, max_batch=1, window_type=p_t) as plan:
        assert plan.window().tobytes() == win.tobytes(), f"{wt}: the plan's window table is not the oracle's"
    if wt not in ("RECTANGULAR", "KAISER"):   # the window does matter: the rectangular spectrum is outside the bar
        if "rect" not in _RANDOM:
            _RANDOM["rect"] = _alone(torch_cuda, 2, 2, x, 2)
        with pytest.raises(AssertionError):
            tol.compare_spectra(_RANDOM["rect"], ref)


def test_window_type_refused_and_dc_ignored_on_cfloat(torch_cuda):
    with pytest.raises(capi.ScannerError):
        WelchPlan(N, 2, max_psd=2, window_type=9)
    x = _random_stream()
    got = {}
    for dc in (False, True):
        with WelchPlan(N, 2, max_psd=2, correct_dc=dc) as w:
            got[dc] = _both_paths(torch_cuda, w, x, 2, f"cfloat correct_dc={dc}")
    assert got[True].tobytes() == got[False].tobytes(), "correct_dc on float samples changes the PSD"


# ---- (e) the caller's destination -----------------------------------------------------------------------------------------------
SENTINEL = 0x7FA5C3D2


def test_callers_device_destination(torch_cuda):
    torch = torch_cuda
    K, max_psd = 3, 4
    sa, sb = wp.flat(CF, K, 3, seed=91), wp.flat(CF, K, 2, seed=92)
    da, db = _dev(torch, sa.raw()), _dev(torch, sb.raw())
    with WelchPlan(N, K, max_psd=max_psd, window_type=capi.WIN_RECTANGULAR) as w:
        parts = w.partition(3)[0]
        _submit_device(w, 0, da, 3)
        own = w.collect(0)                                       # the plan-owned destination
        _check_stream(own, sa, parts, "destination: plan-owned")
        _submit_device(w, 0, db, 2)
        own_b = w.collect(0)
        _check_stream(own_b, sb, parts, "destination: plan-owned, second stream")

        def sentinel():
            return torch.full((max_psd * N,), SENTINEL, dtype=torch.int32, device="cuda")

        def check(t, want, what):
            h = t.cpu().numpy()
            k = want.size
            assert h[:k].tobytes() == want.tobytes(), f"{what}: the caller's tensor does not hold the plan-owned result"
            assert (h[k:] == SENTINEL).all(), f"{what}: the launch wrote past its n_psd * n floats"

        t = sentinel()
        _submit_device(w, 1, da, 3, out=t)
        assert w.collect(1, want_psd=False) is None
        check(t, own, "collect without a host buffer")
        t = sentinel()
        _submit_device(w, 1, da, 3, out=t)
        assert w.collect(1).tobytes() == own.tobytes(), "collect with a host buffer returns the caller's destination"
        check(t, own, "collect with a host buffer")
        # two slots in flight, two destinations
        ta, tb = sentinel(), sentinel()
        _submit_device(w, 2, da, 3, out=ta)
        _submit_device(w, 3, db, 2, out=tb)
        assert w.collect(3).tobytes() == own_b.tobytes()
        assert w.collect(2, want_psd=False) is None
        check(ta, own, "two destinations, slot 2")
        check(tb, own_b, "two destinations, slot 3")
        # and the plan-owned destination is still the default afterwards
        _submit_device(w, 2, db, 2)
        assert w.collect(2).tobytes() == own_b.tobytes()


# ---- (f) slots together ---------------------------------------------------------------------------------------------------------
def test_slots_in_flight_together(torch_cuda):
    torch = torch_cuda
    K, max_psd = 2, 4
    ss = [wp.flat(CF, K, max_psd, seed=200 + i) for i in range(4)]
    raws = [s.raw() for s in ss]
    alone = [_alone(torch, K, max_psd, raws[i], max_psd) for i in range(4)]
    for i in range(4):
        _check_stream(alone[i], ss[i], 2, f"slots: stream {i} alone")
        assert all(alone[i].tobytes() != alone[j].tobytes() for j in range(i))
    alone3 = _alone(torch, K, max_psd, raws[1], 3)
    assert alone3.tobytes() == alone[1][:3].tobytes()
    devs = {0: _dev(torch, raws[0]), 3: _dev(torch, raws[3])}
    with WelchPlan(N, K, max_psd=max_psd, window_type=capi.WIN_RECTANGULAR) as w:
        for n1, order in ((max_psd, (2, 0, 3, 1)), (3, (1, 3, 0, 2)), (max_psd, (3, 2, 1, 0))):   # n1: slot 1's n_psd (a change re-captures its graph)
            _submit_device(w, 0, devs[0], max_psd)
            _submit_pinned(w, 1, raws[1], n1)
            _submit_pinned(w, 2, raws[2], max_psd)
            _submit_device(w, 3, devs[3], max_psd)
            for slot in order:
                got = w.collect(slot)
                want = alone[slot][:n1] if slot == 1 else alone[slot]
                assert got.shape == want.shape and got.tobytes() == want.tobytes(), f"slots: slot {slot} (slot 1 with {n1} PSDs, collected in order {order})"


# ---- (g) refusals that leave the plan usable ------------------------------------------------------------------------------------
def test_refusals_leave_the_plan_usable(torch_cuda):
    torch = torch_cuda
    K, max_psd, n_psd = 3, 4, 3
    s = wp.flat(CF, K, n_psd, seed=300)
    raw = s.raw()
    d = _dev(torch, raw)
    turn = [0]
    with WelchPlan(N, K, max_psd=max_psd, window_type=capi.WIN_RECTANGULAR) as w:
        _submit_device(w, 0, d, n_psd)
        base = w.collect(0)
        _check_stream(base, s, w.partition(n_psd)[0], "refusals: baseline")

        def still_good(what):
            turn[0] += 1
            if turn[0] % 2:
                _submit_device(w, 0, d, n_psd)
                got = w.collect(0)
            else:
                _submit_pinned(w, 3, raw, n_psd)
                got = w.collect(3)
            assert got.tobytes() == base.tobytes(), f"after {what}: a valid submit no longer gives the right bytes"

        def refused(what, fn):
            with pytest.raises(capi.ScannerError):
                fn()
            still_good(what)

        # a submit into a pending slot, on both paths (the pending result is unharmed)
        _submit_device(w, 1, d, n_psd)
        with pytest.raises(capi.ScannerError):
            w.submit_device(1, d, n_psd)
        w.host_buffer(1)
        with pytest.raises(capi.ScannerError):
            w.submit(1, n_psd)
        assert w.collect(1).tobytes() == base.tobytes()
        still_good("a device submit into a pending slot")
        _submit_pinned(w, 2, raw, n_psd)
        with pytest.raises(capi.ScannerError):
            w.submit(2, n_psd)
        with pytest.raises(capi.ScannerError):
            w.submit_device(2, d, n_psd)
        assert w.collect(2).tobytes() == base.tobytes()
        still_good("a pinned submit into a pending slot")
    with WelchPlan(N, K, max_psd=max_psd, window_type=capi.WIN_RECTANGULAR) as w:
        refused("submit before host_buffer", lambda: w.submit(2, n_psd))
        refused("n_psd = 0, device path", lambda: w.submit_device(0, d, 0))
        w.host_buffer(1)
        refused("n_psd = 0, pinned path", lambda: w.submit(1, 0))
        refused("n_psd > max_psd, device path",
                lambda: capi.check(w._L.scn_welch_submit_device(w._h, 0, C.c_void_p(d.data_ptr()), max_psd + 1, None), "submit_device"))
        refused("n_psd > max_psd, pinned path", lambda: w.submit(1, max_psd + 1))
        refused("a null device pointer", lambda: capi.check(w._L.scn_welch_submit_device(w._h, 0, None, n_psd, None), "scn_welch_submit_device"))
        for slot in (-1, capi.NUM_SLOTS):
            refused(f"slot {slot}, device path", lambda: capi.check(w._L.scn_welch_submit_device(w._h, slot, C.c_void_p(d.data_ptr()), n_psd, None), "submit_device"))
            refused(f"slot {slot}, pinned path", lambda: capi.check(w._L.scn_welch_submit(w._h, slot, n_psd), "submit"))
            refused(f"slot {slot}, host_buffer", lambda: w.host_buffer(slot))
            refused(f"slot {slot}, collect", lambda: capi.check(w._L.scn_welch_collect(w._h, slot, None), "collect"))
        refused("collect with nothing pending", lambda: w.collect(2))


def test_zz_figures(request):
    """prints what the module measured; where the whole module ran in this process (no -k, no deselection by node id, no xdist
    worker), asserts that the purity table and the figures were really filled"""
    mine = [i for i in request.session.items if i.fspath.basename == "test_welch_exact_gpu.py"]
    whole = not request.config.option.keyword and not hasattr(request.config, "workerinput") and len(mine) >= 47
    print(f"map error, product form (mean < SCN_P_EXACT_FROM): {_FIG['fast'][0]:.3f} ulp at mean = {_FIG['fast'][1]!r} [{_FIG['fast'][2]}]")
    print(f"map error, product form where the 4.2e-6 dB floor is the bound: {_FIG['fast_abs'][0]:.3e} dB at mean = {_FIG['fast_abs'][1]!r} [{_FIG['fast_abs'][2]}]")
    print(f"map error, exact form (mean >= SCN_P_EXACT_FROM): {_FIG['exact'][0]:.3f} ulp at mean = {_FIG['exact'][1]!r} [{_FIG['exact'][2]}]")
    print(f"purity: {len(_PURE)} distinct means, each with one dB value over {_LAUNCH[0]} launches")
    if whole and mine[-1].name == "test_zz_figures":
        assert len(_PURE) >= 1000 and _LAUNCH[0] >= 500, (len(_PURE), _LAUNCH[0])
        assert _FIG["exact"][1] is not None and _FIG["fast"][1] is not None
        assert _FIG["fast"][0] <= tol.DB_MAP_ULP_FAST and _FIG["exact"][0] <= tol.DB_MAP_ULP_EXACT
