"""The averaged plans (scn_plan_desc.average = K > 1, scn_average.hip) held the way every other kernel family is held by
tests/test_db_map_gpu.py: TO THE BIT, on groups whose every bin power is known exactly (tests/average_probes.py, pinned on the host
by tests/test_average_probes_cpu.py, which also shows that the model tells the faulty forms apart on these very groups).
tests/test_average_gpu.py compares the same path with float64 inside the 1e-5 bar, roughly 170 ulp of the mean; what that bar cannot
see is asserted here: the FORM of the mean (a division by (float)K, not a product with 1.0f / K), the partition into parts, the
order in which scn_avg_combine_kernel adds them, special values inside one group, and the hit decision on the mean.

HOW A MEAN IS HELD.  m_g = average_probes.mean_float(powers of group g, K, P) is the float the kernels owe the dB map, P from
Plan.average_parts.  The reference for the BITS of the group's dB value is a plain plan (K = 1, same n, cfloat, rectangular window)
run on the flat probe average_probes.amp_of_power(m_g), whose every bin holds exactly the power m_g (the plain plan's map is held on
such probes by tests/test_db_map_gpu.py): the averaged group must report the same bits, in the spectrum of both spectrum modes and
in every record's power_db in both hit modes.  Two more partners per group run at the two neighbouring floats of m_g; a group is
DISCRIMINATING when the three partners report three different dB floats, and at least half of the groups of every case must be.
Before anything else the structure: every bin of a flat group holds one bit pattern, even and odd bins of a pair group two.

SHAPES (P as a 256-CU device gives it, asserted there; elsewhere the model takes what average_parts returns, and the restated
formula average_probes.parts_of is asserted against it): all four sizes, both layouts --
  * G = 1 and G = 5 with K = 3 (P = 2), 5 (3), 7 (4: ragged parts of 1, 2, 2, 2), 13 (7), 33 (17: wave 0 adds parts 0 and 16), 64 (32:
    the control where the reciprocal product gives the same mean; K = 130 is nearly one too, see test_average_probes_cpu.py), 130
    (65: every wave of the combine kernel runs its four-loads-in-flight loop once, wave 0 the tail too);
  * P = 1, K = 3 with G = slots + 5 (slots = 3072 / 1536 / 768 / 512): the in-kernel epilogue, two items on some persistent workgroups;
  * pair groups in the four wire formats with correct_dc 0 and 1 (identical bytes), K = 3, 5, 7 at G = 5 and K = 3 at the P = 1 shape
    (1024 and 8192 points): sums exact in any order, the division alone rounds.  Both the even and the odd bins' value must be the
    partner's bits; the discriminating share is counted on the even bins, whose mean the generator places (the odd bins' is far lower).
DECISIONS: per case thresholds ON one group's reported value and at its two neighbouring floats; the hit list of the spectrum + hits
plan is exactly {evaluated bins with stored dB > threshold} ordered by (group, i), seq_id that of the group's first buffer, trigger =
count > trigger_count; the hits-only plan returns the same bytes.
SPECIAL VALUES (test_special_values): cfloat flat groups at the P = 1 multi-item shape and at G = 5, K = 7 (P = 4), the special member
first, in the middle and last in its group (first and last part), in a group that is the first item of a workgroup that goes on to a
second (w and w + gridDim.x) and in that second item.  Every other group byte-identical to the launch without it (spectrum, records,
trigger).  A NaN in re or im: the whole group NaN, no record, no trigger.  2^64: +inf in every bin, one record per evaluated bin,
trigger.  All-zero group: -inf, no record at any threshold, -inf included.  Three finite members of 2^126.8: +inf on both epilogues.
One member of 1.5 * 2^-126, the rest zero: a denormal mean, -inf and no record at -inf or -250 dB (the FLT_MIN limit of scn_device.h
applied to the mean).  Denormal members around one normal member: the IEEE model with denormals kept, to the bit.

MODULE STATE: the figures are module globals filled in test order; test_zz_figures prints them (-rP) and asserts the coverage classes
(P = 1 multi-item, P = 2, 2 < P <= 16, 16 < P < 49, P >= 49, both layouts, four sizes, four wire formats) where the whole module ran.

MEASURED on an MI355X (profiles/average_exact.md; test_zz_figures prints the figures, run with -rP): P as named at every shape;
26309 of 27008 groups discriminating, the lowest case 4 of 6; worst map deviation 1.82 ulp of the value, 1.36e-6 dB, 0.32 of
tolerances.db_map_bound_of_power; 89 tests and 4208 launches in 22 s, the slowest test 1.1 s.  No difference from the model anywhere,
the denormal-member case included: no kernel or header was changed for this module.

MUTATION CHECKS (scripts/build_mutant.py on scn_average.hip, the module run with SCN_LIB=...; each run only produced failing asserts):
  * `acc[16 * hh + o] / kf` -> `* (1.0f / kf)` in the power kernel's epilogue only: 16 failed -- all eight of
    test_in_kernel_epilogue_over_two_items (1616 ... 1628 of 3077 groups report the partner above or below) and test_pair_groups at
    1024 and 8192 points in every wire format (the sizes with the P = 1 shape); every P > 1 test passes, as it must;
  * `s / (float)args.k` -> `s * (1.0f / (float)args.k)` in the combine kernel only: 58 failed -- test_small_group_counts at K = 3, 5,
    7, 13, 33 in every size and layout (40) and at K = 130 once (1024 points, sweeps: the one sum in 64 where the two forms differ
    there), all 16 of test_pair_groups, test_zz_figures (coverage classes); K = 64 and the P = 1 tests pass, as they must;
  * the combine kernel adds its wave sums in reverse order: 47 failed -- test_small_group_counts at 47 of the 48 cases with K >= 5
    (P >= 3; all but 1024 points, dwell, K = 7); K = 3 (two waves: a + b = b + a) and the pair groups (exact sums) pass, as they must;
  * `k_end` of AvgCursor::start_item from `q K / P + K / P`: 61 failed -- test_small_group_counts at K = 3, 5, 7, 13, 33 (40: a member
    dropped wherever P does not divide K; K = 64 and 130 pass, as they must), all 16 of test_pair_groups, test_special_values at the
    four split shapes (K = 7, P = 4), test_zz_figures."""
import time

import numpy as np
import pytest

from scanner_amd import Plan, capi
from tests import average_probes as ap
from tests import db_probes as pr
from tests import tolerances as tol

pytestmark = pytest.mark.gpu
F32 = np.float32
FS = 8000000
FC = 100e6
SEQ0 = 1 << 33
BOTH, HITS, SPEC = capi.OUT_SPECTRUM | capi.OUT_HITS, capi.OUT_HITS, capi.OUT_SPECTRUM
CF = capi.KIND_FLOAT_COMPLEX
NAMES = {capi.KIND_FLOAT_COMPLEX: "cfloat", capi.KIND_SHORT_COMPLEX: "int16", capi.KIND_SHORT: "int16planar", capi.KIND_BYTE_COMPLEX: "int8"}
KINDS = list(NAMES)
LAYOUT = {capi.AVG_DWELL: "dwell", capi.AVG_SWEEPS: "sweeps"}
NEG_INF, POS_INF = 0xFF800000, 0x7F800000
assert (capi.AVG_DWELL, capi.AVG_SWEEPS) == (ap.AVG_DWELL, ap.AVG_SWEEPS)

_T0 = time.time()
_LAUNCH = [0]
_FIG = {"parts": {}, "disc": {}, "map": (0.0, None, None), "map_abs": (0.0, None, None), "map_rel": (0.0, None, None), "classes": set()}


@pytest.fixture(scope="module")
def torch_cuda(built_lib):
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need a GPU; refusing to skip silently"
    return torch


def _cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _slots(torch, n):
    return _cus(torch) * ap.WG_PER_CU[n]


# ---- launching ------------------------------------------------------------------------------------------------------------------
def _dev(torch, raw):
    return torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).reshape(-1)).cuda()


class Case:
    """one input on the device and the plan parameters it runs under"""

    def __init__(self, torch, n, kind, G, K, layout, raw=None, d_raw=None, dc=False, enob=12):
        self.torch, self.n, self.kind, self.G, self.K, self.layout, self.dc, self.enob = torch, n, kind, G, K, layout, dc, enob
        self.d_raw = _dev(torch, raw) if d_raw is None else d_raw
        self.seq = ap.first_buffer(G, K, layout).astype(np.uint64) + np.uint64(SEQ0)   # what a group's records carry

    def plan(self, thr, flags, cap=4096):
        nb = self.G * self.K
        return Plan(self.n, FS, thr, kind=self.kind, enob=self.enob, correct_dc=bool(self.dc), max_batch=nb, max_hits=cap, flags=flags,
                    trigger_count=1, window_type=capi.WIN_RECTANGULAR, average=self.K, average_layout=self.layout)

    def parts(self):
        with self.plan(1e9, SPEC) as plan:
            return plan.average_parts(self.G * self.K)

    def submit(self, plan, d_raw=None):
        nb = self.G * self.K
        slot = _LAUNCH[0] % capi.NUM_SLOTS
        _LAUNCH[0] += 1
        plan.submit_device(slot, self.d_raw if d_raw is None else d_raw, nb, np.full(nb, FC), np.arange(nb, dtype=np.uint64) + np.uint64(SEQ0))
        return plan.collect(slot)

    def run(self, thr, flags, cap=4096):
        with self.plan(thr, flags, cap) as plan:
            return self.submit(plan)


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


def _check_hits(case, p, h, t, thr, what):
    g, i, d, trig = _expected(p, case.n, thr)
    assert len(h) == len(g), f"{what}: {len(h)} records, the reported floats owe {len(g)}"
    assert np.array_equal(h["seq_id"], case.seq[g]), f"{what}: a record carries the seq_id of its group's first buffer"
    assert np.array_equal(h["i"], i.astype(np.uint32)), what
    assert h["power_db"].tobytes() == d.tobytes(), f"{what}: a record carries the float the spectrum holds"
    assert np.array_equal(t, trig), f"{what}: trigger flags follow the counts"
    return len(g)


def _decide(case, p0, thr, what, plans=None, d_raw=None):
    """spectrum + hits and hits-only plans at threshold thr against the floats p0 a plan of threshold 1e9 reported (or, with `plans`
    = (spectrum + hits plan, hits-only plan) of that threshold, whatever the spectrum + hits plan reports); returns (p, h, t)"""
    cap = len(_expected(p0, case.n, thr)[0]) + 1024 if p0 is not None else None
    if plans is None:
        p, h, t = case.run(thr, BOTH, cap)
        ph, hh, th = case.run(thr, HITS, cap)
    else:
        p, h, t = case.submit(plans[0], d_raw)
        ph, hh, th = case.submit(plans[1], d_raw)
    if p0 is not None:
        assert p.tobytes() == p0.tobytes(), f"{what}: the spectrum does not depend on the threshold"
    _check_hits(case, p, h, t, thr, what)
    assert ph is None
    assert len(hh) == len(h), f"{what}: hits-only plan reports {len(hh)} records, spectrum + hits {len(h)}"
    assert hh.tobytes() == h.tobytes(), f"{what}: hits-only records are byte-identical to spectrum + hits records"
    assert np.array_equal(th, t), what
    return p, h, t


# ---- structure, partners, the map -----------------------------------------------------------------------------------------------
def _one_float(p, label, step=1):
    """every bin (step = 2: every even bin, and every odd bin) of a group holds one bit pattern"""
    b = p.view(np.uint32)
    for off in range(step):
        s = b[:, off::step]
        bad = np.flatnonzero((s != s[:, :1]).any(axis=1))
        if bad.size:
            k = bad[0]
            j = np.flatnonzero(s[k] != s[k, 0]) * step + off
            raise AssertionError(f"{label}: {bad.size} groups hold more than one float in their bins {off} mod {step}; group {k}: bin {off} = "
                                 f"{p[k, off]!r}, {j.size} bins differ, first j = {j[:8].tolist()} -> {p[k, j[:8]].tolist()}")


def _partners(torch, n, m, label):
    """float32 [3, len(m)]: what a plain plan of n points reports on the flat probes of exactly the power below m, m, and above m"""
    m = np.asarray(m, F32)
    lo, hi = ap.neighbours(m)
    amps = ap.amp_of_power(np.concatenate([lo, m, hi]))
    nb = len(amps)
    slot = _LAUNCH[0] % capi.NUM_SLOTS
    _LAUNCH[0] += 1
    with Plan(n, FS, 1e9, kind=CF, correct_dc=False, max_batch=nb, flags=SPEC, trigger_count=1, window_type=capi.WIN_RECTANGULAR) as plan:
        plan.submit_device(slot, _dev(torch, pr.flat_raw(n, amps)), nb, np.full(nb, FC), np.arange(nb, dtype=np.uint64))
        p, _, _ = plan.collect(slot)
    _one_float(p, f"{label}: plain partners")
    return p[:, 0].reshape(3, len(m)).copy()


def _same_bits(v, part, m, label):
    """the reported floats v are the bits of the partners at m; the message says which neighbour a wrong one matches"""
    vb, pb = np.asarray(v, F32).view(np.uint32), part.view(np.uint32)
    bad = np.flatnonzero(vb != pb[1])
    if bad.size:
        def who(g):
            return "the partner BELOW" if vb[g] == pb[0, g] else "the partner ABOVE" if vb[g] == pb[2, g] else "no partner"
        raise AssertionError(f"{label}: {bad.size} of {len(vb)} groups do not report the bits of the plain plan at the model mean; first "
                             f"{[(int(g), float(m[g]), float(v[g]), float(part[1, g]), who(g)) for g in bad[:4]]} (group, model mean, reported, partner, matches)")


def _discriminating(part):
    return (part[0] != part[1]) & (part[1] != part[2])


def _check_map(m, v, label):
    """the reported values against float64 and tolerances.db_map_bound_of_power (every mean of this module takes the product form)"""
    m, v = np.asarray(m, F32).reshape(-1), np.asarray(v, F32).reshape(-1)
    assert ((m >= np.finfo(F32).tiny) & (m < tol.P_EXACT_FROM)).all()
    d = pr.db64(m)
    ulp = np.spacing(np.abs(d).astype(F32)).astype(np.float64)
    err = np.abs(v.astype(np.float64) - d)
    bound = tol.db_map_bound_of_power(m, d)
    # (every value of this module lies below 16 dB in magnitude, where the 4.2e-6 dB floor is the bound and 2.2 ulp lie inside it)
    for key, e in (("map", err / ulp), ("map_abs", err), ("map_rel", err / bound)):
        k = int(np.argmax(e))
        if e[k] > _FIG[key][0]:
            _FIG[key] = (float(e[k]), float(m[k]), label)
    bad = ~(err <= bound)
    assert not bad.any(), f"{label}: {int(bad.sum())} of {bad.size} values outside the map's bound"


def _classes(parts, G, layout, n, kind, multi_item=False):
    c = _FIG["classes"]
    c.update({("layout", layout), ("n", n), ("kind", kind)})
    if parts == 1 and multi_item:
        c.add("P=1 multi-item")
    for name, ok in (("P=2", parts == 2), ("2<P<=16", 2 < parts <= 16), ("16<P<49", 16 < parts < 49), ("P>=49", parts >= 49)):
        if ok:
            c.add(name)


def _thresholds(v):
    """one group's reported value (the median group; of many groups one near the top, so that the records stay few) and its neighbours"""
    order = np.argsort(v, kind="stable")
    T = v[order[len(v) // 2 if len(v) <= 100 else (97 * len(v)) // 100]]
    return T, np.nextafter(T, F32(np.inf)), np.nextafter(T, F32(-np.inf))


# ---- flat groups: the form of the mean, the partition, the combine order -------------------------------------------------------
def _hold_flat(torch, n, layout, K, G, named_parts, multi_item=False):
    label = f"flat n={n} {LAYOUT[layout]} K={K} G={G}"
    parts = Case(torch, n, CF, G, K, layout, d_raw=0).parts()
    assert parts == ap.parts_of(n, G, K, _cus(torch)), f"{label}: average_parts {parts}, the restated formula {ap.parts_of(n, G, K, _cus(torch))}"
    if _cus(torch) == 256:
        assert parts == named_parts, (label, parts, named_parts)
    label += f" P={parts}"
    fg = ap.flat_case(n, layout, K, G, parts)
    m = fg.means(parts)
    assert ap.in_ranges(m).all()
    case = Case(torch, n, CF, G, K, layout, raw=fg.raw(n, layout))
    ps, _, _ = case.run(1e9, SPEC)
    p, h, t = case.run(1e9, BOTH)
    assert len(h) == 0 and not t.any()
    _one_float(p, label)
    assert ps.tobytes() == p.tobytes(), f"{label}: spectrum-only and spectrum + hits plans store identical spectra"
    v = p[:, 0].copy()
    part = _partners(torch, n, m, label)
    _same_bits(v, part, m, label)
    _check_map(m, v, label)
    n_ev = int(tol.evaluated_mask(n).sum())
    counts = []
    for thr in _thresholds(v):
        _, hh, _ = _decide(case, p, float(thr), f"{label} thr={thr!r}")
        counts.append(len(hh))
    on_T = int((v == _thresholds(v)[0]).sum())
    assert counts[2] - counts[0] == on_T * n_ev and counts[0] >= counts[1], f"{label}: the group on the threshold has no record at it and all of its own below it ({counts})"
    if G <= 5:   # every group's records, in both hit modes
        _, hh, _ = _decide(case, p, -300.0, f"{label} thr=-300")
        assert len(hh) == G * n_ev
    _FIG["parts"][(n, K, G)] = parts
    _classes(parts, G, layout, n, CF, multi_item)
    return _discriminating(part)


SMALL = [(n, layout, K, P) for n in ap.SIZES for layout in ap.LAYOUTS for K, P in ap.SMALL_SHAPES]


@pytest.mark.parametrize("n,layout,K,P", SMALL, ids=[f"{n}-{LAYOUT[layout]}-K{K}" for n, layout, K, P in SMALL])
def test_small_group_counts(torch_cuda, n, layout, K, P):
    """G = 1 and G = 5: the partial-sum route, P = (K + 1) // 2 parts added by scn_avg_combine_kernel"""
    disc = np.concatenate([_hold_flat(torch_cuda, n, layout, K, G, P) for G in ap.SMALL_G])
    _FIG["disc"][f"flat n={n} {LAYOUT[layout]} K={K} P={P}"] = (int(disc.sum()), len(disc))
    assert 2 * int(disc.sum()) >= len(disc), f"n={n} K={K}: {int(disc.sum())} of {len(disc)} groups are discriminating"


BIG = [(n, layout) for n in ap.SIZES for layout in ap.LAYOUTS]


def _grid(torch, n, G):
    """(items per workgroup, workgroups) of scn_launch_average with P = 1: workgroup w takes the groups w, w + grid, ..."""
    slots = _slots(torch, n)
    per = -(-G // slots)
    return per, -(-G // per)


@pytest.mark.parametrize("n,layout", BIG, ids=[f"{n}-{LAYOUT[layout]}" for n, layout in BIG])
def test_in_kernel_epilogue_over_two_items(torch_cuda, n, layout):
    """P = 1, K = 3, G = slots + 5: the power kernel's own epilogue, the accumulators reset by hand between a workgroup's two items"""
    G = _slots(torch_cuda, n) + 5
    per, grid = _grid(torch_cuda, n, G)
    assert per == 2 and grid < G <= 2 * grid
    if _cus(torch_cuda) == 256:
        assert G == ap.big_groups(n)
    disc = _hold_flat(torch_cuda, n, layout, ap.BIG_K, G, 1, multi_item=True)
    _FIG["disc"][f"flat n={n} {LAYOUT[layout]} K={ap.BIG_K} P=1 G={G}"] = (int(disc.sum()), len(disc))
    assert 2 * int(disc.sum()) >= len(disc)


# ---- pair groups: the division alone, in every wire format ---------------------------------------------------------------------
PAIRS = [(n, kind) for n in ap.SIZES for kind in KINDS]


@pytest.mark.parametrize("n,kind", PAIRS, ids=[f"{n}-{NAMES[k]}" for n, k in PAIRS])
def test_pair_groups(torch_cuda, n, kind):
    torch = torch_cuda
    shapes = [(K, 5, layout) for K in (3, 5, 7) for layout in ap.LAYOUTS]
    if n in (1024, 8192):
        shapes.append((3, _slots(torch, n) + 5, ap.AVG_DWELL))
    n_ev = int(tol.evaluated_mask(n).sum())
    for K, G, layout in shapes:
        pg = ap.pair_case(kind, n, K, G, 0)
        raw = pg.raw(n, layout)
        got = {}
        for dc in (0, 1):
            label = f"pair n={n} {NAMES[kind]} {LAYOUT[layout]} K={K} G={G} correct_dc={dc}"
            case = Case(torch, n, kind, G, K, layout, raw=raw, dc=dc, enob=ap.pair_enob(kind))
            parts = case.parts()
            m = pg.means(parts)
            ps, _, _ = case.run(1e9, SPEC)
            p, h, t = case.run(1e9, BOTH)
            assert len(h) == 0 and not t.any()
            _one_float(p, label, step=2)
            assert ps.tobytes() == p.tobytes(), f"{label}: spectrum-only and spectrum + hits plans store identical spectra"
            got[dc] = p
            if dc:
                assert p.tobytes() == got[0].tobytes(), f"{label}: an integer mean of 0 removed changes the bytes"
                continue
            for name, col in (("even", 0), ("odd", 1)):
                part = _partners(torch, n, m[name], f"{label} {name}")
                _same_bits(p[:, col], part, m[name], f"{label} {name} bins")
                _check_map(m[name], p[:, col], f"{label} {name}")
                if name == "even":
                    disc = _discriminating(part)
                    _FIG["disc"][f"pair n={n} {NAMES[kind]} {LAYOUT[layout]} K={K} P={parts} G={G}"] = (int(disc.sum()), len(disc))
                    assert 2 * int(disc.sum()) >= len(disc), f"{label}: {int(disc.sum())} of {len(disc)} groups are discriminating"
            _classes(parts, G, layout, n, kind, multi_item=G > 5)
        for dc in (0, 1):   # the decision on the even bins' value of one group, and every record once
            case = Case(torch, n, kind, G, K, layout, d_raw=case.d_raw, dc=dc, enob=ap.pair_enob(kind))
            for thr in _thresholds(got[0][:, 0]) + ((-300.0,) if G <= 5 else ()):
                _, hh, _ = _decide(case, got[0], float(thr), f"pair n={n} {NAMES[kind]} K={K} G={G} correct_dc={dc} thr={thr!r}")
            if G <= 5:
                assert len(hh) == G * n_ev


# ---- special values inside one group --------------------------------------------------------------------------------------------
SPECIAL_SHAPES = [(n, shape) for n in ap.SIZES for shape in ("multi-item", "split")]


def _poke(torch, case, d_base, rows):
    """a copy of the input with the amplitudes (sample 0) of the groups in rows {g: complex64 [K]} replaced"""
    y = d_base.clone()
    mb = ap.member_buffers(case.G, case.K, case.layout)
    for g, row in rows.items():
        idx = torch.from_numpy(2 * mb[g] * case.n).cuda()
        y[idx] = torch.from_numpy(np.ascontiguousarray(row.real.astype(F32))).cuda()
        y[idx + 1] = torch.from_numpy(np.ascontiguousarray(row.imag.astype(F32))).cuda()
    return y


@pytest.mark.parametrize("n,shape", SPECIAL_SHAPES, ids=[f"{n}-{s}" for n, s in SPECIAL_SHAPES])
def test_special_values(torch_cuda, n, shape):
    torch = torch_cuda
    layout = ap.LAYOUTS[(n.bit_length() + (shape == "split")) % 2]
    n_ev = int(tol.evaluated_mask(n).sum())
    if shape == "multi-item":
        K, G = ap.BIG_K, _slots(torch, n) + 5
        per, grid = _grid(torch, n, G)
        assert per == 2 and 7 + grid < G
        targets = (7, 7 + grid)           # the first item of workgroup 7, which goes on to a second item, and that second item
    else:
        K, G, targets = 7, 5, (2, 4)
    label = f"special n={n} {LAYOUT[layout]} K={K} G={G}"
    parts = Case(torch, n, CF, G, K, layout, d_raw=0).parts()
    if _cus(torch) == 256:
        assert parts == (1 if shape == "multi-item" else 4)
    fg = ap.flat_case(n, layout, K, G, parts)
    case = Case(torch, n, CF, G, K, layout, raw=fg.raw(n, layout))
    d_base = case.d_raw.view(torch.float32)
    p0, _, _ = case.run(1e9, BOTH)
    thr = float(_thresholds(p0[:, 0])[2])           # just under one group's value: that group and those above it have records
    cap = len(_expected(p0, n, thr)[0]) + 2 * n_ev + 1024
    members = sorted({0, K // 2, K - 1})
    bounds = ap.part_bounds(K, parts)
    if parts > 1:
        assert bounds[0][0] <= members[0] < bounds[0][1] and bounds[-1][0] <= members[-1] < bounds[-1][1], "the first and the last part"
    with case.plan(thr, BOTH, cap) as plan_both, case.plan(thr, HITS, cap) as plan_hits:
        plans = (plan_both, plan_hits)
        p0b, h0, t0 = _decide(case, p0, thr, f"{label} baseline", plans)
        assert len(h0) >= n_ev and t0.any() and not t0.all()
        g0 = np.searchsorted(case.seq, h0["seq_id"])
        assert np.array_equal(case.seq[g0], h0["seq_id"])
        for name in ap.SPECIALS:
            for g in targets:
                for k in (members if name not in ("zero", "overflow") else members[:1]):
                    what = f"{label} P={parts}: {name} at member {k} of group {g}"
                    row = ap.special_row(fg.amps[g], name, k)
                    y = _poke(torch, case, d_base, {g: row})
                    p, h, t = _decide(case, None, thr, what, plans, d_raw=y)
                    keep = np.arange(G) != g
                    assert p[keep].tobytes() == p0[keep].tobytes(), f"{what}: another group's spectrum changed"
                    gh = np.searchsorted(case.seq, h["seq_id"])
                    assert h[gh != g].tobytes() == h0[g0 != g].tobytes(), f"{what}: another group's records changed"
                    assert np.array_equal(t[keep], t0[keep]), f"{what}: another group's trigger changed"
                    bits, cnt = p[g].view(np.uint32), int((gh == g).sum())
                    mean = ap.mean_float(ap.powers(row)[None, :], K, parts)[0]
                    if name in ("nan_re", "nan_im"):
                        assert np.isnan(mean) and np.isnan(p[g]).all() and cnt == 0 and not t[g], \
                            f"{what}: the whole group is NaN, without record or trigger ({int(np.isnan(p[g]).sum())} bins are, {cnt} records)"
                    elif name in ("big", "overflow"):
                        assert np.isposinf(mean) and (bits == POS_INF).all() and cnt == n_ev and t[g], \
                            f"{what}: +inf in every bin, one record per evaluated bin, trigger ({int((bits == POS_INF).sum())} bins are, {cnt} records)"
                        assert (h[gh == g]["power_db"].view(np.uint32) == POS_INF).all()
                    elif name in ("zero", "den_mean"):
                        assert 0 <= mean < np.finfo(F32).tiny and (bits == NEG_INF).all() and cnt == 0 and not t[g], \
                            f"{what}: a mean below FLT_MIN maps to -inf and forms no record ({int((bits == NEG_INF).sum())} bins are, {cnt} records)"
                    else:
                        assert mean >= np.finfo(F32).tiny
                        _one_float(p[g:g + 1], what)
                        part = _partners(torch, n, [mean], what)
                        _same_bits(p[g:g + 1, 0], part, np.array([mean], F32), what + " (the IEEE model with denormals kept)")
                        assert cnt == 0 and not t[g]
    # no record at ANY threshold for a mean below FLT_MIN, -inf included: a launch of zero groups, denormal-mean groups (at both
    # items of a workgroup) and five ordinary groups, whose records are all there are
    rows = {g: np.zeros(K, np.complex64) for g in range(G)}
    ordinary = [1, 3] if shape == "split" else [1, 2, 3, targets[1] + 1, targets[1] + 2]
    for g in ordinary:
        rows[g] = fg.amps[g].astype(np.complex64)
    for j, g in enumerate(targets):
        rows[g] = ap.special_row(fg.amps[g], "den_mean", members[j % len(members)])
    amps = np.stack([rows[g] for g in range(G)])
    low = Case(torch, n, CF, G, K, layout, raw=ap.FlatGroups(G, K, amps=amps).raw(n, layout))
    for t_low in (-np.inf, -250.0):
        p, h, t = _low(low, t_low, len(ordinary) * n_ev + 1024)
        _check_hits(low, p, h, t, t_low, f"{label} thr={t_low}")
        assert len(h) == len(ordinary) * n_ev, f"{label} thr={t_low}: {len(h)} records, the ordinary groups owe {len(ordinary) * n_ev}"
        quiet = np.ones(G, bool)
        quiet[ordinary] = False
        assert (p[quiet].view(np.uint32) == NEG_INF).all() and not t[quiet].any() and t[ordinary].all()
        assert p[ordinary].tobytes() == p0[ordinary].tobytes(), f"{label} thr={t_low}: an ordinary group among zero groups reports other bits"
    _classes(parts, G, layout, n, CF, shape == "multi-item")


def _low(case, thr, cap):
    """spectrum + hits and hits-only at a threshold every finite value exceeds; the hits-only bytes are asserted equal"""
    p, h, t = case.run(thr, BOTH, cap)
    _, hh, th = case.run(thr, HITS, cap)
    assert hh.tobytes() == h.tobytes() and np.array_equal(th, t), f"thr={thr}: hits-only differs from spectrum + hits"
    return p, h, t


# ---- figures --------------------------------------------------------------------------------------------------------------------
def test_zz_figures(request, torch_cuda):
    """prints what the module measured; where the whole module ran in this process (no -k, no deselection by node id, no xdist
    worker), asserts that every coverage class was met"""
    mine = [i for i in request.session.items if i.fspath.basename == "test_average_exact_gpu.py"]
    whole = not request.config.option.keyword and not hasattr(request.config, "workerinput") and len(mine) >= len(SMALL) + len(BIG) + len(PAIRS) + len(SPECIAL_SHAPES) + 1
    by_shape = {}
    for (n, K, G), parts in sorted(_FIG["parts"].items()):
        by_shape.setdefault((K, "slots + 5" if G > 5 else G), {})[n] = parts
    print(f"device: {_cus(torch_cuda)} CUs; P per shape (K, G) by size: " + "; ".join(f"K={K} G={G}: {v}" for (K, G), v in by_shape.items()))
    for name, (d, c) in _FIG["disc"].items():
        print(f"discriminating: {name}: {d} of {c}")
    tot = [sum(v[i] for v in _FIG["disc"].values()) for i in (0, 1)]
    low = min(_FIG["disc"].items(), key=lambda kv: kv[1][0] / kv[1][1]) if _FIG["disc"] else None
    print(f"discriminating groups in all: {tot[0]} of {tot[1]}; lowest share: {low}")
    print(f"worst map deviation: {_FIG['map'][0]:.3f} ulp of the value at mean = {_FIG['map'][1]!r} [{_FIG['map'][2]}]")
    print(f"worst map deviation in dB: {_FIG['map_abs'][0]:.3e} dB at mean = {_FIG['map_abs'][1]!r} [{_FIG['map_abs'][2]}]")
    print(f"worst map deviation against tolerances.db_map_bound_of_power: {_FIG['map_rel'][0]:.3f} of the bound at mean = {_FIG['map_rel'][1]!r} [{_FIG['map_rel'][2]}]")
    print(f"{_LAUNCH[0]} launches, {len(mine)} tests, {time.time() - _T0:.1f} s since the module was imported")
    if whole and mine[-1].name == "test_zz_figures":
        want = {"P=1 multi-item", "P=2", "2<P<=16", "16<P<49", "P>=49"} | {("layout", v) for v in ap.LAYOUTS} | {("n", n) for n in ap.SIZES} | {("kind", k) for k in KINDS}
        if _cus(torch_cuda) == 256:
            assert want <= _FIG["classes"], f"coverage classes not met: {want - _FIG['classes']}"
        assert _FIG["map_rel"][1] is not None and _FIG["map_rel"][0] <= 1.0
