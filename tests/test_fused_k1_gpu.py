"""Every kernel family's OWN sample conversion (K1), bit for bit.

scn_convert_kernel (Plan.convert_raw) is the one K1 pinned to the reference's utility.cpp:9-84 (tests/test_oracle_ref_dsp.py), but no
transform runs it.  A sample's decode is stated once (Wire<KIND>, scanner_amd/csrc/scn_wire.h, held on a CPU by tests/cpp/test_wire.cpp),
but each family still fetches its samples its own way (RawLoader, BigRaw, WelchRaw: planar addressing, lane pairs) and carries its own
integer DC sums, its own `int32 /= uint32` division (search `dc_re = (int)((uint32_t)` in scanner_amd/csrc) and its own fold of
onebymax into the window tap.  Each of them forms
conv(raw, dc, 1.0f) * (w[i] * scale) with scale = +-2^-k, so an integer-kind plan A on the raw bytes and a FLOAT_COMPLEX plan B of the
same size, window, mask, threshold and flags on A.convert_raw(raw) multiply the same two real numbers in every lane
(tests/test_fused_k1_cpu.py proves the fold exact, contracted into an FMA or not), and everything behind that product is the same
template.  So here, with no tolerance, guard band or picked threshold:

  * A.convert_raw(raw) equals the oracle's convert bit for bit (B's input is the pinned one);
  * the spectra of A and B are equal as bit patterns (-inf included), in spectrum-only and spectrum + hits plans;
  * the hit records are byte-equal in spectrum + hits and hits-only plans, at a threshold that is simply the launch's median dB value;
  * the trigger flags are equal, with trigger_count between the launch's smallest and largest count so that both values occur;
  * time-domain plans: max, min and flags equal; Welch plans: PSDs equal, B on oracle.welch_convert of the same stream.

A slip in any family's K1 -- a mean off by one count, a sign extension wrong at full scale, a Q-plane offset wrong in a partly filled
workgroup, the negative-sum quirk applied to I and not to Q -- changes a sample by at least one count and fails the family outright.

INPUTS corner K1, not the transform.  Every launch holds (corner_batch): uniform samples over the type's full range with its minimum
and maximum present; a constant buffer at the minimum and one at the maximum; buffers whose I sum is exactly -1, 0, n - 1, n, n + 1 and
-n (the 0 / 1 boundary of the mean, and the first sums the quirk turns into 2^32 / n); a buffer with a negative I sum and a positive Q
sum and the converse; I and Q of visibly different content throughout (Q is a sawtooth where I is noise, or carries another offset).
61 buffers per launch -- a prime, so that wherever a workgroup holds several buffers (256 ... 8 of them from 16 to 512 points) the last
one's slots stay partly empty -- 29 from 32768 points up (fewer than the column kernel's G = 3 CUs / (n / 4096) workgroup
rows: no workgroup takes a second buffer there; tests/test_launch_shape_gpu.py runs that loop).  Two more launches at 4096 and
8192 points in int16 hold 61 buffers more than the launch has workgroups (scn_kernels.hip launch_kernel: grid = CUs x WG_PER_CU, 3
for Geo<16> and 2 for Geo8k), so that workgroups take further buffers from the queue (scn_uses_queue).

ENOB cycles over the cases: 8 for int8 (the only value its reference path knows: the wrapping, negative scale); 12, 14, 16 and 1 for
the int16 kinds.  16 and 1 are the extremes with a finite scale: the plan accepts up to 32, but from 17 up max wraps to 0 and the scale
is 1 / 0 (tests/test_fused_k1_cpu.py).

EXEMPTIONS: none.  The issue that asked for this module allowed a family to be exempt where the dispatch instantiates another template
or butterfly order for the integer kinds, and named a "wide 8192-point integer form".  No such form exists: scn_launch_fft
(scn_kernels.hip, unit 5 of its table) sends every wire format to Family8k, i.e. scn_fft8k_kernel<KIND, DC, HITS, SPEC>, whose body differs by
KIND only in RawLoader<KIND>::load2, Wire<KIND>::ints / conv and in where the next buffer comes from (DYN); likewise every other family.  EXEMPT
stays as the place to name one, with file and line, should a compiler ever contract the two instantiations differently; an exempt
case is then not skipped but held against float64 (the module fails where EXEMPT is not empty and that path is not written), and the
module fails above MAX_EXEMPT_SHARE.

MODULE STATE: test_zz_summary prints what ran, per family and wire format (run with -s); profiles/fused_k1.txt is that table."""
import numpy as np
import pytest

from scanner_amd import Plan, WelchPlan, build, capi
from tests import tolerances as tol

pytestmark = pytest.mark.gpu
FS = 8000000
SEQ0 = 1 << 33
SPEC, BOTH, HITS = capi.OUT_SPECTRUM, capi.OUT_SPECTRUM | capi.OUT_HITS, capi.OUT_HITS
CF, I16, I16P, I8 = capi.KIND_FLOAT_COMPLEX, capi.KIND_SHORT_COMPLEX, capi.KIND_SHORT, capi.KIND_BYTE_COMPLEX
NAMES = {I16: "int16", I16P: "int16planar", I8: "int8"}
ENOB16 = (12, 14, 16, 1)
MAX_EXEMPT_SHARE = 0.10
EXEMPT = {}    # (family, kind) -> "file:line: cause"

build.build()  # (collection needs scn_size_path; seconds when the library is current, and it needs no GPU)
POW2 = [1 << k for k in range(4, 15) if capi.size_path(1 << k) == capi.PATH_FUSED]
MIXED = [n for n in range(17, 16384) if n & (n - 1) and capi.size_path(n) == capi.PATH_FUSED]
FOUR_STEP = [32768, 65536]
BLUESTEIN = [17, 1004, 1023, 4097]


def _cases(sizes_kinds):
    """(n, kind, enob, dc) with the ENOB cycling over the int16 cases: the k-th int16 case of the s-th size takes entry s + k, so that
    every kind and DC setting meets every ENOB as the sizes go by"""
    out, sizes, k16 = [], [], 0
    for n, kind, dc in sizes_kinds:
        if n not in sizes:
            sizes.append(n)
            k16 = 0
        if kind == I8:
            out.append((n, kind, 8, dc))
        else:
            out.append((n, kind, ENOB16[(len(sizes) - 1 + k16) % len(ENOB16)], dc))
            k16 += 1
    return out


def _id(n, kind, enob, dc):
    return f"{n}-{NAMES[kind]}-enob{enob}{'-dc' if dc else ''}"


CASES = _cases([(n, k, dc) for n in POW2 + MIXED + FOUR_STEP + BLUESTEIN for k in (I16, I16P, I8) for dc in (False, True)])
QUEUE = [(4096, I16, 12, True, 3), (8192, I16, 16, True, 2)]   # (..., WG_PER_CU of the size's geometry)
AVG = [(n, k, lay) for n in (1024, 2048, 4096, 8192) for k in (2, 16) for lay in (capi.AVG_DWELL, capi.AVG_SWEEPS)]
TD = _cases([(n, k, dc) for n in (8192, 1004) for k in (I16, I16P, I8) for dc in (False, True)])
WELCH = _cases([(65536, k, dc) for k in (I16, I16P, I8) for dc in (False, True)])

_DONE = {}   # (family, wire format) -> [launches, buffers, records compared]


def family(n):
    if n in BLUESTEIN:
        return "bluestein"
    if n in FOUR_STEP:
        return "four-step"
    if n in MIXED:
        return "mixed >= 10240" if n >= 10240 else "mixed < 10240"
    return "16 ... 128" if n <= 128 else "256, 512" if n <= 512 else "1024 ... 4096" if n <= 4096 else str(n)


def _note(fam, kind, dc, buffers, records):
    row = _DONE.setdefault((fam, NAMES[kind] + ("/dc" if dc else "")), [0, 0, 0])
    row[0] += 1
    row[1] += buffers
    row[2] += records


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(raw):
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need a GPU; refusing to skip silently"
    return torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).reshape(-1)).cuda()


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def _with_sum(rng, n, target, spread):
    """n integers within +-(2 * spread + 2) whose sum is exactly `target` (|target| <= (spread + 1) n): noise, shifted, a few raised by one"""
    v = rng.integers(-spread, spread + 1, n).astype(np.int64)
    q, r = divmod(int(target) - int(v.sum()), n)
    v += q
    v[:r] += 1
    assert v.sum() == target
    return v


def corner_batch(n, kind, nb, seed):
    """[nb, n, 2] int64 (I, Q) of the launch described in the module docstring, and the list of what each buffer is"""
    dt = np.int8 if kind == I8 else np.int16
    lo, hi = int(np.iinfo(dt).min), int(np.iinfo(dt).max)
    rng = np.random.default_rng(seed)
    saw = ((np.arange(n) * 37) % 251 - 125) * (1 if kind == I8 else 200)   # a sawtooth within the type's range
    x = np.empty((nb, n, 2), np.int64)
    what = []
    for b in range(nb):
        x[b, :, 0] = rng.integers(lo, hi + 1, n)
        x[b, :, 1] = saw if b % 2 else rng.integers(lo, hi + 1, n)
        what.append("uniform")
    x[0, :2, 0], x[0, :2, 1] = (lo, hi), (hi, lo)
    x[1], x[2] = lo, hi
    what[1], what[2] = "const min", "const max"
    for b, s in zip(range(3, 9), (-1, 0, n - 1, n, n + 1, -n)):
        x[b, :, 0] = _with_sum(rng, n, s, 50)
        x[b, :, 1] = _with_sum(rng, n, (7 * n + 3) * (1 if b % 2 else -1), 40)   # Q: a mean of +-7 and a bit, the sign alternating
        what[b] = f"I sum {s}"
    x[9, :, 0], x[9, :, 1] = _with_sum(rng, n, -20 * n - 5, 50), _with_sum(rng, n, 20 * n + 5, 50)
    x[10, :, 0], x[10, :, 1] = _with_sum(rng, n, 20 * n + 5, 50), _with_sum(rng, n, -20 * n - 5, 50)
    what[9], what[10] = "I sum < 0 < Q sum", "Q sum < 0 < I sum"
    assert x.min() == lo and x.max() == hi and x[0].min() == lo and x[0].max() == hi
    for b in range(3, 11):
        assert np.abs(x[b]).max() <= 104
    assert (x[9].sum(axis=0) * (-1, 1) > 0).all() and (x[10].sum(axis=0) * (1, -1) > 0).all()
    assert not any(np.array_equal(x[b, :, 0], x[b, :, 1]) for b in range(nb) if b not in (1, 2))
    return x, what


def to_wire(x, kind):
    """[nb, n, 2] integers -> the kind's wire format: int16 / int8 [nb, n, 2] interleaved, int16 [nb, 2, n] planar"""
    if kind == I8:
        return np.ascontiguousarray(x.astype(np.int8))
    if kind == I16:
        return np.ascontiguousarray(x.astype(np.int16))
    return np.ascontiguousarray(x.astype(np.int16).transpose(0, 2, 1))


def _pinned_convert(oracle_mod, plan, n, kind, enob, dc, raw):
    """plan.convert_raw(raw), asserted equal to the oracle's converter buffer by buffer, bit for bit"""
    conv = plan.convert_raw(raw)
    o = oracle_mod.Oracle(n, kind=kind, enob=enob, correct_dc=dc)
    ref = np.stack([o.convert(r) for r in raw])
    assert np.array_equal(_bits(conv.view(np.float32)), _bits(ref.view(np.float32))), "scn_convert_raw differs from the oracle's converter"
    assert np.isfinite(conv.view(np.float32)).all()
    return conv


# ---- one A / B pair ------------------------------------------------------------------------------------------------------------
def _pair(n, kind, enob, dc, raw, conv, what, copies=1, layout=capi.AVG_DWELL):
    """spectrum-only, spectrum + hits and hits-only plans of the integer kind on `raw` and of FLOAT_COMPLEX on `conv`: everything
    they report must be identical.  Returns the number of records compared."""
    sweeps = layout == capi.AVG_SWEEPS
    nb = len(raw)
    G = nb // copies
    fc_g = 70e6 + 6e6 * np.arange(G)
    fc = np.tile(fc_g, copies) if sweeps else np.repeat(fc_g, copies)
    seq = np.arange(nb, dtype=np.uint64) + np.uint64(SEQ0)
    d = {"A": _dev(raw), "B": _dev(conv)}
    desc = {"A": dict(kind=kind, enob=enob, correct_dc=dc), "B": dict(kind=CF)}
    common = dict(max_batch=nb, average=copies, average_layout=layout)

    def run(which, flags, thr, **kw):
        with Plan(n, FS, thr, flags=flags, **common, **desc[which], **kw) as plan:
            plan.submit_device(0, d[which], nb, fc, seq)
            return plan.collect(0)

    pA, pB = run("A", SPEC, 1e9)[0], run("B", SPEC, 1e9)[0]
    assert pA.shape == (G, n)
    assert not np.isnan(pA).any() and not (pA == np.inf).any()
    diff = _bits(pA) != _bits(pB)
    assert not diff.any(), (f"{what}: {int(diff.sum())} bins differ between the integer plan and the cfloat plan on its converted samples; "
                            f"first (buffer, bin): {np.argwhere(diff)[:4].tolist()}, {pA[diff][:4]} vs {pB[diff][:4]}")
    # the threshold: the launch's median dB value, as the float a plan takes -- no guard band; the counts the spectrum implies
    thr = float(np.float32(np.median(pA[np.isfinite(pA)])))
    counts = (pA[:, tol.evaluated_mask(n)] > np.float32(thr)).sum(axis=1)
    levels = np.unique(counts)
    assert len(levels) >= 2, f"{what}: every buffer has {levels} hits"
    trig = int(max(1, levels[(len(levels) - 1) // 2]))   # (0 means "the reference's 1047" to a plan)
    cap = int(counts.sum()) + 1024
    got = {(w, fl): run(w, fl, thr, max_hits=cap, trigger_count=trig) for w in "AB" for fl in (BOTH, HITS)}
    (p2A, hA, tA), (p2B, hB, tB) = got[("A", BOTH)], got[("B", BOTH)]
    assert np.array_equal(_bits(p2A), _bits(pA)) and np.array_equal(_bits(p2B), _bits(pA)), f"{what}: spectrum + hits plans store other spectra"
    assert len(hA) == counts.sum() and np.array_equal(np.bincount((hA["seq_id"] - seq[0]).astype(np.int64) // (1 if sweeps else copies), minlength=G), counts)
    assert len(hA) == len(hB) and hA.tobytes() == hB.tobytes(), f"{what}: spectrum + hits records differ"
    assert np.array_equal(tA, tB) and np.array_equal(tA, (counts > trig).astype(np.uint8)), f"{what}: trigger flags"
    assert tA.any() and not tA.all(), f"{what}: trigger_count {trig} leaves one flag value unused"
    (_, hhA, thA), (_, hhB, thB) = got[("A", HITS)], got[("B", HITS)]
    assert hhA.tobytes() == hhB.tobytes() and hhA.tobytes() == hA.tobytes(), f"{what}: hits-only records differ"
    assert np.array_equal(thA, tA) and np.array_equal(thB, tA)
    return len(hA)


def _exempt_check():
    assert not EXEMPT, "an exempt family must be held against float64 (tol.compare_spectra, tol.floor_errors, 2 Y): not written, none is exempt"


@pytest.mark.parametrize("n,kind,enob,dc", CASES, ids=[_id(*c) for c in CASES])
def test_k1_of_every_family(built_lib, oracle_mod, n, kind, enob, dc):
    _exempt_check()
    nb = 61 if n <= 16384 else 29
    x, _ = corner_batch(n, kind, nb, seed=n + 7 * kind + dc)
    raw = to_wire(x, kind)
    with Plan(n, FS, 1e9, kind=kind, enob=enob, correct_dc=dc, max_batch=nb, flags=SPEC) as plan:
        conv = _pinned_convert(oracle_mod, plan, n, kind, enob, dc, raw)
    _note(family(n), kind, dc, nb, _pair(n, kind, enob, dc, raw, conv, _id(n, kind, enob, dc)))


@pytest.mark.parametrize("n,kind,enob,dc,wg_per_cu", QUEUE, ids=[_id(*c[:4]) + "-queue" for c in QUEUE])
def test_k1_through_the_buffer_queue(built_lib, oracle_mod, n, kind, enob, dc, wg_per_cu):
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need a GPU; refusing to skip silently"
    grid = torch.cuda.get_device_properties(0).multi_processor_count * wg_per_cu
    x, _ = corner_batch(n, kind, 61, seed=n)
    nb = grid + 61                                       # every workgroup one buffer, 61 of them a second one from the queue
    raw = to_wire(x, kind)[np.arange(nb) % 61]
    with Plan(n, FS, 1e9, kind=kind, enob=enob, correct_dc=dc, max_batch=nb, flags=SPEC) as plan:
        conv = _pinned_convert(oracle_mod, plan, n, kind, enob, dc, raw[:61])[np.arange(nb) % 61]
    _note(family(n) + " queue", kind, dc, nb, _pair(n, kind, enob, dc, raw, np.ascontiguousarray(conv), f"{n} queue"))


@pytest.mark.parametrize("n,k,layout", AVG, ids=[f"{n}-K{k}-{'sweeps' if lay == capi.AVG_SWEEPS else 'dwell'}" for n, k, lay in AVG])
def test_k1_of_averaged_plans(built_lib, oracle_mod, n, k, layout):
    _exempt_check()
    idx = AVG.index((n, k, layout))
    kind, dc = (I16, I16P, I8)[idx % 3], bool((idx // 3) % 2)     # 16 cases over the six (kind, DC) pairs
    enob = 8 if kind == I8 else ENOB16[idx % 4]
    G = 13 if k == 2 else 3
    nb = G * k
    x, _ = corner_batch(n, kind, nb, seed=n + k)
    if k == 16:
        x = x[(np.arange(nb) * 5) % nb]    # (5 and 48 are coprime: the corner buffers spread over the three groups)
    raw = to_wire(x, kind)
    with Plan(n, FS, 1e9, kind=kind, enob=enob, correct_dc=dc, max_batch=nb, flags=SPEC, average=k, average_layout=layout) as plan:
        conv = _pinned_convert(oracle_mod, plan, n, kind, enob, dc, raw)
        parts = plan.average_parts(nb)
    assert (parts > 1) == (k == 16), f"K = {k}, {G} groups: {parts} workgroups per group"
    _note(f"averaged {n}", kind, dc, nb, _pair(n, kind, enob, dc, raw, conv, f"{n} K={k} {_id(n, kind, enob, dc)}", copies=k, layout=layout))


@pytest.mark.parametrize("n,kind,enob,dc", TD, ids=[_id(*c) for c in TD])
def test_k1_of_time_domain_plans(built_lib, oracle_mod, n, kind, enob, dc):
    """8192: the streaming form (one wave per buffer, n % 8 == 0); 1004: the per-sample form (scn_launch_time_domain)"""
    nb = 61
    x, _ = corner_batch(n, kind, nb, seed=n + kind)
    raw = to_wire(x, kind)
    with Plan(n, FS, 1e9, kind=kind, enob=enob, correct_dc=dc, max_batch=nb, flags=SPEC) as plan:
        conv = _pinned_convert(oracle_mod, plan, n, kind, enob, dc, raw)
    d = {"A": _dev(raw), "B": _dev(conv)}
    desc = {"A": dict(kind=kind, enob=enob, correct_dc=dc), "B": dict(kind=CF)}

    def run(which, thr):
        with Plan(n, FS, thr, mode=capi.MODE_TIME_DOMAIN, max_batch=nb, **desc[which]) as plan:
            plan.submit_device(0, d[which], nb)
            return plan.collect_time_domain(0)

    mx, _, _ = run("A", 0.0)
    levels = np.unique(mx)     # (the reference clamps a buffer's maximum at the smallest positive float, process.cpp:207: ties)
    assert len(levels) >= 2
    thr = float(levels[max(1, len(levels) // 2)])    # `max >= threshold` (process.cpp:226) then holds for some buffers, not for all
    (mxA, mnA, abA), (mxB, mnB, abB) = run("A", thr), run("B", thr)
    assert np.array_equal(_bits(mxA), _bits(mx)) and np.array_equal(_bits(mxA), _bits(mxB)), "max"
    assert np.array_equal(_bits(mnA), _bits(mnB)), "min"
    assert np.array_equal(abA, abB) and abA.any() and not abA.all(), "flags"
    _note("time domain " + ("streaming" if n % 8 == 0 else "per sample"), kind, dc, nb, 0)


@pytest.mark.parametrize("n,kind,enob,dc", WELCH, ids=[_id(*c) for c in WELCH])
def test_k1_of_welch_plans(built_lib, oracle_mod, n, kind, enob, dc):
    K, n_psd, hop = 2, 2, n // 2
    blocks = n_psd * K + 1
    x, what = corner_batch(hop, kind, 11, seed=kind + dc)
    x = x[[0, 3, 9, 10, 6][:blocks]]                      # uniform; I sum -1; I < 0 < Q; Q < 0 < I; I sum n: one delivery block each
    raw = to_wire(x, kind)
    conv = oracle_mod.welch_convert(raw, kind, enob, dc, hop)
    psd = {}
    for which, data, desc in (("A", raw, dict(kind=kind, enob=enob, correct_dc=dc)), ("B", conv, dict(kind=CF))):
        with WelchPlan(n, K, max_psd=n_psd, **desc) as wp:
            flat = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            assert flat.size == wp.samples(n_psd) * wp.bytes_per_sample
            wp.submit_device(0, _dev(flat), n_psd)
            psd[which] = wp.collect(0)
    assert not np.isnan(psd["A"]).any()
    diff = _bits(psd["A"]) != _bits(psd["B"])
    assert not diff.any(), f"{int(diff.sum())} bins differ; first (psd, bin): {np.argwhere(diff)[:4].tolist()}"
    _note("welch", kind, dc, blocks, 0)


def test_zz_summary():
    """what the module compared, per family and wire format (run with -s); the exempt share"""
    total = len(CASES) + len(QUEUE) + len(AVG) + len(TD) + len(WELCH)
    assert len(EXEMPT) / total <= MAX_EXEMPT_SHARE
    print(f"build {build.source_hash()}: K1 of every family, integer plan against cfloat plan on scn_convert_raw's output; {total} cases, {len(EXEMPT)} exempt")
    print(f"{'family':<26}{'wire format':<18}{'launch pairs':>12}  {'buffers':>8}  {'records':>9}  result")
    for (fam, wire), (launches, buffers, records) in _DONE.items():
        print(f"{fam:<26}{wire:<18}{launches:>12}  {buffers:>8}  {records:>9}  bit-identical")
