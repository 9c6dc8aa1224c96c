"""What the Bluestein path (scanner_amd/csrc/scn_generic.hip) is held to, stated once for tests/test_bluestein_cases_cpu.py (which
proves on the CPU that the bar sees the faults it is for) and tests/test_bluestein_gpu.py (which holds the kernels to it).

The path serves every size from 17 to 65535 that is neither a power of two nor a mixed-radix size, and promises: "everything between
the windowed input and the final spectrum is DOUBLE ... the spectrum is rounded to float once, in the finish kernel".  The bars the
rest of the suite applies to it (1e-5 of max(bin, mean) on power; twice a float32 pocketfft on the floor) are float yardsticks: a
float work buffer, a chirp or filter table rounded to float, or a fast-math sincos in a table costs about 1e-7 of the rms level per
bin and passes both.  allowance_db is the bar the promise itself implies, derived below and not measured.

SIZES.  The convolution length is m = 2^L, the power of two >= 2 n - 1; the launcher picks its radix-2 / 4 / 16 stage sequence and
the ping-pong parity from L.  For every L in 6 ... 17 the smallest and the largest n of that length, 2^(L-2) + 1 and 2^(L-1) - 1
(all odd; 8191 is prime), and seven even sizes (40000 is 5-smooth but above the mixed-radix range).
"""
import numpy as np

from tests import dr_scenes as sc
from tests import tolerances as tol

L_RANGE = range(6, 18)
EDGE_SIZES = [n for L in L_RANGE for n in ((1 << (L - 2)) + 1, (1 << (L - 1)) - 1)]
EVEN_SIZES = [18, 30, 1002, 11000, 20000, 40000, 65534]
SIZES = EDGE_SIZES + EVEN_SIZES

WIRE_SIZES = [33, 257, 8193, 11000]   # n < 256 threads; one thread with two samples; odd and large; even
MODE_SIZES = [31, 1025, 20000]
POSITION_SIZES = [65, 4095, 16385]
SPECIAL_SIZES = [17, 1023, 4098]
FAULT_SIZES = [17, 257, 1025, 8191, 40000, 65535]

# power_db (scn_device.h, `power_of`: __builtin_fmaf(x.y, x.y, x.x * x.x)) behind the finish kernel's two casts (scn_generic.hip,
# `power_db(cf{(float)X.x, (float)X.y})`): the cast of X.x, the cast of X.y, the product x.x * x.x, the fused multiply-add.  Each
# cast moves its component by 2^-24 relative, hence its square by 2 * 2^-24, and the two squares are weights of the sum: together
# at most 2 * 2^-24 of the power; the product and the fma add 2^-24 each.  k = 4 roundings of 2^-24 of the POWER.
POWER_ROUNDINGS = 4
CHAIN_EPS = 2.0 ** -40          # term (3), of the buffer's rms level in amplitude
EXCLUDE_BELOW = 2.0 ** -20      # term (4), of the buffer's rms level in amplitude
MAX_EXCLUDED_SHARE = 1e-3
FLOOR_BOUND = CHAIN_EPS + 2.0 ** -24   # floor_errors' figure (of the rms level): the chain's own error plus one float rounding


def check_sizes(verbose=True):
    """every entry runs the Bluestein path, says the library; all twelve transform lengths are there, each at its smallest and its
    largest n; prints each size's stage sequence"""
    from scanner_amd import capi
    from tests import launch_caps as caps

    assert len(set(SIZES)) == len(SIZES) == 31
    by_len = {}
    for n in SIZES:
        assert capi.size_path(n) == capi.PATH_BLUESTEIN, n
        m = caps.bluestein_m(n)
        L = m.bit_length() - 1
        by_len.setdefault(L, []).append(n)
        r = caps.bluestein_radices(n)
        assert int(np.prod(r)) == m
        if verbose:
            print(f"n = {n:>5}: m = 2^{L:<2} stages {r} ({len(r) % 2 and 'odd' or 'even'} number of passes)")
    assert sorted(by_len) == list(L_RANGE), sorted(by_len)
    for L in L_RANGE:
        assert min(by_len[L]) == (1 << (L - 2)) + 1 and max(by_len[L]) == (1 << (L - 1)) - 1, (L, by_len[L])
    return by_len


def wire_cases():
    """(n, kind, enob, dc) of every launch of the GPU module's size and wire-format tests: SIZES in cfloat, WIRE_SIZES in int16
    interleaved at ENOB 12 and 16, int16 planar at 14 and int8 at 8, DC removal off and on"""
    from scanner_amd import capi

    out = [(n, capi.KIND_FLOAT_COMPLEX, 12, False) for n in SIZES]
    for n in WIRE_SIZES:
        out += [(n, k, e, dc) for k, e in ((capi.KIND_SHORT_COMPLEX, 12), (capi.KIND_SHORT_COMPLEX, 16), (capi.KIND_SHORT, 14),
                                           (capi.KIND_BYTE_COMPLEX, 8)) for dc in (False, True)]
    return out


def wire_id(n, kind, enob, dc):
    from scanner_amd import capi

    name = {capi.KIND_FLOAT_COMPLEX: "cfloat", capi.KIND_SHORT_COMPLEX: "int16", capi.KIND_SHORT: "int16planar", capi.KIND_BYTE_COMPLEX: "int8"}[kind]
    return f"{n}-{name}" + ("" if kind == capi.KIND_FLOAT_COMPLEX else f"-enob{enob}") + ("-dc" if dc else "")


def count(n):
    """buffers per launch: about 2^16 samples, and five more so that the batch is ragged"""
    return max(3, 65536 // n) + 5


# ---- the reference --------------------------------------------------------------------------------------------------------------
def owed(conv, window):
    """(a64, dB64) float64 [B, n]: what the float64 spectrum owes -- numpy's complex128 FFT of the FLOAT32 product x * w
    (dr_scenes.windowed: the reference's one defined rounding stays out of the error), as dr_scenes.ref64_power forms it; conv is
    the wire buffers through the oracle's bit-pinned converter (dr_scenes.convert), window is plan.window().  dB is the project's:
    10 log10 of the amplitude."""
    a64 = np.sqrt(sc.ref64_power(conv, window))
    with np.errstate(divide="ignore"):
        return a64, 10.0 * np.log10(a64)


def _rms(a64):
    return np.sqrt((a64 * a64).mean(axis=-1, keepdims=True))


def allowance_terms(a64):
    """the three terms of allowance_db, each float64 of a64's shape, in dB"""
    a64 = np.asarray(a64, np.float64)
    pos = a64 > 0
    safe = np.where(pos, a64, 1.0)
    d64 = 10.0 * np.log10(safe)
    t1 = np.where(pos, tol.db_map_bound_of_power(a64 * a64, d64), np.inf)
    t2 = np.full(a64.shape, (5.0 / np.log(10.0)) * POWER_ROUNDINGS * 2.0 ** -24)
    t3 = np.where(pos, (10.0 / np.log(10.0)) * CHAIN_EPS * _rms(a64) / safe, np.inf)
    return t1, t2, t3


def allowance_db(a64):
    """float64, a64's shape: how far a reported dB value may lie from dB64 = 10 log10 a64 if the path keeps its promise.  The sum of
      (1) tolerances.db_map_bound_of_power(a64^2, dB64): the dB map's own proven bound (max(4.2e-6 dB, 2.2 ulp of the value) below
          16 dB, 1 ulp from there up), against the float64 value of the float power the map receives;
      (2) the roundings between the double spectrum and that float power: POWER_ROUNDINGS = 4 (counted above, from `power_of` in
          scn_device.h and the finish kernel's casts), each 2^-24 of the power; dB = (5 / ln 10) ln P, so (5 / ln 10) * 4 * 2^-24
          = 5.2e-7 dB;
      (3) the double chain's own error: 2^-40 of the buffer's rms level in amplitude, (10 / ln 10) * 2^-40 * rms / a64 dB.  2^-40 is
          2^13 double epsilons: two transforms of length m <= 2^17 and a pointwise product, and numpy's own error with them, with three
          orders to spare -- and 2^17 below one float rounding of a work buffer (2^-24 of the rms level, about 1e-7), the fault
          the bar must see.
      (4) Bins with a64 < 2^-20 rms are not held to this (excluded(): there term (3) equals the map's 4.2e-6 dB floor); they stay
          under tolerances.floor_errors, and their share of a launch is a condition: at most MAX_EXCLUDED_SHARE, failing rather than
          skipping.  Checked on the CPU on dr_scenes.batch at every size of SIZES and every wire format the GPU module runs
          (tests/test_bluestein_cases_cpu.py): 0 ... 3.1e-5."""
    t1, t2, t3 = allowance_terms(a64)
    return t1 + t2 + t3


def excluded(a64):
    """boolean, a64's shape: term (4)"""
    a64 = np.asarray(a64, np.float64)
    return a64 < EXCLUDE_BELOW * _rms(a64)


def check_spectrum(db, a64, what):
    """a reported (or emulated) spectrum against the bar: asserts the excluded share and every other bin; returns the figures
    {excess, err_db, terms, excluded_share}: excess = the largest |dB - dB64| / allowance over the held bins, err_db and terms (the
    three of allowance_terms) at that bin"""
    fig = measure_spectrum(db, a64)
    assert fig["excluded_share"] <= MAX_EXCLUDED_SHARE, f"{what}: {fig['excluded_share']:.2e} of the bins lie below 2^-20 of the rms level"
    assert fig["excess"] <= 1.0, (f"{what}: a bin is {fig['err_db']:.3e} dB from float64, {fig['excess']:.3g} times what the promise allows "
                                  f"(map {fig['terms'][0]:.2e}, roundings {fig['terms'][1]:.2e}, chain {fig['terms'][2]:.2e} dB) at (buffer, j) {fig['at']}")
    return fig


def measure_spectrum(db, a64):
    """check_spectrum's figures without its assertions.  A NaN, a +inf or a -inf on a held bin is an infinite excess."""
    db = np.asarray(db, np.float64)
    a64 = np.asarray(a64, np.float64)
    assert db.shape == a64.shape
    out = excluded(a64)
    t1, t2, t3 = allowance_terms(a64)
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(db - 10.0 * np.log10(a64))
    err = np.where(np.isfinite(db), err, np.inf)
    ratio = np.where(out, 0.0, err / (t1 + t2 + t3))
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return {"excess": float(ratio[at]), "err_db": float(err[at]), "terms": (float(t1[at]), float(t2[at]), float(t3[at])),
            "excluded_share": float(out.mean()), "at": tuple(int(v) for v in at)}


def floor_bound_check(db, a64, what):
    """tolerances.floor_errors on the same output, bound by FLOOR_BOUND -- the chain's 2^-40 of the rms level plus one float
    rounding of it -- not by a float32 yardstick; covers the excluded bins, in amplitude"""
    fig = tol.floor_errors(db, a64)
    assert fig["floor_err"] <= FLOOR_BOUND, f"{what}: a floor bin is off by {fig['floor_err']:.3e} of the rms level, over {FLOOR_BOUND:.3e}"
    return fig


# ---- scenes and owed hit lists --------------------------------------------------------------------------------------------------
def scene(oracle_mod, n, kind, enob, dc, seed=500):
    """(raw, conv): a launch of count(n) buffers of dr_scenes.batch in the wire format, and what the oracle's converter makes of it"""
    x, _ = sc.batch(n, count(n), seed=seed + kind + enob + dc)
    raw = sc.to_wire(x, kind, enob, dc)
    return raw, sc.convert(oracle_mod, n, kind, enob, dc, raw)


def threshold_of(a64, d64, n):
    """the float32 threshold of a launch: 6 dB in power (a factor of two in amplitude) over the median of the evaluated bins -- the
    noise floor, the blocker's main lobe being a few dozen bins -- moved up by tolerances.pick_threshold until no evaluated bin lies
    within GUARD_DB of it.  allowance_db is three orders below GUARD_DB on every held bin, so the hit list is owed exactly."""
    ev = tol.evaluated_mask(n)
    return tol.pick_threshold(d64, n, start=float(10.0 * np.log10(2.0 * np.median(a64[..., ev]))))


def trigger_count_of(counts):
    """the plan's trigger_count for a launch that owes `counts` records per buffer: their median, so that about half of the flags
    (count > trigger_count, process.cpp:62) are set; where no buffer exceeds the median (18 points: the blocker's main lobe fills the
    six evaluated bins, nearly every buffer owes three records) the largest count below the maximum, so that flags of both kinds
    still occur -- the callers assert that they do"""
    counts = np.asarray(counts)
    trig = int(np.median(counts))
    if not (counts > trig).any() and (counts < counts.max()).any():
        trig = int(counts[counts < counts.max()].max())
    assert trig >= 1, "a trigger_count of 0 is the descriptor's default, 1047"
    return trig


def owed_hits(d64, n, thr, fc, seq, fs):
    """(records without power_db, counts [B]): what process.cpp:46-62 reports of the float64 spectrum d64 [B, n], ordered by
    (buffer, i): launch_caps.reference_hits for the bins, floor_ref._freq_hz for the frequencies"""
    from scanner_amd import capi
    from tests import floor_ref
    from tests import launch_caps as caps

    b, i = caps.reference_hits(d64, np.float32(thr), tol.evaluated_mask(n), n)
    rec = np.zeros(len(b), capi.HIT_DTYPE)
    rec["seq_id"], rec["i"] = np.asarray(seq, np.uint64)[b], i
    f = np.empty(len(b), np.uint64)
    for u in np.unique(b):
        f[b == u] = floor_ref._freq_hz(fc[u], i[b == u], n, fs)
    rec["freq_hz"] = f
    return rec, np.bincount(b, minlength=d64.shape[0])


# ---- the faults the bar is for, emulated in numpy -------------------------------------------------------------------------------
def bluestein_tables(n):
    """(m, chirp complex128 [n], filter transform / m complex128 [m]) as bluestein_tables of scn_host.hip builds them: w[i] =
    exp(-i pi (i^2 mod 2n) / n), the filter conj(w[|k|]) laid out cyclically over m points"""
    m = 1
    while m < 2 * n - 1:
        m *= 2
    i = np.arange(n, dtype=np.uint64)
    a = -np.pi * ((i * i) % np.uint64(2 * n)).astype(np.float64) / float(n)
    chirp = np.cos(a) + 1j * np.sin(a)
    b = np.zeros(m, np.complex128)
    b[:n] = np.conj(chirp)
    b[m - np.arange(1, n)] = np.conj(chirp[1:])
    return m, chirp, np.fft.fft(b) / m


def _c64(z):
    return z.astype(np.complex64).astype(np.complex128)


FAULTS = ("work", "chirp", "filter")


def emulate(xw, fault=None):
    """float64 dB [B, n]: the path's Bluestein convolution written out in numpy on the windowed float32 samples xw [B, n], in
    complex128 throughout, the spectrum's components cast to float32 once and the dB taken in float64 of their float64 squares.
    fault: None, or one of FAULTS --
      "work"    the work buffers rounded to complex64 after every length-m transform (a float work buffer);
      "chirp"   the chirp table rounded to float32;
      "filter"  the filter transform's table rounded to float32."""
    assert fault is None or fault in FAULTS
    xw = np.asarray(xw, np.complex64)
    n = xw.shape[-1]
    m, chirp, bf = bluestein_tables(n)
    if fault == "chirp":
        chirp = _c64(chirp)
    if fault == "filter":
        bf = _c64(bf)
    v = np.zeros(xw.shape[:-1] + (m,), np.complex128)
    v[..., :n] = xw.astype(np.complex128) * chirp
    f = np.fft.fft(v, axis=-1)
    if fault == "work":
        f = _c64(f)
    z = np.fft.fft(np.conj(f * bf), axis=-1)       # an inverse transform up to conjugations; the 1 / m is in bf
    if fault == "work":
        z = _c64(z)
    z = z[..., :n]                                  # (the final chirp and the conjugation have modulus one)
    re, im = z.real.astype(np.float32).astype(np.float64), z.imag.astype(np.float32).astype(np.float64)
    with np.errstate(divide="ignore"):
        return 5.0 * np.log10(re * re + im * im)


def float_faults(xw):
    """{None: dB, "work": dB, "chirp": dB, "filter": dB} of emulate"""
    return {f: emulate(xw, f) for f in (None,) + FAULTS}
