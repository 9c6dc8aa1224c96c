"""High-dynamic-range scenes, shared by tests/test_dynamic_range_cpu.py (which pins what the scenes are, and the floor metric of
tests/tolerances.py floor_errors on them) and tests/test_dynamic_range_gpu.py (which holds every kernel family to that metric).

The scene a scanner exists for: one strong transmitter in band, weak signals beside it.

* the blocker: amplitude 0.5, at an off-grid frequency inside the used band, drawn per buffer (per GROUP in an averaged scene, once
  in a stream), so that over a launch it visits the whole band;
* complex noise of sigma = 1e-4 per component: 74 dB under the blocker.  A noise bin's power is 2 sigma^2 sum(w^2) against a mean
  over the buffer of 0.25 sum(w^2): 8e-8 of the mean, two orders of magnitude below REL_POWER = 1e-5 of it -- the spectrum is a
  few dozen main-lobe bins and a floor that tests/tolerances.py compare_spectra cannot see;
* three weak tones at WEAK_DB = -20, -5 and +10 dB of sigma, at frequencies fixed per scene (every buffer has them at the same
  bins, within a quarter of a bin of a bin centre), so that their level over the floor can be stated: a tone of amplitude a at
  offset d from a bin centre gives a sum(w) S(d) there, S >= 0.93 for |d| <= 0.25 with Blackman-Harris, against a noise bin's rms
  amplitude sigma sqrt(2 sum(w^2)) -- weak_excess_db();
* a phase per buffer for the blocker and for every tone.

Integer scenes quantise the same floats through scanner_amd.synth.quantize at full scale 2^(ENOB - 1) - 1; the quantisation noise
(1.4e-4 per component at ENOB 12, 8.8e-6 at 16) joins the floor.  With DC removal the scene carries a positive offset for the
integer mean to take out (the negative-sum quirk of utility.cpp:77-78 has its own tests); to_wire() asserts the sums positive."""
import numpy as np

SIGMA = 1e-4
BLOCKER = 0.5
WEAK_DB = (-20.0, -5.0, 10.0)
DC_OFFSET = 0.09 + 0.08j   # above the blocker's largest partial sum over a buffer, 0.5 / (n sin(4.5 pi / n)) < 0.036 per sample


def _band(n):
    """(lo, hi): |signed bin| of the evaluated band, clear of the DC window (4 bins) and of the edge at 0.75 n / 2"""
    return 4.5, max(5.5, 0.70 * n / 2.0)


def _draw_freq(rng, n, size):
    lo, hi = _band(n)
    return rng.uniform(lo, hi, size) * rng.choice([-1.0, 1.0], size)


def weak_freqs(n, seed):
    """the three weak tones' frequencies in signed bins, fixed per (n, seed): bin centre + U[-0.25, 0.25], distinct bins"""
    rng = np.random.default_rng([seed, n, 77])
    top = max(6, int(0.70 * n / 2.0))
    cand = np.concatenate([np.arange(5, top + 1), -np.arange(5, top + 1)]).astype(np.float64)
    k = rng.choice(cand, len(WEAK_DB), replace=False)
    return k + rng.uniform(-0.25, 0.25, len(k))


def weak_excess_db(n, window, db):
    """10 log10 of (a tone of `db` dB of sigma at its bin, scalloping 0.93) / (the rms amplitude of a noise bin), in the project's
    dB (10 log10 of an amplitude)"""
    w = np.asarray(window, np.float64)
    a = SIGMA * 10.0 ** (db / 20.0)
    return 10.0 * np.log10(0.93 * a * w.sum() / (SIGMA * np.sqrt(2.0 * (w * w).sum())))


def _compose(rng, n, f_blocker, copies):
    """complex128 [G * copies, n]: scene g's blocker at f_blocker[g] in each of its copies; fresh noise and a fresh phase per row"""
    G = len(f_blocker)
    B = G * copies
    k = np.arange(n, dtype=np.float64)[None, :]
    fb = np.repeat(f_blocker, copies)[:, None]
    x = BLOCKER * np.exp(1j * (2.0 * np.pi * fb * k / n + rng.uniform(0, 2 * np.pi, (B, 1))))
    x += SIGMA * (rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n)))
    return x


def batch(n, nb, seed, copies=1):
    """(x complex64 [nb * copies, n], info): nb scenes of `copies` buffers each -- the same blocker and weak tones within a scene,
    independent noise and phases per copy -- laid out scene after scene (the dwell layout of an averaged plan; regroup() gives the
    sweeps layout).  info: f_blocker [nb] and f_weak [3] in signed bins."""
    rng = np.random.default_rng([seed, n, copies])
    fb = _draw_freq(rng, n, nb)
    x = _compose(rng, n, fb, copies)
    fw = weak_freqs(n, seed)
    k = np.arange(n, dtype=np.float64)[None, :]
    for f, db in zip(fw, WEAK_DB):
        x += SIGMA * 10.0 ** (db / 20.0) * np.exp(1j * (2.0 * np.pi * f * k / n + rng.uniform(0, 2 * np.pi, (nb * copies, 1))))
    return x.astype(np.complex64), {"f_blocker": fb, "f_weak": fw}


def regroup(x, nb, copies):
    """dwell order (scene g's copies at g K ... g K + K - 1) -> sweeps order (at g, g + G, ...)"""
    perm = np.array([g * copies + k for k in range(copies) for g in range(nb)])
    return x[perm], perm


def stream(n, m, seed):
    """(x complex64 [m], info): the scene as one continuous stream of m samples for a Welch plan of n points: blocker, weak tones
    and noise run through; frequencies in signed bins of the n-point transform"""
    rng = np.random.default_rng([seed, n, m])
    fb = _draw_freq(rng, n, 1)
    fw = weak_freqs(n, seed)
    t = np.arange(m, dtype=np.float64)
    x = BLOCKER * np.exp(1j * (2.0 * np.pi * fb[0] * t / n + rng.uniform(0, 2 * np.pi)))
    x += SIGMA * (rng.standard_normal(m) + 1j * rng.standard_normal(m))
    for f, db in zip(fw, WEAK_DB):
        x += SIGMA * 10.0 ** (db / 20.0) * np.exp(1j * (2.0 * np.pi * f * t / n + rng.uniform(0, 2 * np.pi)))
    return x.astype(np.complex64), {"f_blocker": fb, "f_weak": fw}


def full_scale(enob):
    return (1 << (enob - 1)) - 1


def to_wire(x, kind, enob, dc):
    """the wire format's raw array of scene x ([..., n] complex64) through synth.quantize; with dc the positive offset first"""
    from scanner_amd import capi, synth

    if kind == capi.KIND_FLOAT_COMPLEX:
        assert not dc, "DC removal is the integer converters' (utility.cpp:9-84)"
        return np.ascontiguousarray(x, np.complex64)
    if dc:
        x = (x + np.complex64(DC_OFFSET)).astype(np.complex64)
    raw = synth.quantize(x, kind, full_scale=full_scale(enob))
    if dc:
        sums = raw.astype(np.int64).sum(axis=-1 if kind == capi.KIND_SHORT else -2)   # I and Q sums of every buffer
        assert (sums > 0).all(), "a buffer's integer sum is not positive: the DC quirk would be in play"
    return raw


def signed_to_natural(f, n):
    """nearest natural bin j of a frequency in signed bins"""
    return np.rint(np.asarray(f)).astype(np.int64) % n


# ---- the float64 reference and the yardstick ------------------------------------------------------------------------------------
def convert(oracle_mod, n, kind, enob, dc, raw):
    """complex64 [B, n]: the wire buffers through the oracle's converter (bit-pinned to the reference's utility.cpp)"""
    o = oracle_mod.Oracle(n, kind=kind, enob=enob, correct_dc=dc)
    raw = np.ascontiguousarray(raw)
    return np.stack([o.convert(raw[b]) for b in range(raw.shape[0])])


def windowed(conv, window):
    """the float32 product x * w, as process.cpp:28-34 forms it: the reference's one defined rounding stays out of the error"""
    return (conv * np.asarray(window, np.float32)[None, :]).astype(np.complex64)


def ref64_power(conv, window):
    """float64 [B, n]: |DFT|^2 in complex128 of the float32 product"""
    X = np.fft.fft(windowed(conv, window).astype(np.complex128), axis=-1)
    return X.real ** 2 + X.imag ** 2


def group_mean(P, copies, sweeps=False):
    """[B, n] -> [B / K, n]: the mean over each group's K members (dwell: g K ... g K + K - 1; sweeps: g, g + G, ...)"""
    if copies == 1:
        return P
    G = P.shape[0] // copies
    return (P.reshape(copies, G, -1).mean(axis=0) if sweeps else P.reshape(G, copies, -1).mean(axis=1))


def _db_to_power(db):
    db = np.asarray(db, np.float64)
    return np.where(np.isfinite(db), np.power(10.0, np.where(np.isfinite(db), db, 0.0) / 5.0), 0.0)


def _power_to_db(P):
    with np.errstate(divide="ignore"):
        return 5.0 * np.log10(P)


def float32_dbs(oracle_mod, n, kind, enob, dc, raw, conv, window):
    """{name: dB [B, n]} of the float32 transforms that are not a kernel under test, on the very buffers: the oracle's chain
    through Oracle.run (default mode; powers of two only -- its transform of other lengths runs in double) and scipy.fft on
    complex64 through tests/test_oracle_vs_pocketfft.py float32_chain"""
    from tests.test_oracle_vs_pocketfft import float32_chain

    out = {"pocketfft": float32_chain(conv, window)}
    if n & (n - 1) == 0:
        out["oracle"] = oracle_mod.Oracle(n, 8000000, 1e9, kind=kind, enob=enob, correct_dc=dc).run(raw, want_hits=False, threads=8)[0]
    return out


def yardstick(tol, dbs, a64, copies=1, sweeps=False):
    """Y: the larger floor_errors figure of the float32 transforms `dbs` against the float64 amplitudes a64 [G, n] (of the group
    means where copies > 1: each transform's powers are averaged over the group first); and the figure of each"""
    each = {}
    for name, db in dbs.items():
        if copies > 1:
            db = _power_to_db(group_mean(_db_to_power(db), copies, sweeps))
        each[name] = tol.floor_errors(db, a64)["floor_err"]
    return max(each.values()), each


# ---- what the GPU module covers, and what every scene must be -------------------------------------------------------------------
BLUESTEIN_SIZES = [17, 1023, 4097, 20000, 65535]
FOUR_STEP_SIZES = [32768, 65536]
# below 64 points the blocker's main lobe (9 bins) is half the spectrum: the float64 figures of the cfloat scene, +- 0.02
SMALL_FLOOR_SHARE = {16: 0.521, 17: 0.551, 32: 0.766}


def fused_sizes():
    """(powers of two, mixed-radix sizes) the LIBRARY says it runs fused -- the way tests/test_dispatch_gpu.py takes them"""
    from scanner_amd import capi

    pow2 = [1 << k for k in range(4, 17) if capi.size_path(1 << k) == capi.PATH_FUSED]
    mixed = [n for n in range(17, 16384) if n & (n - 1) and capi.size_path(n) == capi.PATH_FUSED]
    return pow2, mixed


def spectrum_sizes():
    pow2, mixed = fused_sizes()
    return pow2 + mixed + FOUR_STEP_SIZES + BLUESTEIN_SIZES


def assert_floor_share(n, share):
    """every scene's share of floor bins, asserted wherever a scene is used"""
    if n in SMALL_FLOOR_SHARE:
        assert abs(share - SMALL_FLOOR_SHARE[n]) <= 0.02, (n, share)
    else:
        assert n >= 64 and share >= (0.95 if n >= 1000 else 0.85), (n, share)
