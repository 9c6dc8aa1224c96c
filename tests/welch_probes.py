"""Welch streams whose every PSD bin is known EXACTLY, shared by tests/test_welch_probes_cpu.py (which pins this generator against
float64 mathematics and the oracle) and tests/test_welch_exact_gpu.py (which holds the Welch epilogues' mean and dB map to the bit on
them).  Built on tests/db_probes.py; N = 65536, hop = N/2, rectangular window, DC removal off.

* Flat stream: delivery block b is a_b * delta[first sample of the block], a_b a small integer times the wire format's quantum.
  Segment s is blocks s and s + 1, the second impulse sits N/2 samples in:  X_s[k] = a_s + (-1)^k a_{s+1}  at every bin.  In the
  kernel's 256 x 256 decomposition (scn_welch.hip) both impulses sit in column n2 = 0 at n1 = 0 and 128, i.e. in thread 0's fft16
  inputs 0 and 8: they meet the +-1 paths of radix4 only, W^0 twiddles after it, and exact zeros everywhere else.  With every sum
  and difference of neighbours under 2^12 quanta each power is an integer number of quanta^2 under 2^24, and with K times the
  largest power under 2^24 the sum over a PSD's segments is exact in ANY order: the only rounding left is the mean's.
* Line stream: A i^t over the whole stream (constant amplitude: a step would leak) plus the flat stream as a floor.  i^t is constant
  down every column, so the column transform leaves 256 A i^n2 in row k1 = 0 and exact zeros elsewhere; the row transform puts
  N A at k = N/4.  Bin N/4 of segment s holds N A + a_s + a_{s+1} (N/4 is even) under 2^24 quanta, every other bin the flat value.
  The line's power is one rounding of an exact square (its distance to a rounding boundary is asserted, as db_probes.exact_power
  does for complex amplitudes); its sum over segments rounds at every add, which mean_float mirrors.

THE FLOAT THE MAP IS APPLIED TO (mean_float): scn_welch_rows_kernel adds the float powers of its part's segments in segment order
(`acc[q] += (float)fma(...)`, s = s_lo .. s_hi - 1 with s_lo = K part / parts, s_hi = K (part + 1) / parts); with parts == 1 it
reports db_of_power(acc[q] * args.inv_k); otherwise scn_welch_combine_kernel adds the parts in order (`sum = partial[0]; sum +=
partial[part]`) and reports db_of_power(sum[c] * args.inv_k).  inv_k is the float 1.0f / (float)K (welch_enqueue,
scn_welch_plan.hip).  The PRODUCT with the float 1/K is the definition (include/scanner_hip.h); the oracle's division differs from
it by at most one ulp of the mean where K is not a power of two."""
from fractions import Fraction

import numpy as np

from tests import db_probes as pr

F32 = np.float32
N = 65536
HOP = N // 2
# the line's quanta A: powers of two, so that in (N A + e)^2 = N^2 A^2 + 2 N A e + e^2 the middle term is a multiple of the power's ulp
# and only e^2 decides the rounding (with A = 60 or 200 every odd e lands within 1e-3 ulp of a tie)
LINE_A = {pr.KIND_FLOAT_COMPLEX: 128, pr.KIND_SHORT_COMPLEX: 128, pr.KIND_SHORT: 128, pr.KIND_BYTE_COMPLEX: 64}


def mean_float(powers, K, parts):
    """float32: the mean of the float powers [..., K] (segment axis last) as the kernels form it -- see the module docstring"""
    p = np.asarray(powers, F32)
    assert p.shape[-1] == K and 1 <= parts <= max(K, 1)
    total = None
    with np.errstate(over="ignore", invalid="ignore"):
        for part in range(parts):
            acc = np.zeros(p.shape[:-1], F32)
            for s in range((K * part) // parts, (K * (part + 1)) // parts):
                acc = (acc + p[..., s]).astype(F32)
            total = acc if total is None else (total + acc).astype(F32)
        return (total * (F32(1.0) / F32(K))).astype(F32)


def amp_limit(kind, K, line):
    """the largest |a_b| in quanta that keeps every precondition: |a_s +- a_{s+1}| < 2^12, K (2 a)^2 < 2^24, the wire format's range"""
    lim = min(2047, int(2048.0 / np.sqrt(K)) - 1)
    if kind != pr.KIND_FLOAT_COMPLEX:
        lim = min(lim, pr.INT_MAX[kind] - (LINE_A[kind] if line else 0))
    return lim


def amplitudes(kind, K, n_psd, seed, line=False):
    """int64 [n_psd K + 1]: block amplitudes in quanta, all different, no neighbours equal or opposite, as large as the format allows"""
    lim, nb = amp_limit(kind, K, line), n_psd * K + 1
    signed = np.concatenate([np.arange(1, lim + 1), -np.arange(1, lim + 1)])
    assert nb <= len(signed), "more blocks than distinct amplitudes"
    for attempt in range(1000):
        a = np.random.default_rng(list(np.atleast_1d(seed)) + [kind, K, n_psd, attempt]).choice(signed, nb, replace=False)
        if (a[:-1] != -a[1:]).all():
            return a.astype(np.int64)
    raise AssertionError("no amplitude draw without opposite neighbours")


class Stream:
    """One probe stream and what every PSD of it owes.  ia: block amplitudes in quanta [n_psd K + 1]; line: the quanta A of
    A i^t (0: flat stream).  zeros=True admits neighbours that cancel (a -inf bin wanted on purpose); distinct=False admits two blocks
    that are no neighbours with one amplitude (the chains of pin_streams, whose sums are prescribed); shift: a power of two that
    multiplies the float samples' quantum (exact: it moves every power by 2 log2 shift binades, into either half of the map)."""

    def __init__(self, kind, K, ia, line=0, zeros=False, distinct=True, shift=1.0):
        ia = np.asarray(ia, np.int64).reshape(-1)
        assert (len(ia) - 1) % K == 0 and len(ia) > 1
        self.kind, self.K, self.ia, self.line, self.n_psd = kind, K, ia, int(line), (len(ia) - 1) // K
        assert np.frexp(shift)[0] == 0.5 and (shift == 1.0 or kind == pr.KIND_FLOAT_COMPLEX), "shift: a power of two, float samples only"
        self.shift, self.scale = float(shift), pr.scale_of(kind) * float(shift)
        ev, od = ia[:-1] + ia[1:], ia[:-1] - ia[1:]
        # the exactness preconditions, asserted (not hoped for)
        assert max(np.abs(ev).max(), np.abs(od).max()) < 1 << 12, "a sum or difference of neighbours reaches 2^12 quanta"
        assert K * int(max((ev * ev).max(), (od * od).max())) < 1 << 24, "K times the largest power reaches 2^24 quanta^2"
        if not zeros:
            assert (od != 0).all() and (ev != 0).all(), "neighbouring blocks carry equal or opposite amplitudes"
            assert not distinct or len(np.unique(ia)) == len(ia), "two blocks carry the same amplitude"
        ln = N * self.line + ev
        assert np.abs(ln).max() < 1 << 24, "the line bin is no float"
        if kind != pr.KIND_FLOAT_COMPLEX:
            assert np.abs(ia).max() + abs(self.line) <= pr.INT_MAX[kind]
        self.seg_quanta = {"even": ev, "odd": od, "line": ln}
        # the float bin values (exact) and their float powers, [n_psd, K]
        val = {k: (v.astype(np.float64) * self.scale).astype(F32) for k, v in self.seg_quanta.items()}
        for k, v in val.items():
            assert np.array_equal(v.astype(np.float64), self.seg_quanta[k] * self.scale)
        self.power = {k: pr.exact_power(v.astype(np.complex64))[: self.n_psd * K].reshape(self.n_psd, K) for k, v in val.items()}
        for k in ("even", "odd"):   # exact as rationals
            q2 = (self.seg_quanta[k] ** 2).reshape(self.n_psd, K)
            assert np.array_equal(self.power[k].astype(np.float64), q2 * self.scale ** 2), "a flat power is not exact"
            assert np.array_equal(self.power[k].astype(np.float64).sum(axis=1), q2.sum(axis=1) * self.scale ** 2)
        if self.line:   # one rounding of an exact square, clear of a rounding boundary (a residue of the double pass cannot move it)
            for q in ln:
                want, margin = pr._round_f32(Fraction(int(q)) ** 2 * Fraction(self.scale) ** 2)
                assert margin > 2.0 ** -20, "the line's power sits on a rounding boundary"
                assert want == pr.exact_power(np.array([q * self.scale], np.complex64))[0]

    def ints(self):
        """int64 [blocks, HOP, 2] in quanta"""
        nb = len(self.ia)
        return pr.line_ints(HOP, np.full(nb, self.line), np.zeros(nb, np.int64), self.ia)

    def raw(self, n_psd=None):
        """the wire format's bytes of the first n_psd PSDs' blocks (uint8, flat): delivery blocks of HOP samples back to back"""
        nb = len(self.ia) if n_psd is None else n_psd * self.K + 1
        x = pr.pack(self.kind, self.ints()[:nb])
        if self.shift != 1.0:
            x = (x * F32(self.shift)).astype(np.complex64)
        return np.ascontiguousarray(x).view(np.uint8).reshape(-1)

    def complex64(self):
        """the converted stream (what K1 leaves): complex64 [blocks * HOP]"""
        q = self.ints().astype(np.float64) * self.scale
        return (q[..., 0] + 1j * q[..., 1]).astype(np.complex64).reshape(-1)

    def means(self, parts):
        """{"even", "odd", "line"} -> float32 [n_psd]: the float the map is applied to in every even / odd bin and in bin N/4"""
        return {k: mean_float(p, self.K, parts) for k, p in self.power.items()}

    def stated_means(self, parts):
        """float32 [n_psd, N]: the mean every bin of every PSD owes"""
        m = self.means(parts)
        out = np.empty((self.n_psd, N), F32)
        out[:, 0::2], out[:, 1::2] = m["even"][:, None], m["odd"][:, None]
        if self.line:
            out[:, N // 4] = m["line"]
        return out


def flat(kind, K, n_psd, seed=0, shift=1.0):
    return Stream(kind, K, amplitudes(kind, K, n_psd, seed), shift=shift)


def line(kind, K, n_psd, seed=0):
    for attempt in range(100):   # (a draw whose line power sits near a rounding boundary is drawn again)
        try:
            return Stream(kind, K, amplitudes(kind, K, n_psd, [seed, attempt], line=True), line=LINE_A[kind])
        except AssertionError as exc:
            if "rounding boundary" not in str(exc):
                raise
    raise AssertionError("no line stream clear of the rounding boundaries")


def db64_of_mean(m):
    return pr.db64(m)


# ---- K not a power of two: streams whose product-form mean is a float that a K = 4 stream reaches too -------------------------------
def _two_squares(rest, lo, hi):
    """(x, y) in [lo, hi] with x^2 + y^2 == rest, or None"""
    xs = np.arange(lo, hi + 1, dtype=np.int64)
    r = rest - xs * xs
    y = np.sqrt(np.maximum(r, 0)).astype(np.int64)
    ok = np.flatnonzero((r > 0) & (y * y == r) & (y >= lo) & (y <= hi))
    return (int(xs[ok[0]]), int(y[ok[0]])) if ok.size else None


def product_form_pins(K, count, seed=0):
    """[(m, [e_0 .. e_{K-1}], [f_0 .. f_3])]: integers (quanta) with S = sum e_i^2 < 2^24 and every K e_i^2 < 2^24, whose mean under
    the product form m = fl(S * fl(1/K)) differs from the division's fl(S / K), and four f_j with sum f_j^2 == 4 m exactly (every
    4 f_j^2 < 2^24).  A PSD whose K segments hold the even-bin values e_i owes the map the float m quanta^2 under the product form --
    the very float a K = 4 PSD of the f_j owes, where the mean is exact under either form -- and its neighbour under the division."""
    rng = np.random.default_rng([seed, K])
    inv, lim = F32(1.0) / F32(K), int(4096.0 / np.sqrt(K)) - 1
    out = []
    for _ in range(200000):
        if len(out) == count:
            break
        es = rng.integers(min(lim, 2040) - 120, min(lim, 2040) + 1, K)   # (m < 2^22: 4 m stays under 2^24)
        S = int((es * es).sum())
        m = F32(S) * inv
        m4 = 4.0 * float(m)
        if not (S < 1 << 24 and m != F32(S) / F32(K) and m4 == int(m4) and m4 < 1 << 24):
            continue
        q2 = F32(pr.CFLOAT_QUANTUM ** 2)
        if pr.db64(m * q2).astype(F32) == pr.db64(F32(S) / F32(K) * q2).astype(F32):   # (the two means round to one dB float: a blunt pin)
            continue
        r = int(np.sqrt(m4 / 4.0))
        fs = rng.integers(r - 150, r + 150, 2)
        last = _two_squares(int(m4) - int((fs * fs).sum()), max(1, r - 400), min(2047, r + 400))
        if last and int(fs.max()) <= 2047:
            out.append((m, [int(v) for v in es], [int(v) for v in fs] + list(last)))
    assert len(out) == count, f"found {len(out)} of {count} product-form pins for K = {K}"
    return out


def chain(groups, first):
    """block amplitudes with a_s + a_{s+1} running through the values of each group in turn (one group per PSD, taken in the order
    that keeps neighbours closest: the sums are exact, so the order inside a PSD does not matter), starting at `first`"""
    a = [int(first)]
    for g in groups:
        rest = list(g)
        while rest:
            e = min(rest, key=lambda v: (abs(v - 2 * a[-1]) == 0, abs(v - 2 * a[-1])))
            rest.remove(e)
            a.append(int(e) - a[-1])
    return np.array(a, np.int64)


def pin_streams(K, n_psd, seed=0):
    """(the K-segment cfloat stream, its K = 4 partner, the pins): PSD p of the first owes the mean m_p quanta^2 in its even bins
    under the product form, and so does PSD p of the second, where the mean is exact"""
    pins = product_form_pins(K, n_psd, seed)
    out = []
    for k, groups in ((K, [es for _, es, _ in pins]), (4, [fs for _, _, fs in pins])):
        mid = groups[0][0] // 2
        for first in range(mid - 300, mid + 300):
            try:
                out.append(Stream(pr.KIND_FLOAT_COMPLEX, k, chain(groups, first), distinct=False))
                break
            except AssertionError:
                continue
        else:
            raise AssertionError(f"no admissible chain for K = {k}")
    return out[0], out[1], pins
