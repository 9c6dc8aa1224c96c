"""The definition of a signal list (include/scanner_hip.h, "Signals") restated in numpy, independently of the library: what
scn_signals_from_hits and scn_collect_signals are held to, record for record and bit for bit."""
import numpy as np

from scanner_amd import capi


def signals(hits, n, sample_rate, max_gap):
    """hits: a HIT_DTYPE list ordered as collect returns it -> SIGNAL_DTYPE.  A hit starts a signal when it is the first of its
    unit (the first of the list, another seq_id, or an i that does not increase) or lies more than max_gap + 1 bins above the
    hit before it; the peak is the largest power_db, the lowest i among equal ones (numpy's argmax takes the first)."""
    out = np.zeros(0, capi.SIGNAL_DTYPE)
    if len(hits) == 0:
        return out
    seq, i, p = hits["seq_id"], hits["i"].astype(np.int64), hits["power_db"]
    start = np.ones(len(hits), bool)
    start[1:] = (seq[1:] != seq[:-1]) | (i[1:] <= i[:-1]) | (i[1:] - i[:-1] > int(max_gap) + 1)
    a = np.flatnonzero(start)
    b = np.append(a[1:], len(hits))  # exclusive ends
    peak = np.array([lo + int(np.argmax(p[lo:hi])) for lo, hi in zip(a, b)])
    out = np.zeros(len(a), capi.SIGNAL_DTYPE)
    out["seq_id"] = seq[a]
    out["peak_freq_hz"] = hits["freq_hz"][peak]
    out["first_i"], out["last_i"], out["peak_i"] = i[a], i[b - 1], i[peak]
    out["n_hits"] = b - a
    out["peak_power_db"] = p[peak]
    bin_step = (int(sample_rate) & 0xFFFFFFFF) // int(n)  # process.cpp:39, uint32
    out["bandwidth_hz"] = ((i[b - 1] - i[a] + 1) * bin_step) & 0xFFFFFFFF
    return out


def assert_same(got, want, what=""):
    """equal record for record and bit for bit (the float field compared through its bits: -0.0 is not +0.0 here)"""
    assert got.dtype == capi.SIGNAL_DTYPE and want.dtype == capi.SIGNAL_DTYPE
    assert len(got) == len(want), (what, len(got), len(want))
    for f in capi.SIGNAL_DTYPE.names:
        g, w = got[f], want[f]
        if f == "peak_power_db":
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, f, int(bad[0]), got[bad[0]], want[bad[0]])
