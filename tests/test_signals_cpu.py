"""Signals without a GPU: the layout of scn_signal, and scn_signals_from_hits -- the host form of the merge, and the definition
the GPU form is held to (tests/test_signals_gpu.py) -- against the numpy restatement of tests/signals_ref.py and against
records written out by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from scanner_amd import capi
from tests import signals_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 8000000


def _hits(rows):
    """(seq_id, i, power_db, freq_hz) tuples -> HIT_DTYPE"""
    return np.array(rows, capi.HIT_DTYPE) if rows else np.zeros(0, capi.HIT_DTYPE)


def _sig(rows):
    """(seq_id, peak_freq_hz, first_i, last_i, peak_i, n_hits, peak_power_db, bandwidth_hz) tuples -> SIGNAL_DTYPE"""
    return np.array(rows, capi.SIGNAL_DTYPE) if rows else np.zeros(0, capi.SIGNAL_DTYPE)


def _raw(hits, n, fs, max_gap, cap, with_array=True):
    """one call of scn_signals_from_hits: (status, total, the array it was given)"""
    hits = np.ascontiguousarray(hits, capi.HIT_DTYPE)
    out = np.zeros(cap, capi.SIGNAL_DTYPE)
    out["n_hits"] = 0xDEADBEEF  # what the call does not store stays recognisable
    total = C.c_uint64(12345)
    st = capi.lib().scn_signals_from_hits(hits.ctypes.data_as(C.c_void_p), hits.size, n, fs, max_gap,
                                          out.ctypes.data_as(C.c_void_p) if with_array else None, cap, C.byref(total))
    return st, total.value, out


def test_signal_struct_layout(tmp_path):
    """40 bytes in C99 and C++11, every field where SIGNAL_DTYPE has it"""
    d = capi.SIGNAL_DTYPE
    assert d.itemsize == 40 and d.names == ("seq_id", "peak_freq_hz", "first_i", "last_i", "peak_i", "n_hits", "peak_power_db",
                                            "bandwidth_hz")
    checks = " + ".join("(int)(offsetof(scn_signal, %s) != %d) + (int)(sizeof(((scn_signal *)0)->%s) != %d)"
                        % (f, d.fields[f][1], f, d.fields[f][0].itemsize) for f in d.names)
    for comp, std, ext in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")):
        f = tmp_path / f"t.{ext}"
        f.write_text('#include <stddef.h>\n#include "scanner_hip.h"\nint main(void){ return (int)(sizeof(scn_signal) != 40) + %s; }\n' % checks)
        exe = tmp_path / f"t_{ext}"
        subprocess.check_call([comp, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(f), "-o", str(exe)])
        assert subprocess.call([str(exe)]) == 0, "scn_signal differs between the header and SIGNAL_DTYPE"
    assert d.fields["peak_power_db"][0] == np.dtype("<f4") and d.fields["seq_id"][0] == np.dtype("<u8")


def test_exported_where_the_others_are():
    import scanner_amd

    assert scanner_amd.SIGNAL_DTYPE is capi.SIGNAL_DTYPE and scanner_amd.signals_from_hits is capi.signals_from_hits
    assert hasattr(scanner_amd.Plan, "collect_signals")
    assert "scn_collect_signals" in capi.SYMBOLS and "scn_signals_from_hits" in capi.SYMBOLS


def test_empty_list_and_one_hit(built_lib):
    for gap in (0, 5):
        got = capi.signals_from_hits(_hits([]), 4096, FS, gap)
        assert got.dtype == capi.SIGNAL_DTYPE and len(got) == 0
        signals_ref.assert_same(got, signals_ref.signals(_hits([]), 4096, FS, gap))
    st, total, _ = _raw(_hits([]), 4096, FS, 0, 0, with_array=False)
    assert (st, total) == (capi.OK, 0)
    one = _hits([(7, 600, 12.5, 96171875)])
    want = _sig([(7, 96171875, 600, 600, 600, 1, 12.5, 1953)])  # 8000000 / 4096 = 1953 (truncating)
    for gap in (0, 1, 4096):
        got = capi.signals_from_hits(one, 4096, FS, gap)
        signals_ref.assert_same(got, want)
        signals_ref.assert_same(got, signals_ref.signals(one, 4096, FS, gap))


def test_hand_written_lists(built_lib):
    """The expected records are written out: a tie on power_db, a gap of exactly max_gap against max_gap + 1, and a unit boundary
    by seq_id change and by non-increasing i with equal seq_id.  64 points at 6400 Hz: 100 Hz per bin."""
    n, fs = 64, 6400
    hits = _hits([
        # unit seq 5: bins 10, 11, 12 with a tie between 10 and 12; then 15 (two empty bins), then 19 (three empty bins)
        (5, 10, 3.0, 1000), (5, 11, 1.0, 1100), (5, 12, 3.0, 1200), (5, 15, 2.0, 1500), (5, 19, 7.5, 1900),
        # unit seq 6 starts at the bin right above: not a continuation
        (6, 20, 1.5, 2000), (6, 21, 1.25, 2100),
        # another buffer with the SAME seq_id: i does not increase (21 -> 21), a new unit
        (6, 21, 9.0, 2100), (6, 22, -1.0, 2200),
        # and one whose first bin is lower
        (6, 8, 0.5, 800),
    ])
    gap0 = _sig([
        (5, 1000, 10, 12, 10, 3, 3.0, 300), (5, 1500, 15, 15, 15, 1, 2.0, 100), (5, 1900, 19, 19, 19, 1, 7.5, 100),
        (6, 2000, 20, 21, 20, 2, 1.5, 200), (6, 2100, 21, 22, 21, 2, 9.0, 200), (6, 800, 8, 8, 8, 1, 0.5, 100),
    ])
    # max_gap 2 bridges the two empty bins 13, 14 (exactly max_gap) but not the three 16, 17, 18 (max_gap + 1)
    gap2 = _sig([
        (5, 1000, 10, 15, 10, 4, 3.0, 600), (5, 1900, 19, 19, 19, 1, 7.5, 100),
        (6, 2000, 20, 21, 20, 2, 1.5, 200), (6, 2100, 21, 22, 21, 2, 9.0, 200), (6, 800, 8, 8, 8, 1, 0.5, 100),
    ])
    # max_gap 3 bridges both; the peak moves to bin 19; units still end where they ended
    gap3 = _sig([
        (5, 1900, 10, 19, 19, 5, 7.5, 1000),
        (6, 2000, 20, 21, 20, 2, 1.5, 200), (6, 2100, 21, 22, 21, 2, 9.0, 200), (6, 800, 8, 8, 8, 1, 0.5, 100),
    ])
    for gap, want in ((0, gap0), (2, gap2), (3, gap3), (64, gap3), (0xFFFFFFFF, gap3)):
        got = capi.signals_from_hits(hits, n, fs, gap)
        signals_ref.assert_same(got, want, f"gap {gap} against the records written out")
        signals_ref.assert_same(signals_ref.signals(hits, n, fs, gap), want, f"gap {gap}: the numpy reference")
    signals_ref.assert_same(capi.signals_from_hits(hits, n, fs, 1), gap0, "max_gap 1 bridges one bin: none of these gaps")


@pytest.fixture(scope="module")
def noise_lists(oracle_mod):
    """oracle hit lists of seeded complex Gaussian noise, 5 buffers, threshold at the median of the oracle's own spectrum"""
    out = {}
    for n in (16, 64, 4096):
        rng = np.random.default_rng(1)
        x = (rng.standard_normal((5, n, 2), dtype=np.float32) * np.float32(0.05)).view(np.complex64).reshape(5, n)
        fc = 1e9 + 6e6 * np.arange(5)
        seq = np.arange(100, 105, dtype=np.uint64)
        p, _, _ = oracle_mod.Oracle(n, FS, 1e9).run(x, fc, seq)
        _, hits, _ = oracle_mod.Oracle(n, FS, float(np.median(p))).run(x, fc, seq)
        out[n] = np.ascontiguousarray(hits).view(capi.HIT_DTYPE).reshape(-1)
    return out


@pytest.mark.parametrize("max_gap", [0, 1, 7, 64])
@pytest.mark.parametrize("n", [16, 64, 4096])
def test_oracle_noise_lists(built_lib, noise_lists, n, max_gap):
    hits = noise_lists[n]
    assert len(hits) > 5
    want = signals_ref.signals(hits, n, FS, max_gap)
    signals_ref.assert_same(capi.signals_from_hits(hits, n, FS, max_gap), want)
    assert int(want["n_hits"].sum()) == len(hits)
    per_buffer = np.bincount((want["seq_id"] - 100).astype(np.int64), minlength=5)
    if n == 4096:  # the regimes these lists are meant to reach
        if max_gap == 0:
            assert per_buffer.min() > 64 and np.all(want["n_hits"] == want["last_i"] - want["first_i"] + 1)
        if max_gap == 7:
            assert want["n_hits"].max() > 64 and (want["last_i"] - want["first_i"]).max() > 64
        if max_gap == 64:
            assert np.array_equal(per_buffer, np.ones(5, np.int64))


def test_windowing(built_lib, noise_lists):
    hits = noise_lists[4096]
    want = signals_ref.signals(hits, 4096, FS, 1)
    total = len(want)
    assert total > 100
    st, t, out = _raw(hits, 4096, FS, 1, 37)                    # cap below the total: a correct prefix, truncated
    assert (st, t) == (capi.E_TRUNCATED, total)
    signals_ref.assert_same(out, want[:37])
    st, t, out = _raw(hits, 4096, FS, 1, total + 3)             # room to spare: all of them, nothing beyond
    assert (st, t) == (capi.OK, total)
    signals_ref.assert_same(out[:total], want)
    assert np.all(out["n_hits"][total:] == 0xDEADBEEF)
    st, t, _ = _raw(hits, 4096, FS, 1, 0, with_array=False)     # the total alone
    assert (st, t) == (capi.E_TRUNCATED, total)
    st, t, out = _raw(hits, 4096, FS, 1, total)
    assert (st, t) == (capi.OK, total)


def test_peak_fields_are_the_hit_s_own_and_bandwidth_is_uint32(built_lib, noise_lists):
    hits = noise_lists[4096]
    for fs in (FS, 7999999):  # 7999999 / 4096 = 1953 (truncating)
        got = capi.signals_from_hits(hits, 4096, fs, 7)
        signals_ref.assert_same(got, signals_ref.signals(hits, 4096, fs, 7))
        key = {(int(h["seq_id"]), int(h["i"])): h for h in hits}
        for s in got:
            h = key[(int(s["seq_id"]), int(s["peak_i"]))]
            assert s["peak_freq_hz"] == h["freq_hz"] and s["peak_power_db"].tobytes() == h["power_db"].tobytes()
            assert int(s["bandwidth_hz"]) == (int(s["last_i"]) - int(s["first_i"]) + 1) * 1953
    # the product is uint32 arithmetic: it wraps (only a list whose bins exceed n can get there: 100 bins of 4294967295 / 64 Hz)
    wide = _hits([(1, 0, 1.0, 0), (1, 99, 2.0, 0)])
    got = capi.signals_from_hits(wide, 64, 4294967295, 98)
    assert len(got) == 1 and int(got["bandwidth_hz"][0]) == (100 * 67108863) % (1 << 32) != 100 * 67108863
    signals_ref.assert_same(got, signals_ref.signals(wide, 64, 4294967295, 98))
    # a peak of -0.0 keeps its sign bit, and +0.0 after it does not replace it (equal powers: the lowest i)
    zeros = _hits([(1, 5, -0.0, 50), (1, 6, 0.0, 60)])
    got = capi.signals_from_hits(zeros, 64, 6400, 0)
    assert int(got["peak_i"][0]) == 5 and got["peak_power_db"][0].tobytes() == np.float32(-0.0).tobytes()
    signals_ref.assert_same(got, signals_ref.signals(zeros, 64, 6400, 0))


def test_null_arguments_need_no_device(built_lib):
    L = capi.lib()
    total = C.c_uint32(9)
    assert L.scn_collect_signals(None, 0, 0, 0, None, 0, C.byref(total)) == capi.E_INVALID and b"null plan" in L.scn_last_error()
    assert L.scn_collect_signals(None, 0, 0, 0, None, 0, None) == capi.E_INVALID   # (no plan can exist here: both nulls at once)
    assert L.scn_collect_signals(None, 99, 0, 0, None, 0, C.byref(total)) == capi.E_INVALID
    hits = _hits([(1, 5, 1.0, 50)])
    assert L.scn_signals_from_hits(hits.ctypes.data_as(C.c_void_p), 1, 64, 6400, 0, None, 0, None) == capi.E_INVALID
    t64 = C.c_uint64()
    assert L.scn_signals_from_hits(None, 1, 64, 6400, 0, None, 0, C.byref(t64)) == capi.E_INVALID
    assert L.scn_signals_from_hits(hits.ctypes.data_as(C.c_void_p), 1, 0, 6400, 0, None, 0, C.byref(t64)) == capi.E_INVALID
