"""scn_hit_prefilter (scn_kernels.h) on the host: the linear-power gate every hits-only plan applies before it forms a dB value.

The header's own function is compiled into a small driver and run over a dense sweep of thresholds, -230 ... 195 dB and the
special values.  Asserted against float64 mathematics:
  * soundness: every float power P whose dB value 5 log10 P exceeds T minus the device map's error bound (DESIGN.md section
    3.1: max(4.2e-6 dB, 2.2 ulp of the value), plus the half ulp of rounding the value to float) is > p_lo -- so a bin that
    the map can put above the threshold is never dropped by the gate, also where p_lo is a denormal or 10^(T/5) is near
    FLT_MAX;
  * usefulness: in the normal range p_lo is at least 0.999 * 10^(T/5), so the gate still keeps the noise out."""
import os
import subprocess

import numpy as np
import pytest

from scanner_amd import build
from tests import tolerances as tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FLT_MIN, FLT_MAX, DENORM_MIN = np.finfo(F32).tiny, np.finfo(F32).max, F32(np.finfo(F32).smallest_subnormal)

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "scn_kernels.h"
int main(int argc, char **argv) {
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  float t;
  while (fread(&t, 4, 1, in) == 1) {
    const float p = scn_hit_prefilter(t);
    fwrite(&p, 4, 1, out);
  }
  fclose(in);
  fclose(out);
  return 0;
}
"""


@pytest.fixture(scope="module")
def prefilter(tmp_path_factory):
    d = tmp_path_factory.mktemp("prefilter")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    # the compiler that builds the library (scn_submit.hip calls the function in its host pass), host pass only
    subprocess.check_call([build.hipcc(), "-x", "hip", "--offload-host-only", "-std=c++17", "-O2", "-I", build.CSRC, str(src),
                           "-o", str(exe)])

    def run(thr):
        thr = np.ascontiguousarray(thr, F32)
        (d / "t.bin").write_bytes(thr.tobytes())
        subprocess.check_call([str(exe), str(d / "t.bin"), str(d / "p.bin")])
        return np.frombuffer((d / "p.bin").read_bytes(), F32).copy()

    return run


def _db(p):
    with np.errstate(divide="ignore"):
        return 5.0 * np.log10(np.asarray(p, np.float64))


def _map_bound(t):
    """the device map's error bound at a value near t (tests/tolerances.py), plus half an ulp of rounding to float"""
    t = np.abs(np.asarray(t, np.float64))
    return tol.db_map_bound(t) + 0.5 * np.spacing(t.astype(F32)).astype(np.float64)


def _smallest_float_above(t_db):
    """the smallest float P with 5 log10 P > t_db (float64 arithmetic; +inf where none is finite)"""
    t_db = np.asarray(t_db, np.float64)
    with np.errstate(over="ignore"):
        p = np.power(10.0, t_db / 5.0).astype(F32)
    # walk to the boundary: at most a few ulp off after the rounding of pow and of the cast
    for _ in range(8):
        lo = np.nextafter(p, F32(0))
        step_down = (_db(lo) > t_db) & (p > 0)
        p = np.where(step_down, lo, p)
    for _ in range(8):
        step_up = ~(_db(p) > t_db) & np.isfinite(p)
        p = np.where(step_up, np.nextafter(p, F32(np.inf)), p)
    # converged: p is above t_db (or +inf) and its lower neighbour is not
    assert ((_db(p) > t_db) | (p == np.inf)).all()
    assert ~((_db(np.nextafter(p, F32(0))) > t_db) & (p > 0)).any()
    return p


def _sweep():
    dense = np.arange(-230.0, 195.0, 0.0137, dtype=np.float64).astype(F32)
    edges = np.array([_db(FLT_MIN), _db(DENORM_MIN), _db(FLT_MAX), -189.65, -200.0, -224.0, 0.0, -0.0, 1e-3, -1e-3,
                      15.99999, 16.0, 16.00001, 60.0, 150.0, 192.6, 192.65], np.float64).astype(F32)
    near = np.concatenate([e + np.arange(-40, 41) * np.spacing(np.abs(e)) for e in edges]).astype(F32)
    return np.unique(np.concatenate([dense, edges, near]))


def test_prefilter_is_sound_and_useful(prefilter):
    t = _sweep()
    p_lo = prefilter(t)
    assert not np.isnan(p_lo).any()
    # soundness: the first power the map may put above t passes the gate
    first = _smallest_float_above(t.astype(np.float64) - _map_bound(t))
    bad = ~(first > p_lo)
    assert not bad.any(), [(float(a), float(b), float(c)) for a, b, c in zip(t[bad][:5], p_lo[bad][:5], first[bad][:5])]
    # usefulness, in the normal range (below FLT_MIN the float grid itself is coarser than 0.1 %)
    normal = (t > _db(FLT_MIN) + 0.01) & (t < _db(FLT_MAX) - 0.01)
    want = 0.999 * np.power(10.0, t[normal].astype(np.float64) / 5.0)
    assert (p_lo[normal].astype(np.float64) >= want).all()
    # p_lo is a denormal where 10^(T/5) is one, and finite up to the largest threshold a float power can exceed
    assert (p_lo[(t < _db(FLT_MIN) - 1.0) & (t > _db(DENORM_MIN) + 1.0)] < FLT_MIN).all()
    assert np.isfinite(p_lo[t <= _db(FLT_MAX)]).all()
    fin = np.isfinite(first) & (p_lo > 0)
    print(f"{t.size} thresholds; the gate sits {float(np.min(_db(first[fin]) - _db(p_lo[fin]))):.2e} .. "
          f"{float(np.max(_db(first[fin]) - _db(p_lo[fin]))):.2e} dB below the first power the map may put above T")


def test_prefilter_special_values(prefilter):
    t = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 400.0, -400.0], F32)
    p = prefilter(t)
    assert np.isnan(p[0])                      # NaN: nothing passes (P > NaN is false), and nothing can hit
    assert np.isnan(p[1]) or p[1] == np.inf    # +inf: no dB value exceeds it, so the gate may pass nothing
    assert p[2] == 0.0                         # -inf: every nonzero power passes the gate (the device's map then sends a denormal one to -inf: no hit)
    assert p[3] == p[4] and 0.999 < p[3] <= 1.0
    assert p[5] == FLT_MAX or p[5] == np.inf   # above FLT_MAX's 192.65 dB only +inf power can hit: an inf-valued bin
    assert p[6] == 0.0                         # below every denormal: the smallest denormal still passes the gate (tests/test_db_map_gpu.py: not the map)
