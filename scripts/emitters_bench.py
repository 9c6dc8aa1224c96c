"""What one scn_plan_trace_emitters call costs (scn_emitters.hip) -- the first page of 1024 records of a whole trace's emitters on
the MAX line -- beside the route it replaces, in the same process: scn_plan_get_trace of the same window (16 bytes per cell over
PCIe) followed by the host form scn_trace_emitters.

    python scripts/emitters_bench.py [--json OUT] [--reps 20]

Windows of 2^16, 2^20 and 2^22 cells, each with three traces planted by scn_plan_merge_trace:
  sparse       about 1 % of the cells on, in runs of 1 ... 8 cells (seed 1), max_gap 0
  one          every cell on: the whole window is one emitter, max_gap 0
  alternating  every other cell on, max_gap 0: cells / 2 emitters of one cell each, the most a window can hold
The three shapes are the claim under test: no thread or wave walks a run, so a window should cost the same whatever its emitters
look like.  Per row (`reps` timed calls after WARM untimed ones; a host clock around the synchronous call):
  gpu_us           scn_plan_trace_emitters, cap 1024: median; gpu_min_us, gpu_p10_us, gpu_p90_us: the least, and the spread
  get_trace_us     scn_plan_get_trace of the window (median of HOST_REPS)
  host_emitters_us scn_trace_emitters on what it returned, cap 1024 (median of HOST_REPS)
  host_route_us    their sum
  emitters         the window's total
The first page of both routes is compared, byte for byte, in every row.  Each row carries the build hash."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scanner_amd import Plan, build, capi  # noqa: E402

WARM, HOST_REPS, PAGE = 3, 5, 1024
SIZES = (1 << 16, 1 << 20, 1 << 22)
F0, HZ, THR = 400000000, 1000, -50.0


def _clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e6, out


def trace_of(shape, cells):
    on = np.zeros(cells, bool)
    if shape == "one":
        on[:] = True
    elif shape == "alternating":
        on[::2] = True
    else:
        rng = np.random.default_rng(1)
        starts = rng.integers(0, cells, cells // 450)  # runs of 4.5 cells on average: 1 % of the cells
        for k, length in enumerate(rng.integers(1, 9, starts.size)):
            on[starts[k]:starts[k] + length] = True
    mx = np.where(on, np.float32(-20.0), np.float32(-90.0)).astype(np.float32)
    mx[on] += (np.arange(int(on.sum())) % 7).astype(np.float32)
    return mx, (mx - np.float32(5)).astype(np.float32), np.full(cells, 3, np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    L = capi.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rows = []
    with Plan(16, 8000000, 1e9, max_batch=1) as plan:
        for cells in SIZES:
            for shape in ("sparse", "one", "alternating"):
                plan.set_trace(F0, HZ, cells)
                plan.merge_trace(*trace_of(shape, cells))
                page, n = np.zeros(PAGE, capi.EMITTER_DTYPE), C.c_uint32()

                def gpu():
                    st = L.scn_plan_trace_emitters(plan.handle, 0, cells, capi.TRACE_LINE_MAX, THR, 0, 0, vp(page), PAGE, C.byref(n))
                    assert st in (capi.OK, capi.E_TRUNCATED), st

                t = np.array([_clock(gpu)[0] for _ in range(WARM + args.reps)][WARM:])
                get, host = [], []
                host_page, total = np.zeros(PAGE, capi.EMITTER_DTYPE), C.c_uint64()
                for _ in range(HOST_REPS):
                    us, tr = _clock(lambda: plan.trace(0, cells))
                    get.append(us)

                    def on_host():
                        st = L.scn_trace_emitters(vp(tr[0]), vp(tr[1]), vp(tr[2]), F0, HZ, cells, 0, capi.TRACE_LINE_MAX, THR, 0, vp(host_page), PAGE,
                                                  C.byref(total))
                        assert st in (capi.OK, capi.E_TRUNCATED), st

                    host.append(_clock(on_host)[0])
                assert total.value == n.value and page.tobytes() == host_page.tobytes(), (cells, shape)
                row = {"cells": cells, "shape": shape, "emitters": int(n.value), "reps": args.reps, "gpu_us": round(float(np.median(t)), 1),
                       "gpu_min_us": round(float(t.min()), 1), "gpu_p10_us": round(float(np.percentile(t, 10)), 1),
                       "gpu_p90_us": round(float(np.percentile(t, 90)), 1), "get_trace_us": round(float(np.median(get)), 1),
                       "host_emitters_us": round(float(np.median(host)), 1), "build": build.source_hash()}
                row["host_route_us"] = round(row["get_trace_us"] + row["host_emitters_us"], 1)
                rows.append(row)
                print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
