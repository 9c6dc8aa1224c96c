"""What the level histogram's fold costs (scn_plan_update_levels; scn_levels.hip) on a C2-shaped plan -- 8192 buffers of 4096 cfloat
points, spectrum + hits -- beside the two things it stands next to, on the same collected submit and in the same run:
  (a) scn_plan_update_trace on the same collected slot and the same grid: it reads the same 128 MiB;
  (b) the host route the fold replaces: scn_collect with power_db (128 MiB over PCIe) plus scn_levels_fold_spectrum on the host.

    python scripts/levels_bench.py [--json OUT] [--reps 20]

Rows (inputs: synth.cfloat_batch_torch, seed 2; a fixed threshold nothing exceeds, so no hit list is built), those of
scripts/trace_bench.py; the level table has 63 edges one unit apart around the noise level (the median of the first unit's dB values):
  wide      centres 6 MHz apart (adjacent bands touch), cell_hz = 64 bin_step: a unit's band covers about 49 cells, the team's tile 64;
            the sweep's 393258 cells times 64 levels exceed SCN_LEVELS_WORDS_MAX: the grid is its first 2^18 cells (32.8 GHz, 5461 of
            the 8192 units; the others are streamed and fold nowhere), for (a) as well
  wide_1mhz centres 1 MHz apart (eight bands over every hertz), the same cells
  bin_step  centres 1 MHz apart, cell_hz = bin_step, SCN_LEVELS_WORDS_MAX / 64 = 2^18 cells (the sweep's first 512 MHz): a unit's
            band covers 3072 cells, the tile 64 -- all but the first 64 bins' cells go straight to a global atomic
Per row (`reps` calls after WARM untimed ones, the slot collected once before them -- a collected slot may be folded any number of times):
  fold_us            scn_plan_update_levels, host clock around the synchronous call (median; fold_min_us: the least)
  fold_kernel_us     its kernel alone (scn_levels_fold_kernel): begin-to-end time of its dispatches from a kernel trace (rocprofv3
                     --kernel-trace) of a SECOND run of the same workload (median); the call figures come from the run without it
  trace_us, trace_kernel_us   (a), the call by the host clock and its kernel (scn_trace_fold_kernel) from the trace
  bins_folded        bins one fold counts (the host form's sum)
  global_atomics     64-bit global atomicAdds one launch issues, counted by restating the kernel's tile on the host for every unit:
                     one per bin whose cell lies outside the unit's tile (direct_atomics) and one per word of the tile that is not 0
                     when the unit is flushed (flush_atomics); lds_atomics = the bins inside the tile
  summary_us, summary_kernel_us   scn_plan_levels_summary for all cells (median of the row's reps), and scn_levels_summary_kernel
  host_route_us      (b): collect with power_db + the host fold, host clock (median of HOST_REPS; collect_us and host_fold_us apart)
Each row carries the build hash (scanner_amd.build.source_hash)."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scanner_amd import Plan, build, capi, synth  # noqa: E402

FS, N, NB = 8000000, 4096, 8192
BS = FS // N
EDGES = 63
TILE_CELLS = 4096 // (EDGES + 1)  # scn_levels.hip: kLevelsTileWords256 / n_levels, a team of 256 at 4096 points
WARM, HOST_REPS = 3, 3
ROWS = (("wide", 6e6, 64 * BS, None), ("wide_1mhz", 1e6, 64 * BS, None), ("bin_step", 1e6, BS, capi.LEVELS_WORDS_MAX // (EDGES + 1)))


def _clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e6, out


def geometry(step, cell_hz, cells):
    centres = 100e6 + step * np.arange(NB)
    f0 = int(centres[0]) - FS // 2
    if cells is None:
        cells = int((centres[-1] + FS // 2 - f0) // cell_hz) + 1
    return centres, f0, cell_hz, min(cells, capi.LEVELS_WORDS_MAX // (EDGES + 1))


def count_atomics(p, edges, centres, f0, cell_hz, cells, dc_ignore=4, use_bandwidth=0.75):
    """(lds, direct, flush) of one launch: scn_levels.hip's tile restated -- the tile of unit u covers the cells from its first
    evaluated bin's (fftshift index i_lo; 0 where that has none) as far as its last one's (i_hi) or TILE_CELLS cells"""
    i = np.arange(N)
    j = (i + N // 2) % N
    use_window = int(use_bandwidth * N / 2.0)
    i_lo, i_hi = N // 2 - use_window, N // 2 + use_window
    ev = ~((j < dc_ignore) | ((N - j) < dc_ignore)) & ~((i < i_lo) | (i > i_hi))
    off = ((np.arange(N + 1, dtype=np.uint64) * np.uint64(BS)) & np.uint64(0xFFFFFFFF)).astype(np.float64)
    none = np.int64(0xFFFFFFFF)
    lds = direct = flush = 0
    for u, fc in enumerate(centres):
        f = np.trunc(fc - float(FS // 2) + off).astype(np.int64).astype(np.uint64)
        on_grid = f >= np.uint64(f0)
        c = (np.where(on_grid, f - np.uint64(f0), np.uint64(0)) // np.uint64(cell_hz)).astype(np.int64)
        c = np.where(on_grid & (c < cells), c, none)
        c0 = 0 if c[i_lo] == none else int(c[i_lo])
        span = int(c[i_hi]) - c0 + 1 if c[i_hi] != none and c0 <= c[i_hi] < c0 + TILE_CELLS else TILE_CELLS
        v = p[u, j]
        ok = ev & ~np.isnan(v) & (c[:N] != none)
        cu, lv = c[:N][ok], np.searchsorted(edges, v[ok], side="right")
        inside = (cu >= c0) & (cu - c0 < span)
        lds += int(inside.sum())
        direct += int((~inside).sum())
        flush += np.unique(cu[inside] * (EDGES + 1) + lv[inside]).size
    return lds, direct, flush


def child(reps):
    import torch

    dev = torch.device("cuda", 0)
    x = synth.cfloat_batch_torch(N, NB, seed=2, device=dev)
    raw = x.view(torch.uint8).reshape(-1)
    with Plan(N, FS, 1e30, flags=capi.OUT_SPECTRUM | capi.OUT_HITS, kind=capi.KIND_FLOAT_COMPLEX, max_batch=NB) as plan:
        for name, step, cell_hz, cells in ROWS:
            centres, f0, cell_hz, cells = geometry(step, cell_hz, cells)
            collect, host = [], []
            for _ in range(HOST_REPS):  # (b): the spectrum over PCIe, then the host form
                plan.submit_device(0, raw, NB, center_freqs=centres, sync_producer=False)
                us, (p, _, _) = _clock(lambda: plan.collect(0, want_hits=False))
                collect.append(us)
                edges = (np.floor(np.median(p[0])) - 31 + np.arange(EDGES)).astype(np.float32)
                h = np.zeros((cells, EDGES + 1), np.uint64)
                host.append(_clock(lambda: capi.levels_fold_spectrum(h, f0, cell_hz, edges, p, FS, centres))[0])
            plan.set_levels(f0, cell_hz, cells, edges)
            plan.set_trace(f0, cell_hz, cells)
            fold = [_clock(lambda: plan.update_levels(0))[0] for _ in range(WARM + reps)][WARM:]
            trace = [_clock(lambda: plan.update_trace(0))[0] for _ in range(WARM + reps)][WARM:]
            summary = [_clock(lambda: plan.levels_summary(500, 32))[0] for _ in range(WARM + reps)][WARM:]
            # the GPU's histogram after WARM + reps folds of one submit: the host's, that many times; its totals: the trace's counts
            got = plan.levels()
            assert np.array_equal(got, h * np.uint64(WARM + reps)), name
            assert np.array_equal(plan.levels_summary(500, 32)[2], plan.trace()[2]), name
            lds, direct, flush = count_atomics(p, edges, centres, f0, cell_hz, cells)
            assert lds + direct == int(h.sum()), name
            row = {"row": name, "n": N, "n_buffers": NB, "centre_step_hz": step, "cell_hz": cell_hz, "cells": cells, "n_edges": EDGES,
                   "first_edge_db": float(edges[0]), "reps": reps, "bins_folded": int(h.sum()), "levels_occupied": int((h.sum(axis=0) != 0).sum()),
                   "fold_us": round(float(np.median(fold)), 1), "fold_min_us": round(min(fold), 1), "bytes_read": 4 * N * NB,
                   "lds_atomics": lds, "direct_atomics": direct, "flush_atomics": flush, "global_atomics": direct + flush,
                   "global_atomics_per_bin": round((direct + flush) / max(1, int(h.sum())), 4),
                   "trace_us": round(float(np.median(trace)), 1), "trace_min_us": round(min(trace), 1),
                   "summary_us": round(float(np.median(summary)), 1),
                   "collect_us": round(float(np.median(collect)), 1), "host_fold_us": round(float(np.median(host)), 1)}
            row["host_route_us"] = round(row["collect_us"] + row["host_fold_us"], 1)
            row["fold_over_trace"] = round(row["fold_us"] / row["trace_us"], 2)
            print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.reps)
    me = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)]
    plain = subprocess.run(me, stdout=subprocess.PIPE, text=True, check=True).stdout
    rows = [json.loads(ln) for ln in plain.splitlines() if ln.startswith("{")]
    for r in rows:
        r["build"] = build.source_hash()
        print(json.dumps(r), flush=True)
    if args.json:  # (the call figures are kept even if the traced run below fails)
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    trace_dir = tempfile.mkdtemp(prefix="levels_bench_")
    names = ("scn_levels_fold_kernel", "scn_trace_fold_kernel", "scn_levels_summary_kernel")
    t = {k: [] for k in names}
    try:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir, "--"] + me, stdout=subprocess.DEVNULL, check=True)
        for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                for k in names:
                    if k in r["Kernel_Name"]:
                        t[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    finally:
        shutil.rmtree(trace_dir, ignore_errors=True)
    per = WARM + args.reps
    ordered = {k: [x[1] for x in sorted(v)] for k, v in t.items()}
    assert len(ordered["scn_levels_fold_kernel"]) == per * len(rows) and len(ordered["scn_trace_fold_kernel"]) == per * len(rows), {k: len(v) for k, v in t.items()}
    assert len(ordered["scn_levels_summary_kernel"]) == (per + 1) * len(rows), len(ordered["scn_levels_summary_kernel"])
    for k, r in enumerate(rows):
        r["fold_kernel_us"] = round(float(np.median(ordered["scn_levels_fold_kernel"][k * per + WARM:(k + 1) * per])) / 1e3, 2)
        r["trace_kernel_us"] = round(float(np.median(ordered["scn_trace_fold_kernel"][k * per + WARM:(k + 1) * per])) / 1e3, 2)
        r["summary_kernel_us"] = round(float(np.median(ordered["scn_levels_summary_kernel"][k * (per + 1) + WARM:k * (per + 1) + per])) / 1e3, 2)
        r["fold_kernel_over_trace_kernel"] = round(r["fold_kernel_us"] / r["trace_kernel_us"], 2)
        r["read_bytes_per_us"] = round(r["bytes_read"] / r["fold_kernel_us"])
        print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
