"""What the sweep trace's fold costs (scn_plan_update_trace; scn_trace.hip) on a C2-shaped plan -- 8192 buffers of 4096 cfloat points,
spectrum + hits -- beside the two things it stands next to, on the same collected submit and in the same run:
  (a) scn_plan_update_baseline(SCN_BASELINE_MAX) on a baseline plan of the same shape: it reads the same 128 MiB and writes 128 MiB;
  (b) the host route the fold replaces: scn_collect with power_db (128 MiB over PCIe) plus scn_trace_fold_spectrum on the host.

    python scripts/trace_bench.py [--json OUT] [--reps 20]

Rows (inputs: synth.cfloat_batch_torch, seed 2; a fixed threshold nothing exceeds, so no hit list is built):
  wide      centres 6 MHz apart (adjacent bands touch), cell_hz = 64 bin_step: a wave's 256 bins of one load span about four cells
  wide_1mhz centres 1 MHz apart (eight bands over every hertz), the same cells: more units per cell
  bin_step  centres 1 MHz apart, cell_hz = bin_step, 2^22 cells (the sweep's 8.2 GHz fit): the worst case, a triple per evaluated bin
Per row (`reps` calls after WARM untimed ones, the slot collected once before them -- a collected slot may be folded any number of times):
  fold_us          scn_plan_update_trace, host clock around the synchronous call (median; fold_min_us: the least)
  fold_kernel_us   its kernel alone (scn_trace_fold_kernel): begin-to-end time of its dispatches from a kernel trace (rocprofv3
                   --kernel-trace) of a SECOND run of the same workload (median); the call figures come from the run without it
  bytes_read       4 bytes per bin and unit: the spectrum, once
  triples          atomic triples (atomicMax + atomicMin + 64-bit atomicAdd) the launch issues, counted by restating the kernel's runs
                   on the host for every unit: a triple per stretch of equal cell among the 256 consecutive bins of a wave and load;
                   triples_per_wave_load = over the 16 wave-loads of a unit (4 waves x 4 loads at 4096 points)
  update_us, update_kernel_us   (a), the call by the host clock (median of UPDATES) and its kernel from the trace
  host_route_us    (b): collect with power_db + the host fold, host clock (median of HOST_REPS; collect_us and host_fold_us apart)
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
WARM, UPDATES, HOST_REPS = 3, 10, 3
ROWS = (("wide", 6e6, 64 * BS, None), ("wide_1mhz", 1e6, 64 * BS, None), ("bin_step", 1e6, BS, capi.TRACE_CELLS_MAX))


def _clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e6, out


def geometry(step, cell_hz, cells):
    centres = 100e6 + step * np.arange(NB)
    f0 = int(centres[0]) - FS // 2
    if cells is None:
        cells = int((centres[-1] + FS // 2 - f0) // cell_hz) + 1
    return centres, f0, cell_hz, cells


def count_triples(centres, f0, cell_hz, cells, dc_ignore=4, use_bandwidth=0.75):
    """the atomic triples of one launch: scn_trace.hip's runs restated -- team of 256, 16-byte loads: load k, thread t holds natural
    bins 4 (t + 256 k) ... + 3, so a wave and load cover 256 consecutive bins: a triple per stretch of equal cell among them"""
    j = np.arange(N)
    i = (j + N - N // 2) % N
    use_window = int(use_bandwidth * N / 2.0)
    ev = ~((j < dc_ignore) | ((N - j) < dc_ignore)) & ~((i < N // 2 - use_window) | (i > N // 2 + use_window))
    off = ((i.astype(np.uint64) * np.uint64(BS)) & np.uint64(0xFFFFFFFF)).astype(np.float64)
    total = 0
    for fc in centres:
        f = np.trunc(fc - float(FS // 2) + off).astype(np.int64).astype(np.uint64)
        ok = ev & (f >= np.uint64(f0))
        c = np.where(ok, (f - np.uint64(f0)) // np.uint64(cell_hz), np.uint64(0xFFFFFFFF))
        c = np.where(c < np.uint64(cells), c, np.uint64(0xFFFFFFFF)).astype(np.int64).reshape(-1, 256)  # [wave-load, bin]
        head = np.concatenate([np.ones((len(c), 1), bool), c[:, 1:] != c[:, :-1]], axis=1)
        total += int((head & (c != 0xFFFFFFFF)).sum())
    return total


def child(reps):
    import torch

    dev = torch.device("cuda", 0)
    x = synth.cfloat_batch_torch(N, NB, seed=2, device=dev)
    raw = x.view(torch.uint8).reshape(-1)
    kw = dict(kind=capi.KIND_FLOAT_COMPLEX, max_batch=NB)
    with Plan(N, FS, 0.0, flags=capi.OUT_SPECTRUM | capi.OUT_HITS, detect=capi.DETECT_BASELINE, baseline=NB, **kw) as plan:
        plan.submit_device(0, raw, NB)
        plan.collect_counts(0)
        upd = [_clock(lambda: plan.update_baseline(0, capi.BASELINE_MAX))[0] for _ in range(UPDATES)]
    with Plan(N, FS, 1e30, flags=capi.OUT_SPECTRUM | capi.OUT_HITS, **kw) as plan:
        for name, step, cell_hz, cells in ROWS:
            centres, f0, cell_hz, cells = geometry(step, cell_hz, cells)
            plan.submit_device(0, raw, NB, center_freqs=centres, sync_producer=False)
            plan.collect_counts(0)
            plan.set_trace(f0, cell_hz, cells)
            fold = [_clock(lambda: plan.update_trace(0))[0] for _ in range(WARM + reps)][WARM:]
            got = plan.trace()
            collect, host = [], []
            for _ in range(HOST_REPS):  # (b): the spectrum over PCIe, then the host form
                plan.submit_device(0, raw, NB, center_freqs=centres, sync_producer=False)
                us, (p, _, _) = _clock(lambda: plan.collect(0, want_hits=False))
                collect.append(us)
                t = capi.trace_init(cells)
                host.append(_clock(lambda: capi.trace_fold_spectrum(t, f0, cell_hz, p, FS, centres))[0])
            # the GPU's trace after WARM + reps folds of one submit: the host's maxima and minima, its counts that many times
            assert got[0].tobytes() == t[0].tobytes() and got[1].tobytes() == t[1].tobytes() and np.array_equal(got[2], t[2] * np.uint64(WARM + reps)), name
            triples = count_triples(centres, f0, cell_hz, cells)
            row = {"row": name, "n": N, "n_buffers": NB, "centre_step_hz": step, "cell_hz": cell_hz, "cells": cells, "reps": reps,
                   "bins_folded": int(t[2].sum()), "fold_us": round(float(np.median(fold)), 1), "fold_min_us": round(min(fold), 1),
                   "bytes_read": 4 * N * NB, "triples": triples, "triples_per_wave_load": round(triples / (16.0 * NB), 2),
                   "update_us": round(float(np.median(upd)), 1), "update_min_us": round(min(upd), 1),
                   "collect_us": round(float(np.median(collect)), 1), "host_fold_us": round(float(np.median(host)), 1)}
            row["host_route_us"] = round(row["collect_us"] + row["host_fold_us"], 1)
            row["fold_over_update"] = round(row["fold_us"] / row["update_us"], 2)
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
    if args.json:  # (the call figures are kept even if the traced run below fails)
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    trace_dir = tempfile.mkdtemp(prefix="trace_bench_")
    names = ("scn_trace_fold_kernel", "scn_baseline_update_kernel")
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
    folds = [x[1] for x in sorted(t["scn_trace_fold_kernel"])]
    updates = [x[1] for x in sorted(t["scn_baseline_update_kernel"])]
    assert len(folds) == per * len(rows) and len(updates) == UPDATES, (len(folds), len(updates))
    for k, r in enumerate(rows):
        r["fold_kernel_us"] = round(float(np.median(folds[k * per + WARM:(k + 1) * per])) / 1e3, 2)
        r["update_kernel_us"] = round(float(np.median(updates)) / 1e3, 2)
        r["fold_kernel_over_update_kernel"] = round(r["fold_kernel_us"] / r["update_kernel_us"], 2)
        r["read_bytes_per_us"] = round(r["bytes_read"] / r["fold_kernel_us"])
        print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
