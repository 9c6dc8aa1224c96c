"""What the hit history costs (scn_plan_update_history, scn_collect_confirmed; scn_history.hip), beside scn_plan_update_baseline on a
baseline plan of the same shape in the same run -- a kernel that moves a comparable number of bytes.

    python scripts/history_bench.py [--json OUT] [--reps 20]

Shapes (inputs: synth.cfloat_batch_torch, seed 2, quantised for the integer kind; those of scripts/baseline_bench.py):
  c2        8192 x 4096 cfloat        int16     4096 x 8192 int16        small     262144 x 128 cfloat
each with a history of a row per unit, at three hit densities, all hits-only plans:
  none      a fixed plan with threshold 1e30: no hits, the fold shifts in zeros
  half      a floor plan with threshold 0: the evaluated bins above each unit's median
  full      a fixed plan with threshold -1e30: every evaluated bin, the regions are full
Per row (one repetition = submit, collect the counts, then the calls below; `reps` repetitions after WARM untimed ones):
  fold_us            scn_plan_update_history, host clock around the synchronous call (median; fold_min_us: the least)
  fold_kernel_us     its kernel alone (scn_history_fold_kernel): begin-to-end time of its dispatches from a kernel trace (rocprofv3
                     --kernel-trace) of a SECOND run of the same workload (median); the call figures come from the run without it
  fold_bytes         8 bytes per bin and unit (the word read and written) + 8 per stored hit; fold_bytes_per_us = over fold_kernel_us
  count_us           scn_collect_confirmed(m 2, window 2) with cap 0 -- the count kernel, the scan, the total's copy -- host clock; the
                     slot's ordered list is built by an untimed call before it
  window_us          the same call with room for the first min(total, 2^20) records: count, scan, build, and the records' copy
  count_kernel_us, build_kernel_us   the two kernels alone, from the trace (the build: of that window)
  update_us, update_kernel_us        the yardstick: scn_plan_update_baseline(SCN_BASELINE_MAX) on a baseline plan of the same shape
                     (spectrum + hits, a row per unit), the call by the host clock (median of UPDATES) and its kernel from the trace
  fold_over_update, fold_kernel_over_update_kernel   the ratios
Each row carries the build hash (scanner_amd.build.source_hash)."""
import argparse
import csv
import ctypes as C
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

FS = 8000000
SHAPES = (("c2", 4096, 8192, capi.KIND_FLOAT_COMPLEX), ("int16", 8192, 4096, capi.KIND_SHORT_COMPLEX), ("small", 128, 262144, capi.KIND_FLOAT_COMPLEX))
DENSITIES = (("none", dict(threshold=1e30)), ("half", dict(threshold=0.0, detect=capi.DETECT_FLOOR)), ("full", dict(threshold=-1e30)))
WARM, UPDATES, WINDOW = 3, 10, 1 << 20
M, N_OF = 2, 2


def _clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e6, out


def child(reps):
    """prints one JSON line per (shape, density).  Dispatches, in the order of the rows: per row (WARM + reps) folds and, where there
    are hits, 3 x (WARM + reps - 1) count kernels and (WARM + reps - 1) build kernels (the first repetition only folds); per shape,
    before its rows, UPDATES baseline updates -- what the parent's walk of the trace relies on.  The input is the same in every
    repetition, so from the second visit on every hit is confirmed at (2, 2): the build kernel ranks whole units."""
    import torch

    dev = torch.device("cuda", 0)
    for shape, n, nb, kind in SHAPES:
        x = synth.cfloat_batch_torch(n, nb, seed=2, device=dev)
        if kind != capi.KIND_FLOAT_COMPLEX:
            x = torch.from_numpy(synth.quantize(x.cpu().numpy().view(np.complex64).reshape(nb, n), kind)).to(dev)
        raw = x.view(torch.uint8).reshape(-1)
        kw = dict(kind=kind, enob=12, max_batch=nb)
        with Plan(n, FS, 0.0, flags=capi.OUT_SPECTRUM | capi.OUT_HITS, detect=capi.DETECT_BASELINE, baseline=nb, **kw) as plan:
            plan.submit_device(0, raw, nb)
            plan.collect_counts(0)
            upd = [_clock(lambda: plan.update_baseline(0, capi.BASELINE_MAX))[0] for _ in range(UPDATES)]
        for density, how in DENSITIES:
            with Plan(n, FS, flags=capi.OUT_HITS, **how, **kw) as plan:
                plan.set_history(nb)
                total, out = C.c_uint32(), np.zeros(WINDOW, capi.HIT_DTYPE)
                confirm = lambda cap: plan._L.scn_collect_confirmed(plan.handle, 0, M, N_OF, 0, out.ctypes.data_as(C.c_void_p), cap, C.byref(total))  # noqa: E731
                fold, count, window, hits = [], [], [], 0
                for rep in range(WARM + reps):
                    plan.submit_device(0, raw, nb, sync_producer=False)
                    hits = plan.collect_counts(0)
                    fold.append(_clock(lambda: plan.update_history(0))[0])
                    if rep == 0:  # (a first visit confirms nothing at (2, 2): no build kernel would run)
                        count.append(0.0)
                        window.append(0.0)
                        continue
                    st = confirm(0)  # (untimed: builds the slot's ordered list, whose scan the confirm kernels read)
                    assert st in (capi.OK, capi.E_TRUNCATED), st
                    count.append(_clock(lambda: confirm(0))[0])
                    us, st = _clock(lambda: confirm(WINDOW))
                    assert st in (capi.OK, capi.E_TRUNCATED), st
                    window.append(us)
                fold, count, window = fold[WARM:], count[WARM:], window[WARM:]
            fold_bytes = 8 * n * nb + 8 * hits
            row = {"shape": shape, "n": n, "n_buffers": nb, "kind": kind, "density": density, "hits_per_step": hits, "confirmed": total.value,
                   "reps": reps, "fold_us": round(float(np.median(fold)), 1), "fold_min_us": round(min(fold), 1), "fold_bytes": fold_bytes,
                   "count_us": round(float(np.median(count)), 1), "count_min_us": round(min(count), 1),
                   "window_us": round(float(np.median(window)), 1), "window_min_us": round(min(window), 1), "window_records": min(total.value, WINDOW),
                   "update_us": round(float(np.median(upd)), 1), "update_min_us": round(min(upd), 1)}
            row["fold_over_update"] = round(row["fold_us"] / row["update_us"], 2)
            print(json.dumps(row), flush=True)
        del x, raw
        torch.cuda.empty_cache()


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
    trace_dir = tempfile.mkdtemp(prefix="history_trace_")
    names = ("scn_history_fold_kernel", "scn_confirm_count_kernel", "scn_confirm_build_kernel", "scn_baseline_update_kernel")
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
    pos = {k: 0 for k in names}

    def take(k, count, skip=0):
        """median us of the next `count` dispatches of kernel k, the first `skip` of them left out"""
        got = [x[1] for x in sorted(t[k])[pos[k]:pos[k] + count]]
        assert len(got) == count, (k, pos[k], count, len(t[k]))
        pos[k] += count
        return round(float(np.median(got[skip:])) / 1e3, 2)

    per = WARM + args.reps
    for shape, _, _, _ in SHAPES:
        update_kernel_us = take("scn_baseline_update_kernel", UPDATES)
        for r in (r for r in rows if r["shape"] == shape):
            r["update_kernel_us"] = update_kernel_us
            r["fold_kernel_us"] = take("scn_history_fold_kernel", per, WARM)
            r["fold_bytes_per_us"] = round(r["fold_bytes"] / r["fold_kernel_us"])
            r["fold_kernel_over_update_kernel"] = round(r["fold_kernel_us"] / update_kernel_us, 2)
            if r["hits_per_step"]:
                r["count_kernel_us"] = take("scn_confirm_count_kernel", 3 * (per - 1), 3 * (WARM - 1))
                r["build_kernel_us"] = take("scn_confirm_build_kernel", per - 1, WARM - 1)
    assert all(pos[k] == len(t[k]) for k in names), (pos, {k: len(v) for k, v in t.items()})
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
