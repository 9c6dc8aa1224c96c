"""What the floor detector costs (scn_plan_desc.detect = SCN_DETECT_FLOOR, scn_floor.hip; with a floor window: scn_floor_local.hip)
beside the fixed-threshold plan of the same build, in the same loop.

    python scripts/floor_bench.py [--json OUT] [--steps 60]

Shapes (inputs: synth.cfloat_batch_torch, seed 2, quantised for the integer kind):
  c2        8192 x 4096 cfloat   fixed and floor plans with spectrum + hits, and a hits-only floor plan
  int16     4096 x 8192 int16    fixed and floor, spectrum + hits
  small     262144 x 128 cfloat  fixed and floor, spectrum + hits
The fixed plan's threshold is the bench's 10 dB (the other shapes: 8 above their spectrum's median); the floor plan's offset is that
threshold less the median of the shape's spectrum, so both cut at about the same level and report about as many hits.
Every shape also runs the floor plan under the floor windows (16, 2) and (128, 64) (scn_plan_set_floor_window; rows floor_w16_2 and
floor_w128_64, same offset) where the window is valid -- at 128 points (128, 64) leaves bins without a reference cell and has no row.
Per row:
  step_us       us per step of a two-slot loop (submit slot k, collect the counts of slot k ^ 1), host clock over `steps` steps;
                the plans of a shape take turns, round by round, and the median of the rounds is reported
  over_fixed    step_us / the fixed plan's step_us of the same shape
  detect_us     the detect kernel alone (scn_floor_kernel, or scn_floor_local_kernel under a window): begin-to-end time of its
                dispatches from a kernel trace (rocprofv3 --kernel-trace) of a second run of the same workload (median); the step
                figures come from the run WITHOUT the profiler
  over_unit_wide  windowed rows: detect_us / the detect_us of the shape's unit-wide `floor` row
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

FS = 8000000
BOTH = capi.OUT_SPECTRUM | capi.OUT_HITS
SHAPES = (("c2", 4096, 8192, capi.KIND_FLOAT_COMPLEX), ("int16", 8192, 4096, capi.KIND_SHORT_COMPLEX), ("small", 128, 262144, capi.KIND_FLOAT_COMPLEX))
WINDOWS = ((16, 2), (128, 64))
ROUNDS, WARM = 5, 8


def _loop(plan, raw, nb, steps):
    """us per step of the two-slot loop"""
    ptr = raw.data_ptr()
    fc = np.zeros(nb, np.float64)
    fcp = fc.ctypes.data
    for k in range(2):
        plan.submit_prepared(k, ptr, nb, fcp, None, None)
    for s in range(WARM):
        plan.collect_counts(s & 1)
        plan.submit_prepared(s & 1, ptr, nb, fcp, None, None)
    t0 = time.perf_counter()
    for s in range(steps):
        plan.collect_counts(s & 1)
        plan.submit_prepared(s & 1, ptr, nb, fcp, None, None)
    dt = time.perf_counter() - t0
    hits = [plan.collect_counts(k) for k in range(2)]
    return dt / steps * 1e6, hits[0]


def child(steps):
    """prints one JSON line per (shape, plan).  Floor-kernel dispatches per floor plan: ROUNDS x (2 + WARM + steps), in the order
    of the rows -- what the parent's walk of the trace relies on."""
    import torch

    dev = torch.device("cuda", 0)
    for shape, n, nb, kind in SHAPES:
        x = synth.cfloat_batch_torch(n, nb, seed=2, device=dev)
        if kind != capi.KIND_FLOAT_COMPLEX:
            x = torch.from_numpy(synth.quantize(x.cpu().numpy().view(np.complex64).reshape(nb, n), kind)).to(dev)
        raw = x.view(torch.uint8).reshape(-1)
        kw = dict(kind=kind, enob=12, max_batch=nb)
        with Plan(n, FS, 1e9, flags=capi.OUT_SPECTRUM, **kw) as plan:
            plan.submit_device(0, raw, nb)
            med = float(np.median(plan.collect(0)[0][:64]))
        thr = 10.0 if shape == "c2" else med + 8.0  # (the C2 input's median is about 2.8: the bench's threshold lies 7 above it)
        offset = thr - med
        plans = [("fixed", dict(flags=BOTH), thr), ("floor", dict(flags=BOTH, detect=capi.DETECT_FLOOR), offset)]
        if shape == "c2":
            plans.append(("floor_hits_only", dict(flags=capi.OUT_HITS, detect=capi.DETECT_FLOOR), offset))
        open_plans = [(name, Plan(n, FS, t, **k, **kw)) for name, k, t in plans]
        for train, guard in WINDOWS:
            try:
                open_plans.append((f"floor_w{train}_{guard}", Plan(n, FS, offset, flags=BOTH, detect=capi.DETECT_FLOOR, floor_window=(train, guard), **kw)))
            except capi.ScannerError as e:  # (a window that leaves an evaluated bin of this size without a cell)
                if e.status != capi.E_INVALID:
                    raise
        us = {name: [] for name, _ in open_plans}
        hits = {}
        for _ in range(ROUNDS):
            for name, plan in open_plans:
                u, hits[name] = _loop(plan, raw, nb, steps)
                us[name].append(u)
        for name, plan in open_plans:
            plan.close()
        fixed = float(np.median(us["fixed"]))
        for name, _ in open_plans:
            m = float(np.median(us[name]))
            print(json.dumps({"shape": shape, "n": n, "n_buffers": nb, "kind": kind, "plan": name, "median_db": round(med, 2),
                              "threshold": round(thr if name == "fixed" else offset, 2), "hits_per_step": hits[name], "steps": steps,
                              "step_us": round(m, 1), "step_min_us": round(min(us[name]), 1), "over_fixed": round(m / fixed, 3)}), flush=True)
        del x, raw
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.steps)
    me = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps)]
    plain = subprocess.run(me, stdout=subprocess.PIPE, text=True, check=True).stdout
    rows = [json.loads(ln) for ln in plain.splitlines() if ln.startswith("{")]
    trace_dir = tempfile.mkdtemp(prefix="floor_trace_")
    try:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir, "--"] + me, stdout=subprocess.DEVNULL,
                       check=True)
        t = []
        for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                if "scn_floor_kernel" in r["Kernel_Name"] or "scn_floor_local_kernel" in r["Kernel_Name"]:
                    t.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    finally:
        shutil.rmtree(trace_dir, ignore_errors=True)
    t.sort()
    per = 2 + WARM + args.steps  # dispatches per plan and round
    pos = 0
    for shape, _, _, _ in SHAPES:
        floor_rows = [r for r in rows if r["shape"] == shape and r["plan"] != "fixed"]
        d = {r["plan"]: [] for r in floor_rows}
        for _ in range(ROUNDS):
            for r in floor_rows:
                d[r["plan"]] += [x[1] for x in t[pos:pos + per]]
                pos += per
        for r in floor_rows:
            assert len(d[r["plan"]]) == ROUNDS * per, (shape, r["plan"], len(d[r["plan"]]))
            r["detect_us"] = round(float(np.median(d[r["plan"]])) / 1e3, 2)
        unit_wide = next(r["detect_us"] for r in floor_rows if r["plan"] == "floor")
        for r in floor_rows:
            if r["plan"].startswith("floor_w"):
                r["over_unit_wide"] = round(r["detect_us"] / unit_wide, 2)
    assert pos == len(t), (pos, len(t))
    for r in rows:
        r["build"] = build.source_hash()
        print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
