"""What the baseline detector costs (scn_plan_desc.detect = SCN_DETECT_BASELINE, scn_baseline.hip) beside the fixed-threshold plan of
the same build, in the same loop, and beside a plain copy of the bytes its detect kernel has to read.

    python scripts/baseline_bench.py [--json OUT] [--steps 60]

Shapes (inputs: synth.cfloat_batch_torch, seed 2, quantised for the integer kind; those of scripts/floor_bench.py):
  c2        8192 x 4096 cfloat   fixed and baseline plans with spectrum + hits, and a hits-only baseline plan
  int16     4096 x 8192 int16    fixed and baseline, spectrum + hits
  small     262144 x 128 cfloat  fixed and baseline, spectrum + hits
The fixed plan's threshold is the bench's 10 dB (the other shapes: 8 above their spectrum's median).  The baseline has a row per
unit, every entry the median of the shape's spectrum, and the plan's offset is that threshold less the median: a baseline a few dB
over the noise, both plans cut at the same level and report the same hits, which are rare.
Per row:
  step_us       us per step of a two-slot loop (submit slot k, collect the counts of slot k ^ 1), host clock over `steps` steps;
                the plans of a shape take turns, round by round, and the median of the rounds is reported
  over_fixed    step_us / the fixed plan's step_us of the same shape
  detect_us     the detect kernel alone (scn_baseline_kernel): begin-to-end time of its dispatches from a kernel trace (rocprofv3
                --kernel-trace) of a second run of the same workload (median); the step figures come from the run WITHOUT the profiler
  copy_us       a device-to-device copy of read_bytes = 2 * 4 * n * units bytes, the two rows per unit the detect kernel must read
                (median of 20, device events, in the same process as the step figures): the yardstick for detect_us
  update_us     one scn_plan_update_baseline(SCN_BASELINE_MAX) of a collected slot, host clock around the synchronous call (median
                of 10); update_kernel_us: its kernel alone, from the same trace
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
ROUNDS, WARM, UPDATES = 5, 8, 10


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


def _copy_us(torch, dev, nbytes):
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    src.zero_()
    us = []
    for _ in range(24):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return float(np.median(us[4:]))


def child(steps):
    """prints one JSON line per (shape, plan).  Detect-kernel dispatches per baseline plan: ROUNDS x (2 + WARM + steps), in the order
    of the rows, and UPDATES update-kernel dispatches per shape -- what the parent's walk of the trace relies on."""
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
        rows = np.full((nb, n), med, np.float32)  # a row per unit
        plans = [("fixed", dict(flags=BOTH), thr), ("baseline", dict(flags=BOTH, detect=capi.DETECT_BASELINE, baseline=rows), offset)]
        if shape == "c2":
            plans.append(("baseline_hits_only", dict(flags=capi.OUT_HITS, detect=capi.DETECT_BASELINE, baseline=rows), offset))
        open_plans = [(name, Plan(n, FS, t, **k, **kw)) for name, k, t in plans]
        del rows
        us = {name: [] for name, _ in open_plans}
        hits = {}
        for _ in range(ROUNDS):
            for name, plan in open_plans:
                u, hits[name] = _loop(plan, raw, nb, steps)
                us[name].append(u)
        upd = []
        plan = dict(open_plans)["baseline"]  # (both slots collected: the loop's last step)
        for _ in range(UPDATES):
            t0 = time.perf_counter()
            plan.update_baseline(0, capi.BASELINE_MAX)
            upd.append((time.perf_counter() - t0) * 1e6)
        for name, plan in open_plans:
            plan.close()
        read_bytes = 2 * 4 * n * nb
        copy_us = _copy_us(torch, dev, read_bytes)
        fixed = float(np.median(us["fixed"]))
        for name, _ in open_plans:
            m = float(np.median(us[name]))
            row = {"shape": shape, "n": n, "n_buffers": nb, "kind": kind, "plan": name, "median_db": round(med, 2),
                   "threshold": round(thr if name == "fixed" else offset, 2), "hits_per_step": hits[name], "steps": steps,
                   "step_us": round(m, 1), "step_min_us": round(min(us[name]), 1), "over_fixed": round(m / fixed, 3)}
            if name != "fixed":
                row.update(read_bytes=read_bytes, copy_us=round(copy_us, 2))
            if name == "baseline":
                row.update(update_us=round(float(np.median(upd)), 1))
            print(json.dumps(row), flush=True)
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
    if args.json:  # (the step figures are kept even if the traced run below fails)
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    trace_dir = tempfile.mkdtemp(prefix="baseline_trace_")
    try:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir, "--"] + me, stdout=subprocess.DEVNULL,
                       check=True)
        t, tu = [], []
        for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                rec = (int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
                if "scn_baseline_update_kernel" in r["Kernel_Name"]:
                    tu.append(rec)
                elif "scn_baseline_kernel" in r["Kernel_Name"]:
                    t.append(rec)
    finally:
        shutil.rmtree(trace_dir, ignore_errors=True)
    t.sort()
    tu.sort()
    per = 2 + WARM + args.steps  # dispatches per plan and round
    pos = 0
    assert len(tu) == UPDATES * len(SHAPES), len(tu)
    for k, (shape, _, _, _) in enumerate(SHAPES):
        base_rows = [r for r in rows if r["shape"] == shape and r["plan"] != "fixed"]
        d = {r["plan"]: [] for r in base_rows}
        for _ in range(ROUNDS):
            for r in base_rows:
                d[r["plan"]] += [x[1] for x in t[pos:pos + per]]
                pos += per
        for r in base_rows:
            assert len(d[r["plan"]]) == ROUNDS * per, (shape, r["plan"], len(d[r["plan"]]))
            r["detect_us"] = round(float(np.median(d[r["plan"]])) / 1e3, 2)
            r["detect_over_copy"] = round(r["detect_us"] / r["copy_us"], 2)
            if r["plan"] == "baseline":
                r["update_kernel_us"] = round(float(np.median([x[1] for x in tu[k * UPDATES:(k + 1) * UPDATES]])) / 1e3, 2)
    assert pos == len(t), (pos, len(t))
    for r in rows:
        r["build"] = build.source_hash()
        print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
