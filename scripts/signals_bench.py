"""What merging hits into signals on the GPU costs (scn_collect_signals, scn_hits.hip), beside the compaction of the same submit.

    python scripts/signals_bench.py [--json OUT] [--reps 20]

Two shapes of 8192 x 4096-point cfloat buffers, both on the bench's own inputs (synth.cfloat_batch_torch, seed 2): `c2` with the
bench's threshold (10 dB: a few hits per buffer) and `dense` with the threshold at the spectrum's median (every other evaluated
bin a hit).
For max_gap 0 and 8 each:
  e2e_us        one scn_collect_signals call that returns every record, host clock around the call (it ends in a stream
                synchronise): count kernel, scan, the total's read-back, build kernel, the records' copy into pageable memory
  total_only_us the same call with cap 0: count kernel, scan, read-back
  count_us / scan_us / build_us   the three kernels alone, and compact_us, scn_hit_compact_kernel writing the whole ordered hit
                list of the same submit in the same process: begin-to-end times of the dispatches from a kernel trace
                (rocprofv3 --kernel-trace) of a second run of the same workload -- the side stream the library queues them on is
                its own, so no caller can put stream events around them; the end-to-end figures come from the run WITHOUT the
                profiler
  kernels_over_compact            (count + scan + build) / compact
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

N, NB, FS = 4096, 8192, 8000000
GAPS = (0, 8)
SUBMITS, WARM = 6, 2  # submits per shape (each builds the ordered hit list once); untimed signal calls per gap
KERNELS = ("scn_signal_count_kernel", "scn_hit_scan_kernel", "scn_signal_build_kernel", "scn_hit_compact_kernel")


def child(reps):
    """the workload; prints one JSON line per (shape, max_gap).  The order of the dispatches is what the parent relies on: per
    shape SUBMITS x (scan, compact), then per gap (WARM + reps) x (count, scan, build), the last `reps` of them timed."""
    import torch

    dev = torch.device("cuda", 0)
    L = capi.lib()
    x = synth.cfloat_batch_torch(N, NB, seed=2, device=dev)
    raw = x.view(torch.uint8).reshape(-1)
    for shape in ("c2", "dense"):
        thr = 10.0
        if shape == "dense":
            with Plan(N, FS, 1e9, max_batch=NB, flags=capi.OUT_SPECTRUM) as plan:
                plan.submit_device(0, raw, NB)
                thr = float(np.median(plan.collect(0)[0]))
        with Plan(N, FS, thr, max_batch=NB, max_hits=NB * 2048) as plan:  # room for every record: the compaction writes them all
            for _ in range(SUBMITS):
                plan.submit_device(0, raw, NB)
                hits = plan.collect_counts(0)
                assert 0 < hits <= NB * 2048, hits
                plan.collect_more(0, 0, 1)  # builds the whole ordered list on the device (scan + compaction), copies one record
            n_sig = C.c_uint32()
            for gap in GAPS:
                st = L.scn_collect_signals(plan.handle, 0, gap, 0, None, 0, C.byref(n_sig))
                assert st in (capi.OK, capi.E_TRUNCATED), st
                total = n_sig.value
                out = np.zeros(max(total, 1), capi.SIGNAL_DTYPE)
                e2e, only = [], []
                for k in range(WARM + reps):
                    t0 = time.perf_counter()
                    st = L.scn_collect_signals(plan.handle, 0, gap, 0, out.ctypes.data_as(C.c_void_p), total, C.byref(n_sig))
                    t1 = time.perf_counter()
                    assert st == capi.OK and n_sig.value == total, (st, n_sig.value, total)
                    if k >= WARM:
                        e2e.append((t1 - t0) * 1e6)
                assert int(out["n_hits"][:total].sum()) == hits  # every hit is in exactly one signal
                # (the count-only calls last: the parent's walk of the trace skips them, they launch no build kernel)
                for k in range(reps):
                    t0 = time.perf_counter()
                    L.scn_collect_signals(plan.handle, 0, gap, 0, None, 0, C.byref(n_sig))
                    only.append((time.perf_counter() - t0) * 1e6)
                print(json.dumps({"shape": shape, "n": N, "n_buffers": NB, "threshold_db": round(thr, 3), "max_gap": gap, "hits": hits,
                                  "signals": total, "reps": reps, "e2e_us": round(float(np.median(e2e)), 1),
                                  "e2e_min_us": round(min(e2e), 1), "total_only_us": round(float(np.median(only)), 1)}), flush=True)
        torch.cuda.empty_cache()


def kernel_times(trace_dir):
    """begin-to-end ns of every dispatch of KERNELS, per kernel in start order"""
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), k, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    return {k: [d for _, kk, d in rows if kk == k] for k in KERNELS}


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
    trace_dir = tempfile.mkdtemp(prefix="signals_trace_")
    try:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir, "--"] + me, stdout=subprocess.DEVNULL,
                       check=True)
        t = kernel_times(trace_dir)
    finally:
        shutil.rmtree(trace_dir, ignore_errors=True)
    med = lambda d: round(float(np.median(d)) / 1e3, 2)  # noqa: E731
    pos = dict.fromkeys(KERNELS, 0)

    def take(kernel, count):
        d = t[kernel][pos[kernel]:pos[kernel] + count]
        assert len(d) == count, (kernel, pos[kernel], count, len(t[kernel]))
        pos[kernel] += count
        return d

    per = WARM + args.reps
    for shape in ("c2", "dense"):
        # (the dense shape's first plan, spectrum only, launches none of these kernels)
        take("scn_hit_scan_kernel", SUBMITS)
        compact = med(take("scn_hit_compact_kernel", SUBMITS)[1:])
        for row in (r for r in rows if r["shape"] == shape):
            # one count-only call, the timed calls, then `reps` more count-only calls: count and scan 1 + per + reps, build per
            count = take("scn_signal_count_kernel", 1 + per + args.reps)[1 + WARM:1 + per]
            scan = take("scn_hit_scan_kernel", 1 + per + args.reps)[1 + WARM:1 + per]
            built = take("scn_signal_build_kernel", per if row["signals"] else 0)[WARM:]
            row.update(count_us=med(count), scan_us=med(scan), build_us=med(built) if built else 0.0, compact_us=compact)
            row["kernels_over_compact"] = round((row["count_us"] + row["scan_us"] + row["build_us"]) / compact, 2)
            row["build"] = build.source_hash()
            print(json.dumps(row), flush=True)
    assert all(pos[k] == len(t[k]) for k in KERNELS), (pos, {k: len(v) for k, v in t.items()})
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
