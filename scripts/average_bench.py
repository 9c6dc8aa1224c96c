"""Rates of averaged plans (scn_plan_desc.average = K > 1, scn_average.hip) on one GPU.

    python scripts/average_bench.py [--steps 50] [--warmup 5] [--json OUT]

For each shape: device-resident inputs rotated over enough batches (>= 1.5 GiB) that no launch finds its input in the
256 MiB Infinity Cache, two slots in flight (submit, then the counts of the slot's previous submit), both on the plan's stream, timed with HIP events around the
whole loop.  Prints input Gsamples/s and the fraction of HBM peak the traffic model implies: K N B_in + 4 N bytes per
group with the spectrum kept (K N B_in for hits only).  The model counts what the definition needs, not the partial
sums the two kernels exchange (8 N bytes per part and group)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scanner_amd import Plan, build, capi, synth  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X: 8.0 TB/s spec
# (n, kind, enob, n_buffers, K, layout, flags)
# K = 1 rows: the plain plan at the same size, format and batch, for comparison
SHAPES = [
    (4096, "cfloat", 0, 8192, 1, capi.AVG_DWELL, capi.OUT_SPECTRUM | capi.OUT_HITS),
    (4096, "cfloat", 0, 8192, 8, capi.AVG_DWELL, capi.OUT_SPECTRUM | capi.OUT_HITS),
    (4096, "cfloat", 0, 8192, 8, capi.AVG_SWEEPS, capi.OUT_SPECTRUM | capi.OUT_HITS),
    (8192, "int16", 12, 4096, 1, capi.AVG_DWELL, capi.OUT_SPECTRUM | capi.OUT_HITS),
    (8192, "int16", 12, 4096, 16, capi.AVG_DWELL, capi.OUT_SPECTRUM | capi.OUT_HITS),
    (4096, "int16", 12, 8192, 1, capi.AVG_DWELL, capi.OUT_SPECTRUM | capi.OUT_HITS),
    (4096, "int16", 12, 4096, 16, capi.AVG_DWELL, capi.OUT_SPECTRUM | capi.OUT_HITS),
    (4096, "int16", 12, 8192, 8192, capi.AVG_DWELL, capi.OUT_SPECTRUM | capi.OUT_HITS),
    (4096, "int16", 12, 8192, 8, capi.AVG_DWELL, capi.OUT_SPECTRUM | capi.OUT_HITS),
    (4096, "cfloat", 0, 8192, 8192, capi.AVG_DWELL, capi.OUT_SPECTRUM | capi.OUT_HITS),
    (4096, "cfloat", 0, 8192, 8, capi.AVG_DWELL, capi.OUT_HITS),
]
KIND = {"cfloat": capi.KIND_FLOAT_COMPLEX, "int16": capi.KIND_SHORT_COMPLEX}


def run_shape(n, kind_name, enob, nb, K, layout, flags, steps, warmup, dev):
    kind = KIND[kind_name]
    bps = capi.BYTES_PER_SAMPLE[kind]
    step_bytes = nb * n * bps
    R = max(2, -(-(3 << 29) // step_bytes))
    raws = []
    for r in range(R):
        x = synth.cfloat_batch_torch(n, nb, seed=7 + r, device=dev)  # float32 [nb, n, 2]
        if kind_name == "int16":
            x = torch.clamp(torch.round(x * 2047.0), -2048, 2047).to(torch.int16).contiguous()
        raws.append(x.view(torch.uint8).reshape(-1))
    G = nb // K
    fc = np.repeat(1e9 + 1e6 * np.arange(G), K) if layout == capi.AVG_DWELL else np.tile(1e9 + 1e6 * np.arange(G), K)
    with Plan(n, 8000000, 10.0, kind=kind, enob=enob or 12, max_batch=nb, average=K, average_layout=layout, flags=flags,
              max_hits=nb * 64) as plan:
        parts = plan.average_parts(nb)
        stream = torch.cuda.ExternalStream(plan.stream_handle, device=dev)
        torch.cuda.synchronize()

        pending = [False, False]

        def step(k):  # two slots in flight: the host's collect of one overlaps the other's launch
            s = k & 1
            if pending[s]:
                plan.collect_counts(s)
            plan.submit_device(s, raws[k % R], nb, fc, sync_producer=False)
            pending[s] = True

        for k in range(warmup):
            step(k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for k in range(steps):
            step(warmup + k)
        e1.record(stream)
        e1.synchronize()
        for s in range(2):
            if pending[s]:
                plan.collect_counts(s)
        us = e0.elapsed_time(e1) * 1e3 / steps
    spec = bool(flags & capi.OUT_SPECTRUM)
    traffic = G * (K * n * bps + (4 * n if spec else 0))
    return {"n": n, "kind": kind_name, "n_buffers": nb, "K": K, "groups": G, "parts": parts,
            "layout": "sweeps" if layout == capi.AVG_SWEEPS else "dwell",
            "mode": "spectrum+hits" if spec else "hits", "us_per_step": round(us, 2),
            "gsamples_per_s": round(nb * n / us / 1e3, 1), "model_bytes": traffic,
            "hbm_frac": round(traffic / us / 1e3 / HBM_PEAK_GBS, 4), "rotating_batches": R}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []
    for shape in SHAPES:
        r = run_shape(*shape, args.steps, args.warmup, dev)
        r["build"] = build.source_hash()
        print(json.dumps(r), flush=True)
        rows.append(r)
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
