"""Seeded parity fuzz of the averaged kernels (scn_average.hip) against a float64 evaluation, per size.

    python scripts/average_fuzz.py [--trials 40] [--sizes 1024,2048,4096,8192]

Each trial: G groups of K buffers (K drawn from {2, 3, 4, 8}, G such that both the P = 1 route and the split route occur),
cfloat or int16 (ENOB 12, no DC removal: its conversion is exact, so the float64 reference is x * 2^-11), noise plus up to
four tones with a gain per buffer.  The figure is tests/tolerances.py's max |P - P_ref| / max(P_ref, mean P_ref) over all
bins; the bar is 1e-5 and the margin is 1 - worst / 1e-5."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scanner_amd import Plan, build, capi, synth  # noqa: E402

BAR = 1e-5


def figure(db, P_ref):
    P = np.power(10.0, db.astype(np.float64) / 5.0)
    mean = P_ref.mean(axis=-1, keepdims=True)
    return float((np.abs(P - P_ref) / np.maximum(P_ref, mean)).max())


def trial(n, seed, dev):
    rng = np.random.default_rng(seed)
    K = int(rng.choice([2, 3, 4, 8]))
    G = int(rng.choice([1, 2, 5, 40]))
    kind = capi.KIND_SHORT_COMPLEX if rng.integers(2) else capi.KIND_FLOAT_COMPLEX
    x = synth.cfloat_batch(n, G * K, seed=seed, sigma=float(rng.uniform(0.01, 0.1)))
    x *= rng.uniform(0.3, 1.0, size=(G * K, 1)).astype(np.float32)
    raw = synth.quantize(x, kind)
    x64 = raw.astype(np.float64) / 2048.0 if kind != capi.KIND_FLOAT_COMPLEX else x.astype(np.complex128)
    if kind != capi.KIND_FLOAT_COMPLEX:
        x64 = x64[..., 0] + 1j * x64[..., 1]
    layout = capi.AVG_SWEEPS if rng.integers(2) else capi.AVG_DWELL
    with Plan(n, 8000000, 1e9, kind=kind, enob=12, max_batch=G * K, average=K, average_layout=layout) as plan:
        w = plan.window().astype(np.float64)
        parts = plan.average_parts(G * K)
        d = torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).reshape(-1)).to(dev)
        plan.submit_device(0, d, G * K, center_freqs=np.zeros(G * K))
        p, _, _ = plan.collect(0)
    X = np.fft.fft(x64 * w, axis=-1)
    P = X.real ** 2 + X.imag ** 2
    idx = [(g + G * np.arange(K)) if layout == capi.AVG_SWEEPS else (g * K + np.arange(K)) for g in range(G)]
    P_ref = np.stack([P[i].mean(axis=0) for i in idx])
    return figure(p, P_ref), parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=40)
    ap.add_argument("--sizes", default="1024,2048,4096,8192")
    ap.add_argument("--seed", type=int, default=2024)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for n in [int(v) for v in args.sizes.split(",")]:
        figs, split = [], 0
        for t in range(args.trials):
            f, parts = trial(n, args.seed + 1000 * n + t, dev)
            figs.append(f)
            split += parts > 1
        worst = max(figs)
        print(json.dumps({"n": n, "trials": args.trials, "seed": args.seed, "split_trials": split, "worst": worst,
                          "median": float(np.median(figs)), "margin": round(1.0 - worst / BAR, 4), "build": build.source_hash()}),
              flush=True)


if __name__ == "__main__":
    main()
