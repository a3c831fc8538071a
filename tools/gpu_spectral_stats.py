#!/usr/bin/env python3
"""Measures the per-bin statistics on the GPU -> profiles/spectral_stats.json (README.md, "Per-bin statistics").

  * K1 rate (frames/s, Tsample/s) with and without RPF_FLAG_BIN_STATS at N = 4096 and 8192, rectangular and Hann, cu8,
    and cs16 at 4096, on a device-resident stream larger than the Infinity Cache, with the launch geometry and LDS of
    each case (registers and occupancy: profiles/spectral_stats_resources.txt, from the compiler);
  * the catch-all rate at 5000 and 65536 bins with and without the flag;
  * accuracy: S1, S2, PK against float64 truth for the GPU and for the CPU float32 path on the same stream, per case of
    tests/test_gpu_spectral_stats.py (its accuracy_figures), and the spectral kurtosis error against its bound.

Warm-up, then `--runs` timed runs per case (events on the stream); median, min and max are recorded.  `--part` picks
one of the three sections so that each fits a time limit of its own; the parts merge into one file.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rtl_power_fftw_amd as rpf                      # noqa: E402
from rtl_power_fftw_amd import _lib, synth            # noqa: E402

DEV = torch.device("cuda:0")


def engine(N, fmt, window, bin_stats, flags=0):
    w = synth.hann_window(N) if window else None
    return rpf.Datastore(rpf.Params(N=N, window=window, sample_format=fmt, bin_stats=bin_stats), w, flags=flags)


def rate(ds, d_stream, nbytes, runs, warmup=3):
    N = ds.params.N
    with_stats = ds.has_bin_stats
    out = torch.empty((3 if with_stats else 1) * N, dtype=torch.float64, device=DEV)
    s = torch.cuda.current_stream()
    call = ds.accumulate_device_stats if with_stats else ds.accumulate_device
    times, frames = [], 0
    for k in range(warmup + runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        frames = call(d_stream.data_ptr(), nbytes, 1 << 40, out.data_ptr(), s.cuda_stream)
        b.record(s)
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(a.elapsed_time(b) * 1e-3)
    t = np.array(times)
    med = float(np.median(t))
    return {"bin_stats": with_stats, "frames": int(frames), "seconds_median": med, "seconds_min": float(t.min()),
            "seconds_max": float(t.max()), "frames_per_s": frames / med, "tsample_per_s": frames * N / med * 1e-12,
            "runs": runs, **ds.launch_info()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_stats.json"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--samples-log2", type=int, default=28, help="complex samples of the K1 streams (2^28: 0.5 / 1 GB)")
    ap.add_argument("--part", choices=("k1", "catch_all", "accuracy", "all"), default="all")
    args = ap.parse_args()

    res = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    res["device"] = torch.cuda.get_device_name(0)
    nsamples = 1 << args.samples_log2
    if args.part in ("k1", "all"):
        res["k1_rate"] = []
        raw = torch.randint(0, 256, (4 * nsamples,), dtype=torch.uint8, device=DEV)
        for N, window, fmt in ((4096, False, "cu8"), (4096, True, "cu8"), (8192, False, "cu8"), (8192, True, "cu8"),
                               (4096, False, "cs16")):
            pair = []
            for bin_stats in (False, True):
                with engine(N, fmt, window, bin_stats) as ds:
                    pair.append(rate(ds, raw, ds.sample_bytes * nsamples, args.runs))
            row = {"N": N, "window": "hann" if window else "rect", "format": fmt, "plain": pair[0], "stats": pair[1],
                   "stats_over_plain": pair[1]["frames_per_s"] / pair[0]["frames_per_s"]}
            res["k1_rate"].append(row)
            print(row, flush=True)
        del raw
    if args.part in ("catch_all", "all"):
        res["catch_all_rate"] = []
        n = 1 << 24                                        # the catch-all moves 16 bytes per sample and pass
        raw = torch.randint(0, 256, (2 * n,), dtype=torch.uint8, device=DEV)
        for N in (5000, 65536):
            pair = []
            for bin_stats in (False, True):
                with engine(N, "cu8", False, bin_stats, flags=_lib.FLAG_CATCH_ALL) as ds:
                    pair.append(rate(ds, raw, 2 * n, max(3, args.runs // 2), warmup=1))
            with engine(N, "cu8", False, False) as ds:
                tuned = rate(ds, raw, 2 * n, max(3, args.runs // 2), warmup=1)
            row = {"N": N, "catch_all_plain": pair[0], "catch_all_stats": pair[1], "tuned_family_plain": tuned,
                   "stats_over_plain": pair[1]["frames_per_s"] / pair[0]["frames_per_s"],
                   "stats_over_tuned_family": pair[1]["frames_per_s"] / tuned["frames_per_s"]}
            res["catch_all_rate"].append(row)
            print(row, flush=True)
        del raw
    if args.part in ("accuracy", "all"):
        from test_gpu_spectral_stats import K1_CASES, accuracy_figures
        res["accuracy"] = []
        for N, window in K1_CASES + [(5000, False)]:
            for name in ("noise_tones", "uniform"):
                res["accuracy"].append(accuracy_figures(N, window, name, frames=40 if N == 5000 else 80))
                print(res["accuracy"][-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
