#!/usr/bin/env python3
"""Measures cf32 with per-bin statistics on the GPU -> profiles/cf32_stats.json (README.md, "Sample formats").

At N = 512, 4096 and 8192, rectangular and Hann, on a device-resident stream of 2^28 cf32 samples (2 GB), three engines
of the same build:

  k1_stats      a cf32 engine with RPF_FLAG_BIN_STATS: K1's statistics kernels, rpf_accumulate_device_stats
  k1_plain      (a) the plain cf32 engine of the same N, rpf_accumulate_device: what the statistics cost
  catch_all     (b) a cf32 stats engine with RPF_FLAG_CATCH_ALL, rpf_accumulate_device_stats: the route a cf32 stats
                engine had at every size before K1 had these kernels

and the series of statistics at L = 16 and 128 frames per spectrum (one launch, rpf_accumulate_device_series_stats)
against K calls of rpf_accumulate_device_stats on the K slices, on the first 2^24 samples of the stream.  Warm-up, then
`--runs` timed runs per case (events on the stream); the median, the minimum and the maximum are recorded.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rtl_power_fftw_amd as rpf                      # noqa: E402
from rtl_power_fftw_amd import _lib, synth            # noqa: E402

DEV = torch.device("cuda:0")


def engine(N, window, bin_stats, flags=0):
    w = synth.hann_window(N) if window else None
    return rpf.Datastore(rpf.Params(N=N, window=window, sample_format="cf32", bin_stats=bin_stats), w, flags=flags)


def timed(call, runs, warmup=3):
    s = torch.cuda.current_stream()
    times, ret = [], None
    for k in range(warmup + runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        ret = call(s.cuda_stream)
        b.record(s)
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(a.elapsed_time(b) * 1e-3)
    t = np.array(times)
    return ret, {"seconds_median": float(np.median(t)), "seconds_min": float(t.min()), "seconds_max": float(t.max()),
                 "runs": runs}


def rate(ds, d_stream, nbytes, runs):
    N = ds.params.N
    out = torch.empty(3 * N, dtype=torch.float64, device=DEV)
    entry = ds.accumulate_device_stats if ds.has_bin_stats else ds.accumulate_device
    frames, t = timed(lambda s: entry(d_stream.data_ptr(), nbytes, 1 << 40, out.data_ptr(), s), runs)
    med = t["seconds_median"]
    return {"frames": int(frames), **t, "frames_per_s": frames / med, "tsample_per_s": frames * N / med * 1e-12,
            "read_gb_per_s": frames * N * 8 / med * 1e-9, **ds.launch_info()}


def series(ds, d_stream, nbytes, L, runs):
    N = ds.params.N
    K = nbytes // (8 * N * L)
    rows = torch.empty(K * 3 * N, dtype=torch.float64, device=DEV)
    done, one = timed(lambda s: ds.accumulate_device_series_stats(d_stream.data_ptr(), nbytes, L, K, rows.data_ptr(), s), runs)
    launches = ds.series_launches()
    span = 8 * N * L

    def slices(s):
        for k in range(K):
            ds.accumulate_device_stats(d_stream.data_ptr() + k * span, span, L, rows.data_ptr() + 24 * N * k, s)
        return K

    _, many = timed(slices, runs)
    return {"L": L, "K": int(done), "series_launches": launches, "series": one, "slices": many,
            "slices_over_series": many["seconds_median"] / one["seconds_median"],
            "series_tsample_per_s": done * L * N / one["seconds_median"] * 1e-12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cf32_stats.json"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--samples-log2", type=int, default=28, help="complex samples of the stream (2^28: 2 GB of cf32)")
    ap.add_argument("--series-samples-log2", type=int, default=24, help="samples the series cases read")
    args = ap.parse_args()
    nsamples = 1 << args.samples_log2
    nbytes = 8 * nsamples
    series_bytes = 8 << min(args.series_samples_log2, args.samples_log2)
    raw = torch.randn(2 * nsamples, dtype=torch.float32, device=DEV).view(torch.uint8)
    res = {"device": torch.cuda.get_device_name(0), "samples": nsamples, "series_samples": series_bytes // 8, "rate": [],
           "series": []}
    for N in (512, 4096, 8192):
        for window in (False, True):
            case = {"N": N, "window": "hann" if window else "rect"}
            with engine(N, window, True) as ds:
                case["k1_stats"] = rate(ds, raw, nbytes, args.runs)
                for L in (16, 128):
                    res["series"].append({"N": N, "window": case["window"], **series(ds, raw, series_bytes, L, args.runs)})
                    print(res["series"][-1], flush=True)
            with engine(N, window, False) as ds:
                case["k1_plain"] = rate(ds, raw, nbytes, args.runs)
            with engine(N, window, True, _lib.FLAG_CATCH_ALL) as ds:
                case["catch_all"] = rate(ds, raw, nbytes, args.runs)
            case["stats_over_plain_time"] = case["k1_stats"]["seconds_median"] / case["k1_plain"]["seconds_median"]
            case["catch_all_over_k1_time"] = case["catch_all"]["seconds_median"] / case["k1_stats"]["seconds_median"]
            res["rate"].append(case)
            print(case, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
