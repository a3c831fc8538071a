#!/usr/bin/env python3
"""Measures the series of per-bin statistics on the GPU -> profiles/series_stats.json (README.md, "Time-resolved
statistics").

N = 512 and 4096, rectangular, cu8, a device-resident stream of 2^28 complex samples; for L in {1, 2, 16, 128, 1024, all
frames} three rates in Tsample/s, each the median of `--runs` timed runs (events on the stream) after a warm-up:

  * series_stats  rpf_accumulate_device_series_stats of a stats engine: one persistent launch and one fix-up launch;
  * series        comparator (a), the cost of the statistics: rpf_accumulate_device_series of a plain engine, same N, L;
  * slices        comparator (b), the route users had: K calls of rpf_accumulate_device_stats on the slices, enqueued
                  back to back on the stream (a transform launch and a reduce launch each).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rtl_power_fftw_amd as rpf                      # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn, runs, warmup):
    s = torch.cuda.current_stream()
    times = []
    for k in range(warmup + runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn(s.cuda_stream)
        b.record(s)
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(a.elapsed_time(b) * 1e-3)
    return times


def summary(times, samples):
    t = np.array(times)
    med = float(np.median(t))
    return {"seconds_median": med, "seconds_min": float(t.min()), "seconds_max": float(t.max()),
            "tsample_per_s": samples / med * 1e-12, "runs": len(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "series_stats.json"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples-log2", type=int, default=28)
    ap.add_argument("--sizes", default="512,4096")
    args = ap.parse_args()
    nsamples = 1 << args.samples_log2
    nbytes = 2 * nsamples
    raw = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=DEV)
    res = {"device": torch.cuda.get_device_name(0), "samples": nsamples, "cases": []}
    for N in [int(x) for x in args.sizes.split(",")]:
        F = nsamples // N
        with rpf.Datastore(rpf.Params(N=N, bin_stats=True)) as st, rpf.Datastore(rpf.Params(N=N)) as plain:
            lib = st._lib
            for L in (1, 2, 16, 128, 1024, F):
                K = F // L
                out = torch.empty((K, 3, N), dtype=torch.float64, device=DEV)
                done = ctypes.c_int64()
                src, dst = raw.data_ptr(), out.data_ptr()

                def series_stats(s):
                    rc = lib.rpf_accumulate_device_series_stats(st._handle, ctypes.c_void_p(src), nbytes, L, K,
                                                                ctypes.c_void_p(dst), ctypes.c_void_p(s), ctypes.byref(done))
                    assert rc == 0 and done.value == K

                def series(s):
                    rc = lib.rpf_accumulate_device_series(plain._handle, ctypes.c_void_p(src), nbytes, L, K,
                                                          ctypes.c_void_p(dst), ctypes.c_void_p(s), ctypes.byref(done))
                    assert rc == 0 and done.value == K

                def slices(s):
                    fn, h, span, row, cs = lib.rpf_accumulate_device_stats, st._handle, 2 * N * L, 8 * 3 * N, ctypes.c_void_p(s)
                    for k in range(K):
                        fn(h, ctypes.c_void_p(src + k * span), span, L, ctypes.c_void_p(dst + k * row), cs, None)

                case = {"N": N, "L": L, "K": K}
                case["series_stats"] = summary(timed(series_stats, args.runs, args.warmup), K * L * N)
                case["series_stats"]["launches"] = st.series_launches()
                case["series_stats"].update(st.launch_info())
                case["series"] = summary(timed(series, args.runs, args.warmup), K * L * N)
                case["series"].update(plain.launch_info())
                case["slices"] = summary(timed(slices, args.runs, 1), K * L * N)
                case["stats_cost"] = case["series_stats"]["seconds_median"] / case["series"]["seconds_median"] - 1.0
                case["series_stats_over_slices"] = case["slices"]["seconds_median"] / case["series_stats"]["seconds_median"]
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
                del out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
