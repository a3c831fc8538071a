#!/usr/bin/env python3
"""Measures the spectrogram mode on the GPU -> profiles/series.json (README.md, "Spectrogram").

N = 4096 and 512, rectangular, cu8, a device-resident stream of 2^28 complex samples; for L in {1, 2, 16, 128, 1024,
all frames} three rates in Tsample/s, each the median of `--runs` timed runs (events on the stream) after a warm-up:

  * series      rpf_accumulate_device_series: one persistent launch and one fix-up launch whatever K is;
  * hops        the comparator: rpf_accumulate_device_hops fed the same K integrations as hops (16 per launch);
  * single      at L = all frames only: rpf_accumulate_device, runs alternating with the series runs.

The comparator's argument arrays are built before the clock starts; what it pays per 16 hops is a launch and a reduce.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "series.json"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples-log2", type=int, default=28)
    ap.add_argument("--sizes", default="4096,512")
    args = ap.parse_args()
    nsamples = 1 << args.samples_log2
    raw = torch.randint(0, 256, (2 * nsamples,), dtype=torch.uint8, device=DEV)
    res = {"device": torch.cuda.get_device_name(0), "samples": nsamples, "cases": []}
    for N in [int(x) for x in args.sizes.split(",")]:
        F = nsamples // N
        with rpf.Datastore(rpf.Params(N=N)) as ds:
            lib, h = ds._lib, ds._handle
            for L in (1, 2, 16, 128, 1024, F):
                K = F // L
                out = torch.empty((K, N), dtype=torch.float64, device=DEV)
                done = ctypes.c_int64()

                def series(s):
                    rc = lib.rpf_accumulate_device_series(h, ctypes.c_void_p(raw.data_ptr()), 2 * nsamples, L, K,
                                                          ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(s), ctypes.byref(done))
                    assert rc == 0 and done.value == K

                ptrs = (ctypes.c_void_p * K)(*[raw.data_ptr() + 2 * N * L * k for k in range(K)])
                nb = (ctypes.c_size_t * K)(*([2 * N * L] * K))
                rep = (ctypes.c_int64 * K)(*([L] * K))
                hop_done = (ctypes.c_int64 * K)()

                def hops(s):
                    rc = lib.rpf_accumulate_device_hops(h, ptrs, nb, rep, K, ctypes.c_void_p(out.data_ptr()),
                                                        ctypes.c_void_p(s), hop_done)
                    assert rc == 0

                case = {"N": N, "L": L, "K": K}
                if L == F:
                    one = torch.empty(N, dtype=torch.float64, device=DEV)

                    def single(s):
                        assert ds.accumulate_device(raw.data_ptr(), 2 * nsamples, F, one.data_ptr(), s) == F

                    ts, t1 = [], []
                    for k in range(args.warmup + args.runs):            # alternating runs
                        a = timed(series, 1, 0)
                        b = timed(single, 1, 0)
                        if k >= args.warmup:
                            ts += a
                            t1 += b
                    case["series"] = summary(ts, K * L * N)
                    case["series"]["launches"] = ds.series_launches()
                    case["single"] = summary(t1, F * N)
                else:
                    case["series"] = summary(timed(series, args.runs, args.warmup), K * L * N)
                    case["series"]["launches"] = ds.series_launches()
                case["series"].update(ds.launch_info())
                case["hops"] = summary(timed(hops, args.runs, args.warmup), K * L * N)
                case["series_over_hops"] = case["hops"]["seconds_median"] / case["series"]["seconds_median"]
                if "single" in case:
                    case["series_over_single"] = case["single"]["seconds_median"] / case["series"]["seconds_median"]
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
                del out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
