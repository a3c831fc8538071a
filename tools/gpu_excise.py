#!/usr/bin/env python3
"""Measures the excised average on the GPU -> profiles/excise.json (README.md, "Excising interference").

The protocol of tools/gpu_series_stats.py: N = 512 and 4096, rectangular, cu8, a device-resident stream of 2^28 complex
samples; for L in {16, 128, 1024} three times, each the median of `--runs` timed runs (events on the stream) after a
warm-up:

  * excised       rpf_accumulate_device_excised with stats.sk_limits(L) and no mask (and once more with the mask):
                  per piece of rows the series launches and one excise launch, then the combine;
  * series_stats  comparator (a), what the excise pass costs: rpf_accumulate_device_series_stats alone into a K x 3 x N
                  buffer;
  * stats         comparator (b), what a user who does not excise pays: rpf_accumulate_device_stats of the whole stream.
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
from rtl_power_fftw_amd import stats                   # noqa: E402

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "excise.json"))
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
        with rpf.Datastore(rpf.Params(N=N, bin_stats=True)) as st:
            lib = st._lib
            for L in (16, 128, 1024):
                K = F // L
                lo, hi = stats.sk_limits(L)
                rows = torch.empty((K, 3, N), dtype=torch.float64, device=DEV)
                out = torch.empty((3, N), dtype=torch.float64, device=DEV)
                mask = torch.empty((K, N), dtype=torch.uint8, device=DEV)
                done = ctypes.c_int64()
                src = raw.data_ptr()

                def excised(s, d_mask=None):
                    rc = lib.rpf_accumulate_device_excised(st._handle, ctypes.c_void_p(src), nbytes, L, K, lo, hi,
                                                           ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(d_mask),
                                                           ctypes.c_void_p(s), ctypes.byref(done))
                    assert rc == 0 and done.value == K

                def excised_mask(s):
                    excised(s, mask.data_ptr())

                def series_stats(s):
                    rc = lib.rpf_accumulate_device_series_stats(st._handle, ctypes.c_void_p(src), nbytes, L, K,
                                                                ctypes.c_void_p(rows.data_ptr()), ctypes.c_void_p(s),
                                                                ctypes.byref(done))
                    assert rc == 0 and done.value == K

                def whole(s):
                    rc = lib.rpf_accumulate_device_stats(st._handle, ctypes.c_void_p(src), nbytes, K * L,
                                                         ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(s), ctypes.byref(done))
                    assert rc == 0 and done.value == K * L

                case = {"N": N, "L": L, "K": K, "sk_lo": lo, "sk_hi": hi}
                case["excised"] = summary(timed(excised, args.runs, args.warmup), K * L * N)
                case["excised"]["launches"] = st.series_launches()
                kept = out.cpu().numpy()[1]
                case["excised"]["flagged_share"] = float(1.0 - kept.mean() / K)
                case["excised_with_mask"] = summary(timed(excised_mask, args.runs, args.warmup), K * L * N)
                case["series_stats"] = summary(timed(series_stats, args.runs, args.warmup), K * L * N)
                case["stats"] = summary(timed(whole, args.runs, args.warmup), K * L * N)
                case["excised_over_series_stats"] = case["excised"]["seconds_median"] / case["series_stats"]["seconds_median"]
                case["excised_over_stats"] = case["excised"]["seconds_median"] / case["stats"]["seconds_median"]
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
                del rows, out, mask
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
