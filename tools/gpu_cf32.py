#!/usr/bin/env python3
"""Measures the float32 sample format on the GPU -> profiles/cf32.json (README.md, "Sample formats").

K1 rate (frames/s, Tsample/s, bytes/s read) at N = 512, 4096 and 8192, rectangular and Hann, for cf32 beside cu8 and
cs16 of the same build, on a device-resident stream of 2^28 samples (cf32: 2 GB), with the launch geometry (grid, LDS)
of each case and the read rate as a fraction of the measured HBM read bandwidth (--hbm-gbs, from
profiles/r03_hbm_read.txt).  Warm-up, then `--runs` timed runs per case (events on the stream); the median, the
minimum and the maximum are recorded.
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
from rtl_power_fftw_amd import synth                  # noqa: E402

DEV = torch.device("cuda:0")


def engine(N, fmt, window=False):
    w = synth.hann_window(N) if window else None
    return rpf.Datastore(rpf.Params(N=N, window=window, sample_format=fmt), w)


def rate(ds, d_stream, nbytes, runs, warmup=3):
    N = ds.params.N
    out = torch.empty(N, dtype=torch.float64, device=DEV)
    s = torch.cuda.current_stream()
    times = []
    frames = 0
    for k in range(warmup + runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        frames = ds.accumulate_device(d_stream.data_ptr(), nbytes, 1 << 40, out.data_ptr(), s.cuda_stream)
        b.record(s)
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(a.elapsed_time(b) * 1e-3)
    t = np.array(times)
    med = float(np.median(t))
    return {"frames": int(frames), "seconds_median": med, "seconds_min": float(t.min()), "seconds_max": float(t.max()),
            "frames_per_s": frames / med, "tsample_per_s": frames * N / med * 1e-12,
            "read_gb_per_s": frames * N * ds.sample_bytes / med * 1e-9, "runs": runs, **ds.launch_info()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cf32.json"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--samples-log2", type=int, default=28, help="complex samples of the stream (2^28: 2 GB of cf32)")
    ap.add_argument("--hbm-gbs", type=float, default=None, help="measured HBM read bandwidth, GB/s")
    args = ap.parse_args()
    nsamples = 1 << args.samples_log2
    # finite floats: the same buffer is read as cu8 (its first 2 bytes per sample) and cs16 (4) -- any bytes do there
    raw = torch.randn(2 * nsamples, dtype=torch.float32, device=DEV).view(torch.uint8)
    res = {"device": torch.cuda.get_device_name(0), "samples": nsamples, "hbm_read_gb_per_s": args.hbm_gbs, "k1_rate": []}
    for N in (512, 4096, 8192):
        for window in (False, True):
            for fmt in ("cu8", "cs16", "cf32"):
                with engine(N, fmt, window) as ds:
                    r = rate(ds, raw, ds.sample_bytes * nsamples, args.runs)
                if args.hbm_gbs:
                    r["fraction_of_hbm_read"] = r["read_gb_per_s"] / args.hbm_gbs
                res["k1_rate"].append({"N": N, "window": "hann" if window else "rect", "format": fmt, **r})
                print(res["k1_rate"][-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
