#!/usr/bin/env python3
"""Measures the short-time Fourier transform on the GPU -> profiles/stft.json (README.md, "Short-time Fourier transform").

One device-resident stream of 2^28 samples, N = 512, 4096 and 8192, cu8 and cf32, rectangular and Hann; warm-up, then
`--runs` timed runs per case (events on the stream), the median recorded with the smallest and the largest run, whose
distance is the run-to-run spread.  Per case:
  stft       rpf_stft_device on the native route (K1's store kernels): seconds, samples per second, and the bytes
             written per second (8 per sample) against the measured HBM read bandwidth (--hbm-gbs, from
             profiles/r03_hbm_read.txt)
  power      (a) rpf_accumulate_device of the same engine on the same stream: stft - power prices the stores
  catch_all  (b) the same rpf_stft_device call on an RPF_FLAG_CATCH_ALL engine, the only other route; a K1 size stays
             native only where its median beats this one outside both spreads ("native_beats_catch_all")
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


def timed(enqueue, runs, warmup=2):
    s = torch.cuda.current_stream()
    times = []
    for k in range(warmup + runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        enqueue(s.cuda_stream)
        b.record(s)
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(a.elapsed_time(b) * 1e-3)
    return {"median": float(np.median(times)), "min": float(min(times)), "max": float(max(times))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples-log2", type=int, default=28)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--sizes", default="512,4096,8192")
    ap.add_argument("--hbm-gbs", type=float, default=5414.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stft.json"))
    args = ap.parse_args()
    samples = 1 << args.samples_log2
    cases = []
    for fmt in ("cu8", "cf32"):
        b = _lib.SAMPLE_BYTES[fmt]
        # the bytes need not mean anything for the rate: random bytes for cu8, small random floats for cf32
        if fmt == "cu8":
            d_in = torch.randint(0, 256, (samples * b,), dtype=torch.uint8, device=DEV)
        else:
            d_in = torch.randn(samples * 2, dtype=torch.float32, device=DEV).view(torch.uint8)
        d_rows = torch.empty(samples * 2, dtype=torch.float32, device=DEV)
        for N in (int(v) for v in args.sizes.split(",")):
            frames = samples // N
            d_pwr = torch.empty(N, dtype=torch.float64, device=DEV)
            for hann in (False, True):
                w = synth.hann_window(N) if hann else None
                params = rpf.Params(N=N, window=hann, sample_format=fmt, buffers=2, buf_length=16384)
                with rpf.Datastore(params, w) as ds, rpf.Datastore(params, w, flags=_lib.FLAG_CATCH_ALL) as ca:
                    t_stft = timed(lambda s: ds.stft_device(d_in.data_ptr(), d_in.numel(), frames, d_rows.data_ptr(), s), args.runs)
                    info = ds.launch_info()
                    t_pwr = timed(lambda s: ds.accumulate_device(d_in.data_ptr(), d_in.numel(), frames, d_pwr.data_ptr(), s), args.runs)
                    t_ca = timed(lambda s: ca.stft_device(d_in.data_ptr(), d_in.numel(), frames, d_rows.data_ptr(), s), args.runs)
                written = 8.0 * frames * N
                case = {"format": fmt, "N": N, "window": "hann" if hann else "rect", "frames": frames,
                        "stft_seconds": t_stft, "power_seconds": t_pwr, "catch_all_stft_seconds": t_ca,
                        "stft_gsamples_per_s": frames * N / t_stft["median"] * 1e-9,
                        "stft_written_gb_per_s": written / t_stft["median"] * 1e-9,
                        "stft_written_over_hbm_read": written / t_stft["median"] * 1e-9 / args.hbm_gbs,
                        "stft_over_power": t_stft["median"] / t_pwr["median"],
                        "catch_all_over_native": t_ca["median"] / t_stft["median"],
                        "native_beats_catch_all": t_stft["max"] < t_ca["min"],
                        "grid": info["grid"], "lds_bytes": info["lds_bytes"]}
                print(json.dumps(case), flush=True)
                cases.append(case)
        del d_in, d_rows
    rep = {"samples": samples, "runs": args.runs, "hbm_read_gb_per_s": args.hbm_gbs, "cases": cases}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
