#!/usr/bin/env python3
"""Measures the polyphase filter bank front end on the GPU -> profiles/pfb.json (README.md, "Polyphase filter bank").

A device-resident stream of 2^28 samples, N = 512 and 4096, cu8 and cf32, T = 4 and 8 (the sliding-window fold) and
T = 5 (the re-reading fold); warm-up, then `--runs` timed runs per case (events on the stream), the median recorded.
Per case:
  pfb        the PFB engine, fold + transform, per 64 MB chunk of folded frames
  prefolded  (a) the rectangular cf32 engine on a stream of as many frames that is folded already: pfb - prefolded
             prices the fold
  plain      (b) the plain engine of the input format on the same bytes
  fold       the fold alone, as the difference pfb - prefolded: seconds, and bytes per second with b + 8 bytes moved
             per complex sample (the transform reads the 8 again), against the measured HBM read bandwidth
             (--hbm-gbs, from profiles/r03_hbm_read.txt)
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

DEV = torch.device("cuda:0")


def seconds(ds, d_stream, nbytes, runs, warmup=3):
    out = torch.empty(ds.params.N, dtype=torch.float64, device=DEV)
    s = torch.cuda.current_stream()
    times, frames = [], 0
    for k in range(warmup + runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        frames = ds.accumulate_device(d_stream.data_ptr(), nbytes, 1 << 40, out.data_ptr(), s.cuda_stream)
        b.record(s)
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(a.elapsed_time(b) * 1e-3)
    return int(frames), float(np.median(times)), float(min(times)), float(max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pfb.json"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--samples-log2", type=int, default=28)
    ap.add_argument("--hbm-gbs", type=float, default=5414.0, help="measured HBM read bandwidth, GB/s")
    args = ap.parse_args()
    nsamples = 1 << args.samples_log2
    # finite floats: the same buffer is read as cu8 (its first 2 bytes per sample) -- any bytes do there
    raw = torch.randn(2 * nsamples, dtype=torch.float32, device=DEV).view(torch.uint8)
    res = {"device": torch.cuda.get_device_name(0), "samples": nsamples, "hbm_read_gb_per_s": args.hbm_gbs, "cases": []}
    for N in (512, 4096):
        for fmt in ("cu8", "cf32"):
            b = 8 if fmt == "cf32" else 2
            with rpf.Datastore(rpf.Params(N=N, sample_format=fmt)) as plain, \
                    rpf.Datastore(rpf.Params(N=N, sample_format="cf32")) as rect:
                f_plain, t_plain, _, _ = seconds(plain, raw, b * nsamples, args.runs)
                for T in (4, 8, 5):
                    with rpf.Datastore(rpf.Params(N=N, sample_format=fmt, pfb_taps=T)) as ds:
                        frames, t, t_min, t_max = seconds(ds, raw, b * nsamples, args.runs)
                        info = ds.launch_info()
                    _, t_pre, _, _ = seconds(rect, raw, 8 * N * frames, args.runs)
                    t_fold = t - t_pre
                    case = {"N": N, "format": fmt, "taps": T, "form": "sliding" if T in (1, 2, 3, 4, 8) else "re-reading",
                            "frames": frames, "runs": args.runs,
                            "pfb_seconds_median": t, "pfb_seconds_min": t_min, "pfb_seconds_max": t_max,
                            "prefolded_cf32_seconds_median": t_pre, "plain_seconds_median": t_plain, "plain_frames": f_plain,
                            "pfb_over_prefolded": t / t_pre, "pfb_over_plain": t / t_plain,
                            "fold_seconds": t_fold,
                            "fold_gb_per_s": frames * N * (b + 8) / t_fold * 1e-9 if t_fold > 0 else None,
                            "tsample_per_s": frames * N / t * 1e-12, **info}
                    if case["fold_gb_per_s"] and args.hbm_gbs:
                        case["fold_fraction_of_hbm_read"] = case["fold_gb_per_s"] / args.hbm_gbs
                    res["cases"].append(case)
                    print(case, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
