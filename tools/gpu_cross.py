#!/usr/bin/env python3
"""Measures the cross-spectrum of two streams on the GPU -> profiles/cross.json (README.md, "Cross-spectrum").

Two device-resident streams of 2^28 samples each, N = 512 and 4096, cu8 and cf32, rectangular; warm-up, then `--runs`
timed runs per case (events on the stream), the median recorded.  Per case:
  cross      rpf_accumulate_device_cross: four transforms, one combine launch per 64 MB chunk of u and v, one finishing
             launch
  four       (a) the four power runs alone: rpf_accumulate_device on a and on b, and a cf32 engine on two streams of as
             many frames that are combined already; cross - four prices the combine and finishing launches
  combine    that difference: seconds, and bytes per second with 2b bytes read and 16 written per sample of the pair,
             against the measured HBM read bandwidth (--hbm-gbs, from profiles/r03_hbm_read.txt)
  numpy      (b) what a user had: the cross-spectrum of the same two streams with numpy on the host (complex64
             transforms, A conj(B) summed in double), wall clock, ONE run over --numpy-samples-log2 samples scaled to the
             full length (the transform is linear in the number of frames)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rtl_power_fftw_amd as rpf                      # noqa: E402

DEV = torch.device("cuda:0")


def median_seconds(enqueue, runs, warmup=3):
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
    return float(np.median(times)), float(min(times)), float(max(times))


def numpy_cross(a_bytes, b_bytes, fmt, N):
    """Sum over the frames of A conj(B), Saa and Sbb on the host; returns the wall-clock seconds."""
    t0 = time.perf_counter()

    def frames(raw):
        if fmt == "cu8":
            v = raw.astype(np.float32) - np.float32(127)
        else:
            v = raw.view(np.float32)
        z = v.view(np.complex64).reshape(-1, N)
        return z * (1 - 2 * (np.arange(N) % 2)).astype(np.float32)

    acc = np.zeros(N, dtype=np.complex128)
    saa, sbb = np.zeros(N), np.zeros(N)
    rows = max(1, (1 << 22) // N)
    fa, fb = frames(a_bytes), frames(b_bytes)
    for r0 in range(0, fa.shape[0], rows):
        A = np.fft.fft(fa[r0:r0 + rows], axis=1)
        B = np.fft.fft(fb[r0:r0 + rows], axis=1)
        acc += (A.astype(np.complex128) * np.conj(B.astype(np.complex128))).sum(axis=0)
        saa += (np.abs(A).astype(np.float64) ** 2).sum(axis=0)
        sbb += (np.abs(B).astype(np.float64) ** 2).sum(axis=0)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross.json"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--samples-log2", type=int, default=28)
    ap.add_argument("--numpy-samples-log2", type=int, default=28)
    ap.add_argument("--hbm-gbs", type=float, default=5414.0, help="measured HBM read bandwidth, GB/s")
    args = ap.parse_args()
    nsamples = 1 << args.samples_log2
    n_host = 1 << min(args.numpy_samples_log2, args.samples_log2)
    # finite floats: the same buffers are read as cu8 (their first 2 bytes per sample) -- any bytes do there
    raw_a = torch.randn(2 * nsamples, dtype=torch.float32, device=DEV).view(torch.uint8)
    raw_b = torch.randn(2 * nsamples, dtype=torch.float32, device=DEV).view(torch.uint8)
    res = {"device": torch.cuda.get_device_name(0), "samples_per_stream": nsamples, "hbm_read_gb_per_s": args.hbm_gbs,
           "numpy_samples_per_stream": n_host, "cases": []}
    for N in (512, 4096):
        for fmt in ("cu8", "cf32"):
            b = 8 if fmt == "cf32" else 2
            nbytes = b * nsamples
            out = torch.empty(4 * N, dtype=torch.float64, device=DEV)
            with rpf.Datastore(rpf.Params(N=N, sample_format=fmt)) as ds, \
                    rpf.Datastore(rpf.Params(N=N, sample_format="cf32")) as cf:
                frames = ds.frames_in(nbytes)
                t, t_min, t_max = median_seconds(
                    lambda s: ds.accumulate_device_cross(raw_a.data_ptr(), raw_b.data_ptr(), nbytes, 1 << 40, out.data_ptr(), s),
                    args.runs)
                info = ds.launch_info()

                def four(s):
                    ds.accumulate_device(raw_a.data_ptr(), nbytes, 1 << 40, out.data_ptr(), s)
                    ds.accumulate_device(raw_b.data_ptr(), nbytes, 1 << 40, out.data_ptr() + 8 * N, s)
                    cf.accumulate_device(raw_a.data_ptr(), 8 * N * frames, 1 << 40, out.data_ptr() + 16 * N, s)
                    cf.accumulate_device(raw_b.data_ptr(), 8 * N * frames, 1 << 40, out.data_ptr() + 24 * N, s)

                t_four, _, _ = median_seconds(four, args.runs)
            host_a = raw_a[:b * n_host].cpu().numpy()
            host_b = raw_b[:b * n_host].cpu().numpy()
            t_numpy = numpy_cross(host_a, host_b, fmt, N) * (nsamples / n_host)
            t_combine = t - t_four
            case = {"N": N, "format": fmt, "frames": int(frames), "runs": args.runs,
                    "cross_seconds_median": t, "cross_seconds_min": t_min, "cross_seconds_max": t_max,
                    "four_power_runs_seconds_median": t_four, "cross_over_four": t / t_four,
                    "combine_and_finish_seconds": t_combine,
                    "combine_gb_per_s": frames * N * (2 * b + 16) / t_combine * 1e-9 if t_combine > 0 else None,
                    "numpy_host_seconds_scaled": t_numpy, "numpy_over_cross": t_numpy / t,
                    "tsample_per_s_per_stream": frames * N / t * 1e-12, **info}
            if case["combine_gb_per_s"] and args.hbm_gbs:
                case["combine_fraction_of_hbm_read"] = case["combine_gb_per_s"] / args.hbm_gbs
            res["cases"].append(case)
            print(case, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
