#!/usr/bin/env python3
"""Measures the correlator of up to eight streams on the GPU -> profiles/correlate.json (README.md, "Correlator").

M device-resident streams of 2^26 samples each, N = 512 and 4096, M = 2, 4 and 8, cu8 and cf32, rectangular; warm-up,
then `--runs` timed runs per case (events on the stream): the median, the smallest and the largest.  Per case:
  correlate  rpf_correlate_device: per 64 MB chunk of rows M STFT launches and the X-engine, one finishing launch
  stft       (a) the M rpf_stft_device calls alone, on the same streams, into one rows buffer; correlate - stft prices the
             X-engine (and its reduce and finish launches): seconds, and the rows' bytes it reads (8 N M per frame) per
             second against the measured HBM read bandwidth (--hbm-gbs, from profiles/r03_hbm_read.txt)
  cross      (b) at M = 2: rpf_accumulate_device_cross on the same two streams; whether the correlator is faster
             outside both spreads (its largest run below the cross entry's smallest)
  numpy      (c) at M = 4: the visibilities of the same streams with numpy on the host (complex64 transforms, the pair
             products summed in complex128), wall clock, ONE run over --numpy-samples-log2 samples scaled to the full
             length (the work is linear in the number of frames)
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


def timed(enqueue, runs, warmup=3):
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


def numpy_visibilities(streams, fmt, N):
    """Sum over the frames of X_i conj(X_j) of every pair on the host; returns the wall-clock seconds."""
    t0 = time.perf_counter()
    sign = (1 - 2 * (np.arange(N) % 2)).astype(np.float32)

    def frames(raw):
        v = raw.astype(np.float32) - np.float32(127) if fmt == "cu8" else raw.view(np.float32)
        return v.view(np.complex64).reshape(-1, N) * sign

    fr = [frames(s) for s in streams]
    M = len(fr)
    acc = np.zeros((M, M, N), dtype=np.complex128)
    rows = max(1, (1 << 20) // N)
    for r0 in range(0, fr[0].shape[0], rows):
        X = np.stack([np.fft.fft(f[r0:r0 + rows], axis=1) for f in fr]).astype(np.complex128)
        acc += np.einsum("ifk,jfk->ijk", X, np.conj(X))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correlate.json"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--samples-log2", type=int, default=26)
    ap.add_argument("--numpy-samples-log2", type=int, default=20)
    ap.add_argument("--hbm-gbs", type=float, default=5414.0, help="measured HBM read bandwidth, GB/s")
    args = ap.parse_args()
    nsamples = 1 << args.samples_log2
    n_host = 1 << min(args.numpy_samples_log2, args.samples_log2)
    # finite floats: the same buffers are read as cu8 (their first 2 bytes per sample) -- any bytes do there
    raw = [torch.randn(2 * nsamples, dtype=torch.float32, device=DEV).view(torch.uint8) for _ in range(8)]
    res = {"device": torch.cuda.get_device_name(0), "samples_per_stream": nsamples, "hbm_read_gb_per_s": args.hbm_gbs,
           "numpy_samples_per_stream": n_host, "runs": args.runs, "cases": []}
    for N in (512, 4096):
        for fmt in ("cu8", "cf32"):
            b = 8 if fmt == "cf32" else 2
            nbytes = b * nsamples
            with rpf.Datastore(rpf.Params(N=N, sample_format=fmt)) as ds:
                frames = ds.frames_in(nbytes)
                rows = torch.empty(frames * N * 2, dtype=torch.float32, device=DEV)
                for M in (2, 4, 8):
                    ptrs = [r.data_ptr() for r in raw[:M]]
                    out = torch.empty(M * M * 2 * N, dtype=torch.float64, device=DEV)
                    t, t_min, t_max = timed(lambda s: ds.correlate_device(ptrs, nbytes, 1 << 40, out.data_ptr(), s), args.runs)

                    def stft(s):
                        for p in ptrs:
                            ds.stft_device(p, nbytes, 1 << 40, rows.data_ptr(), s)

                    a, a_min, a_max = timed(stft, args.runs)
                    x = t - a
                    case = {"N": N, "format": fmt, "M": M, "frames": int(frames),
                            "correlate_seconds_median": t, "correlate_seconds_min": t_min, "correlate_seconds_max": t_max,
                            "stft_seconds_median": a, "stft_seconds_min": a_min, "stft_seconds_max": a_max,
                            "correlate_over_stft": t / a, "xengine_seconds": x,
                            "xengine_rows_gb_per_s": frames * N * 8 * M / x * 1e-9 if x > 0 else None,
                            "tsample_per_s_per_stream": frames * N / t * 1e-12}
                    if case["xengine_rows_gb_per_s"]:
                        case["xengine_fraction_of_hbm_read"] = case["xengine_rows_gb_per_s"] / args.hbm_gbs
                    if M == 2:
                        c_out = torch.empty(4 * N, dtype=torch.float64, device=DEV)
                        c, c_min, c_max = timed(lambda s: ds.accumulate_device_cross(ptrs[0], ptrs[1], nbytes, 1 << 40,
                                                                                      c_out.data_ptr(), s), args.runs)
                        case.update({"cross_seconds_median": c, "cross_seconds_min": c_min, "cross_seconds_max": c_max,
                                     "correlate_over_cross": t / c,
                                     "faster_than_cross_outside_both_spreads": t_max < c_min})
                    if M == 4:
                        host = [r[:b * n_host].cpu().numpy() for r in raw[:M]]
                        t_numpy = numpy_visibilities(host, fmt, N) * (nsamples / n_host)
                        case.update({"numpy_host_seconds_scaled": t_numpy, "numpy_over_correlate": t_numpy / t})
                    res["cases"].append(case)
                    print(case, flush=True)
                del rows
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
