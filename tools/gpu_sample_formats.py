#!/usr/bin/env python3
"""Measures the sample formats on the GPU -> profiles/sample_formats.json (README.md, "Sample formats").

  * K1 rate (frames/s, Tsample/s) at N = 4096 and 8192, rectangular and Hann, for cu8 / cs8 / cs16 on a device-resident
    stream larger than the Infinity Cache, with the launch geometry of each case;
  * the catch-all rate for cs16 at 5000 and 65536 bins beside the cu8 rate of those sizes' tuned families;
  * accuracy: full-range cs16 against float64 truth per K1 size beside the cu8 figure of the same size, and the cu8
    catch-all comparator at the small sizes the format tests use.

Warm-up, then `--runs` timed runs per case (events on the stream); median, min and max are recorded.
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


def engine(N, fmt, window=False, flags=0):
    w = synth.hann_window(N) if window else None
    return rpf.Datastore(rpf.Params(N=N, window=window, sample_format=fmt), w, flags=flags)


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
    li = ds.launch_info()
    med = float(np.median(t))
    return {"frames": int(frames), "seconds_median": med, "seconds_min": float(t.min()), "seconds_max": float(t.max()),
            "frames_per_s": frames / med, "tsample_per_s": frames * N / med * 1e-12, "runs": runs, **li}


def run_spectrum(ds, stream):
    d = torch.from_numpy(stream).to(DEV)
    out = torch.empty(ds.params.N, dtype=torch.float64, device=DEV)
    n = ds.accumulate_device(d.data_ptr(), stream.size, 1 << 40, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_formats.json"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--samples-log2", type=int, default=28, help="complex samples of the K1 streams (2^28: 0.5 / 1 GB)")
    args = ap.parse_args()
    from helpers import max_err_over_mean, oracle_accumulate, truth_f64
    from test_gpu_sample_formats import clamped_cu8, truth_signed

    res = {"device": torch.cuda.get_device_name(0), "k1_rate": [], "catch_all_rate": [], "accuracy_k1": [],
           "accuracy_catch_all_cu8": []}
    nsamples = 1 << args.samples_log2
    raw = torch.randint(0, 256, (4 * nsamples,), dtype=torch.uint8, device=DEV)
    for N in (4096, 8192):
        for window in (False, True):
            for fmt in ("cu8", "cs8", "cs16"):
                with engine(N, fmt, window) as ds:
                    r = rate(ds, raw, ds.sample_bytes * nsamples, args.runs)
                res["k1_rate"].append({"N": N, "window": "hann" if window else "rect", "format": fmt, **r})
                print(res["k1_rate"][-1], flush=True)
    for N in (5000, 65536):
        n = 1 << 24                                        # the catch-all moves 16 bytes per sample and pass
        for fmt, flags, label in (("cu8", 0, "tuned family"), ("cu8", _lib.FLAG_CATCH_ALL, "catch-all"), ("cs16", 0, "catch-all")):
            with engine(N, fmt, flags=flags) as ds:
                r = rate(ds, raw, ds.sample_bytes * n, max(3, args.runs // 2), warmup=1)
            res["catch_all_rate"].append({"N": N, "format": fmt, "path": label, **r})
            print(res["catch_all_rate"][-1], flush=True)
    del raw
    for N, window in ((64, False), (512, False), (4096, False), (4096, True), (8192, False)):
        R = 80
        w = synth.hann_window(N) if window else None
        s16 = synth.noise_tones_cs16(41, R * N)
        u8 = synth.noise_tones_iq(41, R * N)
        with engine(N, "cs16", window) as a, engine(N, "cu8", window) as b:
            g16, _ = run_spectrum(a, s16)
            g8, _ = run_spectrum(b, u8)
        t16, t8 = truth_signed(N, synth.cs16_values(s16), R, w), truth_f64(N, u8, R, w)
        res["accuracy_k1"].append({"N": N, "window": "hann" if window else "rect", "frames": R,
                                   "cs16_vs_truth": float(np.max(np.abs(g16 - t16) / t16)),
                                   "cu8_vs_truth": float(np.max(np.abs(g8 - t8) / t8))})
        print(res["accuracy_k1"][-1], flush=True)
    for N, R in ((500, 64), (2046, 64), (5000, 64), (16384, 12), (65536, 12)):
        u = clamped_cu8(51, R * N)
        with engine(N, "cu8", flags=_lib.FLAG_CATCH_ALL) as ds:
            got, _ = run_spectrum(ds, u)
        truth = truth_f64(N, u, R)
        o32, _ = oracle_accumulate(N, u, R, None, 32)
        res["accuracy_catch_all_cu8"].append({"N": N, "frames": R, "over_mean_vs_truth": max_err_over_mean(got, truth),
                                              "over_mean_vs_oracle": max_err_over_mean(got, o32),
                                              "total_power": float(abs(got.sum() / truth.sum() - 1))})
        print(res["accuracy_catch_all_cu8"][-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
