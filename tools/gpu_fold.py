#!/usr/bin/env python3
"""Measures the fold of the DM-time plane at trial periods on the GPU -> profiles/fold.json (README.md, "Folding").

One device-resident cu8 stream of 2^26 samples, N = 64 and 256, L = 16 and 128 frames per integration, D = 32 and 256
trials (the DM tables of tools/gpu_dedisperse.py: neighbouring trials one row apart at the lowest bin), P = 64 and 1024
trial periods evenly spaced from 20 to 60 rows, NB = 16 and 128 phase bins.  The plane is dedispersed once per (N, L, D)
into a torch buffer; warm-up, then `--runs` timed runs per case (events on the stream): the median, the smallest and
the largest.  Per case:
  fold        the whole rpf_fold_device call on that plane (prof, hits and mom), events around it on an idle stream; two
              calls where D P NB exceeds the 2^24 cells of one
  dedisperse  (a) rpf_dedisperse_device alone, the plane the fold reads
  numpy       (b) fold.reference on the host, wall clock, ONE run over one series and at most --numpy-periods periods of
              the same T, scaled to D x P: what users had
Reported: the fold against (a), its speed-up over (b), the cell updates (D P T) per second, and the bytes of LDS a wave
holds (512 per phase bin), which bounds the waves a CU keeps: 160 KiB / that.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rtl_power_fftw_amd as rpf                      # noqa: E402
from rtl_power_fftw_amd import dedisperse, fold       # noqa: E402
from gpu_dedisperse import FC, RATE, timed            # noqa: E402

DEV = torch.device("cuda:0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fold.json"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--samples-log2", type=int, default=26)
    ap.add_argument("--numpy-periods", type=int, default=8)
    args = ap.parse_args()
    nsamples = 1 << args.samples_log2
    nbytes = 2 * nsamples
    raw = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=DEV)
    res = {"device": torch.cuda.get_device_name(0), "samples": nsamples, "runs": args.runs, "fc_hz": FC, "rate": RATE,
           "segments": fold.SEGMENTS, "period_rows": [20.0, 60.0], "cases": []}
    for N in (64, 256):
        for L in (16, 128):
            with rpf.Datastore(rpf.Params(N=N)) as ds:
                K = ds.frames_in(nbytes) // L
                ds.quantile_reset()
                assert ds.quantile_append_device(raw.data_ptr(), nbytes, L, K, torch.cuda.current_stream().cuda_stream) == K
                median = ds.quantile_select([0.5])[0]
                w = np.where(median != 0, 1.0 / np.where(median != 0, median, 1.0), 0.0)
                w[N // 2] = 0.0
                for D in (32, 256):
                    want = min(D - 1, K // 4)
                    per_dm = dedisperse.dm_delays([1.0e4], FC, RATE, N, L).max() / 1.0e4
                    delays = dedisperse.dm_delays(np.linspace(0.0, want / per_dm, D), FC, RATE, N, L)
                    T = ds.dedisperse_times(delays)
                    plane = torch.empty(D * T, dtype=torch.float64, device=DEV)
                    dd, dd_min, dd_max = timed(lambda s: ds.dedisperse_device(delays, w, plane.data_ptr(), plane.numel(), s), args.runs)
                    host_series = plane[:T].cpu().numpy().reshape(1, T)
                    for P in (64, 1024):
                        steps = fold.row_period_steps(np.linspace(20.0, 60.0, P))
                        for NB in (16, 128):
                            prof = torch.empty(D * P * NB, dtype=torch.float64, device=DEV)
                            hits = torch.empty(P * NB, dtype=torch.int32, device=DEV)
                            mom = torch.empty(2 * D, dtype=torch.float64, device=DEV)
                            # (a call folds at most 2^24 cells: 256 x 1024 x 128 goes in two calls of 128 series)
                            per_call = min(D, (1 << 24) // (P * NB))

                            def call(s):
                                for s0 in range(0, D, per_call):
                                    ds.fold_device(plane.data_ptr() + 8 * s0 * T, min(per_call, D - s0), T, steps, NB,
                                                   prof.data_ptr() + 8 * s0 * P * NB, per_call * P * NB, hits.data_ptr(),
                                                   mom.data_ptr() + 16 * s0, s)
                            t, t_min, t_max = timed(call, args.runs)
                            some = steps[::max(1, P // args.numpy_periods)][:args.numpy_periods]
                            t0 = time.perf_counter()
                            want_prof = fold.reference(host_series, some, NB)[0]
                            numpy_s = (time.perf_counter() - t0) * (D * P / some.size)
                            got = prof.cpu().numpy().reshape(D, P, NB)[0, ::max(1, P // args.numpy_periods)][:args.numpy_periods]
                            assert got.tobytes() == want_prof[0].tobytes()
                            case = {"N": N, "L": L, "D": D, "P": P, "NB": NB, "K": int(K), "T": int(T), "calls": -(-D // per_call),
                                    "fold_seconds_median": t, "fold_seconds_min": t_min, "fold_seconds_max": t_max,
                                    "dedisperse_seconds_median": dd, "dedisperse_seconds_min": dd_min, "dedisperse_seconds_max": dd_max,
                                    "fold_over_dedisperse": t / dd, "cell_updates_per_s": D * P * T / t,
                                    "lds_bytes_per_wave": 512 * NB, "waves_per_cu_by_lds": (160 * 1024) // (512 * NB),
                                    "numpy_host_seconds_scaled": numpy_s, "numpy_over_fold": numpy_s / t}
                            res["cases"].append(case)
                            print(case, flush=True)
                            del prof, hits, mom
                    del plane
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
