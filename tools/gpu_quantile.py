#!/usr/bin/env python3
"""Measures the per-bin quantiles on the GPU -> profiles/quantile.json (README.md, "Quantiles of the integrations").

The protocol of tools/gpu_excise.py: rectangular, cu8, a device-resident stream of 2^28 complex samples; N in
{64, 512, 4096} x L in {16, 128, 1024} with the K that results (capped by quantile_max_rows), for q = (0.5,) and
q = (0.1, 0.5, 0.9), each the median of `--runs` timed runs (events on the stream) after a warm-up:

  * quantiles   reset + rpf_quantile_append_device + rpf_quantile_select_device;
  * select      the selection alone on the stored rows: its bytes read per second, (16 + 1) K N 8 bytes per call,
                against the HBM read rate of profiles/r03_hbm_read.txt;
  * series      comparator (a): rpf_accumulate_device_series alone into a K x N buffer, so the difference prices the
                selection;
  * host        comparator (b), what users had: accumulate_series to the host plus np.quantile (wall clock, `--host-runs`
                runs: it takes seconds).
"""
import argparse
import ctypes
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
HBM_READ_GBS = 5414.0                                  # profiles/r03_hbm_read.txt
PASSES = 17                                            # 16 counting passes of 4 bits and the one for v_(j+1)


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


def summary(times):
    t = np.array(times)
    return {"us_median": float(np.median(t)) * 1e6, "us_min": float(t.min()) * 1e6, "us_max": float(t.max()) * 1e6,
            "runs": len(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantile.json"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-runs", type=int, default=1)
    ap.add_argument("--samples-log2", type=int, default=28)
    ap.add_argument("--sizes", default="64,512,4096")
    args = ap.parse_args()
    nsamples = 1 << args.samples_log2
    nbytes = 2 * nsamples
    raw = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=DEV)
    host_stream = raw.cpu().numpy() if args.host_runs > 0 else None
    res = {"device": torch.cuda.get_device_name(0), "samples": nsamples, "hbm_read_gb_per_s": HBM_READ_GBS, "cases": []}
    for N in [int(x) for x in args.sizes.split(",")]:
        F = nsamples // N
        with rpf.Datastore(rpf.Params(N=N)) as ds:
            for L in (16, 128, 1024):
                K = min(F // L, ds.quantile_max_rows)
                rows = torch.empty((K, N), dtype=torch.float64, device=DEV)
                src = raw.data_ptr()

                def series(s):
                    assert ds.accumulate_device_series(src, nbytes, L, K, rows.data_ptr(), s) == K

                case = {"N": N, "L": L, "K": K, "rows_mb": K * N * 8 / 1e6}
                case["series"] = summary(timed(series, args.runs, args.warmup))
                case["series"]["launches"] = ds.series_launches()
                for q in ((0.5,), (0.1, 0.5, 0.9)):
                    out = torch.empty((len(q), N), dtype=torch.float64, device=DEV)

                    def quantiles(s):
                        ds.quantile_reset()
                        assert ds.quantile_append_device(src, nbytes, L, K, s) == K
                        ds.quantile_select_device(q, out.data_ptr(), s)

                    def select(s):
                        ds.quantile_select_device(q, out.data_ptr(), s)

                    name = "q" + "_".join("%g" % v for v in q)
                    r = {"quantiles": summary(timed(quantiles, args.runs, args.warmup)),
                         "select": summary(timed(select, args.runs, args.warmup))}
                    # (K odd or even decides whether the median interpolates; count the pass only if some g != 0)
                    passes = PASSES if any((v * (K - 1)) % 1 for v in q) else PASSES - 1
                    r["select"]["passes"] = passes
                    r["select"]["bytes_read"] = passes * K * N * 8
                    r["select"]["gb_per_s"] = passes * K * N * 8 / (r["select"]["us_median"] * 1e-6) / 1e9
                    r["select"]["share_of_hbm_read"] = r["select"]["gb_per_s"] / HBM_READ_GBS
                    r["quantiles_over_series"] = r["quantiles"]["us_median"] / case["series"]["us_median"]
                    if host_stream is not None:
                        wall = []
                        for _ in range(args.host_runs):
                            t0 = time.perf_counter()
                            host_rows, done = ds.accumulate_series(host_stream, L, K)
                            np.quantile(host_rows, q, axis=0)
                            wall.append(time.perf_counter() - t0)
                        r["host"] = summary(wall)
                        r["host_over_quantiles"] = r["host"]["us_median"] / r["quantiles"]["us_median"]
                        del host_rows
                    case[name] = r
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
                del rows
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
