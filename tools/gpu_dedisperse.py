#!/usr/bin/env python3
"""Measures the incoherent dedispersion of the stored integrations on the GPU -> profiles/dedisperse.json (README.md,
"Dedispersion").

One device-resident cu8 stream of 2^26 samples, N = 64, 256 and 4096, L = 16 and 128 frames per integration, D = 32 and
256 trials; the DM tables are dedisperse.dm_delays at 408 MHz / 2.4 MS/s, the trials evenly spaced from 0 so that
neighbouring trials differ by one row at the lowest bin (the usual DM step): the largest delay is D - 1 rows, or a
quarter of the stored rows where that is less.  Warm-up, then `--runs` timed runs per case (events
on the stream): the median, the smallest and the largest.  Per case:
  dedisperse  the whole rpf_dedisperse_device call on the filled store, events around it on an idle stream: the host's
              share (the spans, the pinned fill; the start event has fired by then), the upload and the one launch
  device      the same call with events, but behind eight 2 GiB copies that keep the device at work while the host
              prepares: what the call put on the stream, the table's upload and the launch, without the host's share
  host        wall clock of the call, which returns without synchronising: the host's share alone
  append      (a) rpf_quantile_append_device alone (the reset before it is outside the bracket): filling the store
  copy        (b) a device-to-device copy of a torch buffer of the stored rows' size, K N 8 bytes (the store itself is
              the engine's and is not copied): the bandwidth yardstick
  numpy       (c) dedisperse.reference on the host, wall clock, ONE run over at most --numpy-times times, scaled to T
Reported: bytes of rows per second of the dedisperse call; that rate against (b); the rows the tiling implies are read
(trial tiles x rows, D / DT x K N 8 bytes, the staged overlap not counted) per second against (b); and the share of
(tile, block) pairs that took the direct route (csrc/dedisperse_core.h's span rule, from the test emulator library).
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
from rtl_power_fftw_amd import dedisperse             # noqa: E402

DEV = torch.device("cuda:0")
FC, RATE = 408e6, 2.4e6


def timed(enqueue, runs, warmup=3, before=None, busy=None):
    """Median, smallest and largest of `runs` event-timed runs of enqueue(stream).  before(): host work outside the
    bracket.  busy: (dst, src, times) copies enqueued ahead of the first event, so that the device is still at work
    while the host prepares the call and the bracket holds what the call put on the stream, not the host's share."""
    s = torch.cuda.current_stream()
    times = []
    for k in range(warmup + runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if before:
            before()
        if busy:
            for _ in range(busy[2]):
                busy[0].copy_(busy[1])
        a.record(s)
        enqueue(s.cuda_stream)
        b.record(s)
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(times)), float(min(times)), float(max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dedisperse.json"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--samples-log2", type=int, default=26)
    ap.add_argument("--numpy-times", type=int, default=256)
    args = ap.parse_args()
    emul = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "librpf_emul_dedisperse.so"))
    emul.rpf_emul_dedisperse_direct_pairs.restype = ctypes.c_longlong
    emul.rpf_emul_dedisperse_direct_pairs.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    DT = emul.rpf_emul_dedisperse_dt()
    nsamples = 1 << args.samples_log2
    nbytes = 2 * nsamples
    raw = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=DEV)
    big = torch.zeros((2, 1 << 28), dtype=torch.float64, device=DEV)          # 2 GiB each: a copy takes about 1.5 ms
    res = {"device": torch.cuda.get_device_name(0), "samples": nsamples, "runs": args.runs, "fc_hz": FC, "rate": RATE,
           "tile": {"TT": emul.rpf_emul_dedisperse_tt(), "DT": DT, "BC": emul.rpf_emul_dedisperse_bc()}, "cases": []}
    for N in (64, 256, 4096):
        for L in (16, 128):
            with rpf.Datastore(rpf.Params(N=N)) as ds:
                K = ds.frames_in(nbytes) // L
                append, append_min, append_max = timed(lambda s: ds.quantile_append_device(raw.data_ptr(), nbytes, L, K, s),
                                                       args.runs, before=ds.quantile_reset)
                assert ds.quantile_rows == K
                rows_bytes = K * N * 8
                src = torch.empty(K * N, dtype=torch.float64, device=DEV)
                dst = torch.empty_like(src)
                copy, copy_min, copy_max = timed(lambda s: dst.copy_(src), args.runs)
                del src, dst
                copy_rate = rows_bytes / copy
                median = ds.quantile_select([0.5])[0]
                w = np.where(median != 0, 1.0 / np.where(median != 0, median, 1.0), 0.0)
                w[N // 2] = 0.0
                for D in (32, 256):
                    want = min(D - 1, K // 4)
                    per_dm = dedisperse.dm_delays([1.0e4], FC, RATE, N, L).max() / 1.0e4
                    dms = np.linspace(0.0, want / per_dm, D)
                    delays = dedisperse.dm_delays(dms, FC, RATE, N, L)
                    T = ds.dedisperse_times(delays)
                    out = torch.empty(D * T, dtype=torch.float64, device=DEV)
                    call = lambda s: ds.dedisperse_device(delays, w, out.data_ptr(), out.numel(), s)      # noqa: E731
                    t, t_min, t_max = timed(call, args.runs)
                    g, g_min, g_max = timed(call, args.runs, busy=(big[0], big[1], 8))
                    host = []
                    for _ in range(args.runs):
                        t0 = time.perf_counter()
                        call(torch.cuda.current_stream().cuda_stream)
                        host.append(time.perf_counter() - t0)
                        torch.cuda.synchronize()
                    pairs = ctypes.c_longlong(0)
                    direct = emul.rpf_emul_dedisperse_direct_pairs(delays.ctypes.data, w.ctypes.data, N, D, ctypes.byref(pairs))
                    # (c) numpy on the host, over the first rows only
                    t_host = min(T, args.numpy_times)
                    host_rows = np.random.default_rng(1).random((t_host + int(delays.max()), N))
                    t0 = time.perf_counter()
                    dedisperse.reference(host_rows, delays, w)
                    numpy_s = (time.perf_counter() - t0) * (T / t_host)
                    tiles = -(-D // DT)
                    case = {"N": N, "L": L, "D": D, "K": int(K), "T": int(T), "dm_top": float(dms[-1]), "largest_delay": int(delays.max()),
                            "rows_bytes": rows_bytes,
                            "dedisperse_seconds_median": t, "dedisperse_seconds_min": t_min, "dedisperse_seconds_max": t_max,
                            "device_seconds_median": g, "device_seconds_min": g_min, "device_seconds_max": g_max,
                            "host_seconds_median": float(np.median(host)),
                            "device_rows_gb_per_s": rows_bytes / g * 1e-9, "device_rows_rate_over_copy": rows_bytes / g / copy_rate,
                            "device_tiled_rows_rate_over_copy": tiles * rows_bytes / g / copy_rate,
                            "append_seconds_median": append, "append_seconds_min": append_min, "append_seconds_max": append_max,
                            "copy_seconds_median": copy, "copy_seconds_min": copy_min, "copy_seconds_max": copy_max,
                            "dedisperse_over_append": t / append,
                            "rows_gb_per_s": rows_bytes / t * 1e-9, "copy_rows_gb_per_s": copy_rate * 1e-9,
                            "rows_rate_over_copy": rows_bytes / t / copy_rate,
                            "tiled_rows_gb_per_s": tiles * rows_bytes / t * 1e-9,
                            "tiled_rows_rate_over_copy": tiles * rows_bytes / t / copy_rate,
                            "direct_pairs": int(direct), "pairs": int(pairs.value),
                            "direct_share": direct / pairs.value if pairs.value else 0.0,
                            "numpy_host_seconds_scaled": numpy_s, "numpy_over_dedisperse": numpy_s / t}
                    res["cases"].append(case)
                    print(case, flush=True)
                    del out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
