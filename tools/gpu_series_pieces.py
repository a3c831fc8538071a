#!/usr/bin/env python3
"""Wall time of the series family's host entries from a pageable stream, this build against another build of the library:

    tools/gpu_series_pieces.py --other-lib PATH [--runs 5] [--out profiles/series_pieces_host.json]

rpf_accumulate_series, rpf_accumulate_excised and rpf_quantile_append at N = 4096, cu8, L = 16 over 256 MB: four
pieces of 64 MB.  Every run is a process of its own (a library is loaded once per process) that makes its engines,
calls each entry once to grow the scratch and then times one call; the two libraries alternate.  The medians of an
entry are called equal when they differ by no more than the other library's own fastest-to-slowest spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, L, NBYTES = 4096, 16, 256 << 20
ENTRIES = ("rpf_accumulate_series", "rpf_accumulate_excised", "rpf_quantile_append")


def one_run():
    sys.path.insert(0, ROOT)
    import numpy as np
    import rtl_power_fftw_amd as rpf
    from rtl_power_fftw_amd import stats

    stream = np.random.default_rng(7).integers(0, 256, size=NBYTES, dtype=np.uint8)
    lo, hi = stats.sk_limits(L, 3.0)
    times = {}
    with rpf.Datastore(rpf.Params(N=N)) as plain, rpf.Datastore(rpf.Params(N=N, bin_stats=True)) as with_stats:
        def quantile():
            plain.quantile_reset()
            return plain.quantile_append(stream, L)
        calls = {"rpf_accumulate_series": lambda: plain.accumulate_series(stream, L)[1],
                 "rpf_accumulate_excised": lambda: with_stats.accumulate_excised(stream, L, lo, hi)[2],
                 "rpf_quantile_append": quantile}
        for name in ENTRIES:
            assert calls[name]() == NBYTES // (2 * N * L)            # the warm-up call
            t0 = time.perf_counter()
            calls[name]()
            times[name] = time.perf_counter() - t0
    print(json.dumps(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib", help="the library to compare with (RPF_ENGINE_LIB of every other run)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "series_pieces_host.json"))
    ap.add_argument("--one-run", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one_run:
        return one_run()
    seconds = {"other": {e: [] for e in ENTRIES}, "this": {e: [] for e in ENTRIES}}
    for _ in range(args.runs):
        for which in ("other", "this"):
            env = dict(os.environ)
            env.pop("RPF_ENGINE_LIB", None)
            if which == "other":
                env["RPF_ENGINE_LIB"] = os.path.abspath(args.other_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one-run"], env=env, capture_output=True,
                               text=True, timeout=300, check=True)
            for e, t in json.loads(r.stdout.strip().splitlines()[-1]).items():
                seconds[which][e].append(t)
    result = {"N": N, "L": L, "nbytes": NBYTES, "format": "cu8", "pieces": 4, "runs": args.runs, "seconds": seconds, "entries": {}}
    for e in ENTRIES:
        other, this = seconds["other"][e], seconds["this"][e]
        spread = max(other) - min(other)
        diff = statistics.median(this) - statistics.median(other)
        result["entries"][e] = {"median_other": statistics.median(other), "median_this": statistics.median(this),
                                "difference": diff, "spread_other": spread, "within_spread": abs(diff) <= spread}
        print("%-24s other %.4f s, this %.4f s: %+.4f s against a spread of %.4f s" %
              (e, statistics.median(other), statistics.median(this), diff, spread))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
