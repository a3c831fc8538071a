#!/usr/bin/env python3
"""Records the batch seam of the catch-all route -> profiles/seams_errors.json (README.md, the seam paragraphs of
"Sample formats" and "Per-bin statistics").

For every case of tests/test_gpu_seams.py section 1 -- 500, 4096 (catch-all), 40000 and 65536 bins x cu8, cs8, cs16,
cf32 x rectangular / raised Hann x statistics off / on, 2 B + 5 frames each -- that file's own figure function, so the
record and the test cannot drift apart: the batch the engine reported and the frames it ran; S1 against float64 relative
to max(bin, median bin); with statistics the worst per-bin relative errors of S1, S2, PK of the GPU and of the CPU float32
path against float64 and their ratio; the whole run against the sum of its three parts; and every exact comparison
(peak of the parts, second run, plain engine, format tie) as a flag.  "worst" sums them up, the S2 and PK ratios by
transform: the power-of-two lengths, where the test asserts them, and the Bluestein lengths, where it records them.
"gather" holds the two cases of section 3 (two chunks of gathered frames against the materialised stream and float64).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_seams as seams                        # noqa: E402

FLAGS = ("pk_is_the_maximum_of_the_parts", "second_run_of_the_last_part_equal", "s1_is_the_plain_engines_power")


def label(r):
    return {k: r[k] for k in ("N", "format", "window", "statistics")}


def worst_of(rows):
    out = {"S1_err_over_mean": max(rows, key=lambda r: r["S1_err_over_mean"]), "whole_vs_parts": {}, "gpu_over_cpu": {},
           "gpu_vs_truth": {}, "cpu_f32_vs_truth": {}}
    out["S1_err_over_mean"] = {"value": out["S1_err_over_mean"]["S1_err_over_mean"], "at": label(out["S1_err_over_mean"])}
    for k in ("S1", "S2"):
        r = max((r for r in rows if k in r["whole_vs_parts"]), key=lambda r: r["whole_vs_parts"][k])
        out["whole_vs_parts"][k] = {"value": r["whole_vs_parts"][k], "at": label(r)}
    with_stats = [r for r in rows if r["statistics"]]
    for transform in ("power_of_two", "bluestein"):
        some = [r for r in with_stats if r["transform"] == transform]
        for key in ("gpu_over_cpu", "gpu_vs_truth", "cpu_f32_vs_truth"):
            out[key][transform] = {}
            for k in ("S2", "PK"):
                r = max(some, key=lambda r: r[key][k])
                out[key][transform][k] = {"value": r[key][k], "at": label(r)}
    out["every_exact_comparison_holds"] = all(r[f] for r in rows for f in FLAGS if f in r) and \
        all(r["tie"]["equal"] for r in rows if "tie" in r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seams_errors.json"))
    args = ap.parse_args()
    import torch
    res = {"device": torch.cuda.get_device_name(0),
           "bars": {"ADDITIVITY": seams.ADDITIVITY, "PARITY": seams.PARITY, "STATS_TIMES_CPU_ERR": seams.STATS_TIMES_CPU_ERR},
           "S2_PK_ratio_asserted_at": "power_of_two", "cases": []}
    t0 = time.time()
    for case in seams.CASES:
        res["cases"].append(seams.batch_seam_figures(*case))
        print(res["cases"][-1], flush=True)
    res["worst"] = worst_of(res["cases"])
    res["gather"] = [seams.gather_seam_figures(*case) for case in sorted(seams.GATHER_CHUNK)]
    print("%d cases in %.1f s" % (len(res["cases"]), time.time() - t0), flush=True)
    print(json.dumps(res["worst"], indent=1))
    print(res["gather"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
