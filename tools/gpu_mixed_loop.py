#!/usr/bin/env python3
"""Records the frame loops of the mixed-radix family -> profiles/mixed_loop.json ("Mixed-radix kernels").

For every case of tests/test_gpu_mixed_loop.py -- every (size, window) of mixed_plans.inc and mixed_plans_split.inc and six
Stockham sizes, two and a half loop iterations of the resident grid each -- that file's own figure function, so the record
and the test cannot drift apart: the geometry (grid, frames per workgroup, split factor P, frames per iteration I), the
frames F and bytes of the stream, the whole run against float64 with the bar that applied and which it was, the whole
run against the sum of its first-iteration parts, whether a second run was bit-identical, the first part against the
Bluestein engine where no other test launches the size, what a stale prefetch or an unmasked slot would have moved the
truth by at that geometry, and the seconds the case took.  "worst" sums them up.

The record is written after every case; --resume keeps the cases an earlier run of the same tables recorded."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_mixed_loop as gpu                     # noqa: E402
from parity_bars import ADDITIVITY, PARITY            # noqa: E402


def label(r):
    return {k: r[k] for k in ("N", "windowed", "form")}


def passes(r):
    return (r["whole_vs_truth"] < r["bar"] and r["whole_vs_parts"] < ADDITIVITY and r["judged_grid"] == r["grid"]
            and (r["second_run_equal"] or (r["fused_four_step"] and r["second_run_vs_first"] < ADDITIVITY))
            and r.get("first_part_vs_bluestein", 0.0) < PARITY)


def worst_of(rows):
    def top(key, some=rows):
        r = max(some, key=key)
        return {"value": key(r), "at": label(r)}
    checked = [r for r in rows if "first_part_vs_bluestein" in r]
    return {"whole_vs_truth_over_bar": top(lambda r: r["whole_vs_truth"] / r["bar"]),
            "whole_vs_parts": top(lambda r: r["whole_vs_parts"]),
            "first_part_vs_bluestein": top(lambda r: r["first_part_vs_bluestein"], checked) if checked else None,
            "bytes": top(lambda r: r["bytes"]), "seconds": top(lambda r: r["seconds"]),
            "least_bars_a_stale_prefetch_would_move_the_truth": -top(lambda r: -r["stale_prefetch_would_move_truth_by"] / r["bar"])["value"],
            "least_bars_an_unmasked_slot_would_move_the_truth": -top(lambda r: -r["unmasked_slot_would_move_truth_by"] / r["bar"])["value"],
            "second_run_bit_identical": sum(r["second_run_equal"] for r in rows),
            "judged_at_twice_the_cpu_float32_path": [label(r) for r in rows if r["bar_is"] != "table"],
            "cases": len(rows), "cases_within_every_bar": sum(passes(r) for r in rows),
            "outside_a_bar": [label(r) for r in rows if not passes(r)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_loop.json"))
    ap.add_argument("--resume", action="store_true")
    args = ap.parse_args()
    import torch
    res = {"device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
           "bars": {"ADDITIVITY": ADDITIVITY, "PARITY": PARITY}, "cases": []}
    if args.resume and os.path.exists(args.out):
        with open(args.out) as f:
            res["cases"] = json.load(f)["cases"]
    have = {(r["N"], r["windowed"]) for r in res["cases"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    t0 = time.time()
    for case in gpu.CASES:
        if case in have:
            continue
        r = gpu.loop_figures(case)
        res["cases"].append(r)
        print(gpu.describe(r), flush=True)
        res["cases"].sort(key=lambda r: (r["N"], r["windowed"]))
        res["worst"] = worst_of(res["cases"])
        with open(args.out + ".part", "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        os.replace(args.out + ".part", args.out)
    print("%d cases in %.1f s" % (len(res["cases"]), time.time() - t0), flush=True)
    print(json.dumps(worst_of(res["cases"]), indent=1))


if __name__ == "__main__":
    main()
