#!/usr/bin/env python3
"""Records K1's derived kernels against float64 truth at all sixteen size x window forms -> profiles/k1_forms_errors.json
(README.md, the "Accuracy" sentences of Sample formats, Per-bin statistics, Spectrogram, Time-resolved statistics).

For every form (N = 64 ... 8192, rectangular or Hann) and every family of tests/test_gpu_k1_forms.py -- statistics
planes (cu8, cs16; LDS-DMA and VGPR staging), cs16 on the plain kernel, the strided kernel (steps N/2 and N/2 + 1; cu8,
cs16), series rows (cu8; cs16 at the windowed forms), series-of-statistics rows (cu8; both staging routes) -- the worst
per-bin relative error against float64 truth of the GPU and of the CPU float32 path on the same frames: that file's own
figure functions, so the record and the tests cannot drift apart.  "worst" sums up each family over the sixteen forms.

`--cpu-only` runs the CPU halves alone (no device is opened): the precondition of every case -- the CPU float32 path
holds the bar on the chosen stream and frame count -- with the series' K taken from the resident grid recorded in
tests/golden/k1_launch_geometry.json.  `--part` picks one family so that each fits a time limit of its own; the parts
merge into one file.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_k1_forms as forms                     # noqa: E402

PARTS = ("stats", "formats", "strided", "series", "series_stats")


def recorded_series_case(N, window):
    """(L, K, grid, fpw) as forms.series_case() gives it on the device whose launch geometry the fixture records."""
    with open(os.path.join(ROOT, "tests", "golden", "k1_launch_geometry.json")) as f:
        rec = json.load(f)["records"]["n%d_cu8_%s_series" % (N, "hann" if window else "rect")]
    L = forms.row_frames_of(N, window)
    return L, forms.series_plan(rec["grid"], rec["frames_per_wg"], L), rec["grid"], rec["frames_per_wg"]


def cpu_side(part, N, window):
    """The CPU float32 path against float64 truth for every case of `part` at one form."""
    label = {"N": N, "window": bool(window)}
    if part == "stats":
        return [dict(label, format=fmt, frames=forms.frames_of(N, window),
                     cpu_f32_vs_truth=forms.stats_reference(N, window, fmt)["cpu_f32_vs_truth"]) for fmt in ("cu8", "cs16")]
    if part == "formats":
        return [dict(label, format="cs16", frames=forms.frames_of(N, window),
                     cpu_f32_vs_truth=forms.cs16_reference(N, window)["cpu_vs_truth"])]
    if part == "strided":
        return [dict(label, format=fmt, step=step, frames=forms.frames_of(N, window),
                     cpu_f32_vs_truth=forms.strided_reference(N, window, fmt, step)["cpu_vs_truth"])
                for fmt in ("cu8", "cs16") for step in forms.strided_steps(N)]
    if part == "series":                               # (S1, S2, PK: the series of statistics judges the same rows)
        L, K, _, _ = recorded_series_case(N, window)
        return [dict(label, format=fmt, L=L, K=K,
                     cpu_f32_vs_truth=forms.series_reference(N, window, fmt, L, K)["cpu_f32_vs_truth"])
                for fmt in (("cu8", "cs16") if window else ("cu8",))]
    return []


def gpu_side(part, N, window):
    if part == "stats":
        return [forms.stats_figures(N, window, fmt, flags) for fmt in ("cu8", "cs16") for flags in (0, forms.NO_DMA)]
    if part == "formats":
        return [forms.formats_figures(N, window)]
    if part == "strided":
        return [forms.strided_figures(N, window, fmt, step) for fmt in ("cu8", "cs16") for step in forms.strided_steps(N)]
    case = forms.series_case(N, window)
    if part == "series":
        return [forms.series_figures(N, window, fmt, case) for fmt in (("cu8", "cs16") if window else ("cu8",))]
    return [forms.series_stats_figures(N, window, flags, case) for flags in (0, forms.NO_DMA)]


def worst_of(rows, key):
    """The largest figure `key` of a family over its rows, per statistic where the figure is a dict, and where it is."""
    out = {}
    for r in rows:
        fig = r[key] if isinstance(r[key], dict) else {"S1": r[key]}
        for k, v in fig.items():
            if k not in out or v > out[k]["value"]:
                out[k] = {"value": v, "at": {x: r[x] for x in ("N", "window", "format", "staging", "step") if x in r}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k1_forms_errors.json"))
    ap.add_argument("--part", choices=PARTS + ("all",), default="all")
    ap.add_argument("--cpu-only", action="store_true")
    args = ap.parse_args()

    res = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    res["bars"] = {"VS_TRUTH": forms.VS_TRUTH, "STATS_TIMES_CPU_ERR": forms.STATS_TIMES_CPU_ERR}
    if not args.cpu_only:
        import torch
        res["device"] = torch.cuda.get_device_name(0)
    section = "cpu_side" if args.cpu_only else "gpu"
    res.setdefault(section, {})
    for part in PARTS if args.part == "all" else (args.part,):
        if args.cpu_only and part == "series_stats":
            continue                                   # (its rows are the series' rows)
        t0 = time.time()
        rows = []
        for N, window in forms.FORMS:
            rows += (cpu_side if args.cpu_only else gpu_side)(part, N, window)
            print(rows[-1], flush=True)
        res[section][part] = rows
        res.setdefault("worst", {}).setdefault(section, {})[part] = {
            key: worst_of(rows, key) for key in (("cpu_f32_vs_truth",) if args.cpu_only else
                                                 ("gpu_vs_truth", "cpu_f32_vs_truth") if part != "formats" else
                                                 ("cs16_gpu_vs_truth", "cs16_cpu_f32_vs_truth"))}
        print("%s: %d cases in %.1f s" % (part, len(rows), time.time() - t0), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
