#!/usr/bin/env python3
"""Records the STFT rows' error against float64 at every K1 size x window x format (the plain kernel with LDS-DMA
staging) and on the catch-all route from 2 to 2^22 bins -> profiles/stft_forms_errors.json (README.md, "Short-time
Fourier transform", Accuracy).  The cases, streams and judged rows are tests/stft_forms_bars.py's and the figures come
from tests/test_gpu_stft_forms.py's own functions, so the record and the tests cannot drift apart.

`--cpu-only` opens no device: it computes err of the CPU float32 path (rpf_oracle_fft_f32) on every case's judged rows
and prints the CPU_F32 dict to paste into stft_forms_bars.py -- how the bars get fixed before any device run.  The rows
a K1 case judges depend on the store kernels' resident grid: `--geometry` asks a device for it and prints the GEOMETRY
dict, which has to be in place first.  Without a flag every case runs on the device; per case the file holds err, the
CPU figure, their ratio, grid x frames per workgroup, the frame count, the staging route, the judged rows and the worst
row and bin, and the MEASURED dict is printed to paste."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stft_forms_bars as bars                        # noqa: E402


def print_dict(name, d, fmt):
    items = ["%r: %s" % (k, fmt(v)) for k, v in d.items()]
    print("%s = {%s}" % (name, ",\n    ".join(", ".join(items[i:i + 3]) for i in range(0, len(items), 3))))


def label(case):
    return {"format": case[0], "N": case[1], "window": case[2]}


def cpu_side():
    out, rows = {}, []
    for case in bars.K1_CASES + bars.CATCH_ALL_CASES:
        t0 = time.time()
        frames, want = bars.references(bars.judged_frames(case), case)
        power = want.real ** 2 + want.imag ** 2
        assert power.min() > 0, (case, "a judged bin of power 0: the identity check asks for min > 0")
        out[case] = bars.stft_bars.err(bars.stft_bars.cpu_f32_rows(frames), want)
        rows.append(dict(label(case), cpu_f32=out[case], seconds=round(time.time() - t0, 2)))
        print(rows[-1], flush=True)
    print_dict("CPU_F32", out, lambda v: "%.3e" % v if v else "0.0")
    print("largest CPU figure %.3e; exact: %s" % (max(out.values()), [c for c, v in out.items() if v == 0]))
    return rows


def geometry():
    import test_gpu_stft_forms as forms
    out = {}
    for case in bars.K1_CASES:
        with forms.engine(case[1], case[0], case[2] == "hann") as ds:
            li = forms.resident_grid(ds)
        out[case] = (li["grid"], li["frames_per_wg"])
    print_dict("GEOMETRY", out, repr)


def gpu_side():
    import test_gpu_stft_forms as forms
    rows, measured = [], {}
    for route, cases, figures in (("k1", bars.K1_CASES, forms.k1_plain_figures),
                                  ("catch_all", bars.CATCH_ALL_CASES, forms.catch_all_figures)):
        for case in cases:
            t0 = time.time()
            fig = figures(case, check=False)
            measured[case] = fig["err"]
            rows.append(dict(label(case), route=route, seconds=round(time.time() - t0, 2), **fig))
    print_dict("MEASURED", measured, lambda v: "%.3e" % v if v else "0.0")
    worst = {}
    for route in ("k1", "catch_all"):
        mine = [r for r in rows if r["route"] == route]
        by_err = max(mine, key=lambda r: r["err"])
        by_ratio = max((r for r in mine if r["ratio"] is not None), key=lambda r: r["ratio"])
        worst[route] = {"err": dict(label((by_err["format"], by_err["N"], by_err["window"])), value=by_err["err"]),
                        "ratio": dict(label((by_ratio["format"], by_ratio["N"], by_ratio["window"])), value=by_ratio["ratio"])}
    return rows, worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stft_forms_errors.json"))
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--geometry", action="store_true")
    args = ap.parse_args()
    if args.geometry:
        return geometry()
    res = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    res["bars"] = {"fine": "2 x cpu_f32", "COARSE": bars.COARSE,
                   "recorded_not_asserted": ["%s-%d-%s" % c for c in bars.RECORDED_NOT_ASSERTED]}
    t0 = time.time()
    if args.cpu_only:
        res["cpu_side"] = cpu_side()
    else:
        import torch
        res["device"] = torch.cuda.get_device_name(0)
        res["gpu"], res["worst"] = gpu_side()
    print("%d cases in %.1f s" % (len(res["cpu_side" if args.cpu_only else "gpu"]), time.time() - t0), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
