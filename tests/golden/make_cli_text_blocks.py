#!/usr/bin/env python3
"""Records tests/golden/cli_text_blocks.json: the inputs below and the text that the block writers and headers of the
C++ host (the rpf_host_format_* shims of librpf_host.so) make of them.  Run it on a BUILD OF THE COMMIT WHOSE TEXT IS THE
YARDSTICK, never on the code under change (the fixture in git is from the commit before the shared header and row loop,
with the one shim it lacked, rpf_host_format_header_mode, added to that checkout for the recording), from this
repository's root:

    python tests/golden/make_cli_text_blocks.py <that checkout>/rtl-power-fftw_amd/host <its commit> [OUTPUT.json]

8 bins: the smallest block whose DC bin (4) has both neighbours and a row on either side of them.  Nothing below is
symmetric about the DC bin, whose own values are off the scale of the rest, so an interpolation left out shows.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import test_cli_text_blocks as t  # noqa: E402

N = 8
PWR = [3500.0, 1250.0, 7000.0, 2000.0, 900000.0, 4500.0, 750.0, 9000.0]
REPEATS = 16
SUM_SQ = [p * p / REPEATS * (1.5 + 0.25 * i) for i, p in enumerate(PWR)]
PEAK = [p * (0.2 + 0.03 * i) for i, p in enumerate(PWR)]
BASELINE = [-1.5, 0.25, 2.0, -0.125, 7.0, 0.5, -3.0, 1.0]
K, L = 4, 5
KEPT = [4.0, 3.0, 0.0, 4.0, 1.0, 2.0, 4.0, 1.0]                       # (bin 2: no integration kept)
TOTAL = [p * K * L / REPEATS for p in PWR]
CLEAN = [t_ * k / K * (0.9 - 0.02 * i) for i, (t_, k) in enumerate(zip(TOTAL, KEPT))]
Q3 = [0.1, 0.5, 0.975]
QUANTILE_PLANES = [p * s * (1 + 0.01 * i) for s in (0.4, 1.0, 2.5) for i, p in enumerate(PWR)]
SBB = [p * (0.5 + 0.2 * i) for i, p in enumerate(PWR)]
RE_AB = [300.0, -900.0, 0.0, 1500.0, -40000.0, 0.0, 500.0, -2500.0]    # (bin 2: zero cross-power; bin 5: imaginary only)
IM_AB = [-1200.0, 400.0, 0.0, 700.0, 90000.0, -2100.0, 0.0, 3000.0]
TUNINGS = [(100000000, 2000000), (1420405752, 2400000)]                # (the frequency column: 6 and 7 digits)

WRITERS = {
    "plain": dict(writer="plain", pwr=PWR, repeats=REPEATS),
    "stats": dict(writer="stats", pwr=PWR, sum_sq=SUM_SQ, peak=PEAK, repeats=REPEATS),
    "excised": dict(writer="excised", clean=CLEAN, kept=KEPT, total=TOTAL, K=K, L=L),
    "quantiles_1": dict(writer="quantiles", planes=QUANTILE_PLANES[N:2 * N], q=[0.5], L=L),
    "quantiles_3": dict(writer="quantiles", planes=QUANTILE_PLANES, q=Q3, L=L),
    "cross": dict(writer="cross", planes=PWR + SBB + RE_AB + IM_AB, frames=REPEATS),
}


def main():
    host_dir, commit = sys.argv[1], sys.argv[2]
    assert os.path.abspath(host_dir) != os.path.abspath(t.HOST_DIR), "record this on a build of the yardstick commit"
    lib = t.host_lib(host_dir)
    cases = {}
    recording = {"commit": commit, "N": N, "baseline": BASELINE, "inputs": WRITERS, "cases": cases}
    for name in WRITERS:
        for tuned, rate in TUNINGS:
            for linear in (0, 1):
                for baseline in (None, BASELINE):
                    case = dict(inputs=name, tuned=tuned, rate=rate, linear=linear, baseline=baseline is not None)
                    case["text"] = t.render(lib, t.whole_case(recording, case))
                    cases["%s_%d_%s%s" % (name, tuned, "linear" if linear else "dB", "_baseline" if baseline else "")] = case
    recording["headers"] = {kind: t.render_header(lib, kind) for kind in ("plain", "stats", "excised", "cross")}
    path = sys.argv[3] if len(sys.argv) > 3 else t.FIXTURE
    with open(path, "w") as f:
        json.dump(recording, f, indent=0)
        f.write("\n")
    print("wrote %s: %d blocks, %d headers" % (path, len(cases), len(recording["headers"])))


if __name__ == "__main__":
    main()
