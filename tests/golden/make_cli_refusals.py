#!/usr/bin/env python3
"""Records tests/golden/cli_refusals.json: exit code and message of rpf_host_parse (librpf_host.so: no device is
opened) for the command lines below, and the text of `rpf_power --help`.  Run it on a BUILD OF THE COMMIT WHOSE ANSWERS
ARE THE YARDSTICK, never on the code under change (the fixture in git is from the commit before the replay modes' table:
a checkout of it elsewhere, built there), from this repository's root:

    python tests/golden/make_cli_refusals.py <that checkout>/rtl-power-fftw_amd/host <its commit> [OUTPUT.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import test_cli_refusals as t  # noqa: E402

IN = "--input /dev/null "
GOOD = {                                   # mode -> its option on a good line
    "series": "--series 4", "series-stats": "--series-stats 4", "excise": "--excise 4", "quantile": "--quantile 4",
    "stft": "--stft /dev/null", "cross": "--cross /dev/null",
}
BESIDE = ["-n 10", "-t 1", "-c", "-e 10", "-f 100M:200M", "-m out", "--gpus 0,1", "--stats", "--pfb 4", "-w /dev/null",
          "--frame-overlap 50", "--format cf32"]


def one_fault_lines():
    lines = []
    for mode, good in GOOD.items():
        lines += [IN + good, good]
        lines += [IN + good + " " + other for other in BESIDE]
        for other, its in GOOD.items():
            if other != mode:
                lines += [IN + good + " " + its, IN + its + " " + good]
        if good.endswith(" 4"):
            lines += [IN + "--%s %s" % (mode, frames) for frames in ("0", "1", "x")]
        lines.append(IN + "--" + mode)
    lines += ["--excise-sigma 2"] + [IN + "--excise 4 --excise-sigma " + v for v in ("2", "0", "-1", "inf", "nan", "x")]
    lines += ["--quantiles 0.5"] + [IN + "--quantile 4 --quantiles " + v
                                    for v in ("0.25,0.5,0.75", "0.5,x", "1.5", "0.5,", ",".join(["0.5"] * 8),
                                              ",".join(["0.5"] * 9))]
    lines += [IN + "--stft /dev/null -b 500", IN + "--stft /dev/null -b 512", "--input - --cross -", "--input - --cross /dev/null"]
    lines += ["--pfb 4", "--pfb 0", "--pfb 33", "--pfb x", "--pfb", "--pfb 4 -w /dev/null", "--pfb 4 --frame-overlap 50",
              "--pfb 4 --stats", IN + "--pfb 4 --series 4", IN + "--pfb 4 --series-stats 4", IN + "--pfb 4 --excise 4",
              "--pfb 4 --gpus 0,1", "--pfb 4 --gpu 1"]
    return sorted(set(lines), key=lines.index)          # (a pair of modes comes up from either side)


# two faults in one mode's block: the line, and the two lines above with one of the faults each
SAME_BLOCK = [
    ("--series 4 -n 10", "--series 4", IN + "--series 4 -n 10"),
    (IN + "--series-stats 4 -f 100M:200M --gpus 0,1", IN + "--series-stats 4 -f 100M:200M", IN + "--series-stats 4 --gpus 0,1"),
    (IN + "--excise 1 -m out", IN + "--excise 1", IN + "--excise 4 -m out"),
    (IN + "--excise 4 --excise-sigma -1 -t 1", IN + "--excise 4 --excise-sigma -1", IN + "--excise 4 -t 1"),
    (IN + "--quantile 4 --quantiles 1.5 --stats", IN + "--quantile 4 --quantiles 1.5", IN + "--quantile 4 --stats"),
    (IN + "--quantile 4 --pfb 4 -f 100M:200M", IN + "--quantile 4 --pfb 4", IN + "--quantile 4 -f 100M:200M"),
    (IN + "--stft /dev/null -b 500 -c", IN + "--stft /dev/null -b 500", IN + "--stft /dev/null -c"),
    (IN + "--stft /dev/null --cross /dev/null -m out", IN + "--stft /dev/null --cross /dev/null", IN + "--stft /dev/null -m out"),
    ("--input - --cross - -e 10", "--input - --cross -", IN + "--cross /dev/null -e 10"),
    (IN + "--cross /dev/null --gpus 0,1 -m out", IN + "--cross /dev/null --gpus 0,1", IN + "--cross /dev/null -m out"),
]
# faults in two blocks: the earlier block speaks, so these are exact like the lines with one fault
TWO_BLOCKS = [
    IN + "--series 4 --excise 4 -n 10",
    IN + "--series 0 --quantile 0",
    IN + "--pfb 4 --stats --quantile 4",
    IN + "--stats -m out --series 4",
    IN + "--excise-sigma 2 --series 4 -n 10",
    IN + "--quantiles 0.5 --excise 4 -c",
    IN + "--series 4 --series-stats 4 -n 10",
    IN + "--excise 4 --cross /dev/null -m out",
    "--quantile 4 --stft /dev/null -b 500",
]


def main():
    host_dir, commit = sys.argv[1], sys.argv[2]
    assert os.path.abspath(host_dir) != os.path.abspath(t.HOST_DIR), "record this on a build of the yardstick commit"
    lines = {}
    for line in one_fault_lines() + [s[0] for s in SAME_BLOCK] + TWO_BLOCKS:
        assert line not in lines, line
        code, message = t.parse(host_dir, line)
        lines[line] = {"code": code, "message": message if code else ""}
    for line, first, second in SAME_BLOCK:
        lines[line]["either"] = [first, second]
        assert lines[line]["message"] in (lines[first]["message"], lines[second]["message"]), line
        assert lines[first]["code"] and lines[second]["code"] and lines[first]["message"] != lines[second]["message"], line
    path = sys.argv[3] if len(sys.argv) > 3 else t.FIXTURE
    with open(path, "w") as f:
        json.dump({"commit": commit, "help": t.help_text(host_dir), "lines": lines}, f, indent=0)
        f.write("\n")
    print("wrote %s: %d lines, %d refused" % (path, len(lines), sum(1 for v in lines.values() if v["code"])))


if __name__ == "__main__":
    main()
