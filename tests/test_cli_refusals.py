"""What the command line refuses, as the build before the replay modes' table refused it: exit code and message of
rpf_host_parse (librpf_host.so, which opens no device) for every command line of tests/golden/cli_refusals.json, and the
text of `rpf_power --help`.  tests/golden/make_cli_refusals.py holds the list and recorded it from a build of the commit
the file names.  Code and message are equal for every line; a line with two faults inside ONE mode's block ("either":
the two lines with one of the faults each) keeps its code and gives the message of one of the two, since the table
checks a block's faults in one order for all modes -- which block speaks, with faults in two blocks, is part of the
exact lines."""
import ctypes
import json
import os
import subprocess

import pytest
import torch  # noqa: F401  (same HIP runtime for librpf_engine.so, see _lib.load)

from helpers import GOLDEN, ROOT

FIXTURE = os.path.join(GOLDEN, "cli_refusals.json")
HOST_DIR = os.path.join(ROOT, "rtl-power-fftw_amd", "host")


def parse(host_dir, line):
    """(exit code, message) of the command line `line` (options separated by blanks); the message of code 0 is ""."""
    lib = ctypes.CDLL(os.path.join(host_dir, "librpf_host.so"))
    args = line.split()
    argv = (ctypes.c_char_p * (len(args) + 1))(b"rpf_power", *[a.encode() for a in args])
    i = [ctypes.c_int() for _ in range(6)]
    ll = [ctypes.c_longlong() for _ in range(4)]
    d = ctypes.c_double()
    msg = ctypes.create_string_buffer(4096)
    rc = lib.rpf_host_parse(len(args) + 1, argv, ctypes.byref(i[0]), ctypes.byref(i[1]), ctypes.byref(i[2]),
                            ctypes.byref(ll[0]), ctypes.byref(i[3]), ctypes.byref(ll[1]), ctypes.byref(ll[2]),
                            ctypes.byref(ll[3]), ctypes.byref(i[4]), ctypes.byref(d), msg, len(msg))
    return rc, msg.value.decode()


def help_text(host_dir):
    r = subprocess.run([os.path.join(host_dir, "rpf_power"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    return r.stdout


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_list_is_what_the_issue_asked_for(golden):
    lines = golden["lines"]
    assert len(lines) >= 150 and len(set(lines)) == len(lines)
    either = {k: v for k, v in lines.items() if "either" in v}
    assert len(either) >= 6 and all(len(v["either"]) == 2 and set(v["either"]) <= set(lines) for v in either.values())
    for mode in ("series", "series-stats", "excise", "quantile", "stft", "cross"):
        good = [k for k, v in lines.items() if v["code"] == 0 and ("--%s " % mode) in k + " "]
        assert good, mode


def test_every_line_is_refused_as_before(golden):
    wrong = []
    for line, want in golden["lines"].items():
        code, message = parse(HOST_DIR, line)
        if "either" in want:
            allowed = [golden["lines"][k]["message"] for k in want["either"]]
            assert want["message"] in allowed, line          # (the recording itself)
            ok = code == want["code"] and message in allowed
        else:
            ok = (code, message) == (want["code"], want["message"])
        if not ok:
            wrong.append((line, (code, message), want))
    assert not wrong, wrong


def test_help_is_the_text_of_before(golden):
    assert help_text(HOST_DIR) == golden["help"]
