"""The text blocks of the CLI, byte for byte as the build before the shared header and row loop wrote them: every
writer of rtl-power-fftw_amd/host/acquisition.cpp (plain, --stats, --excise, --quantile with one and three columns,
--cross) and its header through the rpf_host_format_* shims of librpf_host.so, on the inputs that
tests/golden/cli_text_blocks.json holds beside the recorded text (tests/golden/make_cli_text_blocks.py made both, from
a build of the commit the file names): 8 bins, dB and linear, with and without a baseline, two tunings whose frequency
column takes different numbers of digits."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch  # noqa: F401  (same HIP runtime for librpf_engine.so, see _lib.load)

from helpers import GOLDEN, ROOT, dp

FIXTURE = os.path.join(GOLDEN, "cli_text_blocks.json")
HOST_DIR = os.path.join(ROOT, "rtl-power-fftw_amd", "host")
LL, I, SZ, TEXT = ctypes.c_longlong, ctypes.c_int, ctypes.c_size_t, ctypes.c_char_p
TAIL = [LL, I, I, dp, TEXT, SZ]                 # tuned frequency, sample rate, linear, baseline, out, cap


def host_lib(host_dir):
    lib = ctypes.CDLL(os.path.join(host_dir, "librpf_host.so"))
    for name, args in [("rpf_host_format_text", [dp, I, LL] + TAIL),
                       ("rpf_host_format_text_stats", [dp, dp, dp, I, LL] + TAIL),
                       ("rpf_host_format_text_excised", [dp, dp, dp, I, LL, LL] + TAIL),
                       ("rpf_host_format_text_quantiles", [dp, dp, I, I, LL] + TAIL),
                       ("rpf_host_format_text_cross", [dp, I, LL] + TAIL),
                       ("rpf_host_format_header", [TEXT, TEXT, I, TEXT, SZ]),
                       ("rpf_host_format_header_mode", [TEXT, TEXT, I, TEXT, SZ])]:
        getattr(lib, name).restype = ctypes.c_long
        getattr(lib, name).argtypes = args
    return lib


def whole_case(golden, case):
    """A case of the recording with what it names put in: its writer's inputs, N and the baseline (or None)."""
    return dict(golden["inputs"][case["inputs"]], N=golden["N"], tuned=case["tuned"], rate=case["rate"],
                linear=case["linear"], baseline=golden["baseline"] if case["baseline"] else None)


def render(lib, case):
    """The text of one whole case: {"writer", "N", "tuned", "rate", "linear", "baseline" (list or None), and the
    writer's own planes and counts}."""
    N = case["N"]
    arrays = {k: np.array(v, dtype=np.float64) for k, v in case.items() if isinstance(v, list)}
    p = {k: a.ctypes.data_as(dp) for k, a in arrays.items()}
    out = ctypes.create_string_buffer(1 << 16)
    tail = (case["tuned"], case["rate"], case["linear"], p.get("baseline"), out, len(out))
    w = case["writer"]
    if w == "plain":
        n = lib.rpf_host_format_text(p["pwr"], N, case["repeats"], *tail)
    elif w == "stats":
        n = lib.rpf_host_format_text_stats(p["pwr"], p["sum_sq"], p["peak"], N, case["repeats"], *tail)
    elif w == "excised":
        n = lib.rpf_host_format_text_excised(p["clean"], p["kept"], p["total"], N, case["K"], case["L"], *tail)
    elif w == "quantiles":
        n = lib.rpf_host_format_text_quantiles(p["planes"], p["q"], len(case["q"]), N, case["L"], *tail)
    else:
        assert w == "cross"
        n = lib.rpf_host_format_text_cross(p["planes"], N, case["frames"], *tail)
    assert n > 0
    return out.value.decode()


def render_header(lib, kind):
    out = ctypes.create_string_buffer(4096)
    start, end = b"2026-01-02 03:04:05 UTC", b"2026-01-02 03:04:06 UTC"
    if kind in ("plain", "stats"):
        n = lib.rpf_host_format_header(start, end, int(kind == "stats"), out, len(out))
    else:
        n = lib.rpf_host_format_header_mode(start, end, int(kind == "cross"), out, len(out))
    assert n > 0
    return out.value.decode()


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_recording_covers_every_writer_both_scales_baseline_and_two_tunings(golden):
    cases, inputs = golden["cases"].values(), golden["inputs"]
    assert golden["N"] == 8
    assert sorted((i["writer"], len(i.get("q", []))) for i in inputs.values()) == [
        ("cross", 0), ("excised", 0), ("plain", 0), ("quantiles", 1), ("quantiles", 3), ("stats", 0)]
    for name in inputs:
        assert sorted((c["linear"], c["baseline"], c["tuned"]) for c in cases if c["inputs"] == name) == [
            (lin, base, f) for lin in (0, 1) for base in (False, True) for f in (100000000, 1420405752)]
    digits = {c["tuned"]: len(c["text"].split()[0]) for c in cases if c["inputs"] == "plain"}
    assert len(set(digits.values())) == 2                              # the frequency column's precision differs
    assert 0.0 in inputs["excised"]["kept"]
    cross = inputs["cross"]["planes"]
    assert any(re == 0.0 and im == 0.0 for re, im in zip(cross[16:24], cross[24:32]))
    assert set(golden["headers"]) == {"plain", "stats", "excised", "cross"}


def test_every_block_is_written_byte_for_byte_as_before(golden):
    lib = host_lib(HOST_DIR)
    wrong = [name for name, case in golden["cases"].items() if render(lib, whole_case(golden, case)) != case["text"]]
    assert not wrong, wrong


def test_every_header_is_written_byte_for_byte_as_before(golden):
    lib = host_lib(HOST_DIR)
    for kind, text in golden["headers"].items():
        assert render_header(lib, kind) == text, kind
