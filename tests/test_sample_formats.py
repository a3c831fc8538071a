"""Sample formats (signed 8-bit and signed 16-bit little-endian I/Q beside the reference's unsigned 8-bit), the parts
that need no GPU: the C-ABI additions, the byte-count formulas with 4-byte samples, the CLI option, the synthetic
converters, and the host build of the kernels' unpack over every bit pattern."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, sharding, synth
from rtl_power_fftw_amd.datastore import frame_span, frames_in
from helpers import ROOT

HEADER = os.path.join(ROOT, "include", "rpf_engine.h")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")


def header_constants(tmp_path):
    src = tmp_path / "consts.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rpf_engine.h"\n'
                   'int main(void) { printf("%d %d %d %u %u %u %zu %zu\\n", RPF_FORMAT_CU8, RPF_FORMAT_CS8, RPF_FORMAT_CS16, '
                   'RPF_FLAG_SAMPLE_FORMAT(RPF_FORMAT_CS16), RPF_FLAG_SAMPLE_FORMAT(0x1f), RPF_FLAG_CATCH_ALL, '
                   'sizeof(rpf_config), offsetof(rpf_config, frame_step)); return 0; }\n')
    exe = tmp_path / "consts"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    return list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))


def test_header_and_binding_agree_on_the_formats(tmp_path):
    cu8, cs8, cs16, flag16, flag_masked, catch_all, size, step_off = header_constants(tmp_path)
    assert (cu8, cs8, cs16) == (_lib.FORMAT_CU8, _lib.FORMAT_CS8, _lib.FORMAT_CS16) == (0, 1, 2)
    assert flag16 == _lib.FLAG_SAMPLE_FORMAT(_lib.FORMAT_CS16) == 2 << 16
    assert flag_masked == _lib.FLAG_SAMPLE_FORMAT(0x1f) == 0xf << 16           # four bits, 16..19
    assert catch_all == _lib.FLAG_CATCH_ALL == 16
    # the format lives in `flags`: the config did not grow and frame_step is still its last field
    assert size == ctypes.sizeof(_lib.rpf_config) == 48
    assert step_off == _lib.rpf_config.frame_step.offset == 40
    assert [f[0] for f in _lib.rpf_config._fields_][-1] == "frame_step"
    # no flag shares a bit with another
    flags = [_lib.FLAG_NO_LDS_DMA, _lib.FLAG_FOURSTEP_FUSED, _lib.FLAG_NO_MIXED_RADIX, _lib.FLAG_NO_FOURSTEP_FUSED,
             _lib.FLAG_CATCH_ALL, 0xff << 8, 0xf << 16]
    assert sum(flags) == np.bitwise_or.reduce(flags)


def test_library_exports_the_new_symbols():
    text = open(HEADER).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in ("rpf_sample_bytes", "rpf_sample_format"):
        assert re.search(r"\bint %s\(const rpf_engine\* e\);" % name, text), name
        assert name in _lib.symbol_names()
        assert re.search(r"\bT %s$" % name, exported, re.M), name
    lib = rpf.load()
    assert lib.rpf_sample_bytes(None) == 0 and lib.rpf_sample_format(None) == -1


@pytest.mark.parametrize("fmt", [3, 7, 15])
def test_unknown_format_is_invalid_argument_before_any_device(fmt):
    with pytest.raises(rpf.RPFError) as e:
        rpf.Datastore(rpf.Params(N=512), flags=_lib.FLAG_SAMPLE_FORMAT(fmt))
    assert e.value.retval == rpf.ReturnValue.InvalidArgument
    assert "Sample format" in str(e.value) and str(fmt) in str(e.value)


def test_params_know_the_formats():
    assert rpf.Params(N=512).sample_format == "cu8"
    assert rpf.Params(N=512, sample_format="cs16").sample_format == "cs16"
    # the default repeats are a sample budget: the same bytes hold half the 16-bit samples
    assert rpf.Params(N=512, sample_format="cs16").repeats * 2 == rpf.Params(N=512, sample_format="cs8").repeats
    with pytest.raises(rpf.RPFError) as e:
        rpf.Params(N=512, sample_format="cs12")
    assert e.value.retval == rpf.ReturnValue.InvalidArgument


def test_buffer_must_hold_whole_samples_before_any_device():
    with pytest.raises(rpf.RPFError) as e:
        rpf.Datastore(rpf.Params(N=512, buf_length=16386, sample_format="cs16"))
    assert e.value.retval == rpf.ReturnValue.InvalidArgument and "sample size" in str(e.value)


def brute_force_frames(nbytes, N, step, b):
    n, f = 0, 0
    while b * (f * step + N) <= nbytes:
        n, f = n + 1, f + 1
    return n


def test_frame_formulas_with_four_byte_samples():
    N = 64
    for step in (1, 7, 33, 64):
        for nbytes in list(range(0, 4 * N + 40)) + [4 * N * 5, 4 * N * 5 + 4 * step - 1, 4 * (N + 9 * step)]:
            assert frames_in(nbytes, N, step, sample_bytes=4) == brute_force_frames(nbytes, N, step, 4), (step, nbytes)
            assert frames_in(nbytes, N, step) == frames_in(nbytes, N, step, 2) == brute_force_frames(nbytes, N, step, 2)
        for frames in range(0, 6):
            span = frame_span(frames, N, step, sample_bytes=4)
            assert span == 2 * frame_span(frames, N, step)
            assert frames_in(span, N, step, 4) == frames and (frames == 0 or frames_in(span - 1, N, step, 4) == frames - 1)
            assert sharding.frame_byte_range(3, frames, N, step, sample_bytes=4) == (12 * step, span)
    assert sharding.frame_byte_range(3, 2, N, 16) == (96, 2 * N + 32)          # the positional form is what it was


def run_cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True)


def test_cli_format_option():
    r = run_cli("--format", "cs12", "--input", "/dev/null")
    assert r.returncode == 3
    assert all(name in r.stderr for name in ("cu8", "cs8", "cs16"))
    for fmt in ("cs8", "cs16"):
        r = run_cli("--format", fmt, "--synthetic", "1")
        assert r.returncode == 3, r.stderr
        r = run_cli("--format", fmt)                      # a live dongle delivers cu8
        assert r.returncode == 3, r.stderr
    r = run_cli("--help")
    assert r.returncode == 0 and "--format <cu8|cs8|cs16>" in r.stdout


def test_synth_converters():
    u = synth.noise_tones_iq(3, 5000)
    clamped = np.minimum(u, 254)
    s8 = synth.to_cs8(clamped)
    assert s8.dtype == np.uint8 and s8.size == clamped.size
    assert np.array_equal(s8.view(np.int8).astype(np.int32) + 127, clamped.astype(np.int32))       # round trip
    with pytest.raises(ValueError):
        synth.to_cs8(np.array([255, 0], dtype=np.uint8))
    # little-endian, by hand: samples (1, -2) and (-128, 127)
    two = np.array([1, -2, -128, 127], dtype=np.int8).view(np.uint8)
    assert synth.to_cs16(two).tolist() == [0x01, 0x00, 0xFE, 0xFF, 0x80, 0xFF, 0x7F, 0x00]
    assert synth.to_cs16(two, shift=8).tolist() == [0x00, 0x01, 0x00, 0xFE, 0x00, 0x80, 0x00, 0x7F]
    assert synth.to_cs16(two, shift=3).tolist() == [0x08, 0x00, 0xF0, 0xFF, 0x00, 0xFC, 0xF8, 0x03]
    assert synth.cs16_values(synth.to_cs16(two, 3)).tolist() == [8, -16, -1024, 1016]
    s16 = synth.noise_tones_cs16(4, 100000)
    assert s16.dtype == np.uint8 and s16.size == 400000
    assert np.array_equal(s16, synth.noise_tones_cs16(4, 100000, chunk=777))     # chunking does not change the bytes
    v = synth.cs16_values(s16).astype(np.float64)
    assert 5000 < v.std() < 8000 and abs(v.mean()) < 100
    assert v.max() > 16384 and v.min() < -16384


def test_emulated_unpack_is_exact_for_every_bit_pattern():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "librpf_emul_formats.so"))
    for name in ("rpf_emul_cs8_unpack_mismatches", "rpf_emul_cs16_unpack_mismatches"):
        fn = getattr(lib, name)
        fn.restype = ctypes.c_long
        assert fn() == 0, name
    # the wave-local raw layout: what raw_source stages is what phase_unpack reads, sample t + T a in register a
    N = lib.rpf_emul_formats_n()
    frame = synth.uniform_iq(9, 2 * N)
    for name, nbytes in (("rpf_emul_cs8_layout_mismatches", 2 * N), ("rpf_emul_cs16_layout_mismatches", 4 * N)):
        fn = getattr(lib, name)
        fn.restype = ctypes.c_long
        fn.argtypes = [ctypes.c_void_p]
        assert fn(frame[:nbytes].ctypes.data) == 0, name
