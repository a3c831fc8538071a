"""float32 I/Q (cf32): everything that needs no GPU -- the format's number in the header and the binding, Params, the
format check of rpf_engine_create, the byte-count formulas with 8-byte samples, the CLI option, the synthetic streams,
and the cf32 code of fft_core.h on the host emulator (tests/emul/cf32_emul.cpp): the raw layout of every K1 geometry,
the unpack arithmetic, and cf32 against cs16 through the emulated transform."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, sharding, synth
from rtl_power_fftw_amd.datastore import _as_bytes, frame_span, frames_in
from helpers import ROOT

CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
K1_SIZES = [64, 128, 256, 512, 1024, 2048, 4096, 8192]


def test_header_and_binding_agree_on_cf32():
    text = open(os.path.join(ROOT, "include", "rpf_engine.h")).read()
    m = re.search(r"#define\s+RPF_FORMAT_CF32\s+(\d+)", text)
    assert m and int(m.group(1)) == 4 == _lib.FORMAT_CF32
    assert _lib.FORMATS["cf32"] == 4 and _lib.SAMPLE_BYTES["cf32"] == 8
    assert rpf.load().rpf_abi_version() == 2, "no new symbol, the same ABI"


def test_params_know_cf32():
    p = rpf.Params(N=512, sample_format="cf32")
    assert p.sample_format == "cf32"
    # the default repeats are a byte budget: the same bytes hold a quarter of the 8-byte samples
    assert p.repeats * 4 == rpf.Params(N=512, sample_format="cs8").repeats
    with pytest.raises(rpf.RPFError) as e:
        rpf.Params(N=512, sample_format="cs12")
    assert e.value.retval == rpf.ReturnValue.InvalidArgument


@pytest.mark.parametrize("fmt", [3, 5, 15])
def test_other_numbers_are_still_no_format(fmt):
    with pytest.raises(rpf.RPFError) as e:
        rpf.Datastore(rpf.Params(N=512), flags=_lib.FLAG_SAMPLE_FORMAT(fmt))
    assert e.value.retval == rpf.ReturnValue.InvalidArgument
    assert "Sample format" in str(e.value) and str(fmt) in str(e.value)


def test_format_4_is_a_format():
    """With a device the engine is created; without one creation fails later, at the device -- never at the format."""
    try:
        with rpf.Datastore(rpf.Params(N=512, sample_format="cf32")) as ds:
            assert ds.sample_bytes == 8 and ds.sample_format == 4
    except rpf.RPFError as e:
        assert "Sample format" not in str(e)
        assert e.retval != rpf.ReturnValue.InvalidArgument


def test_buffer_must_hold_whole_samples_before_any_device():
    with pytest.raises(rpf.RPFError) as e:
        rpf.Datastore(rpf.Params(N=512, buf_length=16388, sample_format="cf32"))
    assert e.value.retval == rpf.ReturnValue.InvalidArgument and "sample size" in str(e.value)


def brute_force_frames(nbytes, N, step, b):
    n, f = 0, 0
    while b * (f * step + N) <= nbytes:
        n, f = n + 1, f + 1
    return n


def test_frame_formulas_with_eight_byte_samples():
    N = 64
    for step in (1, 7, 32, 33, 64):                       # even and odd steps
        for nbytes in list(range(0, 8 * N + 80)) + [8 * N * 5, 8 * N * 5 + 8 * step - 1, 8 * (N + 9 * step)]:
            assert frames_in(nbytes, N, step, sample_bytes=8) == brute_force_frames(nbytes, N, step, 8), (step, nbytes)
        for frames in range(0, 6):
            span = frame_span(frames, N, step, sample_bytes=8)
            assert span == 4 * frame_span(frames, N, step)
            assert frames_in(span, N, step, 8) == frames and (frames == 0 or frames_in(span - 1, N, step, 8) == frames - 1)
            assert sharding.frame_byte_range(3, frames, N, step, sample_bytes=8) == (24 * step, span)


def run_cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True)


def test_cli_format_option():
    r = run_cli("--format", "cf31", "--input", "/dev/null")
    assert r.returncode == 3 and "cf32" in r.stderr
    # cf32 parses: what is refused next is the source, not the format
    r = run_cli("--format", "cf32", "--synthetic", "1")
    assert r.returncode == 3 and "Unknown sample format" not in r.stderr, r.stderr
    r = run_cli("--format", "cf32", "--input", "/dev/null", "-b", "512")
    assert "Unknown sample format" not in r.stderr, r.stderr
    r = run_cli("--help")
    assert r.returncode == 0 and "cf32" in r.stdout


def test_synth_and_byte_views():
    s16 = synth.noise_tones_cs16(5, 1000)
    z = synth.to_cf32(s16)
    assert z.dtype == np.complex64 and z.size == 1000
    assert np.array_equal(z.view(np.float32), synth.cs16_values(s16).astype(np.float32))
    assert np.array_equal(synth.to_cf32(s16, 2.0 ** -9).view(np.float32) * 512.0, z.view(np.float32))
    g = synth.gaussian_cf32(7, 4096)
    assert g.dtype == np.complex64 and g.size == 4096 and np.array_equal(g, synth.gaussian_cf32(7, 4096))
    assert 0.9 < g.real.std() < 1.2 and np.count_nonzero(g.view(np.uint32) & 0xff) > g.size
    # Datastore.accumulate* take a complex64 or float32 array by its bytes, and raw bytes as they are
    b = _as_bytes(z)
    assert b.dtype == np.uint8 and b.size == 8000 and np.array_equal(b, _as_bytes(z.view(np.float32)))
    assert np.array_equal(b, _as_bytes(b)) and np.array_equal(b.view("<f4"), z.view(np.float32))


# ---- the emulator --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "librpf_emul_cf32.so"))
    vp = ctypes.c_void_p
    for name in ("rpf_emul_cf32_fpw", "rpf_emul_cf32_coverage_violations"):
        getattr(lib, name).restype = ctypes.c_long
        getattr(lib, name).argtypes = [ctypes.c_int]
    lib.rpf_emul_cf32_unpack_mismatches.restype = ctypes.c_long
    lib.rpf_emul_cf32_unpack_mismatches.argtypes = [ctypes.c_int, vp, vp]
    lib.rpf_emul_cf32_vs_cs16.restype = ctypes.c_long
    lib.rpf_emul_cf32_vs_cs16.argtypes = [ctypes.c_int, vp, vp, vp, vp, vp]
    assert lib.rpf_emul_cf32_sample_bytes() == 8 and lib.rpf_emul_cf32_format() == 4
    return lib


def test_the_emulator_has_the_rows_of_the_size_table(emul):
    """The emulator builds its rows from k1_sizes.h (k1_size(i, cf32, false)); the list the tests below are
    parametrised over is that table's, no more and no fewer."""
    sizes = []
    while emul.rpf_emul_cf32_size(len(sizes)) > 0:
        sizes.append(emul.rpf_emul_cf32_size(len(sizes)))
    assert sizes == K1_SIZES
    assert emul.rpf_emul_cf32_fpw(1000) == -1


@pytest.mark.parametrize("N", K1_SIZES)
def test_raw_layout_covers_every_byte_once_in_aligned_pieces(emul, N):
    assert emul.rpf_emul_cf32_coverage_violations(N) == 0


@pytest.mark.parametrize("N", K1_SIZES)
def test_unpack_is_exact_and_the_window_rounds_once(emul, N):
    fpw = emul.rpf_emul_cf32_fpw(N)
    assert fpw >= 1
    frames = synth.gaussian_cf32(N, fpw * N).view(np.float32).copy()
    frames[:6] = (np.inf, -0.0, 1e-42, np.float32(2 ** -149), 3.4e38, -1.0)     # values no integer format has
    assert emul.rpf_emul_cf32_unpack_mismatches(N, frames.ctypes.data, None) == 0
    w = synth.hann_window(N).astype(np.float32)
    assert emul.rpf_emul_cf32_unpack_mismatches(N, frames.ctypes.data, w.ctypes.data) == 0


@pytest.mark.parametrize("N", K1_SIZES)
@pytest.mark.parametrize("window", [False, True])
def test_cf32_frame_of_int16_values_gives_the_bits_of_the_cs16_frame(emul, N, window):
    s16 = synth.noise_tones_cs16(100 + N, N)
    z = synth.to_cf32(s16)
    w = synth.hann_window(N).astype(np.float32) if window else None
    a, b = np.zeros(N), np.zeros(N)
    rc = emul.rpf_emul_cf32_vs_cs16(N, s16.ctypes.data, z.ctypes.data, w.ctypes.data if window else None,
                                    a.ctypes.data, b.ctypes.data)
    assert rc == 0 and a.min() > 0
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
