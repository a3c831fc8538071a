"""Overlapped FFT frames (rpf_config::frame_step, --frame-overlap) on the CPU: the ABI layout, argument checks that
come before any device, the host's derived counts, and the checker the GPU tests rely on -- an engine at frame step
S on stream X must equal an engine at step N on the materialised stream X' = concat_f X[2fS : 2fS + 2N]."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, synth
from rtl_power_fftw_amd.datastore import frame_span, frames_for_budget, frames_in
from rtl_power_fftw_amd.sharding import frame_byte_range
from helpers import ROOT, oracle_accumulate, truth_f64
from parity_bars import VS_TRUTH

HOST_DIR = os.path.join(ROOT, "rtl-power-fftw_amd", "host")
CLI = os.path.join(HOST_DIR, "rpf_power")


def materialise(stream, N, step):
    """X' = the frames of X at frame step S, side by side (what today's path runs)."""
    frames = sliding_window_view(np.asarray(stream, dtype=np.uint8), 2 * N)[::2 * step]
    return np.ascontiguousarray(frames).reshape(-1)


def gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def test_config_layout_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rpf_engine.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(rpf_config), offsetof(rpf_config, flags), '
                   'offsetof(rpf_config, frame_step)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    size, flags, step = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == ctypes.sizeof(_lib.rpf_config)
    assert flags == _lib.rpf_config.flags.offset
    assert step == _lib.rpf_config.frame_step.offset == _lib.CONFIG_SIZE_V2_0 == 40
    assert [f[0] for f in _lib.rpf_config._fields_][-1] == "frame_step"


@pytest.mark.parametrize("step", [-1, 514])
def test_bad_frame_step_is_invalid_argument_before_any_device(step):
    with pytest.raises(rpf.RPFError) as e:
        rpf.Datastore(rpf.Params(N=512, frame_step=step))
    assert e.value.retval == rpf.ReturnValue.InvalidArgument
    assert "Frame step" in str(e.value)


def test_old_config_size_is_accepted():
    # ABI 2's first form of rpf_config ends at `flags`: accepted up to the device probe (frame step N)
    if gpu_present():
        with rpf.Datastore(rpf.Params(N=512), struct_size=_lib.CONFIG_SIZE_V2_0) as ds:
            assert ds.frames_in(10 * 1024) == 10
    else:
        with pytest.raises(rpf.RPFError) as e:
            rpf.Datastore(rpf.Params(N=512), struct_size=_lib.CONFIG_SIZE_V2_0)
        assert e.value.retval == rpf.ReturnValue.HardwareError
    with pytest.raises(rpf.RPFError) as e:
        rpf.Datastore(rpf.Params(N=512), struct_size=_lib.CONFIG_SIZE_V2_0 + 4)
    assert e.value.retval == rpf.ReturnValue.InvalidArgument


def test_frame_formulas():
    N = 512
    assert frames_in(2 * N - 2, N, 256) == 0 and frames_in(2 * N, N, 256) == 1
    assert frames_in(2 * N + 511, N, 256) == 1 and frames_in(2 * N + 512, N, 256) == 2
    assert frames_in(20 * N, N, N) == 10 and frames_in(20 * N + 2, N, N) == 10
    for step in (1, 7, 256, 384, 512):
        for f in range(0, 9):
            span = frame_span(f, N, step)
            assert frames_in(span, N, step) == f
            if f:
                assert frames_in(span - 2, N, step) == f - 1
    assert frames_for_budget(10, N, N) == 10 and frames_for_budget(10, N, 256) == 19
    assert rpf.Params(N=512, buf_length=16384 * 100).repeats == 1600
    assert rpf.Params(N=512, buf_length=16384 * 100, frame_step=256).repeats == 3199
    assert frame_byte_range(3, 4, N, 256) == (3 * 512, 2 * N + 3 * 512)
    assert frame_byte_range(3, 4, N) == (3 * 1024, 4 * 1024)
    X = synth.uniform_iq(5, 40 * N)
    for step in (N, 256, 129):
        Xp = materialise(X, N, step)
        assert Xp.size == 2 * N * frames_in(X.size, N, step)
        off, length = frame_byte_range(2, 3, N, step)
        assert np.array_equal(materialise(X[off:off + length], N, step), Xp[2 * 2 * N: 5 * 2 * N])


# ---- the host (rtl-power-fftw_amd/host) ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host():
    if not (os.path.exists(os.path.join(HOST_DIR, "librpf_host.so")) and os.path.exists(CLI)):
        subprocess.run(["make", "-C", HOST_DIR], check=True)
    import torch  # noqa: F401  (same HIP runtime for librpf_engine.so, see _lib.load)
    lib = ctypes.CDLL(os.path.join(HOST_DIR, "librpf_host.so"))
    ll = ctypes.POINTER(ctypes.c_longlong)
    ip = ctypes.POINTER(ctypes.c_int)
    lib.rpf_host_parse_frames.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ip, ip, ll, ll,
                                          ctypes.c_char_p, ctypes.c_size_t]
    return lib


def parse_frames(host, *args, rate=2000000):
    argv = (ctypes.c_char_p * (len(args) + 1))(b"rpf_power", *[a.encode() for a in args])
    N, step = ctypes.c_int(), ctypes.c_int()
    repeats, samples = ctypes.c_longlong(), ctypes.c_longlong()
    msg = ctypes.create_string_buffer(512)
    rc = host.rpf_host_parse_frames(len(args) + 1, argv, rate, ctypes.byref(N), ctypes.byref(step),
                                    ctypes.byref(repeats), ctypes.byref(samples), msg, len(msg))
    return rc, (N.value, step.value, repeats.value, samples.value), msg.value.decode()


def test_host_frame_overlap_option(host):
    rc, got, _ = parse_frames(host, "--frame-overlap", "50", "-b", "512", "-n", "10")
    assert rc == 0 and got == (512, 256, 10, 512 + 9 * 256)
    rc, got, _ = parse_frames(host, "--frame-overlap", "12.5", "-b", "512", "-n", "4")
    assert rc == 0 and got[1] == 448
    rc, got, _ = parse_frames(host, "--frame-overlap", "99.99", "-b", "512", "-n", "4")
    assert rc == 0 and got[1] == 1                       # N - floor(N p / 100), never below 1
    rc, got, _ = parse_frames(host, "-b", "512", "-n", "10")
    assert rc == 0 and got == (512, 512, 10, 5120)


def test_host_sample_budgets_become_frames(host):
    # -t: R0 = ceil(rate t / N) side-by-side frames' worth of samples; p = 0 is the option being absent
    for extra in ([], ["--frame-overlap", "0"]):
        rc, got, _ = parse_frames(host, "-b", "1000", "-t", "1", *extra, rate=2000000)
        assert rc == 0 and got == (1000, 1000, 2000, 2000000)
    rc, got, _ = parse_frames(host, "-b", "1000", "-t", "1", "--frame-overlap", "50", rate=2000000)
    assert rc == 0 and got[1] == 500 and got[2] == (2000 - 1) * 1000 // 500 + 1
    assert got[3] == 1000 + 500 * (got[2] - 1) == 2000000            # the same samples acquired
    # the default repeats = buf_length / (2N), the same way
    rc, plain, _ = parse_frames(host, "-b", "512")
    rc2, zero, _ = parse_frames(host, "-b", "512", "--frame-overlap", "0")
    assert rc == rc2 == 0 and plain == zero and plain[2] == 1600
    rc, got, _ = parse_frames(host, "-b", "512", "--frame-overlap", "75")
    assert rc == 0 and got[1] == 128 and got[2] == (1600 - 1) * 4 + 1 and got[3] == 1600 * 512


@pytest.mark.parametrize("value", ["100", "-1", "abc"])
def test_host_frame_overlap_rejects(host, value):
    rc, _, msg = parse_frames(host, "-b", "512", "--frame-overlap", value)
    assert rc == 3 and msg
    r = subprocess.run([CLI, "-b", "512", "--frame-overlap", value, "--synthetic", "1"], capture_output=True, text=True)
    assert r.returncode == 3 and "frame-overlap" in r.stderr


def test_host_help_lists_frame_overlap():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    text = r.stdout + r.stderr
    assert "--frame-overlap" in text and "not the hop overlap" in text


# ---- the checker ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,step,window", [(512, 256, False), (512, 257, True), (5000, 2500, False)])
def test_oracle_on_materialised_stream_matches_truth(N, step, window):
    X = synth.noise_tones_iq(3, 40 * N)
    Xp = materialise(X, N, step)
    R = frames_in(X.size, N, step)
    w = synth.hann_window(N) if window else None
    got, done = oracle_accumulate(N, Xp, R, w)
    assert done == R
    want = truth_f64(N, Xp, R, w)
    assert np.max(np.abs(got - want) / want) < VS_TRUTH


def spread(pwr):
    N = pwr.size
    keep = np.ones(N, dtype=bool)
    keep[N // 2 - 2: N // 2 + 3] = False            # the DC bin +- 2 (bin N/2 is DC)
    p = pwr[keep]
    return np.var(p / p.mean())


def variance_ratio(N, window, accumulate):
    """Spread across bins of the averaged spectrum of ~4000 frames at 50 % overlap against ~2000 plain frames of the
    same white u8 noise.  accumulate(stream, step) -> (pwr, frames)."""
    X = synth.uniform_iq(11, 2000 * N)
    plain, f0 = accumulate(X, N)
    over, f1 = accumulate(X, N // 2)
    assert f0 == 2000 and f1 == 3999
    return spread(over / f1) / spread(plain / f0)


def oracle_at_step(N, window):
    def run(X, step):
        Xp = materialise(X, N, step)
        R = frames_in(X.size, N, step)
        return oracle_accumulate(N, Xp, R, window)
    return run


def test_variance_ratio_hann_half_overlap():
    N = 4096
    r = variance_ratio(N, True, oracle_at_step(N, synth.hann_window(N)))
    assert 0.45 <= r <= 0.62, r                        # theory (1 + 2 c^2) / 2 = 0.53, c = 0.167


def test_variance_ratio_rectangular_half_overlap():
    N = 4096
    r = variance_ratio(N, False, oracle_at_step(N, None))
    assert 0.68 <= r <= 0.82, r                        # theory (1 + 2 * 0.5^2) / 2 = 0.75
