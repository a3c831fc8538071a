"""Polyphase filter bank front end, everything that needs no GPU: the two C-ABI additions, what rpf_engine_create_pfb
refuses before any device is touched, the byte formulas with a span of T N samples (Python and the C++ host), the fold
of csrc/pfb_core.h on the host emulator (tests/emul/pfb_emul.cpp) against the float64 fold of pfb.fold, the default
prototype, the leakage it buys (float64 numpy), and the CLI option."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, pfb, synth
from rtl_power_fftw_amd.datastore import frame_span, frames_in
from helpers import ROOT, dp, fp, oracle_lib
import pfb_bars

HEADER = os.path.join(ROOT, "include", "rpf_engine.h")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
FORMATS = ["cu8", "cs8", "cs16", "cf32"]


def host_lib():
    lib = ctypes.CDLL(os.path.join(ROOT, "rtl-power-fftw_amd", "host", "librpf_host.so"))
    lib.rpf_host_pfb_coefficients.argtypes = [ctypes.c_int, ctypes.c_int, fp]
    for name in ("rpf_host_pfb_frames_in", "rpf_host_pfb_frame_span"):
        getattr(lib, name).restype = ctypes.c_longlong
        getattr(lib, name).argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong]
    return lib


def emul_lib():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "librpf_emul_pfb.so"))
    lib.rpf_emul_pfb_fold.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, fp, fp]
    return lib


def emul_fold(stream, frames, N, taps, fmt, h):
    """The emulator's z: frames x N x 2 float32 (I, Q)."""
    raw = np.ascontiguousarray(stream).reshape(-1).view(np.uint8)
    assert raw.size >= _lib.SAMPLE_BYTES[fmt] * N * (frames + taps - 1)
    h = np.ascontiguousarray(h, dtype=np.float32)
    z = np.full((frames, N, 2), np.nan, dtype=np.float32)
    assert emul_lib().rpf_emul_pfb_fold(raw.ctypes.data, frames, N, taps, _lib.FORMATS[fmt], h.ctypes.data_as(fp),
                                        z.ctypes.data_as(fp)) == 0
    return z


def make_stream(fmt, seed, nsamples):
    """uniform cu8 bytes, every cs8 value, full-range cs16, Gaussian cf32 with full mantissas -- as bytes"""
    if fmt == "cu8":
        return synth.uniform_iq(seed, nsamples)
    if fmt == "cs8":
        s = synth.uniform_iq(seed, nsamples)
        s[:4] = (0x80, 0x7F, 0x80, 0x80)
        return s
    if fmt == "cs16":
        v = (synth.splitmix64(seed, 2 * nsamples) >> np.uint64(48)).astype(np.uint16)
        v[:4] = (0x8000, 0x7FFF, 0x8000, 0x8000)
        return v.astype("<u2").view(np.uint8)
    return synth.gaussian_cf32(seed, nsamples).view(np.uint8)



# ---- header and binding ---------------------------------------------------------------------------------------------

def test_header_binding_and_library_agree_on_the_two_symbols(tmp_path):
    text = open(HEADER).read()
    assert re.search(r"\bint rpf_engine_create_pfb\(const rpf_config\* cfg, int taps, const float\* coeffs[^;]*, rpf_engine\*\* out\);", text)
    assert re.search(r"\bint rpf_pfb_taps\(const rpf_engine\* e\);", text)
    m = re.search(r"#define RPF_ABI_VERSION 2(.*?)\*/", text, re.S)
    assert m and "rpf_engine_create_pfb" in m.group(1) and "rpf_pfb_taps" in m.group(1)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in ("rpf_engine_create_pfb", "rpf_pfb_taps"):
        assert name in _lib.symbol_names()
        assert re.search(r"\bT %s$" % name, exported, re.M), name
    lib = rpf.load()
    assert lib.rpf_abi_version() == 2
    assert lib.rpf_pfb_taps(None) == -1
    # rpf_config did not grow
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "rpf_engine.h"\nint main(void) { printf("%zu\\n", sizeof(rpf_config)); return 0; }\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "size"), str(src)], check=True)
    size = int(subprocess.run([str(tmp_path / "size")], capture_output=True, text=True, check=True).stdout)
    assert size == ctypes.sizeof(_lib.rpf_config) == 48
    assert [f[0] for f in _lib.rpf_config._fields_][-1] == "frame_step"


# ---- refusals, all before any device ----------------------------------------------------------------------------------

def refused(message_part, N=512, taps=4, coeffs="default", flags=0, window=False, **kw):
    params = rpf.Params(N=N, pfb_taps=taps, window=window, **kw)
    if coeffs != "default":
        params.pfb_coeffs = coeffs
    with pytest.raises(rpf.RPFError) as e:
        rpf.Datastore(params, synth.hann_window(N) if window else None, flags=flags)
    assert e.value.retval == rpf.ReturnValue.InvalidArgument, str(e.value)
    assert message_part in str(e.value), str(e.value)


def test_taps_out_of_range():
    refused("between 1 and 32", taps=-1)
    refused("between 1 and 32", taps=33)
    lib = rpf.load()
    cfg = _lib.rpf_config()
    cfg.struct_size, cfg.N, cfg.n_buffers, cfg.buffer_capacity = ctypes.sizeof(cfg), 512, 2, 16384
    h = np.ones(512, dtype=np.float32)
    handle = ctypes.c_void_p()
    rc = lib.rpf_engine_create_pfb(ctypes.byref(cfg), 0, h.ctypes.data_as(fp), ctypes.byref(handle))
    assert rc == rpf.ReturnValue.InvalidArgument and not handle.value
    assert b"between 1 and 32" in lib.rpf_last_global_error()


def test_taps_times_bins_too_large():
    N = 1 << 22                                            # 32 x 2^22 = 2^27 > 2^26; the coefficients are never read
    lib = rpf.load()
    cfg = _lib.rpf_config()
    cfg.struct_size, cfg.N, cfg.n_buffers, cfg.buffer_capacity = ctypes.sizeof(cfg), N, 2, 16384
    h = np.ones(4, dtype=np.float32)
    handle = ctypes.c_void_p()
    rc = lib.rpf_engine_create_pfb(ctypes.byref(cfg), 32, h.ctypes.data_as(fp), ctypes.byref(handle))
    assert rc == rpf.ReturnValue.InvalidArgument and b"67108864" in lib.rpf_last_global_error()


def test_null_coefficients():
    lib = rpf.load()
    cfg = _lib.rpf_config()
    cfg.struct_size, cfg.N, cfg.n_buffers, cfg.buffer_capacity = ctypes.sizeof(cfg), 512, 2, 16384
    handle = ctypes.c_void_p()
    rc = lib.rpf_engine_create_pfb(ctypes.byref(cfg), 4, None, ctypes.byref(handle))
    assert rc == rpf.ReturnValue.InvalidArgument and b"coeffs is NULL" in lib.rpf_last_global_error()


def test_window_frame_step_and_flags():
    refused("coefficients are the window", window=True)
    refused("frame_step must be 0 or 512", frame_step=256)
    refused("RPF_FLAG_BIN_STATS", bin_stats=True)
    refused("RPF_FLAG_FOURSTEP_FUSED", flags=_lib.FLAG_FOURSTEP_FUSED)
    refused("kernel variant", flags=1 << 8)


def test_a_pfb_engine_is_refused_for_nothing_else():
    """With a device the engine is created; without one creation fails at the device, never at an argument."""
    for fmt in FORMATS:
        for N, taps in ((512, 4), (500, 5), (64, 1), (512, 32)):
            try:
                with rpf.Datastore(rpf.Params(N=N, pfb_taps=taps, sample_format=fmt)) as ds:
                    assert ds.pfb_taps == taps and ds.sample_bytes == _lib.SAMPLE_BYTES[fmt]
            except rpf.RPFError as e:
                assert e.retval == rpf.ReturnValue.HardwareError, str(e)


def test_wrong_number_of_coefficients_is_invalid_input():
    with pytest.raises(rpf.RPFError) as e:
        rpf.Datastore(rpf.Params(N=512, pfb_taps=4, pfb_coeffs=np.ones(512, dtype=np.float32)))
    assert e.value.retval == rpf.ReturnValue.InvalidInput


# ---- byte formulas ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b", [2, 4, 8])
@pytest.mark.parametrize("N,T", [(64, 1), (64, 4), (500, 5), (512, 8)])
def test_frame_formulas_with_a_span(b, N, T):
    host = host_lib()
    edges = {b * T * N - b: 0, b * T * N: 1, b * T * N + b * N - b: 1, b * T * N + b * N: 2, 0: 0, b * N: 1 if T == 1 else 0}
    for nbytes, want in edges.items():
        assert frames_in(nbytes, N, N, b, taps=T) == want, (nbytes, want)
        assert pfb.frames_in(nbytes, N, T, b) == want
        assert host.rpf_host_pfb_frames_in(N, T, b, nbytes) == want
    for frames in range(0, 7):
        span = frame_span(frames, N, N, b, taps=T)
        assert span == (b * N * (T - 1 + frames) if frames else 0)
        assert host.rpf_host_pfb_frame_span(N, T, b, frames) == span
        assert frames_in(span, N, N, b, taps=T) == frames
        assert frames == 0 or frames_in(span - b, N, N, b, taps=T) == frames - 1
    # taps = 1 is the formula there always was
    for nbytes in range(0, 3 * b * N, b):
        assert frames_in(nbytes, N, N, b, taps=1) == frames_in(nbytes, N, N, b)
    assert host.rpf_host_pfb_frames_in(N, 0, b, 3 * b * N) == 3 and host.rpf_host_pfb_frame_span(N, 0, b, 3) == 3 * b * N


def test_default_repeats_are_a_sample_budget():
    plain = rpf.Params(N=512).repeats
    assert rpf.Params(N=512, pfb_taps=4).repeats == plain - 3
    assert rpf.Params(N=512, pfb_taps=1).repeats == plain
    assert rpf.Params(N=512, pfb_taps=4, repeats=7).repeats == 7


# ---- the emulator's fold against float64 -----------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("N", [64, 500])
@pytest.mark.parametrize("T", [1, 3, 4, 5, 8])
def test_emulator_fold_against_float64(fmt, N, T):
    frames = 9
    stream = make_stream(fmt, 1000 + N + T, (frames + T - 1) * N)
    h = pfb.coefficients(N, T)
    z = emul_fold(stream, frames, N, T, fmt, h)
    truth = pfb.fold(stream, N, T, h, fmt)
    assert truth.shape == (frames, N)
    x = pfb.sample_values(stream, fmt).reshape(-1, N)
    h64 = h.astype(np.float64).reshape(T, N)
    for part, xs in ((0, x.real), (1, x.imag)):
        bound = T * 2.0 ** -24 * sum(np.abs(h64[t] * xs[t:t + frames]) for t in range(T))
        want = truth.real if part == 0 else truth.imag
        err = np.abs(z[..., part].astype(np.float64) - want)
        assert np.all(err <= bound), (fmt, N, T, part, float(np.max(err - bound)))


@pytest.mark.parametrize("fmt", FORMATS)
def test_one_tap_of_ones_is_the_conversion(fmt):
    N, frames = 64, 9
    stream = make_stream(fmt, 7, frames * N)
    z = emul_fold(stream, frames, N, 1, fmt, np.ones(N, dtype=np.float32))
    x = pfb.sample_values(stream, fmt)
    got = z[..., 0].astype(np.float64).ravel() + 1j * z[..., 1].astype(np.float64).ravel()
    assert np.array_equal(got, x)
    if fmt == "cu8":
        assert x.real.min() == -127 and x.real.max() == 128


# ---- the prototype -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,T", [(64, 1), (64, 2), (500, 3), (512, 4), (512, 5), (4096, 8), (64, 32)])
def test_default_prototype(N, T):
    h = pfb.coefficients(N, T)
    assert h.dtype == np.float32 and h.size == T * N
    assert abs(np.sum(h.astype(np.float64) ** 2) / N - 1.0) < 1e-6
    assert np.array_equal(h, h[::-1])
    g = np.zeros(T * N, dtype=np.float32)
    assert host_lib().rpf_host_pfb_coefficients(N, T, g.ctypes.data_as(fp)) == 0
    ulp = np.spacing(np.maximum(np.abs(h), np.abs(g)))
    assert np.all(np.abs(h.astype(np.float64) - g.astype(np.float64)) <= ulp), "Python and the C++ host within 1 ulp"
    assert host_lib().rpf_host_pfb_coefficients(N, 33, g.ctypes.data_as(fp)) == rpf.ReturnValue.InvalidArgument


# ---- what it buys: leakage, in float64 ------------------------------------------------------------------------------------

def tone(N, samples, amplitude=100.0):
    n = np.arange(samples, dtype=np.float64)
    return amplitude * np.exp(2j * np.pi * (N / 4 + 0.5) * n / N)


@pytest.mark.parametrize("N", [64, 512])
@pytest.mark.parametrize("T", [2, 3, 4, 8])
def test_leakage_three_bins_away(N, T):
    frames = 40
    rows = tone(N, (frames + T - 1) * N).reshape(-1, N)
    h = pfb.coefficients(N, T).astype(np.float64).reshape(T, N)
    k = N // 2 + N // 4                                            # the tone's bin with DC in the middle
    rect = pfb.spectrum(rows[:frames])
    fold = pfb.spectrum(sum(h[t] * rows[t:t + frames] for t in range(T)))
    r_rect, r_pfb = rect[k + 3] / rect[k], fold[k + 3] / fold[k]
    print("N=%d T=%d: p[k+3]/p[k] rectangular %.3g, PFB %.3g (%.3g of it)" % (N, T, r_rect, r_pfb, r_pfb / r_rect))
    assert 0.03 < r_rect < 0.05
    assert r_pfb <= 1e-3 * r_rect


# ---- the recorded CPU float32 figures behind the GPU bar ---------------------------------------------------------------------

def cpu_f32_spectrum(z):
    """The CPU float32 path on folded frames: (-1)^n, the oracle's float32 transform, |X|^2 summed in double."""
    frames, N, _ = z.shape
    orc = oracle_lib()
    plan = orc.rpf_oracle_plan_create(N)
    sign = (1 - 2 * (np.arange(N) % 2)).astype(np.float32)
    total = np.zeros(N)
    y = np.zeros(2 * N, dtype=np.float32)
    for f in range(frames):
        x = np.ascontiguousarray((z[f] * sign[:, None]).reshape(-1), dtype=np.float32)
        orc.rpf_oracle_fft_f32(plan, x.ctypes.data_as(fp), y.ctypes.data_as(fp))
        re, im = y[0::2].astype(np.float64), y[1::2].astype(np.float64)
        total += re * re + im * im
    orc.rpf_oracle_plan_destroy(plan)
    return total


@pytest.mark.parametrize("fmt,N", pfb_bars.ACCURACY_CASES)
def test_recorded_cpu_float32_error_is_what_the_cpu_path_gives(fmt, N):
    """pfb_bars.CPU_F32 (half the GPU test's bar) against a fresh run of the path it records."""
    from helpers import max_err_over_mean
    stream, h = pfb_bars.accuracy_stream(fmt, N), pfb.coefficients(N, pfb_bars.ACCURACY_TAPS)
    z = emul_fold(stream, pfb_bars.ACCURACY_FRAMES, N, pfb_bars.ACCURACY_TAPS, fmt, h)
    truth = pfb.spectrum(pfb.fold(stream, N, pfb_bars.ACCURACY_TAPS, h, fmt))
    err = max_err_over_mean(cpu_f32_spectrum(z), truth)
    print("%s N=%d: CPU float32 path vs float64 %.4g (recorded %.4g)" % (fmt, N, err, pfb_bars.CPU_F32[(fmt, N)]))
    assert abs(err / pfb_bars.CPU_F32[(fmt, N)] - 1.0) < 0.02


# ---- the CLI ---------------------------------------------------------------------------------------------------------------

def run_cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True)


@pytest.mark.parametrize("other,shown", [(("-w", "/dev/null"), "-w"), (("--frame-overlap", "50"), "--frame-overlap"),
                                         (("--stats",), "--stats"), (("--series", "4"), "--series"),
                                         (("--series-stats", "4"), "--series-stats"), (("--excise", "4"), "--excise"),
                                         (("--gpus", "0,1"), "--gpus")])
def test_cli_refuses_what_pfb_does_not_combine_with(other, shown):
    r = run_cli("--pfb", "4", "--input", "/dev/null", *other)
    assert r.returncode == 3, r.stderr
    assert "--pfb" in r.stderr and shown in r.stderr, r.stderr


def test_cli_parses_the_option():
    r = run_cli("--pfb", "4", "--help")
    assert r.returncode == 0 and "--pfb <taps>" in r.stdout
    for bad in ("0", "33", "-2"):
        r = run_cli("--pfb", bad, "--input", "/dev/null")
        assert r.returncode == 3 and "--pfb" in r.stderr, r.stderr
    r = run_cli("--pfb", "four", "--input", "/dev/null")
    assert r.returncode == 4
    # a good value: what fails next is not the option (there is no device here, or the file is empty)
    r = run_cli("--pfb", "4", "-b", "512", "-q", "--input", "/dev/null")
    assert "--pfb" not in r.stderr, r.stderr
