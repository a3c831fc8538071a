"""Cross-spectrum of two streams, everything that needs no GPU: the two C-ABI additions, the combined streams and the
finishing expression of csrc/cross_core.h on the host emulator (tests/emul/cross_emul.cpp), coherence and phase in
Python and in the C++ host, the polarisation identity in float64, the CLI option and what it refuses, and the recorded
CPU float32 figures behind the GPU test's bar (cross_bars.py).  tests/test_gpu_cross.py imports the helpers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, pfb, stats, synth
from helpers import ROOT, dp, fp, oracle_lib
import cross_bars

HEADER = os.path.join(ROOT, "include", "rpf_engine.h")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
FORMATS = ["cu8", "cs8", "cs16", "cf32"]


# ---- helpers (shared with tests/test_gpu_cross.py) --------------------------------------------------------------------

def emul_lib():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "librpf_emul_cross.so"))
    lib.rpf_emul_cross_combine.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, fp, fp]
    lib.rpf_emul_cross_finish.argtypes = [dp, ctypes.c_int, dp]
    return lib


def host_lib():
    lib = ctypes.CDLL(os.path.join(ROOT, "rtl-power-fftw_amd", "host", "librpf_host.so"))
    lib.rpf_host_coherence.argtypes = [dp, ctypes.c_int, dp]
    lib.rpf_host_cross_phase.argtypes = [dp, ctypes.c_int, dp]
    lib.rpf_host_format_text_cross.restype = ctypes.c_long
    lib.rpf_host_format_text_cross.argtypes = [dp, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int,
                                               ctypes.c_int, dp, ctypes.c_char_p, ctypes.c_size_t]
    return lib


def as_bytes(stream):
    return np.ascontiguousarray(stream).reshape(-1).view(np.uint8)


def emul_combine(a, b, fmt):
    """The emulator's u = a + b and v = a + i b: two (nsamples, 2) float32 arrays (I, Q) from two byte streams."""
    a, b = as_bytes(a), as_bytes(b)
    assert a.size == b.size and a.size % _lib.SAMPLE_BYTES[fmt] == 0
    n = a.size // _lib.SAMPLE_BYTES[fmt]
    u = np.full((n, 2), np.nan, dtype=np.float32)
    v = np.full((n, 2), np.nan, dtype=np.float32)
    assert emul_lib().rpf_emul_cross_combine(a.ctypes.data, b.ctypes.data, n, _lib.FORMATS[fmt], u.ctypes.data_as(fp),
                                             v.ctypes.data_as(fp)) == 0
    return u, v


def emul_finish(planes):
    """The emulator's finishing expression: (4, N) Paa, Pbb, Puu, Pvv -> (4, N) Saa, Sbb, Re Sab, Im Sab."""
    planes = np.ascontiguousarray(planes, dtype=np.float64)
    assert planes.ndim == 2 and planes.shape[0] == 4
    out = np.full(planes.shape, np.nan)
    assert emul_lib().rpf_emul_cross_finish(planes.ctypes.data_as(dp), planes.shape[1], out.ctypes.data_as(dp)) == 0
    return out


def frames_of(x, N, step=None, frames=None):
    """(frames, N) rows of a sample array: frame f = samples [f S, f S + N)."""
    step = N if step is None else step
    have = 0 if x.shape[0] < N else (x.shape[0] - N) // step + 1
    frames = have if frames is None else min(frames, have)
    idx = np.arange(frames)[:, None] * step + np.arange(N)[None, :]
    return x[idx]


def prepared_frames(values, N, step=None, window=None, frames=None):
    """Frames of complex128 sample values as the engine's transform sees them: (-1)^n, and the window multiplied in
    float32 with one rounding per component (exact without a window)."""
    rows = frames_of(values, N, step, frames)
    sign = 1.0 - 2.0 * (np.arange(N) % 2)
    re, im = rows.real, rows.imag
    if window is not None:
        w = np.asarray(window, dtype=np.float32)
        re = (re.astype(np.float32) * w).astype(np.float64)
        im = (im.astype(np.float32) * w).astype(np.float64)
    return (re + 1j * im) * sign


def truth_cross(a, b, fmt, N, step=None, window=None, frames=None):
    """Saa, Sbb (float64) and Sab (complex128) = sum over the frames of A conj(B), numpy complex128 on the exactly
    converted, float32-windowed frames of the two byte streams; bin N/2 = DC."""
    A = np.fft.fft(prepared_frames(pfb.sample_values(a, fmt), N, step, window, frames), axis=1)
    B = np.fft.fft(prepared_frames(pfb.sample_values(b, fmt), N, step, window, frames), axis=1)
    return (np.abs(A) ** 2).sum(axis=0), (np.abs(B) ** 2).sum(axis=0), (A * np.conj(B)).sum(axis=0)


def cross_err(planes, saa, sbb, sab):
    """max_k |S^ab - Sab| / max(m_k, median m), m = (Saa + Sbb) / 2 of the truth (cross_bars.py)."""
    m = 0.5 * (saa + sbb)
    got = planes[2] + 1j * planes[3]
    return float(np.max(np.abs(got - sab) / np.maximum(m, np.median(m))))


def cpu_f32_power(x32, N, step=None, window=None, frames=None):
    """The CPU float32 path on (nsamples, 2) float32 samples: (-1)^n and the window in float32, the oracle's float32
    transform, |X|^2 summed in double."""
    rows = frames_of(x32, N, step, frames)
    orc = oracle_lib()
    plan = orc.rpf_oracle_plan_create(N)
    scale = (1 - 2 * (np.arange(N) % 2)).astype(np.float32)
    total = np.zeros(N)
    y = np.zeros(2 * N, dtype=np.float32)
    for f in range(rows.shape[0]):
        x = rows[f]
        if window is not None:
            x = x * np.asarray(window, dtype=np.float32)[:, None]
        x = np.ascontiguousarray((x * scale[:, None]).reshape(-1), dtype=np.float32)
        orc.rpf_oracle_fft_f32(plan, x.ctypes.data_as(fp), y.ctypes.data_as(fp))
        re, im = y[0::2].astype(np.float64), y[1::2].astype(np.float64)
        total += re * re + im * im
    orc.rpf_oracle_plan_destroy(plan)
    return total


def values_f32(stream, fmt):
    v = pfb.sample_values(stream, fmt)
    return np.stack([v.real, v.imag], axis=1).astype(np.float32)       # exact: every format's value is a float32


def cpu_f32_cross(a, b, fmt, N, step=None, window=None, frames=None):
    """The CPU float32 path of cross_bars.py: four float32 power spectra and the emulator's finishing expression."""
    u, v = emul_combine(a, b, fmt)
    planes = np.stack([cpu_f32_power(x, N, step, window, frames) for x in (values_f32(a, fmt), values_f32(b, fmt), u, v)])
    return emul_finish(planes)


def format_cross_block(planes, frames, N, cfreq=1420405752, rate=2000000, linear=False):
    """The data lines of the CLI's --cross block from (4, N) planes, by the C++ host's writer."""
    planes = np.ascontiguousarray(planes, dtype=np.float64)
    buf = ctypes.create_string_buffer(160 * N)
    host_lib().rpf_host_format_text_cross(planes.ctypes.data_as(dp), N, frames, cfreq, rate, int(linear), None, buf, len(buf))
    return [l for l in buf.value.decode().split("\n") if l.strip()]


# ---- header, binding and library ----------------------------------------------------------------------------------------

def test_header_binding_and_library_agree_on_the_two_symbols():
    text = open(HEADER).read()
    assert re.search(r"\bint rpf_accumulate_device_cross\(rpf_engine\* e, const void\* d_a, const void\* d_b, size_t nbytes, "
                     r"int64_t repeats,\s+double\* d_out[^;]*, void\* hip_stream, int64_t\* repeats_done\);", text)
    assert re.search(r"\bint rpf_accumulate_cross\(rpf_engine\* e, const uint8_t\* a, const uint8_t\* b, size_t nbytes, "
                     r"int64_t repeats,\s+double\* out[^;]*, int64_t\* repeats_done\);", text)
    m = re.search(r"#define RPF_ABI_VERSION 2(.*?)\*/", text, re.S)
    assert m and "rpf_accumulate_device_cross" in m.group(1) and "rpf_accumulate_cross" in m.group(1)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in ("rpf_accumulate_device_cross", "rpf_accumulate_cross"):
        assert name in _lib.symbol_names()
        assert re.search(r"\bT %s$" % name, exported, re.M), name
    lib = rpf.load()
    assert lib.rpf_abi_version() == 2
    out = np.zeros(4)
    assert lib.rpf_accumulate_cross(None, None, None, 0, 0, out.ctypes.data_as(dp), None) == rpf.ReturnValue.InvalidArgument
    assert lib.rpf_accumulate_device_cross(None, None, None, 0, 0, None, None, None) == rpf.ReturnValue.InvalidArgument
    assert hasattr(rpf.Datastore, "accumulate_cross") and hasattr(rpf.Datastore, "accumulate_device_cross")


# ---- the emulator: combined streams ----------------------------------------------------------------------------------------

def integer_stream(fmt, values):
    """A stream whose I and Q values are `values` (converted values, not bytes), as bytes of the format."""
    v = np.asarray(values, dtype=np.int64)
    if fmt == "cu8":
        return (v + 127).astype(np.uint8)
    if fmt == "cs8":
        return v.astype(np.int8).view(np.uint8)
    return v.astype("<i2").view(np.uint8)


@pytest.mark.parametrize("fmt,lo,hi", [("cu8", -127, 128), ("cs8", -128, 127), ("cs16", -32768, 32767)])
def test_combined_streams_are_exact_integers_at_the_extremes(fmt, lo, hi):
    # every pairing of the two extreme values (and 0, 1) in aI, aQ, bI, bQ
    ext = [lo, hi, 0, 1]
    quads = np.array([(ai, aq, bi, bq) for ai in ext for aq in ext for bi in ext for bq in ext])
    a = integer_stream(fmt, quads[:, :2].reshape(-1))
    b = integer_stream(fmt, quads[:, 2:].reshape(-1))
    if fmt == "cu8":
        assert a.min() == 0 and a.max() == 255
    u, v = emul_combine(a, b, fmt)
    ai, aq, bi, bq = (quads[:, k] for k in range(4))
    assert np.array_equal(u.astype(np.int64), np.stack([ai + bi, aq + bq], axis=1))
    assert np.array_equal(v.astype(np.int64), np.stack([ai - bq, aq + bi], axis=1))
    assert u.dtype == np.float32 and np.array_equal(u, np.rint(u))


def test_combined_streams_of_cf32_are_the_single_float32_sums():
    a, b = synth.gaussian_cf32(1, 1001), synth.gaussian_cf32(2, 1001) * np.float32(3.7)
    a[:3] = (np.float32(1e30) + 0j, 1 + 1j * np.float32(2.0 ** -30), np.float32(16777216.0) + 1j)
    b[:3] = (np.float32(1e30) + 0j, np.float32(2.0 ** -30) + 1j, 1 + 1j * np.float32(16777216.0))
    b = b.astype(np.complex64)
    u, v = emul_combine(a, b, "cf32")
    fa, fb = a.view(np.float32).reshape(-1, 2), b.view(np.float32).reshape(-1, 2)
    assert np.array_equal(u[:, 0], fa[:, 0] + fb[:, 0]) and np.array_equal(u[:, 1], fa[:, 1] + fb[:, 1])
    assert np.array_equal(v[:, 0], fa[:, 0] - fb[:, 1]) and np.array_equal(v[:, 1], fa[:, 1] + fb[:, 0])
    # ... and they are roundings: the float64 sums differ somewhere
    assert not np.array_equal(u[:, 0].astype(np.float64), fa[:, 0].astype(np.float64) + fb[:, 0].astype(np.float64))


# ---- the emulator: finishing expression ----------------------------------------------------------------------------------------

def test_finish_of_a_stream_with_itself_is_exact():
    rng = np.random.default_rng(5)
    paa = rng.random(257) * 1e9 + 1.0
    out = emul_finish(np.stack([paa, paa, 4.0 * paa, 2.0 * paa]))
    # C = 2 Paa exactly, Puu - C = 2 Paa exactly, half of it Paa: b = a gives Re Sab = Saa bit for bit; Pvv = 2 Paa: Im = 0
    assert np.array_equal(out[0], paa) and np.array_equal(out[1], paa)
    assert np.array_equal(out[2], out[0]) and np.array_equal(out[3], np.zeros(257))


def test_finish_of_float64_planes_reproduces_the_cross_spectrum():
    N, F = 64, 80
    rng = np.random.default_rng(6)
    A = rng.standard_normal((F, N)) + 1j * rng.standard_normal((F, N))
    B = 0.5 * A + rng.standard_normal((F, N)) + 1j * rng.standard_normal((F, N))
    p = lambda X: (X.real ** 2 + X.imag ** 2).sum(axis=0)
    planes = np.stack([p(A), p(B), p(A + B), p(A + 1j * B)])
    out = emul_finish(planes)
    sab = (A * np.conj(B)).sum(axis=0)
    c = planes[0] + planes[1]
    assert np.array_equal(out[2], 0.5 * (planes[2] - c)) and np.array_equal(out[3], 0.5 * (planes[3] - c))
    # double rounding: every term of the F-term sums carries a few 2^-53 of itself, and Puu, Pvv <= 2 (Paa + Pbb)
    err = np.abs(out[2] + 1j * out[3] - sab) / c
    print("finishing expression on float64 planes: %.3g of Saa + Sbb" % err.max())
    assert err.max() < 64 * 2.0 ** -52


# ---- derived quantities ------------------------------------------------------------------------------------------------------

def test_coherence_and_phase_on_hand_made_planes():
    planes = np.array([[4.0, 1.0, 0.0, 2.0, 0.0, 9.0],       # Saa
                       [1.0, 4.0, 3.0, 0.0, 0.0, 1.0],       # Sbb
                       [2.0, 0.0, 1.0, 1.0, 0.0, -3.0],      # Re Sab
                       [0.0, -1.0, 0.0, 1.0, 0.0, 0.0]])     # Im Sab
    g = stats.coherence(planes)
    ph = stats.cross_phase(planes)
    assert g[0] == 1.0 and g[1] == 0.25 and g[5] == 1.0
    assert np.isnan(g[2]) and np.isnan(g[3]) and np.isnan(g[4])              # a zero denominator: NaN, not inf
    assert ph[0] == 0.0 and ph[1] == -np.pi / 2 and ph[5] == np.pi and ph[3] == np.pi / 4
    # not clamped
    assert stats.coherence(np.array([[1.0], [1.0], [1.0 + 2.0 ** -20], [0.0]]))[0] > 1.0
    with pytest.raises(ValueError):
        stats.coherence(np.zeros((3, 4)))
    with pytest.raises(ValueError):
        stats.cross_phase(np.zeros((3, 4)))


def test_the_host_computes_the_same_coherence_and_phase():
    rng = np.random.default_rng(7)
    n = 1000
    planes = np.stack([rng.random(n) * 1e6, rng.random(n) * 1e3, rng.standard_normal(n) * 1e4, rng.standard_normal(n) * 1e4])
    planes[0, :5] = 0.0
    planes[1, 5:9] = 0.0
    g, ph = np.zeros(n), np.zeros(n)
    host_lib().rpf_host_coherence(planes.ctypes.data_as(dp), n, g.ctypes.data_as(dp))
    host_lib().rpf_host_cross_phase(planes.ctypes.data_as(dp), n, ph.ctypes.data_as(dp))
    assert np.array_equal(g, stats.coherence(planes), equal_nan=True) and np.isnan(g[:9]).all() and not np.isnan(g[9:]).any()
    assert np.max(np.abs(ph - stats.cross_phase(planes))) <= 2.0 ** -51        # two atan2 implementations: an ulp of pi


# ---- the identity in float64 -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("N", [64, 500])
def test_four_power_spectra_give_the_cross_spectrum_in_float64(N, windowed):
    frames = 23
    for step in (N, N // 2 + 1):
        samples = N + step * (frames - 1)
        a = synth.uniform_iq(11 + N, samples)
        b = np.roll(a, 6) // 2 + synth.uniform_iq(12 + N, samples) // 2
        window = synth.hann_window(N) if windowed else None
        saa, sbb, sab = truth_cross(a, b, "cu8", N, step, window)
        va, vb = pfb.sample_values(a, "cu8"), pfb.sample_values(b, "cu8")
        # (the window applies to a and b in float32, so u and v are combined AFTER it here: the identity is the subject)
        fa, fb = prepared_frames(va, N, step, window), prepared_frames(vb, N, step, window)
        assert fa.shape == (frames, N)
        p = lambda x: (np.abs(np.fft.fft(x, axis=1)) ** 2).sum(axis=0)
        planes = np.stack([p(fa), p(fb), p(fa + fb), p(fa + 1j * fb)])
        c = planes[0] + planes[1]
        got = 0.5 * (planes[2] - c) + 0.5j * (planes[3] - c)
        err = float(np.max(np.abs(got - sab) / (saa + sbb)))
        print("N=%d step=%d %s: four-plane route vs sum A conj B %.3g of Saa + Sbb" % (N, step, "hann" if windowed else "rect", err))
        assert err < 1e-12
        assert np.array_equal(planes[0], saa) and np.array_equal(planes[1], sbb)


# ---- the recorded CPU float32 figures behind the GPU bar ------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,N,windowed", cross_bars.ACCURACY_CASES)
def test_recorded_cpu_float32_error_is_what_the_cpu_path_gives(fmt, N, windowed):
    """cross_bars.CPU_F32 (half the GPU test's bar) against a fresh run of the path it records."""
    a, b = cross_bars.accuracy_streams(fmt, N)
    window = synth.hann_window(N) if windowed else None
    saa, sbb, sab = truth_cross(a, b, fmt, N, window=window)
    planes = cpu_f32_cross(a, b, fmt, N, window=window)
    err = cross_err(planes, saa, sbb, sab)
    coh = float(np.mean(np.abs(sab) ** 2 / (saa * sbb)))
    key = (fmt, N, windowed)
    print("%s N=%d %s: CPU float32 path vs float64 %.4g (recorded %.4g); mean coherence %.3f"
          % (fmt, N, "hann" if windowed else "rect", err, cross_bars.CPU_F32[key], coh))
    assert 0.35 < coh < 0.65
    assert abs(err / cross_bars.CPU_F32[key] - 1.0) < 0.02


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------

def run_cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True)


def test_cli_parses_the_option():
    r = run_cli("--help")
    assert r.returncode == 0 and "--cross <file>" in r.stdout
    # a good command line: what fails next is not the option (there is no device here, or the files are empty)
    r = run_cli("--input", "/dev/null", "--cross", "/dev/null", "-b", "512", "-q", "--format", "cs16", "-l",
                "--frame-overlap", "50")
    assert r.returncode != 3 and "--cross" not in r.stderr, r.stderr
    r = run_cli("--input", "/dev/null", "--cross")
    assert r.returncode == 4


@pytest.mark.parametrize("other,shown", [(("-n", "10"), "--repeats"), (("-t", "1"), "--time"), (("-c",), "--continue"),
                                         (("-e", "10"), "--elapsed"), (("-f", "100M:200M"), "frequency range"),
                                         (("-m", "out"), "-m"), (("--gpus", "0,1"), "--gpus"), (("--stats",), "--stats"),
                                         (("--series", "4"), "--series"), (("--series-stats", "4"), "--series-stats"),
                                         (("--excise", "4"), "--excise"), (("--quantile", "4"), "--quantile"),
                                         (("--pfb", "4"), "--pfb")])
def test_cli_refuses_what_cross_does_not_combine_with(other, shown):
    r = run_cli("--input", "/dev/null", "--cross", "/dev/null", *other)
    assert r.returncode == 3, r.stderr
    assert "--cross" in r.stderr and shown in r.stderr, r.stderr


def test_cli_cross_needs_input():
    r = run_cli("--cross", "/dev/null")
    assert r.returncode == 3 and "--cross" in r.stderr and "--input" in r.stderr, r.stderr
    r = run_cli("--cross", "-", "--input", "-")
    assert r.returncode == 3 and "stdin" in r.stderr, r.stderr


def test_cli_block_writer():
    """write_spectrum_text_cross: five columns, the DC bin of all four planes interpolated before coherence and phase."""
    N, frames, rate = 8, 10, 2000000
    rng = np.random.default_rng(8)
    planes = np.stack([rng.random(N) + 1.0, rng.random(N) + 1.0, rng.standard_normal(N), rng.standard_normal(N)])
    planes[:, N // 2] = (1e9, 1e9, -1e9, 1e9)
    lines = format_cross_block(planes, frames, N, rate=rate, linear=True)
    assert len(lines) == N
    p = planes.copy()
    p[:, N // 2] = 0.5 * (p[:, N // 2 - 1] + p[:, N // 2 + 1])
    g, ph = stats.coherence(p), stats.cross_phase(p)
    for i, line in enumerate(lines):
        f = [float(x) for x in line.split()]
        assert len(f) == 5
        want = [p[0, i] / frames / N / rate, p[1, i] / frames / N / rate, g[i], ph[i]]
        assert np.allclose(f[1:], want, rtol=2e-5, atol=0), (i, f, want)
