"""Per-bin statistics (RPF_FLAG_BIN_STATS: S2 = sum of the squared frame powers and PK = peak hold beside the power,
the spectral kurtosis from them), the parts that need no GPU: the host build of K1's statistics accumulate and its
slot / partial combine against the definitions and the CPU float32 path, the estimator in Python and C++, the text
writer, the CLI option and the C-ABI additions."""
import ctypes
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, stats, synth
import helpers
from helpers import ROOT, dp, fp, u8p
from stats_bars import EMUL_VS_ORACLE_FRAME

HEADER = os.path.join(ROOT, "include", "rpf_engine.h")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")

_emul = None


def emul_stats_lib():
    global _emul
    if _emul is None:
        lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "librpf_emul_stats.so"))
        lib.rpf_emul_stats.argtypes = [ctypes.c_int, fp, u8p, ctypes.c_long, ctypes.c_int, ctypes.c_int, dp, fp]
        _emul = lib
    return _emul


def emul_stats(N, stream, nframes, slots=1, groups=1, window=None, want_spectra=False):
    stream = np.ascontiguousarray(stream, dtype=np.uint8)
    out = np.zeros((3, N))
    spectra = np.zeros((nframes, N, 2), dtype=np.float32) if want_spectra else None
    w = None
    if window is not None:
        window = np.ascontiguousarray(window, dtype=np.float32)
        w = window.ctypes.data_as(fp)
    rc = emul_stats_lib().rpf_emul_stats(N, w, stream.ctypes.data_as(u8p), nframes, slots, groups, out.ctypes.data_as(dp),
                                         None if spectra is None else spectra.ctypes.data_as(fp))
    assert rc == 0, rc
    return out, spectra


def fma(a, b, c):
    """round(a * b + c), correctly rounded, for doubles (float(Fraction) rounds to nearest even)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def by_definition(spectra, frame_order):
    """S1, S2, PK of one accumulator from float32 spectra (frames x N x 2), the header's definitions literally."""
    N = spectra.shape[1]
    s1, s2, pk = [0.0] * N, [0.0] * N, [0.0] * N
    for f in frame_order:
        re = spectra[f, :, 0].astype(np.float64)
        im = spectra[f, :, 1].astype(np.float64)
        for k in range(N):
            r, i = float(re[k]), float(im[k])
            s1[k] = fma(i, i, fma(r, r, s1[k]))
            p = fma(i, i, r * r)
            assert p == r * r + i * i          # both squares are exact in double: one rounding either way
            s2[k] = fma(p, p, s2[k])
            pk[k] = max(pk[k], p)
    return np.array([s1, s2, pk])


def oracle_frame_powers(N, stream, nframes, window=None):
    """p of every frame and bin on the CPU float32 path: rpf_oracle_fft_f32 on the exactly unpacked frame."""
    orc = helpers.oracle_lib()
    plan = orc.rpf_oracle_plan_create(N)
    sign = (1 - 2 * (np.arange(N) % 2)).astype(np.float32)
    out = np.zeros((nframes, N))
    try:
        for f in range(nframes):
            x = np.asarray(stream[2 * N * f: 2 * N * (f + 1)]).astype(np.float32).reshape(N, 2) - np.float32(127.0)
            x = x * sign[:, None]
            if window is not None:
                x = x * np.asarray(window, dtype=np.float32)[:, None]
            x = np.ascontiguousarray(x, dtype=np.float32)
            y = np.zeros((N, 2), dtype=np.float32)
            orc.rpf_oracle_fft_f32(plan, x.ctypes.data_as(fp), y.ctypes.data_as(fp))
            re, im = y[:, 0].astype(np.float64), y[:, 1].astype(np.float64)
            out[f] = re * re + im * im
    finally:
        orc.rpf_oracle_plan_destroy(plan)
    return out


@pytest.mark.parametrize("N,frames", [(64, 12), (512, 7), (4096, 3)])
def test_emulated_accumulate_follows_the_definitions(N, frames):
    stream = synth.noise_tones_iq(41, N * frames)
    P = emul_stats_lib().rpf_emul_stats_p(N)
    got, spectra = emul_stats(N, stream, frames, want_spectra=True)
    # the power is untouched: the same instruction sequence as the plain accumulate
    assert np.array_equal(got[0], helpers.emul_accumulate(N, P, stream, frames))
    want = by_definition(spectra, range(frames))
    assert np.array_equal(got, want)
    # one frame: PK == S1 and S2 == S1 * S1
    one, _ = emul_stats(N, stream, 1)
    assert np.array_equal(one[2], one[0]) and np.array_equal(one[1], one[0] * one[0])
    # and p is what the CPU float32 path gives for that frame, to float32 accuracy
    p_emul = spectra[..., 0].astype(np.float64) ** 2 + spectra[..., 1].astype(np.float64) ** 2
    p_orc = oracle_frame_powers(N, stream, frames)
    for f in range(frames):
        err = np.max(np.abs(p_emul[f] - p_orc[f]) / np.maximum(p_orc[f], p_orc[f].mean()))
        assert err < EMUL_VS_ORACLE_FRAME, (f, err)
    assert np.array_equal(got[2], p_emul.max(axis=0))
    assert np.array_equal(np.argmax(p_emul, axis=0), np.argmax(p_orc, axis=0)) or \
        helpers.max_rel(p_orc.max(axis=0), got[2]) < 10 * EMUL_VS_ORACLE_FRAME


@pytest.mark.parametrize("N,frames,slots,groups", [(64, 23, 4, 3), (512, 11, 2, 2), (4096, 5, 2, 2)])
def test_emulated_slot_and_partial_combine(N, frames, slots, groups):
    """Frame f -> workgroup (f / slots) mod groups, slot f mod slots; slots combine from 0 in slot order, workgroups
    in workgroup order, by +, +, max -- restated here on the emulator's own per-frame spectra."""
    stream = synth.uniform_iq(41, N * frames)
    got, spectra = emul_stats(N, stream, frames, slots=slots, groups=groups, want_spectra=True)
    total = np.zeros((3, N))
    for wg in range(groups):
        part = np.zeros((3, N))
        for k in range(slots):
            mine = [f for f in range(frames) if (f // slots) % groups == wg and f % slots == k]
            acc = by_definition(spectra, mine)
            part[0] += acc[0]
            part[1] += acc[1]
            part[2] = np.maximum(part[2], acc[2])
        total[0] += part[0]
        total[1] += part[1]
        total[2] = np.maximum(total[2], part[2])
    assert np.array_equal(got, total)
    # the maximum does not care how the frames were dealt; the sums only regroup double additions
    flat, _ = emul_stats(N, stream, frames)
    assert np.array_equal(got[2], flat[2])
    assert helpers.max_rel(got[0], flat[0]) < 1e-12 and helpers.max_rel(got[1], flat[1]) < 1e-12
    # a windowed run goes through the same code
    win = np.hanning(N).astype(np.float32)
    w, ws = emul_stats(N, stream, 2, window=win, want_spectra=True)
    assert np.array_equal(w, by_definition(ws, range(2)))


def host_lib():
    lib = ctypes.CDLL(os.path.join(ROOT, "rtl-power-fftw_amd", "host", "librpf_host.so"))
    lib.rpf_host_spectral_kurtosis.argtypes = [dp, dp, ctypes.c_longlong, dp, ctypes.c_int]
    lib.rpf_host_spectral_kurtosis.restype = None
    lib.rpf_host_format_text_stats.restype = ctypes.c_long
    lib.rpf_host_format_text_stats.argtypes = [dp, dp, dp, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int,
                                               ctypes.c_int, dp, ctypes.c_char_p, ctypes.c_size_t]
    lib.rpf_host_format_text.restype = ctypes.c_long
    lib.rpf_host_format_text.argtypes = [dp, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                         dp, ctypes.c_char_p, ctypes.c_size_t]
    lib.rpf_host_format_header.restype = ctypes.c_long
    lib.rpf_host_format_header.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    return lib


def test_spectral_kurtosis_formula():
    M = 50
    p = np.array([3.0, 1e-9, 7.5e12])
    sk = stats.spectral_kurtosis(M * p, M * p * p, M)           # a constant power: M S2 / S1^2 = 1
    assert np.all(np.abs(sk) < 1e-14)
    # exponentially distributed powers (Gaussian noise): E p^2 = 2 (E p)^2, so SK -> 1
    rng = np.random.default_rng(7)
    x = rng.exponential(2.0, size=(4000, 16))
    sk = stats.spectral_kurtosis(x.sum(axis=0), (x * x).sum(axis=0), 4000)
    assert np.all(np.abs(sk - 1) < 6 * 2 / math.sqrt(4000))
    # one frame in ten carries everything: M S2 / S1^2 = 10
    on = np.zeros(1000)
    on[::10] = 5.0
    assert abs(stats.spectral_kurtosis(on.sum(), (on * on).sum(), 1000) - (1001 / 999) * 9) < 1e-12
    # by hand
    assert stats.spectral_kurtosis(np.array([6.0]), np.array([14.0]), 3)[0] == (4.0 / 2.0) * (3 * 14.0 / 36.0 - 1.0)
    # undefined: fewer than two frames, or no power at all
    assert np.all(np.isnan(stats.spectral_kurtosis(p, p * p, 1))) and np.all(np.isnan(stats.spectral_kurtosis(p, p * p, 0)))
    got = stats.spectral_kurtosis(np.array([0.0, 2.0]), np.array([0.0, 3.0]), 5)
    assert np.isnan(got[0]) and not np.isnan(got[1])


def test_spectral_kurtosis_python_equals_cpp_to_the_last_bit():
    rng = np.random.default_rng(11)
    lib = host_lib()
    for M in (2, 3, 80, 1000, 123457):
        s1 = rng.exponential(1.0, 5000) * 10.0 ** rng.uniform(-6, 12, 5000)
        s2 = s1 * s1 / M * rng.uniform(1.0, M, 5000)
        s1[::97] = 0.0
        out = np.zeros(5000)
        lib.rpf_host_spectral_kurtosis(s1.ctypes.data_as(dp), s2.ctypes.data_as(dp), M, out.ctypes.data_as(dp), 5000)
        want = stats.spectral_kurtosis(s1, s2, M)
        assert np.array_equal(np.isnan(out), np.isnan(want)) and np.isnan(out[0])
        assert np.array_equal(out[~np.isnan(out)], want[~np.isnan(want)])
    one = np.zeros(3)
    lib.rpf_host_spectral_kurtosis(np.ones(3).ctypes.data_as(dp), np.ones(3).ctypes.data_as(dp), 1, one.ctypes.data_as(dp), 3)
    assert np.all(np.isnan(one))


def g6(v):
    return "%.6g" % v


def stats_text(pwr, s2, pk, N, M, tuned, rate, linear, baseline):
    """The --stats writer restated: frequency, power, peak hold (no division by M), spectral kurtosis."""
    pwr, pk = pwr.copy(), pk.copy()
    sk = stats.spectral_kurtosis(pwr, s2, M)
    for col in (sk, pwr, pk):
        col[N // 2] = (col[N // 2 - 1] + col[N // 2 + 1]) / 2
    digits = int(math.ceil(math.floor(math.log10(float(tuned))) - math.log10(rate // N) + 1 + 2))

    def value(acc, i, reps):
        p = acc[i] / reps / N / rate
        b = baseline[i] if baseline is not None else 0
        return (p if linear else (10 * math.log10(p) if p > 0 else -math.inf)) - b

    lines = []
    for i in range(N):
        freq = tuned + (i - N / 2.0) * rate / N
        lines.append("%s %s %s %s\n" % ("%.*g" % (digits, freq), g6(value(pwr, i, M)), g6(value(pk, i, 1)), g6(sk[i])))
    return "".join(lines) + "\n"


@pytest.mark.parametrize("linear,with_baseline", [(0, False), (1, False), (0, True), (1, True)])
def test_stats_writer_bytes(linear, with_baseline):
    N, M, tuned, rate = 64, 37, 1420405752, 2000000
    rng = np.random.default_rng(3)
    frames = rng.exponential(1.0, size=(M, N)) * 1e5
    pwr, s2, pk = frames.sum(axis=0), (frames * frames).sum(axis=0), frames.max(axis=0)
    pwr[5] = s2[5] = pk[5] = 0.0                           # a bin without power: -inf dB (linear: 0) and "nan"
    baseline = rng.normal(0, 3, N) if with_baseline else None
    lib = host_lib()
    buf = ctypes.create_string_buffer(1 << 16)
    a, b, c = pwr.copy(), s2.copy(), pk.copy()
    n = lib.rpf_host_format_text_stats(a.ctypes.data_as(dp), b.ctypes.data_as(dp), c.ctypes.data_as(dp), N, M, tuned, rate,
                                       linear, None if baseline is None else baseline.ctypes.data_as(dp), buf, len(buf))
    assert n > 0
    text = buf.value.decode()
    assert text == stats_text(pwr, s2, pk, N, M, tuned, rate, linear, baseline)
    assert " nan\n" in text and text.count("\n") == N + 1
    assert len(text.splitlines()[0].split()) == 4
    # the DC bin of the arrays handed back is the mean of its neighbours, sum_sq is left alone
    assert a[N // 2] == (pwr[N // 2 - 1] + pwr[N // 2 + 1]) / 2 and c[N // 2] == (pk[N // 2 - 1] + pk[N // 2 + 1]) / 2
    assert np.array_equal(b, s2)

    # without --stats the writer is still the reference's, byte for byte
    orc = helpers.oracle_lib()
    safe = pwr.copy()
    safe[5] = 1.0
    x, y = safe.copy(), safe.copy()
    buf2, buf3 = ctypes.create_string_buffer(1 << 16), ctypes.create_string_buffer(1 << 16)
    bl = None if baseline is None else baseline.ctypes.data_as(dp)
    assert lib.rpf_host_format_text(x.ctypes.data_as(dp), N, M, tuned, rate, linear, bl, buf2, len(buf2)) > 0
    assert orc.rpf_oracle_format_text(y.ctypes.data_as(dp), N, M, tuned, rate, linear, bl, buf3, len(buf3)) > 0
    assert buf2.value == buf3.value
    # and its first two columns are the stats writer's first two
    s, t = safe.copy(), safe.copy()
    lib.rpf_host_format_text_stats(s.ctypes.data_as(dp), b.ctypes.data_as(dp), c.ctypes.data_as(dp), N, M, tuned, rate,
                                   linear, bl, buf, len(buf))
    assert [l.split()[:2] for l in buf.value.decode().splitlines()] == [l.split() for l in buf2.value.decode().splitlines()]


def test_header_line_names_the_columns():
    lib = host_lib()
    buf = ctypes.create_string_buffer(4096)
    assert lib.rpf_host_format_header(b"A", b"B", 1, buf, len(buf)) > 0
    lines = buf.value.decode().splitlines()
    assert lines[-1] == "# frequency [Hz] power spectral density [dB/Hz] peak hold [dB/Hz] spectral kurtosis"
    assert lib.rpf_host_format_header(b"A", b"B", 0, buf, len(buf)) > 0
    plain = buf.value.decode().splitlines()
    assert plain[-1] == "# frequency [Hz] power spectral density [dB/Hz]" and plain[:-1] == lines[:-1]
    assert plain[:4] == ["# rtl-power-fftw output", "# Acquisition start: A", "# Acquisition end: B", "#"]


def run_cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True)


def test_cli_stats_option():
    r = run_cli("--help")
    assert r.returncode == 0 and "--stats" in r.stdout
    r = run_cli("--stats", "-m", "x", "--synthetic", "1")
    assert r.returncode == 3 and "--stats" in r.stderr, r.stderr
    assert not os.path.exists("x.bin")
    r = run_cli("--stats", "--gpus", "0,1", "--synthetic", "1")
    assert r.returncode == 3 and "--stats" in r.stderr, r.stderr


def test_header_binding_and_library_agree(tmp_path):
    src = tmp_path / "consts.c"
    src.write_text('#include <stdio.h>\n#include "rpf_engine.h"\n'
                   'int main(void) { printf("%u %d\\n", RPF_FLAG_BIN_STATS, RPF_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "consts"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    flag, abi = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert flag == _lib.FLAG_BIN_STATS == 32 and abi == 2
    others = [_lib.FLAG_NO_LDS_DMA, _lib.FLAG_FOURSTEP_FUSED, _lib.FLAG_NO_MIXED_RADIX, _lib.FLAG_NO_FOURSTEP_FUSED,
              _lib.FLAG_CATCH_ALL, 0xff << 8, 0xf << 16]
    assert all(flag & o == 0 for o in others)
    text = open(HEADER).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in ("rpf_has_bin_stats", "rpf_get_bin_stats", "rpf_accumulate_device_stats"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _lib.symbol_names()
        assert re.search(r"\bT %s$" % name, exported, re.M), name
    lib = rpf.load()
    assert lib.rpf_has_bin_stats(None) == 0
    assert lib.rpf_get_bin_stats(None, None, None) == rpf.ReturnValue.InvalidArgument
    assert rpf.Params(N=512).bin_stats is False and rpf.Params(N=512, bin_stats=True).bin_stats is True


@pytest.mark.parametrize("flags", [_lib.FLAG_BIN_STATS | _lib.FLAG_FOURSTEP_FUSED, _lib.FLAG_BIN_STATS | (1 << 8),
                                   _lib.FLAG_BIN_STATS | (60 << 8)])
def test_invalid_flag_combinations_before_any_device(flags):
    N = 65536 if flags & _lib.FLAG_FOURSTEP_FUSED else 4096
    with pytest.raises(rpf.RPFError) as e:
        rpf.Datastore(rpf.Params(N=N), flags=flags)
    assert e.value.retval == rpf.ReturnValue.InvalidArgument and "RPF_FLAG_BIN_STATS" in str(e.value)


def test_valid_stats_configurations_get_as_far_as_the_device():
    """On a machine without a GPU a configuration that passes validation fails with HardwareError (no CPU path); with
    one it is created.  Either way it is not InvalidArgument: K1 sizes, catch-all sizes, every format, a frame step."""
    for kw in (dict(N=4096), dict(N=5000), dict(N=4096, sample_format="cs16", frame_step=2049), dict(N=65536)):
        try:
            with rpf.Datastore(rpf.Params(bin_stats=True, **kw)) as ds:
                assert ds.has_bin_stats and ds.sum_sq.shape == (kw["N"],) and ds.peak.shape == (kw["N"],)
        except rpf.RPFError as e:
            assert e.retval == rpf.ReturnValue.HardwareError, (kw, str(e))
