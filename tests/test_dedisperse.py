"""Incoherent dedispersion of the stored integrations, everything that needs no GPU: the three C-ABI additions, the walk of
the kernel's tiles, blocks, spans and LDS indices on the host emulator (tests/emul/dedisperse_emul.cpp over
csrc/dedisperse_core.h) against dedisperse.reference, dm_delays in C++ and in Python, the LDS pitch under
tools/lds_bank_model.py's rules, the CLI options and what they refuse, and the block writer.
tests/test_gpu_dedisperse.py imports the helpers."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, dedisperse
from helpers import ROOT, dp

HEADER = os.path.join(ROOT, "include", "rpf_engine.h")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
ll = ctypes.c_longlong
vp = ctypes.c_void_p
_emul = None
_host = None


# ---- helpers (shared with tests/test_gpu_dedisperse.py) -------------------------------------------------------------------

def emul():
    global _emul
    if _emul is None:
        lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "librpf_emul_dedisperse.so"))
        lib.rpf_emul_dedisperse.restype = ll
        lib.rpf_emul_dedisperse.argtypes = [vp, ll, ctypes.c_int, vp, vp, ctypes.c_int, vp, vp, vp, vp]
        lib.rpf_emul_dedisperse_direct_pairs.restype = ll
        lib.rpf_emul_dedisperse_direct_pairs.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp]
        lib.rpf_emul_dedisperse_times.restype = ll
        lib.rpf_emul_dedisperse_times.argtypes = [ll, ll]
        lib.rpf_emul_dedisperse_lds_index.argtypes = [ctypes.c_int, ctypes.c_int]
        _emul = lib
    return _emul


def TT():
    return emul().rpf_emul_dedisperse_tt()


def DT():
    return emul().rpf_emul_dedisperse_dt()


def BC():
    return emul().rpf_emul_dedisperse_bc()


def host_lib():
    global _host
    if _host is None:
        lib = ctypes.CDLL(os.path.join(ROOT, "rtl-power-fftw_amd", "host", "librpf_host.so"))
        lib.rpf_host_parse_dedisperse.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ll), dp,
                                                  ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
        lib.rpf_host_dm_delays.argtypes = [dp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, ll, ll, vp,
                                           ctypes.c_char_p, ctypes.c_size_t]
        lib.rpf_host_format_text_dedisperse.restype = ctypes.c_long
        lib.rpf_host_format_text_dedisperse.argtypes = [dp, ll, ll, ll, ll, ctypes.c_int, ctypes.c_int, ctypes.c_double, ll,
                                                        ctypes.c_char_p, ctypes.c_size_t]
        _host = lib
    return _host


def same_bits(x, y):
    """Equal as doubles, NaN where the other is NaN."""
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and np.array_equal(x, y, equal_nan=True)


def emul_dedisperse(rows, delays, weights=None):
    """The emulator's walk: (out (D, T), visits (D, T), disorder, direct terms)."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    delays = np.ascontiguousarray(delays, dtype=np.int32)
    K, N = rows.shape
    D = delays.shape[0]
    T = dedisperse.times(K, delays)
    out = np.full(max(D * T, 1), -7.0)
    visits = np.zeros(max(D * T, 1), dtype=np.int32)
    bad, direct = ll(-1), ll(-1)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    got = emul().rpf_emul_dedisperse(rows.ctypes.data, K, N, delays.ctypes.data, None if w is None else w.ctypes.data, D,
                                     out.ctypes.data, visits.ctypes.data, ctypes.byref(bad), ctypes.byref(direct))
    assert got == T
    return out[:D * T].reshape(D, T), visits[:D * T].reshape(D, T), bad.value, direct.value


def direct_share(delays, weights, N):
    """(pairs read straight from the store, (tile, block) pairs that are not empty) of this table."""
    delays = np.ascontiguousarray(delays, dtype=np.int32)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    pairs = ll(0)
    direct = emul().rpf_emul_dedisperse_direct_pairs(delays.ctypes.data, None if w is None else w.ctypes.data, N,
                                                     delays.shape[0], ctypes.byref(pairs))
    return direct, pairs.value


def cli_weights(median):
    """The weights the CLI makes of the per-bin medians: 1 / median, 0 at the DC bin and where the median is 0."""
    median = np.asarray(median, dtype=np.float64)
    w = np.zeros_like(median)
    ok = median != 0
    w[ok] = 1.0 / median[ok]
    w[median.size // 2] = 0.0
    return w


def format_block(trial, nb, L, step, rate, linear, dm, largest):
    """Header and block of one trial by the C++ host's writer, as lines."""
    trial = np.ascontiguousarray(trial, dtype=np.float64)
    buf = ctypes.create_string_buffer(400 + 48 * trial.size)
    n = host_lib().rpf_host_format_text_dedisperse(trial.ctypes.data_as(dp), trial.size, nb, L, step, rate, int(linear), dm,
                                                   largest, buf, len(buf))
    assert n > 0
    return buf.value.decode().split("\n")


def python_block(trial, nb, L, step, rate, linear):
    """The block's data lines as the definition gives them: t L S / rate in nine digits, then the power in six."""
    lines = []
    for t, x in enumerate(np.asarray(trial, dtype=np.float64)):
        with np.errstate(divide="ignore", invalid="ignore"):
            p = x / float(nb)
            v = p if linear else 10 * np.log10(p)
        lines.append("%.9g %s" % (float(t * L * step) / rate, c_six(v)))
    return lines


def c_six(v):
    """A double as a C++ stream writes it at precision 6."""
    if np.isnan(v):
        return "-nan" if np.signbit(v) else "nan"
    if np.isinf(v):
        return "-inf" if v < 0 else "inf"
    return "%.6g" % v


def cpp_dm_delays(dms, fc, rate, N, L, S):
    dms = np.ascontiguousarray(dms, dtype=np.float64)
    out = np.full((dms.size, N), -1, dtype=np.int32)
    msg = ctypes.create_string_buffer(512)
    rc = host_lib().rpf_host_dm_delays(dms.ctypes.data_as(dp), dms.size, fc, rate, N, L, S, out.ctypes.data, msg, 512)
    return rc, out, msg.value.decode()


def parse(*args):
    argv = [b"rpf_power"] + [a.encode() for a in args]
    arr = (ctypes.c_char_p * len(argv))(*argv)
    frames = ll(-1)
    dms = np.full(5000, -1.0)
    msg = ctypes.create_string_buffer(1024)
    n = host_lib().rpf_host_parse_dedisperse(len(argv), arr, ctypes.byref(frames), dms.ctypes.data_as(dp), dms.size, msg, 1024)
    return n, frames.value, dms[:max(n, 0)], msg.value.decode()


# ---- header, binding and library ----------------------------------------------------------------------------------------

def test_header_binding_and_library_agree_on_the_three_symbols():
    text = open(HEADER).read()
    assert re.search(r"\bint rpf_dedisperse_device\(rpf_engine\* e, const int32_t\* delays[^;]*const double\* weights[^;]*"
                     r"int n_trials, double\* d_out[^;]*int64_t capacity[^;]*void\* hip_stream, int64_t\* times[^;]*\);", text)
    assert re.search(r"\bint rpf_dedisperse\(rpf_engine\* e, const int32_t\* delays, const double\* weights, int n_trials, "
                     r"double\* out[^;]*int64_t capacity, int64_t\* times\);", text)
    assert re.search(r"\bint64_t rpf_dedisperse_times\(const rpf_engine\* e, const int32_t\* delays, int n_trials\);", text)
    m = re.search(r"#define RPF_ABI_VERSION 2(.*?)\*/", text, re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in ("rpf_dedisperse_device", "rpf_dedisperse", "rpf_dedisperse_times"):
        assert m and re.search(r"\b%s\b" % name, m.group(1)), name
        assert name in _lib.symbol_names()
        assert re.search(r"\bT %s$" % name, exported, re.M), name
    lib = rpf.load()
    assert lib.rpf_abi_version() == 2
    out, times = np.full(8, -3.0), ctypes.c_int64(-1)
    table = np.zeros(8, dtype=np.int32)
    tp = table.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert lib.rpf_dedisperse(None, tp, None, 1, out.ctypes.data_as(dp), 8, ctypes.byref(times)) == rpf.ReturnValue.InvalidArgument
    assert lib.rpf_dedisperse_device(None, tp, None, 1, None, 8, None, ctypes.byref(times)) == rpf.ReturnValue.InvalidArgument
    assert lib.rpf_dedisperse_times(None, tp, 1) == -1
    assert np.all(out == -3.0)
    for name in ("dedisperse", "dedisperse_device", "dedisperse_times"):
        assert hasattr(rpf.Datastore, name)


# ---- the emulator's walk of the kernel's tiles equals the reference ---------------------------------------------------------

def table(kind, rng, D, N, K):
    if kind == "zero":
        return np.zeros((D, N), dtype=np.int32)
    if kind == "dm":
        return dedisperse.dm_delays(np.arange(D) * 1.5, 408e6, 2.4e6, N, 4)
    if kind == "random_small":                    # spans that fit the LDS tile: every block staged
        return rng.integers(0, TT() + 9, (D, N)).astype(np.int32)
    assert kind == "random_large"                 # spans beyond the LDS tile: every block read straight from the store
    return rng.integers(0, emul().rpf_emul_dedisperse_rows() + 40, (D, N)).astype(np.int32)


@pytest.mark.parametrize("N", [64, 500])
@pytest.mark.parametrize("kind", ["zero", "dm", "random_small", "random_large"])
@pytest.mark.parametrize("weights", ["none", "positive", "zeros"])
def test_the_tile_walk_equals_the_reference_bit_for_bit(N, kind, weights):
    rng = np.random.default_rng([N, len(kind), len(weights)])
    D = DT() + 1
    delays = table(kind, rng, D, N, 0)
    K = int(delays.max()) + 2 * TT() + 3                       # T = 2 TT + 3: three time tiles, the last one ragged
    rows = rng.standard_normal((K, N)) ** 2 * 10.0 ** rng.uniform(-3, 3, (K, N))
    w = None
    if weights != "none":
        w = rng.uniform(0.25, 4.0, N)
    if weights == "zeros":
        w[N // 2] = 0.0
        w[rng.integers(0, N, N // 5)] = 0.0
        w[BC():2 * BC()] = 0.0                                 # one whole block without a bin: skipped
        rows[:, w == 0] = np.nan                               # a bin of weight 0 is not read
    want = dedisperse.reference(rows, delays, w)
    got, visits, disorder, direct = emul_dedisperse(rows, delays, w)
    assert want.shape == (D, 2 * TT() + 3)
    assert same_bits(got, want) and not np.isnan(got).any()
    # every (d, t, b) of non-zero weight exactly once, in ascending b; no LDS cell read that was not staged
    assert disorder == 0
    assert np.all(visits == (N if w is None else np.count_nonzero(w)))
    took, pairs = direct_share(delays, w, N)
    if kind == "random_large":
        assert direct > 0 and took == pairs
    else:
        assert direct == 0 and took == 0 and pairs > 0


def test_the_mixed_table_takes_both_routes():
    rng = np.random.default_rng(5)
    N, D = 96, 3
    delays = rng.integers(0, 20, (D, N)).astype(np.int32)
    delays[1, 40] = 400                                         # block 1 of the one tile: direct; blocks 0 and 2: staged
    rows = rng.standard_normal((500, N))
    got, visits, disorder, direct = emul_dedisperse(rows, delays)
    assert same_bits(got, dedisperse.reference(rows, delays)) and disorder == 0 and np.all(visits == N)
    assert direct_share(delays, None, N) == (1, 3) and direct == D * got.shape[1] * BC()


def test_t_is_k_minus_the_largest_delay():
    assert [emul().rpf_emul_dedisperse_times(K, d) for K, d in ((10, 0), (10, 9), (10, 10), (10, 11), (0, 0))] == [10, 1, 0, 0, 0]
    rows = np.arange(12.0).reshape(4, 3)
    assert dedisperse.reference(rows, [[0, 3, 0]]).shape == (1, 1)
    assert dedisperse.reference(rows, [[0, 4, 0]]).shape == (1, 0)
    out, _, disorder, _ = emul_dedisperse(rows, np.array([[0, 3, 1]], dtype=np.int32))
    assert out.tolist() == [[0.0 + 10.0 + 5.0]] and disorder == 0


def test_a_wave_reads_one_bin_at_64_rows_without_a_bank_conflict():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lds_bank_model as model
    pitch = emul().rpf_emul_dedisperse_pitch()
    assert pitch % 2 == 1 and pitch >= BC()
    for col in (0, 1, BC() - 1):
        for first in (0, 37):
            dwords = [2 * emul().rpf_emul_dedisperse_lds_index(first + lane, col) for lane in range(64)]
            assert model.cycles(dwords, model.G32, 64, 2) == (2, 2)             # ds_read_b64: two groups, one cycle each
    # the staging stores: 16 consecutive lanes write 16 consecutive bins of one row
    dwords = [2 * emul().rpf_emul_dedisperse_lds_index(lane // BC(), lane % BC()) for lane in range(64)]
    assert model.cycles(dwords, model.G16, 32, 2) == (4, 4)                     # ds_write_b64: four groups, one cycle each
    assert 8 * pitch * emul().rpf_emul_dedisperse_rows() <= 65536


# ---- dm_delays ---------------------------------------------------------------------------------------------------------------

def test_cpp_and_python_dm_delays_agree_on_a_grid():
    dms = np.array([0.0, 0.3, 1.0, 15.0, 56.78, 300.0, 2500.0])
    checked = 0
    for fc in (151.3e6, 408e6, 1420405752.0):
        for rate in (250000.0, 2.4e6, 3.2e6):
            for N in (8, 64, 500, 4096):
                for L, S in ((1, N), (4, N), (16, N // 2), (128, N), (3, N // 4 * 3)):
                    want = dedisperse.dm_delays(dms, fc, rate, N, L, S)
                    rc, got, msg = cpp_dm_delays(dms, fc, rate, N, L, S)
                    assert rc == 0, msg
                    assert np.array_equal(got, want), (fc, rate, N, L, S)
                    assert np.all(want[:, -1] == 0) and np.all(want[0] == 0) and np.all(np.diff(want, axis=1) <= 0)
                    checked += 1
    assert checked == 180
    # the issue's case: 2.4 MHz at 408 MHz, DM 15, rows of 4 frames of 64 bins
    d = dedisperse.dm_delays(np.arange(31.0), 408e6, 2.4e6, 64, 4)
    assert d.shape == (31, 64) and d.dtype == np.int32 and d.max() == 81 and d[15].max() == 41


def test_dm_delays_refuses_in_both_languages():
    for dms, fc, word in (([-1.0], 408e6, "negative"), ([float("nan")], 408e6, "finite"), ([float("inf")], 408e6, "finite"),
                          ([1.0], 1.0e6, "lowest bin"), ([1e12], 408e6, "32 bits")):
        with pytest.raises(ValueError):
            dedisperse.dm_delays(dms, fc, 2.4e6, 64, 4)
        rc, _, msg = cpp_dm_delays(dms, fc, 2.4e6, 64, 4, 64)
        assert rc == -3 and word in msg, msg


def test_snr_is_the_deviation_in_robust_sigmas():
    rng = np.random.default_rng(3)
    plane = rng.standard_normal((3, 2001)) * np.array([[1.0], [5.0], [0.1]]) + np.array([[10.0], [-2.0], [0.0]])
    plane[1, 700] += 100.0
    s = dedisperse.snr(plane)
    assert s.shape == plane.shape and np.unravel_index(np.argmax(s), s.shape) == (1, 700)
    assert np.allclose(np.median(s, axis=1), 0) and np.allclose(np.median(np.abs(s), axis=1), 1 / 1.4826)
    assert 18 < s[1, 700] < 22


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------

def run_cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True)


def test_cli_parses_the_options():
    r = run_cli("--help")                    # (the --help text is the one tests/golden/cli_refusals.json pins)
    assert r.returncode == 0 and "--dedisperse" not in r.stdout and "--dm" not in r.stdout
    n, frames, dms, msg = parse("--input", "x", "--dedisperse", "16", "--dm", "0:30:1")
    assert (n, frames) == (31, 16) and np.array_equal(dms, np.arange(31.0)), msg
    n, frames, dms, msg = parse("--input", "x", "--dedisperse", "1", "--dm", "56.78")
    assert (n, frames) == (1, 1) and dms.tolist() == [56.78]
    n, _, dms, _ = parse("--input", "x", "--dedisperse", "4", "--dm", "0.1:0.4:0.1")       # lo + i step, i <= (hi - lo) / step + 1e-9
    assert n == 4 and dms.tolist() == [0.1 + i * 0.1 for i in range(4)]
    n, _, dms, _ = parse("--input", "x", "--dedisperse", "4", "--dm", "5:5.9:1")
    assert n == 1 and dms.tolist() == [5.0]
    n, _, dms, _ = parse("--input", "x", "--dedisperse", "4", "--dm", "0:4095:1")
    assert n == 4096
    assert parse("--input", "x", "-b", "64")[:2] == (0, 0)
    # a good command line: what fails next is not the option (there is no device here, or the file is empty)
    r = run_cli("--input", "/dev/null", "--dedisperse", "4", "--dm", "0:30:1", "-b", "64", "-q", "--format", "cs16", "-l",
                "--frame-overlap", "50", "-w", "/dev/null")
    assert "--dedisperse" not in r.stderr and "--dm" not in r.stderr, r.stderr


@pytest.mark.parametrize("other,shown", [(("-n", "10"), "--repeats"), (("-t", "1"), "--time"), (("-c",), "--continue"),
                                         (("-e", "10"), "--elapsed"), (("-f", "100M:200M"), "frequency range"),
                                         (("-m", "out"), "-m"), (("-B", "/dev/null"), "--baseline"),
                                         (("--gpus", "0,1"), "--gpus"), (("--stats",), "--stats"),
                                         (("--series", "4"), "--series"), (("--series-stats", "4"), "--series-stats"),
                                         (("--excise", "4"), "--excise"), (("--quantile", "4"), "--quantile"),
                                         (("--cross", "/dev/null"), "--cross"), (("--stft", "/dev/null"), "--stft"),
                                         (("--correlate", "/dev/null"), "--correlate"), (("--pfb", "4"), "--pfb")])
def test_cli_refuses_what_dedisperse_does_not_combine_with(other, shown):
    r = run_cli("--input", "/dev/null", "--dedisperse", "4", "--dm", "0:10:1", *other)
    assert r.returncode == 3, r.stderr
    assert shown in r.stderr and "Exiting." in r.stderr, r.stderr
    if shown in ("--repeats", "--time", "--continue", "--elapsed", "frequency range", "-m", "--baseline", "--gpus", "--stats",
                 "--pfb"):
        assert "--dedisperse" in r.stderr, r.stderr                # (with another replay mode, the first one's refusal speaks)


def test_cli_dedisperse_refuses_its_own_misuse():
    r = run_cli("--dedisperse", "4", "--dm", "1")
    assert r.returncode == 3 and "--dedisperse" in r.stderr and "--input" in r.stderr, r.stderr
    r = run_cli("--input", "/dev/null", "--dedisperse", "4")
    assert r.returncode == 3 and "--dedisperse" in r.stderr and "--dm" in r.stderr, r.stderr
    r = run_cli("--input", "/dev/null", "--dm", "1")
    assert r.returncode == 3 and "--dm needs --dedisperse" in r.stderr, r.stderr
    r = run_cli("--input", "/dev/null", "--dedisperse", "0", "--dm", "1")
    assert r.returncode == 3 and "at least 1" in r.stderr, r.stderr
    for bad in ("", "a", "1:2", "1:2:3:4", "2:1:1", "0:10:0", "0:10:-1", "-1", "nan", "inf", "0:inf:1", "1:", ":1:1", " 1", "1 ", "0x10", "0:0x10:1",
                "infinity"):
        r = run_cli("--input", "/dev/null", "--dedisperse", "4", "--dm", bad)
        assert r.returncode == 3 and "--dedisperse" in r.stderr and "--dm" in r.stderr, (bad, r.stderr)
    r = run_cli("--input", "/dev/null", "--dedisperse", "4", "--dm", "0:4096:1")
    assert r.returncode == 3 and "at most 4096 trials" in r.stderr and "4097" in r.stderr, r.stderr


@pytest.mark.parametrize("linear", [False, True])
def test_cli_block_writer(linear):
    rng = np.random.default_rng(11)
    L, S, rate, nb = 4, 64, 2400000, 63
    trial = rng.uniform(50.0, 80.0, 175)
    trial[3] = 0.0                      # -inf in dB
    trial[5] = np.nan
    lines = format_block(trial, nb, L, S, rate, linear, 15.0, 40)
    assert lines[0] == "# rtl-power-fftw output" and lines[1] == "# Acquisition start: a" and lines[2] == "# Acquisition end: b"
    assert lines[3] == "# DM 15 pc cm^-3, largest delay 40 integrations"
    assert lines[4] == "#" and lines[5] == "# time [s] power [median units]"
    assert lines[6 + trial.size:] == ["", ""]                                   # the blank line that ends a block
    assert lines[6:6 + trial.size] == python_block(trial, nb, L, S, rate, linear)
    first = lines[6].split()
    assert float(first[0]) == 0.0 and float(lines[7].split()[0]) == pytest.approx(L * S / rate, rel=1e-8)
    value = trial[0] / nb
    assert float(first[1]) == pytest.approx(value if linear else 10 * np.log10(value), rel=1e-5)
    assert format_block(trial, nb, L, S, rate, linear, 0.25, 0)[3] == "# DM 0.25 pc cm^-3, largest delay 0 integrations"
