"""The excised average (SK-flagged integrations left out of the sum), the parts that need no GPU: the C-ABI additions,
stats.sk_limits and stats.excise, the kernels' element step and addition order on the host (tests/emul/excise_emul.cpp
compiles csrc/excise_core.h, the text the kernels compile), the CLI's options and its block writer.

The reference is stats.excise, the numpy statement of the definition in include/rpf_engine.h."""
import ctypes
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, stats
from helpers import ROOT
from excise_bars import ADDITIVITY

HEADER = os.path.join(ROOT, "include", "rpf_engine.h")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
NEW = ("rpf_accumulate_device_excised", "rpf_accumulate_excised")
INF = float("inf")


def err_over_total(got, want, total):
    """Worst |got - want| relative to the bin's total (the scale of every sum of the bin; a bin whose total is 0 holds
    zeros only and is compared absolutely)."""
    total = np.asarray(total, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.where(total > 0, total, 1.0)))


def host_lib():
    return ctypes.CDLL(os.path.join(ROOT, "rtl-power-fftw_amd", "host", "librpf_host.so"))


# ---- interface agreement ------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_excised_entries(tmp_path):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"\s+", " ", text)
    assert ("int rpf_accumulate_device_excised(rpf_engine* e, const void* d_stream, size_t nbytes, "
            "int64_t frames_per_spectrum, int64_t max_spectra, double sk_lo, double sk_hi, double* d_out , "
            "uint8_t* d_mask , void* hip_stream, int64_t* spectra_done);") in text
    assert ("int rpf_accumulate_excised(rpf_engine* e, const uint8_t* stream, size_t nbytes, "
            "int64_t frames_per_spectrum, int64_t max_spectra, double sk_lo, double sk_hi, double* out , "
            "uint8_t* mask , int64_t* spectra_done);") in text
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True,
                              check=True).stdout
    sym = {s[0]: s for s in _lib._SYMBOLS}
    for name in NEW:
        assert name in _lib.symbol_names()
        assert re.search(r"\bT %s$" % name, exported, re.M), name
    P, i64, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
    assert sym["rpf_accumulate_device_excised"][1:] == (
        ctypes.c_int, [P, P, ctypes.c_size_t, i64, i64, dbl, dbl, P, P, P, ctypes.POINTER(i64)])
    assert sym["rpf_accumulate_excised"][1:] == (
        ctypes.c_int, [P, P, ctypes.c_size_t, i64, i64, dbl, dbl, ctypes.POINTER(dbl), ctypes.POINTER(ctypes.c_uint8),
                       ctypes.POINTER(i64)])
    # the ABI version did not move: the entries are additive within 2, and the header's comment lists them
    assert re.search(r"#define RPF_ABI_VERSION 2\b", open(HEADER).read())
    comment = open(HEADER).read().split("#define RPF_ABI_VERSION 2", 1)[1].split("*/", 1)[0]
    assert all(name in comment for name in NEW)
    lib = rpf.load()
    assert lib.rpf_abi_version() == 2
    # NULL engine: invalid argument, nothing dereferenced
    assert lib.rpf_accumulate_device_excised(None, None, 0, 2, 1, 0.0, 2.0, None, None, None, None) == rpf.ReturnValue.InvalidArgument
    assert lib.rpf_accumulate_excised(None, None, 0, 2, 1, 0.0, 2.0, None, None, None) == rpf.ReturnValue.InvalidArgument
    for method in ("accumulate_device_excised", "accumulate_excised"):
        assert callable(getattr(rpf.Datastore, method))
    host = host_lib()
    assert host.rpf_host_accumulate_excised and host.rpf_host_sk_limits


# ---- thresholds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 64, 1000])
def test_sk_limits_is_the_closed_form(M):
    var = Fraction(4 * M * M, (M - 1) * (M + 2) * (M + 3))             # exact
    for sigma in (3.0, 1.0, 4.5):
        d = sigma * math.sqrt(var)
        lo, hi = stats.sk_limits(M, sigma)
        assert isinstance(lo, float) and isinstance(hi, float)
        assert abs(hi - (1.0 + d)) <= 4e-16 * (1.0 + d)
        assert abs(lo - max(1.0 - d, 0.0)) <= 4e-16 and lo >= 0.0
    assert stats.sk_limits(M) == stats.sk_limits(M, 3.0)
    if M == 2:
        assert stats.sk_limits(2)[0] == 0.0                            # 1 - 3 sqrt(0.8) < 0: clipped
    if M == 64:
        assert abs(math.sqrt(var) - 0.2425) < 1e-4                     # the figure series_stats_bars.py quotes


def test_sk_limits_refuses_fewer_than_two_frames_and_the_cpp_host_agrees():
    for M in (1, 0, -5):
        with pytest.raises(ValueError):
            stats.sk_limits(M)
    host = host_lib()
    fn = host.rpf_host_sk_limits
    fn.argtypes = [ctypes.c_longlong, ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                   ctypes.c_char_p, ctypes.c_size_t]
    msg = ctypes.create_string_buffer(256)
    lo, hi = ctypes.c_double(), ctypes.c_double()
    for M in (2, 3, 16, 64, 1000, 100000):
        for sigma in (3.0, 0.0, 2.5):
            assert fn(M, sigma, ctypes.byref(lo), ctypes.byref(hi), msg, 256) == 0
            assert (lo.value, hi.value) == stats.sk_limits(M, sigma), (M, sigma)      # the same operations: the same bits
    assert fn(1, 3.0, ctypes.byref(lo), ctypes.byref(hi), msg, 256) == -3 and b"at least 2" in msg.value


# ---- stats.excise -------------------------------------------------------------------------------------------------
def test_stats_excise_is_the_definition_row_by_row():
    rng = np.random.default_rng(5)
    K, L, N = 7, 16, 6
    p = rng.exponential(size=(K, L, N))
    rows = np.stack([p.sum(axis=1), (p * p).sum(axis=1), p.max(axis=1)], axis=1)
    rows[2, :2, 3] = 0.0                                                # S1 = 0: NaN, flagged whatever the thresholds
    lo, hi = 0.7, 1.4
    out, mask = stats.excise(rows, L, lo, hi)
    assert out.shape == (3, N) and mask.shape == (K, N) and mask.dtype == np.uint8
    for b in range(N):
        clean = kept = total = 0.0
        for k in range(K):
            sk = stats.spectral_kurtosis(rows[k, 0, b], rows[k, 1, b], L)
            keep = bool(lo <= sk <= hi)
            assert mask[k, b] == (0 if keep else 1)
            total += rows[k, 0, b]
            if keep:
                clean += rows[k, 0, b]
                kept += 1
        assert out[1, b] == kept and abs(out[0, b] - clean) <= 1e-14 * total and abs(out[2, b] - total) <= 1e-14 * total
    assert mask[2, 3] == 1
    assert 0 < mask.sum() < K * N                                       # the thresholds cut the sample somewhere


# ---- the kernels' element step and addition order, on the host -----------------------------------------------------
@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "librpf_emul_excise.so"))
    ll, i, d, pd = ctypes.c_longlong, ctypes.c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_double)
    lib.rpf_emul_excise.restype = ll
    lib.rpf_emul_excise.argtypes = [pd, ll, i, ll, d, d, ll, pd, ctypes.POINTER(ctypes.c_uint8)]
    lib.rpf_emul_excise_sk.restype = None
    lib.rpf_emul_excise_sk.argtypes = [pd, pd, ll, pd, ll]
    lib.rpf_emul_excise_groups.argtypes = [i]
    return lib


def emulate(emul, rows, L, lo, hi, piece, want_mask=True):
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    K, _, N = rows.shape
    pd = ctypes.POINTER(ctypes.c_double)
    out = np.full((3, N), -1.0)
    mask = np.full((K, N), 7, dtype=np.uint8) if want_mask else None
    pieces = emul.rpf_emul_excise(rows.ctypes.data_as(pd), K, N, L, lo, hi, piece, out.ctypes.data_as(pd),
                                  mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if want_mask else None)
    assert pieces == -(-K // piece)
    return out, mask


def power_rows(seed, K, L, N):
    """(K, 3, N) rows from float64 frame powers (exponential: the power of Gaussian noise), bins of different levels,
    a few bins with an intermittent carrier, and S1 = S2 = 0 in some (row, bin) pairs."""
    rng = np.random.default_rng(seed)
    level = 10.0 ** rng.uniform(2, 7, size=N)
    p = rng.exponential(size=(K, L, N)) * level
    hot = rng.choice(N, size=max(N // 16, 1), replace=False)
    p[:, ::5, :][:, :, hot] *= 30.0                                     # every fifth frame: SK well above 1
    rows = np.stack([p.sum(axis=1), (p * p).sum(axis=1), p.max(axis=1)], axis=1)
    zk, zb = rng.integers(0, K, size=5), rng.integers(0, N, size=5)
    rows[zk, :, zb] = 0.0
    return rows, list(zip(zk.tolist(), zb.tolist()))


def test_emulated_sk_is_stats_spectral_kurtosis_bit_for_bit(emul):
    rng = np.random.default_rng(1)
    pd = ctypes.POINTER(ctypes.c_double)
    for L in (2, 3, 16, 64, 1000):
        p = rng.exponential(size=(L, 4000)) * 10.0 ** rng.uniform(0, 9, size=4000)
        s1, s2 = np.ascontiguousarray(p.sum(axis=0)), np.ascontiguousarray((p * p).sum(axis=0))
        s1[::97] = 0.0
        s2[::97] = 0.0
        got = np.empty_like(s1)
        emul.rpf_emul_excise_sk(s1.ctypes.data_as(pd), s2.ctypes.data_as(pd), L, got.ctypes.data_as(pd), s1.size)
        want = stats.spectral_kurtosis(s1, s2, L)
        assert np.all(np.isnan(got[::97])) and np.array_equal(got, want, equal_nan=True), L


# (N, K, L): K below, at and above the row groups of N; N = 500 is no multiple of the kernels' 64-bin tile
EMUL_CASES = [(64, 600, 2), (500, 1100, 16), (8192, 70, 3), (4096, 64, 64), (512, 1, 5)]


@pytest.mark.parametrize("N,K,L", EMUL_CASES)
def test_emulator_against_stats_excise(emul, N, K, L):
    G = emul.rpf_emul_excise_groups(N)
    assert G == max(1, (1 << 18) // N)
    rows, zeros = power_rows(N + K, K, L, N)
    sk = stats.spectral_kurtosis(rows[:, 0], rows[:, 1], L)
    finite = np.sort(sk[np.isfinite(sk)])
    # thresholds placed EXACTLY on two values of the sample: both are kept (the comparison is inclusive), their
    # neighbours outside are not
    on_lo, on_hi = float(finite[finite.size // 10]), float(finite[(9 * finite.size) // 10])
    cases = [(on_lo, on_hi), stats.sk_limits(L), (-INF, INF), (INF, INF), (on_hi, on_hi)]
    for lo, hi in cases:
        want, want_mask = stats.excise(rows, L, lo, hi)
        got, mask = emulate(emul, rows, L, lo, hi, K)
        flagged = int(want_mask.sum())
        # (a bin with nothing kept has clean = 0 on both sides: the bin's total is the scale)
        err = max(err_over_total(got[0], want[0], want[2]), err_over_total(got[2], want[2], want[2]))
        print("N=%d K=%d L=%d G=%d thresholds (%g, %g): %d of %d flagged, clean/total vs numpy %.3g (bar %g)"
              % (N, K, L, G, lo, hi, flagged, K * N, err, ADDITIVITY))
        assert np.array_equal(mask, want_mask) and np.array_equal(got[1], want[1])
        for k, b in zeros:
            assert mask[k, b] == 1                                      # S1 = 0: flagged, also with (-inf, +inf)
        assert err < ADDITIVITY
        # bitwise: the same rows cut into pieces of 1, 7 and all rows
        for piece in (1, 7):
            again, again_mask = emulate(emul, rows, L, lo, hi, piece)
            assert again.tobytes() == got.tobytes() and np.array_equal(again_mask, mask), (piece, lo, hi)
        no_mask, none = emulate(emul, rows, L, lo, hi, 7, want_mask=False)
        assert none is None and no_mask.tobytes() == got.tobytes()
        if (lo, hi) == (on_lo, on_hi):
            assert np.count_nonzero(sk == on_lo) >= 1 and np.all(mask[sk == on_lo] == 0) and np.all(mask[sk == on_hi] == 0)
            assert 0.15 < flagged / (K * N) < 0.25 or K * N < 1000
        if (lo, hi) == (on_hi, on_hi):
            assert got[1].sum() == np.count_nonzero(sk == on_hi) >= 1   # only the values ON the threshold are kept
        if (lo, hi) == (-INF, INF):
            assert flagged == len(set(zeros)) and got[0].tobytes() == got[2].tobytes()   # clean == total bit for bit
            assert np.array_equal(got[1], K - want_mask.sum(axis=0))
        if (lo, hi) == (INF, INF):
            assert flagged == K * N and not got[0].any() and not got[1].any()
            assert got[0].tobytes() == np.zeros(N).tobytes()            # +0.0, not -0.0


def test_emulator_with_no_rows_writes_zeros(emul):
    out, mask = emulate(emul, np.zeros((0, 3, 64)), 4, 0.5, 1.5, 3)
    assert not out.any() and mask.shape == (0, 64)


# ---- CLI ------------------------------------------------------------------------------------------------------------
def run_cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True)


def test_cli_excise_option_conflicts():
    r = run_cli("--help")
    assert r.returncode == 0 and "--excise <frames>" in r.stdout and "--excise-sigma <sigma>" in r.stdout
    base = ["--excise", "16", "--input", "/dev/null"]
    conflicts = [
        (["--excise", "16"], "--input"),
        (base + ["--series", "16"], "--series:"),
        (base + ["--series-stats", "16"], "--series-stats:"),
        (base + ["-m", "/tmp/rpf_excise_m"], "-m"),
        (base + ["-n", "16"], "--repeats (-n)"),
        (base + ["-t", "1"], "--time (-t)"),
        (base + ["-c"], "--continue (-c)"),
        (base + ["-e", "10"], "--elapsed (-e)"),
        (base + ["-f", "100M:110M"], "frequency range in -f"),
        (base + ["--gpus", "0,1"], "--gpus"),
        (["--excise", "1", "--input", "/dev/null"], "at least 2"),
        (["--excise", "-3", "--input", "/dev/null"], "at least 2"),
        (base + ["--excise-sigma", "-1"], "--excise-sigma"),
    ]
    for args, word in conflicts:
        r = run_cli(*args)
        assert r.returncode == 3, (args, r.returncode, r.stderr)
        assert "--excise" in r.stderr and word in r.stderr, (args, r.stderr)
    r = run_cli("--excise-sigma", "2", "--input", "/dev/null")
    assert r.returncode == 3 and "--excise-sigma" in r.stderr and "needs --excise" in r.stderr
    r = run_cli("--excise", "many", "--input", "/dev/null")
    assert r.returncode == 4            # not a number: the parser's own error, as for every numeric option
    # what applies: -w, --format, --frame-overlap, -l and a baseline parse beside it (the run then fails for want of a
    # device or of input, not of arguments)
    r = run_cli(*(base + ["--excise-sigma", "2.5", "--format", "cs16", "--frame-overlap", "50", "-l", "-q"]))
    assert r.returncode not in (3, 4), r.stderr


def test_cli_excised_block_writer():
    """write_spectrum_text_excised: clean / (kept L) where something was kept, total / (K L) where nothing was, the DC
    bin the mean of its neighbours, the usual / N / rate and dB; third column kept / K."""
    host = host_lib()
    fn = host.rpf_host_format_text_excised
    fn.restype = ctypes.c_long
    pd = ctypes.POINTER(ctypes.c_double)
    fn.argtypes = [pd, pd, pd, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int,
                   ctypes.c_int, pd, ctypes.c_char_p, ctypes.c_size_t]
    N, K, L, rate, freq = 8, 10, 4, 2000000, 100000000
    rng = np.random.default_rng(2)
    kept = np.array([10, 9, 0, 10, 3, 10, 1, 10], dtype=np.float64)
    total = rng.uniform(1e6, 2e6, size=N) * K * L
    clean = total * kept / K * rng.uniform(0.8, 1.0, size=N)
    for linear in (0, 1):
        buf = ctypes.create_string_buffer(1 << 14)
        n = fn(clean.ctypes.data_as(pd), kept.ctypes.data_as(pd), total.ctypes.data_as(pd), N, K, L, freq, rate, linear, None,
               buf, 1 << 14)
        assert n > 0
        lines = [ln.split() for ln in buf.value.decode().splitlines() if ln.strip()]
        assert len(lines) == N and all(len(ln) == 3 for ln in lines)
        mean = np.where(kept > 0, clean / np.where(kept > 0, kept * L, 1.0), total / (K * L))
        mean[N // 2] = (mean[N // 2 - 1] + mean[N // 2 + 1]) / 2
        want = mean / N / rate
        if not linear:
            want = 10 * np.log10(want)
        for i, ln in enumerate(lines):
            assert abs(float(ln[1]) - want[i]) <= 1e-5 * abs(want[i])            # six significant digits printed
            assert abs(float(ln[2]) - kept[i] / K) <= 1e-6
    hdr = host.rpf_host_format_header                                   # the existing headers did not change
    hdr.restype = ctypes.c_long
    hdr.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    buf = ctypes.create_string_buffer(1024)
    assert hdr(b"a", b"b", 0, buf, 1024) > 0 and b"kept fraction" not in buf.value
