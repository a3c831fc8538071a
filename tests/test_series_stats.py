"""Time-resolved per-bin statistics (a series of S1, S2, PK per launch), the parts that need no GPU: the C-ABI additions,
the series partition walked with three planes and float64 stand-ins for the frames' powers, and the CLI option."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib
from helpers import ROOT
from test_series import cases

HEADER = os.path.join(ROOT, "include", "rpf_engine.h")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
NEW = ("rpf_accumulate_device_series_stats", "rpf_accumulate_series_stats")


# ---- interface agreement ------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_series_stats_entries(tmp_path):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"\s+", " ", text)
    assert ("int rpf_accumulate_device_series_stats(rpf_engine* e, const void* d_stream, size_t nbytes, "
            "int64_t frames_per_spectrum, int64_t max_spectra, double* d_out , void* hip_stream, "
            "int64_t* spectra_done);") in text
    assert ("int rpf_accumulate_series_stats(rpf_engine* e, const uint8_t* stream, size_t nbytes, "
            "int64_t frames_per_spectrum, int64_t max_spectra, double* out , int64_t* spectra_done);") in text
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True,
                              check=True).stdout
    sym = {s[0]: s for s in _lib._SYMBOLS}
    for name in NEW:
        assert name in _lib.symbol_names()
        assert re.search(r"\bT %s$" % name, exported, re.M), name
    P, i64 = ctypes.c_void_p, ctypes.c_int64
    assert sym["rpf_accumulate_device_series_stats"][1:] == (
        ctypes.c_int, [P, P, ctypes.c_size_t, i64, i64, P, P, ctypes.POINTER(i64)])
    assert sym["rpf_accumulate_series_stats"][1:] == (
        ctypes.c_int, [P, P, ctypes.c_size_t, i64, i64, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(i64)])
    # the ABI version did not move: the entries are additive within 2
    src = tmp_path / "v.c"
    src.write_text('#include <stdio.h>\n#include "rpf_engine.h"\nint main(void) { printf("%d\\n", RPF_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "v"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    assert int(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout) == 2
    lib = rpf.load()
    assert lib.rpf_abi_version() == 2
    # NULL engine: invalid argument, nothing dereferenced
    assert lib.rpf_accumulate_device_series_stats(None, None, 0, 1, 1, None, None, None) == rpf.ReturnValue.InvalidArgument
    assert lib.rpf_accumulate_series_stats(None, None, 0, 1, 1, None, None) == rpf.ReturnValue.InvalidArgument
    for method in ("accumulate_device_series_stats", "accumulate_series_stats"):
        assert callable(getattr(rpf.Datastore, method))
    host = ctypes.CDLL(os.path.join(ROOT, "rtl-power-fftw_amd", "host", "librpf_host.so"))
    assert host.rpf_host_accumulate_series_stats


def test_spectral_kurtosis_per_row():
    # stats.spectral_kurtosis over (K, N) planes with M = L is the estimator of every row
    rng = np.random.default_rng(3)
    p = rng.exponential(size=(5, 64, 8))                     # K, L, N
    s1, s2 = p.sum(axis=1), (p * p).sum(axis=1)
    sk = rpf.stats.spectral_kurtosis(s1, s2, 64)
    assert sk.shape == (5, 8)
    for k in range(5):
        assert np.array_equal(sk[k], rpf.stats.spectral_kurtosis(s1[k], s2[k], 64))
    assert np.all(np.isnan(rpf.stats.spectral_kurtosis(s1, s2, 1)))


# ---- the kernel's walk with three planes, emulated ----------------------------------------------------------------
@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "librpf_emul_series_stats.so"))
    ll, i, pi, pd = ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    lib.rpf_emul_series_stats_walk.argtypes = [ll, ll, i, i, pd, pd, pi, pi, pi]
    return lib


def walk(emul, power, L, fpw, max_grid):
    """-> rows (K + 2, 3) pre-filled with -1, and the checks that hold for every case."""
    pd, pi = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    frames = power.size
    K = frames // L
    grid = min(K * -(-L // fpw), max_grid)
    rows = np.full((K + 2, 3), -1.0)
    owner = np.zeros(frames, dtype=np.int32)
    row_writes = np.zeros((K + 2, 3), dtype=np.int32)
    slot_writes = np.zeros((2 * grid, 3), dtype=np.int32)
    assert emul.rpf_emul_series_stats_walk(K, L, fpw, max_grid, power.ctypes.data_as(pd), rows.ctypes.data_as(pd),
                                           owner.ctypes.data_as(pi), row_writes.ctypes.data_as(pi),
                                           slot_writes.ctypes.data_as(pi)) == grid
    assert np.all(rows[K:] == -1.0)                                   # rows >= K untouched
    assert np.all(owner[:K * L] == 1) and np.all(owner[K * L:] == 0)
    assert np.all(row_writes[:K] == 1) and np.all(row_writes[K:] == 0)
    assert slot_writes.max(initial=0) <= 1
    # a slot is written in all three planes or in none
    assert np.all(slot_writes == slot_writes[:, :1])
    return rows


def want_of(power, L):
    K = power.size // L
    g = power[:K * L].reshape(K, L)
    return np.stack([g.sum(axis=1), (g * g).sum(axis=1), g.max(axis=1)], axis=1)


def test_emulated_walk_reproduces_sum_sum_of_squares_and_maximum(emul):
    rng = np.random.default_rng(11)
    checked = 0
    for frames, L, fpw, max_grid in cases()[:17] + cases()[17::10]:
        K = frames // L
        if K == 0:
            continue
        # integers below 2^20: sums of up to 3000 squares stay below 2^52, every order of the additions gives the same double
        power = rng.integers(1, 1 << 20, size=frames).astype(np.float64)
        rows = walk(emul, power, L, fpw, max_grid)
        assert np.array_equal(rows[:K], want_of(power, L)), (frames, L, fpw, max_grid)
        checked += 1
    assert checked > 250


@pytest.mark.parametrize("L,fpw,max_grid,K", [(999, 4, 7, 1), (600, 2, 16, 3), (257, 1, 64, 2), (80, 2, 256, 13)])
def test_the_peak_survives_the_fix_up_from_any_segment(emul, L, fpw, max_grid, K):
    """Spectra that span many workgroups: the largest frame in the first, a middle and the last segment."""
    rng = np.random.default_rng(L)
    ips = -(-L // fpw)
    grid = min(K * ips, max_grid)
    q, r = divmod(K * ips, grid)
    bounds = [w * q + min(w, r) for w in range(grid + 1)]            # hop_range: the first r ranges have q + 1
    spans = 0
    for where in ("first", "middle", "last"):
        power = rng.integers(1, 1 << 19, size=K * L + L - 1).astype(np.float64)      # (a tail of L - 1 frames is dropped)
        for k in range(K):
            # the segments of spectrum k: its iterations cut at the workgroup bounds
            cuts = [k * ips] + [b for b in bounds if k * ips < b < (k + 1) * ips] + [(k + 1) * ips]
            segs = list(zip(cuts[:-1], cuts[1:]))
            spans = max(spans, len(segs))
            lo, hi = {"first": segs[0], "middle": segs[len(segs) // 2], "last": segs[-1]}[where]
            f = k * L + min((lo - k * ips) * fpw if where != "last" else (hi - 1 - k * ips) * fpw, L - 1)
            power[f] = float((1 << 20) - 1 - k)
        power[K * L:] = float((1 << 20) - 1)                          # larger than every peak, and in no spectrum
        rows = walk(emul, power, L, fpw, max_grid)
        want = want_of(power, L)
        assert np.array_equal(rows[:K], want), (where, L, fpw, max_grid)
        assert np.array_equal(rows[:K, 2], [(1 << 20) - 1 - k for k in range(K)])
    assert spans >= 3            # the fix-up's maximum ran over more than two segments


# ---- CLI -----------------------------------------------------------------------------------------------------------
def run_cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True)


def test_cli_series_stats_option_conflicts():
    r = run_cli("--help")
    assert r.returncode == 0 and "--series-stats <frames>" in r.stdout
    base = ["--series-stats", "16", "--input", "/dev/null"]
    conflicts = [
        (["--series-stats", "16"], "--input"),
        (base + ["--series", "16"], "with --series:"),
        (base + ["-f", "100M:110M"], "frequency range"),
        (base + ["-n", "16"], "--repeats"),
        (base + ["-t", "1"], "--time"),
        (base + ["-c"], "--continue"),
        (base + ["-e", "10"], "--elapsed"),
        (base + ["-m", "/tmp/rpf_series_stats_m"], "-m"),
        (base + ["--gpus", "0,1"], "--gpus"),
        (["--series-stats", "0", "--input", "/dev/null"], "at least 1"),
        (["--series-stats", "-3", "--input", "/dev/null"], "at least 1"),
    ]
    for args, word in conflicts:
        r = run_cli(*args)
        assert r.returncode == 3, (args, r.returncode, r.stderr)
        assert "--series-stats" in r.stderr and word in r.stderr, (args, r.stderr)
    # the plain series beside --stats stays refused
    r = run_cli("--series", "16", "--input", "/dev/null", "--stats")
    assert r.returncode == 3 and "--series" in r.stderr and "--stats" in r.stderr
    r = run_cli("--series-stats", "many", "--input", "/dev/null")
    assert r.returncode == 4            # not a number: the parser's own error, as for every numeric option
