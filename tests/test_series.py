"""Spectrogram mode (consecutive L-frame spectra of one stream per launch), the parts that need no GPU: the C-ABI
additions, the partition arithmetic of csrc/series_partition.h by brute force, the partition walked with float64
stand-ins for the frames' powers, and the CLI option."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib
from helpers import ROOT

HEADER = os.path.join(ROOT, "include", "rpf_engine.h")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
NEW = ("rpf_accumulate_device_series", "rpf_accumulate_series", "rpf_series_launches")


# ---- interface agreement ------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_series_entries(tmp_path):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"\s+", " ", text)
    assert ("int rpf_accumulate_device_series(rpf_engine* e, const void* d_stream, size_t nbytes, "
            "int64_t frames_per_spectrum, int64_t max_spectra, double* d_out , void* hip_stream, "
            "int64_t* spectra_done);") in text
    assert ("int rpf_accumulate_series(rpf_engine* e, const uint8_t* stream, size_t nbytes, int64_t frames_per_spectrum, "
            "int64_t max_spectra, double* out , int64_t* spectra_done);") in text
    assert "int rpf_series_launches(const rpf_engine* e);" in text
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True,
                              check=True).stdout
    sym = {s[0]: s for s in _lib._SYMBOLS}
    for name in NEW:
        assert name in _lib.symbol_names()
        assert re.search(r"\bT %s$" % name, exported, re.M), name
    P, i64 = ctypes.c_void_p, ctypes.c_int64
    assert sym["rpf_accumulate_device_series"][1:] == (
        ctypes.c_int, [P, P, ctypes.c_size_t, i64, i64, P, P, ctypes.POINTER(i64)])
    assert sym["rpf_accumulate_series"][1:] == (
        ctypes.c_int, [P, P, ctypes.c_size_t, i64, i64, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(i64)])
    assert sym["rpf_series_launches"][1:] == (ctypes.c_int, [P])
    # the ABI version did not move: the entries are additive within 2
    src = tmp_path / "v.c"
    src.write_text('#include <stdio.h>\n#include "rpf_engine.h"\nint main(void) { printf("%d\\n", RPF_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "v"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    assert int(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout) == 2
    lib = rpf.load()
    assert lib.rpf_abi_version() == 2
    assert lib.rpf_series_launches(None) == 0
    # NULL engine: invalid argument, nothing dereferenced
    assert lib.rpf_accumulate_device_series(None, None, 0, 1, 1, None, None, None) == rpf.ReturnValue.InvalidArgument
    assert lib.rpf_accumulate_series(None, None, 0, 1, 1, None, None) == rpf.ReturnValue.InvalidArgument
    for method in ("accumulate_device_series", "accumulate_series", "series_launches"):
        assert callable(getattr(rpf.Datastore, method))


# ---- partition arithmetic -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "librpf_emul_series.so"))
    ll, i, pi, pll = ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)
    pd = ctypes.POINTER(ctypes.c_double)
    lib.rpf_emul_series_partition.argtypes = [ll, ll, i, i, pll]
    lib.rpf_emul_series_max_spectra.argtypes = [ll, i]
    lib.rpf_emul_series_max_spectra.restype = ll
    lib.rpf_emul_series_div.argtypes = [i, pi, i, pi]
    lib.rpf_emul_series_div.restype = None
    lib.rpf_emul_series_ranges.argtypes = [ll, ll, i, i, pi]
    lib.rpf_emul_series_complete.argtypes = [ll, ll, i, i, i, i]
    lib.rpf_emul_series_slot.argtypes = [ll, ll, i, i, i, i]
    lib.rpf_emul_series_spectrum_wgs.argtypes = [ll, ll, i, i, i, pi, pi]
    lib.rpf_emul_series_spectrum_wgs.restype = None
    lib.rpf_emul_series_walk.argtypes = [ll, ll, i, i, pd, pd, pi, pi]
    return lib


def partition(emul, K, L, fpw, max_grid):
    out = (ctypes.c_longlong * 8)()
    grid = emul.rpf_emul_series_partition(K, L, fpw, max_grid, out)
    return grid, dict(zip(("K", "L", "ips", "total", "q", "r", "shift", "magic"), list(out)))


def cases():
    """(frames, L, fpw, max_grid): the edges the kernel can meet, then a few thousand random ones."""
    edge = [
        (700, 1, 2, 256), (700, 1, 1, 8), (5, 1, 4, 256),            # L = 1
        (200, 3, 4, 16), (200, 5, 4, 16), (200, 4, 4, 16),           # L = fpw - 1, fpw + 1, fpw
        (10, 11, 2, 8), (0, 3, 2, 8), (2, 3, 2, 8),                  # L > all frames: K = 0
        (12, 4, 2, 256),                                             # K ips = 6 < grid
        (16, 4, 2, 8),                                               # K ips = 8 = grid
        (26, 4, 2, 8),                                               # q = 1 with r > 0 (K ips = 12)
        (1040, 80, 2, 256), (523, 7, 2, 5), (97, 97, 4, 16), (1000, 999, 4, 7),
        (41, 13, 2, 3),                                              # a dropped tail of L - 1 ... frames
    ]
    rng = random.Random(20260117)
    rand = []
    for _ in range(3000):
        fpw = rng.choice([1, 2, 4, 8])
        L = rng.choice([1, fpw, fpw + 1, max(1, fpw - 1), rng.randint(1, 40), rng.randint(1, 400)])
        frames = rng.choice([rng.randint(0, 60), rng.randint(0, 3000)])
        rand.append((frames, L, fpw, rng.choice([1, 2, 3, 7, 16, 64, 256, 1024])))
    return edge + rand


def test_partition_assigns_every_frame_once_and_the_closed_forms_hold(emul):
    checked = 0
    for frames, L, fpw, max_grid in cases():
        K = frames // L
        grid, a = partition(emul, K, L, fpw, max_grid)
        ips = -(-L // fpw)
        assert a["ips"] == ips and a["total"] == K * ips and a["K"] == K
        assert grid == min(K * ips, max_grid)
        if K == 0:
            assert grid == 0
            continue
        assert a["q"] * grid + a["r"] == a["total"] and a["q"] >= 1
        ranges = (ctypes.c_int * (4 * grid))()
        assert emul.rpf_emul_series_ranges(K, L, fpw, max_grid, ranges) == grid
        owner = np.zeros(frames, dtype=np.int64)          # how many (workgroup, spectrum) pairs hold frame f
        wgs_of = {}                                       # spectrum -> workgroups, enumerated
        slots = set()
        at = 0
        for w in range(grid):
            lo, hi, first, last = ranges[4 * w:4 * w + 4]
            assert lo == at and hi > lo                   # contiguous, never empty
            at = hi
            assert (first, last) == (lo // ips, (hi - 1) // ips)
            for k in range(first, last + 1):
                wgs_of.setdefault(k, []).append(w)
                seg_lo, seg_hi = max(lo, k * ips), min(hi, (k + 1) * ips)
                for it in range(seg_lo, seg_hi):          # the frame slots of iteration `it` that are active
                    f0 = k * L + (it - k * ips) * fpw
                    owner[f0:min(f0 + fpw, (k + 1) * L)] += 1
                complete = emul.rpf_emul_series_complete(K, L, fpw, max_grid, w, k) == 1
                assert complete == (lo <= k * ips and (k + 1) * ips <= hi)
                slot = emul.rpf_emul_series_slot(K, L, fpw, max_grid, w, k)
                if complete:
                    assert slot == -1
                else:
                    assert 0 <= slot < 2 * grid and slot not in slots
                    assert slot == (2 * w if k * ips < lo else 2 * w + 1)
                    slots.add(slot)
            # a workgroup has at most two incomplete segments
            assert sum(1 for k in range(first, last + 1)
                       if emul.rpf_emul_series_slot(K, L, fpw, max_grid, w, k) >= 0) <= 2
        assert at == a["total"]
        assert np.all(owner[:K * L] == 1) and np.all(owner[K * L:] == 0)
        wa, wb = ctypes.c_int(), ctypes.c_int()
        for k in (range(K) if K <= 64 else list(range(8)) + random.Random(K).sample(range(K), 24) + [K - 1]):
            emul.rpf_emul_series_spectrum_wgs(K, L, fpw, max_grid, k, ctypes.byref(wa), ctypes.byref(wb))
            assert list(range(wa.value, wb.value + 1)) == wgs_of[k], (frames, L, fpw, max_grid, k)
            assert (len(wgs_of[k]) == 1) == (emul.rpf_emul_series_complete(K, L, fpw, max_grid, wgs_of[k][0], k) == 1)
        checked += 1
    assert checked > 2000


def test_division_free_hop_of_is_exact_to_two_to_the_31(emul):
    top = 2 ** 31 - 1
    rng = random.Random(7)
    divisors = list(range(1, 70)) + [127, 128, 129, 255, 256, 257, 1000, 4095, 4096, 4097, 65535, 65536, 65537,
                                     2 ** 20 - 1, 2 ** 20 + 1, 2 ** 30 - 1, 2 ** 30, 2 ** 30 + 1, top - 1, top]
    divisors += [rng.randint(2, top) for _ in range(200)]
    for d in divisors:
        its = {0, 1, d - 1, d, d + 1, top, top - 1, top - d, (top // d) * d, (top // d) * d - 1}
        for _ in range(40):
            m = rng.randint(0, top // d)
            its.update((m * d - 1, m * d, m * d + 1, m * d + d - 1))
        its = np.array(sorted(i for i in its if 0 <= i <= top), dtype=np.int32)
        out = np.zeros(its.size, dtype=np.int32)
        emul.rpf_emul_series_div(d, its.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), its.size,
                                 out.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        assert np.array_equal(out.astype(np.int64), its.astype(np.int64) // d), d


def test_launch_limit(emul):
    out = (ctypes.c_longlong * 8)()
    for L, fpw in ((1, 2), (3, 2), (1000, 4)):
        most = emul.rpf_emul_series_max_spectra(L, fpw)
        ips = -(-L // fpw)
        assert most * ips <= 2 ** 31 - 1 < (most + 1) * ips
        assert emul.rpf_emul_series_partition(most, L, fpw, 1024, out) == 1024
        assert emul.rpf_emul_series_partition(most + 1, L, fpw, 1024, out) == -1
    assert emul.rpf_emul_series_partition(5, 0, 2, 8, out) == -1
    assert emul.rpf_emul_series_partition(-1, 1, 2, 8, out) == -1


# ---- the kernel's walk, emulated -----------------------------------------------------------------------------------
def test_emulated_walk_reproduces_the_per_spectrum_sums(emul):
    rng = np.random.default_rng(5)
    pd, pi = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    for frames, L, fpw, max_grid in cases()[:17] + cases()[17::10]:
        K = frames // L
        if K == 0:
            continue
        # integers: every order of the additions gives the same double
        power = rng.integers(1, 1 << 20, size=frames).astype(np.float64)
        rows = np.full(K + 2, -1.0)
        owner = np.zeros(frames, dtype=np.int32)
        grid = min(K * -(-L // fpw), max_grid)
        writes = np.zeros(2 * grid, dtype=np.int32)
        assert emul.rpf_emul_series_walk(K, L, fpw, max_grid, power.ctypes.data_as(pd), rows.ctypes.data_as(pd),
                                         owner.ctypes.data_as(pi), writes.ctypes.data_as(pi)) == grid
        want = power[:K * L].reshape(K, L).sum(axis=1)
        assert np.array_equal(rows[:K], want), (frames, L, fpw, max_grid)
        assert np.all(rows[K:] == -1.0)
        assert np.all(owner[:K * L] == 1) and np.all(owner[K * L:] == 0)
        assert writes.max(initial=0) <= 1


# ---- CLI -----------------------------------------------------------------------------------------------------------
def run_cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True)


def test_cli_series_option_conflicts():
    r = run_cli("--help")
    assert r.returncode == 0 and "--series <frames>" in r.stdout
    conflicts = [
        (["--series", "16"], "--input"),
        (["--series", "16", "--input", "/dev/null", "-f", "100M:110M"], "frequency range"),
        (["--series", "16", "--input", "/dev/null", "-n", "16"], "--repeats"),
        (["--series", "16", "--input", "/dev/null", "-t", "1"], "--time"),
        (["--series", "16", "--input", "/dev/null", "-c"], "--continue"),
        (["--series", "16", "--input", "/dev/null", "-e", "10"], "--elapsed"),
        (["--series", "16", "--input", "/dev/null", "-m", "/tmp/rpf_series_m"], "-m"),
        (["--series", "16", "--input", "/dev/null", "--stats"], "--stats"),
        (["--series", "16", "--input", "/dev/null", "--gpus", "0,1"], "--gpus"),
        (["--series", "0", "--input", "/dev/null"], "at least 1"),
        (["--series", "-3", "--input", "/dev/null"], "at least 1"),
    ]
    for args, word in conflicts:
        r = run_cli(*args)
        assert r.returncode == 3, (args, r.returncode, r.stderr)
        assert "--series" in r.stderr and word in r.stderr, (args, r.stderr)
    r = run_cli("--series", "many", "--input", "/dev/null")
    assert r.returncode == 4            # not a number: the parser's own error, as for every numeric option
