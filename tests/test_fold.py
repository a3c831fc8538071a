"""Fold of a plane at trial periods, everything that needs no GPU: the two C-ABI additions, fold.reference against a plain
Python loop, the walk of the kernel's waves on the host emulator (tests/emul/fold_emul.cpp over csrc/fold_core.h) against
fold.reference, period_steps and chi2 in C++ and in Python, the LDS index under tools/lds_bank_model.py's rules, the CLI
options and what they refuse, the two block writers, and the detection case on a float64 model of the engine's rows.
tests/test_gpu_fold.py imports the helpers."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, dedisperse, fold
from helpers import ROOT, dp

HEADER = os.path.join(ROOT, "include", "rpf_engine.h")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
ll = ctypes.c_longlong
vp = ctypes.c_void_p
u64p = ctypes.POINTER(ctypes.c_uint64)
i32p = ctypes.POINTER(ctypes.c_int32)
_emul = None
_host = None

TIMES = (1, 15, 16, 17, 1000, 4099)
BINS = (1, 2, 7, 64, 128)


# ---- helpers (shared with tests/test_gpu_fold.py) -------------------------------------------------------------------------

def emul():
    global _emul
    if _emul is None:
        lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "librpf_emul_fold.so"))
        lib.rpf_emul_fold.restype = ll
        lib.rpf_emul_fold.argtypes = [vp, ctypes.c_int, ll, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
        for name in ("max_cells", "scratch_cap", "lds_bytes", "segment_begin", "scratch_bytes"):
            getattr(lib, "rpf_emul_fold_" + name).restype = ll
        lib.rpf_emul_fold_lds_bytes.argtypes = [ctypes.c_int]
        lib.rpf_emul_fold_segment_begin.argtypes = [ll, ctypes.c_int]
        lib.rpf_emul_fold_scratch_bytes.argtypes = [ctypes.c_int] * 3
        lib.rpf_emul_fold_group_series.argtypes = [ctypes.c_int] * 3
        lib.rpf_emul_fold_lds_index.argtypes = [ctypes.c_int, ctypes.c_int]
        lib.rpf_emul_fold_bin.restype = ctypes.c_uint
        lib.rpf_emul_fold_bin.argtypes = [ctypes.c_ulonglong, ll, ctypes.c_uint]
        _emul = lib
    return _emul


def host_lib():
    global _host
    if _host is None:
        lib = ctypes.CDLL(os.path.join(ROOT, "rtl-power-fftw_amd", "host", "librpf_host.so"))
        lib.rpf_host_parse_fold.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), dp, ctypes.c_int, ctypes.POINTER(ll),
                                            ctypes.c_char_p, ctypes.c_size_t]
        lib.rpf_host_period_steps.argtypes = [dp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ll, ll, vp,
                                              ctypes.c_char_p, ctypes.c_size_t]
        lib.rpf_host_fold_chi2.restype = None
        lib.rpf_host_fold_chi2.argtypes = [dp, i32p, dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ll, dp]
        lib.rpf_host_format_text_fold.restype = ctypes.c_long
        lib.rpf_host_format_text_fold.argtypes = [dp, ctypes.c_int, dp, ctypes.c_int, ctypes.c_int, ll, dp, ctypes.c_int, ctypes.c_int,
                                                  dp, i32p, ll, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
        _host = lib
    return _host


def same_bits(x, y):
    """Equal as doubles, NaN where the other is NaN."""
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and np.array_equal(x, y, equal_nan=True)


def make_steps(rng, P):
    """P steps: the corner values, period_steps values and random ones, in that order (P = 1: a random one)."""
    fixed = [0, 1, 1 << 63, (1 << 64) - 1] + [int(v) for v in fold.row_period_steps([50.3, 2.0, 40.3])] + \
            [int(v) for v in fold.period_steps([0.004256], 2.4e6, 64, 4)]
    rand = [int(rng.integers(0, 1 << 62)) * 4 + int(rng.integers(0, 4)) for _ in range(P)]
    return np.array((fixed + rand)[:P] if P > 1 else rand[:1], dtype=np.uint64)


def make_series(rng, D, T):
    """Doubles of mixed sign over seven decades: a sum in another order would differ."""
    return rng.standard_normal((D, T)) * 10.0 ** rng.integers(-3, 4, (D, T))


def loop_reference(x, step, NB):
    """The definition as a plain Python loop, one series and one step: (prof, hits, mom)."""
    T = len(x)
    G = -(-T // 16)
    parts = [[0.0] * NB for _ in range(16)]
    m = [[0.0, 0.0] for _ in range(16)]
    hits = [0] * NB
    phase = 0
    for t in range(T):
        b = ((phase >> 32) * NB) >> 32
        assert b == (((t * step) % (1 << 64)) >> 32) * NB >> 32
        v = float(x[t])
        parts[t // G][b] += v
        m[t // G][0] += v
        m[t // G][1] += v * v
        hits[b] += 1
        phase = (phase + step) & ((1 << 64) - 1)
    prof, mom = [0.0] * NB, [0.0, 0.0]
    for g in range(16):
        for b in range(NB):
            prof[b] = prof[b] + parts[g][b]
        mom = [mom[0] + m[g][0], mom[1] + m[g][1]]
    return np.array(prof), np.array(hits, dtype=np.int32), np.array(mom)


def emul_fold(x, steps, NB, per_group=0):
    """The emulator's walk: (prof, hits, mom, disorder, groups)."""
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
    steps = np.ascontiguousarray(steps, dtype=np.uint64)
    D, T = x.shape
    P = steps.size
    prof, hits, mom = np.full((D, P, NB), -7.0), np.full((P, NB), -7, dtype=np.int32), np.full((D, 2), -7.0)
    bad = ll(-1)
    groups = emul().rpf_emul_fold(x.ctypes.data, D, T, steps.ctypes.data, P, NB, per_group, prof.ctypes.data, hits.ctypes.data,
                                  mom.ctypes.data, ctypes.byref(bad))
    return prof, hits, mom, bad.value, groups


def cpp_period_steps(periods, rate, N, L, S, in_rows=False):
    periods = np.ascontiguousarray(periods, dtype=np.float64)
    out = np.zeros(periods.size, dtype=np.uint64)
    msg = ctypes.create_string_buffer(512)
    rc = host_lib().rpf_host_period_steps(periods.ctypes.data_as(dp), periods.size, int(in_rows), rate, N, L, S, out.ctypes.data, msg, 512)
    return rc, out, msg.value.decode()


def cpp_chi2(prof, hits, mom, T):
    prof = np.ascontiguousarray(prof, dtype=np.float64)
    hits = np.ascontiguousarray(hits, dtype=np.int32)
    mom = np.ascontiguousarray(mom, dtype=np.float64)
    D, P, NB = prof.shape
    out = np.zeros((D, P))
    host_lib().rpf_host_fold_chi2(prof.ctypes.data_as(dp), hits.ctypes.data_as(i32p), mom.ctypes.data_as(dp), D, P, NB, T,
                                  out.ctypes.data_as(dp))
    return out


def c_six(v, digits=6):
    """A double as a C++ stream writes it at this precision."""
    if np.isnan(v):
        return "-nan" if np.signbit(v) else "nan"
    if np.isinf(v):
        return "-inf" if v < 0 else "inf"
    return "%.*g" % (digits, v)


def best_cell(chi2):
    """The strongest cell: the first of the largest values that are not NaN; None where all are."""
    flat = np.asarray(chi2).ravel()
    if np.all(np.isnan(flat)):
        return None
    return np.unravel_index(int(np.nanargmax(flat)), np.asarray(chi2).shape)


def python_blocks(dms, periods, NB, T, chi2, prof, hits, nb, linear):
    """The two --fold blocks as the issue defines them, without the '# Acquisition' lines and the blank ones."""
    lines = ["# rtl-power-fftw output", "# fold: %d DMs x %d periods, %d phase bins, %d times" % (len(dms), len(periods), NB, T), "#",
             "# DM [pc cm^-3] period [s] reduced chi2"]
    for d, dm in enumerate(dms):
        for p, period in enumerate(periods):
            lines.append("%s %s %s" % (c_six(dm), c_six(period, 9), c_six(chi2[d, p])))
    cell = best_cell(chi2)
    if cell is None:
        return lines
    d, p = cell
    lines += ["# rtl-power-fftw output",
              "# DM %s pc cm^-3, period %s s, reduced chi2 %s" % (c_six(dms[d]), c_six(periods[p], 9), c_six(chi2[d, p])), "#",
              "# phase [turns] power [median units] hits"]
    for b in range(NB):
        if hits[p, b] == 0:
            v = "nan"
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                x = prof[d, p, b] / (float(hits[p, b]) * float(nb))
                v = c_six(x if linear else 10 * np.log10(x))
        lines.append("%s %s %d" % (c_six((b + 0.5) / NB), v, hits[p, b]))
    return lines


def cpp_blocks(dms, periods, NB, T, chi2, prof, hits, nb, linear):
    """The same by the C++ host's writers, as all lines (the strongest cell chosen here)."""
    dms, periods = np.ascontiguousarray(dms, dtype=np.float64), np.ascontiguousarray(periods, dtype=np.float64)
    chi2 = np.ascontiguousarray(chi2, dtype=np.float64)
    d, p = best_cell(chi2)
    cell = np.ascontiguousarray(prof[d, p], dtype=np.float64)
    h = np.ascontiguousarray(hits[p], dtype=np.int32)
    buf = ctypes.create_string_buffer(2000 + 64 * (chi2.size + len(dms) + NB))
    n = host_lib().rpf_host_format_text_fold(dms.ctypes.data_as(dp), dms.size, periods.ctypes.data_as(dp), periods.size, NB, T,
                                             chi2.ctypes.data_as(dp), int(d), int(p), cell.ctypes.data_as(dp), h.ctypes.data_as(i32p),
                                             nb, int(linear), buf, len(buf))
    assert n > 0
    return buf.value.decode().split("\n")


def essential(lines):
    return [ln for ln in lines if ln.strip() and not ln.startswith("# Acquisition")]


def parse(*args):
    argv = [b"rpf_power"] + [a.encode() for a in args]
    arr = (ctypes.c_char_p * len(argv))(*argv)
    periods = np.full(5000, -1.0)
    nbins = ll(-1)
    msg = ctypes.create_string_buffer(1024)
    n = host_lib().rpf_host_parse_fold(len(argv), arr, periods.ctypes.data_as(dp), periods.size, ctypes.byref(nbins), msg, 1024)
    return n, periods[:max(n, 0)], nbins.value, msg.value.decode()


# The detection case of the issue: the stream of test_gpu_dedisperse.pulse_stream with a pulse in every period.
PULSAR = dict(N=64, L=4, K=2048, fc=408000000, rate=2400000, dm_index=5, period_rows=40.3, amp=2.0, NB=16)
PULSAR_DMS = np.arange(0.0, 31.0, 3.0)
PULSAR_PERIODS_ROWS = PULSAR["period_rows"] + np.arange(-4, 5) * 0.1


def pulsar_stream(seed):
    """cu8 Gaussian noise of sigma 20 per component and, for every bin but DC, a bin-centred tone of amplitude 2 with a
    random phase in the L frames of the rows floor(40.3 m + 5) + delays[DM 15][b], for every m that fits.  Returns the
    stream and the delay table of DM 0:30:3."""
    N, L, K = PULSAR["N"], PULSAR["L"], PULSAR["K"]
    rng = np.random.default_rng(seed)
    delays = dedisperse.dm_delays(PULSAR_DMS, PULSAR["fc"], PULSAR["rate"], N, L)
    own = delays[PULSAR["dm_index"]]
    z = 20.0 * (rng.standard_normal(N * L * K) + 1j * rng.standard_normal(N * L * K))
    z = z.reshape(K, L * N)
    n = np.arange(L * N)
    m = 0
    while True:
        at = int(math.floor(m * PULSAR["period_rows"] + 5.0))
        m += 1
        if at + own.max() >= K:
            break
        for b in range(N):
            if b != N // 2:
                z[at + own[b]] += PULSAR["amp"] * np.exp(1j * (2 * np.pi * (b - N // 2) * n / N + rng.uniform(0, 2 * np.pi)))
    z = z.reshape(-1)
    u = np.empty(2 * z.size, dtype=np.float64)
    u[0::2], u[1::2] = z.real, z.imag
    u = np.rint(u + 127.0)
    assert u.min() >= 0 and u.max() <= 255                                    # no sample saturates
    return u.astype(np.uint8), delays


def model_rows(stream, N, L):
    """A float64 model of the engine's rows: sum over the L frames of a row of |FFT|^2 of the cu8 values, bin N/2 = DC."""
    u = stream.astype(np.float64) - 127.0
    z = (u[0::2] + 1j * u[1::2]).reshape(-1, L, N) * ((-1.0) ** np.arange(N))
    return (np.abs(np.fft.fft(z, axis=2)) ** 2).sum(axis=1)


def pulsar_steps():
    return fold.row_period_steps(PULSAR_PERIODS_ROWS)


# ---- header, binding and library ----------------------------------------------------------------------------------------

def test_header_binding_and_library_agree_on_the_two_symbols():
    text = open(HEADER).read()
    assert re.search(r"\bint rpf_fold_device\(rpf_engine\* e, const double\* d_series[^;]*int n_series, int64_t T,\s*"
                     r"const uint64_t\* steps[^;]*int n_periods, int phase_bins,\s*double\* d_prof[^;]*int64_t capacity[^;]*"
                     r"int32_t\* d_hits[^;]*double\* d_mom[^;]*void\* hip_stream\);", text)
    assert re.search(r"\bint rpf_dedisperse_fold\(rpf_engine\* e, const int32_t\* delays, const double\* weights, int n_trials,\s*"
                     r"const uint64_t\* steps, int n_periods, int phase_bins,\s*double\* prof[^;]*int64_t capacity, "
                     r"int32_t\* hits[^;]*double\* mom[^;]*int64_t\* times\);", text)
    assert re.search(r"#define RPF_FOLD_SEGMENTS 16\b", text) and emul().rpf_emul_fold_segments() == 16 == fold.SEGMENTS
    m = re.search(r"#define RPF_ABI_VERSION 2(.*?)\*/", text, re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in ("rpf_fold_device", "rpf_dedisperse_fold"):
        assert m and re.search(r"\b%s\b" % name, m.group(1)), name
        assert name in _lib.symbol_names()
        assert re.search(r"\bT %s$" % name, exported, re.M), name
    lib = rpf.load()
    assert lib.rpf_abi_version() == 2
    prof, times = np.full(8, -3.0), ctypes.c_int64(-1)
    table, steps = np.zeros(8, dtype=np.int32), np.zeros(1, dtype=np.uint64)
    bad = rpf.ReturnValue.InvalidArgument
    assert lib.rpf_dedisperse_fold(None, table.ctypes.data_as(i32p), None, 1, steps.ctypes.data_as(u64p), 1, 4,
                                   prof.ctypes.data_as(dp), 8, None, None, ctypes.byref(times)) == bad
    assert lib.rpf_fold_device(None, None, 1, 8, steps.ctypes.data_as(u64p), 1, 4, None, 8, None, None, None) == bad
    assert np.all(prof == -3.0)
    for name in ("fold_device", "dedisperse_fold"):
        assert hasattr(rpf.Datastore, name)
    for name in ("period_steps", "row_period_steps", "phase_bins", "reference", "chi2"):
        assert callable(getattr(fold, name))


# ---- the reference, the plain loop and the emulator's walk agree bit for bit ----------------------------------------------

@pytest.mark.parametrize("NB", BINS)
@pytest.mark.parametrize("T", TIMES)
def test_reference_equals_a_plain_loop_bit_for_bit(T, NB):
    rng = np.random.default_rng([T, NB])
    steps = make_steps(rng, 10)
    x = make_series(rng, 1, T)
    prof, hits, mom = fold.reference(x, steps, NB)
    assert prof.shape == (1, 10, NB) and hits.shape == (10, NB) and hits.dtype == np.int32 and mom.shape == (1, 2)
    for p, step in enumerate(steps):
        want_prof, want_hits, want_mom = loop_reference(x[0], int(step), NB)
        assert prof[0, p].tobytes() == want_prof.tobytes(), (T, NB, int(step))
        assert np.array_equal(hits[p], want_hits) and mom[0].tobytes() == want_mom.tobytes()
        assert fold.phase_bins(step, T, NB)[:40].tolist() == [emul().rpf_emul_fold_bin(int(step), t, NB) for t in range(min(T, 40))]
    assert np.all(hits.sum(axis=1) == T) and np.all(hits[0, 1:] == 0)            # step 0: every time in bin 0


@pytest.mark.parametrize("NB", BINS)
@pytest.mark.parametrize("T", TIMES)
def test_the_wave_walk_equals_the_reference_bit_for_bit(T, NB):
    for P in (1, 64, 65):
        for D in (1, 3):
            rng = np.random.default_rng([T, NB, P, D])
            steps, x = make_steps(rng, P), make_series(rng, D, T)
            want_prof, want_hits, want_mom = fold.reference(x, steps, NB)
            # D = 3 in groups of 2 series: the second group is smaller than the first
            prof, hits, mom, disorder, groups = emul_fold(x, steps, NB, per_group=2 if D > 1 else 0)
            assert disorder == 0 and groups == (2 if D > 1 else 1)
            assert prof.tobytes() == want_prof.tobytes(), (T, NB, P, D)
            assert np.array_equal(hits, want_hits) and mom.tobytes() == want_mom.tobytes()
            assert np.all(hits.sum(axis=1) == T)


def test_segments_are_sixteen_and_may_be_empty():
    for T in (0, 1, 15, 16, 17, 1000, 4099, (1 << 31) - 1):
        bounds = [emul().rpf_emul_fold_segment_begin(T, g) for g in range(17)]
        assert bounds == fold.segment_bounds(T) and bounds[0] == 0 and bounds[16] == T and bounds == sorted(bounds)
    assert fold.segment_bounds(17) == [0, 2, 4, 6, 8, 10, 12, 14, 16] + [17] * 8


def test_a_nan_reaches_exactly_the_cells_of_its_bins():
    rng = np.random.default_rng(7)
    T, NB, at = 1000, 7, 613
    steps, x = make_steps(rng, 9), make_series(rng, 2, T)
    x[1, at] = np.nan
    for prof, hits, mom in (fold.reference(x, steps, NB), emul_fold(x, steps, NB)[:3]):
        expect = np.zeros(prof.shape, bool)
        for p, step in enumerate(steps):
            expect[1, p, fold.phase_bins(step, T, NB)[at]] = True
        assert np.array_equal(np.isnan(prof), expect)
        assert np.isnan(mom[1]).all() and np.isfinite(mom[0]).all()


def test_the_scratch_never_exceeds_its_cap_and_the_series_run_in_groups():
    lib = emul()
    cap = lib.rpf_emul_fold_scratch_cap()
    assert cap == 256 << 20
    for D, P, NB in ((1, 1, 1), (11, 9, 16), (256, 1024, 64), (32, 4096, 128), (4096, 32, 128), (4096, 4096, 1)):
        assert D * P * NB <= lib.rpf_emul_fold_max_cells()
        per = lib.rpf_emul_fold_group_series(D, P, NB)
        assert 1 <= per <= D and lib.rpf_emul_fold_scratch_bytes(per, P, NB) <= cap
        assert per == D or lib.rpf_emul_fold_scratch_bytes(per + 1, P, NB) > cap
    assert lib.rpf_emul_fold_group_series(32, 4096, 128) == 3                    # 64 MB of partials per series, 32 MB of hits


# ---- the LDS index ------------------------------------------------------------------------------------------------------------

def test_a_wave_reads_arbitrary_bins_without_a_bank_conflict():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lds_bank_model as model
    lib = emul()
    rng = np.random.default_rng(3)
    NB = lib.rpf_emul_fold_max_bins()
    assert lib.rpf_emul_fold_lanes() == 64 and lib.rpf_emul_fold_lds_bytes(NB) == 65536
    patterns = [rng.integers(0, NB, 64) for _ in range(50)] + [np.zeros(64, int), np.arange(64) % NB, np.arange(64)[::-1] * 2 % NB]
    for bins in patterns:
        dwords = [2 * lib.rpf_emul_fold_lds_index(int(bins[lane]), lane) for lane in range(64)]
        assert model.cycles(dwords, model.G32, 64, 2) == (2, 2)                  # ds_read_b64: two halves, one cycle each
        assert model.cycles(dwords, model.G16, 32, 2) == (4, 4)                  # ds_write_b64: four groups, one cycle each
        assert len(set(dwords)) == 64 and max(dwords) + 2 <= 2 * NB * 64


# ---- period_steps and chi2 in both languages --------------------------------------------------------------------------------

def test_cpp_and_python_period_steps_agree_on_a_grid():
    periods = np.array([0.004256, 0.0043, 0.0333924, 0.089, 0.253, 0.7145, 1.337, 3.7])
    checked = 0
    for rate in (250000.0, 2.4e6, 3.2e6):
        for N in (8, 64, 500, 4096):
            for L, S in ((1, N), (4, N), (16, N // 2), (3, N // 4 * 3)):
                t_row = L * S / rate
                ok = periods[periods / t_row >= 2]
                want = fold.period_steps(ok, rate, N, L, S)
                rc, got, msg = cpp_period_steps(ok, rate, N, L, S)
                assert rc == 0, msg
                assert want.dtype == np.uint64 and np.array_equal(got, want), (rate, N, L, S)
                assert all(0 < int(v) <= 1 << 63 for v in want)
                checked += ok.size
    assert checked > 200
    rows = np.array([2.0, 2.0000000001, 3.0, 40.3, 50.3, 1e6, 1e19, 1e300])
    rc, got, _ = cpp_period_steps(rows, 1.0, 1, 1, 1, in_rows=True)
    want = fold.row_period_steps(rows)
    assert rc == 0 and np.array_equal(got, want)
    assert int(want[0]) == 1 << 63 and abs(int(want[2]) - (1 << 64) // 3) < 1 << 11 and int(want[-1]) == 0
    # the issue's example: 408 MHz, 2.4 MS/s, rows of 4 frames of 64 bins
    assert int(fold.period_steps([40.3 * 4 * 64 / 2.4e6], 2.4e6, 64, 4)[0]) == int(math.ldexp(1.0 / ((40.3 * 4 * 64 / 2.4e6) / (256 / 2.4e6)), 64))


def test_period_steps_refuses_in_both_languages():
    t_row = 4 * 64 / 2.4e6
    for periods in ([1.9 * t_row], [0.0], [float("nan")], [float("inf")], [1.0, 0.5 * t_row]):
        with pytest.raises(ValueError):
            fold.period_steps(periods, 2.4e6, 64, 4)
        rc, _, msg = cpp_period_steps(periods, 2.4e6, 64, 4, 64)
        assert rc == -3 and "two rows" in msg, msg
    for rate in (0.0, -1.0):
        with pytest.raises(ValueError):
            fold.period_steps([1.0], rate, 64, 4)
        rc, _, msg = cpp_period_steps([1.0], rate, 64, 4, 64)
        assert rc == -3 and "rate" in msg, msg
    for rows in ([1.999], [float("nan")], [-5.0]):
        with pytest.raises(ValueError):
            fold.row_period_steps(rows)
        assert cpp_period_steps(rows, 1.0, 1, 1, 1, in_rows=True)[0] == -3


def test_chi2_agrees_between_cpp_and_python():
    rng = np.random.default_rng(5)
    D, T, NB = 3, 3000, 16
    x = rng.standard_normal((D, T)) * 3.0 + 50.0
    x[1, ::40] += 20.0                                                           # a period of 40 rows in series 1
    x[2] = 7.0                                                                   # no variance: NaN
    steps = np.concatenate([fold.row_period_steps([40.0, 41.7, 2.0]), np.array([0], dtype=np.uint64)])
    prof, hits, mom = fold.reference(x, steps, NB)
    a, b = fold.chi2(prof, hits, mom, T), cpp_chi2(prof, hits, mom, T)
    assert a.shape == b.shape == (D, 4)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.isnan(a[2]).all() and np.isnan(a[:, 3]).all() and np.isfinite(a[:2, :3]).all()      # step 0: one bin has hits
    ok = np.isfinite(a)
    assert np.max(np.abs(a[ok] - b[ok]) / np.abs(a[ok])) < 1e-9
    # 75 pulses of 20 in one of 16 bins of 187.5 hits each, variance 9 + 400 (1/40) (39/40) = 18.75: that bin's mean is 7.5
    # above mu, the others 0.5 below, so chi2 is about (187.5 56.25 + 15 187.5 0.25) / 18.75 / 15 = 40; noise alone gives
    # 1 +- sqrt(2 / 15)
    assert a[1, 0] > 20 and a[0, 0] < 3 and a[1, 1] < 5
    # against the definition spelled out
    mu, var = x[1].sum() / T, (x[1] * x[1]).sum() / T - (x[1].sum() / T) ** 2
    used = hits[0] > 0
    spelled = np.sum(hits[0][used] * (prof[1, 0][used] / hits[0][used] - mu) ** 2 / var) / (used.sum() - 1)
    assert a[1, 0] == pytest.approx(spelled, rel=1e-9)
    assert np.isnan(fold.chi2(prof, hits, mom, 0)).all() and np.isnan(cpp_chi2(prof, hits, mom, 0)).all()


# ---- the CLI -----------------------------------------------------------------------------------------------------------------------

def run_cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True)


BASE = ("--input", "/dev/null", "-b", "64", "-r", "2400000", "--dedisperse", "4", "--dm", "0:30:3")


def test_cli_parses_the_options():
    r = run_cli("--help")                    # (the --help text is the one tests/golden/cli_refusals.json pins)
    assert r.returncode == 0 and "--fold" not in r.stdout and "--phase-bins" not in r.stdout
    n, periods, nbins, msg = parse(*BASE, "--fold", "0.004256:0.004342:0.0000107")
    assert n == 9 and nbins == 16, msg
    assert periods.tolist() == [0.004256 + i * 0.0000107 for i in range(9)]
    n, periods, nbins, msg = parse(*BASE, "--fold", "0.0043", "--phase-bins", "128")
    assert n == 1 and periods.tolist() == [0.0043] and nbins == 128, msg
    assert parse(*BASE, "--fold", "1:4096:1")[0] == 4096
    assert parse(*BASE, "--fold", "0.0043", "--phase-bins", "1")[2] == 1
    assert parse(*BASE)[0] == 0 and parse("--input", "x", "-b", "64")[0] == 0
    # a good command line: what fails next is not the option (there is no device here, or the file is empty)
    r = run_cli(*BASE, "--fold", "0.0043:0.0044:0.00001", "--phase-bins", "32", "-q", "-l")
    assert "--fold" not in r.stderr and "--phase-bins" not in r.stderr and "--dedisperse" not in r.stderr, r.stderr


def test_cli_refuses_the_misuse_of_fold():
    for args, words in (
            (("--input", "/dev/null", "--fold", "0.0043"), ("--fold needs --dedisperse",)),
            (("--input", "/dev/null", "--phase-bins", "16"), ("--phase-bins needs --dedisperse",)),
            (("--input", "/dev/null", "--quantile", "4", "--fold", "0.0043"), ("--fold needs --dedisperse",)),
            (BASE + ("--phase-bins", "16"), ("--phase-bins needs --fold",)),
            (BASE + ("--fold", "0.0043", "--phase-bins", "0"), ("--dedisperse", "1 to 128 phase bins", "got 0")),
            (BASE + ("--fold", "0.0043", "--phase-bins", "129"), ("--dedisperse", "1 to 128 phase bins", "got 129")),
            (BASE + ("--fold", "1:4097:1"), ("--dedisperse", "at most 4096 trials in --fold", "4097")),
            (("--input", "/dev/null", "-b", "64", "--dedisperse", "4", "--dm", "0:4095:1", "--fold", "1:1024:1", "--phase-bins", "128"),
             ("--dedisperse", "at most 16777216 cells", str(4096 * 1024 * 128))),
            # a period under two integrations: 4 frames of 64 samples at 2.4 MS/s are 106.667 us
            (BASE + ("--fold", "0.0002"), ("--dedisperse", "--fold", "under two integrations", "shortest period that works is 0.000213333333 s")),
            (BASE + ("--fold", "0.0043:0.0044:0.00001", "--stats"), ("--dedisperse", "--stats")),
            (BASE + ("--fold", "0.0043", "-n", "10"), ("--dedisperse", "--repeats"))):
        r = run_cli(*args)
        assert r.returncode == 3, (args, r.stderr)
        for word in words:
            assert word in r.stderr, (args, r.stderr)
        assert "Exiting." in r.stderr and "# fold" not in r.stdout
    for bad in ("", "a", "1:2", "1:2:3:4", "2:1:1", "0:10:0", "-1", "nan", "inf", "1:", " 1", "0x10"):
        r = run_cli(*BASE, "--fold", bad)
        assert r.returncode == 3 and "--dedisperse" in r.stderr and "--fold" in r.stderr, (bad, r.stderr)
    # what --dedisperse refuses stays refused, with its present message
    r = run_cli("--input", "/dev/null", "--dedisperse", "4", "--fold", "0.0043")
    assert r.returncode == 3 and "needs --dm" in r.stderr, r.stderr


@pytest.mark.parametrize("linear", [False, True])
def test_cli_block_writers(linear):
    rng = np.random.default_rng(13)
    D, P, NB, T, nb = 4, 5, 16, 1967, 63
    dms, periods = np.arange(D) * 7.5, 0.004256 + np.arange(P) * 0.0000107
    prof = rng.uniform(50.0, 80.0, (D, P, NB)) * 123.0
    hits = rng.integers(100, 130, (P, NB)).astype(np.int32)
    chi2 = rng.uniform(0.5, 2.0, (D, P))
    chi2[2, 3], chi2[1, 1] = 19.25, np.nan
    hits[3, 5], prof[2, 3, 5] = 0, 0.0                                           # a bin without hits: nan
    prof[2, 3, 7] = 0.0                                                          # -inf in dB
    lines = cpp_blocks(dms, periods, NB, T, chi2, prof, hits, nb, linear)
    assert lines[0] == "# rtl-power-fftw output" and lines[1] == "# Acquisition start: a" and lines[2] == "# Acquisition end: b"
    assert lines[3] == "# fold: 4 DMs x 5 periods, 16 phase bins, 1967 times" and lines[4] == "#"
    assert lines[5] == "# DM [pc cm^-3] period [s] reduced chi2"
    # DM-major, a blank line between the DMs and one more at the end of the block
    body = lines[6:6 + D * (P + 1) + 1]
    assert [i for i, ln in enumerate(body) if ln == ""] == [5, 11, 17, 23, 24]
    assert body[0] == "0 0.004256 %s" % c_six(chi2[0, 0]) and body[7] == "7.5 0.0042667 nan"
    second = lines[6 + D * (P + 1) + 1:]
    assert second[0] == "# rtl-power-fftw output" and second[3] == "# DM 15 pc cm^-3, period 0.0042881 s, reduced chi2 19.25"
    assert second[4] == "#" and second[5] == "# phase [turns] power [median units] hits"
    assert second[6].split()[0] == "0.03125" and second[6 + 5] == "0.34375 nan 0" and second[6 + NB:] == ["", ""]
    assert second[6 + 7].split()[1] == ("0" if linear else "-inf")
    assert essential(lines) == python_blocks(dms, periods, NB, T, chi2, prof, hits, nb, linear)
    value = prof[2, 3, 0] / (hits[3, 0] * nb)
    assert float(second[6].split()[1]) == pytest.approx(value if linear else 10 * np.log10(value), rel=1e-5)


# ---- what it is for: a pulsar too weak for any single pulse -------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_reference_alone_finds_the_pulsar_in_a_model_of_the_rows(seed):
    N, L, NB = PULSAR["N"], PULSAR["L"], PULSAR["NB"]
    stream, delays = pulsar_stream(seed)
    rows = model_rows(stream, N, L)
    w = 1.0 / np.median(rows, axis=0)
    w[N // 2] = 0.0
    plane = dedisperse.reference(rows, delays, w)
    T = plane.shape[1]
    assert delays.max() == 81 and T == 1967
    prof, hits, mom = fold.reference(plane, pulsar_steps(), NB)
    c = fold.chi2(prof, hits, mom, T)
    assert c.shape == (11, 9) and np.isfinite(c).all()
    order = np.sort(c.ravel())
    print("seed %d: strongest cell %s, reduced chi2 %.1f, second %.1f, DM 0 at most %.1f"
          % (seed, best_cell(c), order[-1], order[-2], c[0].max()))
    assert best_cell(c) == (PULSAR["dm_index"], 4)
    assert np.all(c.max() > 2 * c[0])
