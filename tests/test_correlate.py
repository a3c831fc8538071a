"""Correlator of up to eight streams, everything that needs no GPU: the two C-ABI additions, the shared core of
csrc/correlate_core.h on the host emulator (tests/emul/correlate_emul.cpp: the per-frame term, the pair -> plane map, the
frame-group partition, the chunk rule), the float64 reference, coherence in Python and in the C++ host, the CLI option
and what it refuses, and the recorded CPU float32 figures behind the GPU test's bar (correlate_bars.py).
tests/test_gpu_correlate.py imports the helpers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, correlate, stats, stft, synth
from helpers import ROOT, dp
import correlate_bars

HEADER = os.path.join(ROOT, "include", "rpf_engine.h")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
ll = ctypes.c_longlong
_emul = None


# ---- helpers (shared with tests/test_gpu_correlate.py) --------------------------------------------------------------------

def emul():
    global _emul
    if _emul is None:
        lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "librpf_emul_correlate.so"))
        lib.rpf_emul_correlate_term.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ll, dp, dp]
        lib.rpf_emul_correlate_plane.argtypes = [ctypes.c_int] * 4
        lib.rpf_emul_correlate_chunk_frames.restype = ll
        lib.rpf_emul_correlate_chunk_frames.argtypes = [ctypes.c_int]
        lib.rpf_emul_correlate_groups.restype = ll
        lib.rpf_emul_correlate_groups.argtypes = [ctypes.c_int, ctypes.c_int, ll]
        lib.rpf_emul_correlate_group_begin.restype = ll
        lib.rpf_emul_correlate_group_begin.argtypes = [ll, ll, ll]
        _emul = lib
    return _emul


def host_lib():
    lib = ctypes.CDLL(os.path.join(ROOT, "rtl-power-fftw_amd", "host", "librpf_host.so"))
    lib.rpf_host_coherence_pair.argtypes = [dp, dp, dp, dp, ctypes.c_int, dp]
    lib.rpf_host_format_text_correlate.restype = ctypes.c_long
    lib.rpf_host_format_text_correlate.argtypes = [dp, ctypes.c_int, ctypes.c_int, ll, ll, ctypes.c_int, ctypes.c_int, dp,
                                                   ctypes.c_char_p, ctypes.c_size_t]
    lib.rpf_host_format_header_correlate.restype = ctypes.c_long
    lib.rpf_host_format_header_correlate.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p,
                                                     ctypes.c_size_t]
    return lib


def emul_term(a, b):
    """The emulator's (t_re, t_im) of float32 (n, 2) values a and b."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    n = a.shape[0]
    re, im = np.full(n, np.nan), np.full(n, np.nan)
    assert emul().rpf_emul_correlate_term(a.ctypes.data, b.ctypes.data, n, re.ctypes.data_as(dp), im.ctypes.data_as(dp)) == 0
    return re, im


def as_vis(V):
    """(M, M, N) complex -> the engine's (M, M, 2, N) doubles."""
    V = np.asarray(V)
    return np.ascontiguousarray(np.stack([V.real, V.imag], axis=2), dtype=np.float64)


def format_correlate_block(V, frames, N, cfreq=1420405752, rate=2000000, linear=False, baseline=None):
    """The data lines of the CLI's --correlate block from (M, M, N) visibilities, by the C++ host's writer; `baseline`:
    the N values -B subtracts from every power column."""
    vis = as_vis(V)
    M = vis.shape[0]
    buf = ctypes.create_string_buffer((40 + 30 * M * M) * N)
    if baseline is not None:
        baseline = np.ascontiguousarray(baseline, dtype=np.float64)
        assert baseline.shape == (N,)
    host_lib().rpf_host_format_text_correlate(vis.ctypes.data_as(dp), M, N, frames, cfreq, rate, int(linear),
                                              None if baseline is None else baseline.ctypes.data_as(dp), buf, len(buf))
    return [l for l in buf.value.decode().split("\n") if l.strip()]


def correlate_header_titles(M):
    buf = ctypes.create_string_buffer(4096)
    host_lib().rpf_host_format_header_correlate(b"start", b"end", M, buf, len(buf))
    return [l for l in buf.value.decode().split("\n") if l.startswith("#")][-1]


def same_bits(x, y):
    """Equal as doubles (-0 == +0), NaN where the other is NaN."""
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(x[~np.isnan(x)], y[~np.isnan(y)])


# ---- header, binding and library ----------------------------------------------------------------------------------------

def test_header_binding_and_library_agree_on_the_two_symbols():
    text = open(HEADER).read()
    assert re.search(r"\bint rpf_correlate_device\(rpf_engine\* e, const void\* const\* d_streams, int n_streams, size_t nbytes, "
                     r"int64_t repeats,\s+double\* d_out[^;]*, void\* hip_stream, int64_t\* frames_done\);", text)
    assert re.search(r"\bint rpf_correlate\(rpf_engine\* e, const uint8_t\* const\* streams, int n_streams, size_t nbytes, "
                     r"int64_t repeats,\s+double\* out[^;]*, int64_t\* frames_done\);", text)
    m = re.search(r"#define RPF_ABI_VERSION 2(.*?)\*/", text, re.S)
    assert m and re.search(r"\brpf_correlate_device\b", m.group(1)) and re.search(r"\brpf_correlate\b", m.group(1))
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in ("rpf_correlate_device", "rpf_correlate"):
        assert name in _lib.symbol_names()
        assert re.search(r"\bT %s$" % name, exported, re.M), name
    lib = rpf.load()
    assert lib.rpf_abi_version() == 2
    out = np.zeros(8)
    assert lib.rpf_correlate(None, None, 2, 0, 0, out.ctypes.data_as(dp), None) == rpf.ReturnValue.InvalidArgument
    assert lib.rpf_correlate_device(None, None, 2, 0, 0, None, None, None) == rpf.ReturnValue.InvalidArgument
    assert hasattr(rpf.Datastore, "correlate") and hasattr(rpf.Datastore, "correlate_device")


# ---- the per-frame term ---------------------------------------------------------------------------------------------------

def special_pairs(n, seed):
    """n random float32 pairs (a, b) as (n, 2) arrays, with subnormals, +-0, values near FLT_MAX, Inf and NaN mixed in."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 1 << 32, size=(2, n, 2), dtype=np.uint64).astype(np.uint32)
    x = bits.view(np.float32)                              # every exponent, NaN and Inf included
    normal = (rng.standard_normal((2, n, 2)) * 10.0 ** rng.uniform(-30, 30, (2, n, 2))).astype(np.float32)
    x = np.where(rng.random((2, n, 2)) < 0.5, normal, x)
    fmax = np.finfo(np.float32).max
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, fmax, -fmax, np.float32(1e-45), np.float32(-3e-39),
                        np.float32(1.17e-38), 1.0, -1.0], dtype=np.float32)
    pick = rng.random((2, n, 2)) < 0.05
    x = np.where(pick, special[rng.integers(0, special.size, (2, n, 2))], x)
    return np.ascontiguousarray(x[0]), np.ascontiguousarray(x[1])


def test_the_term_is_numpys_float64_expression_bit_for_bit():
    a, b = special_pairs(1_000_000, 1)
    assert np.isnan(a).any() and np.isinf(b).any() and (np.abs(a[a != 0]) < np.finfo(np.float32).tiny).any()
    re, im = emul_term(a, b)
    with np.errstate(invalid="ignore", over="ignore"):
        ar, ai = a[:, 0].astype(np.float64), a[:, 1].astype(np.float64)
        br, bi = b[:, 0].astype(np.float64), b[:, 1].astype(np.float64)
        want_re = ar * br + ai * bi
        want_im = ai * br - ar * bi
    for got, want in ((re, want_re), (im, want_im)):
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        assert np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64))          # the bits, signs of zeros included
    print("term: %d pairs, %d NaN, %d Inf, %d zero terms" % (a.shape[0], int(np.isnan(want_re).sum()),
                                                              int(np.isinf(want_re).sum()), int((want_re == 0).sum())))


def test_swapping_the_operands_negates_the_imaginary_part():
    a, b = special_pairs(1_000_000, 2)
    re_ab, im_ab = emul_term(a, b)
    re_ba, im_ba = emul_term(b, a)
    assert same_bits(re_ab, re_ba)
    assert same_bits(im_ba, -im_ab)


def test_the_term_of_a_value_with_itself_is_its_power():
    a, _ = special_pairs(100_000, 3)
    re, im = emul_term(a, a)
    with np.errstate(invalid="ignore", over="ignore"):
        ar, ai = a[:, 0].astype(np.float64), a[:, 1].astype(np.float64)
        assert same_bits(re, ar * ar + ai * ai)
    fin = np.isfinite(a).all(axis=1)
    assert np.array_equal(im[fin].view(np.int64), np.zeros(int(fin.sum()), dtype=np.int64))     # +0, not -0


# ---- pair map, partition, chunk rule --------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", range(2, 9))
def test_the_pair_map_is_a_bijection_onto_the_planes(M):
    planes = [emul().rpf_emul_correlate_plane(M, i, j, 0) for i in range(M) for j in range(i, M)]
    planes += [emul().rpf_emul_correlate_plane(M, i, j, 1) for i in range(M) for j in range(i + 1, M)]
    assert sorted(planes) == list(range(M * M))


@pytest.mark.parametrize("N", [64, 512, 4096, 1 << 20])
def test_the_frame_groups_cover_every_frame_once(N):
    for M in (2, 5, 8):
        for F in (1, 2, 3, 63, 64, 65, 1000, 4099):
            G = emul().rpf_emul_correlate_groups(N, M, F)
            assert 1 <= G <= F
            bounds = [emul().rpf_emul_correlate_group_begin(F, G, g) for g in range(G + 1)]
            assert bounds[0] == 0 and bounds[-1] == F
            assert all(bounds[g] < bounds[g + 1] for g in range(G))               # every group non-empty, in order
            covered = np.concatenate([np.arange(bounds[g], bounds[g + 1]) for g in range(G)])
            assert np.array_equal(covered, np.arange(F))
            if N >= 64 * 4096:
                assert G == 1                                                     # the bins alone fill the GPU
            # the partial planes stay within 64 MB
            assert G == 1 or G * M * M * N * 8 <= 64 << 20


def test_the_chunk_rule():
    assert [emul().rpf_emul_correlate_chunk_frames(N) for N in (4096, 8192, 1 << 20)] == [2048, 1024, 8]
    assert emul().rpf_emul_correlate_chunk_frames(1 << 26) == 1


# ---- reference and derived quantities ----------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,N,step,windowed", [("cu8", 64, None, False), ("cs16", 128, 64, True), ("cf32", 256, None, False)])
def test_the_reference_is_an_einsum_over_the_stft_rows(fmt, N, step, windowed):
    from test_pfb import make_stream
    frames, S = 7, N if step is None else step
    streams = [make_stream(fmt, 10 + m, N + S * (frames - 1) + (5 if m == 1 else 0)) for m in range(3)]
    window = synth.hann_window(N) if windowed else None
    V = correlate.reference(streams, N, fmt, step=step, window=window)
    X = np.stack([stft.reference(s, N, fmt, step=step, window=window)[:frames] for s in streams])
    assert V.shape == (3, 3, N)
    assert np.allclose(V, np.einsum("ifk,jfk->ijk", X, np.conj(X)), rtol=1e-13, atol=0)
    assert np.array_equal(np.diagonal(V, axis1=0, axis2=1).imag, np.zeros((N, 3)))


def test_coherence_matrix_on_hand_made_visibilities():
    V = np.zeros((3, 3, 4), dtype=np.complex128)
    V[0, 0] = [4.0, 2.0, 0.0, 9.0]
    V[1, 1] = [4.0, 8.0, 1.0, 1.0]
    V[2, 2] = [4.0, 3.0, 0.0, 0.0]
    V[0, 1] = [4.0, 2.0 + 2.0j, 0.0, -3.0]
    V[0, 2] = [4.0, 1.0j, 0.0, 0.0]
    V[1, 2] = [4.0, 0.0, 0.0, 0.0]
    for i in range(3):
        for j in range(i):
            V[i, j] = np.conj(V[j, i])
    g = stats.coherence_matrix(V)
    assert g[0, 1, 0] == 1.0 and g[0, 2, 0] == 1.0 and g[1, 2, 0] == 1.0      # V_ij = V_ii = V_jj: exactly 1
    assert g[0, 1, 1] == 0.5 and g[0, 2, 1] == 1.0 / 6.0 and g[1, 0, 3] == 1.0
    assert np.isnan(g[0, 2, 2]) and np.isnan(g[1, 2, 3]) and np.isnan(g[0, 0, 2])   # a zero denominator: NaN, not inf
    assert np.array_equal(g, np.transpose(g, (1, 0, 2)), equal_nan=True)
    W = np.array([[1.0, 1.0 + 2.0 ** -20], [1.0 + 2.0 ** -20, 1.0]], dtype=np.complex128)[:, :, None]
    assert stats.coherence_matrix(W)[0, 1, 0] > 1.0                                # not clamped
    with pytest.raises(ValueError):
        stats.coherence_matrix(np.zeros((2, 3, 4)))


def test_the_host_computes_the_same_coherence():
    rng = np.random.default_rng(7)
    n = 1000
    vii, vjj = rng.random(n) * 1e6, rng.random(n) * 1e3
    re, im = rng.standard_normal(n) * 1e4, rng.standard_normal(n) * 1e4
    vii[:5] = 0.0
    vjj[5:9] = 0.0
    V = np.zeros((2, 2, n), dtype=np.complex128)
    V[0, 0], V[1, 1], V[0, 1], V[1, 0] = vii, vjj, re + 1j * im, re - 1j * im
    g = np.zeros(n)
    host_lib().rpf_host_coherence_pair(vii.ctypes.data_as(dp), vjj.ctypes.data_as(dp), re.ctypes.data_as(dp),
                                       im.ctypes.data_as(dp), n, g.ctypes.data_as(dp))
    assert np.array_equal(g, stats.coherence_matrix(V)[0, 1], equal_nan=True) and np.isnan(g[:9]).all()


# ---- the C++ block writer ------------------------------------------------------------------------------------------------

def six_digits(got, want):
    """`got` is `want` as a stream writes it with six significant digits: within half a unit of the sixth digit (0.51:
    the float parse of the text)."""
    want = np.asarray(want, dtype=np.float64)
    unit = 10.0 ** (np.floor(np.log10(np.maximum(np.abs(want), 1e-300))) - 5)
    return bool(np.all(np.abs(np.asarray(got) - want) <= 0.51 * unit))


@pytest.mark.parametrize("with_baseline", [False, True], ids=["plain", "baseline"])
@pytest.mark.parametrize("linear", [True, False], ids=["linear", "dB"])
@pytest.mark.parametrize("M", [2, 4])
def test_cli_block_writer(M, linear, with_baseline):
    """write_spectrum_text_correlate: the powers by the usual rules (-l or dB, then -B's baseline subtracted from every
    power column and from nothing else), then coherence and phase of every pair i < j, the DC bin of every plane
    interpolated before they are derived."""
    N, frames, rate = 8, 10, 2000000
    rng = np.random.default_rng(8 + M)
    X = rng.standard_normal((M, 5, N)) + 1j * rng.standard_normal((M, 5, N))
    V = np.einsum("ifk,jfk->ijk", X, np.conj(X))
    V[:, :, N // 2] = 1e9 * (1 + 1j)
    # baseline values of the size of the column they are taken from, so that a baseline left out, added or applied in
    # the wrong unit moves the column by far more than its sixth digit
    baseline = (rng.random(N) * (1e-7 if linear else 30.0) + (1e-8 if linear else 1.0)) if with_baseline else None
    lines = format_correlate_block(V, frames, N, rate=rate, linear=linear, baseline=baseline)
    assert len(lines) == N
    vis = as_vis(V)
    vis[:, :, :, N // 2] = 0.5 * (vis[:, :, :, N // 2 - 1] + vis[:, :, :, N // 2 + 1])
    W = vis[:, :, 0] + 1j * vis[:, :, 1]
    g, ph = stats.coherence_matrix(W), np.angle(W)
    pairs = [(i, j) for i in range(M) for j in range(i + 1, M)]
    for k, line in enumerate(lines):
        f = [float(x) for x in line.split()]
        assert len(f) == 1 + M + 2 * len(pairs)
        power = np.array([W[m, m, k].real / frames / N / rate for m in range(M)])
        if not linear:
            power = 10 * np.log10(power)
        if with_baseline:
            power = power - baseline[k]
        want = list(power)
        for i, j in pairs:
            want += [g[i, j, k], ph[i, j, k]]
        assert six_digits(f[1:], want), (k, f, want)
    titles = correlate_header_titles(M)
    assert titles.startswith("# frequency [Hz] power spectral density 0 [dB/Hz]")
    assert titles.endswith("coherence %d-%d phase %d-%d [rad]" % (M - 2, M - 1, M - 2, M - 1))


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------

def run_cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True)


def test_cli_parses_the_option():
    r = run_cli("--help")                    # (the --help text is the one tests/golden/cli_refusals.json pins)
    assert r.returncode == 0 and "--correlate" not in r.stdout
    # a good command line: what fails next is not the option (there is no device here, or the files are empty)
    for more in (("--frame-overlap", "50"), ("--pfb", "4")):
        r = run_cli("--input", "/dev/null", "--correlate", "/dev/null,/dev/null", "-b", "512", "-q", "--format", "cs16", "-l",
                    *more)
        assert r.returncode != 3 and "--correlate" not in r.stderr, (more, r.stderr)


@pytest.mark.parametrize("other,shown", [(("-n", "10"), "--repeats"), (("-t", "1"), "--time"), (("-c",), "--continue"),
                                         (("-e", "10"), "--elapsed"), (("-f", "100M:200M"), "frequency range"),
                                         (("-m", "out"), "-m"), (("--gpus", "0,1"), "--gpus"), (("--stats",), "--stats"),
                                         (("--series", "4"), "--series"), (("--series-stats", "4"), "--series-stats"),
                                         (("--excise", "4"), "--excise"), (("--quantile", "4"), "--quantile"),
                                         (("--cross", "/dev/null"), "--cross"), (("--stft", "/dev/null"), "--stft")])
def test_cli_refuses_what_correlate_does_not_combine_with(other, shown):
    r = run_cli("--input", "/dev/null", "--correlate", "/dev/null", *other)
    assert r.returncode == 3, r.stderr
    assert "--correlate" in r.stderr and shown in r.stderr, r.stderr


def test_cli_correlate_refuses_its_own_misuse():
    r = run_cli("--correlate", "/dev/null")
    assert r.returncode == 3 and "--correlate" in r.stderr and "--input" in r.stderr, r.stderr
    for bad in ("", ",", "/dev/null,", ",".join(["/dev/null"] * 8)):
        r = run_cli("--input", "/dev/null", "--correlate", bad)
        assert r.returncode == 3 and "--correlate" in r.stderr, (bad, r.stderr)
    r = run_cli("--input", "/dev/null", "--correlate", ",".join(["/dev/null"] * 7), "-q")
    assert r.returncode != 3, r.stderr                                              # seven are allowed
    r = run_cli("--input", "/dev/null", "--correlate", "/dev/null", "-b", "500")
    assert r.returncode == 3 and "power-of-two" in r.stderr, r.stderr
    r = run_cli("--input", "-", "--correlate", "/dev/null,-")
    assert r.returncode == 3 and "stdin" in r.stderr, r.stderr


# ---- the recorded CPU float32 figures behind the GPU bar ------------------------------------------------------------------------

@pytest.mark.parametrize("case", correlate_bars.ACCURACY_CASES)
def test_recorded_cpu_float32_error_is_what_the_cpu_path_gives(case):
    """correlate_bars.CPU_F32 (half the GPU test's bar) against a fresh run of the path it records."""
    streams = correlate_bars.accuracy_streams(*case)
    want = correlate_bars.truth(streams, *case)
    got = correlate_bars.cpu_f32(streams, *case)
    err = correlate_bars.err(got, want)
    print("%s N=%d %s M=%d: CPU float32 path vs float64 %.4g (recorded %.4g)" % (case + (err, correlate_bars.CPU_F32[case])))
    assert abs(err / correlate_bars.CPU_F32[case] - 1.0) < 0.02
