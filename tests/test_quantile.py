"""Per-bin quantiles of the integrations, the parts that need no GPU: the C-ABI additions, stats.quantiles against
numpy, the kernels' steps and pass order on the host (tests/emul/quantile_emul.cpp compiles csrc/quantile_core.h, the
text the kernels compile), the CLI's options and its block writer.

The reference is stats.quantiles, the numpy statement of the definition in include/rpf_engine.h."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, stats
from helpers import ROOT

HEADER = os.path.join(ROOT, "include", "rpf_engine.h")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
NEW = ("rpf_quantile_reset", "rpf_quantile_append_device", "rpf_quantile_append", "rpf_quantile_select_device",
       "rpf_quantile_select", "rpf_quantile_rows", "rpf_quantile_max_rows")
Q8 = np.array([0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1], dtype=np.float64)
# stats.quantiles against np.quantile on positive rows: both interpolate once between the same two doubles a <= b.  Each
# evaluation rounds b - a, the product with g (or 1 - g) and the sum, every rounding at most 2^-53 of a quantity no
# larger than the result, so each lies within 3 x 1.1e-16 of the exact value and the two within 7e-16 of each other:
# 1e-14 leaves a factor of over ten.  (Rows are sums of |X|^2, never negative; with mixed signs a result near zero
# has no relative accuracy in either formula.)
NUMPY_REL = 1e-14


def host_lib():
    return ctypes.CDLL(os.path.join(ROOT, "rtl-power-fftw_amd", "host", "librpf_host.so"))


# ---- interface agreement ------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_quantile_entries():
    raw = open(HEADER).read()
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    for decl in (
            "int rpf_quantile_reset(rpf_engine* e);",
            "int rpf_quantile_append_device(rpf_engine* e, const void* d_stream, size_t nbytes, int64_t frames_per_spectrum, "
            "int64_t max_spectra, void* hip_stream, int64_t* appended);",
            "int rpf_quantile_append(rpf_engine* e, const uint8_t* stream, size_t nbytes, int64_t frames_per_spectrum, "
            "int64_t max_spectra, int64_t* appended);",
            "int rpf_quantile_select_device(rpf_engine* e, const double* q , int nq, double* d_out , void* hip_stream);",
            "int rpf_quantile_select(rpf_engine* e, const double* q, int nq, double* out );",
            "int64_t rpf_quantile_rows(const rpf_engine* e);",
            "int64_t rpf_quantile_max_rows(const rpf_engine* e);"):
        assert decl in text, decl
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True,
                              check=True).stdout
    for name in NEW:
        assert name in _lib.symbol_names()
        assert re.search(r"\bT %s$" % name, exported, re.M), name
    sym = {s[0]: s for s in _lib._SYMBOLS}
    P, i64, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
    assert sym["rpf_quantile_append_device"][1:] == (ctypes.c_int, [P, P, ctypes.c_size_t, i64, i64, P, ctypes.POINTER(i64)])
    assert sym["rpf_quantile_append"][1:] == (ctypes.c_int, [P, P, ctypes.c_size_t, i64, i64, ctypes.POINTER(i64)])
    assert sym["rpf_quantile_select_device"][1:] == (ctypes.c_int, [P, ctypes.POINTER(dbl), ctypes.c_int, P, P])
    assert sym["rpf_quantile_select"][1:] == (ctypes.c_int, [P, ctypes.POINTER(dbl), ctypes.c_int, ctypes.POINTER(dbl)])
    assert sym["rpf_quantile_rows"][1:] == (i64, [P]) and sym["rpf_quantile_max_rows"][1:] == (i64, [P])
    # the ABI version did not move: the entries are additive within 2, and the header's comment lists them
    assert re.search(r"#define RPF_ABI_VERSION 2\b", raw)
    comment = raw.split("#define RPF_ABI_VERSION 2", 1)[1].split("*/", 1)[0]
    assert all(name in comment for name in NEW)
    lib = rpf.load()
    assert lib.rpf_abi_version() == 2
    # NULL engine: invalid argument or -1, nothing dereferenced
    bad = rpf.ReturnValue.InvalidArgument
    q = (ctypes.c_double * 1)(0.5)
    assert lib.rpf_quantile_reset(None) == bad
    assert lib.rpf_quantile_append_device(None, None, 0, 1, 1, None, None) == bad
    assert lib.rpf_quantile_append(None, None, 0, 1, 1, None) == bad
    assert lib.rpf_quantile_select_device(None, q, 1, None, None) == bad
    assert lib.rpf_quantile_select(None, q, 1, None) == bad
    assert lib.rpf_quantile_rows(None) == -1 and lib.rpf_quantile_max_rows(None) == -1
    for method in ("quantile_reset", "quantile_append", "quantile_append_device", "quantile_select",
                   "quantile_select_device", "accumulate_quantiles"):
        assert callable(getattr(rpf.Datastore, method))
    assert isinstance(rpf.Datastore.quantile_rows, property) and isinstance(rpf.Datastore.quantile_max_rows, property)
    host = host_lib()
    assert host.rpf_host_accumulate_quantiles and host.rpf_host_format_text_quantiles


# ---- stats.quantiles ----------------------------------------------------------------------------------------------
def positive_rows(seed, K, N):
    rng = np.random.default_rng(seed)
    return rng.exponential(size=(K, N)) * 10.0 ** rng.uniform(2, 9, size=N)


@pytest.mark.parametrize("K", [1, 2, 3, 64, 257])
def test_stats_quantiles_against_numpy(K):
    rows = positive_rows(K, K, 300)
    got = stats.quantiles(rows, Q8)
    want = np.quantile(rows, Q8, axis=0)
    rel = float(np.max(np.abs(got - want) / want))
    print("K=%d: stats.quantiles vs np.quantile, worst relative difference %.3g (bar %g)" % (K, rel, NUMPY_REL))
    assert got.shape == (8, 300) and rel < NUMPY_REL
    # exact at q = 0 and 1 and wherever g = 0
    assert np.array_equal(got[0], rows.min(axis=0)) and np.array_equal(got[7], rows.max(axis=0))
    ordered = np.sort(rows, axis=0)
    for i, q in enumerate(Q8):
        h = q * (K - 1)
        if h == np.floor(h):
            assert np.array_equal(got[i], ordered[int(h)]), q
    if K % 2 == 1:
        assert np.array_equal(got[3], np.median(rows, axis=0))


def test_stats_quantiles_edges():
    assert np.all(np.isnan(stats.quantiles(np.zeros((0, 5)), [0.5, 1.0]))) and stats.quantiles(np.zeros((0, 5)), [0.5, 1.0]).shape == (2, 5)
    rows = np.array([[1.0, np.nan], [3.0, 2.0], [2.0, -np.nan], [np.inf, 1.0]])
    got = stats.quantiles(rows, [0.0, 0.5, 1.0])
    assert np.array_equal(got[:, 0], [1.0, 2.5, np.inf])
    assert got[0, 1] == 1.0 and np.isnan(got[1, 1]) and np.isnan(got[2, 1])          # NaN last; 1.5: between 2 and NaN
    assert stats.quantiles(rows[:, :1], 0.5).shape == (1, 1)
    for bad in (-0.1, 1.5, np.nan):
        with pytest.raises(ValueError):
            stats.quantiles(rows, [0.5, bad])


# ---- the kernels' steps and pass order, on the host ---------------------------------------------------------------
@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "librpf_emul_quantile.so"))
    ll, i, pd = ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_double)
    lib.rpf_emul_quantile.restype = ll
    lib.rpf_emul_quantile.argtypes = [pd, ll, i, pd, i, i, pd]
    lib.rpf_emul_quantile_keys.restype = None
    lib.rpf_emul_quantile_keys.argtypes = [pd, ll, ctypes.POINTER(ctypes.c_ulonglong), pd]
    return lib


def emulate(emul, rows, q, groups):
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    q = np.ascontiguousarray(q, dtype=np.float64)
    K, N = rows.shape
    pd = ctypes.POINTER(ctypes.c_double)
    out = np.full((q.size, N), -1.0)
    passes = emul.rpf_emul_quantile(rows.ctypes.data_as(pd), K, N, q.ctypes.data_as(pd), q.size, groups, out.ctypes.data_as(pd))
    assert passes >= 0
    return out, passes


SPECIALS = [np.inf, -np.inf, np.nan, -np.nan, 0.0, -0.0, 5e-324, -5e-324, 1e-310, 2.2250738585072014e-308, 1.0, -1.0]


def test_keys_ascend_as_np_sort_orders_and_come_back(emul):
    rng = np.random.default_rng(3)
    v = np.concatenate([SPECIALS, rng.standard_normal(2000) * 10.0 ** rng.uniform(-300, 300, size=2000)])
    keys = np.zeros(v.size, dtype=np.uint64)
    back = np.zeros(v.size)
    emul.rpf_emul_quantile_keys(v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), v.size,
                                keys.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)),
                                back.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert np.array_equal(np.sort(v), v[np.argsort(keys, kind="stable")], equal_nan=True)
    finite = ~np.isnan(v)
    assert back[finite].tobytes() == v[finite].tobytes()                   # bit for bit, -0.0 and subnormals included
    assert np.all(np.isnan(back[~finite])) and np.all(keys[~finite] == np.uint64(0xFFFFFFFFFFFFFFFF))
    assert keys[1] == keys.min() and np.all(keys[finite] < np.uint64(0xFFFFFFFFFFFFFFFF))


@pytest.mark.parametrize("K", [1, 2, 3, 64, 257])
def test_emulator_equals_stats_quantiles(emul, K):
    rng = np.random.default_rng(10 + K)
    N = 40
    rows = rng.standard_normal((K, N)) * 10.0 ** rng.uniform(-300, 300, size=N)            # random doubles, both signs
    rows[:, 0] = 3.25                                                      # all equal
    rows[:, 1] = np.where(rng.random(K) < 0.5, 1.0, 2.0)                   # two distinct values
    rows[:, 2] = np.where(np.arange(K) % 2 == 0, 7.0, 9.0)                 # ... in equal shares (up to one)
    rows[:, 3] = rng.choice(SPECIALS, size=K)                              # +-inf, NaN of both signs, zeros, subnormals
    rows[:, 4] = rng.choice([np.nan, -np.nan, 1.0], size=K)
    rows[:, 5] = np.nan
    rows[:, 6] = rng.choice([0.0, 5e-324, 1e-310, 1.5e-310], size=K)
    want = stats.quantiles(rows, Q8)
    first = None
    for groups in (1, 3, 8):
        got, passes = emulate(emul, rows, Q8, groups)
        assert np.array_equal(got, want, equal_nan=True), (K, groups)
        assert passes == (16 if K == 1 else 17)                            # K = 1: g = 0 everywhere, no further pass
        first = got if first is None else first
        assert got.tobytes() == first.tobytes()                            # the split of the rows changes nothing
    # one quantile at a time gives the same planes as all eight together
    for i in (1, 3, 6):
        one, _ = emulate(emul, rows, Q8[i:i + 1], 3)
        assert one.tobytes() == first[i:i + 1].tobytes()
    # q = 0, 0.5 (K odd), 1 need no further pass: g = 0
    if K % 2 == 1:
        got, passes = emulate(emul, rows, [0.0, 0.5, 1.0], 2)
        assert passes == 16 and np.array_equal(got, want[[0, 3, 7]], equal_nan=True)


def test_emulator_on_exact_ties_and_no_rows(emul):
    # 51 / 50 copies of two values: every rank falls inside a run of equal keys, except the one that straddles them
    rows = np.tile(np.array([[2.0], [5.0]]), (51, 3))[:101]
    got, _ = emulate(emul, rows, Q8, 4)
    assert np.array_equal(got, stats.quantiles(rows, Q8))
    assert np.array_equal(got[:, 0], [2, 2, 2, 2, 5, 5, 5, 5])
    out, passes = emulate(emul, np.zeros((0, 6)), [0.5, 1.0], 2)
    assert passes == 0 and out.shape == (2, 6) and np.all(np.isnan(out))


# ---- CLI ------------------------------------------------------------------------------------------------------------
def run_cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True)


def test_cli_quantile_option_conflicts():
    r = run_cli("--help")
    assert r.returncode == 0 and "--quantile <frames>" in r.stdout and "--quantiles <a,b,...>" in r.stdout
    base = ["--quantile", "16", "--input", "/dev/null"]
    conflicts = [
        (["--quantile", "16"], "--input"),
        (base + ["--series", "16"], "--series:"),
        (base + ["--series-stats", "16"], "--series-stats:"),
        (base + ["--excise", "16"], "--excise:"),
        (base + ["--stats"], "--stats"),
        (base + ["--pfb", "4"], "--pfb"),
        (base + ["-m", "/tmp/rpf_quantile_m"], "-m"),
        (base + ["-n", "16"], "--repeats (-n)"),
        (base + ["-t", "1"], "--time (-t)"),
        (base + ["-c"], "--continue (-c)"),
        (base + ["-e", "10"], "--elapsed (-e)"),
        (base + ["-f", "100M:110M"], "frequency range in -f"),
        (base + ["--gpus", "0,1"], "--gpus"),
        (["--quantile", "0", "--input", "/dev/null"], "at least 1"),
        (["--quantile", "-3", "--input", "/dev/null"], "at least 1"),
        (base + ["--quantiles", ""], "--quantiles"),
        (base + ["--quantiles", "0.1,,0.5"], "--quantiles"),
        (base + ["--quantiles", "0.1,1.5"], "[0, 1]"),
        (base + ["--quantiles", "-0.1"], "[0, 1]"),
        (base + ["--quantiles", "0.5,half"], "--quantiles"),
        (base + ["--quantiles", "nan"], "[0, 1]"),
        (base + ["--quantiles", "0,.1,.2,.3,.4,.5,.6,.7,.8"], "at most 8"),
    ]
    for args, word in conflicts:
        r = run_cli(*args)
        assert r.returncode == 3, (args, r.returncode, r.stderr)
        assert "--quantile" in r.stderr and word in r.stderr, (args, r.stderr)
    r = run_cli("--quantiles", "0.5", "--input", "/dev/null")
    assert r.returncode == 3 and "--quantiles" in r.stderr and "needs --quantile" in r.stderr
    r = run_cli("--quantile", "many", "--input", "/dev/null")
    assert r.returncode == 4            # not a number: the parser's own error, as for every numeric option
    # what applies: -w, --format, --frame-overlap, -l and a baseline parse beside it (the run then fails for want of a
    # device or of input, not of arguments)
    r = run_cli(*(base + ["--quantiles", "0.1,0.5,0.9", "--format", "cs16", "--frame-overlap", "50", "-l", "-q"]))
    assert r.returncode not in (3, 4), r.stderr


def test_host_options_carry_the_quantile_list():
    host = host_lib()
    fn = host.rpf_host_parse_quantiles
    fn.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_longlong),
                   ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]

    def parse(*args):
        argv = (ctypes.c_char_p * (len(args) + 1))(b"rpf_power", *[a.encode() for a in args])
        frames, q, msg = ctypes.c_longlong(-1), (ctypes.c_double * 8)(), ctypes.create_string_buffer(512)
        n = fn(len(args) + 1, argv, ctypes.byref(frames), q, 8, msg, 512)
        return n, frames.value, list(q)[:max(n, 0)], msg.value.decode()

    assert parse("--quantile", "32", "--input", "x") == (1, 32, [0.5], "")
    assert parse("--quantile", "1", "--quantiles", "0.1,0.5,0.9,1", "--input", "x") == (4, 1, [0.1, 0.5, 0.9, 1.0], "")
    assert parse("--input", "x") == (0, 0, [], "")
    n, _, _, msg = parse("--quantile", "8", "--quantiles", "2", "--input", "x")
    assert n == -3 and "[0, 1]" in msg
    n, _, _, msg = parse("--quantiles", "0.5", "--input", "x")
    assert n == -3 and "needs --quantile" in msg


def test_cli_quantile_block_writer():
    """write_spectrum_text_quantiles: every column is its plane / L with the DC bin the mean of its neighbours, then the
    usual / N / rate, dB and baseline; the header names one column per quantile."""
    host = host_lib()
    fn = host.rpf_host_format_text_quantiles
    fn.restype = ctypes.c_long
    pd = ctypes.POINTER(ctypes.c_double)
    fn.argtypes = [pd, pd, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, pd,
                   ctypes.c_char_p, ctypes.c_size_t]
    N, L, rate, freq = 8, 4, 2000000, 100000000
    rng = np.random.default_rng(2)
    q = np.array([0.1, 0.5, 0.99])
    planes = np.sort(rng.uniform(1e6, 2e6, size=(3, N)) * L, axis=0)
    base = rng.uniform(-1, 1, size=N)
    for linear, baseline in ((0, None), (1, None), (0, base)):
        buf = ctypes.create_string_buffer(1 << 14)
        n = fn(planes.ctypes.data_as(pd), q.ctypes.data_as(pd), 3, N, L, freq, rate, linear,
               None if baseline is None else baseline.ctypes.data_as(pd), buf, 1 << 14)
        assert n > 0
        text = buf.value.decode().splitlines()
        head = [ln for ln in text if ln.startswith("#")]
        assert head[-1] == "# frequency [Hz] quantile 0.1 [dB/Hz] quantile 0.5 [dB/Hz] quantile 0.99 [dB/Hz]"
        lines = [ln.split() for ln in text if ln.strip() and not ln.startswith("#")]
        assert len(lines) == N and all(len(ln) == 4 for ln in lines)
        for c in range(3):
            col = planes[c] / L
            col[N // 2] = (col[N // 2 - 1] + col[N // 2 + 1]) / 2
            want = col / N / rate
            if not linear:
                want = 10 * np.log10(want)
            if baseline is not None:
                want = want - baseline
            for i, ln in enumerate(lines):
                assert abs(float(ln[1 + c]) - want[i]) <= 1e-5 * abs(want[i])        # six significant digits printed
    # one quantile: the block of the plain writer for the same plane and repeats_done = L
    plain = host.rpf_host_format_text
    plain.restype = ctypes.c_long
    plain.argtypes = [pd, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, pd, ctypes.c_char_p,
                      ctypes.c_size_t]
    a, b = ctypes.create_string_buffer(1 << 14), ctypes.create_string_buffer(1 << 14)
    half = np.array([0.5])
    assert fn(planes[1].ctypes.data_as(pd), half.ctypes.data_as(pd), 1, N, L, freq, rate, 0, None, a, 1 << 14) > 0
    assert plain(planes[1].copy().ctypes.data_as(pd), N, L, freq, rate, 0, None, b, 1 << 14) > 0
    body = [ln for ln in a.value.decode().splitlines() if not ln.startswith("#")]
    assert body == b.value.decode().splitlines()
