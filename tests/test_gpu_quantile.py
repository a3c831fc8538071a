"""Per-bin quantiles of the integrations on the MI355X: rpf_quantile_* / Datastore.quantile_* / rpf_power --quantile.

The reference is stats.quantiles (the numpy statement of the definition in include/rpf_engine.h) on the rows
rpf_accumulate_device_series of THE SAME ENGINE writes for the same stream.  The selection is exact -- integer counts
over order-preserving keys, one interpolation in the reference's order of operations -- so every comparison is
np.array_equal (a NaN equal to a NaN): any mismatch is a defect."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import stats, synth
from helpers import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
Q8 = np.array([0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1], dtype=np.float64)
PERMUTED = [5, 0, 7, 3, 1, 6, 2, 4]


def engine(N, fmt="cu8", step=None, window=False, flags=0, **kw):
    w = synth.hann_window(N) if window else None
    return rpf.Datastore(rpf.Params(N=N, window=window, frame_step=step, sample_format=fmt, **kw), w, flags=flags)


def noise(fmt, seed, nsamples):
    """A stream of nsamples complex samples, as bytes."""
    if fmt == "cu8":
        return synth.noise_tones_iq(seed, nsamples)
    if fmt == "cs16":
        return np.ascontiguousarray(synth.noise_tones_cs16(seed, nsamples)).view(np.uint8).reshape(-1)
    assert fmt == "cf32"
    return np.ascontiguousarray(synth.gaussian_cf32(seed, nsamples, sigma=20.0)).view(np.uint8).reshape(-1)


def to_device(stream):
    return torch.from_numpy(np.ascontiguousarray(stream)).to(DEV)


def current():
    return torch.cuda.current_stream().cuda_stream


def series_rows(ds, d_stream, nbytes, L, K):
    """The engine's own rows: (K, N) from rpf_accumulate_device_series, and its transform launches."""
    out = torch.full((K, ds.params.N), -1.0, dtype=torch.float64, device=DEV)
    done = ds.accumulate_device_series(d_stream.data_ptr(), nbytes, L, K, out.data_ptr(), current())
    torch.cuda.synchronize()
    assert done == K
    return out.cpu().numpy(), ds.series_launches()


def select_device(ds, q):
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    out = torch.full((q.size, ds.params.N), -1.0, dtype=torch.float64, device=DEV)
    ds.quantile_select_device(q, out.data_ptr(), current())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def check_against_rows(ds, stream, L, K, what, launches_want):
    d = to_device(stream)
    rows, launches = series_rows(ds, d, stream.size, L, K)
    assert launches == launches_want, what
    ds.quantile_reset()
    done = ds.quantile_append_device(d.data_ptr(), stream.size, L, K, current())
    assert done == K and ds.quantile_rows == K and ds.series_launches() == launches_want, what
    got = select_device(ds, Q8)
    want = stats.quantiles(rows, Q8)
    wrong = int(np.count_nonzero(~((got == want) | (np.isnan(got) & np.isnan(want)))))
    print("%s: L=%d K=%d launches=%d: %d of %d values differ from stats.quantiles of the engine's rows"
          % (what, L, K, launches, wrong, want.size))
    assert same(got, want), what
    assert same(got[0], rows.min(axis=0)) and same(got[7], rows.max(axis=0)), what
    # the host entry gives the device entry's planes; the rows survived: a permuted q gives the permuted planes
    assert same(ds.quantile_select(Q8), got), what
    assert same(select_device(ds, Q8[PERMUTED]), got[PERMUTED]), what
    assert same(select_device(ds, [0.5]), got[3:4]), what
    assert ds.quantile_rows == K


# ---- 1. equals the reference on the series' own rows, bit for bit -------------------------------------------------------
def test_rows_of_a_bin_span_workgroups_at_64():
    # 5000 rows of 64 bins: one tile of bins, the rows split over hundreds of workgroups
    N, L, K = 64, 1, 5000
    with engine(N) as ds:
        check_against_rows(ds, noise("cu8", 11, N * K * L), L, K, "N=64", 1)


@pytest.mark.parametrize("K", [1, 2, 3, 257])
def test_small_and_odd_row_counts_at_512(K):
    N, L = 512, 4
    with engine(N) as ds:
        check_against_rows(ds, noise("cu8", 20 + K, N * (K * L + 1)), L, K, "N=512 K=%d" % K, 1)


def test_hann_at_4096():
    N, L, K = 4096, 2, 65
    with engine(N, window=True) as ds:
        check_against_rows(ds, noise("cu8", 31, N * K * L), L, K, "N=4096 hann", 1)


def test_fallback_route_at_5000():
    # no multiple of the 64-bin tile, and the series runs spectrum by spectrum
    N, L, K = 5000, 2, 9
    with engine(N) as ds:
        check_against_rows(ds, noise("cu8", 41, N * (K * L + 1)), L, K, "N=5000 spectrum by spectrum", K)


def test_overlapped_frames_at_4096():
    N, L, K = 4096, 3, 9
    S = N // 2 + 1
    with engine(N, step=S) as ds:
        check_against_rows(ds, noise("cu8", 51, N + S * (K * L - 1) + 5), L, K, "N=4096 step %d" % S, K)


@pytest.mark.parametrize("fmt", ["cs16", "cf32"])
def test_formats_at_512(fmt):
    N, L, K = 512, 4, 33
    with engine(N, fmt) as ds:
        # (the plain series has its one-launch kernel for the integer formats; a cf32 engine runs spectrum by spectrum)
        check_against_rows(ds, noise(fmt, 61, N * K * L), L, K, "%s N=512" % fmt, K if fmt == "cf32" else 1)


# ---- 2. exact ties ------------------------------------------------------------------------------------------------------
def test_exact_ties():
    N, L, K = 512, 1, 101
    two = synth.noise_tones_iq(71, 2 * N).reshape(2, 2 * N)
    stream = np.ascontiguousarray(two[np.arange(K) % 2]).reshape(-1)          # frames A B A B ... A: 51 / 50 copies
    with engine(N) as ds:
        d = to_device(stream)
        rows, _ = series_rows(ds, d, stream.size, L, K)
        assert all(np.unique(rows[:, b]).size <= 2 for b in range(N)) and np.unique(rows[:, 7]).size == 2
        assert np.array_equal(rows[0], rows[2]) and np.array_equal(rows[1], rows[3])
        ds.quantile_append_device(d.data_ptr(), stream.size, L, K, current())
        got = select_device(ds, Q8)
        assert same(got, stats.quantiles(rows, Q8))
        lo, hi = np.minimum(rows[0], rows[1]), np.maximum(rows[0], rows[1])
        assert same(got[0], lo) and same(got[7], hi) and np.all((got == lo) | (got == hi))


# ---- 3. NaN -------------------------------------------------------------------------------------------------------------
def test_a_nan_sample_is_the_largest_value_of_every_bin():
    N, L, K = 512, 2, 17
    z = synth.gaussian_cf32(81, N * K * L, sigma=20.0).copy()
    z[5 * L * N + 300] = np.nan                                               # one sample of integration 5
    stream = z.view(np.uint8).reshape(-1)
    with engine(N, "cf32") as ds:
        d = to_device(stream)
        rows, _ = series_rows(ds, d, stream.size, L, K)
        assert np.all(np.isnan(rows[5])) and not np.isnan(np.delete(rows, 5, axis=0)).any()
        ds.quantile_append_device(d.data_ptr(), stream.size, L, K, current())
        got = select_device(ds, Q8)
        assert np.all(np.isnan(got[7]))                                       # q = 1: the NaN, in every bin
        assert not np.isnan(got[:6]).any()
        assert same(got, stats.quantiles(rows, Q8))                           # 0.99: between v_(15) and the NaN -> NaN


# ---- 4. appending -------------------------------------------------------------------------------------------------------
def test_appends_stack_and_reset_empties():
    N, L, K1, K2 = 512, 4, 40, 23
    stream = noise("cu8", 91, N * L * (K1 + K2))
    cut = 2 * N * L * K1
    with engine(N) as ds:
        assert ds.quantile_rows == 0 and ds.quantile_max_rows == (1 << 27) // N
        assert np.all(np.isnan(select_device(ds, [0.5, 1.0])))                # nothing stored, nothing allocated
        d = to_device(stream)
        first, _ = series_rows(ds, d[:cut], cut, L, K1)
        second, _ = series_rows(ds, d[cut:], stream.size - cut, L, K2)
        assert ds.quantile_append_device(d[:cut].data_ptr(), cut, L, 1 << 40, current()) == K1
        half = select_device(ds, Q8)
        assert ds.quantile_append_device(d[cut:].data_ptr(), stream.size - cut, L, 1 << 40, current()) == K2
        assert ds.quantile_rows == K1 + K2
        both = select_device(ds, Q8)
        assert same(half, stats.quantiles(first, Q8))
        assert same(both, stats.quantiles(np.concatenate([first, second]), Q8))
        # a quota below what the stream holds, and a stream without a whole integration
        assert ds.quantile_append_device(d.data_ptr(), stream.size, L, 2, current()) == 2 and ds.quantile_rows == K1 + K2 + 2
        assert ds.quantile_append_device(d.data_ptr(), 2 * N * L - 2, L, 5, current()) == 0 and ds.series_launches() == 0
        assert same(select_device(ds, Q8), stats.quantiles(np.concatenate([first, second, first[:2]]), Q8))
        ds.quantile_reset()
        assert ds.quantile_rows == 0
        empty = select_device(ds, Q8)
        assert empty.shape == (8, N) and np.all(np.isnan(empty)) and np.all(np.isnan(ds.quantile_select([0.0, 1.0])))
        # and the store fills again from the start
        assert ds.quantile_append_device(d[cut:].data_ptr(), stream.size - cut, L, K2, current()) == K2
        assert same(select_device(ds, Q8), stats.quantiles(second, Q8))


# ---- 5. host route --------------------------------------------------------------------------------------------------------
def test_host_route_one_piece():
    N, L, K = 512, 8, 50
    stream = noise("cu8", 101, N * (K * L + 3))
    with engine(N) as ds:
        rows, done = ds.accumulate_series(stream, L)
        assert done == K
        got, appended = ds.accumulate_quantiles(stream, L, Q8)
        assert appended == K and ds.quantile_rows == K and same(got, stats.quantiles(rows, Q8))
        median, appended = ds.accumulate_quantiles(stream, L)                 # the default list: the median
        assert appended == K and ds.quantile_rows == K and same(median, got[3:4])
        few, appended = ds.accumulate_quantiles(stream, L, [0.25], max_spectra=7)
        assert appended == 7 and same(few, stats.quantiles(rows[:7], [0.25]))


def test_host_route_two_pieces():
    # just over 64 MB of input: 128 integrations fill the first piece, two more make the second
    N, L, K = 4096, 64, 130
    stream = np.random.default_rng(111).integers(0, 256, size=2 * N * L * K, dtype=np.uint8)
    assert stream.size > 64 << 20
    with engine(N) as ds:
        rows, done = ds.accumulate_series(stream, L)
        launches = ds.series_launches()
        got, appended = ds.accumulate_quantiles(stream, L, [0.1, 0.5, 0.9])
        assert done == appended == K and launches == ds.series_launches() == 2
        assert same(got, stats.quantiles(rows, [0.1, 0.5, 0.9]))


def test_cpp_host_datastore():
    host = ctypes.CDLL(os.path.join(ROOT, "rtl-power-fftw_amd", "host", "librpf_host.so"))
    fn = host.rpf_host_accumulate_quantiles
    fn.restype = ctypes.c_longlong
    pd = ctypes.POINTER(ctypes.c_double)
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_longlong, ctypes.c_int,
                   pd, ctypes.c_int, pd, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_int), ctypes.c_char_p,
                   ctypes.c_size_t]
    N, L, K = 512, 4, 37
    stream = noise("cu8", 121, N * K * L)
    with engine(N) as ds:
        rows, _ = ds.accumulate_series(stream, L)
    want = stats.quantiles(rows, Q8)
    for pieces in (1, 3):
        out = np.zeros((8, N))
        stored, launches, msg = ctypes.c_longlong(), ctypes.c_int(), ctypes.create_string_buffer(512)
        done = fn(N, 0, 0, stream.ctypes.data, stream.size, L, pieces, Q8.ctypes.data_as(pd), 8, out.ctypes.data_as(pd),
                  ctypes.byref(stored), ctypes.byref(launches), msg, 512)
        assert done == K == stored.value and launches.value == 1, msg.value
        assert same(out, want), pieces
    msg = ctypes.create_string_buffer(512)
    bad = np.array([0.5, 1.5])
    assert fn(N, 0, 0, stream.ctypes.data, stream.size, L, 1, bad.ctypes.data_as(pd), 2, np.zeros((2, N)).ctypes.data_as(pd),
              None, None, msg, 512) == -3 and b"[0, 1]" in msg.value


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def refused(call, word):
    with pytest.raises(rpf.RPFError) as e:
        call()
    assert e.value.retval == rpf.ReturnValue.InvalidArgument and word in str(e.value), str(e.value)


def test_refusals_leave_the_store_alone():
    N, L, K = 512, 4, 10
    stream = noise("cu8", 131, N * K * L)
    out = torch.zeros((9, N), dtype=torch.float64, device=DEV)
    d = to_device(stream)
    for kw, word in ((dict(bin_stats=True), "RPF_FLAG_BIN_STATS"), (dict(pfb_taps=4), "PFB")):
        with engine(N, **kw) as ds:
            refused(lambda: ds.quantile_append_device(d.data_ptr(), stream.size, L, K, current()), word)
            refused(lambda: ds.quantile_append(stream, L), word)
            refused(lambda: ds.quantile_select_device([0.5], out.data_ptr(), current()), word)
            refused(lambda: ds.quantile_select([0.5]), word)
            assert ds.quantile_rows == 0
    with engine(N) as ds:
        assert ds.quantile_append_device(d.data_ptr(), stream.size, L, K, current()) == K
        for q in (-0.1, 1.5, float("nan")):
            refused(lambda: ds.quantile_select_device([0.5, q], out.data_ptr(), current()), "[0, 1]")
            refused(lambda: ds.quantile_select([q]), "[0, 1]")
        for q in ([], [0.1] * 9):
            refused(lambda: ds.quantile_select_device(q, out.data_ptr(), current()), "nq")
            refused(lambda: ds.quantile_select(q), "nq")
        refused(lambda: ds.quantile_select_device([0.5], out.data_ptr() + 8, current()), "16-byte")
        refused(lambda: ds.quantile_append_device(d.data_ptr(), stream.size, 0, K, current()), "at least 1")
        refused(lambda: ds.quantile_append(stream, 0, max_spectra=3), "at least 1")
        refused(lambda: ds.quantile_append_device(d.data_ptr(), stream.size, L, -1, current()), "max_spectra")
        refused(lambda: ds.quantile_append_device(d.data_ptr() + 1, stream.size - 2, L, K, current()), "aligned")
        assert ds.quantile_rows == K
        torch.cuda.synchronize()
    # over the cap, through the HOST entry: the refusal precedes any copy
    N = 8192
    with engine(N) as ds:
        cap = ds.quantile_max_rows
        assert cap == 16384
        zeros = np.zeros(2 * N * (cap + 1), dtype=np.uint8)
        refused(lambda: ds.quantile_append(zeros, 1), "at most %d rows" % cap)
        assert ds.quantile_rows == 0
        assert "raise the frames per integration or cap max_spectra" in ds._lib.rpf_last_error(ds._handle).decode()


# ---- 7. what it is for ------------------------------------------------------------------------------------------------------
BURST = dict(N=512, L=16, K=64, seed=1)


def burst_stream(N, L, K, seed):
    """Gaussian noise of sigma 20 per component around 127 and, in the integrations k with k mod 8 = 3 only, a tone of
    amplitude 60 at N/4 bins of the stream (period 4 samples), rounded to bytes."""
    rng = np.random.default_rng(seed)
    n = np.arange(K * L * N)
    x = rng.normal(127.0, 20.0, size=(n.size, 2))
    on = (n // (L * N)) % 8 == 3
    phase = 2 * np.pi * (n % 4) / 4.0
    x[:, 0] += np.where(on, 60.0 * np.cos(phase), 0.0)
    x[:, 1] += np.where(on, 60.0 * np.sin(phase), 0.0)
    return np.clip(np.rint(x), 0, 255).astype(np.uint8).reshape(-1)


def truth_rows(u, N, L, K):
    x = u.astype(np.float64).reshape(K, L, N, 2) - 127.0
    z = (x[..., 0] + 1j * x[..., 1]) * (1 - 2 * (np.arange(N) % 2))
    s = np.fft.fft(z, axis=2)
    return (s.real ** 2 + s.imag ** 2).sum(axis=1)


def burst_conditions(rows, median, N):
    mean = rows.mean(axis=0)
    clean = float(np.median(mean))
    burst = 3 * N // 4                                                        # N/4 of the stream, DC in the middle
    others = np.ones(N, dtype=bool)
    others[[burst, N // 2]] = False
    figures = (mean[burst] / clean, median[burst] / clean, float((median[others] / clean).min()),
               float((median[others] / clean).max()))
    ok = figures[0] > 100 and 0.8 <= figures[1] <= 1.25 and 0.8 <= figures[2] and figures[3] <= 1.2
    return ok, figures


def test_the_median_ignores_an_intermittent_tone():
    N, L, K, seed = (BURST[k] for k in ("N", "L", "K", "seed"))
    u = burst_stream(N, L, K, seed)
    truth = truth_rows(u, N, L, K)
    ok, figures = burst_conditions(truth, stats.quantiles(truth, [0.5])[0], N)
    print("float64 truth: burst bin mean %.1f x clean, median %.3f x, other bins' medians %.3f .. %.3f x" % figures)
    if not ok:
        pytest.skip("the float64 reference misses the conditions for seed %d: %r" % (seed, figures))
    with engine(N) as ds:
        rows, _ = ds.accumulate_series(u, L)
        median, done = ds.accumulate_quantiles(u, L)
    assert done == K
    ok, figures = burst_conditions(rows, median[0], N)
    print("engine:        burst bin mean %.1f x clean, median %.3f x, other bins' medians %.3f .. %.3f x" % figures)
    assert ok, figures


# ---- 8. CLI -----------------------------------------------------------------------------------------------------------------
def data_lines(text):
    return [ln for ln in text.split("\n") if ln.strip() and not ln.startswith("#")]


def test_cli_one_integration_prints_the_average(tmp_path):
    N, R = 512, 64
    u = synth.noise_tones_iq(141, N * R)
    path = tmp_path / "rec.cu8"
    u.tofile(str(path))
    r = subprocess.run([CLI, "-b", str(N), "--quantile", str(R), "--quantiles", "0.5", "--input", str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "# frequency [Hz] quantile 0.5 [dB/Hz]" in r.stdout.split("\n")
    assert r.stdout.count("# rtl-power-fftw output") == 1
    assert "Quantiles: 1 of 1 integrations of %d frames (one launch per piece)" % R in r.stderr
    p = subprocess.run([CLI, "-b", str(N), "-n", str(R), "-q", "--input", str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    a, b = data_lines(r.stdout), data_lines(p.stdout)
    assert len(a) == len(b) == N
    if a != b:      # another geometry: every printed value within its last printed digit
        for la, lb in zip(a, b):
            fa, fb = la.split(), lb.split()
            assert fa[0] == fb[0]
            digits = len(fa[1].split(".")[1]) if "." in fa[1] else 0
            assert abs(round((float(fa[1]) - float(fb[1])) * 10 ** digits)) <= 1


def test_cli_three_quantiles_are_three_columns(tmp_path):
    N, L, K, rate = 512, 8, 9, 2000000
    u = synth.noise_tones_iq(151, N * (K * L + 2))
    path = tmp_path / "rec.cu8"
    u.tofile(str(path))
    r = subprocess.run([CLI, "-b", str(N), "--quantile", str(L), "--quantiles", "0.1,0.5,0.9", "-l", "--input", str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "# frequency [Hz] quantile 0.1 [dB/Hz] quantile 0.5 [dB/Hz] quantile 0.9 [dB/Hz]" in r.stdout.split("\n")
    assert r.stdout.count("# rtl-power-fftw output") == 1                 # one block for the file
    assert "Quantiles: 3 of %d integrations of %d frames" % (K, L) in r.stderr
    cols = [ln.split() for ln in data_lines(r.stdout)]
    assert len(cols) == N and all(len(x) == 4 for x in cols)
    with engine(N) as ds:
        planes, done = ds.accumulate_quantiles(u, L, [0.1, 0.5, 0.9])
    assert done == K
    for c in range(3):
        col = planes[c] / L
        col[N // 2] = (col[N // 2 - 1] + col[N // 2 + 1]) / 2
        want = col / N / rate
        for i, x in enumerate(cols):
            assert abs(float(x[1 + c]) - want[i]) <= 1e-5 * abs(want[i])      # six significant digits printed
    assert all(float(x[1]) <= float(x[2]) <= float(x[3]) for x in cols)
