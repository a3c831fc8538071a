"""The excised average on the MI355X: rpf_accumulate_device_excised / rpf_accumulate_excised / rpf_power --excise.

The reference is stats.excise (the numpy statement of the definition in include/rpf_engine.h) on the rows
rpf_accumulate_device_series_stats of THE SAME ENGINE writes for the same stream: mask and kept are compared exactly --
any mismatch is a defect in the kernels' arithmetic --, clean and total within ADDITIVITY of the bin's total.  Every
threshold is imported from excise_bars; each test prints the figures it judged."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, stats, synth
from helpers import ROOT
from excise_bars import ADDITIVITY, NEIGHBOUR_SPREAD, NOISE_FLAGGED_SHARE_CAP, TOTAL_EXCESS_ABOVE
from test_excise import err_over_total

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
INF = float("inf")


def engine(N, fmt="cu8", step=None, window=False, flags=0, bin_stats=True, **kw):
    w = synth.hann_window(N) if window else None
    return rpf.Datastore(rpf.Params(N=N, window=window, frame_step=step, sample_format=fmt, bin_stats=bin_stats, **kw), w,
                         flags=flags)


def noise(fmt, seed, nsamples):
    return synth.noise_tones_iq(seed, nsamples) if fmt == "cu8" else synth.noise_tones_cs16(seed, nsamples)


def to_device(stream):
    return torch.from_numpy(np.ascontiguousarray(stream)).to(DEV)


def series_rows(ds, d_stream, nbytes, L, K):
    """The engine's own rows: (K, 3, N) from rpf_accumulate_device_series_stats, and its transform launches."""
    out = torch.full((K, 3, ds.params.N), -1.0, dtype=torch.float64, device=DEV)
    done = ds.accumulate_device_series_stats(d_stream.data_ptr(), nbytes, L, K, out.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert done == K
    return out.cpu().numpy(), ds.series_launches()


def excised(ds, d_stream, nbytes, L, lo, hi, max_spectra=1 << 40, want_mask=True, mask_rows=None):
    """(out (3, N), mask (mask_rows, N) pre-filled with 7, K) of one rpf_accumulate_device_excised call."""
    N = ds.params.N
    fit = min(ds.frames_in(nbytes) // L, max_spectra)
    out = torch.full((3, N), -1.0, dtype=torch.float64, device=DEV)
    mask = torch.full((fit if mask_rows is None else mask_rows, N), 7, dtype=torch.uint8, device=DEV) if want_mask else None
    K = ds.accumulate_device_excised(d_stream.data_ptr(), nbytes, L, max_spectra, lo, hi, out.data_ptr(),
                                     mask.data_ptr() if want_mask else 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (mask.cpu().numpy() if want_mask else None), K


def check_against_rows(ds, stream, L, K, what, launches_want):
    """At stats.sk_limits(L), 3 sigma, and again at 1 sigma (with M = 2 or 3 frames SK cannot reach the 3 sigma limits, so
    only the second run takes both branches of the comparison)."""
    d = to_device(stream)
    rows, _ = series_rows(ds, d, stream.size, L, K)
    for sigma in (3.0, 1.0):
        lo, hi = stats.sk_limits(L, sigma)
        want, want_mask = stats.excise(rows, L, lo, hi)
        got, mask, done = excised(ds, d, stream.size, L, lo, hi)
        launches = ds.series_launches()
        assert done == K, (what, done)
        wrong = int(np.count_nonzero(mask != want_mask))
        e_clean, e_total = err_over_total(got[0], want[0], want[2]), err_over_total(got[2], want[2], want[2])
        print("%s: L=%d K=%d launches=%d thresholds (%.4f, %.4f): %d of %d flagged, mask unequal in %d, kept unequal in %d, "
              "clean %.3g total %.3g (bar %g)"
              % (what, L, K, launches, lo, hi, int(want_mask.sum()), want_mask.size, wrong,
                 int(np.count_nonzero(got[1] != want[1])), e_clean, e_total, ADDITIVITY))
        assert launches == launches_want, what
        assert wrong == 0 and np.array_equal(got[1], want[1]), what
        assert e_clean < ADDITIVITY and e_total < ADDITIVITY, what
    assert 0 < want_mask.sum() < want_mask.size              # at 1 sigma the case takes both branches


# ---- exactness against the engine's own rows ------------------------------------------------------------------------
# N = 64, L = 2: 32 frames per workgroup, L below it; 600 rows are cut by the series' workgroup ranges and fall into
# 600 of the 4096 row groups.  N = 8192: 32 row groups, so K = 9 leaves some of them without a row.
@pytest.mark.parametrize("N,L,K,window", [(64, 2, 600, False), (512, 64, 40, False), (4096, 3, 50, False),
                                          (8192, 16, 9, True)])
def test_mask_and_kept_are_exact_against_the_engines_rows(N, L, K, window):
    with engine(N, window=window) as ds:
        check_against_rows(ds, noise("cu8", 100 + N, N * (K * L + 1)), L, K, "N=%d%s" % (N, " hann" if window else ""), 1)


def test_cs16_at_512():
    N, L, K = 512, 5, 70
    with engine(N, "cs16") as ds:
        check_against_rows(ds, noise("cs16", 3, N * K * L), L, K, "cs16 N=%d" % N, 1)


def test_fallback_route_at_500():
    N, L, K = 500, 8, 6
    with engine(N) as ds:
        check_against_rows(ds, noise("cu8", 5, N * (K * L + 3)), L, K, "N=%d spectrum by spectrum" % N, K)


# ---- identities ---------------------------------------------------------------------------------------------------
def test_identities():
    N, L, K = 512, 4, 300
    stream = noise("cu8", 7, N * (K * L + 2))
    with engine(N) as ds:
        d = to_device(stream)
        lo, hi = stats.sk_limits(L)
        # nothing flagged: clean == total bit for bit
        out, mask, done = excised(ds, d, stream.size, L, -INF, INF)
        assert done == K and np.all(out[1] == K) and not mask.any()
        assert out[0].tobytes() == out[2].tobytes() and np.all(out[2] > 0)
        total = out[2].copy()
        # everything flagged
        out, mask, done = excised(ds, d, stream.size, L, INF, INF)
        assert done == K and np.all(mask == 1)
        assert out[0].tobytes() == np.zeros(N).tobytes() and out[1].tobytes() == np.zeros(N).tobytes()
        assert out[2].tobytes() == total.tobytes()
        # the same call twice; without a mask
        a, am, _ = excised(ds, d, stream.size, L, lo, hi)
        b, bm, _ = excised(ds, d, stream.size, L, lo, hi)
        c, none, _ = excised(ds, d, stream.size, L, lo, hi, want_mask=False)
        assert a.tobytes() == b.tobytes() == c.tobytes() and np.array_equal(am, bm) and none is None
        assert a[2].tobytes() == total.tobytes()
        # a quota below F / L: the mask rows from K on keep the sentinel
        q, qm, done = excised(ds, d, stream.size, L, lo, hi, max_spectra=K - 5, mask_rows=K)
        assert done == K - 5 and np.all(qm[K - 5:] == 7) and np.array_equal(qm[:K - 5], am[:K - 5])
        assert np.array_equal(q[1], (am[:K - 5] == 0).sum(axis=0))
        # K = 0: zeros, nothing launched
        z, zm, done = excised(ds, d, stream.size, L, lo, hi, max_spectra=0, mask_rows=2)
        assert done == 0 and not z.any() and np.all(zm == 7) and ds.series_launches() == 0
        print("identities: N=%d L=%d K=%d, %d of %d flagged at 3 sigma" % (N, L, K, int(am.sum()), am.size))


# ---- several pieces -----------------------------------------------------------------------------------------------
def test_several_pieces_host_route_against_device_route():
    """N = 8192, cs16, L = 2: a row is 192 KB, so 64 MB of rows is 341 of them and K = 1100 takes four pieces; the
    stream is 72 MB, more than one 64 MB piece of input."""
    N, L, K = 8192, 2, 1100
    stream = np.random.default_rng(11).integers(0, 256, size=4 * N * K * L, dtype=np.uint8)      # (uniform 16-bit noise)
    assert stream.size > (64 << 20) and K * 3 * N * 8 > 3 * (64 << 20)
    lo, hi = stats.sk_limits(L, 1.0)                      # (M = 2: at 1 sigma a good share of the pairs is flagged)
    with engine(N, "cs16") as ds:
        before = ds.pwr.copy(), ds.sum_sq.copy(), ds.peak.copy(), ds.repeats_done
        host, hmask, hk = ds.accumulate_excised(stream, L, lo, hi, want_mask=True)
        host_launches = ds.series_launches()
        assert np.array_equal(ds.pwr, before[0]) and np.array_equal(ds.sum_sq, before[1])
        assert np.array_equal(ds.peak, before[2]) and ds.repeats_done == before[3]
        d = to_device(stream)
        dev, dmask, dk = excised(ds, d, stream.size, L, lo, hi)
        dev_launches = ds.series_launches()
        nomask, none, _ = ds.accumulate_excised(stream, L, lo, hi)
    assert hk == dk == K and hmask.shape == (K, N)
    e_clean, e_total = err_over_total(host[0], dev[0], dev[2]), err_over_total(host[2], dev[2], dev[2])
    print("several pieces: launches host %d device %d, %d of %d flagged, host vs device clean %.3g total %.3g (bar %g)"
          % (host_launches, dev_launches, int(dmask.sum()), dmask.size, e_clean, e_total, ADDITIVITY))
    assert host_launches == dev_launches == 4
    assert np.array_equal(hmask, dmask) and np.array_equal(host[1], dev[1])
    assert e_clean < ADDITIVITY and e_total < ADDITIVITY
    assert 0 < dmask.sum() < dmask.size
    assert none is None and nomask.tobytes() == host.tobytes()


# ---- it takes the interference out of the average --------------------------------------------------------------------
def burst_stream(N, L, K, hit, input_bin, seed):
    """8-bit Gaussian noise (sigma 20 about 127) and a carrier of amplitude 30 on `input_bin` in every eighth frame of the
    integrations `hit` only; rounded, clipped to 0 .. 255."""
    rng = np.random.default_rng(seed)
    F = K * L
    x = rng.normal(127.0, 20.0, size=(F, N, 2))
    carrier = 30.0 * np.exp(2j * np.pi * input_bin * np.arange(N) / N)
    frames = np.arange(F)
    on = np.isin(frames // L, hit) & (frames % 8 == 5)
    x[on, :, 0] += carrier.real
    x[on, :, 1] += carrier.imag
    return np.clip(np.rint(x), 0, 255).astype(np.uint8).reshape(-1)


DETECTION = dict(N=512, L=64, K=24, hit=(7, 16), input_bin=100, seed=3)


def truth_rows(u, N, L, K):
    """(K, 3, N) rows of the stream in float64: the unpack the header defines, numpy's FFT."""
    sign = (1 - 2 * (np.arange(N) % 2)).astype(np.float64)
    x = (u.astype(np.float64).reshape(K * L, N, 2) - 127.0) * sign[None, :, None]
    p = np.abs(np.fft.fft(x[..., 0] + 1j * x[..., 1], axis=1)) ** 2
    g = p.reshape(K, L, N)
    return np.stack([g.sum(axis=1), (g * g).sum(axis=1), g.max(axis=1)], axis=1)


def judge_detection(out, mask, what):
    N, L, K, hit = DETECTION["N"], DETECTION["L"], DETECTION["K"], DETECTION["hit"]
    b = DETECTION["input_bin"] + N // 2                                   # (the (-1)^n shift)
    clean, kept, total = out
    noise_bins = np.array([i for i in range(N) if i not in (b, N // 2)])
    clean_mean = clean / np.where(kept > 0, kept * L, 1.0)
    total_mean = total / (K * L)
    med = np.median(clean_mean[noise_bins])
    near = np.array([i for i in range(b - 16, b + 17) if i != b])
    spread = float(np.max(np.abs(clean_mean[near] / med - 1.0)))
    at_bin = float(clean_mean[b] / med - 1.0)
    excess = float(total_mean[b] / med - 1.0)
    share = float(mask[:, noise_bins].mean())
    print("%s: burst pairs flagged %s, kept[%d] = %g of %d; clean mean there %+.4f of the median, neighbours within %.4f "
          "(bar %g); unexcised %+.3f (above %g); noise pairs flagged %.4f (cap %g)"
          % (what, [int(mask[k, b]) for k in hit], b, kept[b], K, at_bin, spread, NEIGHBOUR_SPREAD, excess,
             TOTAL_EXCESS_ABOVE, share, NOISE_FLAGGED_SHARE_CAP))
    assert all(mask[k, b] == 1 for k in hit)
    assert kept[b] == K - 2
    assert spread < NEIGHBOUR_SPREAD and abs(at_bin) < NEIGHBOUR_SPREAD
    assert excess > TOTAL_EXCESS_ABOVE
    assert share <= NOISE_FLAGGED_SHARE_CAP


def test_a_burst_is_excised_from_its_bin_and_nothing_else_moves():
    N, L, K = DETECTION["N"], DETECTION["L"], DETECTION["K"]
    u = burst_stream(N, L, K, DETECTION["hit"], DETECTION["input_bin"], DETECTION["seed"])
    lo, hi = stats.sk_limits(L)
    # first the float64 truth: if it does not show the burst, the stream is wrong, not the kernel
    judge_detection(*stats.excise(truth_rows(u, N, L, K), L, lo, hi), what="float64 truth")
    with engine(N) as ds:
        out, mask, done = ds.accumulate_excised(u, L, lo, hi, want_mask=True)
        assert done == K and ds.series_launches() == 1
    judge_detection(out, mask, what="excised on the GPU")


# ---- refusals -----------------------------------------------------------------------------------------------------
def test_refusals():
    N = 512
    stream = noise("cu8", 1, N * 8)
    d = to_device(stream)
    out = torch.zeros((3, N), dtype=torch.float64, device=DEV)
    nan = float("nan")
    with engine(N, bin_stats=False) as plain:
        for call in (lambda: plain.accumulate_device_excised(d.data_ptr(), stream.size, 2, 4, 0.5, 1.5, out.data_ptr()),
                     lambda: plain.accumulate_excised(stream, 2, 0.5, 1.5)):
            with pytest.raises(rpf.RPFError) as e:
                call()
            assert e.value.retval == rpf.ReturnValue.InvalidArgument and "RPF_FLAG_BIN_STATS" in str(e.value)
    with engine(N) as ds:
        cases = (((2, 4, 0.5, 1.5, out.data_ptr() + 8), "16-byte"),
                 ((1, 4, 0.5, 1.5, out.data_ptr()), "at least 2"),
                 ((2, 4, 1.5, 0.5, out.data_ptr()), "sk_lo is above sk_hi"),
                 ((2, 4, nan, 1.5, out.data_ptr()), "NaN"),
                 ((2, 4, 0.5, nan, out.data_ptr()), "NaN"),
                 ((2, -1, 0.5, 1.5, out.data_ptr()), "max_spectra"))
        for (L, cap, lo, hi, ptr), word in cases:
            with pytest.raises(rpf.RPFError) as e:
                ds.accumulate_device_excised(d.data_ptr(), stream.size, L, cap, lo, hi, ptr)
            assert e.value.retval == rpf.ReturnValue.InvalidArgument and word in str(e.value), word
        for L, lo, hi, word in ((1, 0.5, 1.5, "at least 2"), (2, 1.5, 0.5, "sk_lo"), (2, nan, nan, "NaN")):
            with pytest.raises(rpf.RPFError) as e:
                ds.accumulate_excised(stream, L, lo, hi)
            assert e.value.retval == rpf.ReturnValue.InvalidArgument and word in str(e.value), word
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()                       # a refused call wrote nothing


def test_cpp_host_datastore_excised_calls():
    """rpf_host::Datastore::accumulate_excised / accumulate_device_excised through the test shim."""
    host = ctypes.CDLL(os.path.join(ROOT, "rtl-power-fftw_amd", "host", "librpf_host.so"))
    fn = host.rpf_host_accumulate_excised
    fn.restype = ctypes.c_longlong
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_longlong,
                   ctypes.c_longlong, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong,
                   ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_size_t]
    N, L, K = 512, 9, 40
    stream = noise("cu8", 37, N * (K * L + 3))
    lo, hi = stats.sk_limits(L)
    with engine(N) as ds:
        want, want_mask, wk = ds.accumulate_excised(stream, L, lo, hi, want_mask=True)
    msg, launches = ctypes.create_string_buffer(512), ctypes.c_int()
    out, mask = np.full((3, N), -1.0), np.full((K, N), 7, dtype=np.uint8)
    got = fn(N, 0, 0, stream.ctypes.data, stream.size, L, 1 << 40, lo, hi, out.ctypes.data, mask.ctypes.data, K, 0,
             ctypes.byref(launches), msg, 512)
    assert got == wk == K and launches.value == 1, msg.value
    assert out.tobytes() == want.tobytes() and np.array_equal(mask, want_mask)
    d = to_device(stream)
    d_out = torch.full((3, N), -1.0, dtype=torch.float64, device=DEV)
    d_mask = torch.full((K, N), 7, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    got = fn(N, 0, 0, d.data_ptr(), stream.size, L, K, lo, hi, d_out.data_ptr(), d_mask.data_ptr(), K, 1,
             ctypes.byref(launches), msg, 512)
    torch.cuda.synchronize()
    assert got == K and launches.value == 1, msg.value
    assert d_out.cpu().numpy().tobytes() == want.tobytes() and np.array_equal(d_mask.cpu().numpy(), want_mask)
    assert fn(N, 0, 0, stream.ctypes.data, stream.size, 1, 4, lo, hi, out.ctypes.data, None, K, 0, None, msg, 512) == -3
    assert b"at least 2" in msg.value


# ---- CLI -----------------------------------------------------------------------------------------------------------
def one_unit_of_the_last_digit(text):
    mant = text.lower().split("e")
    digits = len(mant[0].split(".")[1]) if "." in mant[0] else 0
    return 10.0 ** (-digits + (int(mant[1]) if len(mant) > 1 else 0))


@pytest.mark.parametrize("linear", [False, True])
def test_cli_excise_prints_one_block(tmp_path, linear):
    N, L, K, rate = 512, 64, DETECTION["K"], 2000000
    u = burst_stream(N, L, K, DETECTION["hit"], DETECTION["input_bin"], DETECTION["seed"])
    path = tmp_path / "rec.cu8"
    u.tofile(str(path))
    r = subprocess.run([CLI, "-b", str(N), "--excise", str(L), "--input", str(path)] + (["-l"] if linear else []),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "# frequency [Hz] power spectral density [dB/Hz] kept fraction" in r.stdout.split("\n")
    assert r.stdout.count("# rtl-power-fftw output") == 1                 # one block for the file
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.strip() and not ln.startswith("#")]
    assert len(rows) == N and all(len(x) == 3 for x in rows)
    lo, hi = stats.sk_limits(L)
    with engine(N) as ds:
        out, _, done = ds.accumulate_excised(u, L, lo, hi)
    assert done == K
    clean, kept, total = out
    mean = np.where(kept > 0, clean / np.where(kept > 0, kept * L, 1.0), total / (K * L))
    mean[N // 2] = (mean[N // 2 - 1] + mean[N // 2 + 1]) / 2
    want = mean / N / rate
    if not linear:
        want = 10 * np.log10(want)
    worst = 0.0
    for i, (f, p, frac) in enumerate(rows):
        unit = one_unit_of_the_last_digit(p)
        worst = max(worst, abs(float(p) - want[i]) / unit)
        assert abs(float(p) - want[i]) <= unit * (0.5 + 1e-6), (i, p, want[i])           # the printed rounding
        assert abs(float(frac) - kept[i] / K) <= 0.5e-6 * 1.000001 + 1e-12, (i, frac)
    summary = [ln for ln in r.stderr.splitlines() if ln.startswith("Excised:")]
    assert len(summary) == 1
    flagged = int(K * N - kept.sum())
    assert ("%d of %d (integration, bin) pairs flagged" % (flagged, K * N)) in summary[0]
    print("%s: worst difference %.3g units of the last printed digit; %s" % ("-l" if linear else "dB", worst, summary[0]))
