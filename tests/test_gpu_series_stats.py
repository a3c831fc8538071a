"""Time-resolved per-bin statistics on the MI355X: rpf_accumulate_device_series_stats / rpf_accumulate_series_stats /
rpf_power --series-stats.

The reference of every row is rpf_accumulate_device_stats run BY THE SAME ENGINE on that row's slice of the stream: the
same arithmetic on the same frames, the double additions grouped differently -- S1 and S2 within ADDITIVITY, PK (a
maximum: no grouping) equal; on the spectrum-by-spectrum route all three planes are equal bit for bit.  Identities that
hold for any grid are asserted exactly.  Every threshold is imported from series_stats_bars; each test prints the figures it
judged."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, stats, synth
from helpers import ROOT, max_rel
from series_stats_bars import ADDITIVITY, SAME_KERNELS, SK_BURST_ABOVE, SK_NOISE_RANGE_M64

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
NO_DMA = _lib.FLAG_NO_LDS_DMA

CASES = [(64, False), (512, False), (4096, False), (4096, True), (8192, False)]


def engine(N, fmt="cu8", step=None, window=False, flags=0, bin_stats=True, **kw):
    w = synth.hann_window(N) if window else None
    return rpf.Datastore(rpf.Params(N=N, window=window, frame_step=step, sample_format=fmt, bin_stats=bin_stats, **kw), w,
                         flags=flags)


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)


def to_device(stream, misalign=0):
    t = torch.empty(stream.size + 64, dtype=torch.uint8, device=DEV)
    t[misalign:misalign + stream.size].copy_(torch.from_numpy(np.ascontiguousarray(stream)))
    return t, t.data_ptr() + misalign


def series_run(ds, stream, L, max_spectra=1 << 40, misalign=0, extra_rows=2):
    """(rows (K + extra_rows, planes, N) with the extra ones still -1, K, launches, (grid, fpw)) of one device series
    call: rpf_accumulate_device_series_stats on a stats engine (3 planes), rpf_accumulate_device_series on a plain one."""
    N = ds.params.N
    planes = 3 if ds.has_bin_stats else 1
    fit = ds.frames_in(stream.size) // L
    keep, ptr = to_device(stream, misalign)
    out = torch.full((max(min(fit, max_spectra), 0) + extra_rows, planes, N), -1.0, dtype=torch.float64, device=DEV)
    call = ds.accumulate_device_series_stats if planes == 3 else ds.accumulate_device_series
    K = call(ptr, stream.size, L, max_spectra, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del keep
    li = ds.launch_info()
    return out.cpu().numpy(), K, ds.series_launches(), (li["grid"], li["frames_per_wg"])


def slice_rows(ds, stream, L, K, misalign=0):
    """Row k = rpf_accumulate_device_stats of the same engine on the frames [k L, (k + 1) L): K enqueues, one synchronise."""
    N, b, S = ds.params.N, ds.sample_bytes, ds.params.frame_step
    keep, ptr = to_device(stream, misalign)
    out = torch.full((K, 3, N), -2.0, dtype=torch.float64, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    span = ds.frame_span(L)
    for k in range(K):
        assert ds.accumulate_device_stats(ptr + k * L * b * S, span, L, out.data_ptr() + 8 * 3 * N * k, s) == L
    torch.cuda.synchronize()
    del keep
    return out.cpu().numpy()


def geometry(ds):
    """(resident grid of the series kernel, frames per workgroup): from a launch with more iterations than any grid."""
    N, b = ds.params.N, ds.sample_bytes
    fpw = ds.launch_info()["frames_per_wg"]
    probe = np.zeros(4096 * fpw * b * N // (8 if N >= 4096 else 1), dtype=np.uint8)
    _, K, launches, (grid, fpw2) = series_run(ds, probe, fpw)
    assert launches == 1 and fpw2 == fpw and K > grid
    return grid, fpw


def check_rows(ds, stream, L, what, misalign=0, max_spectra=1 << 40):
    F = ds.frames_in(stream.size)
    K = min(F // L, max_spectra)
    rows, done, launches, geom = series_run(ds, stream, L, max_spectra, misalign)
    assert done == K and launches == (1 if K else 0), (what, done, K, launches)
    assert np.all(rows[K:] == -1.0), "%s: rows >= K were touched" % what
    want = slice_rows(ds, stream, L, K, misalign)
    e1 = max_rel(rows[:K, 0], want[:, 0]) if K else 0.0
    e2 = max_rel(rows[:K, 1], want[:, 1]) if K else 0.0
    pk_differ = int(np.count_nonzero(rows[:K, 2] != want[:, 2]))
    print("%s: L=%d K=%d frames=%d geometry=%s vs slices: S1 %.3g S2 %.3g (bar %g), PK unequal in %d of %d"
          % (what, L, K, F, geom, e1, e2, ADDITIVITY, pk_differ, K * ds.params.N))
    assert e1 < ADDITIVITY and e2 < ADDITIVITY, what
    assert pk_differ == 0, what
    return rows[:K]


# ---- identities that hold for any grid --------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,window", CASES)
def test_one_frame_rows_are_exact(N, window):
    """L = 1: the peak of one frame is its power and S2 its square, bit for bit, whichever workgroup and slot held it."""
    K = 700
    with engine(N, window=window) as ds:
        rows, done, launches, geom = series_run(ds, random_bytes(41, 2 * N * K), 1)
    assert done == K and launches == 1
    assert np.all(rows[K:] == -1.0)
    s1, s2, pk = rows[:K, 0], rows[:K, 1], rows[:K, 2]
    print("N=%d%s geometry=%s: S1 %.3g .. %.3g" % (N, " hann" if window else "", geom, s1.min(), s1.max()))
    assert np.array_equal(pk, s1) and np.array_equal(s2, s1 * s1)
    assert np.all(s1[:, np.arange(N) != N // 2] > 0)


@pytest.mark.parametrize("N,window", CASES)
def test_peak_of_halves(N, window):
    with engine(N, window=window) as ds:
        G, fpw = geometry(ds)
        L, K = 2 * (fpw + 1), (G if N < 8192 else G // 4) // 2 + 3
        stream = random_bytes(43, 2 * N * (K * L + 1))
        whole, kw, lw, _ = series_run(ds, stream, L, extra_rows=0)
        half, kh, lh, _ = series_run(ds, stream, L // 2, extra_rows=0)
    assert kw == K and kh == 2 * K and lw == lh == 1
    assert np.array_equal(whole[:, 2], np.maximum(half[0::2, 2], half[1::2, 2]))
    e1 = max_rel(whole[:, 0], half[0::2, 0] + half[1::2, 0])
    e2 = max_rel(whole[:, 1], half[0::2, 1] + half[1::2, 1])
    print("N=%d%s L=%d K=%d: S1 %.3g S2 %.3g of the halves' sums (bar %g)" % (N, " hann" if window else "", L, K, e1, e2, ADDITIVITY))
    assert e1 < ADDITIVITY and e2 < ADDITIVITY


# ---- every plane against rpf_accumulate_device_stats on the slices -------------------------------------------------------

@pytest.mark.parametrize("N,window", CASES)
def test_planes_equal_the_slices(N, window):
    with engine(N, window=window) as ds:
        G, fpw = geometry(ds)
        plan = [                                   # (L, K, tail frames): test_gpu_series.py's plan
            (1, 700, 0),
            (fpw, 3 * G + 7, 0),
            (fpw + 1, G + G // 2 + 3, fpw),
            (3 * fpw + 1, G // 2 + 3, 3 * fpw),
            (40 * fpw, 13, 40 * fpw - 1),          # each spectrum spans many workgroups: the fix-up's maximum
            (3 * fpw + 1, 5, 0),
        ]
        if fpw > 1:
            plan.append((fpw - 1, 2 * G + 5, fpw - 2))
        if N == 8192:
            plan[1] = (fpw, G + 7, 0)
            plan[2] = (fpw + 1, G // 2 + 3, fpw)
        for i, (L, K, tail) in enumerate(plan):
            stream = random_bytes(100 + i, 2 * N * (K * L + tail))
            check_rows(ds, stream, L, "N=%d%s" % (N, " hann" if window else ""))


@pytest.mark.parametrize("N,window", CASES)
def test_s1_plane_is_the_plain_series(N, window):
    with engine(N, window=window) as st, engine(N, window=window, bin_stats=False) as plain:
        G, fpw = geometry(st)
        L, K = 3 * fpw + 1, (G if N < 8192 else G // 4) // 2 + 3
        stream = random_bytes(47, 2 * N * K * L)
        got, kg, lg, gg = series_run(st, stream, L)
        want, kp, lp, gp = series_run(plain, stream, L)
    assert kg == kp == K and lg == lp == 1
    if gg == gp:
        print("N=%d%s: same geometry %s -> array_equal" % (N, " hann" if window else "", gg))
        assert np.array_equal(got[:K, 0], want[:K, 0])
    else:
        err = max_rel(got[:K, 0], want[:K, 0])
        print("N=%d%s: geometry %s vs %s -> ADDITIVITY, measured %.3g" % (N, " hann" if window else "", gg, gp, err))
        assert err < ADDITIVITY


# ---- formats and staging -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,window", [(512, False), (4096, True)])
def test_cs8_equals_cu8_and_cs16_runs(N, window):
    with engine(N, "cu8", window=window) as a, engine(N, "cs8", window=window) as b, engine(N, "cs16", window=window) as c:
        G, fpw = geometry(a)
        L, K = 2 * fpw + 1, G + 3
        u = np.minimum(random_bytes(11, 2 * N * K * L), 254).astype(np.uint8)
        s8 = synth.to_cs8(u)
        ra, ka, la, ga = series_run(a, u, L)
        rb, kb, lb, gb = series_run(b, s8, L)
        assert ka == kb == K and la == lb == 1
        assert ga == gb, "cs8 shares cu8's staging: same launch geometry"
        assert np.array_equal(ra, rb), "cs8 vs cu8"
        if N == 4096:
            check_rows(c, synth.to_cs16(s8), L, "cs16 N=%d" % N)


@pytest.mark.parametrize("N,window", [(64, False), (4096, True)])
def test_vgpr_staging_and_a_misaligned_stream(N, window):
    for flags, misalign in ((NO_DMA, 0), (0, 2)):
        with engine(N, window=window, flags=flags) as ds:
            G, fpw = geometry(ds)
            L, K = fpw + 1, G + 11
            check_rows(ds, random_bytes(8, 2 * N * (K * L + 1)), L, "N=%d flags=%d misalign=%d" % (N, flags, misalign),
                       misalign=misalign)


def test_two_runs_are_byte_identical_and_the_quota_holds():
    N = 512
    with engine(N) as ds:
        G, fpw = geometry(ds)
        L, K = fpw + 1, G + 9
        stream = random_bytes(3, 2 * N * K * L)
        r1, k1, _, _ = series_run(ds, stream, L)
        r2, k2, _, _ = series_run(ds, stream, L)
        assert k1 == k2 == K and r1.tobytes() == r2.tobytes()
        part = check_rows(ds, stream, L, "quota K-2", max_spectra=K - 2)          # (asserts rows K-2, K-1 are still -1)
        assert part.shape[0] == K - 2
        assert np.array_equal(part[:, 2], r1[:K - 2, 2])                           # (another partition of the same frames)
        assert max_rel(part[:, :2], r1[:K - 2, :2]) < ADDITIVITY
        rows, done, launches, _ = series_run(ds, stream, L, 0)
        assert done == 0 and launches == 0 and np.all(rows == -1.0)                # K = 0: nothing launched


# ---- the spectrum-by-spectrum route --------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,step,flags", [(5000, None, 0), (4096, 4096 // 2 + 1, 0), (4096, None, _lib.FLAG_CATCH_ALL)])
def test_fallback_is_the_stats_path_bit_for_bit(N, step, flags):
    with engine(N, step=step, flags=flags) as ds:
        L, K = 5, 9
        stream = random_bytes(17, ds.frame_span(K * L + L - 1))
        rows, done, launches, _ = series_run(ds, stream, L)
        assert done == K and launches == K
        assert np.all(rows[K:] == -1.0)
        want = slice_rows(ds, stream, L, K)
        assert np.array_equal(rows[:K], want)
        host, hk = ds.accumulate_series_stats(stream, L)
        assert hk == K and ds.series_launches() == K and host.shape == (K, 3, N) and np.array_equal(host, want)


def test_host_entry_equals_the_device_entry_and_leaves_the_engine_alone():
    N = 4096
    with engine(N) as ds:
        G, fpw = geometry(ds)
        L, K = 3 * fpw + 1, G // 2 + 3
        stream = random_bytes(19, 2 * N * (K * L + 2))
        dev, dk, _, _ = series_run(ds, stream, L, extra_rows=0)
        before = ds.pwr.copy(), ds.sum_sq.copy(), ds.peak.copy(), ds.repeats_done
        host, hk = ds.accumulate_series_stats(stream, L)
        assert hk == dk == K and ds.series_launches() == 1
        err = max_rel(host[:, :2], dev[:, :2])                           # one piece: the same launch on the same bytes
        print("host path vs device entry, one piece: S1, S2 %.3g (bar %g)" % (err, SAME_KERNELS))
        assert err < SAME_KERNELS and np.array_equal(host[:, 2], dev[:, 2])
        capped, ck = ds.accumulate_series_stats(stream, L, max_spectra=3)
        assert ck == 3 and capped.shape == (3, 3, N)
        assert np.array_equal(ds.pwr, before[0]) and np.array_equal(ds.sum_sq, before[1])
        assert np.array_equal(ds.peak, before[2]) and ds.repeats_done == before[3]
        sk = stats.spectral_kurtosis(host[:, 0], host[:, 1], L)
        assert sk.shape == (K, N) and np.all(np.isfinite(sk[:, np.arange(N) != N // 2]))


def test_cpp_host_datastore_series_stats_calls():
    """rpf_host::Datastore::accumulate_series_stats / accumulate_device_series_stats through the test shim."""
    host = ctypes.CDLL(os.path.join(ROOT, "rtl-power-fftw_amd", "host", "librpf_host.so"))
    fn = host.rpf_host_accumulate_series_stats
    fn.restype = ctypes.c_longlong
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_longlong,
                   ctypes.c_longlong, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                   ctypes.c_char_p, ctypes.c_size_t]
    N, L, K = 512, 9, 40
    stream = random_bytes(37, 2 * N * (K * L + 3))
    with engine(N) as ds:
        want, wk = ds.accumulate_series_stats(stream, L)
    msg, launches = ctypes.create_string_buffer(512), ctypes.c_int()
    out = np.full((K + 1, 3, N), -1.0)
    got = fn(N, 0, 0, stream.ctypes.data, stream.size, L, 1 << 40, out.ctypes.data, K, 0, ctypes.byref(launches), msg, 512)
    assert got == wk == K and launches.value == 1, msg.value
    assert np.array_equal(out[:K], want) and np.all(out[K] == -1.0)
    keep, ptr = to_device(stream)
    d_out = torch.full((K + 1, 3, N), -1.0, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    got = fn(N, 0, 0, ptr, stream.size, L, K - 1, d_out.data_ptr(), K, 1, ctypes.byref(launches), msg, 512)
    torch.cuda.synchronize()
    rows = d_out.cpu().numpy()
    assert got == K - 1 and launches.value == 1, msg.value
    assert np.array_equal(rows[:K - 1, 2], want[:K - 1, 2]) and max_rel(rows[:K - 1, :2], want[:K - 1, :2]) < ADDITIVITY
    assert np.all(rows[K - 1:] == -1.0)
    assert fn(N, 0, 0, stream.ctypes.data, stream.size, 0, 4, out.ctypes.data, K, 0, None, msg, 512) == -3
    assert b"frames_per_spectrum" in msg.value


# ---- refusals ------------------------------------------------------------------------------------------------------------

def test_refusals():
    N = 512
    stream = random_bytes(1, 2 * N * 8)
    keep, ptr = to_device(stream)
    out = torch.zeros((5, 3, N), dtype=torch.float64, device=DEV)
    with engine(N, bin_stats=False) as plain:
        for call in (lambda: plain.accumulate_device_series_stats(ptr, stream.size, 2, 4, out.data_ptr()),
                     lambda: plain.accumulate_series_stats(stream, 2)):
            with pytest.raises(rpf.RPFError) as e:
                call()
            assert e.value.retval == rpf.ReturnValue.InvalidArgument and "RPF_FLAG_BIN_STATS" in str(e.value)
    with engine(N) as ds:
        for args, word in (((ptr, stream.size, 0, 4, out.data_ptr()), "frames_per_spectrum"),
                           ((ptr, stream.size, 2, -1, out.data_ptr()), "max_spectra"),
                           ((ptr + 1, stream.size - 2, 2, 4, out.data_ptr()), "aligned"),
                           ((ptr, stream.size, 2, 4, out.data_ptr() + 8), "16-byte")):
            with pytest.raises(rpf.RPFError) as e:
                ds.accumulate_device_series_stats(*args)
            assert e.value.retval == rpf.ReturnValue.InvalidArgument and word in str(e.value), word
        for L, cap, word in ((0, 4, "frames_per_spectrum"), (2, -1, "max_spectra")):
            with pytest.raises(rpf.RPFError) as e:
                ds.accumulate_series_stats(stream, L, max_spectra=cap)
            assert e.value.retval == rpf.ReturnValue.InvalidArgument and word in str(e.value), word


# ---- it places the interference in time -----------------------------------------------------------------------------------

def burst_stream(N, L, K, rows, input_bin):
    """8-bit Gaussian noise (sigma 20 about 127) and a carrier of amplitude 30 on `input_bin` in every eighth frame of the
    spectra `rows` only; rounded, clipped to 0 .. 255."""
    rng = np.random.default_rng(9)
    n = np.arange(N)
    F = K * L
    noise = rng.normal(0.0, 20.0, size=(F, N, 2))
    burst = 30.0 * np.exp(2j * np.pi * input_bin * n / N)
    f = np.arange(F)
    on = (np.isin(f // L, rows) & (f % 8 == 3)).astype(np.float64)
    z = on[:, None] * burst[None, :]
    x = noise + np.stack([z.real, z.imag], axis=-1) + 127.0
    return np.clip(np.rint(x), 0, 255).astype(np.uint8).reshape(-1)


def test_a_burst_is_found_in_its_rows_and_nowhere_else():
    N, L, K, hit, input_bin = 512, 64, 24, (7, 16), 100
    out_bin = input_bin + N // 2                                          # (the (-1)^n shift)
    u = burst_stream(N, L, K, hit, input_bin)
    quiet = np.array([k for k in range(K) if k not in hit])

    def check(sk, what):
        col = sk[:, out_bin]
        print("%s: SK of bin %d in the burst rows %s, in the others %.3f .. %.3f (range %s, burst above %g)"
              % (what, out_bin, col[list(hit)].round(3).tolist(), col[quiet].min(), col[quiet].max(), SK_NOISE_RANGE_M64,
                 SK_BURST_ABOVE))
        assert np.all(col[list(hit)] > SK_BURST_ABOVE)
        assert np.all(col[quiet] >= SK_NOISE_RANGE_M64[0]) and np.all(col[quiet] <= SK_NOISE_RANGE_M64[1])

    # first the float64 truth: if it does not show the burst, the stream is wrong, not the kernel
    sign = (1 - 2 * (np.arange(N) % 2)).astype(np.float32)
    x = (u.astype(np.float32).reshape(K * L, N, 2) - np.float32(127.0)) * sign[None, :, None]
    p = np.abs(np.fft.fft(x[..., 0].astype(np.float64) + 1j * x[..., 1].astype(np.float64), axis=1)) ** 2
    g = p.reshape(K, L, N)
    check(stats.spectral_kurtosis(g.sum(axis=1), (g * g).sum(axis=1), L), "float64 truth")

    with engine(N) as ds:
        rows, done = ds.accumulate_series_stats(u, L)
        assert done == K and ds.series_launches() == 1
    check(stats.spectral_kurtosis(rows[:, 0], rows[:, 1], L), "series of statistics")


# ---- CLI -----------------------------------------------------------------------------------------------------------------

def blocks_of(text):
    """The text output as blocks of token rows; comment lines (timestamps) dropped."""
    blocks, cur = [], []
    for line in text.splitlines():
        if line.startswith("#"):
            continue
        if line.strip():
            cur.append(line.split())
        elif cur:
            blocks.append(cur)
            cur = []
    if cur:
        blocks.append(cur)
    return blocks


def one_unit_of_the_last_digit(text):
    mant = text.lower().split("e")
    digits = len(mant[0].split(".")[1]) if "." in mant[0] else 0
    return 10.0 ** (-digits + (int(mant[1]) if len(mant) > 1 else 0))


@pytest.mark.parametrize("fmt,window", [("cu8", False), ("cs16", True)])
def test_cli_series_stats_matches_stats_in_continue_mode(tmp_path, fmt, window):
    N, L, K = 512, 16, 12
    b = _lib.SAMPLE_BYTES[fmt]
    assert (L * b * N) % 16384 == 0            # -c reads whole 16384-byte transfers: its integrations are then contiguous
    stream = synth.noise_tones_iq(31, N * K * L) if fmt == "cu8" else synth.noise_tones_cs16(31, N * K * L)
    path = tmp_path / "rec.bin"
    stream.tofile(str(path))
    extra = ["--format", fmt] if fmt != "cu8" else []
    if window:
        wpath = tmp_path / "hann.txt"
        wpath.write_text("\n".join("%.9g" % v for v in synth.hann_window(N)) + "\n")
        extra += ["-w", str(wpath)]
    common = [CLI, "-b", str(N), "-q", "--input", str(path)] + extra
    a = subprocess.run(common + ["--series-stats", str(L)], capture_output=True, text=True)
    r = subprocess.run(common + ["--stats", "-c", "-n", str(L)], capture_output=True, text=True)
    assert a.returncode == 0, a.stderr
    assert r.returncode == 0, r.stderr
    assert "# frequency [Hz] power spectral density [dB/Hz] peak hold [dB/Hz] spectral kurtosis" in a.stdout.split("\n")
    got, want = blocks_of(a.stdout), blocks_of(r.stdout)
    assert len(got) == len(want) == K
    worst = 0.0
    for g, w in zip(got, want):
        assert len(g) == len(w) == N
        assert [x[0] for x in g] == [x[0] for x in w]                    # the frequency column
        for rg, rw in zip(g, w):
            assert len(rg) == len(rw) == 4
            for vg, vw in zip(rg[1:], rw[1:]):                           # power, peak hold, spectral kurtosis
                unit = max(one_unit_of_the_last_digit(vg), one_unit_of_the_last_digit(vw))
                worst = max(worst, abs(float(vg) - float(vw)) / unit)
                assert abs(float(vg) - float(vw)) <= unit * (1 + 1e-9), (vg, vw)
    print("%s%s: %d blocks, worst difference %.3g units of the last printed digit" % (fmt, " -w" if window else "", K, worst))
    # --stats beside it changes nothing
    a2 = subprocess.run(common + ["--series-stats", str(L), "--stats"], capture_output=True, text=True)
    assert a2.returncode == 0 and blocks_of(a2.stdout) == got
