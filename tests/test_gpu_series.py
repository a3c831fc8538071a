"""Spectrogram mode on the MI355X: rpf_accumulate_device_series / rpf_accumulate_series / rpf_power --series.

The reference of every row is rpf_accumulate_device run BY THE SAME ENGINE on that row's slice of the stream: the same
kernels' arithmetic on the same frames, the double additions grouped differently (frame slots, workgroups) -- the bar is
ADDITIVITY; where the grouping is the same too (the spectrum-by-spectrum route, two runs of one input) rows are equal
bit for bit.  One case goes against float64 truth.  Every threshold is imported from parity_bars; each test prints the
figures it judged."""
import os
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, synth
from helpers import ROOT, max_rel, oracle_accumulate, truth_f64
from parity_bars import ADDITIVITY, SAME_KERNELS, VS_TRUTH

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
NO_DMA = _lib.FLAG_NO_LDS_DMA

CASES = [(64, False), (512, False), (4096, False), (4096, True), (8192, False)]


def engine(N, fmt="cu8", step=None, window=False, flags=0, **kw):
    w = synth.hann_window(N) if window else None
    return rpf.Datastore(rpf.Params(N=N, window=window, frame_step=step, sample_format=fmt, **kw), w, flags=flags)


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)


def to_device(stream, misalign=0):
    t = torch.empty(stream.size + 64, dtype=torch.uint8, device=DEV)
    t[misalign:misalign + stream.size].copy_(torch.from_numpy(np.ascontiguousarray(stream)))
    return t, t.data_ptr() + misalign


def series_run(ds, stream, L, max_spectra=1 << 40, misalign=0, extra_rows=2):
    """(rows incl. `extra_rows` pre-filled with -1 past the end, K, launches, (grid, fpw)) of one device series call."""
    N = ds.params.N
    fit = ds.frames_in(stream.size) // L
    keep, ptr = to_device(stream, misalign)
    out = torch.full((max(min(fit, max_spectra), 0) + extra_rows, N), -1.0, dtype=torch.float64, device=DEV)
    K = ds.accumulate_device_series(ptr, stream.size, L, max_spectra, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del keep
    li = ds.launch_info()
    return out.cpu().numpy(), K, ds.series_launches(), (li["grid"], li["frames_per_wg"])


def slice_rows(ds, stream, L, K, misalign=0):
    """Row k = rpf_accumulate_device of the same engine on the frames [k L, (k + 1) L): K enqueues, one synchronise."""
    N, b, S = ds.params.N, ds.sample_bytes, ds.params.frame_step
    keep, ptr = to_device(stream, misalign)
    out = torch.full((K, N), -2.0, dtype=torch.float64, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    span = ds.frame_span(L)
    for k in range(K):
        assert ds.accumulate_device(ptr + k * L * b * S, span, L, out.data_ptr() + 8 * N * k, s) == L
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
    err = max_rel(rows[:K], want) if K else 0.0
    print("%s: L=%d K=%d frames=%d geometry=%s max rel vs slices %.3g (bar %g)" % (what, L, K, F, geom, err, ADDITIVITY))
    assert err < ADDITIVITY, what
    return rows[:K]


# ---- every case against rpf_accumulate_device on the slices ---------------------------------------------------------------

@pytest.mark.parametrize("N,window", CASES)
def test_rows_equal_the_slices(N, window):
    with engine(N, window=window) as ds:
        G, fpw = geometry(ds)
        plan = [                                   # (L, K, tail frames): what each is there for
            (1, 700, 0),                           # many whole spectra inside a range (or, G > 700: iterations below the grid)
            (fpw, 3 * G + 7, 0),                   # whole spectra inside every range, ranges of unequal length
            (fpw + 1, G + G // 2 + 3, fpw),        # two iterations per spectrum: spectra straddle one boundary; tail L - 1
            (3 * fpw + 1, G // 2 + 3, 3 * fpw),    # four iterations per spectrum, total just above the grid; tail L - 1
            (40 * fpw, 13, 40 * fpw - 1),          # each spectrum spans many workgroups
            (3 * fpw + 1, 5, 0),                   # total iterations (20) below the grid size
        ]
        if fpw > 1:
            plan.append((fpw - 1, 2 * G + 5, fpw - 2))
        if N == 8192:                              # (the same properties on fewer bytes: 16 KB per frame)
            plan[1] = (fpw, G + 7, 0)
            plan[2] = (fpw + 1, G // 2 + 3, fpw)
        for i, (L, K, tail) in enumerate(plan):
            stream = random_bytes(100 + i, 2 * N * (K * L + tail))
            check_rows(ds, stream, L, "N=%d%s" % (N, " hann" if window else ""))


def test_quota_leaves_the_rows_past_it_alone():
    N = 512
    with engine(N) as ds:
        G, fpw = geometry(ds)
        L, K = fpw + 1, G + 9
        stream = random_bytes(3, 2 * N * K * L)
        full = check_rows(ds, stream, L, "no quota")
        part = check_rows(ds, stream, L, "quota K-2", max_spectra=K - 2)      # (asserts rows K-2, K-1 are still -1)
        assert part.shape[0] == K - 2
        print("quota vs full, shared rows: max rel %.3g" % max_rel(part, full[:K - 2]))
        assert max_rel(part, full[:K - 2]) < ADDITIVITY                        # (another partition of the same frames)
        rows, done, launches, _ = series_run(ds, stream, L, 0)
        assert done == 0 and launches == 0 and np.all(rows == -1.0)            # K = 0: nothing launched


@pytest.mark.parametrize("N", [512, 4096])
def test_loud_frames_land_in_their_rows(N):
    with engine(N) as ds:
        G, fpw = geometry(ds)
        L, K, k = 3 * fpw + 1, G // 2 + 5, G // 4 + 1
        stream = np.full(2 * N * K * L, 127, dtype=np.uint8)
        stream[::2] += random_bytes(5, stream.size // 2) % 3                   # a little noise around zero
        for f in (k * L - 1, k * L, (k + 1) * L - 1):
            stream[2 * N * f:2 * N * (f + 1)] = 255
        rows = check_rows(ds, stream, L, "loud frames")
        dc = rows[:, N // 2]
        loud = np.flatnonzero(dc > 100 * np.median(dc))
        print("DC bin: median %.3g, rows above 100x: %s (k = %d)" % (np.median(dc), loud.tolist(), k))
        assert loud.tolist() == [k - 1, k]
        assert dc[k] > 1.9 * dc[k - 1]                                         # two loud frames against one
        keep, ptr = to_device(stream)
        whole = torch.empty(N, dtype=torch.float64, device=DEV)
        assert ds.accumulate_device(ptr, stream.size, K * L, whole.data_ptr(), torch.cuda.current_stream().cuda_stream) == K * L
        torch.cuda.synchronize()
        err = max_rel(rows.sum(axis=0), whole.cpu().numpy())
        print("sum of the rows vs the whole-stream spectrum: %.3g (bar %g)" % (err, ADDITIVITY))
        assert err < ADDITIVITY


@pytest.mark.parametrize("N,window", [(64, False), (4096, True)])
def test_vgpr_staging_and_a_misaligned_stream(N, window):
    for flags, misalign in ((NO_DMA, 0), (0, 2), (NO_DMA, 2)):
        with engine(N, window=window, flags=flags) as ds:
            G, fpw = geometry(ds)
            L, K = fpw + 1, G + 11
            check_rows(ds, random_bytes(8, 2 * N * (K * L + 1)), L, "N=%d flags=%d misalign=%d" % (N, flags, misalign),
                       misalign=misalign)


@pytest.mark.parametrize("N,window", CASES)
def test_format_identities_row_by_row(N, window):
    """cs8 == cu8 on clamped streams and cs16 == cs8 on 8-bit values (test_gpu_sample_formats.py), row by row."""
    with engine(N, "cu8", window=window) as a, engine(N, "cs8", window=window) as b, engine(N, "cs16", window=window) as c:
        G, fpw = geometry(a)
        L, K = 2 * fpw + 1, (G if N < 8192 else G // 2) + 3
        u = np.minimum(random_bytes(11, 2 * N * K * L), 254).astype(np.uint8)
        s8 = synth.to_cs8(u)
        s16 = synth.to_cs16(s8)
        ra, ka, la, ga = series_run(a, u, L)
        rb, kb, lb, gb = series_run(b, s8, L)
        rc, kc, lc, gc = series_run(c, s16, L)
        assert ka == kb == kc == K and la == lb == lc == 1
        assert ga == gb, "cs8 shares cu8's staging: same launch geometry"
        assert np.array_equal(ra, rb), "cs8 vs cu8"
        if gc == gb:
            print("N=%d: cs16 geometry %s = cs8's -> array_equal" % (N, gc))
            assert np.array_equal(rc, rb)
        else:
            err = max_rel(rc[:K], rb[:K])
            print("N=%d: cs16 geometry %s vs %s -> ADDITIVITY, measured %.3g" % (N, gc, gb, err))
            assert err < ADDITIVITY
        check_rows(c, s16, L, "cs16 N=%d" % N)


@pytest.mark.parametrize("N", [512, 4096])
def test_one_spectrum_of_everything_and_determinism(N):
    with engine(N) as ds:
        F = 333
        stream = random_bytes(13, 2 * N * F + 100)
        rows = check_rows(ds, stream, F, "K = 1", max_spectra=1)
        assert rows.shape[0] == 1
        _, fpw = geometry(ds)
        r1, k1, _, _ = series_run(ds, stream, fpw + 1)
        r2, k2, _, _ = series_run(ds, stream, fpw + 1)
        assert k1 == k2 and r1.tobytes() == r2.tobytes()


# ---- the spectrum-by-spectrum route --------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,step,flags", [(5000, None, 0), (4096, 4096 // 2 + 1, 0), (4096, None, _lib.FLAG_CATCH_ALL)])
def test_fallback_is_the_single_acquisition_path_bit_for_bit(N, step, flags):
    with engine(N, step=step, flags=flags) as ds:
        L, K = 5, 9
        stream = random_bytes(17, ds.frame_span(K * L + L - 1))
        rows, done, launches, _ = series_run(ds, stream, L)
        assert done == K and launches == K
        assert np.all(rows[K:] == -1.0)
        want = slice_rows(ds, stream, L, K)
        assert np.array_equal(rows[:K], want)
        host, hk = ds.accumulate_series(stream, L)
        assert hk == K and ds.series_launches() == K and np.array_equal(host, want)


def test_stats_engine_is_refused_by_name():
    with rpf.Datastore(rpf.Params(N=512, bin_stats=True)) as ds:
        stream = random_bytes(1, 2 * 512 * 8)
        keep, ptr = to_device(stream)
        out = torch.zeros((4, 512), dtype=torch.float64, device=DEV)
        for call in (lambda: ds.accumulate_device_series(ptr, stream.size, 2, 4, out.data_ptr()),
                     lambda: ds.accumulate_series(stream, 2)):
            with pytest.raises(rpf.RPFError) as e:
                call()
            assert e.value.retval == rpf.ReturnValue.InvalidArgument and "RPF_FLAG_BIN_STATS" in str(e.value)


def test_invalid_arguments():
    with engine(512) as ds:
        stream = random_bytes(1, 2 * 512 * 8)
        keep, ptr = to_device(stream)
        out = torch.zeros((5, 512), dtype=torch.float64, device=DEV)
        for args, word in (((ptr, stream.size, 0, 4, out.data_ptr()), "frames_per_spectrum"),
                           ((ptr, stream.size, 2, -1, out.data_ptr()), "max_spectra"),
                           ((ptr + 1, stream.size - 2, 2, 4, out.data_ptr()), "aligned"),
                           ((ptr, stream.size, 2, 4, out.data_ptr() + 8), "16-byte")):
            with pytest.raises(rpf.RPFError) as e:
                ds.accumulate_device_series(*args)
            assert e.value.retval == rpf.ReturnValue.InvalidArgument and word in str(e.value), word


# ---- host path -----------------------------------------------------------------------------------------------------------

def test_host_path_one_piece_and_registered_stream():
    N = 4096
    with engine(N) as ds:
        G, fpw = geometry(ds)
        L, K = 3 * fpw + 1, G // 2 + 3
        stream = random_bytes(19, 2 * N * (K * L + 2))
        dev, dk, _, _ = series_run(ds, stream, L, extra_rows=0)
        before = ds.pwr.copy(), ds.repeats_done
        host, hk = ds.accumulate_series(stream, L)
        assert hk == dk == K and ds.series_launches() == 1
        err = max_rel(host, dev)
        print("host path vs device entry, one piece: %.3g (bar %g)" % (err, SAME_KERNELS))
        assert err < SAME_KERNELS
        capped, ck = ds.accumulate_series(stream, L, max_spectra=3)
        assert ck == 3 and max_rel(capped, dev[:3]) < ADDITIVITY
        ds.register_stream(stream)
        try:
            pinned, pk = ds.accumulate_series(stream, L)
        finally:
            ds.unregister_stream(stream)
        assert pk == K and np.array_equal(pinned, host)
        assert np.array_equal(ds.pwr, before[0]) and ds.repeats_done == before[1]      # pwr / repeats_done untouched


def test_host_path_in_several_pieces():
    """L b N > 64 MB / 3 at N = 8192: three spectra do not fit one piece, the stream goes through in two."""
    N, L, K = 8192, 1400, 3
    assert 3 * L * 2 * N > (64 << 20) >= 2 * L * 2 * N
    with engine(N) as ds:
        stream = random_bytes(23, 2 * N * K * L)
        host, hk = ds.accumulate_series(stream, L)
        assert hk == K and ds.series_launches() == 2          # one launch per piece
        dev, dk, launches, _ = series_run(ds, stream, L, extra_rows=0)
        assert dk == K and launches == 1
        err = max_rel(host, dev)
        print("host path in two pieces vs device entry: %.3g (bar %g)" % (err, ADDITIVITY))
        assert err < ADDITIVITY


def test_cpp_host_datastore_series_calls():
    """rpf_host::Datastore::accumulate_series / accumulate_device_series (host/datastore.h) through the test shim."""
    import ctypes
    host = ctypes.CDLL(os.path.join(ROOT, "rtl-power-fftw_amd", "host", "librpf_host.so"))
    fn = host.rpf_host_accumulate_series
    fn.restype = ctypes.c_longlong
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_longlong,
                   ctypes.c_longlong, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                   ctypes.c_char_p, ctypes.c_size_t]
    N, L, K = 512, 9, 40
    stream = random_bytes(37, 2 * N * (K * L + 3))
    with engine(N) as ds:
        want, wk = ds.accumulate_series(stream, L)
    msg, launches = ctypes.create_string_buffer(512), ctypes.c_int()
    out = np.full((K + 1, N), -1.0)
    got = fn(N, 0, 0, stream.ctypes.data, stream.size, L, 1 << 40, out.ctypes.data, K, 0, ctypes.byref(launches), msg, 512)
    assert got == wk == K and launches.value == 1, msg.value
    assert np.array_equal(out[:K], want) and np.all(out[K] == -1.0)
    keep, ptr = to_device(stream)
    d_out = torch.full((K + 1, N), -1.0, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    got = fn(N, 0, 0, ptr, stream.size, L, K - 1, d_out.data_ptr(), K, 1, ctypes.byref(launches), msg, 512)
    torch.cuda.synchronize()
    rows = d_out.cpu().numpy()
    assert got == K - 1 and launches.value == 1, msg.value
    assert max_rel(rows[:K - 1], want[:K - 1]) < ADDITIVITY and np.all(rows[K - 1:] == -1.0)
    assert fn(N, 0, 0, stream.ctypes.data, stream.size, 0, 4, out.ctypes.data, K, 0, None, msg, 512) == -3
    assert b"frames_per_spectrum" in msg.value


# ---- truth ---------------------------------------------------------------------------------------------------------------

def test_rows_against_float64_truth():
    N, L, K = 4096, 16, 20
    stream = synth.noise_tones_iq(29, N * K * L)
    with engine(N) as ds:
        rows, done, launches, _ = series_run(ds, stream, L, extra_rows=0)
    assert done == K and launches == 1
    worst_gpu = worst_orc = 0.0
    for k in range(K):
        sl = stream[2 * N * L * k:2 * N * L * (k + 1)]
        truth = truth_f64(N, sl, L)
        orc, _ = oracle_accumulate(N, sl, L)
        worst_orc = max(worst_orc, max_rel(orc, truth))
        worst_gpu = max(worst_gpu, max_rel(rows[k], truth))
    print("vs float64 truth over %d rows: CPU path %.3g, series %.3g (bar %g)" % (K, worst_orc, worst_gpu, VS_TRUTH))
    assert worst_orc < VS_TRUTH, "the bar is one the reference itself meets on this input"
    assert worst_gpu < VS_TRUTH


# ---- CLI -----------------------------------------------------------------------------------------------------------------

def blocks_of(text):
    """The text output as blocks of (frequency text, power text) lines; comment lines (timestamps) dropped."""
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
def test_cli_series_matches_continue_mode(tmp_path, fmt, window):
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
    a = subprocess.run(common + ["--series", str(L)], capture_output=True, text=True)
    r = subprocess.run(common + ["-c", "-n", str(L)], capture_output=True, text=True)
    assert a.returncode == 0, a.stderr
    assert r.returncode == 0, r.stderr
    got, want = blocks_of(a.stdout), blocks_of(r.stdout)
    assert len(got) == len(want) == K
    worst = 0.0
    for g, w in zip(got, want):
        assert len(g) == len(w) == N
        assert [x[0] for x in g] == [x[0] for x in w]                    # the frequency column
        for (_, pg), (_, pw) in zip(g, w):
            unit = max(one_unit_of_the_last_digit(pg), one_unit_of_the_last_digit(pw))
            worst = max(worst, abs(float(pg) - float(pw)) / unit)
            assert abs(float(pg) - float(pw)) <= unit * (1 + 1e-9), (pg, pw)
    print("%s%s: %d blocks, worst difference %.3g units of the last printed digit" % (fmt, " -w" if window else "", K, worst))
