"""Correlator of up to eight streams on the MI355X.  The definition (include/rpf_engine.h) builds the visibilities on
tested ground: V_ij is the sum over the frames of terms of the rows rpf_stft_device gives for each stream, so the main
test recomputes those terms in float64 from the device's own rows and holds V to the sum: equal as doubles for one
frame, within the derived bound 2 gamma_{F-1} sum |t| for more.  Beside it: the Hermitian layout and the symmetries,
the autos against the power path, chunk and piece seams, known answers, accuracy against float64 at the bar of
correlate_bars, what a call leaves alone, what is refused, NaN, and the CLI.  Each test prints the figures it judged."""
import os
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, correlate, stats, synth
from helpers import ROOT, dp, max_rel
import correlate_bars
import cross_bars
from test_correlate import correlate_header_titles, format_correlate_block
from test_gpu_sample_formats import device_run, to_device
from test_pfb import make_stream

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
K1_FRAMES = {64: 4099, 128: 2000, 256: 1500, 512: 1000, 1024: 700, 2048: 500, 4096: 300, 8192: 131}


def cuda_stream():
    return torch.cuda.current_stream().cuda_stream


def engine(N, fmt="cu8", flags=0, step=None, windowed=False, taps=0, **kw):
    kw.setdefault("buffers", 2)
    kw.setdefault("buf_length", 16384)
    if taps:
        kw["pfb_taps"] = taps
    return rpf.Datastore(rpf.Params(N=N, sample_format=fmt, frame_step=step, window=windowed, **kw),
                         synth.hann_window(N) if windowed else None, flags=flags)


class Resident:
    """Streams copied to the device (stream m `mis[m]` bytes past a 64-byte boundary)."""

    def __init__(self, streams, mis=None):
        mis = mis or [0] * len(streams)
        self.keep, self.ptrs = [], []
        for s, m in zip(streams, mis):
            t, p = to_device(s, m)
            self.keep.append(t)
            self.ptrs.append(p)
        self.nbytes = streams[0].size


def corr(ds, res, repeats=1 << 40, nbytes=None):
    """((M, M, 2, N) doubles, F) of one device-resident call."""
    M, N = len(res.ptrs), ds.params.N
    out = torch.empty(M * M * 2 * N, dtype=torch.float64, device=DEV)
    F = ds.correlate_device(res.ptrs, res.nbytes if nbytes is None else nbytes, repeats, out.data_ptr(), cuda_stream())
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(M, M, 2, N), F


def device_rows(ds, res, F):
    """The rows rpf_stft_device gives for every resident stream: (M, F, N, 2) float32 on the device."""
    M, N = len(res.ptrs), ds.params.N
    X = torch.empty((M, F, N, 2), dtype=torch.float32, device=DEV)
    for m in range(M):
        assert ds.stft_device(res.ptrs[m], res.nbytes, F, X[m].data_ptr(), cuda_stream()) == F
    torch.cuda.synchronize()
    return X


def terms(X, i, j):
    """(t_re, t_im), (F, N) float64 on the device: each product of float32 values is exact, each sum rounded once."""
    a, b = X[i].double(), X[j].double()
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1], a[..., 1] * b[..., 0] - a[..., 0] * b[..., 1]


def gamma(n):
    u = 2.0 ** -53
    return n * u / (1.0 - n * u)


def sums_of_terms(X):
    """(S, A): the float64 sum of the terms of every pair i <= j and the sum of their magnitudes, (M, M, 2, N) each."""
    M, N = X.shape[0], X.shape[2]
    S, A = np.zeros((M, M, 2, N)), np.zeros((M, M, 2, N))
    for i in range(M):
        for j in range(i, M):
            for c, t in enumerate(terms(X, i, j)):
                S[i, j, c] = t.sum(dim=0).cpu().numpy()
                A[i, j, c] = t.abs().sum(dim=0).cpu().numpy()
    return S, A


def check_layout(vis):
    M = vis.shape[0]
    for i in range(M):
        assert np.array_equal(vis[i, i, 1], np.zeros(vis.shape[3]))
        for j in range(i + 1, M):
            assert np.array_equal(vis[j, i, 0], vis[i, j, 0]) and np.array_equal(vis[j, i, 1], -vis[i, j, 1]), (i, j)


def check_against_rows(vis, X, F, what):
    """V against the terms of the device's own rows: equal as doubles for F = 1, within 2 gamma_{F-1} sum |t| after."""
    check_layout(vis)
    S, A = sums_of_terms(X)
    M = vis.shape[0]
    worst = 0.0
    for i in range(M):
        for j in range(i, M):
            for c in (0, 1):
                got, want, mag = vis[i, j, c], S[i, j, c], A[i, j, c]
                if F == 1:
                    assert np.array_equal(got, want), (what, i, j, c)
                    continue
                bound = 2.0 * gamma(F - 1) * mag
                assert np.all(np.abs(got - want) <= bound), (what, i, j, c, float(np.max(np.abs(got - want) - bound)))
                nz = bound > 0
                if nz.any():
                    worst = max(worst, float(np.max(np.abs(got - want)[nz] / bound[nz])))
    print("%s: F=%d, M=%d, largest |V - S| / (2 gamma_{F-1} sum |t|) %.3g" % (what, F, M, worst))


def rows_case(ds, streams, F, what, mis=None):
    res = Resident(streams, mis)
    vis, n = corr(ds, res)
    assert n == F, (n, F)
    check_against_rows(vis, device_rows(ds, res, F), F, what)
    return vis, res


def streams_of(fmt, seed, M, nsamples):
    return [make_stream(fmt, seed + 101 * m, nsamples) for m in range(M)]


# ---- 1. against the rows -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", sorted(K1_FRAMES))
def test_cu8_at_every_k1_size_against_the_rows(N):
    F = K1_FRAMES[N]
    with engine(N) as ds:
        for M in (2, 5, 8):
            vis, res = rows_case(ds, streams_of("cu8", 10 + N, M, N * F), F, "cu8 N=%d M=%d" % (N, M))
        one, n = corr(ds, res, repeats=1)                                            # F = 1 (M = 8): the terms themselves
        assert n == 1
        check_against_rows(one, device_rows(ds, res, 1), 1, "cu8 N=%d M=8, one frame" % N)


@pytest.mark.parametrize("M", range(2, 9))
def test_every_number_of_streams_at_512(M):
    N, F = 512, K1_FRAMES[512]
    with engine(N) as ds:
        rows_case(ds, streams_of("cu8", 20 + M, M, N * F), F, "cu8 N=512 M=%d" % M)


@pytest.mark.parametrize("fmt", ["cs8", "cs16", "cf32"])
@pytest.mark.parametrize("N", [512, 4096])
def test_formats_against_the_rows(fmt, N):
    F = K1_FRAMES[N]
    with engine(N, fmt) as ds:
        rows_case(ds, streams_of(fmt, 30 + N, 3, N * F), F, "%s N=%d" % (fmt, N))


def test_a_window_against_the_rows():
    N, F = 4096, K1_FRAMES[4096]
    with engine(N, "cu8", windowed=True) as ds:
        rows_case(ds, streams_of("cu8", 40, 3, N * F), F, "cu8 N=4096 hann")


def test_overlapped_frames_against_the_rows():
    N, F, S = 4096, K1_FRAMES[4096], 2048
    with engine(N, "cu8", step=S) as ds:
        rows_case(ds, streams_of("cu8", 41, 3, N + S * (F - 1)), F, "cu8 N=4096 step N/2")


def test_without_lds_dma_against_the_rows():
    N, F = 512, K1_FRAMES[512]
    with engine(N, "cu8", flags=_lib.FLAG_NO_LDS_DMA) as ds:
        rows_case(ds, streams_of("cu8", 42, 3, N * F), F, "cu8 N=512 no LDS-DMA")


def test_a_stream_at_an_odd_sample_offset_against_the_rows():
    """Stream 1 one cs16 sample (4 bytes) past a 16-byte boundary: its rows come from the VGPR staging route."""
    N, F = 512, K1_FRAMES[512]
    with engine(N, "cs16") as ds:
        rows_case(ds, streams_of("cs16", 43, 3, N * F), F, "cs16 N=512, stream 1 at an odd sample", mis=[0, 4, 0])


@pytest.mark.parametrize("N", [1 << 14, 1 << 15])
def test_the_catch_all_route_against_the_rows(N):
    """301 frames: ragged frame groups at 2^14; two chunks (256 + 45) at 2^15."""
    F = 301
    with engine(N) as ds:
        rows_case(ds, streams_of("cu8", 44, 3, N * F), F, "cu8 N=%d catch-all" % N)


def test_a_pfb_engine_against_the_rows():
    N, F, T = 512, K1_FRAMES[512], 4
    with engine(N, taps=T) as ds:
        rows_case(ds, streams_of("cu8", 45, 3, N * (F + T - 1)), F, "cu8 N=512 PFB T=4")


# ---- 2. layout and symmetry ------------------------------------------------------------------------------------------------

def test_reversing_the_streams_calling_twice_and_the_autos():
    N, F, M = 512, 1000, 5
    streams = streams_of("cu8", 50, M, N * F)
    with engine(N) as ds:
        res = Resident(streams)
        vis, n = corr(ds, res)
        again, _ = corr(ds, res)
        rev, _ = corr(ds, Resident(streams[::-1]))
        assert n == F
        check_layout(vis)
        assert np.array_equal(again.view(np.int64), vis.view(np.int64))                     # the same bits
        for i in range(M):
            for j in range(M):
                assert np.array_equal(rev[i, j], vis[M - 1 - i, M - 1 - j]), (i, j)
        one, _ = corr(ds, res, repeats=1)
        worst = 0.0
        for m in range(M):
            p1, n1, _ = device_run(ds, streams[m], repeats=1)
            pF, nF, _ = device_run(ds, streams[m])
            assert n1 == 1 and nF == F
            assert np.array_equal(one[m, m, 0], p1), m                                        # one frame: bit for bit
            worst = max(worst, max_rel(vis[m, m, 0], pF))
        print("autos over %d frames vs accumulate_device: %.3g (bar 1e-12)" % (F, worst))
        assert worst < 1e-12


# ---- 3. seams ------------------------------------------------------------------------------------------------------------------

def seam_case(N, F, cuts, seed):
    """V over F frames (M = 2) against the sum of V over the single-chunk slices [cuts[k], cuts[k + 1])."""
    streams = streams_of("cu8", seed, 2, N * F)
    with engine(N) as ds:
        res = Resident(streams)
        vis, n = corr(ds, res)
        assert n == F
        total = np.zeros_like(vis)
        for f0, f1 in zip(cuts[:-1], cuts[1:]):
            part, m = corr(ds, Resident([s[2 * N * f0:2 * N * f1] for s in streams]))
            assert m == f1 - f0
            total += part
        _, A = sums_of_terms(device_rows(ds, res, F))
        bound = 2.0 * gamma(F - 1) * A
        for i, j in ((0, 0), (0, 1), (1, 1)):
            for c in (0, 1) if i != j else (0,):
                assert np.all(np.abs(vis[i, j, c] - total[i, j, c]) <= bound[i, j, c]), (N, i, j, c)
        print("N=%d, %d frames vs the sum of %d single-chunk slices: largest |diff| / bound %.3g" %
              (N, F, len(cuts) - 1, float(np.max(np.abs(vis - total)[bound > 0] / bound[bound > 0]))))
        # a quota inside the first chunk: that slice's bits
        q = cuts[1] // 2
        part, m = corr(ds, res, repeats=q)
        head, _ = corr(ds, Resident([s[:2 * N * q] for s in streams]))
        assert m == q and np.array_equal(part, head)


def test_two_chunks_at_8192():
    seam_case(8192, 1024 + 100, [0, 1024, 1124], 60)


def test_three_chunks_at_2_20():
    seam_case(1 << 20, 2 * 8 + 3, [0, 8, 16, 19], 61)


def test_host_entry_across_pieces():
    N, F, M = 8192, 2085, 3                                        # cs16: 2048 frames a piece, then 37
    streams = streams_of("cs16", 62, M, N * F)
    with engine(N, "cs16") as ds:
        V, n = ds.correlate(streams)
        res = Resident(streams)
        vis, n0 = corr(ds, res)
        _, A = sums_of_terms(device_rows(ds, res, F))
    assert n == n0 == F
    host = np.stack([V.real, V.imag], axis=2)
    check_layout(host)
    bound = 2.0 * gamma(F - 1) * A
    iu = [(i, j) for i in range(M) for j in range(i, M)]
    for i, j in iu:
        assert np.all(np.abs(host[i, j] - vis[i, j]) <= bound[i, j]), (i, j)
    print("N=%d cs16 M=%d, %d frames: correlate in two pieces vs correlate_device, largest |diff| / bound %.3g"
          % (N, M, F, max(float(np.max(np.abs(host[i, j] - vis[i, j])[bound[i, j] > 0] / bound[i, j][bound[i, j] > 0]))
                          for i, j in iu)))


# ---- 4. known answers ---------------------------------------------------------------------------------------------------------

KNOWN = ("cu8", 512, "rect", 4)


def test_a_stream_with_itself():
    N, F = 512, 80
    a = synth.uniform_iq(70, N * F)
    with engine(N) as ds:
        vis, n = corr(ds, Resident([a, a.copy()]))
    assert n == F
    assert np.array_equal(vis[0, 1, 0], vis[0, 0, 0]) and np.array_equal(vis[0, 1, 1], np.zeros(N))
    g = stats.coherence_matrix(vis[:, :, 0] + 1j * vis[:, :, 1])
    assert np.array_equal(g[0, 1], np.ones(N))


def test_a_circular_shift_of_every_frame():
    N, F, d = 512, 80, 3
    a = synth.uniform_iq(71, N * F)
    b = np.roll(a.reshape(F, N, 2), d, axis=1).reshape(-1).copy()
    c = synth.uniform_iq(72, N * F)
    want = correlate.reference([a, b, c], N, "cu8")
    with engine(N) as ds:
        vis, n = corr(ds, Resident([a, b, c]))
    assert n == F
    V = vis[:, :, 0] + 1j * vis[:, :, 1]
    g = stats.coherence_matrix(V)
    dphi = np.angle(np.exp(1j * (np.angle(V[0, 1]) - np.angle(want[0, 1]))))
    bar = correlate_bars.BAR[KNOWN]
    print("stream 1 = every frame of stream 0 shifted by %d: |coherence - 1| %.3g, phase vs float64 %.3g rad (bar %.3g); "
          "mean coherence with the independent stream %.3f" % (d, np.max(np.abs(g[0, 1] - 1.0)), np.max(np.abs(dphi)), bar,
                                                             float(np.mean(g[0, 2]))))
    assert np.max(np.abs(g[0, 1] - 1.0)) < bar
    assert np.max(np.abs(dphi)) < bar


def test_two_streams_agree_with_the_cross_entry():
    N = 512
    a, b = cross_bars.accuracy_streams("cu8", N)
    with engine(N) as ds:
        vis, n = corr(ds, Resident([a, b]))
        ka, pa = to_device(a)
        kb, pb = to_device(b)
        out = torch.empty(4 * N, dtype=torch.float64, device=DEV)
        n2 = ds.accumulate_device_cross(pa, pb, a.size, 1 << 40, out.data_ptr(), cuda_stream())
        torch.cuda.synchronize()
        planes = out.cpu().numpy().reshape(4, N)
    assert n == n2 == cross_bars.ACCURACY_FRAMES
    m = 0.5 * (vis[0, 0, 0] + vis[1, 1, 0])
    e = float(np.max(np.abs((vis[0, 1, 0] - planes[2]) + 1j * (vis[0, 1, 1] - planes[3])) / np.maximum(m, np.median(m))))
    bar = correlate_bars.BAR[KNOWN] + cross_bars.BAR[("cu8", 512, False)]
    print("M = 2: V_01 vs Sab of accumulate_device_cross %.3g (bar %.3g)" % (e, bar))
    assert e < bar


# ---- 5. accuracy ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", correlate_bars.ACCURACY_CASES)
def test_accuracy_against_float64(case):
    fmt, N, form, M = case
    streams = correlate_bars.accuracy_streams(*case)
    want = correlate_bars.truth(streams, *case)
    with engine(N, fmt, windowed=form == "hann", taps=correlate_bars.PFB_TAPS if form == "pfb" else 0) as ds:
        vis, n = corr(ds, Resident(streams))
    assert n == correlate_bars.ACCURACY_FRAMES
    err = correlate_bars.err(vis[:, :, 0] + 1j * vis[:, :, 1], want)
    print("%s N=%d %s M=%d: V vs float64 %.3g (bar %.3g = twice the CPU float32 path's %.3g)"
          % (fmt, N, form, M, err, correlate_bars.BAR[case], correlate_bars.CPU_F32[case]))
    assert err < correlate_bars.BAR[case]


# ---- 6. the engine's state is left alone -------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["cu8", "cf32"])
def test_a_correlator_call_leaves_the_engine_alone(fmt):
    N, F, M = 512, 37, 3
    streams = streams_of(fmt, 80, M, N * F)
    with engine(N, fmt, repeats=1 << 40) as ds:
        pwr, done = ds.accumulate(streams[0])
        before, _, g_before = device_run(ds, streams[0])
        res = Resident(streams)
        first, n = corr(ds, res)
        assert n == F and done == F
        lib, held = rpf.load(), np.zeros(N)
        assert lib.rpf_get_power(ds._handle, held.ctypes.data_as(dp)) == 0
        assert np.array_equal(held, pwr) and lib.rpf_get_repeats_done(ds._handle) == F
        after, _, g_after = device_run(ds, streams[0])
        assert g_before == g_after and np.array_equal(before, after)
        V, n1 = ds.correlate(streams)
        assert n1 == F and np.array_equal(np.stack([V.real, V.imag], axis=2), first)   # one piece, one chunk: the same launches
        again, done = ds.accumulate(streams[0])
        assert done == F and max_rel(again, pwr) < 1e-13
        # a quota, and streams without a whole frame
        part, n2 = corr(ds, res, repeats=5)
        want, _ = corr(ds, Resident([s[:5 * N * ds.sample_bytes] for s in streams]))
        assert n2 == 5 and np.array_equal(part, want)
        short = ds.sample_bytes * (N - 1)
        none, n3 = corr(ds, res, nbytes=short)
        assert n3 == 0 and np.array_equal(none, np.zeros((M, M, 2, N)))
        V0, n4 = ds.correlate([s[:short] for s in streams])
        assert n4 == 0 and np.array_equal(V0, np.zeros((M, M, N)))


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------

def refused(call, part):
    with pytest.raises(rpf.RPFError) as e:
        call()
    assert e.value.retval == rpf.ReturnValue.InvalidArgument and part in str(e.value), str(e.value)


def test_refusals_launch_nothing():
    N, F, M = 512, 8, 3
    streams = streams_of("cs16", 90, M, N * F)
    res = Resident(streams)
    p, nb = res.ptrs, res.nbytes
    out = torch.zeros(9 * M * M * 2 * N + 2, dtype=torch.float64, device=DEV)
    o = out.data_ptr()
    with engine(500, "cs16") as ds:
        refused(lambda: ds.correlate_device(p, nb, F, o), "power of two")
    with engine(N, "cs16", bin_stats=True) as ds:
        refused(lambda: ds.correlate_device(p, nb, F, o), "RPF_FLAG_BIN_STATS")
        refused(lambda: ds.correlate(streams), "RPF_FLAG_BIN_STATS")
    # a kernel variant other than 0: the shipped library has none, so no such engine exists to make the call on
    with pytest.raises(rpf.RPFError):
        engine(N, "cs16", flags=1 << 8)
    with engine(N, "cs16") as ds:
        lib = _lib.load()
        assert lib.rpf_correlate_device(ds._handle, None, M, nb, F, o, None, None) == rpf.ReturnValue.InvalidArgument
        assert "NULL" in ds._lib.rpf_last_error(ds._handle).decode()
        refused(lambda: ds.correlate_device([p[0], 0, p[2]], nb, F, o), "NULL")
        refused(lambda: ds.correlate_device(p, nb, F, 0), "NULL")
        refused(lambda: ds.correlate_device(p[:1], nb, F, o), "n_streams")
        refused(lambda: ds.correlate_device(p * 3, nb, F, o), "n_streams")
        refused(lambda: ds.correlate([streams[0]]), "n_streams")
        refused(lambda: ds.correlate_device(p, nb, -1, o), "repeats")
        refused(lambda: ds.correlate_device(p, nb - 2, F, o), "multiple of the sample size")
        refused(lambda: ds.correlate([s[:nb - 2] for s in streams]), "multiple of the sample size")
        refused(lambda: ds.correlate_device([p[0], p[1] + 2, p[2]], nb - 4, F, o), "aligned")
        refused(lambda: ds.correlate_device(p, nb, F, o + 8), "16-byte aligned")
        with pytest.raises(rpf.RPFError):
            ds.correlate([streams[0], streams[1][:-4], streams[2]])                # unequal lengths
        ds.begin(4)
        refused(lambda: ds.correlate_device(p, nb, F, o), "acquisition running")
        ds.finish()
        # ... and the engine still works
        vis, n = corr(ds, res)
        assert n == F and vis[0, 0, 0].min() > 0
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0                             # nothing was launched


# ---- 8. NaN ----------------------------------------------------------------------------------------------------------------------

def test_a_nan_in_one_stream_stays_in_its_row_and_column():
    N, F, M = 512, 9, 3
    s = [synth.gaussian_cf32(100 + m, N * F) for m in range(M)]
    s[2][4 * N + 17] = np.complex64(complex(np.nan, 0.0))
    with engine(N, "cf32") as ds:
        vis, n = corr(ds, Resident([x.view(np.uint8) for x in s]))
    assert n == F
    for i in range(M):
        for j in range(M):
            nan = i == 2 or j == 2
            for c in (0, 1):
                if i == j and c == 1:
                    continue
                assert (np.isnan(vis[i, j, c]).all() if nan else np.isfinite(vis[i, j, c]).all()), (i, j, c)


# ---- 9. the CLI ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["cu8", "cs16"])
@pytest.mark.parametrize("M", [2, 3, 4, 5])
def test_cli_writes_the_block_of_correlate(tmp_path, fmt, M):
    """The block of `rpf_power --input s0 --correlate s1,... -b 512` (M streams: 1 to 4 files listed) is
    Datastore.correlate over the whole frames of the shortest file, written by the C++ host's writer (which tests/test_correlate.py checks against numpy): the CLI reads
    every file in one piece here, so the lines are equal as text."""
    N, F = 512, 21
    sb = _lib.SAMPLE_BYTES[fmt]
    streams = streams_of(fmt, 110, M, N * F + N // 2 + 1)            # every file holds half a frame more than it gives
    names = []
    for m, s in enumerate(streams):
        data = np.concatenate([s, make_stream(fmt, 120, 3 * N)]) if m == M - 1 else s    # the last one three frames more
        (tmp_path / ("s%d.iq" % m)).write_bytes(data.tobytes())
        names.append(str(tmp_path / ("s%d.iq" % m)))
    with engine(N, fmt) as ds:
        V, n = ds.correlate([s[:sb * N * F] for s in streams])
    assert n == F
    want = format_correlate_block(V, F, N)
    r = subprocess.run([CLI, "-b", str(N), "--format", fmt, "--input", names[0], "--correlate", ",".join(names[1:])],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    head = [l for l in r.stdout.split("\n") if l.startswith("#")]
    assert head[-1] == correlate_header_titles(M)
    got = [l for l in r.stdout.split("\n") if l.strip() and not l.startswith("#")]
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:3]
    note = [l for l in r.stderr.split("\n") if l.startswith("Correlator:")]
    assert len(note) == 1 and ("%d frames" % F) in note[0] and ("%d streams" % M) in note[0] and "differ in length" in note[0], r.stderr
