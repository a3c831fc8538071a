"""Per-bin statistics on the MI355X (RPF_FLAG_BIN_STATS): S2 = sum of the squared frame powers and PK = peak hold
beside the power S1, from K1 (powers of two 64 .. 8192) and from the catch-all path (every other size).

Identities first, asserted with np.array_equal unless said otherwise: the power is untouched; one frame gives PK == S1
and S2 == S1 * S1; powers of two scale exactly; cs8 == cu8; the maximum does not care how a stream is cut; the queue
path is the device path; the inequalities S1/M <= PK <= S1 and S1^2/M <= S2 <= PK S1.  Then accuracy against float64
truth, measured against what the CPU float32 path reaches on the same stream (stats_bars.py), and one acquisition
through the CLI in which the spectral kurtosis has to find what it is for.  Each test prints the figures it judged."""
import os
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, stats, synth
from rtl_power_fftw_amd.datastore import frames_in
from helpers import ROOT, max_rel, oracle_accumulate
from stats_bars import (ADDITIVITY, MEAN_LOWER_DB, PARITY, PEAK_WITHIN_DB, SAME_KERNELS, SK_BURST_ABOVE, SK_NOISE_RANGE,
                        SK_SLACK, SK_STEADY_BELOW, STATS_TIMES_CPU_ERR, VS_TRUTH)
from test_frame_overlap import materialise
from test_spectral_stats import oracle_frame_powers

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
NO_DMA = _lib.FLAG_NO_LDS_DMA
CATCH_ALL = _lib.FLAG_CATCH_ALL

# (N, windowed): the sizes of the LDS-resident kernel the identities are checked on
K1_CASES = [(64, False), (512, False), (4096, False), (4096, True), (8192, False)]


def to_device(stream):
    t = torch.empty(stream.size + 64, dtype=torch.uint8, device=DEV)
    t[:stream.size].copy_(torch.from_numpy(np.ascontiguousarray(stream)))
    return t


def engine(N, fmt="cu8", step=None, window=False, flags=0, bin_stats=True, **kw):
    w = synth.hann_window(N) if window else None
    return rpf.Datastore(rpf.Params(N=N, window=window, frame_step=step, sample_format=fmt, bin_stats=bin_stats, **kw), w,
                         flags=flags)


def stats_run(ds, stream, repeats=1 << 40):
    """((S1, S2, PK), frames, launch geometry) of one device-resident acquisition with statistics."""
    keep = to_device(stream)
    out = torch.full((3, ds.params.N), -1.0, dtype=torch.float64, device=DEV)
    n = ds.accumulate_device_stats(keep.data_ptr(), stream.size, repeats, out.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    li = ds.launch_info()
    del keep
    return out.cpu().numpy(), n, (li["grid"], li["frames_per_wg"])


def power_run(ds, stream, repeats=1 << 40):
    keep = to_device(stream)
    out = torch.full((ds.params.N,), -1.0, dtype=torch.float64, device=DEV)
    n = ds.accumulate_device(keep.data_ptr(), stream.size, repeats, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    li = ds.launch_info()
    del keep
    return out.cpu().numpy(), n, (li["grid"], li["frames_per_wg"])


def same(got, want, geom_got, geom_want, what):
    """test_gpu_sample_formats.py's sense of "equal"; says which of the two it applied."""
    if geom_got == geom_want:
        print("%s: same geometry %s -> array_equal" % (what, geom_got))
        return np.array_equal(got, want)
    err = max_rel(got, want)
    print("%s: geometry %s vs %s -> ADDITIVITY, measured %.3g" % (what, geom_got, geom_want, err))
    return err < ADDITIVITY


def check_inequalities(s, M, what):
    """S1/M <= PK <= S1 and S1^2/M <= S2 <= PK S1 hold in exact arithmetic; relative slack ADDITIVITY."""
    s1, s2, pk = s
    lo, hi = 1 - ADDITIVITY, 1 + ADDITIVITY
    assert np.all(s1 / M * lo <= pk) and np.all(pk * lo <= s1), what
    assert np.all(s1 * s1 / M * lo <= s2) and np.all(s2 * lo <= pk * s1 * hi), what


# ---- 1, 2, 7: the power is untouched; one frame; the inequalities ----------------------------------------------------

@pytest.mark.parametrize("N,window", K1_CASES)
def test_power_untouched_one_frame_and_inequalities(N, window):
    R = 70
    u = synth.noise_tones_iq(31, R * N)
    for step in (N, N // 2 + 1):
        M = frames_in(u.size, N, step)
        for flags in (0, NO_DMA):
            with engine(N, step=step, window=window, flags=flags) as st, \
                    engine(N, step=step, window=window, flags=flags, bin_stats=False) as plain:
                assert st.has_bin_stats and not plain.has_bin_stats
                got, n, g = stats_run(st, u)
                s1_only, n1, g1 = power_run(st, u)                 # the same engine's rpf_accumulate_device
                want, n0, g0 = power_run(plain, u)
                one, m1, _ = stats_run(st, u[:2 * N])
                with pytest.raises(rpf.RPFError) as e:             # a plain engine has no statistics to give
                    stats_run(plain, u)
                assert e.value.retval == rpf.ReturnValue.InvalidArgument
            assert n == n0 == n1 == M and m1 == 1
            assert np.array_equal(got[0], s1_only)
            assert same(got[0], want, g, g0, "S1 N=%d win=%d step=%d flags=%d" % (N, window, step, flags))
            assert np.array_equal(one[2], one[0]) and np.array_equal(one[1], one[0] * one[0])
            assert np.all(one[0] > 0)
            check_inequalities(got, M, (N, window, step, flags))
            assert np.all(got[2] > got[0] / M)                     # noise: some frame is above the mean


# ---- 3. powers of two scale exactly ----------------------------------------------------------------------------------

@pytest.mark.parametrize("N,window", K1_CASES)
def test_cs16_scaling_is_exact(N, window):
    k, R = 3, 40
    v8 = synth.to_cs8(np.minimum(synth.noise_tones_iq(33, R * N), 254).astype(np.uint8))
    a, b = synth.to_cs16(v8), synth.to_cs16(v8, shift=k)
    for step in (N, N // 2 + 1):
        for flags in (0, NO_DMA):
            with engine(N, "cs16", step, window, flags) as ds:
                base, n0, _ = stats_run(ds, a)
                big, n1, _ = stats_run(ds, b)
            assert n0 == n1 == frames_in(a.size, N, step, 4)
            assert np.array_equal(big[0], base[0] * 4.0 ** k) and np.array_equal(big[2], base[2] * 4.0 ** k)
            assert np.array_equal(big[1], base[1] * 16.0 ** k)


# ---- 4. cs8 == cu8 ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,window", K1_CASES)
def test_cs8_equals_cu8(N, window):
    R = 50
    u = np.minimum(synth.noise_tones_iq(35, R * N), 254).astype(np.uint8)
    s = synth.to_cs8(u)
    for step in (N, N // 2 + 1):
        for flags in (0, NO_DMA):
            with engine(N, "cu8", step, window, flags) as a, engine(N, "cs8", step, window, flags) as b:
                want, n0, g0 = stats_run(a, u)
                got, n1, g1 = stats_run(b, s)
            assert n0 == n1 and g0 == g1, "cs8 shares cu8's staging: same launch geometry"
            assert np.array_equal(got, want), (N, step, flags)


# ---- 5. the maximum is order-free ------------------------------------------------------------------------------------

def check_halves(ds, u, N, R):
    half = (R // 2) * 2 * N
    whole, n, _ = stats_run(ds, u)
    a, na, _ = stats_run(ds, u[:half])
    b, nb, _ = stats_run(ds, u[half:])
    assert n == R == na + nb
    assert np.array_equal(whole[2], np.maximum(a[2], b[2]))
    e1, e2 = max_rel(whole[0], a[0] + b[0]), max_rel(whole[1], a[1] + b[1])
    print("halves N=%d: S1 %.3g S2 %.3g (bar %.1g)" % (N, e1, e2, ADDITIVITY))
    assert e1 < ADDITIVITY and e2 < ADDITIVITY
    return whole


@pytest.mark.parametrize("N,window", K1_CASES)
def test_peak_of_halves(N, window):
    R = 61
    u = synth.noise_tones_iq(37, R * N)
    for flags in (0, NO_DMA):
        with engine(N, window=window, flags=flags) as ds:
            check_halves(ds, u, N, R)


# ---- 6. queue path == device path ------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,window", K1_CASES)
def test_queue_path_equals_device_path(N, window):
    R, keep = 90, 77                                  # the stream holds more frames than are asked for
    u = synth.noise_tones_iq(39, R * N)
    u[2 * N * keep:] = 255                            # dropped frames are LOUD: they must not reach PK
    for step in (N, N // 2 + 1):
        M = keep
        for flags in (0, NO_DMA):
            # a buffer size that is no multiple of the frame: frames straddle buffers
            with engine(N, step=step, window=window, flags=flags, buffers=3, buf_length=2 * (3 * N // 2 + 7)) as ds:
                pwr, done = ds.accumulate(u, M)
                q = np.array([pwr, ds.sum_sq.copy(), ds.peak.copy()])
                d, n, _ = stats_run(ds, u, M)
                sk = ds.spectral_kurtosis()
            assert done == n == M
            assert np.array_equal(q[2], d[2])
            e1, e2 = max_rel(q[0], d[0]), max_rel(q[1], d[1])
            print("queue vs device N=%d step=%d flags=%d: S1 %.3g S2 %.3g" % (N, step, flags, e1, e2))
            assert e1 < SAME_KERNELS and e2 < SAME_KERNELS
            assert np.array_equal(sk, stats.spectral_kurtosis(q[0], q[1], M))
            # nothing of the frames past `repeats` (all-255 samples, loud at DC) got in: the stream cut after them says the same
            with engine(N, step=step, window=window, flags=flags) as cut:
                quiet, nq, _ = stats_run(cut, u[:2 * (N + step * (M - 1))])
            assert nq == M and np.array_equal(quiet[2], q[2])
    # the dropped frames would have been seen: the same engine over the whole stream has a larger DC peak
    with engine(N, window=window) as ds:
        everything, _, _ = stats_run(ds, u)
        kept, _, _ = stats_run(ds, u, keep)
    assert everything[2][N // 2] > kept[2][N // 2]


# ---- 8. the catch-all path -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,R,flags", [(5000, 40, 0), (65536, 8, 0), (4096, 40, CATCH_ALL)])
def test_catch_all_identities(N, R, flags):
    u = synth.noise_tones_iq(41, R * N)
    with engine(N, flags=flags) as ds:
        one, m1, _ = stats_run(ds, u[:2 * N])
        whole = check_halves(ds, u, N, R)
        s1_only, _, _ = power_run(ds, u)
    assert m1 == 1 and np.array_equal(one[2], one[0]) and np.array_equal(one[1], one[0] * one[0])
    assert np.array_equal(whole[0], s1_only)
    check_inequalities(whole, R, N)
    # overlapped frames go through the gather: every frame of the materialised stream, the same numbers
    step = N // 2 + 1
    M = frames_in(u.size, N, step)
    with engine(N, step=step, flags=flags) as a, engine(N, flags=flags) as b:
        got, n, _ = stats_run(a, u)
        want, n2, _ = stats_run(b, materialise(u, N, step))
    assert n == n2 == M
    assert np.array_equal(got[2], want[2])
    assert max_rel(got[0], want[0]) < ADDITIVITY and max_rel(got[1], want[1]) < ADDITIVITY
    if flags & CATCH_ALL:
        # the K1-sized catch-all run against the K1 run: two float32 transforms, each inside the accuracy bars below
        with engine(N) as k1:
            native, _, _ = stats_run(k1, u)
        fig = accuracy_figures(N, False, "noise_tones", flags=flags, frames=R)
        print("catch-all vs K1 N=%d: S1 %.3g S2 %.3g PK %.3g" % (N, max_rel(whole[0], native[0]), max_rel(whole[1], native[1]),
                                                                 max_rel(whole[2], native[2])))
        assert max_rel(whole[0], native[0]) < PARITY
        judge(fig)


# ---- accuracy --------------------------------------------------------------------------------------------------------

def truth_frame_powers(N, stream, frames, window=None):
    """p of every frame and bin in float64: helpers.truth_f64's evaluation, kept per frame."""
    sign = (1 - 2 * (np.arange(N) % 2)).astype(np.float32)
    x = np.asarray(stream[:2 * N * frames]).astype(np.float32).reshape(frames, N, 2) - np.float32(127.0)
    x = x * sign[None, :, None]
    if window is not None:
        x = x * np.asarray(window, dtype=np.float32)[None, :, None]
    z = x[..., 0].astype(np.float64) + 1j * x[..., 1].astype(np.float64)
    spec = np.fft.fft(z, axis=1)
    return spec.real ** 2 + spec.imag ** 2


def planes(p):
    return np.array([p.sum(axis=0), (p * p).sum(axis=0), p.max(axis=0)])


def accuracy_figures(N, window, stream_name, flags=0, frames=80):
    """Worst per-bin relative errors of S1, S2, PK against float64 truth, for the GPU and for the CPU float32 path on
    the same stream; and the spectral kurtosis of both ends.  (tools/gpu_spectral_stats.py records them.)"""
    gen = synth.noise_tones_iq if stream_name == "noise_tones" else synth.uniform_iq
    u = gen(41, frames * N)
    w = synth.hann_window(N) if window else None
    with engine(N, window=window, flags=flags) as ds:
        gpu, n, _ = stats_run(ds, u)
    assert n == frames
    truth = planes(truth_frame_powers(N, u, frames, w))
    cpu = planes(oracle_frame_powers(N, u, frames, w))
    orc, _ = oracle_accumulate(N, u, frames, w)
    names = ("S1", "S2", "PK")
    fig = {"N": N, "window": bool(window), "stream": stream_name, "frames": frames, "catch_all": bool(flags & CATCH_ALL),
           "gpu_vs_truth": {k: max_rel(gpu[i], truth[i]) for i, k in enumerate(names)},
           "cpu_f32_vs_truth": {k: max_rel(cpu[i], truth[i]) for i, k in enumerate(names)},
           "S1_gpu_vs_oracle": max_rel(gpu[0], orc)}
    sk_gpu, sk_truth = stats.spectral_kurtosis(gpu[0], gpu[1], frames), stats.spectral_kurtosis(truth[0], truth[1], frames)
    d1, d2 = fig["gpu_vs_truth"]["S1"], fig["gpu_vs_truth"]["S2"]
    bound = (frames + 1) / (frames - 1) * (frames * truth[1] / truth[0] ** 2) * (d2 + 2 * d1) * SK_SLACK
    fig["sk_err_over_bound"] = float(np.max(np.abs(sk_gpu - sk_truth) / bound))
    fig["sk_abs_err"] = float(np.max(np.abs(sk_gpu - sk_truth)))
    return fig


def judge(fig):
    print(fig)
    g, c = fig["gpu_vs_truth"], fig["cpu_f32_vs_truth"]
    assert fig["S1_gpu_vs_oracle"] < PARITY and g["S1"] < VS_TRUTH
    assert g["S2"] <= STATS_TIMES_CPU_ERR * c["S2"], ("S2", g["S2"], c["S2"])
    assert g["PK"] <= STATS_TIMES_CPU_ERR * c["PK"], ("PK", g["PK"], c["PK"])
    assert fig["sk_err_over_bound"] <= 1.0


@pytest.mark.parametrize("stream_name", ["noise_tones", "uniform"])
@pytest.mark.parametrize("N,window", K1_CASES + [(5000, False)])
def test_accuracy_against_truth(N, window, stream_name):
    judge(accuracy_figures(N, window, stream_name, frames=40 if N == 5000 else 80))


# ---- it detects what it is for ---------------------------------------------------------------------------------------

def interference_stream(N=4096, frames=1000):
    """8-bit Gaussian noise (sigma 20 about 127), a steady carrier of amplitude 30 on input bin 1000 and a second one on
    input bin 3000 in every tenth frame only; rounded, clipped to 0 .. 255."""
    rng = np.random.default_rng(5)
    n = np.arange(N)
    noise = rng.normal(0.0, 20.0, size=(frames, N, 2))
    steady = 30.0 * np.exp(2j * np.pi * 1000 * n / N)
    burst = 30.0 * np.exp(2j * np.pi * 3000 * n / N)
    on = (np.arange(frames) % 10 == 0).astype(np.float64)
    z = steady[None, :] + on[:, None] * burst[None, :]
    x = noise + np.stack([z.real, z.imag], axis=-1) + 127.0
    return np.clip(np.rint(x), 0, 255).astype(np.uint8).reshape(-1)


def test_cli_finds_the_interference(tmp_path):
    N, M, steady_bin, burst_bin = 4096, 1000, 3048, 952      # output bins: input bin + N/2 (the (-1)^n shift)
    u = interference_stream(N, M)
    noise_bins = np.array([k for k in range(N) if k not in (steady_bin, burst_bin, N // 2)])

    def check(sk, pk_db, mean_db, what):
        print("%s: noise SK %.3f .. %.3f (sd %.3f), steady %.3g, burst %.3f; peaks %.2f dB apart, means %.2f dB apart"
              % (what, sk[noise_bins].min(), sk[noise_bins].max(), sk[noise_bins].std(), sk[steady_bin], sk[burst_bin],
                 abs(pk_db[burst_bin] - pk_db[steady_bin]), mean_db[steady_bin] - mean_db[burst_bin]))
        assert np.all(sk[noise_bins] >= SK_NOISE_RANGE[0]) and np.all(sk[noise_bins] <= SK_NOISE_RANGE[1])
        assert sk[steady_bin] < SK_STEADY_BELOW and sk[burst_bin] > SK_BURST_ABOVE
        assert abs(pk_db[burst_bin] - pk_db[steady_bin]) < PEAK_WITHIN_DB
        assert MEAN_LOWER_DB[0] < mean_db[steady_bin] - mean_db[burst_bin] < MEAN_LOWER_DB[1]

    # first the float64 truth: if it does not show the interference, the stream is wrong, not the kernel
    t = planes(truth_frame_powers(N, u, M))
    check(stats.spectral_kurtosis(t[0], t[1], M), 10 * np.log10(t[2]), 10 * np.log10(t[0] / M), "float64 truth")

    (tmp_path / "rfi.cu8").write_bytes(u.tobytes())
    r = subprocess.run([CLI, "-b", str(N), "-n", str(M), "-q", "--stats", "--input", str(tmp_path / "rfi.cu8")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "# frequency [Hz] power spectral density [dB/Hz] peak hold [dB/Hz] spectral kurtosis" in r.stdout.split("\n")
    rows = np.array([[float(v) for v in l.split()] for l in r.stdout.split("\n") if l.strip() and not l.startswith("#")])
    assert rows.shape == (N, 4)
    check(rows[:, 3], rows[:, 2], rows[:, 1], "rpf_power --stats")
    # without --stats the same acquisition prints the same first two columns and nothing else
    r2 = subprocess.run([CLI, "-b", str(N), "-n", str(M), "-q", "--input", str(tmp_path / "rfi.cu8")],
                        capture_output=True, text=True)
    assert r2.returncode == 0, r2.stderr
    plain = [l.split() for l in r2.stdout.split("\n") if l.strip() and not l.startswith("#")]
    with_stats = [l.split()[:2] for l in r.stdout.split("\n") if l.strip() and not l.startswith("#")]
    assert plain == with_stats


# ---- out of scope fails loudly ----------------------------------------------------------------------------------------

def test_out_of_scope_entries_say_so():
    N = 4096
    u = synth.noise_tones_iq(43, 8 * N)
    keep = to_device(u)
    out = torch.zeros(2 * N, dtype=torch.float64, device=DEV)
    with engine(N) as ds:
        for call in (lambda: ds.device_fused(keep.data_ptr(), u.size, 8), lambda: ds.device_reduce(out.data_ptr()),
                     lambda: ds.device_fused_hops([keep.data_ptr()], [u.size], [8])):
            with pytest.raises(rpf.RPFError) as e:
                call()
            assert e.value.retval == rpf.ReturnValue.InvalidArgument and "RPF_FLAG_BIN_STATS" in str(e.value)
        # a scan on a stats engine: hop by hop, the power alone
        half = u.size // 2
        done = ds.accumulate_device_hops([keep.data_ptr(), keep.data_ptr() + half], [half, half], [4, 4], out.data_ptr())
        torch.cuda.synchronize()
        a, _, _ = power_run(ds, u[:half])
        b, _, _ = power_run(ds, u[half:])
    assert done == [4, 4]
    assert np.array_equal(out.cpu().numpy(), np.concatenate([a, b]))
