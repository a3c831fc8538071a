"""K1's derived kernels against float64 truth at all sixteen size x window forms (N = 64 ... 8192, rectangular or Hann).

The plain cu8 kernel has been judged at every form since test_device_path_matches_oracle; the families added after it
(cs8 / cs16, per-bin statistics, the strided kernel, the series kernel, the series of statistics) were judged at five
forms only, and k1_size() departs from the plain table exactly at the others: two waves per SIMD for the statistics
kernels at 128, 256 and 1024, three at windowed 512, the LDS twiddle table of passes 2 and 3 at windowed 8192.  Here
every family runs at every form against ONE reference, frame_truth.truth_frame_powers (numpy complex128 of the exactly
unpacked samples), and beside it the CPU float32 path (the oracle's transform on the same frames).

No threshold is written here: VS_TRUTH, STATS_TIMES_CPU_ERR and SK_SLACK come from stats_bars (parity_bars), and judge()
and same() of test_gpu_spectral_stats apply PARITY and ADDITIVITY as they do there.  Every bin of every row is judged.
Every comparison against the truth at VS_TRUTH is made only after the CPU float32 path itself has met that bar on the
same frames: the stream and the frame count of every form were fixed on the CPU before any GPU run (FRAMES, ROW_FRAMES
below).  Each figure function splits into a CPU part (`*_reference`, cached and shared by the cases that judge the same
stream) and the GPU run; tools/gpu_k1_forms.py calls them and records both sides in profiles/k1_forms_errors.json.
Each test prints the figures it judges."""
import functools

import numpy as np
import pytest

import test_gpu_cf32
import test_hops
from rtl_power_fftw_amd import _lib, stats, synth
from frame_truth import planes, row_planes, truth_frame_powers, unpacked
from helpers import max_rel, oracle_accumulate
from stats_bars import SK_SLACK, STATS_TIMES_CPU_ERR, VS_TRUTH
from test_gpu_sample_formats import device_run
from test_gpu_series import geometry
from test_gpu_series_stats import series_run
from test_gpu_spectral_stats import engine, judge, power_run, same, stats_run
from test_spectral_stats import oracle_frame_powers

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
NO_DMA = _lib.FLAG_NO_LDS_DMA

SIZES = [64, 128, 256, 512, 1024, 2048, 4096, 8192]
FORMS = [(N, window) for N in SIZES for window in (False, True)]
FORM_IDS = ["%d-%s" % (N, "hann" if w else "rect") for N, w in FORMS]

# Frames of a single-acquisition case: the count at which the project's recorded errors were taken.  A form whose CPU
# float32 path missed VS_TRUTH at 80 frames on the CPU would be listed in FRAMES_AT with 160 (none had to be).
FRAMES = 80
FRAMES_AT = {}
# Frames per series row, and the stream.  A row of few frames can leave a bin nearly empty, where no float32 transform has
# relative accuracy.  The rule, applied on the CPU alone (tools/gpu_k1_forms.py --cpu-only; the figures are the
# "cpu_side" section of profiles/k1_forms_errors.json): the smallest of 16, 32, 64 frames per row at which the CPU
# float32 path holds VS_TRUTH in every bin of every row, for every format the form is run with, on noise_tones_iq /
# noise_tones_cs16.  At 16 frames it measured 5.3e-7 and 5.2e-7 at 2048 (rect, Hann), 7.0e-7 at windowed 4096, 7.4e-7
# (cs16 1.1e-6) at windowed 8192, where cs16 still has 5.4e-7 at 32.  At rectangular 8192 the tones' coherent rounding
# error keeps the CPU path at 6.8e-7 even with 64 frames per row (parity_bars.py section 4 describes the effect), so that
# form takes synth.uniform_iq, on which it measures 3.3e-7 at 16.
ROW_FRAMES = 16
ROW_FRAMES_AT = {(2048, False): 32, (2048, True): 32, (4096, True): 32, (8192, True): 64}
UNIFORM_ROWS_AT = {(8192, False)}
SEEDS = {"stats": 41, "formats": 41, "clamped": 31, "strided": 21, "series": 29}


def frames_of(N, window):
    return FRAMES_AT.get((N, window), FRAMES)


def row_frames_of(N, window):
    return ROW_FRAMES_AT.get((N, window), ROW_FRAMES)


def name_of(N, window, *more):
    return " ".join(["N=%d %s" % (N, "hann" if window else "rect")] + [str(m) for m in more])


def window_of(N, window):
    return synth.hann_window(N) if window else None


def stream_of(fmt, seed, nsamples):
    """The default stream of a format: noise and tones, 8-bit for cu8 and full-range 16-bit for cs16."""
    return synth.noise_tones_iq(seed, nsamples) if fmt == "cu8" else synth.noise_tones_cs16(seed, nsamples)


def cpu_frame_powers(N, fmt, stream, frames, window=None, step=None):
    """p[f, b] on the CPU float32 path: test_spectral_stats.oracle_frame_powers as it is.  It unpacks `value - 127`, so a
    signed stream goes in as its values + 127 (exact in float32 up to 2^24: the subtraction gives the stored integer
    back), and overlapped frames go in side by side."""
    if fmt == "cu8" and step in (None, N):
        return oracle_frame_powers(N, stream, frames, window)
    v = unpacked(fmt, stream).reshape(-1, 2)
    idx = (np.arange(frames) * (N if step is None else step))[:, None] + np.arange(N)[None, :]
    return oracle_frame_powers(N, (v[idx] + np.float32(127.0)).reshape(-1), frames, window)


def series_plan(grid, fpw, L):
    """K of a series case: K ceil(L / FPW) iterations exceed the resident grid by about a quarter, so some workgroups
    take a second range, spectra straddle range boundaries and the fix-up kernel runs."""
    per = -(-L // fpw)
    return (grid + grid // 4) // per + 1


# ---- a. statistics planes ------------------------------------------------------------------------------------------

def figures_of(gpu, truth, cpu, orc, frames, **labels):
    """The figures judge() reads -- test_gpu_spectral_stats.accuracy_figures' own, which builds them for cu8 inside its GPU
    run -- from the (3, N) planes of the GPU, of float64 truth and of the CPU float32 path on one stream of `frames`
    frames and the CPU path's accumulated power `orc`: worst per-bin relative errors against the truth, S1 against the
    CPU path, and the spectral kurtosis error over the first-order bound stats_bars.SK_SLACK belongs to."""
    names = ("S1", "S2", "PK")
    fig = dict(labels, frames=frames,
               gpu_vs_truth={k: max_rel(gpu[i], truth[i]) for i, k in enumerate(names)},
               cpu_f32_vs_truth={k: max_rel(cpu[i], truth[i]) for i, k in enumerate(names)},
               S1_gpu_vs_oracle=max_rel(gpu[0], orc))
    sk_gpu, sk_truth = stats.spectral_kurtosis(gpu[0], gpu[1], frames), stats.spectral_kurtosis(truth[0], truth[1], frames)
    d1, d2 = fig["gpu_vs_truth"]["S1"], fig["gpu_vs_truth"]["S2"]
    bound = (frames + 1) / (frames - 1) * (frames * truth[1] / truth[0] ** 2) * (d2 + 2 * d1) * SK_SLACK
    fig["sk_err_over_bound"] = float(np.max(np.abs(sk_gpu - sk_truth) / bound))
    fig["sk_abs_err"] = float(np.max(np.abs(sk_gpu - sk_truth)))
    return fig


@functools.lru_cache(maxsize=2)
def stats_reference(N, window, fmt):
    frames = frames_of(N, window)
    u = stream_of(fmt, SEEDS["stats"], frames * N)
    w = window_of(N, window)
    truth = planes(truth_frame_powers(N, unpacked(fmt, u), frames, w))
    cpu = planes(cpu_frame_powers(N, fmt, u, frames, w))
    # the CPU path's accumulated power: rpf_oracle_accumulate reads cu8 only; for cs16 the sum of the same transform's frames
    orc = oracle_accumulate(N, u, frames, w)[0] if fmt == "cu8" else cpu[0]
    return {"stream": u, "frames": frames, "truth": truth, "cpu": cpu, "orc": orc,
            "cpu_f32_vs_truth": {k: max_rel(cpu[i], truth[i]) for i, k in enumerate(("S1", "S2", "PK"))}}


def stats_figures(N, window, fmt, flags):
    ref = stats_reference(N, window, fmt)
    u, frames = ref["stream"], ref["frames"]
    with engine(N, fmt, window=window, flags=flags) as ds:
        gpu, n, _ = stats_run(ds, u)
        s1_only, n1, _ = power_run(ds, u)                      # the same engine's rpf_accumulate_device
        one, m1, _ = stats_run(ds, u[:_lib.SAMPLE_BYTES[fmt] * N])
    assert n == n1 == frames and m1 == 1
    fig = figures_of(gpu, ref["truth"], ref["cpu"], ref["orc"], frames, N=N, window=bool(window), format=fmt,
                     staging="vgpr" if flags & NO_DMA else "lds_dma")
    fig["S1_equals_accumulate_device"] = bool(np.array_equal(gpu[0], s1_only))
    fig["one_frame_exact"] = bool(np.array_equal(one[2], one[0]) and np.array_equal(one[1], one[0] * one[0])
                                  and np.all(one[0] > 0))
    return fig


@pytest.mark.parametrize("flags", [0, NO_DMA], ids=["lds_dma", "vgpr"])
@pytest.mark.parametrize("fmt", ["cu8", "cs16"])
@pytest.mark.parametrize("N,window", FORMS, ids=FORM_IDS)
def test_statistics_planes(N, window, fmt, flags):
    fig = stats_figures(N, window, fmt, flags)
    assert fig["cpu_f32_vs_truth"]["S1"] < VS_TRUTH, "the bar is one the reference itself meets on this input"
    judge(fig)                                                 # (prints the figures)
    assert fig["S1_equals_accumulate_device"] and fig["one_frame_exact"]


# ---- b. sample formats on the plain kernel -------------------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def cs16_reference(N, window):
    frames = frames_of(N, window)
    s = synth.noise_tones_cs16(SEEDS["formats"], frames * N)   # test_full_range_cs16_against_truth's stream
    v = synth.cs16_values(s)
    assert int(v.max()) > 16384 and int(v.min()) < -16384, "the stream uses the high byte"
    w = window_of(N, window)
    truth = truth_frame_powers(N, unpacked("cs16", s), frames, w).sum(axis=0)
    cpu = cpu_frame_powers(N, "cs16", s, frames, w).sum(axis=0)
    return {"stream": s, "frames": frames, "truth": truth, "cpu_vs_truth": max_rel(cpu, truth)}


def formats_figures(N, window):
    ref = cs16_reference(N, window)
    with engine(N, "cs16", window=window, bin_stats=False) as ds:
        got, n, _ = device_run(ds, ref["stream"])
    assert n == ref["frames"]
    u = np.minimum(synth.noise_tones_iq(SEEDS["clamped"], ref["frames"] * N), 254).astype(np.uint8)
    with engine(N, "cu8", window=window, bin_stats=False) as a, engine(N, "cs8", window=window, bin_stats=False) as b:
        want, n0, g0 = device_run(a, u)
        got8, n1, g1 = device_run(b, synth.to_cs8(u))
    assert n0 == n1 == ref["frames"] and g0 == g1, "cs8 shares cu8's staging: same launch geometry"
    return {"N": N, "window": bool(window), "frames": ref["frames"], "cs16_gpu_vs_truth": max_rel(got, ref["truth"]),
            "cs16_cpu_f32_vs_truth": ref["cpu_vs_truth"], "cs8_equals_cu8": bool(np.array_equal(got8, want))}


@pytest.mark.parametrize("N,window", FORMS, ids=FORM_IDS)
def test_sample_formats_on_the_plain_kernel(N, window):
    fig = formats_figures(N, window)
    print(fig)
    assert fig["cs8_equals_cu8"]
    assert fig["cs16_cpu_f32_vs_truth"] < VS_TRUTH, "the bar is one the reference itself meets on this input"
    assert fig["cs16_gpu_vs_truth"] < VS_TRUTH


# ---- c. the strided kernel -----------------------------------------------------------------------------------------

def strided_steps(N):
    return (N // 2, N // 2 + 1)


@functools.lru_cache(maxsize=2)
def strided_reference(N, window, fmt, step):
    frames = frames_of(N, window)
    X = stream_of(fmt, SEEDS["strided"], N + step * (frames - 1))          # as many samples as give `frames` frames
    w = window_of(N, window)
    truth = truth_frame_powers(N, unpacked(fmt, X), frames, w, step=step).sum(axis=0)
    cpu = cpu_frame_powers(N, fmt, X, frames, w, step=step).sum(axis=0)
    return {"stream": X, "frames": frames, "truth": truth, "cpu_vs_truth": max_rel(cpu, truth)}


def strided_figures(N, window, fmt, step):
    ref = strided_reference(N, window, fmt, step)
    with engine(N, fmt, step=step, window=window, bin_stats=False) as ds:
        assert ds.frames_in(ref["stream"].size) == ref["frames"]
        got, n, _ = device_run(ds, ref["stream"])
    assert n == ref["frames"]
    return {"N": N, "window": bool(window), "format": fmt, "step": step, "frames": ref["frames"],
            "gpu_vs_truth": max_rel(got, ref["truth"]), "cpu_f32_vs_truth": ref["cpu_vs_truth"]}


@pytest.mark.parametrize("fmt", ["cu8", "cs16"])
@pytest.mark.parametrize("N,window", FORMS, ids=FORM_IDS)
def test_strided_kernel(N, window, fmt):
    for step in strided_steps(N):
        fig = strided_figures(N, window, fmt, step)
        print(fig)
        assert fig["cpu_f32_vs_truth"] < VS_TRUTH, "the bar is one the reference itself meets on this input"
        assert fig["gpu_vs_truth"] < VS_TRUTH


# ---- d. series rows; e. series-of-statistics rows --------------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def series_reference(N, window, fmt, L, K):
    """Rows of S1, S2, PK (K, 3, N) of the truth and of the CPU float32 path over the frames [k L, (k + 1) L), and the
    stream: K L frames and a tail of L - 1 that belong to no row."""
    frames = K * L
    if (N, window) in UNIFORM_ROWS_AT:
        assert fmt == "cu8"
        u = synth.uniform_iq(SEEDS["series"], (frames + L - 1) * N)
    else:
        u = stream_of(fmt, SEEDS["series"], (frames + L - 1) * N)
    w = window_of(N, window)
    truth = row_planes(truth_frame_powers(N, unpacked(fmt, u), frames, w), L, K)
    cpu = row_planes(cpu_frame_powers(N, fmt, u, frames, w), L, K)
    return {"stream": u, "truth": truth, "cpu": cpu,
            "cpu_f32_vs_truth": {k: max_rel(cpu[:, i], truth[:, i]) for i, k in enumerate(("S1", "S2", "PK"))}}


def series_case(N, window):
    """(L, K) of the form's series cases: from the plain cu8 engine's resident grid, shared by (d) and (e) and by both
    formats so that they share one reference per stream."""
    L = row_frames_of(N, window)
    with engine(N, window=window, bin_stats=False) as ds:
        grid, fpw = geometry(ds)
    return L, series_plan(grid, fpw, L), grid, fpw


def series_figures(N, window, fmt, case=None):
    L, K, grid, fpw = case or series_case(N, window)
    ref = series_reference(N, window, fmt, L, K)
    with engine(N, fmt, window=window, bin_stats=False) as ds:
        rows, done, launches, geom = series_run(ds, ref["stream"], L)
    assert done == K and launches == 1, (done, K, launches)
    assert K * -(-L // geom[1]) > geom[0], "more iterations than workgroups: ranges share spectra, the fix-up runs"
    return {"N": N, "window": bool(window), "format": fmt, "L": L, "K": K, "grid": geom[0], "frames_per_wg": geom[1],
            "rows_past_K_untouched": bool(np.all(rows[K:] == -1.0)),
            "gpu_vs_truth": max_rel(rows[:K, 0], ref["truth"][:, 0]), "cpu_f32_vs_truth": ref["cpu_f32_vs_truth"]["S1"]}


@pytest.mark.parametrize("N,window", FORMS, ids=FORM_IDS)
def test_series_rows(N, window):
    case = series_case(N, window)
    for fmt in ("cu8", "cs16") if window else ("cu8",):
        fig = series_figures(N, window, fmt, case)
        print(fig)
        assert fig["rows_past_K_untouched"]
        assert fig["cpu_f32_vs_truth"] < VS_TRUTH, "the bar is one the reference itself meets on this input"
        assert fig["gpu_vs_truth"] < VS_TRUTH


# ---- f. the scan kernel and cf32 at the sizes their own files leave out ----------------------------------------------

@pytest.mark.parametrize("windowed", [False, True], ids=["rect", "hann"])
@pytest.mark.parametrize("N", [128, 256, 2048])
def test_scan_kernel_at_the_sizes_test_hops_leaves_out(N, windowed):
    """test_hops.test_hops_entry_matches_oracle_and_single_entry (64, 512, 1024, 4096, 8192) as it is, at the other three."""
    test_hops.test_hops_entry_matches_oracle_and_single_entry(N, windowed, torch.device("cuda:0"))


@pytest.mark.parametrize("window", [False, True], ids=["rect", "hann"])
def test_cf32_at_128(window):
    """test_gpu_cf32's identities (cf32 of integers == cs16, exact scaling) as they are, at the size its K1_SIZES leaves
    out; and its Gaussian-against-truth case at windowed 128, one of the three cf32 forms that gave up a wave to compile."""
    test_gpu_cf32.test_cf32_of_integers_equals_cs16_and_scales_exactly(128, window)
    if window:
        test_gpu_cf32.test_gaussian_cf32_against_truth(128, True)


def series_stats_figures(N, window, flags, case=None):
    L, K, grid, fpw = case or series_case(N, window)
    ref = series_reference(N, window, "cu8", L, K)
    with engine(N, window=window, flags=flags) as st, engine(N, window=window, flags=flags, bin_stats=False) as plain:
        rows, done, launches, geom = series_run(st, ref["stream"], L)
        want, kp, lp, gp = series_run(plain, ref["stream"], L)
    assert done == kp == K and launches == lp == 1, (done, kp, K, launches, lp)
    assert K * -(-L // geom[1]) > geom[0], "more iterations than workgroups: ranges share spectra, the fix-up runs"
    fig = {"N": N, "window": bool(window), "staging": "vgpr" if flags & NO_DMA else "lds_dma", "L": L, "K": K,
           "grid": geom[0], "frames_per_wg": geom[1], "plain_grid": gp[0],
           "rows_past_K_untouched": bool(np.all(rows[K:] == -1.0)),
           "S1_equals_plain_series": bool(same(rows[:K, 0], want[:K, 0], geom, gp, name_of(N, window, "S1 plane"))),
           "gpu_vs_truth": {k: max_rel(rows[:K, i], ref["truth"][:, i]) for i, k in enumerate(("S1", "S2", "PK"))},
           "cpu_f32_vs_truth": ref["cpu_f32_vs_truth"]}
    return fig


# (last in the file: at eleven of the forms these kernels have not been launched on a GPU before)
@pytest.mark.parametrize("flags", [0, NO_DMA], ids=["lds_dma", "vgpr"])
@pytest.mark.parametrize("N,window", FORMS, ids=FORM_IDS)
def test_series_of_statistics_rows(N, window, flags):
    fig = series_stats_figures(N, window, flags)
    print(fig)
    g, c = fig["gpu_vs_truth"], fig["cpu_f32_vs_truth"]
    assert fig["rows_past_K_untouched"] and fig["S1_equals_plain_series"]
    assert c["S1"] < VS_TRUTH, "the bar is one the reference itself meets on this input"
    assert g["S1"] < VS_TRUTH
    assert g["S2"] <= STATS_TIMES_CPU_ERR * c["S2"], ("S2", g["S2"], c["S2"])
    assert g["PK"] <= STATS_TIMES_CPU_ERR * c["PK"], ("PK", g["PK"], c["PK"])
