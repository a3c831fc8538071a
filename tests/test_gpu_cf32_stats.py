"""cf32 with per-bin statistics on K1, on the MI355X: a cf32 engine with RPF_FLAG_BIN_STATS runs the LDS-resident
kernel at the powers of two 64 .. 8192 (rpf_kernels_stats_cf32.hip, rpf_kernels_series_stats_cf32.hip), its series of
statistics and its excised average take the one-launch route.

The route is read from launch_info() (the catch-all path reports no LDS) and series_launches().  The numbers are tied
to the tested cs16 statistics kernels by the identities of test_gpu_cf32.py: a cf32 stream of int16 values leaves the
unpack as the cs16 stream of those values does, so S1, S2 and PK are the cs16 engine's -- np.array_equal where both runs
report the same launch geometry, ADDITIVITY otherwise for the two sums (same() of test_gpu_sample_formats), and always
np.array_equal for PK, a maximum, which no partition of the frames changes.  Gaussian float32 input with full mantissas
is judged against numpy complex128 at the bars of cf32_bars and stats_bars.  Each test prints the figures it judged."""
import functools
import os
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, stats, synth
from rtl_power_fftw_amd.datastore import frames_in
from cf32_bars import CF32_VS_TRUTH
from cf32_stats_bars import NAN_ROUTES_PK
from frame_truth import planes, truth_frame_powers, unpacked
from helpers import ROOT, fp, max_err_over_mean, max_rel, oracle_lib
from parity_bars import ADDITIVITY, SAME_KERNELS
from test_cf32_stats import geometry
from test_excise import err_over_total
from test_gpu_excise import excised, series_rows
from test_gpu_k1_forms import figures_of, series_plan
from test_gpu_sample_formats import same, to_device
from test_gpu_series_stats import blocks_of, one_unit_of_the_last_digit, series_run, slice_rows
from test_gpu_spectral_stats import engine, judge

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")
NO_DMA = _lib.FLAG_NO_LDS_DMA
CATCH_ALL = _lib.FLAG_CATCH_ALL
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")

K1_SIZES = [64, 128, 256, 512, 1024, 2048, 4096, 8192]
FORMS = [(N, window) for N in K1_SIZES for window in (False, True)]
FORM_IDS = ["%d-%s" % (N, "hann" if w else "rect") for N, w in FORMS]


def as_bytes(stream):
    return np.ascontiguousarray(stream).view(np.uint8).reshape(-1)


def stats_run(ds, stream, repeats=1 << 40, misalign=0):
    """((S1, S2, PK), frames, (grid, frames per workgroup), launch_info) of one rpf_accumulate_device_stats call on the
    bytes of `stream`, placed `misalign` bytes past a 16-byte boundary."""
    b = as_bytes(stream)
    keep, ptr = to_device(b, misalign)
    out = torch.full((3, ds.params.N), -1.0, dtype=torch.float64, device=DEV)
    n = ds.accumulate_device_stats(ptr, b.size, repeats, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del keep
    li = ds.launch_info()
    return out.cpu().numpy(), n, (li["grid"], li["frames_per_wg"]), li


def int16_streams(seed, nsamples):
    s16 = synth.noise_tones_cs16(seed, nsamples)
    return s16, synth.to_cf32(s16)


def same_planes(got, want, g_got, g_want, what):
    """S1 and S2 by same(), PK bit for bit."""
    assert np.array_equal(got[2], want[2]), "%s: PK" % what
    return same(got[0], want[0], g_got, g_want, what + " S1") and same(got[1], want[1], g_got, g_want, what + " S2")


# ---- the route ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,window", FORMS, ids=FORM_IDS)
def test_a_cf32_stats_engine_runs_k1(N, window):
    """launch_info() after rpf_accumulate_device is the geometry k1_sizes.h states for the form (workgroup, frames per
    workgroup, dynamic LDS); the catch-all path reports no LDS and one frame per workgroup."""
    _, z = int16_streams(3, 5 * N)
    with engine(N, "cf32", window=window) as ds:
        out = torch.empty(N, dtype=torch.float64, device=DEV)
        keep, ptr = to_device(as_bytes(z))
        assert ds.accumulate_device(ptr, 8 * z.size, 1 << 40, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 5
        torch.cuda.synchronize()
        li = ds.launch_info()
    assert li["lds_bytes"] > 0
    assert (li["block"], li["frames_per_wg"], li["lds_bytes"]) == geometry()[(N, window)]


def test_other_sizes_are_still_the_catch_all():
    N = 1000
    _, z = int16_streams(3, 5 * N)
    with engine(N, "cf32") as ds:
        got, n, _, li = stats_run(ds, z)
    assert n == 5 and li["lds_bytes"] == 0 and np.all(got[0] > 0)


@pytest.mark.parametrize("N", [64, 512, 4096])
def test_series_of_statistics_is_one_launch(N):
    L, K = 3, 7
    _, z = int16_streams(5, K * L * N)
    with engine(N, "cf32") as ds:
        rows, done, launches, _ = series_run(ds, as_bytes(z), L)
        assert ds.launch_info()["lds_bytes"] == geometry()[(N, False)][2]
    assert done == K and launches == 1 and np.all(rows[:K, 0] > 0)


def test_excision_is_one_launch():
    N, L, K = 512, 8, 6
    _, z = int16_streams(7, K * L * N)
    with engine(N, "cf32") as ds:
        d = torch.from_numpy(as_bytes(z)).to(DEV)
        out, _, done = excised(ds, d, 8 * z.size, L, -np.inf, np.inf)
        assert ds.series_launches() == 1
    assert done == K and out[2].min() > 0


# ---- identity with cs16, exact scaling, one frame ---------------------------------------------------------------------------

@pytest.mark.parametrize("N,window", FORMS, ids=FORM_IDS)
def test_cf32_of_integers_equals_cs16_and_scales_exactly(N, window):
    R = 37                                     # the last iteration is partly clamped
    s16, z = int16_streams(11, R * N)
    for flags in (0, NO_DMA):
        what = "N=%d window=%s flags=%d" % (N, window, flags)
        with engine(N, "cs16", window=window, flags=flags) as a, engine(N, "cf32", window=window, flags=flags) as b:
            want, n0, g0, _ = stats_run(a, s16)
            got, n1, g1, li = stats_run(b, z)
            assert n0 == n1 == R and li["lds_bytes"] > 0
            assert same_planes(got, want, g1, g0, what)
            scaled, _, _, _ = stats_run(b, synth.to_cf32(s16, 2.0 ** -9))
            assert np.array_equal(scaled[0], got[0] * 2.0 ** -18), what
            assert np.array_equal(scaled[1], got[1] * 2.0 ** -36), what
            assert np.array_equal(scaled[2], got[2] * 2.0 ** -18), what
            one, m1, _, _ = stats_run(b, z[:N])
            assert m1 == 1 and np.all(one[0] > 0)
            assert np.array_equal(one[2], one[0]) and np.array_equal(one[1], one[0] * one[0]), what


# ---- second iteration and refill -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [64, 8192])
def test_second_iteration_of_every_workgroup(N):
    """More frames than any resident grid holds: every workgroup takes a second iteration and reads what the refill of
    its ring brought (8192: the ring of depth 1, refilled behind the unpack)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    with engine(N, "cs16") as a, engine(N, "cf32") as b:
        _, _, (_, fpw), _ = stats_run(b, synth.to_cf32(synth.noise_tones_cs16(12, N)))
        R = cus * 8 * fpw + 3                  # (no K1 kernel has more than 8 resident workgroups per CU)
        s16, z = int16_streams(13, R * N)
        want, n0, g0, _ = stats_run(a, s16)
        got, n1, g1, _ = stats_run(b, z)
    assert n0 == n1 == R
    assert R > g1[0] * g1[1] + 3, "workgroups take a second iteration"
    assert same_planes(got, want, g1, g0, "N=%d frames=%d" % (N, R))


# ---- overlapped frames: the strided kernel ---------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [512, 4096])
def test_strided_equals_cs16(N):
    R = 37
    for step in (N // 2, N // 2 + 1):          # pitch 8 S: a multiple of 16 (LDS-DMA), and not (VGPR staging)
        s16, z = int16_streams(41, N + step * (R - 1))
        with engine(N, "cs16", step) as a, engine(N, "cf32", step) as b:
            want, n0, g0, _ = stats_run(a, s16)
            got, n1, g1, li = stats_run(b, z)
        assert n0 == n1 == R == frames_in(8 * z.size, N, step, 8) and li["lds_bytes"] > 0
        assert same_planes(got, want, g1, g0, "N=%d step=%d" % (N, step))


# ---- device pointer alignment ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,window", [(512, False), (4096, True)])
def test_device_pointer_alignment(N, window):
    R = 37
    _, z = int16_streams(31, R * N)
    with engine(N, "cf32", window=window) as ds:
        want, n0, g0, _ = stats_run(ds, z)
        got, n1, g1, _ = stats_run(ds, z, misalign=8)          # 8- but not 16-byte aligned: VGPR staging
        assert n0 == n1 == R
        assert same_planes(got, want, g1, g0, "N=%d window=%s misaligned by 8" % (N, window))
        with pytest.raises(rpf.RPFError) as e:
            stats_run(ds, z, misalign=4)
        assert e.value.retval == rpf.ReturnValue.InvalidArgument


# ---- Gaussian float32 against float64 truth ---------------------------------------------------------------------------------

def cpu_frame_powers_cf32(N, z, frames, window=None):
    """p[f, b] on the CPU float32 path: rpf_oracle_fft_f32 on the frame as the kernels unpack it (the stored floats,
    (-1)^n exact, the window one float32 rounding) -- test_spectral_stats.oracle_frame_powers without its `- 127`."""
    orc = oracle_lib()
    plan = orc.rpf_oracle_plan_create(N)
    sign = (1 - 2 * (np.arange(N) % 2)).astype(np.float32)
    v = unpacked("cf32", z).reshape(-1, N, 2)
    out = np.zeros((frames, N))
    try:
        for f in range(frames):
            x = v[f] * sign[:, None]
            if window is not None:
                x = x * np.asarray(window, dtype=np.float32)[:, None]
            x = np.ascontiguousarray(x, dtype=np.float32)
            y = np.zeros((N, 2), dtype=np.float32)
            orc.rpf_oracle_fft_f32(plan, x.ctypes.data_as(fp), y.ctypes.data_as(fp))
            re, im = y[:, 0].astype(np.float64), y[:, 1].astype(np.float64)
            out[f] = re * re + im * im
    finally:
        orc.rpf_oracle_plan_destroy(plan)
    return out


@pytest.mark.parametrize("N,window", [(64, False), (512, False), (1024, True), (4096, True), (8192, False)])
def test_gaussian_cf32_statistics_against_truth(N, window):
    """S1 within CF32_VS_TRUTH of numpy complex128; S2 and PK within STATS_TIMES_CPU_ERR times the CPU float32 path's own
    worst-bin error on the same frames; SK within its first-order bound (stats_bars.SK_SLACK): judge() of
    test_gpu_spectral_stats on the figures of test_gpu_k1_forms.figures_of.  cf32_stats_bars.MEASURED records them."""
    R = 80
    z = synth.gaussian_cf32(21, R * N)
    w = synth.hann_window(N) if window else None
    truth = planes(truth_frame_powers(N, unpacked("cf32", z), R, w))
    cpu = planes(cpu_frame_powers_cf32(N, z, R, w))
    with engine(N, "cf32", window=window) as ds:
        gpu, n, _, li = stats_run(ds, z)
    assert n == R and li["lds_bytes"] > 0
    fig = figures_of(gpu, truth, cpu, cpu[0], R, N=N, window=bool(window), format="cf32")
    judge(fig)                                 # (prints the figures)
    assert fig["gpu_vs_truth"]["S1"] < CF32_VS_TRUTH


# ---- the series of statistics ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, NO_DMA], ids=["lds_dma", "vgpr"])
@pytest.mark.parametrize("window", [False, True], ids=["rect", "hann"])
@pytest.mark.parametrize("N", [64, 512, 2048, 8192])
def test_series_of_statistics(N, window, flags):
    """K from the engine's own plan, so that the launch's iterations exceed the resident grid by a quarter: workgroup
    ranges cut spectra and the fix-up kernel runs.  L is no multiple of the frames per workgroup (at 8192, one frame per
    workgroup, there is no such L: 3); a tail of L - 1 frames follows the last spectrum."""
    what = "N=%d window=%s flags=%d" % (N, window, flags)
    with engine(N, "cs16", window=window, flags=flags) as a, engine(N, "cf32", window=window, flags=flags) as b:
        li = b.launch_info()                   # (before any launch: the resident grid of the plan)
        grid, fpw = li["grid"], li["frames_per_wg"]
        L = 3 * fpw + 1 if fpw > 1 else 3
        K = series_plan(grid, fpw, L)
        s16, z = int16_streams(29, (K * L + L - 1) * N)
        got, done, launches, g1 = series_run(b, as_bytes(z), L)
        assert done == K and launches == 1, what
        assert K * -(-L // g1[1]) > g1[0], "%s: more iterations than workgroups" % what
        assert np.all(got[K:] == -1.0), "%s: rows >= K were touched" % what
        again, _, _, _ = series_run(b, as_bytes(z), L)
        assert got.tobytes() == again.tobytes(), "%s: two runs" % what
        want, dw, lw, g0 = series_run(a, s16, L)
        assert dw == K and lw == 1
        assert np.array_equal(got[:K, 2], want[:K, 2]), "%s: PK vs cs16" % what
        assert same(got[:K, 0], want[:K, 0], g1, g0, what + " S1 vs cs16")
        assert same(got[:K, 1], want[:K, 1], g1, g0, what + " S2 vs cs16")
        slices = slice_rows(b, as_bytes(z), L, K)
    e1, e2 = max_rel(got[:K, 0], slices[:, 0]), max_rel(got[:K, 1], slices[:, 1])
    print("%s: L=%d K=%d geometry=%s vs slices: S1 %.3g S2 %.3g (bar %g)" % (what, L, K, g1, e1, e2, ADDITIVITY))
    assert e1 < ADDITIVITY and e2 < ADDITIVITY
    assert np.array_equal(got[:K, 2], slices[:, 2]), "%s: PK vs slices" % what


# ---- excision ----------------------------------------------------------------------------------------------------------------

def test_excision_against_the_engines_own_rows():
    N, L, K = 512, 8, 40
    _, z = int16_streams(91, K * L * N)
    lo, hi = stats.sk_limits(L, 1.0)
    with engine(N, "cf32") as ds:
        d = torch.from_numpy(as_bytes(z)).to(DEV)
        rows, launches = series_rows(ds, d, 8 * z.size, L, K)
        assert launches == 1
        want, want_mask = stats.excise(rows, L, lo, hi)
        got, mask, done = excised(ds, d, 8 * z.size, L, lo, hi)
        assert done == K and ds.series_launches() == 1
        everything, _, _ = excised(ds, d, 8 * z.size, L, -np.inf, np.inf)
    assert 0 < want_mask.sum() < want_mask.size, "the case takes both branches"
    assert np.array_equal(mask, want_mask) and np.array_equal(got[1], want[1])
    e_clean, e_total = err_over_total(got[0], want[0], want[2]), err_over_total(got[2], want[2], want[2])
    print("N=%d L=%d K=%d: %d of %d flagged, clean %.3g total %.3g (bar %g)"
          % (N, L, K, int(want_mask.sum()), want_mask.size, e_clean, e_total, ADDITIVITY))
    assert e_clean < ADDITIVITY and e_total < ADDITIVITY
    assert everything[2].min() > 0 and np.array_equal(everything[0], everything[2])


# ---- the queue path ----------------------------------------------------------------------------------------------------------

def test_queue_path():
    N, R, buf_length = 4096, 37, 16384 + 8
    _, z = int16_streams(61, R * N + N // 3)
    assert buf_length % 8 == 0 and buf_length % (8 * N) != 0
    with engine(N, "cf32", buf_length=buf_length, repeats=1 << 40) as ds:
        want, n, _, li = stats_run(ds, z)
        pwr, done = ds.accumulate(z)
        s2, pk = ds.sum_sq.copy(), ds.peak.copy()
    assert done == n == R and li["lds_bytes"] > 0
    e1, e2 = max_rel(pwr, want[0]), max_rel(s2, want[1])
    print("N=%d: queue vs device S1 %.3g S2 %.3g (bar %g)" % (N, e1, e2, SAME_KERNELS))
    assert e1 < SAME_KERNELS and e2 < SAME_KERNELS
    assert np.array_equal(pk, want[2])


# ---- NaN ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def impulse_frames(N, frames):
    """Frame f = one sample a_f at n = 0, zeros elsewhere: X[k] = a_f in every bin, and every float32 transform computes
    it exactly (the twiddles that meet the one non-zero input are W^0 = 1), so two routes agree bit for bit."""
    z = np.zeros(frames * N, dtype=np.complex64)
    z[::N] = (np.arange(frames) % 5 + 1) * (3.0 + 2.0j)      # frame 4 is the loudest; frame 3 takes the NaN
    return z


def nan_sets(s):
    return [np.isnan(s[i]) for i in range(3)]


def test_a_nan_does_what_it_does_on_the_catch_all_route():
    """One NaN sample in frame 3 of 8 reaches every bin of that frame's spectrum: S1 and S2 are NaN, PK -- a maximum,
    fmax drops a NaN operand -- is the peak of the other frames.  The same on both routes: the sets of NaN entries are
    equal, plane by plane.  The finite entries of PK are equal bit for bit on frames both transforms compute exactly
    (impulse_frames; under the Hann window, w[0] = 0, they are zeros); on noise the two float32 transforms differ by their rounding, and the finite entries agree within
    cf32_stats_bars.NAN_ROUTES_PK."""
    N, R = 512, 8
    for name, z in (("impulses", impulse_frames(N, R).copy()), ("noise", int16_streams(71, R * N)[1].copy())):
        z[3 * N + 17] = np.complex64(complex(np.nan, z[3 * N + 17].imag))
        for window in (False, True):
            with engine(N, "cf32", window=window) as a, engine(N, "cf32", window=window, flags=CATCH_ALL) as b:
                got, n0, _, li = stats_run(a, z)
                want, n1, _, lj = stats_run(b, z)
            assert n0 == n1 == R and li["lds_bytes"] > 0 and lj["lds_bytes"] == 0
            for i, plane in enumerate(("S1", "S2", "PK")):
                assert np.array_equal(np.isnan(got[i]), np.isnan(want[i])), (name, window, plane)
            assert np.all(np.isnan(got[0])) and np.all(np.isnan(got[1])) and not np.any(np.isnan(got[2]))
            finite = np.isfinite(got[2])
            assert np.array_equal(finite, np.isfinite(want[2]))
            if name == "impulses":
                assert np.array_equal(got[2][finite], want[2][finite]), window
                assert window or np.all(got[2] == 25.0 * 13.0), "the loudest frame that is not the NaN frame: a = 5 (3 + 2j)"
            else:
                err = max_err_over_mean(got[2][finite], want[2][finite])
                print("%s window=%s: PK of the two routes %.3g (bar %g)" % (name, window, err, NAN_ROUTES_PK))
                assert err < NAN_ROUTES_PK


# ---- the CLI -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [["--stats"], ["--series-stats", "16"], ["--excise", "16"]], ids=["stats", "series-stats", "excise"])
def test_cli_prints_for_cf32_what_it_prints_for_cs16(tmp_path, mode):
    """rpf_power needs no new option: `--format cf32` with --stats, --series-stats and --excise prints the blocks it
    prints for the cs16 file of the same int16 values -- every column within one unit of its last printed digit (the two
    engines may group their sums differently)."""
    N, L, K = 512, 16, 6
    s16, z = int16_streams(33, N * K * L)
    (tmp_path / "rec.cs16").write_bytes(s16.tobytes())
    (tmp_path / "rec.cf32").write_bytes(z.tobytes())
    out = {}
    for fmt in ("cs16", "cf32"):
        count = ["-n", str(K * L)] if mode == ["--stats"] else []          # (the other two take every frame of the file)
        r = subprocess.run([CLI, "-b", str(N), "-q", "--input", str(tmp_path / ("rec." + fmt)), "--format", fmt] + count + mode,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out[fmt] = blocks_of(r.stdout)
    assert len(out["cf32"]) == len(out["cs16"]) >= 1
    worst = 0.0
    for g, w in zip(out["cf32"], out["cs16"]):
        assert len(g) == len(w) == N
        for rg, rw in zip(g, w):
            assert len(rg) == len(rw) >= 3 and rg[0] == rw[0]
            for vg, vw in zip(rg[1:], rw[1:]):
                unit = max(one_unit_of_the_last_digit(vg), one_unit_of_the_last_digit(vw))
                worst = max(worst, abs(float(vg) - float(vw)) / unit)
                assert abs(float(vg) - float(vw)) <= unit * (1 + 1e-9), (vg, vw)
    print("%s: %d blocks, worst difference %.3g units of the last printed digit" % (" ".join(mode), len(out["cf32"]), worst))
