"""The batch and chunk seams of the catch-all route on the MI355X, with every sample format and with statistics.

launch_generic (rpf_generic.hip) runs an acquisition in batches of B = generic_batch(N) frames.  From the second batch on
the source pointer advances by B b N bytes (b bytes per sample of the format), the accumulate kernels read back what the
first batch left in S1, S2 and PK, and the peak hold carries its maximum over.  One level up launch_gathered
(rpf_engine.cpp) cuts overlapped frames into chunks of 64 MB that add into the output by +, +, max; and the quantile
selection (rpf_quantile.hip) walks the bins in chunks of 32768 and is instantiated for 1 .. 8 quantiles per call.  Every
other GPU test of a format other than cu8, or with statistics, stays inside the first batch, the first chunk and the
instantiations for 1, 3 and 8 quantiles.  Here every seam is crossed:

  1. 2 B + 5 frames (three batches, the last ragged) at four sizes x four formats x two windows x statistics off / on;
  2. the spectrum-by-spectrum series of statistics with rows of 2 B + 5 frames;
  3. two chunks of gathered frames, cs16 with statistics and windowed cf32, at a pitch that is no multiple of 16 bytes;
  4. the quantile selection over two chunks of bins, and with 1 .. 8 quantiles per call.

What is asserted is exact wherever the engine promises it -- np.array_equal for PK against the maximum of the parts, for
a second run, for S1 of a stats engine against the plain engine, for the ties cs8 == cu8, cs16 == cs8 on 8-bit values,
cf32 == cs16 on 16-bit values, for the series' rows and for the quantiles -- ADDITIVITY where the same doubles are added
in another grouping (the whole run against the sum of its parts, each part a single batch from its own device pointer),
and against float64 the bars the route is already held to: PARITY relative to max(bin, median bin) for S1, and for S2
and PK STATS_TIMES_CPU_ERR times the CPU float32 path's own worst-bin error on the same frames.  At the Bluestein lengths
(500, 40000) the last of these is printed and recorded, not asserted: a Bluestein run is two transforms of length M and
three table products where the CPU path has one transform of length N, and the recorded ratios (profiles/
seams_errors.json, 69 and 133 frames) reach 3.6 for S2 and 2.6 for PK at 500 bins, 1.8 and 1.2 at 40000 -- errors of
5.4e-7 ... 1.3e-6 against the CPU path's 2.0e-7 ... 1.8e-6.  They would have been asserted at the project's factor had
every one been under 1.5; S2 and PK are carried there by the exact comparisons.  Every threshold is
imported from parity_bars / stats_bars; tests/test_seams.py checks on the CPU what is taken for granted here (B, the
chunk lengths, the reference's own whole-against-parts difference, filled bins).  tools/gpu_seams.py records the figures
of section 1 in profiles/seams_errors.json.  Each test prints the batch or chunk length it read and the count it ran."""
import functools

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, stats, synth
from frame_truth import planes, unpacked
from helpers import max_err_over_mean, max_rel
from parity_bars import ADDITIVITY, PARITY
from stats_bars import STATS_TIMES_CPU_ERR
from test_gpu_cf32_stats import K1_SIZES, as_bytes, stats_run
from test_gpu_k1_forms import cpu_frame_powers
from test_gpu_quantile import Q8, check_against_rows, noise, same, select_device, series_rows
from test_gpu_quantile import engine as quantile_engine
from test_gpu_quantile import to_device as quantile_to_device
from test_gpu_sample_formats import device_run, truth_signed
from test_gpu_series_stats import series_run
from test_seams import (BATCH, FORMATS, GATHER_CHUNK, GATHER_FRAMES, QUANTILE_CHUNK, SEEDS, family_of, frames_of,
                        gather_materialised, gather_step, gather_stream, seam_window, stream_of, transform_length,
                        truth_powers)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
CATCH_ALL = _lib.FLAG_CATCH_ALL
NAMES = ("S1", "S2", "PK")

CASES = [(N, fmt, windowed, with_stats) for N in sorted(BATCH) for fmt in FORMATS for windowed in (False, True)
         for with_stats in (False, True)]
CASE_IDS = ["%d-%s-%s-%s" % (N, fmt, "raised_hann" if w else "rect", "stats" if s else "plain") for N, fmt, w, s in CASES]


def seam_engine(N, fmt, windowed=False, with_stats=False, step=None):
    """An engine on the catch-all route: cu8, and every format at a size K1 serves, has to ask for it."""
    flags = CATCH_ALL if fmt == "cu8" or N in K1_SIZES else 0
    w = seam_window(N) if windowed else None
    return rpf.Datastore(rpf.Params(N=N, window=windowed, frame_step=step, sample_format=fmt, bin_stats=with_stats), w,
                         flags=flags)


def run(ds, stream):
    """(planes (1, N) or (3, N), frames, launch_info) of one device-resident acquisition of the bytes `stream`, copied to
    a device buffer of its own."""
    if ds.has_bin_stats:
        out, n, _, li = stats_run(ds, stream)
        return out, n, li
    out, n, _ = device_run(ds, stream)
    return out[None, :], n, ds.launch_info()


def combine(parts):
    """S1 and S2 add, PK takes the maximum."""
    out = np.sum(parts, axis=0)
    if out.shape[0] == 3:
        out[2] = np.max([p[2] for p in parts], axis=0)
    return out


@functools.lru_cache(maxsize=2)
def cpu_planes(family, N, windowed):
    """S1, S2, PK of the CPU float32 path on the family's frames."""
    fmt = "cu8" if family == "8" else "cs16"
    return planes(cpu_frame_powers(N, fmt, stream_of(fmt, N), frames_of(N), seam_window(N) if windowed else None))


def tie_of(N, fmt, windowed, with_stats):
    """(what, planes, frames) of the run a format is tied to bit for bit, on the stream that says the same thing."""
    if fmt == "cs8":
        with seam_engine(N, "cu8", windowed, with_stats) as ds:
            return ("cu8 on the catch-all route",) + run(ds, stream_of("cu8", N))[:2]
    if fmt == "cf32":
        with seam_engine(N, "cs16", windowed, with_stats) as ds:
            return ("cs16",) + run(ds, stream_of("cs16", N))[:2]
    assert fmt == "cs16"
    with seam_engine(N, "cs8", windowed, with_stats) as ds:
        return ("cs8",) + run(ds, stream_of("cs8", N))[:2]


def batch_seam_figures(N, fmt, windowed, with_stats):
    """One case of section 1: what the engine reported, every exact comparison as a flag, every other as its figure."""
    R = frames_of(N)
    stream = stream_of(fmt, N)
    frame = _lib.SAMPLE_BYTES[fmt] * N
    fig = {"N": N, "format": fmt, "window": "raised_hann" if windowed else "rect", "statistics": bool(with_stats),
           "transform": "power_of_two" if transform_length(N) == N else "bluestein", "frames": R}
    with seam_engine(N, fmt, windowed, with_stats) as ds:
        whole, n, li = run(ds, stream)
        B = li["frames_per_wg"]
        fig.update(batch=B, frames_done=n, lds_bytes=li["lds_bytes"])
        if (B, n, li["lds_bytes"]) != (BATCH[N], R, 0) or R <= 2 * B:
            return fig                                        # another route, or the seam is not crossed: the test fails
        cuts = ((0, B), (B, 2 * B), (2 * B, R))
        parts = [run(ds, stream[a * frame:b * frame]) for a, b in cuts]
        again, _, _ = run(ds, stream[2 * B * frame:])
        if fmt == "cs16":                                     # cs16 of 8-bit values, on this engine
            eight, n8, _ = run(ds, synth.to_cs16(stream_of("cs8", N)))
    fig["parts_frames"] = [p[1] for p in parts]
    summed = combine([p[0] for p in parts])
    fig["whole_vs_parts"] = {k: max_rel(whole[i], summed[i]) for i, k in enumerate(NAMES[:whole.shape[0]]) if k != "PK"}
    if with_stats:
        fig["pk_is_the_maximum_of_the_parts"] = bool(np.array_equal(whole[2], summed[2]))
    fig["second_run_of_the_last_part_equal"] = bool(np.array_equal(again, parts[2][0]))
    if with_stats:
        with seam_engine(N, fmt, windowed, False) as plain:
            power, n_plain, _ = run(plain, stream)
        fig["s1_is_the_plain_engines_power"] = bool(n_plain == R and np.array_equal(whole[0], power[0]))
    if fmt != "cu8":
        what, want, n_tie = tie_of(N, fmt, windowed, with_stats)
        got = eight if fmt == "cs16" else whole
        fig["tie"] = {"with": what, "equal": bool(n_tie == R and (fmt != "cs16" or n8 == R) and np.array_equal(got, want))}
    truth = planes(truth_powers(family_of(fmt), N, windowed))
    fig["S1_err_over_mean"] = max_err_over_mean(whole[0], truth[0])
    if with_stats:
        cpu = cpu_planes(family_of(fmt), N, windowed)
        g = {k: max_rel(whole[i], truth[i]) for i, k in enumerate(NAMES)}
        c = {k: max_rel(cpu[i], truth[i]) for i, k in enumerate(NAMES)}
        fig.update(gpu_vs_truth=g, cpu_f32_vs_truth=c, gpu_over_cpu={k: g[k] / c[k] for k in ("S2", "PK")})
    return fig


# ---- 1. the batch seam of launch_generic ---------------------------------------------------------------------------------

@pytest.mark.parametrize("N,fmt,windowed,with_stats", CASES, ids=CASE_IDS)
def test_batch_seam(N, fmt, windowed, with_stats):
    fig = batch_seam_figures(N, fmt, windowed, with_stats)
    print(fig)
    B, R = fig["batch"], fig["frames"]
    assert fig["lds_bytes"] == 0, "the catch-all route keeps nothing in LDS"
    assert B == BATCH[N] and R == 2 * B + 5 and fig["frames_done"] == R
    assert fig["parts_frames"] == [B, B, 5], "each part is a single batch"
    for k, err in fig["whole_vs_parts"].items():
        assert err < ADDITIVITY, (k, err)
    assert fig["second_run_of_the_last_part_equal"], "the partial planes start from 0, 0, 0 in every launch"
    if with_stats:
        assert fig["pk_is_the_maximum_of_the_parts"]
        assert fig["s1_is_the_plain_engines_power"]
    if fmt != "cu8":
        assert fig["tie"]["equal"], fig["tie"]["with"]
    assert fig["S1_err_over_mean"] < PARITY
    if with_stats and fig["transform"] == "power_of_two":       # (the Bluestein lengths: recorded, see the module docstring)
        g, c = fig["gpu_vs_truth"], fig["cpu_f32_vs_truth"]
        assert g["S2"] <= STATS_TIMES_CPU_ERR * c["S2"], ("S2", g["S2"], c["S2"])
        assert g["PK"] <= STATS_TIMES_CPU_ERR * c["PK"], ("PK", g["PK"], c["PK"])


# ---- 2. the fallback series across the batch seam ------------------------------------------------------------------------

def test_fallback_series_across_the_batch_seam():
    """test_gpu_series_stats.test_fallback_is_the_stats_path_bit_for_bit with rows of three batches: what the rows of
    --series-stats, --excise and --quantile are made of at such a size."""
    N, K = 500, 3
    L = frames_of(N)
    stream = as_bytes(synth.noise_tones_cs16(SEEDS["16"] + 1, K * L * N))
    row = _lib.SAMPLE_BYTES["cs16"] * N * L
    with seam_engine(N, "cs16", True, True) as ds:
        rows, done, launches, (_, B) = series_run(ds, stream, L)
        li = ds.launch_info()
        print("N=%d cs16 raised Hann: batch %d, rows of %d frames, %d rows in %d launches" % (N, B, L, done, launches))
        assert B == BATCH[N] and L == 2 * B + 5 and li["lds_bytes"] == 0
        assert done == K and launches == K == ds.series_launches()
        assert np.all(rows[K:] == -1.0), "rows >= K were touched"
        for k in range(K):
            want, n, _, _ = stats_run(ds, stream[k * row:(k + 1) * row])
            assert n == L and np.array_equal(rows[k], want), k


# ---- 3. the gather chunk seam ---------------------------------------------------------------------------------------------

def gather_seam_figures(fmt, N, with_stats, windowed):
    """One case of section 3: the gathered run of GATHER_FRAMES overlapped frames against the materialised stream on a
    step-N engine, and against float64."""
    b, step, R = _lib.SAMPLE_BYTES[fmt], gather_step(fmt, N), GATHER_FRAMES
    chunk = (64 << 20) // (b * N)
    X = gather_stream(fmt, N)                                  # (white: test_seams.gather_stream says why)
    Xp = gather_materialised(fmt, N, X)
    assert X.size == b * (N + step * (R - 1)) and Xp.size == b * N * R
    with seam_engine(N, fmt, windowed, with_stats) as ref:    # (one engine after the other: 67 MB of frames each)
        want, n0, li0 = run(ref, Xp)
    with seam_engine(N, fmt, windowed, with_stats, step=step) as ds:
        got, n, li = run(ds, X)
    truth = truth_signed(N, unpacked(fmt, Xp), R, seam_window(N) if windowed else None)
    fig = {"N": N, "format": fmt, "window": "raised_hann" if windowed else "rect", "statistics": bool(with_stats),
           "frames": R, "frames_done": [n, n0], "chunk": chunk, "step": step, "pitch_bytes": b * step,
           "batch": li["frames_per_wg"], "lds_bytes": [li["lds_bytes"], li0["lds_bytes"]],
           "gathered_vs_materialised": {k: max_rel(got[i], want[i]) for i, k in enumerate(NAMES[:got.shape[0]]) if k != "PK"},
           "S1_err_over_mean": max_err_over_mean(got[0], truth)}
    if with_stats:
        fig["pk_equal"] = bool(np.array_equal(got[2], want[2]))
    return fig


@pytest.mark.parametrize("fmt,N,with_stats,windowed", sorted(GATHER_CHUNK))
def test_gather_chunk_seam(fmt, N, with_stats, windowed):
    """test_gpu_frame_overlap.test_gather_path_in_several_chunks with 4- and 8-byte samples, statistics, a window, and a
    pitch the 16-byte copy cannot take."""
    fig = gather_seam_figures(fmt, N, with_stats, windowed)
    print(fig)
    R = fig["frames"]
    assert R > fig["chunk"] and fig["pitch_bytes"] % 16 != 0
    assert fig["frames_done"] == [R, R] and fig["lds_bytes"] == [0, 0]
    for k, err in fig["gathered_vs_materialised"].items():
        assert err < ADDITIVITY, (k, err)
    if with_stats:
        assert fig["pk_equal"]
    assert fig["S1_err_over_mean"] < PARITY


# ---- 4. the quantile selection's bin chunks and NQ forms -----------------------------------------------------------------

@pytest.mark.parametrize("N,cap", [(36000, 3728), (65536, 2048)])
def test_quantile_selection_over_two_chunks_of_bins(N, cap):
    """36000: a second chunk of 3232 bins, 50 tiles and a half; 65536: two full chunks.  The rows are the engine's own."""
    L, K = 1, 9
    stream = noise("cu8", 171, N * K * L)
    with quantile_engine(N) as ds:
        assert ds.quantile_max_rows == cap
        assert QUANTILE_CHUNK < N <= 2 * QUANTILE_CHUNK
        print("N=%d: chunks of %d and %d bins, %d rows" % (N, QUANTILE_CHUNK, N - QUANTILE_CHUNK, K))
        check_against_rows(ds, stream, L, K, "N=%d" % N, K)
        # a reference nobody here wrote: with K = 9 the quantiles 0, 1/4, 1/2, 3/4, 1 are order statistics themselves
        d = quantile_to_device(stream)
        rows, launches = series_rows(ds, d, stream.size, L, K)
        assert launches == K and ds.quantile_rows == K
        got = select_device(ds, [0, 0.25, 0.5, 0.75, 1])
    assert same(got, np.sort(rows, axis=0)[[0, 2, 4, 6, 8]])
    assert same(got, stats.quantiles(rows, [0, 0.25, 0.5, 0.75, 1]))


def test_every_number_of_quantiles_per_call():
    """The count and above kernels are instantiated for 1 .. 8 quantiles: each gives the planes the eight give."""
    N, L, K = 512, 4, 33
    stream = noise("cu8", 181, N * K * L)
    with quantile_engine(N) as ds:
        d = quantile_to_device(stream)
        rows, _ = series_rows(ds, d, stream.size, L, K)
        assert ds.quantile_append_device(d.data_ptr(), stream.size, L, K, torch.cuda.current_stream().cuda_stream) == K
        eight = select_device(ds, Q8)
        assert same(eight, stats.quantiles(rows, Q8))
        for nq in range(1, 9):
            assert same(select_device(ds, Q8[:nq]), eight[:nq]), nq
    print("N=%d K=%d: 1 .. 8 quantiles per call give the first planes of the eight" % (N, K))
