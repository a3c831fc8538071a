"""Every shipped run of the mixed-radix family past its first loop iteration, on the MI355X, against float64.

mixed_plan_kernel, mixed_split_kernel and the run-time Stockham mixed_kernel (rpf_mixed.hip, mixed_plan_kernels.h) are
persistent frame loops: accumulators, twiddles and window values stay in registers for the launch, the next iteration's
samples are fetched while the later passes run, one LDS slab is reused behind the barriers, the split form carries a
section across the loop edge, a ragged last iteration is masked while its loads are clamped to the last frame.
launch_mixed trims the grid to the frames, so the runs of 3 to 64 frames the other tests make never loop.  Here every
(size, window) of mixed_plans.inc and mixed_plans_split.inc -- find_form picks the form, so the moves of
mixed_plans_override.inc are among them -- and six Stockham sizes of 2 to 8 passes run F = 2 I + I / 2 + 1 frames, I =
(grid / P) x frames_per_wg the frames of one iteration of the resident grid: two full iterations and a third in which
about half the workgroups run, the last of them with idle slots.

The stream gathers a pool of 64 distinct frames by a seeded index sequence without a period (tests/test_mixed_loop.py,
which also shows on the CPU that a frame read twice or from the wrong iteration moves the truth), so the float64 truth
is sum_d count[d] |FFT64(pool frame d)|^2 at the cost of 64 transforms.  Judged per case, every bar from parity_bars:

  1. the whole run against that truth, per bin, at the bar the size is held to at 53 to 64 frames (test_mixed_loop.table_bar);
  2. the whole run against the sum of its parts of at most I frames, each a first-iteration launch from its own device
     pointer -- the ground the other tests stand on -- within ADDITIVITY;
  3. a second whole run, bit for bit (a race shows as a run-to-run difference);
  4. for the sizes of mixed_plans.inc that no other GPU test launches, the first part against the Bluestein engine of the
     size (FLAG_NO_MIXED_RADIX) within PARITY.

Each test prints N, the form, the geometry, the bytes and the figures it judged; tools/gpu_mixed_loop.py writes them to
profiles/mixed_loop.json."""
import time

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib
from helpers import max_rel
from parity_bars import ADDITIVITY, PARITY
import test_gpu_parity
import test_mixed_loop as loop
from test_mixed_loop import CASES, case_id

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")


def _sizes_of(test):
    (mark,) = [m for m in test.pytestmark if m.name == "parametrize" and m.args[0] == "N"]
    return set(mark.args[1])


# the sizes of mixed_plans.inc that tests/test_gpu_parity.py launches on their mixed-radix kernel
LAUNCHED_ELSEWHERE = (_sizes_of(test_gpu_parity.test_mixed_radix_sizes_match_oracle_and_bluestein)
                      | _sizes_of(test_gpu_parity.test_non_power_of_two_sizes_match_oracle)
                      | _sizes_of(test_gpu_parity.test_large_non_power_of_two_sizes_match_oracle)) & set(loop.planned_table())
ONLY_HERE = set(loop.planned_table()) - LAUNCHED_ELSEWHERE


def cuda_stream():
    return torch.cuda.current_stream().cuda_stream


def engine(N, windowed, flags=0):
    return rpf.Datastore(rpf.Params(N=N, window=windowed, buffers=2, buf_length=16384), loop.loop_window(N, windowed), flags=flags)


def power(ds, ptr, frames, out):
    """accumulate_device over `frames` frames at device address ptr; the N doubles on the host."""
    n = ds.accumulate_device(ptr, ds.frame_span(frames), frames, out.data_ptr(), cuda_stream())
    torch.cuda.synchronize()
    assert n == frames
    return out.cpu().numpy()


def resident_grid(ds):
    """launch_info of the resident grid: runs over zeros, four times the frames each, until the frames and not the grid
    are the more (test_gpu_stft.resident_grid, through accumulate_device)."""
    frames = 64
    out = torch.empty(ds.params.N, dtype=torch.float64, device=DEV)
    while True:
        z = torch.zeros(ds.frame_span(frames), dtype=torch.uint8, device=DEV)
        power(ds, z.data_ptr(), frames, out)
        li = ds.launch_info()
        if li["grid"] * li["frames_per_wg"] < frames:
            return li
        frames *= 4
        assert frames <= 1 << 22


def loop_figures(case):
    """One case, run and measured: the record tools/gpu_mixed_loop.py keeps and the test judges."""
    N, windowed = case
    t0 = time.time()
    P = 1 if case in loop.NOT_MIXED else loop.split_factor(N, windowed)
    pool = loop.pool_frames(N)
    p = loop.pool_powers(N, windowed, pool)
    with engine(N, windowed) as ds:
        li = resident_grid(ds)
        grid, fpw = li["grid"], li["frames_per_wg"]
        assert grid % P == 0 and (P == 1 or fpw == 1)
        I = (grid // P) * fpw
        F = loop.frames_of(I, fpw)
        idx = loop.index_sequence(N, F)
        counts = loop.counts_of(idx)
        stream = torch.from_numpy(pool).to(DEV)[torch.from_numpy(idx).to(DEV)].reshape(-1)
        assert stream.is_contiguous() and stream.numel() == ds.frame_span(F) == 2 * N * F
        out = torch.full((N,), float("nan"), dtype=torch.float64, device=DEV)
        whole = power(ds, stream.data_ptr(), F, out)
        judged_grid = ds.launch_info()["grid"]
        cuts = loop.parts_of(F, I)
        parts = []
        for a, b in cuts:
            out.fill_(float("nan"))
            parts.append(power(ds, stream.data_ptr() + 2 * N * a, b - a, out))
        out.fill_(float("nan"))
        again = power(ds, stream.data_ptr(), F, out)
        fused = bool(ds.fused_status()["active"])
    truth = counts @ p
    bar, which = loop.bar_against_truth(case, counts, p, pool)
    stale, extra = loop.wrong_frame_shifts(idx, I, p)
    rec = {"N": N, "windowed": windowed, "form": loop.form_of(N, windowed), "grid": grid, "frames_per_wg": fpw, "P": P, "I": I,
           "F": F, "bytes": int(stream.numel()), "judged_grid": judged_grid, "parts": [b - a for a, b in cuts],
           "pool_frames_in_the_smallest_part": int(min(np.unique(idx[a:b]).size for a, b in cuts)),
           "whole_vs_truth": max_rel(whole, truth), "bar": bar, "bar_is": which,
           "whole_vs_parts": max_rel(whole, sum(parts)), "second_run_equal": bool(np.array_equal(whole, again)),
           "second_run_vs_first": max_rel(again, whole), "fused_four_step": fused,
           "stale_prefetch_would_move_truth_by": stale, "unmasked_slot_would_move_truth_by": extra}
    if N in ONLY_HERE:
        with engine(N, windowed, flags=_lib.FLAG_NO_MIXED_RADIX) as blu:
            other = power(blu, stream.data_ptr(), cuts[0][1], out)
        rec["first_part_vs_bluestein"] = max_rel(parts[0], other)
    rec["seconds"] = round(time.time() - t0, 3)
    return rec


def describe(r):
    s = ("N=%d %s, %s: grid %d x %d frames, P=%d, I=%d, F=%d in parts %s, %d bytes, %.2f s; whole against float64 %.3g (bar %.3g, "
         "%s); against the sum of the parts %.3g (ADDITIVITY %.0e); second run %s; a stale prefetch would move the truth by "
         "%.3g, an unmasked slot by %.3g; the smallest part holds %d of the pool's frames"
         % (r["N"], "windowed" if r["windowed"] else "plain", r["form"], r["grid"], r["frames_per_wg"], r["P"], r["I"], r["F"],
            r["parts"], r["bytes"], r["seconds"], r["whole_vs_truth"], r["bar"], r["bar_is"], r["whole_vs_parts"], ADDITIVITY,
            "bit for bit" if r["second_run_equal"] else "differs by %.3g" % r["second_run_vs_first"],
            r["stale_prefetch_would_move_truth_by"], r["unmasked_slot_would_move_truth_by"],
            r["pool_frames_in_the_smallest_part"]))
    if "first_part_vs_bluestein" in r:
        s += "; first part against the Bluestein engine %.3g (PARITY %.0e)" % (r["first_part_vs_bluestein"], PARITY)
    return s


def test_the_sizes_no_other_test_launches():
    print("%d of the %d sizes of mixed_plans.inc run on the GPU in tests/test_gpu_parity.py; the other %d get the "
          "Bluestein cross-check here" % (len(LAUNCHED_ELSEWHERE), len(loop.planned_table()), len(ONLY_HERE)))
    assert len(ONLY_HERE) + len(LAUNCHED_ELSEWHERE) == len(loop.planned_table()) and len(ONLY_HERE) >= 83


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_two_and_a_half_iterations_against_float64_and_the_sum_of_the_parts(case):
    """Measured on the MI355X (profiles/mixed_loop.json, 430 cases, 256 compute units): I from 24 (80000 bins, 10 x 8000) to
    65536 frames, streams of 0.2 to 21 MB (108000 bins: 17.5 MB, I = 32 -- the resident grid of 256 is shared by P = 8
    residues; the four-step run of 32768 windowed: 42 MB), 0.26 s for the slowest case.  Whole against float64 at most
    0.47 of its bar (4374 windowed, Stockham, 8 passes); against the sum of the parts at most 9.5e-16; all 430 second
    runs bit for bit; first part against Bluestein at most 4.9e-7 (6500 windowed).  At these geometries a stale prefetch
    would have moved the truth by at least 9300 bars and one unmasked slot by at least 49 (50 bins, F = 163201).  A build
    with the mistakes put in on purpose -- the slot mask of the planned and the Stockham kernel dropped, the split
    form's fetch-ahead reading the frame in hand -- failed assertion 1 in all 179 cases with more than one slot (by 1400
    bars at least) and all 151 split-form cases (assertion 2 as well); with one slot there is nothing to mask."""
    r = loop_figures(case)
    print(describe(r))
    assert r["judged_grid"] == r["grid"], "the judged launch ran the resident grid"
    assert r["F"] > 2 * r["I"] + r["I"] // 2 and len(r["parts"]) == 3
    assert r["frames_per_wg"] == 1 or r["F"] % r["frames_per_wg"], "the last workgroup has idle slots"
    assert r["fused_four_step"] == (case in loop.NOT_MIXED)
    assert r["whole_vs_truth"] < r["bar"]
    assert r["whole_vs_parts"] < ADDITIVITY
    if case in loop.NOT_MIXED:
        # the fused four-step kernel's teams add their rounds in the order they finish (tests/test_gpu_engine_families.py):
        # its runs are equal as sums of the same doubles regrouped, not bit for bit
        assert r["second_run_vs_first"] < ADDITIVITY
    else:
        assert r["second_run_equal"]
    if case[0] in ONLY_HERE:
        assert r["first_part_vs_bluestein"] < PARITY
