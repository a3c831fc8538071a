"""The frame loops of the mixed-radix family, without a GPU: what tests/test_gpu_mixed_loop.py takes for granted.

Every kernel of the family (mixed_plan_kernel, mixed_split_kernel, the run-time Stockham mixed_kernel; rpf_mixed.hip,
mixed_plan_kernels.h) is a persistent loop over frames with state that lives across iterations, and launch_mixed trims the
grid to the frames: a run of up to grid x frames_per_wg frames never enters a second iteration.  The GPU tests run two
and a half iterations of every shipped run, built by gathering a pool of POOL distinct frames by a seeded index sequence,
and compare with sum_d count[d] |FFT64(pool frame d)|^2.  Here, on the CPU:

  * the case list, read from the tables the library is compiled from (mixed_plans.inc, mixed_plans_split.inc, the
    split factors of mixed_plans_override.inc) and tied to them by count and to the emulator's compiled copy of them;
  * the streams, index sequences, frame counts and bars those tests share (imported from here);
  * the weighted pool truth is helpers.truth_f64 of the gathered stream;
  * the index sequences notice a wrong frame: at a stand-in for the frames per iteration (STAND_IN_I: the real figure
    is the device's) every part holds every pool frame, and a stale prefetch (iteration 2 transforming iteration 1's
    frames) or an unmasked slot (the clamped last frame added once more) moves the truth by more than 1000 bars in its
    worst bin -- the GPU tests print the same two figures at the geometry they ran (I = 24 ... 65536 on the MI355X: a
    part of 24 frames cannot hold 64, and one frame among 163201 moves the truth by 49 bars, not 1000:
    profiles/mixed_loop.json);
  * the CPU float32 path on the same pool is within the case's bar of float64, so the bar judges the kernel and not
    float32; TWICE_CPU names the cases where it is not, which are judged at twice the CPU path's own error instead."""
import functools
import os
import re

import numpy as np
import pytest

from rtl_power_fftw_amd import synth
from helpers import ROOT, OracleWorker, emul_shipped_sizes, max_rel, oracle_accumulate, truth_f64
from parity_bars import TRUTH_BAR, VS_TRUTH, VS_TRUTH_DEEP

CSRC = os.path.join(ROOT, "rtl-power-fftw_amd", "csrc")
POOL = 64                       # distinct frames of a case's stream
POOL_SEED = 610000000           # + N: synth.uniform_iq bytes of the pool
INDEX_SEED = 620000000          # + N: the index sequence
STAND_IN_I = 1024               # frames per loop iteration assumed here (the GPU tests take grid x frames_per_wg / P)
NOTICED = 1000                  # bars a wrong frame moves the truth by
# run-time Stockham sizes (in neither table): 2, 3, 4, 6, 7 and 8 passes, both parities of mixed_kernel's one barrier
STOCKHAM = {6: 2, 30: 3, 108: 4, 486: 6, 1458: 7, 4374: 8}
# select_family (engine_family.h) gives a windowed run of 32768 bins to the four-step kernels: the split form's windowed
# twin is compiled and never launched by a shipped engine.  The case stays in the list and judges what such an engine runs.
NOT_MIXED = {(32768, True)}
# (N, windowed) -> the CPU float32 path's distance from float64 on the case's pool, where that is not within the case's
# bar: judged at twice this path's error on the pool as gathered (bar_against_truth).  test_the_cpu_float32_path_... keeps
# the list exact in both directions.
TWICE_CPU = {}


def table_text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read().split("#ifdef RPF_TUNING")[0]


def _plan_length(plan, macros):
    m = re.match(r"MixPlan<(\d+), (\d+), ", macros.get(plan, plan))
    assert m, plan
    return int(m.group(1)), int(m.group(2))


@functools.lru_cache(maxsize=None)
def planned_table():
    """{N: frame slots per workgroup} of mixed_plans.inc."""
    rows = re.findall(r"plan_entry<MixPlan<(\d+), (\d+), ", table_text("mixed_plans.inc"))
    return {int(n): int(fpw) for n, fpw in rows}


@functools.lru_cache(maxsize=None)
def split_table():
    """{N: P} of mixed_plans_split.inc, N = P x the length of the entry's plan."""
    text = table_text("mixed_plans_split.inc")
    macros = dict(re.findall(r"#define (RPF_M\w+) (MixPlan<.*>)", text))
    out = {}
    for p, plan in re.findall(r"^\s+split_entry<(\d+), (RPF_M\w+|MixPlan<[^()]*?>)(?:, \d, (?:true|false))?>\(0\)", text, flags=re.M):
        out[int(p) * _plan_length(plan, macros)[0]] = int(p)
    return out


@functools.lru_cache(maxsize=None)
def override_table():
    """{(N, windowed): P} of mixed_plans_override.inc (find_form looks here first)."""
    rows = re.findall(r"^\s+\{(\d+), (true|false), split_form<(\d+), MixPlan<(\d+), ", table_text("mixed_plans_override.inc"), flags=re.M)
    assert all(int(n) == int(p) * int(m) for n, _, p, m in rows)
    return {(int(n), w == "true"): int(p) for n, w, p, _ in rows}


def split_factor(N, windowed):
    """P of the form find_form gives the run: 1 for the planned and the Stockham kernel."""
    return override_table().get((N, windowed), split_table().get(N, 1))


def form_of(N, windowed):
    if (N, windowed) in NOT_MIXED:
        return "four-step"
    P = split_factor(N, windowed)
    if P > 1:
        return "split %d x %d%s" % (P, N // P, " (override)" if (N, windowed) in override_table() else "")
    return "planned" if N in planned_table() else "stockham %d passes" % STOCKHAM[N]


SIZES = sorted(set(planned_table()) | set(split_table()) | set(STOCKHAM))
CASES = [(N, windowed) for N in SIZES for windowed in (False, True)]


def case_id(case):
    return "%d-%s" % (case[0], "windowed" if case[1] else "plain")


def table_bar(N):
    """What tests/test_gpu_parity.py holds the size to against float64 at 53 to 64 frames: VS_TRUTH for the sizes of
    mixed_plans.inc and the Stockham kernel, VS_TRUTH_DEEP for the sizes of mixed_plans_split.inc, TRUTH_BAR where it
    names the size."""
    if N in TRUTH_BAR:
        return TRUTH_BAR[N]
    return VS_TRUTH_DEEP if N in split_table() else VS_TRUTH


def loop_window(N, windowed):
    return synth.hann_window(N) + np.float32(0.25) if windowed else None


def pool_frames(N):
    """POOL x 2 N bytes: the distinct frames of the size's stream."""
    return synth.uniform_iq(POOL_SEED + N, POOL * N).reshape(POOL, 2 * N)


def index_sequence(N, frames):
    """idx[f], uniform over the pool: the top six bits of splitmix64's words (a prefix of every longer sequence)."""
    return (synth.splitmix64(INDEX_SEED + N, frames) >> np.uint64(58)).astype(np.int64)


def frames_of(I, fpw):
    """Two full iterations and a third in which about half the workgroups run, the last of them with idle slots."""
    F = 2 * I + I // 2 + 1
    return F + 1 if fpw > 1 and F % fpw == 0 else F


def parts_of(F, I):
    return [(a, min(a + I, F)) for a in range(0, F, I)]


def counts_of(idx):
    return np.bincount(idx, minlength=POOL).astype(np.float64)


def pool_powers(N, windowed, pool=None):
    """p[d, k] = |FFT64(prepared pool frame d)[k]|^2."""
    pool = pool_frames(N) if pool is None else pool
    w = loop_window(N, windowed)
    return np.stack([truth_f64(N, frame, 1, w) for frame in pool])


def cpu_pool_powers(N, windowed, pool=None):
    """The CPU float32 path on every pool frame: oracle_accumulate(N, frame, 1, w, 32), from one plan."""
    pool = pool_frames(N) if pool is None else pool
    worker, rows = OracleWorker(N, loop_window(N, windowed), 32), []
    try:
        for frame in pool:
            worker.begin(1)
            worker.consume(frame)
            assert worker.repeats_done == 1
            rows.append(worker.pwr)
    finally:
        worker.close()
    return np.stack(rows)


def wrong_frame_shifts(idx, I, p):
    """The relative shift of the truth's worst bin under the two loop-edge mistakes a sum can hide: (every frame of the
    second iteration replaced by the one I frames before it, the last frame added once more)."""
    truth = counts_of(idx) @ p
    stale = idx.copy()
    stale[I:2 * I] = idx[:I]
    extra = counts_of(idx)
    extra[idx[-1]] += 1
    return max_rel(counts_of(stale) @ p, truth), max_rel(extra @ p, truth)


def bar_against_truth(case, counts, p, pool=None):
    """(bar, which): the case's table bar, or twice the CPU float32 path's error under the same counts (TWICE_CPU)."""
    N, windowed = case
    if case not in TWICE_CPU:
        return table_bar(N), "table"
    return 2 * max_rel(counts @ cpu_pool_powers(N, windowed, pool), counts @ p), "twice the CPU float32 path"


# ---- the case list -----------------------------------------------------------------------------------------------------

def test_case_list_is_the_tables():
    planned, split = planned_table(), split_table()
    assert len(planned) == len(re.findall(r"^\s+plan_entry<", table_text("mixed_plans.inc"), flags=re.M))
    assert len(split) == len(re.findall(r"^\s+split_entry<", table_text("mixed_plans_split.inc"), flags=re.M))
    assert not set(planned) & set(split)
    assert sorted(emul_shipped_sizes()) == sorted(list(planned) + list(split)), "the compiled tables"
    assert len(CASES) == len(set(CASES)) == 2 * (len(planned) + len(split) + len(STOCKHAM))
    assert all(N in planned or N in split for N, _ in override_table())


def test_stockham_sizes_and_their_pass_counts():
    """factorise (rpf_mixed.hip): radices 5, 4, 3, 2 in that order."""
    for N, passes in STOCKHAM.items():
        assert N not in planned_table() and N not in split_table() and N % 2 == 0 and N <= 5120 and N & (N - 1)
        rest, n = N, 0
        for r in (5, 4, 3, 2):
            while rest % r == 0 and rest > 1:
                rest, n = rest // r, n + 1
        assert rest == 1 and n == passes
    assert {p % 2 for p in STOCKHAM.values()} == {0, 1}


def test_the_one_run_another_family_takes():
    with open(os.path.join(CSRC, "engine_family.h")) as f:
        text = f.read()
    assert "windowed_32768 = q.N == 32768 && q.windowed && shipped" in text and "q.mixed && !windowed_32768" in text
    assert NOT_MIXED == {(32768, True)} and 32768 in split_table()


def test_seeds_are_new():
    from test_gpu_heldout import held_out_seed
    for N in SIZES:
        held = {held_out_seed(name, N) for name in ("held_out_a", "held_out_b", "held_out_c", "held_out_d", "held_out_e")}
        used = {400 + N, 77 + N % 101, 900 + N, 300 + N % 89, 1300 + N % 97}       # tests/test_gpu_parity.py
        assert not {POOL_SEED + N, INDEX_SEED + N} & (held | used)


def test_frame_counts():
    for I, fpw in ((1024, 1), (1020, 51), (1024, 3), (6, 3), (32, 1), (10, 2), (100 * 51, 51)):
        F = frames_of(I, fpw)
        assert F == 2 * I + I // 2 + 1 + (fpw > 1 and (2 * I + I // 2 + 1) % fpw == 0) and (fpw == 1 or F % fpw)
        cuts = parts_of(F, I)
        assert len(cuts) == 3 and cuts[0] == (0, I) and cuts[-1][1] == F and all(0 < b - a <= I for a, b in cuts)


def test_the_worker_is_oracle_accumulate():
    N = 500
    pool = pool_frames(N)[:3]
    for windowed in (False, True):
        rows = cpu_pool_powers(N, windowed, pool)
        for frame, row in zip(pool, rows):
            assert np.array_equal(row, oracle_accumulate(N, frame, 1, loop_window(N, windowed), 32)[0])


# ---- the reference -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("windowed", [False, True], ids=["plain", "windowed"])
@pytest.mark.parametrize("N", [50, 500, 3750])
def test_pool_truth_is_the_truth_of_the_gathered_stream(N, windowed):
    F = frames_of(STAND_IN_I, planned_table()[N])
    idx = index_sequence(N, F)
    stream = pool_frames(N)[idx].reshape(-1)
    assert stream.size == 2 * N * F
    whole = truth_f64(N, stream, F, loop_window(N, windowed))
    err = max_rel(counts_of(idx) @ pool_powers(N, windowed), whole)
    print("N=%d %s, %d frames: weighted pool truth against the stream's %.3g" % (N, "windowed" if windowed else "plain", F, err))
    assert err < 1e-12


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_index_sequence_notices_and_the_cpu_float32_path_holds_the_bar(case):
    N, windowed = case
    I, bar = STAND_IN_I, table_bar(N)
    F = frames_of(I, planned_table().get(N, 1))
    idx = index_sequence(N, F)
    assert np.array_equal(idx[:I], index_sequence(N, I)) and idx.min() >= 0 and idx.max() < POOL
    for a, b in parts_of(F, I)[:2]:
        assert np.unique(idx[a:b]).size == POOL, "every full part holds every pool frame"
    assert not np.array_equal(idx[:I], idx[I:2 * I])
    pool = pool_frames(N)
    assert len({frame.tobytes() for frame in pool}) == POOL
    p = pool_powers(N, windowed, pool)
    stale, extra = wrong_frame_shifts(idx, I, p)
    counts = counts_of(idx)
    cpu = max_rel(counts @ cpu_pool_powers(N, windowed, pool), counts @ p)
    print("N=%d %s (%s), I=%d F=%d: stale prefetch moves the truth by %.3g, an unmasked slot by %.3g (%d x bar %.3g); "
          "CPU float32 path %.3g of float64 (bar %.3g)"
          % (N, "windowed" if windowed else "plain", form_of(N, windowed), I, F, stale, extra, NOTICED, NOTICED * bar, cpu, bar))
    assert stale > NOTICED * bar and extra > NOTICED * bar
    if case in TWICE_CPU:
        assert cpu >= bar and abs(cpu / TWICE_CPU[case] - 1) < 0.01, "a stale entry of TWICE_CPU"
    else:
        assert cpu < bar, "the CPU float32 path misses the bar: the case belongs in TWICE_CPU with this figure"
