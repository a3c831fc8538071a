"""BASELINE.json's full-size configurations on the GPU, on the streams SURVEY.md 8d
specifies for them: against the committed float64 fixtures (tests/golden/), against
the float32 CPU oracle run over the WHOLE stream (all host cores: C2 0.2 s, C4 a few
seconds), and through size-independent properties.  Run with  pytest -m gpu."""
import ctypes
import json
import os

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from helpers import (C4_CASE, C5_CASES, ROOT, dp, golden_stream_device, harmonic_bins, load_golden, max_rel,
                     oracle_lib, u8p)
from parity_bars import ADDITIVITY, C4_LINE_BINS_VS_TRUTH, PARITY, PARSEVAL, TOTAL_POWER

pytestmark = pytest.mark.gpu

N, R = 4096, 10000            # config C2 (and C3 with the Hann window)


def oracle_all_cores(n, stream, repeats, window=None):
    """The float32 oracle over a whole full-size stream, frames dealt to every host core."""
    pwr = np.zeros(n)
    done = ctypes.c_int64()
    w = None if window is None else np.ascontiguousarray(window, dtype=np.float32).ctypes.data_as(
        ctypes.POINTER(ctypes.c_float))
    rc = oracle_lib().rpf_oracle_accumulate_mt(n, w, stream.ctypes.data_as(u8p), stream.size, repeats,
                                               os.cpu_count() or 1, pwr.ctypes.data_as(dp), ctypes.byref(done))
    assert rc == 0 and done.value == repeats
    return pwr


def record(name, **values):
    """Measured errors of the full-size runs, kept for DESIGN.md: into the file $RPF_PARITY_RECORD names
    (tools/gpu_r06.sh sets it); without it nothing is written -- running the tests leaves the tree alone."""
    path = os.environ.get("RPF_PARITY_RECORD")
    if not path:
        return
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[name] = values
    json.dump(data, open(path, "w"), indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def c2():
    import torch
    dev = torch.device("cuda:0")
    d_in = rpf.synth.noise_tones_iq_torch(2, N * R, dev)       # bit-identical to synth.noise_tones_iq (test_synth.py)
    stream = d_in.cpu().numpy()
    assert np.array_equal(stream[: 2 * N * 16], rpf.synth.noise_tones_iq(2, N * 16))
    return stream, d_in, dev


def device_run(ds, d_in, first_frame, frames, dev, n=N):
    import torch
    out = torch.empty(n, dtype=torch.float64, device=dev)
    got = ds.accumulate_device(d_in.data_ptr() + 2 * n * first_frame, 2 * n * frames, frames,
                               out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert got == frames
    return out.cpu().numpy()


@pytest.mark.parametrize("windowed", [False, True])
def test_c2_c3_full_size(c2, windowed):
    stream, d_in, dev = c2
    w = rpf.synth.hann_window(N) if windowed else None
    with rpf.Datastore(rpf.Params(N=N, window=windowed, repeats=R), w) as ds:
        full = device_run(ds, d_in, 0, R, dev)
        # (1) additivity over frames: pwr(A ++ B) = pwr(A) + pwr(B), any cut point
        a = device_run(ds, d_in, 0, 3333, dev)
        b = device_run(ds, d_in, 3333, R - 3333, dev)
        assert max_rel(a + b, full) < ADDITIVITY
        # (2) run-to-run reproducibility (deterministic two-stage reduce)
        assert np.array_equal(full, device_run(ds, d_in, 0, R, dev))
        # (3) Parseval: sum_k pwr[k] = N * sum |x[n]|^2, the right side exact in integers
        x = stream.astype(np.int64).reshape(R, N, 2) - 127
        if not windowed:
            energy = float(N * np.sum(x * x))
        else:
            e_n = np.sum(x * x, axis=(0, 2)).astype(np.float64)          # per sample position
            energy = float(N * np.sum(e_n * w.astype(np.float64) ** 2))
        assert abs(full.sum() / energy - 1.0) < PARSEVAL
        # (4) the float32 oracle over ALL 10000 frames, plain per-bin relative error
        want = oracle_all_cores(N, stream, R, w)
        err = max_rel(full, want)
        record("c3" if windowed else "c2", gpu_vs_oracle=err)
        assert err < PARITY
        # (5) the queue path over the whole stream (50 reference-sized buffers)
        host, done = ds.accumulate(stream, R)
        assert done == R and max_rel(host, full) < ADDITIVITY


def test_c5_eight_hops_match_golden_and_shard_like_multi_gpu():
    """Config C5 as specified: 8 hops x 5000 frames of N = 4096, hop h = seed 50 + h,
    every hop with its own accumulator (acquisition.cxx:252-254).  Each hop against its
    float64 fixture and the float32 oracle; then cut into the frame ranges 2 and 3 ranks
    would own (sharding.shard_hops): the shard sums are the whole hop."""
    import torch
    dev = torch.device("cuda:0")
    hops, per_hop = 8, 5000
    worst_truth = worst_oracle = 0.0
    with rpf.Datastore(rpf.Params(N=N, repeats=per_hop)) as ds:
        whole = []
        d_hops = []
        for hop in range(hops):
            g = load_golden(C5_CASES[hop])
            assert int(g["N"]) == N and int(g["repeats"]) == per_hop and int(g["seed"]) == 50 + hop
            stream, d_in = golden_stream_device(g, dev)
            d_hops.append(d_in)
            got = device_run(ds, d_in, 0, per_hop, dev)
            whole.append(got)
            worst_truth = max(worst_truth, max_rel(got, g["pwr"]))
            worst_oracle = max(worst_oracle, max_rel(got, oracle_all_cores(N, stream, per_hop)))
        record("c5", gpu_vs_truth=worst_truth, gpu_vs_oracle=worst_oracle)
        assert worst_truth < PARITY and worst_oracle < PARITY
        for world in (2, 3):
            acc = np.zeros((hops, N))
            for rank in range(world):
                for hop, first, count in rpf.sharding.shard_hops(hops, per_hop, world, rank):
                    acc[hop] += device_run(ds, d_hops[hop], first, count, dev)
            for hop in range(hops):
                assert max_rel(acc[hop], whole[hop]) < ADDITIVITY


@pytest.fixture(scope="module")
def c4():
    import torch
    g = load_golden(C4_CASE)
    dev = torch.device("cuda:0")
    stream, d_in = golden_stream_device(g, dev)        # noise_tones_iq(4, 262144 * 1000): C4's own stream
    return g, stream, d_in, dev


def rocfft_power(d_in, n, frames, dev, chunk=40):
    """Independent float32 FFT (torch.fft = rocFFT) of the same frames, |X|^2 summed in double."""
    import torch
    sign = (1 - 2 * (torch.arange(n, device=dev) % 2)).to(torch.float32)
    acc = torch.zeros(n, dtype=torch.float64, device=dev)
    for f0 in range(0, frames, chunk):
        f1 = min(frames, f0 + chunk)
        x = d_in[2 * n * f0: 2 * n * f1].to(torch.float32).reshape(f1 - f0, n, 2) - 127.0
        spec = torch.fft.fft(torch.complex(x[..., 0] * sign, x[..., 1] * sign), dim=1)
        acc += (spec.real.double() ** 2 + spec.imag.double() ** 2).sum(0)
    return acc.cpu().numpy()


def test_c4_full_size_on_its_own_stream(c4):
    """Config C4: N = 262144 x 1000 repeats on the stream SURVEY.md 8d specifies (seed 4,
    tones included), all 1000 frames, against the float64 fixture (every 64th bin, +-512
    bins around the two lines, the total), the float32 oracle over the whole stream, and
    rocFFT on the same frames.  Plain per-bin relative error, no median floor.

    The 16 bins at multiples of N/16 carry the tones and the harmonics of their integer
    rounding -- deterministic lines, identical in every frame, so a float32 FFT's rounding
    error there is coherent and does not average down with R; the weakest of them sit 2e4
    below the strongest line.  They are held to the bar too and, should any float32 FFT
    below the strongest line.  Round 6: the row transform's last pass runs in double at this size, which holds them to the
    bar against the TRUTH (0.6e-6; the float32 pass had 1.5e-6, like the oracle and rocFFT)."""
    g, stream, d_in, dev = c4
    n4, r4 = int(g["N"]), int(g["repeats"])
    st = int(g["stride"])
    with rpf.Datastore(rpf.Params(N=n4, repeats=r4, buf_length=1638400)) as ds:
        full = device_run(ds, d_in, 0, r4, dev, n4)
        a, b = device_run(ds, d_in, 0, 337, dev, n4), device_run(ds, d_in, 337, r4 - 337, dev, n4)
        assert max_rel(a + b, full) < ADDITIVITY                       # additivity over frames
        assert np.array_equal(full, device_run(ds, d_in, 0, r4, dev, n4))   # reproducible
        x = stream.astype(np.int64).reshape(-1, 2) - 127
        energy = float(n4) * float(np.sum(x * x))
        assert abs(full.sum() / energy - 1.0) < PARSEVAL              # Parseval, right side exact
        host, done = ds.accumulate(stream, r4)                    # 320 buffers of 3.125 frames
        assert done == r4 and max_rel(host, full) < ADDITIVITY

    oracle = oracle_all_cores(n4, stream, r4)
    rocfft = rocfft_power(d_in, n4, r4, dev)
    lines = harmonic_bins(n4)
    sampled = np.arange(0, n4, st)
    is_line = np.isin(sampled, lines)
    near = g["near_bins"]
    near_is_line = np.isin(near, lines)

    def errors(p):
        rel_s = np.abs(p[sampled] - g["pwr"]) / g["pwr"]
        rel_n = np.abs(p[near] - g["near_pwr"]) / g["near_pwr"]
        return {"floor": float(max(rel_s[~is_line].max(), rel_n[~near_is_line].max())),
                "near_tone": float(rel_n[~near_is_line].max()),
                "lines": float(rel_s[is_line].max()),
                "total": float(abs(p.sum() / float(g["total"]) - 1))}

    e_gpu, e_orc, e_roc = errors(full), errors(oracle), errors(rocfft)
    floor_bins = np.ones(n4, dtype=bool)
    floor_bins[lines] = False
    vs_oracle_floor = max_rel(full[floor_bins], oracle[floor_bins])
    vs_oracle_lines = max_rel(full[lines], oracle[lines])
    record("c4", gpu_vs_truth=e_gpu, oracle_vs_truth=e_orc, rocfft_vs_truth=e_roc,
           gpu_vs_oracle_floor=vs_oracle_floor, gpu_vs_oracle_lines=vs_oracle_lines)
    print("C4 vs float64 truth  gpu %s  oracle %s  rocfft %s  gpu-vs-oracle floor %.2e lines %.2e"
          % (e_gpu, e_orc, e_roc, vs_oracle_floor, vs_oracle_lines))
    # every bin that is not one of the 16 deterministic lines: the plain bar, vs truth and vs the CPU path
    assert e_gpu["floor"] < PARITY and vs_oracle_floor < PARITY
    assert e_gpu["total"] < TOTAL_POWER
    # the 16 line bins against float64 TRUTH (parity_bars.py section 4).  Their distance from the CPU path is in the
    # record, not asserted: the CPU path is itself ~1.6e-6 from the truth there (e_orc["lines"]), and the 4.8e-7 that the
    # float32 last pass of rounds 1 - 5 showed against it was two transforms making the same roundings beside a line
    # (profiles/r05_fourstep_wide.txt), not closeness to what FFTW would print.
    assert e_gpu["lines"] < C4_LINE_BINS_VS_TRUTH


def _bench_line(args, env_extra=None, nproc=0):
    import subprocess
    import sys
    env = dict(os.environ, **(env_extra or {}))
    if nproc:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
               "--master-addr", "127.0.0.1", "--master-port", "29577", os.path.join(ROOT, "bench.py")] + args
    else:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + args
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.split("\n") if l.strip()]
    assert len(lines) == 1, "bench.py must print exactly one line on stdout: %r" % lines[:3]
    return json.loads(lines[0])


def test_bench_c5_line_through_rccl_is_checked_against_the_fixtures():
    """bench.py --workload C5 --full with torch.distributed initialised (RCCL, world size 1 on this box):
    the strong-scaling line carries the check of the REDUCED spectra against the committed C5
    fixtures, the same-workload one-GPU figure and what RCCL saw, and stdout is the one JSON line (RCCL's banner goes
    to stderr).  Two consecutive scans share a launch at one rank (8 hops x 2 = the kernel's 16-entry hop table); an odd
    step count leaves a ragged tail that goes hop by hop."""
    d = _bench_line(["--workload", "C5", "--force-dist", "--steps", "9", "--warmup", "2", "--full", "--no-cpu-baseline"])
    assert d["scaling"] == "strong" and d["n_gpus"] == 1 and d["config"]["reduce"].startswith("one async RCCL reduce")
    assert d["check"]["hops"] == 8 and d["check"]["reduced_spectra_vs_float64_fixtures_max_rel"] < PARITY
    assert d["value"] > 5e10 and d["roofline"]["frac"] > 0.05
    assert d["config"]["scans_per_launch"] == 2 and d["roofline"]["hops_per_launch"] == 16
    assert d["rccl"]["world_size"] == 1 and d["rccl"]["version"] and d["rccl"]["backend"] == "nccl"
    assert d["one_gpu_same_workload"]["value"] > 5e10
    # a launch per scan (round 5's form) gives the same spectra
    d1 = _bench_line(["--workload", "C5", "--steps", "8", "--warmup", "2", "--full", "--no-cpu-baseline",
                      "--scans-per-launch", "1"])
    assert d1["config"]["scans_per_launch"] == 1 and d1["check"]["reduced_spectra_vs_float64_fixtures_max_rel"] < PARITY


def test_bench_default_line_carries_the_multi_gpu_reference():
    """`python bench.py --full` (one rank: config C2, the metric): the line also carries config C5's one-GPU rate, the
    denominator of the C5 lines a `--gpus N > 1` run of the same script prints."""
    d = _bench_line(["--steps", "20", "--warmup", "5", "--full", "--no-cpu-baseline", "--no-end-to-end"])
    assert d["config"]["workload_name"] == "C2" and d["scaling"] == "weak" and d["n_gpus"] == 1
    assert d["multi_gpu_reference"]["workload_name"] == "C5" and d["multi_gpu_reference"]["value"] > 5e10


def test_bench_plain_line_is_lean_and_dumps_the_last_step(c2, tmp_path):
    """A plain run (no --full) times exactly --steps steps in one region and carries nothing --full owns;
    --dump-outputs writes the last timed step's spectrum.  With 3 replay buffers, step 7 reads buffer 0: the
    unrotated C2 stream, whose spectrum the C-ABI gives directly."""
    stream, d_in, dev = c2
    d = _bench_line(["--steps", "7", "--warmup", "2", "--replay-buffers", "3", "--dump-outputs", str(tmp_path)])
    assert d["config"]["workload_name"] == "C2" and d["steps"] == 7 and d["warmup"] == 2
    assert d["unit"] == "samples/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] == pytest.approx(d["timing"]["region_s"] * 1e3 / 7)
    assert d["value"] == pytest.approx(N * R * 7 / d["timing"]["region_s"])
    assert d["roofline"] is None and not {"cpu_baseline", "end_to_end", "multi_gpu_reference"} & set(d)
    got = np.load(tmp_path / "power.npy")
    assert got.dtype == np.float64 and got.shape == (N,)
    with rpf.Datastore(rpf.Params(N=N, repeats=R)) as ds:
        want = device_run(ds, d_in, 0, R, dev)
    assert max_rel(got, want) < ADDITIVITY


def test_bench_c5_dump_is_the_last_scan(tmp_path):
    """--workload C5 --dump-outputs: the last timed scan's 8 spectra (3 steps: one launch of two scans, then a ragged
    tail hop by hop), each against its float64 fixture; without --full the line carries no check of its own."""
    d = _bench_line(["--workload", "C5", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert d["steps"] == 3 and "check" not in d and "one_gpu_same_workload" not in d
    got = np.load(tmp_path / "power.npy")
    assert got.dtype == np.float64 and got.shape == (8, N)
    for hop in range(8):
        assert max_rel(got[hop], load_golden(C5_CASES[hop])["pwr"]) < PARITY


def test_bench_c5_two_ranks():
    """`python bench.py --gpus 2`, no wrapper: bench.py starts the two ranks itself (two GPUs): hop-major
    shards, one RCCL reduce per block of scans, reduced spectra checked."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU on this box: the 2-rank RCCL run needs two")
    d = _bench_line(["--gpus", "2", "--steps", "8", "--warmup", "2", "--full"])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["workload_name"] == "C5"
    assert len(d["per_rank"]) == 2 and {p["rank"] for p in d["per_rank"]} == {0, 1}
    assert d["check"]["reduced_spectra_vs_float64_fixtures_max_rel"] < PARITY
    assert d["one_gpu_same_workload"]["value"] > 0
    assert d["rccl"]["world_size"] == 2 and d["rccl"]["devices"] == [0, 1]


def test_bench_refuses_more_ranks_than_gpus():
    """The shape of the driver's command with more GPUs than the box has: exit code 2 and NO line --
    never a one-GPU measurement reported under a larger --gpus."""
    import subprocess
    import sys
    import torch
    n = torch.cuda.device_count() + 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "4"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and r.stdout.strip() == ""
    assert "%d ranks asked for" % n in r.stderr


@pytest.mark.parametrize("ranks,form", [(2, "self"), (8, "self"), (8, "driver")])
def test_bench_c5_rehearsal_ranks_share_one_gpu(ranks, form):
    """The multi-rank run rehearsed on ONE GPU (`--dist-backend gloo --share-device`): shard_hops, the scans-per-launch
    batching and the block layout every rank must agree on, the ScanRing's reuse, per-rank reports and the fixture
    check of the REDUCED spectra, all on the real kernels; only the exchange differs from the RCCL run (gloo, staged
    through the host).  form "self": `python bench.py --gpus N` starts the ranks itself; form "driver": the driver's
    exact command -- `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py --gpus N ...`, ranks from the environment.  10 steps: two whole
    blocks of four scans and a ragged one."""
    args = ["--gpus", str(ranks), "--dist-backend", "gloo", "--share-device", "--steps", "10", "--warmup", "2", "--full"]
    d = _bench_line(args, nproc=ranks if form == "driver" else 0)
    assert d["n_gpus"] == ranks and d["scaling"] == "strong" and d["config"]["workload_name"] == "C5"
    assert "rehearsal" in d and "gloo" in d["config"]["reduce"]
    assert d["config"]["scans_per_launch"] == 4
    assert d["rccl"]["world_size"] == 0 and "gloo" in d["rccl"]["backend"]
    assert len(d["per_rank"]) == ranks and sorted(p["rank"] for p in d["per_rank"]) == list(range(ranks))
    assert sum(p["frames_per_step"] for p in d["per_rank"]) == 8 * 5000
    assert d["check"]["hops"] == 8 and d["check"]["reduced_spectra_vs_float64_fixtures_max_rel"] < PARITY
    assert d["one_gpu_same_workload"]["value"] > 0
