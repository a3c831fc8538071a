"""Overlapped FFT frames on the MI355X.  The central check: an engine at frame step S on stream X gives what an engine
at step N gives on the materialised stream X' = concat_f X[2fS : 2fS + 2N] -- bit for bit where the same kernels run
over the same frames -- and X' goes through today's parity-tested path and the unchanged oracle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, synth
from rtl_power_fftw_amd.datastore import frame_span, frames_in
from helpers import ROOT, dp, oracle_accumulate, oracle_lib
from parity_bars import ADDITIVITY, PARITY, SAME_KERNELS
from test_frame_overlap import materialise, spread

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")
NO_FUSED = _lib.FLAG_NO_FOURSTEP_FUSED          # the reference engine on X': four-step sizes on the two-kernel path too
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")


def to_device(stream, misalign=0):
    """A device copy of `stream` starting `misalign` bytes past a 256-byte boundary; returns (keep-alive, pointer)."""
    t = torch.empty(stream.size + 64, dtype=torch.uint8, device=DEV)
    t[misalign:misalign + stream.size].copy_(torch.from_numpy(np.ascontiguousarray(stream)))
    return t, t.data_ptr() + misalign


def device_run(ds, stream, repeats=1 << 40, misalign=0):
    keep, ptr = to_device(stream, misalign)
    out = torch.empty(ds.params.N, dtype=torch.float64, device=DEV)
    n = ds.accumulate_device(ptr, stream.size, repeats, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del keep
    return out.cpu().numpy(), n


def engine(N, step=None, window=False, flags=0, **kw):
    w = synth.hann_window(N) if window else None
    return rpf.Datastore(rpf.Params(N=N, window=window, frame_step=step, **kw), w, flags=flags)


def per_bin_rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


# ---- K1 (native stride) -------------------------------------------------------------------------------------------

K1_CASES = [(64, False), (512, False), (4096, False), (4096, True), (8192, False)]


@pytest.mark.parametrize("N,window", K1_CASES)
def test_k1_strided_equals_materialised(N, window):
    X = synth.noise_tones_iq(21, 300 * N)
    w = synth.hann_window(N) if window else None
    with engine(N, window=window) as ref:
        for step in (N // 2, N // 4, 3 * N // 4, N - 8, N // 2 + 1):
            Xp = materialise(X, N, step)
            R = frames_in(X.size, N, step)
            want, n0 = device_run(ref, Xp)
            assert n0 == R
            for flags, misalign in ((0, 0), (0, 2), (_lib.FLAG_NO_LDS_DMA, 0)):
                with engine(N, step, window, flags) as ds:
                    assert ds.frames_in(X.size) == R and ds.frame_span(R) == frame_span(R, N, step)
                    got, n = device_run(ds, X, misalign=misalign)
                assert n == R
                assert np.array_equal(got, want), (N, step, flags, misalign)
            orc, _ = oracle_accumulate(N, Xp, R, w)
            assert per_bin_rel(want, orc) < PARITY


# ---- the gather path (every other family) ---------------------------------------------------------------------------

GATHER_CASES = [(500, False, 40), (5000, False, 40), (16384, False, 12), (20000, False, 12), (32768, True, 12),
                (65536, False, 10), (262144, False, 8), (2046, False, 40), (131070, False, 8), (524288, False, 4)]


@pytest.mark.parametrize("N,window,R", GATHER_CASES)
def test_gather_path_equals_materialised(N, window, R):
    step = N // 2 + (2 if N % 4 == 0 else 1)        # an odd pitch / 4-byte misalignment where N allows
    X = synth.noise_tones_iq(5, N + step * (R - 1))
    Xp = materialise(X, N, step)
    assert Xp.size == 2 * N * R
    with engine(N, window=window, flags=NO_FUSED) as ref:
        want, _ = device_run(ref, Xp)
    with engine(N, step, window) as ds:
        got, n = device_run(ds, X)
        got2, _ = device_run(ds, X, misalign=2)
    assert n == R
    assert np.array_equal(got, want) and np.array_equal(got2, want), N
    if N <= 20000:
        orc, _ = oracle_accumulate(N, Xp, R, synth.hann_window(N) if window else None)
        assert per_bin_rel(want, orc) < PARITY


def test_gather_path_in_several_chunks():
    N, step = 65536, 32768
    R = (64 << 20) // (2 * N) + 263                 # 775 frames: two chunks of at most 64 MB of gathered frames
    X = synth.noise_tones_iq(6, N + step * (R - 1))
    Xp = materialise(X, N, step)
    with engine(N, flags=NO_FUSED) as ref:
        want, _ = device_run(ref, Xp)
    with engine(N, step) as ds:
        got, n = device_run(ds, X)
    assert n == R
    assert per_bin_rel(got, want) < ADDITIVITY          # the chunks' sums added: double addition regrouped


def test_device_fused_refuses_overlap_off_k1():
    with engine(5000, 2500) as ds:
        keep, ptr = to_device(synth.uniform_iq(1, 5000 * 4))
        with pytest.raises(rpf.RPFError) as e:
            ds.device_fused(ptr, 5000 * 8, 10, torch.cuda.current_stream().cuda_stream)
        assert e.value.retval == rpf.ReturnValue.InvalidArgument
        torch.cuda.synchronize()


# ---- the buffer-queue path ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,buf", [(4096, 2730), (4096, 16384 + 6), (262144, 1 << 20), (262144, 174762)])
def test_queue_path_equals_device_path(N, buf):
    step = N // 2
    X = synth.noise_tones_iq(8, 40 * N + 1234)
    R = frames_in(X.size, N, step)
    with engine(N, step, buf_length=buf) as ds:
        want, _ = device_run(ds, X)
        got, done = ds.accumulate(X, 1 << 40)
        assert done == R == ds.frames_in(X.size)
        assert per_bin_rel(got, want) < SAME_KERNELS
        # the quota reached in the middle of a buffer
        quota = R - 5
        want_q, _ = device_run(ds, X, repeats=quota)
        got_q, done_q = ds.accumulate(X, quota)
        assert done_q == min(quota, R)
        assert per_bin_rel(got_q, want_q) < SAME_KERNELS


# ---- hops ---------------------------------------------------------------------------------------------------------

def test_hops_with_overlap_run_hop_by_hop():
    N, step = 4096, 2048
    streams = [synth.noise_tones_iq(30 + h, (20 + 3 * h) * N) for h in range(3)]
    with engine(N, step) as ds:
        singles = [device_run(ds, s)[0] for s in streams]
        keep = [to_device(s) for s in streams]
        out = torch.empty(3 * N, dtype=torch.float64, device=DEV)
        done = ds.accumulate_device_hops([p for _, p in keep], [s.size for s in streams], [1 << 40] * 3,
                                         out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert done == [frames_in(s.size, N, step) for s in streams]
        got = out.cpu().numpy().reshape(3, N)
        for h in range(3):
            assert np.array_equal(got[h], singles[h])
        with pytest.raises(rpf.RPFError) as e:
            ds.device_fused_hops([p for _, p in keep], [s.size for s in streams], [1 << 40] * 3,
                                 torch.cuda.current_stream().cuda_stream)
        assert e.value.retval == rpf.ReturnValue.InvalidArgument


# ---- the default is unchanged -------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [4096, 5000, 65536])
def test_default_frame_step_is_todays_engine(N):
    X = synth.noise_tones_iq(9, 30 * N + 100)
    with rpf.Datastore(rpf.Params(N=N), struct_size=_lib.CONFIG_SIZE_V2_0) as old:
        want, n0 = device_run(old, X)
        assert old.frames_in(X.size) == 30
    for step in (N, 0):
        with engine(N, step) as ds:
            got, n = device_run(ds, X)
        assert n == n0 == 30 and np.array_equal(got, want)


# ---- the point of the feature -------------------------------------------------------------------------------------

def test_engine_variance_ratio_hann_half_overlap():
    N = 4096
    X = synth.uniform_iq(11, 2000 * N)
    with engine(N, window=True) as plain, engine(N, N // 2, window=True) as over:
        p0, f0 = device_run(plain, X)
        p1, f1 = device_run(over, X)
    assert f0 == 2000 and f1 == 3999
    r = spread(p1 / f1) / spread(p0 / f0)
    assert 0.45 <= r <= 0.62, r


# ---- the CLI ------------------------------------------------------------------------------------------------------

def _data_lines(text):
    return [l for l in text.split("\n") if not l.startswith("#")]


def test_cli_frame_overlap_matches_python_path(tmp_path):
    N, R, cfreq = 4096, 200, 1420405752
    step = N // 2
    r = subprocess.run([CLI, "--frame-overlap", "50", "-b", str(N), "-n", str(R), "--synthetic", "2"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "Total number of (complex) samples to collect: %d" % (N + step * (R - 1)) in r.stderr
    X = synth.noise_tones_iq(2 + cfreq % 9973, N + step * (R - 1))      # SyntheticSource::seed_for
    with engine(N) as ds:
        pwr, done = ds.accumulate(materialise(X, N, step), R)
    assert done == R
    buf = ctypes.create_string_buffer(64 * N)
    oracle_lib().rpf_oracle_format_text(pwr.ctypes.data_as(dp), N, R, cfreq, 2000000, 0, None, buf, len(buf))
    want = buf.value.decode().split("\n")[:-1]
    assert _data_lines(r.stdout)[:len(want)] == want
    # two engines on one device, host reduce: each reads its frame range (bytes from 2 S first_frame)
    r2 = subprocess.run([CLI, "--frame-overlap", "50", "-b", str(N), "-n", str(R), "--synthetic", "2",
                         "--gpus", "0,0", "--reduce", "host"], capture_output=True, text=True)
    assert r2.returncode == 0, r2.stderr
    a = [l for l in _data_lines(r.stdout) if l.strip()]
    b = [l for l in _data_lines(r2.stdout) if l.strip()]
    assert len(a) == len(b) == N
    va = np.array([float(l.split()[1]) for l in a])
    vb = np.array([float(l.split()[1]) for l in b])
    # (the text carries six significant digits: the sums, equal within ADDITIVITY, print alike up to the last digit)
    assert np.max(np.abs(va - vb) / np.abs(va)) <= 1e-5
