"""float32 I/Q (cf32) on the MI355X.  The format is tied to the tested cs16 path by identities that hold exactly:

  1. a cf32 stream of int16 values == the cs16 stream of those values (the same floats leave the unpack);
  2. the stream x 2^-9 gives the spectrum x 2^-18, exactly (powers of two scale every float32 and double operation
     exactly; nothing overflows or goes subnormal);
  3. Gaussian float32 input with full mantissas against numpy complex128, at the bar of cf32_bars.

"Equal" is np.array_equal where the two runs report the same launch geometry, ADDITIVITY otherwise (same() of
test_gpu_sample_formats).  Each test prints the figures it judged."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, synth
from rtl_power_fftw_amd.datastore import frames_in
from helpers import ROOT, dp, max_err_over_mean, max_rel, oracle_lib
from parity_bars import ADDITIVITY, PARITY, SAME_KERNELS
from cf32_bars import CF32_VS_TRUTH
from test_gpu_sample_formats import device_run, engine, same, to_device

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
NO_DMA = _lib.FLAG_NO_LDS_DMA
CATCH_ALL = _lib.FLAG_CATCH_ALL

# every structural case of K1 for cf32: the tiny sizes' ring (64), P = 16 with one exchange (256), four slots (512), a
# two-deep ring with LDS twiddles (1024), the first size with the ring of depth 1 (2048), the 512-thread workgroup with
# two slots (4096), one slot (8192)
K1_SIZES = [64, 256, 512, 1024, 2048, 4096, 8192]


def int16_streams(seed, nsamples):
    s16 = synth.noise_tones_cs16(seed, nsamples)
    return s16, synth.to_cf32(s16)


def nbytes(z):
    return z.size * z.itemsize


def run_cf32(ds, z, **kw):
    return device_run(ds, z.view(np.uint8), **kw)


def truth_cf32(N, z, repeats, window=None):
    """numpy complex128 of the float32 samples as stored: (-1)^n exact, one float32 window rounding, float64 transform
    and accumulate."""
    sign = (1 - 2 * (np.arange(N) % 2)).astype(np.float32)
    x = z[: N * repeats].view(np.float32).reshape(repeats, N, 2) * sign[None, :, None]
    if window is not None:
        x = x * np.asarray(window, dtype=np.float32)[None, :, None]
    assert x.dtype == np.float32
    spec = np.fft.fft(x[..., 0].astype(np.float64) + 1j * x[..., 1].astype(np.float64), axis=1)
    return (spec.real ** 2 + spec.imag ** 2).sum(axis=0)


# ---- 1. cf32 of integers == cs16; 2. exact scaling -------------------------------------------------------------------

@pytest.mark.parametrize("N", K1_SIZES)
@pytest.mark.parametrize("window", [False, True])
def test_cf32_of_integers_equals_cs16_and_scales_exactly(N, window):
    R = 37                                     # the last iteration is partly clamped
    s16, z = int16_streams(11, R * N)
    for flags in (0, NO_DMA):
        with engine(N, "cs16", window=window, flags=flags) as a, engine(N, "cf32", window=window, flags=flags) as b:
            assert b.sample_bytes == 8 and b.sample_format == _lib.FORMAT_CF32
            assert b.frames_in(nbytes(z)) == R
            want, n0, g0 = device_run(a, s16)
            got, n1, g1 = run_cf32(b, z)
            assert n0 == n1 == R
            assert same(got, want, g1, g0, "N=%d window=%s flags=%d" % (N, window, flags))
            scaled, _, _ = run_cf32(b, synth.to_cf32(s16, 2.0 ** -9))
            assert np.array_equal(scaled, got * 2.0 ** -18), (N, window, flags)


@pytest.mark.parametrize("N", [64, 512])
def test_second_iteration_of_every_workgroup(N):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    with engine(N, "cs16") as a, engine(N, "cf32") as b:
        _, _, (_, fpw) = run_cf32(b, synth.to_cf32(synth.noise_tones_cs16(12, N)))
        R = cus * 8 * fpw + 3                  # (no K1 kernel has more than 8 resident workgroups per CU)
        s16, z = int16_streams(13, R * N)
        want, n0, g0 = device_run(a, s16)
        got, n1, g1 = run_cf32(b, z)
    assert n0 == n1 == R
    assert R > g1[0] * g1[1] + 3, "workgroups take a second iteration"
    assert same(got, want, g1, g0, "N=%d frames=%d" % (N, R))


# ---- 3. Gaussian float32 against float64 truth ------------------------------------------------------------------------

@pytest.mark.parametrize("N,window", [(64, False), (512, False), (4096, False), (4096, True), (8192, False)])
def test_gaussian_cf32_against_truth(N, window):
    R = 80
    z = synth.gaussian_cf32(21, R * N)
    assert np.count_nonzero(z.view(np.uint32) & 0xff) > z.size, "full mantissas"
    w = synth.hann_window(N) if window else None
    truth = truth_cf32(N, z, R, w)
    with engine(N, "cf32", window=window) as ds:
        got, n, _ = run_cf32(ds, z)
    assert n == R
    err = float(np.max(np.abs(got - truth) / truth))
    print("N=%d window=%s cf32 vs float64 truth: %.3g (bar %.3g)" % (N, window, err, CF32_VS_TRUTH))
    assert err < CF32_VS_TRUTH


# ---- 4. device pointer alignment ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [512, 4096])
def test_device_pointer_alignment(N):
    R = 37
    _, z = int16_streams(31, R * N)
    with engine(N, "cf32") as ds:
        want, n0, g0 = run_cf32(ds, z)
        got, n1, g1 = run_cf32(ds, z, misalign=8)          # 8- but not 16-byte aligned: VGPR staging
        assert n0 == n1 == R
        assert same(got, want, g1, g0, "N=%d misaligned by 8" % N)
        with pytest.raises(rpf.RPFError) as e:
            run_cf32(ds, z, misalign=4)
        assert e.value.retval == rpf.ReturnValue.InvalidArgument


# ---- 5. overlapped frames -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("step", [256, 257])
def test_overlap_against_catch_all(step):
    N, R = 512, 37
    _, z = int16_streams(41, N + step * (R - 1))
    for flags in (0, NO_DMA):
        with engine(N, "cf32", step, flags=flags) as a, engine(N, "cf32", step, flags=CATCH_ALL) as b:
            got, n0, _ = run_cf32(a, z)
            want, n1, _ = run_cf32(b, z)
        assert n0 == n1 == R == frames_in(nbytes(z), N, step, 8)
        err = max_err_over_mean(got, want)
        print("N=%d step=%d flags=%d: K1 vs catch-all %.3g" % (N, step, flags, err))
        assert err < PARITY


# ---- 6. catch-all sizes ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,R", [(1000, 37), (5000, 37), (65536, 3)])
def test_catch_all_sizes_equal_cs16(N, R):
    s16, z = int16_streams(51, R * N)
    with engine(N, "cs16") as a, engine(N, "cf32") as b:
        want, n0, g0 = device_run(a, s16)
        got, n1, g1 = run_cf32(b, z)
        got8, _, _ = run_cf32(b, z, misalign=8)
    assert n0 == n1 == R and g0 == g1
    assert np.array_equal(got, want) and np.array_equal(got8, want)


# ---- 7. the queue path ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [4096, 5000])
def test_queue_path(N):
    R, buf_length = 37, 16384 + 8
    _, z = int16_streams(61, R * N + N // 3)
    assert buf_length % 8 == 0 and buf_length % (8 * N) != 0
    with engine(N, "cf32", buf_length=buf_length, repeats=1 << 40) as ds:
        assert ds.frames_in(nbytes(z)) == R
        want, n, _ = run_cf32(ds, z)
        got, done = ds.accumulate(z)                       # a complex64 array, viewed as bytes
        got_b, done_b = ds.accumulate(z.view(np.uint8))
    assert done == done_b == n == R
    err = max_rel(got, want)
    print("N=%d: queue vs device %.3g" % (N, err))
    assert err < SAME_KERNELS and np.array_equal(got, got_b)


def test_submit_of_half_a_sample_is_invalid_argument():
    with engine(4096, "cf32") as ds:
        ds.begin(4)
        buf = ds.acquire()
        with pytest.raises(rpf.RPFError) as e:
            ds.submit(buf, 4)
        assert e.value.retval == rpf.ReturnValue.InvalidArgument
        ds.unget(buf)
        assert ds.finish() == 0


# ---- 8. statistics, 9. series, 10. excision --------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [512, 1000])
def test_bin_stats_of_one_frame(N):
    _, z = int16_streams(71, N)
    with engine(N, "cf32", bin_stats=True) as ds:
        pwr, done = ds.accumulate(z, 1)
        s2, pk = ds.sum_sq.copy(), ds.peak.copy()
    assert done == 1 and pwr.min() > 0
    assert np.array_equal(pk, pwr) and np.array_equal(s2, pwr * pwr)


@pytest.mark.parametrize("N", [512, 4096])
def test_series_rows_equal_single_acquisitions(N):
    L, K = 3, 5
    _, z = int16_streams(81, K * L * N)
    with engine(N, "cf32") as ds:
        keep, ptr = to_device(z.view(np.uint8))
        out = torch.empty(K * N, dtype=torch.float64, device=DEV)
        k = ds.accumulate_device_series(ptr, nbytes(z), L, K, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        rows = out.cpu().numpy().reshape(K, N)
        assert k == K and ds.series_launches() == K, "spectrum by spectrum through the plain K1"
        for i in range(K):
            single, n, _ = run_cf32(ds, z[i * L * N: (i + 1) * L * N])
            assert n == L and np.array_equal(rows[i], single), i


def test_excision_with_infinite_limits_keeps_everything():
    N, L, K = 512, 8, 4
    _, z = int16_streams(91, K * L * N)
    with engine(N, "cf32", bin_stats=True) as ds:
        out, _, k = ds.accumulate_excised(z, L, -np.inf, np.inf)
    assert k == K and out[2].min() > 0
    assert np.array_equal(out[0], out[2])


# ---- 11. hops: the scan kernel, one launch for several acquisitions ------------------------------------------------------

# the tiny sizes' ring (64), the two-deep ring (512), the ring of depth 1 that only cf32 has, with two slots (4096) and
# with one (8192)
@pytest.mark.parametrize("N", [64, 512, 4096, 8192])
def test_cf32_hops_in_one_launch(N):
    """A cf32 scan against the cs16 scan of the same int16 values, both staging routes.  The hops are sized from the
    engine's own launch plan so that the launch has about 1.5 iterations per workgroup: some workgroups take a second
    iteration (the refill of the ring is read), ranges cross hop boundaries (the staging cursor turns into the next hop
    ahead of the compute cursor) and the last workgroups run out of iterations (the cursor parks)."""
    H, weights = 5, (1, 9, 2, 5, 7)
    with engine(N, "cf32") as probe:                       # (before any launch: the resident grid of the plan)
        grid, fpw = probe.launch_info()["grid"], probe.launch_info()["frames_per_wg"]
    total = grid * fpw * 3 // 2
    frames = [max(1, total * w // sum(weights)) + h for h, w in enumerate(weights)]     # (no multiples of fpw)
    hops16 = [synth.noise_tones_cs16(111 + h, frames[h] * N) for h in range(H)]
    hops32 = [synth.to_cf32(x).view(np.uint8) for x in hops16]

    def scan(ds, hops):
        keeps = [to_device(x) for x in hops]
        out = torch.empty(H * N, dtype=torch.float64, device=DEV)
        done = ds.accumulate_device_hops([p for _, p in keeps], [x.size for x in hops], [1 << 40] * H, out.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        li = ds.launch_info()
        return out.cpu().numpy().reshape(H, N), done, (li["grid"], li["frames_per_wg"])

    for flags in (0, NO_DMA):
        with engine(N, "cs16", flags=flags) as a, engine(N, "cf32", flags=flags) as b:
            assert H <= b.max_hops_per_launch()
            want, d0, g0 = scan(a, hops16)
            got, d1, g1 = scan(b, hops32)
            assert d0 == d1 == frames
            iterations = sum(-(-f // g1[1]) for f in frames)
            assert g1[0] < iterations < 2 * g1[0], "some workgroups take two iterations, some one"
            assert same(got, want, g1, g0, "N=%d flags=%d: scan of %d hops, %d frames" % (N, flags, H, sum(frames)))
            for h in (0, H - 1):
                single, n, _ = run_cf32(b, hops32[h].view(np.complex64))
                err = max_rel(got[h], single)
                print("N=%d flags=%d hop %d: scan vs single %.3g" % (N, flags, h, err))
                assert n == frames[h] and err < ADDITIVITY       # (the scan kernel partitions frames differently)


# ---- 12. the CLI ---------------------------------------------------------------------------------------------------------------

def cli_block(*args):
    r = subprocess.run([CLI] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [l for l in r.stdout.split("\n") if l.strip() and not l.startswith("#")]


def test_cli_replays_cf32(tmp_path):
    """The block of `rpf_power --format cf32 --input` is the spectrum of Datastore.accumulate on the file's first R
    frames, written as the reference writes it (the oracle's formatter, as the overlap test formats).  The CLI cuts
    the file into buffers of its own length, so the sums may be grouped differently than Python's (ADDITIVITY, 1e-12):
    a line may then differ from the formatted one, by one unit of the last of its printed digits at the most."""
    N, R, cfreq, rate = 4096, 64, 1420405752, 2000000
    _, z = int16_streams(101, (R + 3) * N)                 # (the file holds more than -n asks for)
    (tmp_path / "f.cf32").write_bytes(z.tobytes())
    got = cli_block("-b", str(N), "-n", str(R), "-q", "--input", str(tmp_path / "f.cf32"), "--format", "cf32")
    with engine(N, "cf32") as ds:
        pwr, done = ds.accumulate(z, R)
    assert done == R
    buf = ctypes.create_string_buffer(64 * N)
    oracle_lib().rpf_oracle_format_text(pwr.ctypes.data_as(dp), N, R, cfreq, rate, 0, None, buf, len(buf))
    want = [l for l in buf.value.decode().split("\n") if l.strip()]
    assert len(got) == len(want) == N
    differing = 0
    for lg, lw in zip(got, want):
        if lg == lw:
            continue
        differing += 1
        fg, fw = lg.split(), lw.split()
        assert fg[0] == fw[0]
        digits = len(fw[1].split(".")[1]) if "." in fw[1] else 0
        assert abs(round((float(fg[1]) - float(fw[1])) * 10 ** digits)) <= 1, (lg, lw)
    print("CLI vs Datastore.accumulate: %d of %d lines differ in the last printed digit" % (differing, N))


def test_cli_drops_a_trailing_half_sample(tmp_path):
    """A file that ends inside a sample: the file source keeps whole samples (as for every format) and the block is
    the block of the file without the odd bytes."""
    N, R = 512, 16
    _, z = int16_streams(102, R * N)
    (tmp_path / "whole.cf32").write_bytes(z.tobytes())
    (tmp_path / "odd.cf32").write_bytes(z.tobytes() + b"\x00\x00\x80\x7f")      # four bytes more: half a sample
    args = ("-b", str(N), "-q", "--format", "cf32", "--input")
    a = cli_block(*args, str(tmp_path / "whole.cf32"))
    b = cli_block(*args, str(tmp_path / "odd.cf32"))
    assert len(a) == N and a == b
