"""Polyphase filter bank front end on the MI355X.  The definition (include/rpf_engine.h) ties a PFB engine to tested
ground exactly: its spectrum is what a rectangular cf32 engine computes from the folded frames z, and z is what the
host emulator (tests/emul/pfb_emul.cpp, the kernels' own pfb_core.h) computes -- so the main test is bit identity, for
every format, both kernel forms, every tap count with its own instantiation, aligned and not.  Beside it: more than one
64 MB chunk, the buffer queue with a carry of several rows, accuracy against float64 at the bar of pfb_bars, the
leakage the filter buys, what is refused, the hop entry and the CLI.  Each test prints the figures it judged."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, pfb, synth
from rtl_power_fftw_amd.datastore import frames_in
from helpers import ROOT, dp, max_err_over_mean, max_rel, oracle_lib
import pfb_bars
from test_gpu_sample_formats import device_run, to_device
from test_pfb import emul_fold, make_stream

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
FORMATS = ["cu8", "cs8", "cs16", "cf32"]
SLIDING = [1, 2, 3, 4, 8]
ADDITIVITY = 1e-12          # the same terms added in another grouping (double additions)


def segment_frames(T, fmt):
    """Output frames a lane of the fold kernel walks (csrc/rpf_pfb.hip, pfb_segment_frames)."""
    return 16 if fmt == "cf32" else 8


def pfb_engine(N, T, fmt, flags=0, coeffs=None, **kw):
    kw.setdefault("buffers", 2)
    kw.setdefault("buf_length", 16384)
    return rpf.Datastore(rpf.Params(N=N, pfb_taps=T, pfb_coeffs=coeffs, sample_format=fmt, **kw), flags=flags)


@pytest.fixture(scope="module")
def rect():
    """Rectangular cf32 engines by (N, flags), shared by the tests of the module."""
    engines = {}

    def get(N, flags=0):
        if (N, flags) not in engines:
            engines[(N, flags)] = rpf.Datastore(rpf.Params(N=N, sample_format="cf32", buffers=2, buf_length=16384), flags=flags)
        return engines[(N, flags)]

    yield get
    for ds in engines.values():
        ds.close()


def identity_case(rect, N, T, fmt, counts, seed, flags=0):
    h = pfb.coefficients(N, T)
    with pfb_engine(N, T, fmt, flags=flags) as ds:
        assert ds.pfb_taps == T and ds.sample_bytes == _lib.SAMPLE_BYTES[fmt] and ds.sample_format == _lib.FORMATS[fmt]
        for frames in counts:
            stream = make_stream(fmt, seed + frames, (frames + T - 1) * N)
            assert ds.frames_in(stream.size) == frames and ds.frame_span(frames) == stream.size
            z = emul_fold(stream, frames, N, T, fmt, h)
            want, n0, g0 = device_run(rect(N, flags), z.view(np.uint8).reshape(-1))
            got, n1, g1 = device_run(ds, stream)
            assert n0 == n1 == frames and g0 == g1, (n0, n1, g0, g1)
            assert want.min() > 0
            assert np.array_equal(got, want), (N, T, fmt, frames, max_rel(got, want))


# ---- 1. bit identity --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("T", SLIDING + [5])
@pytest.mark.parametrize("N", [64, 512])
def test_bit_identity_with_the_cf32_engine_on_the_emulators_frames(rect, N, T, fmt):
    L = segment_frames(T, fmt)
    identity_case(rect, N, T, fmt, [1, T, 2 * L + 5], seed=10 * T)        # the last: three segments, the third of 5 frames


def test_bit_identity_at_4096(rect):
    identity_case(rect, 4096, 4, "cu8", [1, 4, 2 * segment_frames(4, "cu8") + 5], seed=77)


def test_bit_identity_without_lds_dma(rect):
    identity_case(rect, 512, 4, "cu8", [37], seed=78, flags=_lib.FLAG_NO_LDS_DMA)


def test_bit_identity_on_the_catch_all_path(rect):
    """N = 500: rows of 1000 bytes, a multiple of 8 but not of 16."""
    identity_case(rect, 500, 4, "cu8", [12], seed=79)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("T", [4, 5])
def test_stream_at_an_odd_sample_offset(fmt, T):
    N, frames = 512, 2 * segment_frames(T, fmt) + 5
    stream = make_stream(fmt, 90 + T, (frames + T - 1) * N)
    b = _lib.SAMPLE_BYTES[fmt]
    with pfb_engine(N, T, fmt) as ds:
        want, n0, _ = device_run(ds, stream)
        got, n1, _ = device_run(ds, stream, misalign=b)          # one sample in: a multiple of b, not of 2b
        assert n0 == n1 == frames and np.array_equal(got, want)
        if b > 2:
            with pytest.raises(rpf.RPFError) as e:
                device_run(ds, stream, misalign=b // 2)
            assert e.value.retval == rpf.ReturnValue.InvalidArgument


# ---- 2. more than one chunk -------------------------------------------------------------------------------------------

def test_more_than_one_chunk(rect):
    N, T, frames = 8192, 2, 1024 + 100                              # 64 MB of folded frames are 1024 of them
    stream = make_stream("cu8", 5, (frames + T - 1) * N)
    h = pfb.coefficients(N, T)
    z = emul_fold(stream, frames, N, T, "cu8", h).view(np.uint8).reshape(-1)
    with pfb_engine(N, T, "cu8") as ds:
        got, n, _ = device_run(ds, stream)
        want, n0, _ = device_run(rect(N), z)
        assert n == n0 == frames
        err = max_rel(got, want)
        print("N=%d T=%d %d frames in two chunks vs the cf32 engine on all of z: %.3g" % (N, T, frames, err))
        assert err < ADDITIVITY
        # a quota that cuts inside the first chunk: one fold, one transform, the same bits
        got, n, _ = device_run(ds, stream, repeats=700)
        want, n0, _ = device_run(rect(N), z, repeats=700)
        assert n == n0 == 700 and np.array_equal(got, want)


# ---- 3. the buffer queue ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["cu8", "cs16"])
def test_queue_with_frames_across_buffers(fmt):
    N, T, R = 512, 4, 37
    b = _lib.SAMPLE_BYTES[fmt]
    capacity = -(-(3 * 2 * N + 2) // b) * b                         # three cu8 rows and a sample: no multiple of a row
    stream = make_stream(fmt, 33, (R + T - 1) * N + N // 3)
    assert capacity % (b * N) != 0 and capacity < b * T * N, "a frame spans more than one buffer"
    with pfb_engine(N, T, fmt, buffers=5, buf_length=capacity, repeats=1 << 40) as ds:
        assert ds.frames_in(stream.size) == R == frames_in(stream.size, N, N, b, taps=T)
        want, n, _ = device_run(ds, stream)
        got, done = ds.accumulate(stream)
        assert done == n == R
        err = max_rel(got, want)
        print("%s: queue vs device %.3g" % (fmt, err))
        assert err < ADDITIVITY
        part, _, _ = device_run(ds, stream, repeats=20)
        got, done = ds.accumulate(stream, 20)
        assert done == 20 and max_rel(got, part) < ADDITIVITY


def test_queue_carries_several_rows_between_staging_slots():
    """More than one 32 MB staging slot of 3074-byte buffers: the slot boundary falls inside a frame's span, more than
    one row before its end, and the carry brings those rows along."""
    N, T, b, capacity = 512, 4, 2, 3074
    slot = ((32 << 20) // capacity) * capacity
    assert slot % (b * N) > 0
    R = slot // (b * N) + 3000
    stream = synth.uniform_iq(44, (R + T - 1) * N)
    with pfb_engine(N, T, "cu8", buffers=5, buf_length=capacity, repeats=1 << 40) as ds:
        want, n, _ = device_run(ds, stream)
        got, done = ds.accumulate(stream)
        assert done == n == R
        err = max_rel(got, want)
        print("queue over two staging slots vs device: %.3g" % err)
        assert err < ADDITIVITY


# ---- 4. accuracy against float64 ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,N", pfb_bars.ACCURACY_CASES)
def test_accuracy_against_float64(fmt, N):
    T, frames = pfb_bars.ACCURACY_TAPS, pfb_bars.ACCURACY_FRAMES
    stream = pfb_bars.accuracy_stream(fmt, N)
    truth = pfb.spectrum(pfb.fold(stream, N, T, pfb.coefficients(N, T), fmt))
    with pfb_engine(N, T, fmt) as ds:
        got, n, _ = device_run(ds, stream)
    assert n == frames
    err = max_err_over_mean(got, truth)
    print("%s N=%d: PFB engine vs float64 %.3g (bar %.3g = twice the CPU float32 path's %.3g)"
          % (fmt, N, err, pfb_bars.BAR[(fmt, N)], pfb_bars.CPU_F32[(fmt, N)]))
    assert err < pfb_bars.BAR[(fmt, N)]


# ---- 5. what it buys ----------------------------------------------------------------------------------------------------------

def test_leakage_on_the_device():
    N, T, frames = 512, 4, 40
    n = np.arange((frames + T - 1) * N, dtype=np.float64)
    tone = 100.0 * np.exp(2j * np.pi * (N / 4 + 0.5) * n / N)
    stream = np.empty(2 * n.size, dtype=np.uint8)
    stream[0::2] = np.rint(tone.real) + 127
    stream[1::2] = np.rint(tone.imag) + 127
    k = N // 2 + N // 4
    with rpf.Datastore(rpf.Params(N=N, buffers=2, buf_length=16384)) as plain, pfb_engine(N, T, "cu8") as ds:
        p0, n0, _ = device_run(plain, stream[:2 * N * frames])
        p1, n1, _ = device_run(ds, stream)
    assert n0 == n1 == frames
    r0, r1 = p0[k + 3] / p0[k], p1[k + 3] / p1[k]
    print("p[k+3]/p[k]: plain %.3g, PFB %.3g (%.3g of it)" % (r0, r1, r1 / r0))
    assert 0.03 < r0 < 0.05 and r1 < 1e-3 * r0


# ---- 6. entry points --------------------------------------------------------------------------------------------------------------

def test_refused_entry_points_name_pfb():
    N, T = 512, 4
    stream = make_stream("cu8", 3, (16 + T - 1) * N)
    with pfb_engine(N, T, "cu8") as ds:
        keep, ptr = to_device(stream)
        out = torch.zeros(16 * 3 * N, dtype=torch.float64, device=DEV)
        calls = [lambda: ds.accumulate_device_series(ptr, stream.size, 4, 4, out.data_ptr()),
                 lambda: ds.accumulate_device_series_stats(ptr, stream.size, 4, 4, out.data_ptr()),
                 lambda: ds.accumulate_device_excised(ptr, stream.size, 4, 4, 0.0, 2.0, out.data_ptr()),
                 lambda: ds.accumulate_series(stream, 4),
                 lambda: ds.accumulate_series_stats(stream, 4),
                 lambda: ds.accumulate_excised(stream, 4, 0.0, 2.0),
                 lambda: ds.device_fused(ptr, stream.size, 16),
                 lambda: ds.device_fused_hops([ptr], [stream.size], [16]),
                 lambda: ds.device_reduce(out.data_ptr())]
        for call in calls:
            with pytest.raises(rpf.RPFError) as e:
                call()
            assert e.value.retval == rpf.ReturnValue.InvalidArgument and "PFB" in str(e.value), str(e.value)
        # ... and the engine still works
        got, n, _ = device_run(ds, stream)
        assert n == 16 and got.min() > 0


def test_hops_run_hop_by_hop():
    N, T, H = 512, 4, 3
    frames = [21, 1, 40]
    hops = [make_stream("cu8", 60 + h, (frames[h] + T - 1) * N) for h in range(H)]
    with pfb_engine(N, T, "cu8") as ds:
        keeps = [to_device(x) for x in hops]
        out = torch.empty(H * N, dtype=torch.float64, device=DEV)
        done = ds.accumulate_device_hops([p for _, p in keeps], [x.size for x in hops], [1 << 40] * H, out.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        rows = out.cpu().numpy().reshape(H, N)
        assert done == frames
        for h in range(H):
            single, n, _ = device_run(ds, hops[h])
            assert n == frames[h] and np.array_equal(rows[h], single), h


# ---- 7. the CLI ----------------------------------------------------------------------------------------------------------------------

def test_cli_replays_through_the_filter_bank(tmp_path):
    """The block of `rpf_power --pfb 4 -b 512 -n 20 --input rec.cu8` is the spectrum of Datastore.accumulate with the
    default prototype on the file's first 20 frames, written as the reference writes it (the oracle's formatter).  The
    CLI cuts the file into buffers of its own length, so a line may differ from the formatted one by one unit of the
    last of its printed digits."""
    N, T, R, cfreq, rate = 512, 4, 20, 1420405752, 2000000
    stream = synth.noise_tones_iq(8, (R + T + 5) * N)               # (the file holds more than -n asks for)
    (tmp_path / "rec.cu8").write_bytes(stream.tobytes())
    r = subprocess.run([CLI, "--pfb", str(T), "-b", str(N), "-n", str(R), "-q", "--input", str(tmp_path / "rec.cu8")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [l for l in r.stdout.split("\n") if l.strip() and not l.startswith("#")]
    with pfb_engine(N, T, "cu8") as ds:
        pwr, done = ds.accumulate(stream, R)
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
