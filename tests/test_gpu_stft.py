"""Short-time Fourier transform on the MI355X (include/rpf_engine.h, rpf_stft_device).  The definition ties a row to
tested ground exactly: re^2 + im^2 of a row, formed in double, is bit for bit what accumulate_device of the same engine
writes for that frame alone -- so the main tests are bit identities: K1's store kernels at every size, window form and
format over a second iteration, a ragged last one and a ring wrap; both staging routes; overlapped frames against the
materialised ones; the catch-all route over three batches; a PFB engine against the cf32 engine on the emulator's folded
frames.  Beside them: accuracy against float64 at the bar of stft_bars, the edges, what is refused, and the host entry
over three pieces.  Each test prints the figures it judged."""
import os
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, pfb, stft, synth
from helpers import ROOT, max_rel
import stft_bars
from test_gpu_sample_formats import to_device
from test_pfb import emul_fold, make_stream

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")
ADDITIVITY = 1e-12          # the same terms added in another grouping (double additions)
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
K1_SIZES = [64, 128, 256, 512, 1024, 2048, 4096, 8192]
SENTINEL = -12345.5


def engine(N, fmt="cu8", hann=False, step=None, flags=0, **kw):
    kw.setdefault("buffers", 2)
    kw.setdefault("buf_length", 16384)
    w = synth.hann_window(N) if hann else None
    return rpf.Datastore(rpf.Params(N=N, window=hann, frame_step=step, sample_format=fmt, **kw), w, flags=flags)


def cuda_stream():
    return torch.cuda.current_stream().cuda_stream


def stft_rows(ds, stream, max_frames=1 << 40, misalign=0, rows=None):
    """(rows x N complex64 as the device buffer holds them after the call, F): the buffer starts filled with SENTINEL."""
    stream = np.ascontiguousarray(stream).reshape(-1).view(np.uint8)
    keep, ptr = to_device(stream, misalign)
    F = max(min(max_frames, ds.frames_in(stream.size)), 0)
    out = torch.full((max(rows or F, 1), ds.params.N, 2), SENTINEL, dtype=torch.float32, device=DEV)
    n = ds.stft_device(ptr, stream.size, max_frames, out.data_ptr(), cuda_stream())
    torch.cuda.synchronize()
    del keep
    return out.cpu().numpy().view(np.complex64)[..., 0], n


def power_of(rows):
    """re re + im im in double: both squares exact, one rounding."""
    re, im = rows.real.astype(np.float64), rows.imag.astype(np.float64)
    return re * re + im * im


class Resident:
    """A stream in HBM and the powers accumulate_device gives for single frames of it and for all of it."""

    def __init__(self, ds, stream):
        self.ds, self.stream = ds, np.ascontiguousarray(stream).reshape(-1).view(np.uint8)
        self.keep, self.ptr = to_device(self.stream)
        self.out = torch.empty(ds.params.N, dtype=torch.float64, device=DEV)

    def frame_power(self, f):
        off = ds_pitch(self.ds) * f
        n = self.ds.accumulate_device(self.ptr + off, self.ds.frame_span(1), 1, self.out.data_ptr(), cuda_stream())
        torch.cuda.synchronize()
        assert n == 1
        return self.out.cpu().numpy()

    def power(self):
        n = self.ds.accumulate_device(self.ptr, self.stream.size, 1 << 40, self.out.data_ptr(), cuda_stream())
        torch.cuda.synchronize()
        return self.out.cpu().numpy(), n


def ds_pitch(ds):
    return ds.sample_bytes * ds.params.frame_step


def resident_grid(ds):
    """(grid, fpw) of the store kernels' resident grid: calls over zeros until the frames, not the grid, are the more."""
    frames = 64
    while True:
        z = torch.zeros(ds.frame_span(frames), dtype=torch.uint8, device=DEV)
        out = torch.empty((frames, ds.params.N, 2), dtype=torch.float32, device=DEV)
        assert ds.stft_device(z.data_ptr(), z.numel(), frames, out.data_ptr(), cuda_stream()) == frames
        torch.cuda.synchronize()
        li = ds.launch_info()
        if li["grid"] * li["frames_per_wg"] < frames:
            return li
        frames *= 4
        assert frames <= 1 << 20


def check_identity(ds, stream, rows, frames, what):
    res = Resident(ds, stream)
    for f in frames:
        want = res.frame_power(f)
        assert want.min() > 0
        assert np.array_equal(power_of(rows[f]), want), (what, f, max_rel(power_of(rows[f]), want))
    whole, n = res.power()
    assert n == rows.shape[0]
    err = max_rel(power_of(rows).sum(axis=0), whole)
    print("%s: frames %s bit for bit; sum over %d rows against the whole stream %.3g (ADDITIVITY %.0e)"
          % (what, sorted(set(frames)), n, err, ADDITIVITY))
    assert err <= ADDITIVITY


# ---- 1. identity, native route ----------------------------------------------------------------------------------------

NATIVE = [(N, "cu8") for N in K1_SIZES] + [(N, fmt) for fmt in ("cs16", "cf32") for N in (64, 512, 1024, 4096, 8192)]


@pytest.mark.parametrize("hann", [False, True], ids=["rect", "hann"])
@pytest.mark.parametrize("N,fmt", NATIVE)
def test_rows_square_to_the_power_of_their_frame_on_the_native_route(N, fmt, hann):
    with engine(N, fmt, hann) as ds:
        li = resident_grid(ds)
        grid, fpw = li["grid"], li["frames_per_wg"]
        assert li["lds_bytes"] > 0 and li["block"] >= 256
        F = grid * fpw + fpw + 1              # a second iteration, a ragged last one, a ring wrap
        stream = make_stream(fmt, 700 + N, F * N)
        rows, n = stft_rows(ds, stream)
        assert n == F == rows.shape[0]
        li2 = ds.launch_info()
        assert li2["grid"] == grid and li2["lds_bytes"] == li["lds_bytes"]
        check_identity(ds, stream, rows, [0, 1, fpw - 1, grid * fpw, F - 1],
                       "N=%d %s %s grid %d x %d" % (N, fmt, "hann" if hann else "rect", grid, fpw))



# A workgroup's first RAWD iterations are fed by the kernel's prologue; from iteration RAWD on every frame comes from a
# ring slot refilled inside the loop, between the row stores, behind the counted wait.  (cu8 ring depths, k1_sizes.h: 4 up
# to 256 bins, 2 beyond.)
@pytest.mark.parametrize("strided", [False, True], ids=["plain", "strided"])
@pytest.mark.parametrize("N,rawd", [(64, 4), (512, 2), (4096, 2)])
def test_rows_of_frames_staged_inside_the_loop(N, rawd, strided):
    S = N // 2 if strided else N
    with engine(N, "cu8", step=S) as ds:
        li = resident_grid(ds)
        per_iteration = li["grid"] * li["frames_per_wg"]
        F = (rawd + 1) * per_iteration + 1          # iteration RAWD in full, the first of RAWD + 1
        stream = make_stream("cu8", 750 + N, N + S * (F - 1))
        rows, n = stft_rows(ds, stream)
        assert n == F and ds.launch_info()["grid"] == li["grid"]
        first = rawd * per_iteration
        check_identity(ds, stream, rows, [first - 1, first, first + 1, first + per_iteration // 2, F - 2, F - 1],
                       "N=%d cu8 ring %d %s, %d frames per iteration" % (N, rawd, "strided" if strided else "plain", per_iteration))


# ---- 2. staging and alignment -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["cu8", "cf32"])
@pytest.mark.parametrize("N", [512, 4096])
def test_a_stream_one_sample_off_gives_the_aligned_rows(N, fmt):
    with engine(N, fmt) as ds:
        F = 3 * 64 + 5
        stream = make_stream(fmt, 800 + N, F * N)
        aligned, n0 = stft_rows(ds, stream)
        shifted, n1 = stft_rows(ds, stream, misalign=_lib.SAMPLE_BYTES[fmt])
        assert n0 == n1 == F
        assert np.array_equal(aligned.view(np.uint32), shifted.view(np.uint32))
    with engine(N, fmt, flags=_lib.FLAG_NO_LDS_DMA) as ds:
        plain, n2 = stft_rows(ds, stream)
        assert n2 == F and np.array_equal(aligned.view(np.uint32), plain.view(np.uint32))


# ---- 3. overlapped frames ---------------------------------------------------------------------------------------------

def materialised(stream, fmt, N, S, F):
    b = _lib.SAMPLE_BYTES[fmt]
    raw = np.ascontiguousarray(stream).reshape(-1).view(np.uint8)
    return np.concatenate([raw[f * b * S: f * b * S + b * N] for f in range(F)])


@pytest.mark.parametrize("fmt", ["cu8", "cf32"])
@pytest.mark.parametrize("N", [512, 4096])
@pytest.mark.parametrize("half_plus", [0, 1])
def test_overlapped_rows_are_the_rows_of_the_materialised_frames(N, fmt, half_plus):
    S, F = N // 2 + half_plus, 45
    stream = make_stream(fmt, 900 + N, N + S * (F - 1))
    with engine(N, fmt, hann=True, step=S) as ds:
        got, n = stft_rows(ds, stream)
    with engine(N, fmt, hann=True) as ds:
        want, m = stft_rows(ds, materialised(stream, fmt, N, S, F))
    assert n == m == F
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- 4. catch-all route -----------------------------------------------------------------------------------------------

def generic_batch(N):
    return max(1, min(64, (1 << 22) // N))


@pytest.mark.parametrize("N,fmt,hann", [(16384, "cu8", False), (16384, "cu8", True), (16384, "cf32", False),
                                        (16384, "cf32", True), (65536, "cu8", False), (65536, "cf32", False),
                                        (4096, "cu8", False), (4096, "cf32", False)])
def test_rows_square_to_the_power_of_their_frame_on_the_catch_all_route(N, fmt, hann):
    B = generic_batch(N)
    F = 2 * B + 5                            # three batches, the last ragged
    stream = make_stream(fmt, 1000 + N, F * N)
    with engine(N, fmt, hann, flags=_lib.FLAG_CATCH_ALL) as ds:
        rows, n = stft_rows(ds, stream)
        assert n == F
        assert ds.launch_info()["lds_bytes"] == 0
        check_identity(ds, stream, rows, [0, B - 1, B, 2 * B + 4], "catch-all N=%d %s %s" % (N, fmt, "hann" if hann else "rect"))
    if N >= 16384:
        # the engine of the family that serves the size for power takes the same route, by its catch-all twin
        with engine(N, fmt, hann) as ds:
            twin, m = stft_rows(ds, stream)
            assert m == F and ds.launch_info()["lds_bytes"] == 0
        assert np.array_equal(twin.view(np.uint32), rows.view(np.uint32))


@pytest.mark.parametrize("fmt", ["cu8", "cf32"])
def test_overlapped_rows_on_the_catch_all_route(fmt):
    N = 16384
    S, F = N // 2 + 1, 70
    stream = make_stream(fmt, 1100, N + S * (F - 1))
    with engine(N, fmt, step=S) as ds:
        got, n = stft_rows(ds, stream)
    with engine(N, fmt, flags=_lib.FLAG_CATCH_ALL) as ds:
        want, m = stft_rows(ds, materialised(stream, fmt, N, S, F))
    assert n == m == F
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- 5. accuracy against float64 --------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,N,form", [c for c in stft_bars.ACCURACY_CASES if c[2] != "pfb"])
def test_accuracy_against_float64(fmt, N, form):
    """err of stft_bars against stft.reference, at most twice the CPU float32 path's.  Measured on the MI355X:
    stft_bars.MEASURED."""
    case = (fmt, N, form)
    stream = stft_bars.accuracy_stream(*case)
    window, _, _ = stft_bars.case_arguments(*case)
    with engine(N, fmt, form == "hann") as ds:
        rows, n = stft_rows(ds, stream)
    want = stft.reference(stream, N, fmt, window=window)
    assert n == stft_bars.ACCURACY_FRAMES == want.shape[0]
    err = stft_bars.err(rows, want)
    print("STFT accuracy %s N=%d %s: err %.3e, CPU float32 path %.3e, ratio %.2f (bar 2)"
          % (fmt, N, form, err, stft_bars.CPU_F32[case], err / stft_bars.CPU_F32[case]))
    assert err <= stft_bars.BAR[case]


# ---- 6. PFB: the channelizer ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["cu8", "cf32"])
def test_pfb_rows_are_the_cf32_engines_rows_of_the_folded_frames(fmt):
    N, T, F = 512, 4, 2 * 16 + 5
    h = pfb.coefficients(N, T)
    stream = make_stream(fmt, 1200, (F + T - 1) * N)
    with engine(N, fmt, pfb_taps=T) as ds:
        got, n = stft_rows(ds, stream)
        assert n == F == ds.frames_in(stream.size)
        check_identity(ds, stream, got, [0, 1, F - 1], "PFB N=%d T=%d %s" % (N, T, fmt))
    z = emul_fold(stream, F, N, T, fmt, h)
    with engine(N, "cf32") as ds:
        want, m = stft_rows(ds, z.view(np.uint8).reshape(-1))
    assert m == F
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("fmt", ["cu8", "cf32"])
def test_pfb_accuracy_against_float64(fmt):
    case = (fmt, 512, "pfb")
    stream = stft_bars.accuracy_stream(*case)
    _, T, h = stft_bars.case_arguments(*case)
    with engine(512, fmt, pfb_taps=T) as ds:
        rows, n = stft_rows(ds, stream)
    want = stft.reference(stream, 512, fmt, taps=T, coeffs=h)
    assert n == stft_bars.ACCURACY_FRAMES == want.shape[0]
    err = stft_bars.err(rows, want)
    print("STFT accuracy %s N=512 pfb T=%d: err %.3e, CPU float32 path %.3e, ratio %.2f (bar 2)"
          % (fmt, T, err, stft_bars.CPU_F32[case], err / stft_bars.CPU_F32[case]))
    assert err <= stft_bars.BAR[case]


# ---- 7. edges ---------------------------------------------------------------------------------------------------------

def untouched(rows):
    return bool(np.all(rows.real == np.float32(SENTINEL)) and np.all(rows.imag == np.float32(SENTINEL)))


def test_rows_past_the_count_stay_and_the_count_is_capped():
    N, F = 512, 21
    stream = make_stream("cu8", 1300, F * N)
    with engine(N) as ds:
        full, n = stft_rows(ds, stream, rows=F + 3)
        assert n == F and untouched(full[F:]) and not untouched(full[:F])
        capped, n = stft_rows(ds, stream, max_frames=5, rows=F)
        assert n == 5 and untouched(capped[5:])
        assert np.array_equal(capped[:5].view(np.uint32), full[:5].view(np.uint32))
        for s, m in ((stream, 0), (stream[:2 * N - 1 - 1], 1 << 40)):      # no frame asked for; a sample short of one
            before = ds.launch_info()
            none, n = stft_rows(ds, s, max_frames=m, rows=2)
            assert n == 0 and untouched(none) and ds.launch_info() == before
        one_byte_short = torch.zeros(2 * N, dtype=torch.uint8, device=DEV)
        out = torch.full((1, N, 2), SENTINEL, dtype=torch.float32, device=DEV)
        with pytest.raises(rpf.RPFError):            # (an odd byte count is refused: cu8 samples are two bytes)
            ds.stft_device(one_byte_short.data_ptr(), 2 * N - 1, 1, out.data_ptr(), cuda_stream())
        assert ds.stft_device(one_byte_short.data_ptr(), 2 * N - 2, 1, out.data_ptr(), cuda_stream()) == 0
        torch.cuda.synchronize()
        assert untouched(out.cpu().numpy().view(np.complex64)[..., 0])


def test_a_nan_stays_in_its_row():
    N, F = 1024, 9
    clean = synth.gaussian_cf32(1400, F * N)
    dirty = clean.copy()
    dirty[3 * N + 17] = np.complex64(complex(np.nan, 1.0))
    with engine(N, "cf32") as ds:
        want, _ = stft_rows(ds, clean.view(np.uint8))
        got, n = stft_rows(ds, dirty.view(np.uint8))
    assert n == F
    assert np.all(np.isnan(got[3].real) | np.isnan(got[3].imag))
    keep = [f for f in range(F) if f != 3]
    assert np.array_equal(got[keep].view(np.uint32), want[keep].view(np.uint32))


def refused(ds, message, ptr, nbytes, max_frames, out):
    with pytest.raises(rpf.RPFError) as e:
        ds.stft_device(ptr, nbytes, max_frames, out.data_ptr() if hasattr(out, "data_ptr") else out, cuda_stream())
    assert e.value.retval == rpf.ReturnValue.InvalidArgument and message in str(e.value), str(e.value)


def test_refusals_name_their_reason_and_leave_the_buffer():
    N = 512
    dev_in = torch.zeros(8 * N * 4 + 64, dtype=torch.uint8, device=DEV)
    out = torch.full((4, N, 2), SENTINEL, dtype=torch.float32, device=DEV)
    p = dev_in.data_ptr()
    with engine(500) as ds:
        refused(ds, "power of two", p, 2 * 500 * 4, 4, out)
    with engine(N, bin_stats=True) as ds:
        refused(ds, "RPF_FLAG_BIN_STATS", p, 2 * N * 4, 4, out)
    # (a kernel variant other than 0 is refused by name too, but the shipped library creates no such engine)
    with engine(N, "cs16") as ds:
        refused(ds, "NULL", 0, 4 * N * 4, 4, out)
        refused(ds, "NULL", p, 4 * N * 4, 4, 0)
        refused(ds, "multiple of the sample size", p, 4 * N * 4 + 2, 4, out)
        refused(ds, "4-byte", p + 2, 4 * N * 4, 4, out)
        refused(ds, "16-byte aligned", p, 4 * N * 4, 4, out.data_ptr() + 8)
        refused(ds, "max_frames", p, 4 * N * 4, -1, out)
        ds.begin(4)
        refused(ds, "acquisition running", p, 4 * N * 4, 4, out)
        ds.finish()
        lib = _lib.load()
        assert lib.rpf_stft_device(None, p, 8, 1, out.data_ptr(), None, None) == 3
    torch.cuda.synchronize()
    assert untouched(out.cpu().numpy().view(np.complex64)[..., 0])


@pytest.mark.parametrize("N,flags", [(512, 0), (16384, 0), (4096, _lib.FLAG_CATCH_ALL)])
def test_nothing_of_the_engines_state_moves(N, flags):
    F = 12
    stream = make_stream("cu8", 1500 + N, F * N)
    with engine(N, flags=flags, buf_length=2 * N * 4) as ds:
        res = Resident(ds, stream)
        dev_before, _ = res.power()
        queue_before, done_before = ds.accumulate(stream, F)
        rows, n = stft_rows(ds, stream)
        assert n == F and ds.repeats_done == done_before == F
        assert np.array_equal(ds.pwr, queue_before)
        dev_after, _ = res.power()
        queue_after, done_after = ds.accumulate(stream, F)
        assert done_after == F
        assert np.array_equal(dev_after, dev_before) and np.array_equal(queue_after, queue_before)


# ---- 8. the host entry ------------------------------------------------------------------------------------------------

def test_host_entry_over_three_pieces_cut_by_the_rows():
    N, S = 8192, 64
    per_piece = (64 << 20) // (8 * N)         # the rows, not the input, are the bound (series_pieces.h, stft_pieces)
    F = 2 * per_piece + 5
    stream = make_stream("cu8", 1600, N + S * (F - 1))
    with engine(N, step=S) as ds:
        assert ds.frames_in(stream.size) == F
        want, n = stft_rows(ds, stream)
        got = ds.stft(stream)
        assert n == F and got.shape == (F, N) and got.dtype == np.complex64
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        few = ds.stft(stream, max_frames=3)
        assert few.shape == (3, N) and np.array_equal(few.view(np.uint32), want[:3].view(np.uint32))
        assert ds.stft(stream[:100]).shape == (0, N)


@pytest.mark.parametrize("extra,kw,route", [((), {}, "K1 store kernels"),
                                            (("--frame-overlap", "50"), {"step": 256}, "K1 store kernels"),
                                            (("--pfb", "4"), {"pfb_taps": 4}, "PFB fold, then K1 store kernels"),
                                            ((), {"N": 16384}, "catch-all transform")])
def test_cli_writes_the_rows_of_the_host_entry(tmp_path, extra, kw, route):
    kw = dict(kw)
    N = kw.pop("N", 512)
    stream = make_stream("cu8", 1700, 23 * N + 77)
    src, dst = tmp_path / "rec.cu8", tmp_path / "out.cf32"
    stream.tofile(src)
    r = subprocess.run([CLI, "--input", str(src), "--stft", str(dst), "-b", str(N), "-q", *extra], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == ""
    line = [l for l in r.stderr.splitlines() if l.startswith("STFT:")]
    with engine(N, **kw) as ds:
        want = ds.stft(stream)
    assert len(line) == 1 and ("%d frames of %d bins" % (want.shape[0], N)) in line[0] and line[0].endswith("route: " + route), r.stderr
    assert want.shape[0] >= 20
    got = np.fromfile(dst, dtype="<f4")
    assert got.size == want.size * 2
    assert np.array_equal(got.view(np.uint32), want.view(np.float32).reshape(-1).view(np.uint32))


def test_the_c_plus_plus_hosts_two_calls_give_the_engines_rows():
    """rpf_host::Datastore::stft and stft_device (host/datastore.h) through host_capi.cpp's rpf_host_stft."""
    import ctypes
    host = ctypes.CDLL(os.path.join(ROOT, "rtl-power-fftw_amd", "host", "librpf_host.so"))
    fn = host.rpf_host_stft
    fn.restype = ctypes.c_longlong
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_longlong,
                   ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    N, S, F = 1024, 640, 19
    stream = make_stream("cs16", 1800, N + S * (F - 1))
    with engine(N, "cs16", step=S) as ds:
        want, n = stft_rows(ds, stream)
    assert n == F
    msg = ctypes.create_string_buffer(512)
    got = np.full((F, N), np.nan, dtype=np.complex64)
    assert fn(N, _lib.FORMAT_CS16, S, stream.ctypes.data, stream.size, 1 << 40, got.ctypes.data, F, 0, msg, len(msg)) == F, msg.value
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    keep, ptr = to_device(stream)
    d_out = torch.full((F, N, 2), SENTINEL, dtype=torch.float32, device=DEV)
    assert fn(N, _lib.FORMAT_CS16, S, ptr, stream.size, 7, d_out.data_ptr(), F, 1, msg, len(msg)) == 7, msg.value
    torch.cuda.synchronize()
    dev = d_out.cpu().numpy().view(np.complex64)[..., 0]
    assert np.array_equal(dev[:7].view(np.uint32), want[:7].view(np.uint32)) and untouched(dev[7:])
    # a refusal comes back as the exit code with its message
    assert fn(500, _lib.FORMAT_CU8, 0, stream.ctypes.data, 4000, 1, got.ctypes.data, 1, 0, msg, len(msg)) == -3
    assert b"power of two" in msg.value
