"""Cross-spectrum of two streams on the MI355X.  The definition (include/rpf_engine.h) ties the four output planes to
tested ground exactly: Saa and Sbb are what accumulate_device of the same engine writes, and Re Sab, Im Sab are the
finishing expression over those and over what a cf32 engine of the same N, window, step and flags computes from the
combined streams u and v of the host emulator (tests/emul/cross_emul.cpp, the kernels' own cross_core.h) -- so the main
test is bit identity, for every format, aligned and not.  Beside it: more than one chunk of scratch, known answers,
accuracy against float64 at the bar of cross_bars, the host entry across pieces, what a cross call leaves alone, what is
refused, and the CLI.  Each test prints the figures it judged."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, stats, synth
from helpers import ROOT, dp, max_err_over_mean, max_rel
import cross_bars
from parity_bars import VS_TRUTH
from test_cross import cross_err, emul_combine, emul_finish, format_cross_block, truth_cross
from test_gpu_sample_formats import device_run, to_device
from test_pfb import make_stream

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
FORMATS = ["cu8", "cs8", "cs16", "cf32"]
ADDITIVITY = 1e-12          # the same terms added in another grouping (double additions)


def engine(N, fmt, flags=0, step=None, windowed=False, **kw):
    kw.setdefault("buffers", 2)
    kw.setdefault("buf_length", 16384)
    return rpf.Datastore(rpf.Params(N=N, sample_format=fmt, frame_step=step, window=windowed, **kw),
                         synth.hann_window(N) if windowed else None, flags=flags)


@pytest.fixture(scope="module")
def cf32():
    """cf32 engines by (N, flags, step, windowed), shared by the tests of the module."""
    engines = {}

    def get(N, flags=0, step=None, windowed=False):
        key = (N, flags, step, windowed)
        if key not in engines:
            engines[key] = engine(N, "cf32", flags, step, windowed)
        return engines[key]

    yield get
    for ds in engines.values():
        ds.close()


def cross_run(ds, a, b, repeats=1 << 40, mis_a=0, mis_b=0):
    """((4, N) planes, frames, launch geometry) of one device-resident cross call."""
    N = ds.params.N
    keep_a, pa = to_device(a, mis_a)
    keep_b, pb = to_device(b, mis_b)
    out = torch.empty(4 * N, dtype=torch.float64, device=DEV)
    n = ds.accumulate_device_cross(pa, pb, a.size, repeats, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del keep_a, keep_b
    li = ds.launch_info()
    return out.cpu().numpy().reshape(4, N), n, (li["grid"], li["frames_per_wg"])


def two_streams(fmt, seed, nsamples):
    return make_stream(fmt, seed, nsamples), make_stream(fmt, seed + 1000, nsamples)


def definition(ds, cf, a, b, fmt):
    """The four planes by the definition: this engine on a and on b, the cf32 engine on the emulator's u and v, the
    emulator's finishing expression.  Returns (planes, frames, the cf32 engine's launch geometry)."""
    paa, n, _ = device_run(ds, a)
    pbb, _, _ = device_run(ds, b)
    u, v = emul_combine(a, b, fmt)
    puu, n0, g0 = device_run(cf, u.view(np.uint8).reshape(-1))
    pvv, _, _ = device_run(cf, v.view(np.uint8).reshape(-1))
    assert n == n0
    return emul_finish(np.stack([paa, pbb, puu, pvv])), n, g0


def identity_case(cf32, N, fmt, counts, seed, flags=0, step=None, windowed=False):
    S = N if step is None else step
    with engine(N, fmt, flags, step, windowed) as ds:
        cf = cf32(N, flags, step, windowed)
        for frames in counts:
            a, b = two_streams(fmt, seed + frames, N + S * (frames - 1))
            assert ds.frames_in(a.size) == frames
            want, n0, g0 = definition(ds, cf, a, b, fmt)
            got, n1, g1 = cross_run(ds, a, b)
            assert n0 == n1 == frames and g0 == g1, (n0, n1, g0, g1)
            assert want[0].min() > 0 and want[1].min() > 0
            for p in range(4):
                assert np.array_equal(got[p], want[p]), (N, fmt, frames, p, max_rel(got[p], want[p]))


# ---- 1. bit identity with the definition -------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("N", [64, 512])
def test_bit_identity_with_the_definition(cf32, N, fmt):
    identity_case(cf32, N, fmt, [1, 3, 37], seed=20)


def test_bit_identity_at_4096(cf32):
    identity_case(cf32, 4096, "cu8", [1, 3, 37], seed=21)


def test_bit_identity_without_lds_dma(cf32):
    identity_case(cf32, 512, "cu8", [37], seed=22, flags=_lib.FLAG_NO_LDS_DMA)


def test_bit_identity_under_a_window(cf32):
    identity_case(cf32, 512, "cs16", [3, 37], seed=23, windowed=True)


def test_bit_identity_with_overlapped_frames(cf32):
    """Frame step N/2 + 1: an odd number of samples in every span but a single frame's."""
    identity_case(cf32, 512, "cu8", [1, 2, 37], seed=24, step=257)


def test_bit_identity_where_the_two_engines_are_of_different_families(cf32):
    """N = 500 cu8: the engine runs the mixed-radix family, its cf32 engine the catch-all path; rows of 1000 bytes are
    no multiple of 16."""
    identity_case(cf32, 500, "cu8", [1, 12], seed=25)


# ---- 2. unaligned streams ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["cu8", "cf32"])
def test_streams_at_an_odd_sample_offset(fmt):
    N, frames = 512, 37
    a, b = two_streams(fmt, 30, N * frames)
    sb = _lib.SAMPLE_BYTES[fmt]
    with engine(N, fmt) as ds:
        want, n0, _ = cross_run(ds, a, b)
        for mis_a, mis_b in ((sb, 0), (0, sb), (sb, sb)):        # one sample in: a multiple of b, not of the pair's bytes
            got, n1, _ = cross_run(ds, a, b, mis_a=mis_a, mis_b=mis_b)
            assert n0 == n1 == frames
            assert np.array_equal(got, want), (fmt, mis_a, mis_b)
        for mis_a, mis_b in ((sb // 2, 0), (0, sb // 2)):        # half a sample
            with pytest.raises(rpf.RPFError) as e:
                cross_run(ds, a, b, mis_a=mis_a, mis_b=mis_b)
            assert e.value.retval == rpf.ReturnValue.InvalidArgument


# ---- 3. more than one chunk ------------------------------------------------------------------------------------------------

def in_units_of_the_powers(got, want):
    """Worst deviation of the four planes: the powers relative to themselves, Re and Im Sab in units of Saa + Sbb."""
    scale = want[0] + want[1]
    return max(max_rel(got[0], want[0]), max_rel(got[1], want[1]),
               float(np.max(np.abs(got[2] - want[2]) / scale)), float(np.max(np.abs(got[3] - want[3]) / scale)))


def test_more_than_one_chunk():
    N, first, frames = 8192, 1024, 1024 + 100                       # 64 MB of cf32 are 1024 frames of this size
    a, b = synth.uniform_iq(40, N * frames), synth.uniform_iq(41, N * frames)
    with engine(N, "cu8") as ds:
        got, n, _ = cross_run(ds, a, b)
        cut = 2 * N * first
        head, n0, _ = cross_run(ds, a[:cut], b[:cut])               # each slice is one chunk: the definition, bit for bit
        tail, n1, _ = cross_run(ds, a[cut:], b[cut:])
        assert n == frames and n0 == first and n1 == frames - first
        err = in_units_of_the_powers(got, head + tail)
        print("N=%d, %d frames in two chunks vs the sum of its single-chunk slices: %.3g" % (N, frames, err))
        assert err < ADDITIVITY
        # a quota that cuts inside the first chunk: the slice's bits
        part, n2, _ = cross_run(ds, a, b, repeats=first)
        assert n2 == first and np.array_equal(part, head)


# ---- 4. known answers ---------------------------------------------------------------------------------------------------------

KNOWN_BAR = cross_bars.BAR[("cu8", 512, False)]


def test_a_stream_with_itself():
    N, frames = 512, 80
    a = synth.uniform_iq(50, N * frames)
    with engine(N, "cu8") as ds:
        got, n, _ = cross_run(ds, a, a.copy())
    assert n == frames and np.array_equal(got[0], got[1])
    err = max_rel(got[2], got[0])
    g = stats.coherence(got)
    print("b = a: Re Sab vs Saa %.3g; |coherence - 1| %.3g, largest Im Sab / Saa %.3g (bar %.3g)"
          % (err, np.max(np.abs(g - 1.0)), np.max(np.abs(got[3]) / got[0]), KNOWN_BAR))
    assert err < ADDITIVITY
    assert np.max(np.abs(g - 1.0)) < KNOWN_BAR


def test_a_stream_with_itself_times_i():
    N, frames = 512, 80
    a = np.minimum(synth.uniform_iq(51, N * frames), 254).astype(np.uint8)      # values in [-127, 127]
    va = a.astype(np.int16).reshape(-1, 2) - 127
    b = (np.stack([-va[:, 1], va[:, 0]], axis=1) + 127).astype(np.uint8).reshape(-1)        # b = i a = (-aQ, aI)
    with engine(N, "cu8") as ds:
        got, n, _ = cross_run(ds, a, b)
    assert n == frames
    m = 0.5 * (got[0] + got[1])
    floor = np.maximum(m, np.median(m))
    e_im, e_re = float(np.max(np.abs(got[3] + got[0]) / floor)), float(np.max(np.abs(got[2]) / floor))
    print("b = i a: Im Sab + Saa %.3g, Re Sab %.3g (bar %.3g)" % (e_im, e_re, KNOWN_BAR))
    assert e_im < KNOWN_BAR and e_re < KNOWN_BAR


def test_a_circular_shift_of_every_frame():
    N, frames, d = 512, 80, 3
    a = synth.uniform_iq(52, N * frames)
    b = np.roll(a.reshape(frames, N, 2), d, axis=1).reshape(-1).copy()
    saa, sbb, sab = truth_cross(a, b, "cu8", N)
    with engine(N, "cu8") as ds:
        got, n, _ = cross_run(ds, a, b)
    assert n == frames
    g = stats.coherence(got)
    dphi = np.angle(np.exp(1j * (stats.cross_phase(got) - np.angle(sab))))
    print("b = every frame of a shifted by %d: |coherence - 1| %.3g, phase vs float64 %.3g rad (bar %.3g)"
          % (d, np.max(np.abs(g - 1.0)), np.max(np.abs(dphi)), KNOWN_BAR))
    assert np.max(np.abs(g - 1.0)) < KNOWN_BAR
    assert np.max(np.abs(dphi)) < KNOWN_BAR


# ---- 5. accuracy against float64 ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,N,windowed", cross_bars.ACCURACY_CASES)
def test_accuracy_against_float64(fmt, N, windowed):
    a, b = cross_bars.accuracy_streams(fmt, N)
    window = synth.hann_window(N) if windowed else None
    saa, sbb, sab = truth_cross(a, b, fmt, N, window=window)
    with engine(N, fmt, windowed=windowed) as ds:
        got, n, _ = cross_run(ds, a, b)
        paa, _, _ = device_run(ds, a)
        pbb, _, _ = device_run(ds, b)
    assert n == cross_bars.ACCURACY_FRAMES
    key = (fmt, N, windowed)
    err = cross_err(got, saa, sbb, sab)
    e_a, e_b = max_err_over_mean(got[0], saa), max_err_over_mean(got[1], sbb)
    print("%s N=%d %s: Sab vs float64 %.3g (bar %.3g = twice the CPU float32 path's %.3g); Saa %.3g, Sbb %.3g (bar %.3g); "
          "mean coherence %.3f" % (fmt, N, "hann" if windowed else "rect", err, cross_bars.BAR[key], cross_bars.CPU_F32[key],
                                   e_a, e_b, VS_TRUTH, float(np.mean(stats.coherence(got)))))
    assert np.array_equal(got[0], paa) and np.array_equal(got[1], pbb)        # the plain engine's bits ...
    assert e_a < VS_TRUTH and e_b < VS_TRUTH                                  # ... at the plain engine's bar
    assert err < cross_bars.BAR[key]


# ---- 6. the host entry across pieces ------------------------------------------------------------------------------------------------

def test_host_entry_across_pieces():
    N, frames = 8192, 2048 + 37                                     # 68 MB per stream: two pieces of the host loop
    a, b = two_streams("cs16", 60, N * frames)
    with engine(N, "cs16") as ds:
        got, n = ds.accumulate_cross(a, b)
        want, n0, _ = cross_run(ds, a, b)
    assert n == n0 == frames
    err = in_units_of_the_powers(got, want)
    print("N=%d cs16, %d frames: accumulate_cross in two pieces vs accumulate_device_cross %.3g" % (N, frames, err))
    assert err < ADDITIVITY


# ---- 7. the engine's state is left alone -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["cu8", "cf32"])
def test_a_cross_call_leaves_the_engine_alone(fmt):
    N, frames = 512, 37
    a, b = two_streams(fmt, 70, N * frames)
    with engine(N, fmt, repeats=1 << 40) as ds:
        pwr, done = ds.accumulate(a)
        before, _, g_before = device_run(ds, a)
        first, n, _ = cross_run(ds, a, b)
        assert n == frames and done == frames
        lib, held = rpf.load(), np.zeros(N)
        assert lib.rpf_get_power(ds._handle, held.ctypes.data_as(dp)) == 0
        assert np.array_equal(held, pwr) and lib.rpf_get_repeats_done(ds._handle) == frames
        after, _, g_after = device_run(ds, a)
        assert g_before == g_after and np.array_equal(before, after)
        second, _, _ = cross_run(ds, a, b)
        assert np.array_equal(first, second)
        host, n1 = ds.accumulate_cross(a, b)
        assert n1 == frames and np.array_equal(host, first)             # one piece, one chunk: the same launches
        again, done = ds.accumulate(a)
        assert done == frames and max_rel(again, pwr) < 1e-13           # (the queue path: same kernels, same reduce order)
        # a quota, and streams without a whole frame
        part, n2, _ = cross_run(ds, a, b, repeats=5)
        want, _, _ = cross_run(ds, a[:5 * N * ds.sample_bytes], b[:5 * N * ds.sample_bytes])
        assert n2 == 5 and np.array_equal(part, want)
        short = ds.sample_bytes * (N - 1)
        none, n3, _ = cross_run(ds, a[:short], b[:short])
        assert n3 == 0 and np.array_equal(none, np.zeros((4, N)))


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------

def refused(call, part=None):
    with pytest.raises(rpf.RPFError) as e:
        call()
    assert e.value.retval == rpf.ReturnValue.InvalidArgument, str(e.value)
    if part:
        assert part in str(e.value), str(e.value)


def test_refused_configurations():
    N, frames = 512, 8
    a, b = two_streams("cu8", 80, N * (frames + 4))
    keep_a, pa = to_device(a)
    keep_b, pb = to_device(b)
    out = torch.zeros(4 * N + 2, dtype=torch.float64, device=DEV)
    with engine(N, "cu8", bin_stats=True) as ds:
        refused(lambda: ds.accumulate_device_cross(pa, pb, a.size, frames, out.data_ptr()), "RPF_FLAG_BIN_STATS")
        refused(lambda: ds.accumulate_cross(a, b), "RPF_FLAG_BIN_STATS")
    with rpf.Datastore(rpf.Params(N=N, pfb_taps=4, buffers=2, buf_length=16384)) as ds:
        refused(lambda: ds.accumulate_device_cross(pa, pb, a.size, frames, out.data_ptr()), "PFB")
        refused(lambda: ds.accumulate_cross(a, b), "PFB")
    # a kernel variant other than 0: the shipped library has none, so no such engine exists to make the call on
    refused(lambda: engine(N, "cu8", flags=1 << 8))
    with engine(N, "cs16") as ds:
        n4 = a.size // 4 * 4
        refused(lambda: ds.accumulate_device_cross(0, pb, n4, frames, out.data_ptr()), "NULL")
        refused(lambda: ds.accumulate_device_cross(pa, 0, n4, frames, out.data_ptr()), "NULL")
        refused(lambda: ds.accumulate_device_cross(pa, pb, n4, frames, 0), "NULL")
        refused(lambda: ds.accumulate_device_cross(pa, pb, n4 - 2, frames, out.data_ptr()), "multiple of the sample size")
        refused(lambda: ds.accumulate_cross(a[:n4 - 2], b[:n4 - 2]), "multiple of the sample size")
        refused(lambda: ds.accumulate_device_cross(pa, pb, n4, frames, out.data_ptr() + 8), "16-byte aligned")
        refused(lambda: ds.accumulate_device_cross(pa + 2, pb, n4, frames, out.data_ptr()), "aligned")
        refused(lambda: ds.accumulate_device_cross(pa, pb + 2, n4, frames, out.data_ptr()), "aligned")
        refused(lambda: ds.accumulate_device_cross(pa, pb, n4, -1, out.data_ptr()), "repeats")
        # ... and the engine still works
        got, n, _ = cross_run(ds, a[:n4], b[:n4])
        assert n == ds.frames_in(n4) and got[0].min() > 0
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0                             # nothing was launched
    del keep_a, keep_b


def test_a_nan_in_b_stays_out_of_saa():
    N, frames = 512, 9
    a, b = synth.gaussian_cf32(81, N * frames), synth.gaussian_cf32(82, N * frames)
    b[4 * N + 17] = np.float32(np.nan) + 0j
    with engine(N, "cf32") as ds:
        got, n, _ = cross_run(ds, a.view(np.uint8), b.view(np.uint8))
    assert n == frames
    assert np.isfinite(got[0]).all() and got[0].min() > 0
    assert np.isnan(got[1]).all() and np.isnan(got[2]).all() and np.isnan(got[3]).all()


# ---- 9. the CLI ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["cu8", "cs16"])
def test_cli_writes_the_block_of_accumulate_cross(tmp_path, fmt):
    """The block of `rpf_power --input a --cross b -b 512` is the four planes of Datastore.accumulate_cross over the whole
    frames of the shorter file, written by the rules of the option (the C++ host's writer, which tests/test_cross.py
    checks against numpy): the CLI reads both files in one piece each here, so the lines are equal as text."""
    N, frames = 512, 21
    sb = _lib.SAMPLE_BYTES[fmt]
    a, b = two_streams(fmt, 90, N * frames + N // 2 + 1)             # both files hold half a frame more than they give
    longer = np.concatenate([b, make_stream(fmt, 92, 3 * N)])       # ... and b three frames more than a
    (tmp_path / "a.iq").write_bytes(a.tobytes())
    (tmp_path / "b.iq").write_bytes(b.tobytes())
    (tmp_path / "b_longer.iq").write_bytes(longer.tobytes())
    with engine(N, fmt) as ds:
        whole = sb * N * frames
        planes, n = ds.accumulate_cross(a[:whole], b[:whole])
    assert n == frames
    want = format_cross_block(planes, frames, N)
    for other, differ in (("b.iq", False), ("b_longer.iq", True)):
        r = subprocess.run([CLI, "-b", str(N), "--format", fmt, "--input", str(tmp_path / "a.iq"), "--cross", str(tmp_path / other)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        head = [l for l in r.stdout.split("\n") if l.startswith("#")]
        assert head[-1] == ("# frequency [Hz] power spectral density a [dB/Hz] power spectral density b [dB/Hz] "
                            "coherence phase [rad]")
        got = [l for l in r.stdout.split("\n") if l.strip() and not l.startswith("#")]
        assert got == want, (other, [(g, w) for g, w in zip(got, want) if g != w][:3])
        note = [l for l in r.stderr.split("\n") if l.startswith("Cross-spectrum:")]
        assert len(note) == 1 and ("%d frames" % frames) in note[0] and (("differ in length" in note[0]) == differ), r.stderr
