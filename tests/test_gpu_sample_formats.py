"""Signed 8-bit (cs8) and signed 16-bit little-endian (cs16) I/Q on the MI355X.  The new formats are tied to the
parity-tested cu8 path by identities that hold exactly:

  1. cs8 stream u - 127 == cu8 stream u (no byte 255): the same floats leave the unpack;
  2. the cs16 stream holding int8 values == the cs8 stream of those values;
  3. cs16 stream 2^k v gives 4^k x the spectrum of cs16 stream v, exactly (powers of two scale every float32 and
     double operation exactly; nothing overflows or goes subnormal);
  4. full-range cs16 against numpy complex128 of the exactly unpacked samples, at the project's own bar.

"Equal" is np.array_equal whenever the two runs have the same launch geometry (grid, frames per workgroup: the same
frames then meet the same accumulators in the same order); if a cs16 instantiation comes out with another grid than
its cs8 counterpart the same doubles are added in another grouping and the bar is ADDITIVITY.  Every threshold is
imported from parity_bars.  Each test prints the figures it judged."""
import os
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, synth
from rtl_power_fftw_amd.datastore import frames_in
from helpers import ROOT, max_err_over_mean, max_rel, oracle_accumulate, truth_f64
from parity_bars import ADDITIVITY, PARITY, SAME_KERNELS, TOTAL_POWER_CATCH_ALL, VS_TRUTH
from test_frame_overlap import materialise

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
NO_DMA = _lib.FLAG_NO_LDS_DMA
CATCH_ALL = _lib.FLAG_CATCH_ALL

# (N, windowed): sizes of the LDS-resident kernel the identities are checked on
K1_CASES = [(64, False), (512, False), (4096, False), (4096, True), (8192, False)]


def to_device(stream, misalign=0):
    t = torch.empty(stream.size + 64, dtype=torch.uint8, device=DEV)
    t[misalign:misalign + stream.size].copy_(torch.from_numpy(np.ascontiguousarray(stream)))
    return t, t.data_ptr() + misalign


def device_run(ds, stream, repeats=1 << 40, misalign=0):
    """(spectrum, frames, launch geometry) of one device-resident acquisition."""
    keep, ptr = to_device(stream, misalign)
    out = torch.empty(ds.params.N, dtype=torch.float64, device=DEV)
    n = ds.accumulate_device(ptr, stream.size, repeats, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del keep
    li = ds.launch_info()
    return out.cpu().numpy(), n, (li["grid"], li["frames_per_wg"])


def engine(N, fmt="cu8", step=None, window=False, flags=0, **kw):
    w = synth.hann_window(N) if window else None
    return rpf.Datastore(rpf.Params(N=N, window=window, frame_step=step, sample_format=fmt, **kw), w, flags=flags)


def same(got, want, geom_got, geom_want, what):
    """The sense of "equal" of the module docstring; says which of the two it applied."""
    if geom_got == geom_want:
        print("%s: same geometry %s -> array_equal" % (what, geom_got))
        return np.array_equal(got, want)
    err = max_rel(got, want)
    print("%s: geometry %s vs %s -> ADDITIVITY, measured %.3g" % (what, geom_got, geom_want, err))
    return err < ADDITIVITY


def clamped_cu8(seed, nsamples):
    return np.minimum(synth.noise_tones_iq(seed, nsamples), 254).astype(np.uint8)


def full_range_cs8(seed, nsamples):
    """Uniform bytes read as signed: every int8 value, -128 included."""
    s = synth.uniform_iq(seed, nsamples)
    s[:4] = (0x80, 0x7F, 0x80, 0x80)
    return s


def truth_signed(N, values, repeats, window=None):
    """numpy complex128 of the signed samples `values` (I0, Q0, I1, ...): exact unpack, (-1)^n, one float32 window
    rounding, float64 transform and accumulate -- helpers.truth_f64 with v in place of v - 127."""
    sign = (1 - 2 * (np.arange(N) % 2)).astype(np.float32)
    total = np.zeros(N)
    chunk = max(1, (1 << 22) // N)
    for f0 in range(0, repeats, chunk):
        f1 = min(repeats, f0 + chunk)
        x = np.asarray(values[2 * N * f0: 2 * N * f1]).astype(np.float32).reshape(f1 - f0, N, 2)
        x = x * sign[None, :, None]
        if window is not None:
            x = x * np.asarray(window, dtype=np.float32)[None, :, None]
        z = x[..., 0].astype(np.float64) + 1j * x[..., 1].astype(np.float64)
        spec = np.fft.fft(z, axis=1)
        total += (spec.real ** 2 + spec.imag ** 2).sum(axis=0)
    return total


# ---- 1. cs8 == cu8 where both can say the same thing ------------------------------------------------------------------

@pytest.mark.parametrize("N,window", K1_CASES)
def test_cs8_equals_cu8_on_k1(N, window):
    R = 70
    u = clamped_cu8(31, R * N)
    s = synth.to_cs8(u)
    w = synth.hann_window(N) if window else None
    for step in (N, N // 2 + 1):
        frames = frames_in(u.size, N, step)
        for flags in (0, NO_DMA):
            for misalign in (0, 2):
                with engine(N, "cu8", step, window, flags) as a, engine(N, "cs8", step, window, flags) as b:
                    assert b.sample_bytes == 2 and b.sample_format == _lib.FORMAT_CS8
                    want, n0, g0 = device_run(a, u, misalign=misalign)
                    got, n1, g1 = device_run(b, s, misalign=misalign)
                assert n0 == n1 == frames
                assert g0 == g1, "cs8 shares cu8's staging: same launch geometry"
                assert np.array_equal(got, want), (N, step, flags, misalign)
        orc, _ = oracle_accumulate(N, materialise(u, N, step), frames, w)
        err = float(np.max(np.abs(want - orc) / np.abs(orc)))
        print("N=%d step=%d cu8 vs oracle %.3g" % (N, step, err))
        assert err < PARITY


# ---- 2. cs16 == cs8 on 8-bit values; 3. the high byte, exactly ---------------------------------------------------------

@pytest.mark.parametrize("N,window", K1_CASES)
def test_cs16_equals_cs8_and_scales_exactly_on_k1(N, window):
    R = 70
    s8 = full_range_cs8(32, R * N)
    s16 = synth.to_cs16(s8)
    assert s16.size == 2 * s8.size
    for step in (N, N // 2 + 1):
        frames = frames_in(s8.size, N, step)
        for flags in (0, NO_DMA):
            with engine(N, "cs8", step, window, flags) as a, engine(N, "cs16", step, window, flags) as b:
                assert b.sample_bytes == 4 and b.frames_in(s16.size) == frames
                want, n0, g0 = device_run(a, s8)
                for misalign in (0, 4):
                    got, n1, g1 = device_run(b, s16, misalign=misalign)
                    assert n0 == n1 == frames
                    assert same(got, want, g1, g0, "N=%d step=%d flags=%d misalign=%d" % (N, step, flags, misalign))
                # the same engine, the same geometry: powers of two scale exactly
                base, _, _ = device_run(b, s16)
                for shift in (8, 3):
                    scaled, _, _ = device_run(b, synth.to_cs16(s8, shift))
                    assert np.array_equal(scaled, float(4 ** shift) * base), (N, step, flags, shift)


# ---- 4. full-range cs16 against float64 truth --------------------------------------------------------------------------

@pytest.mark.parametrize("N,window", [(64, False), (512, False), (4096, False), (4096, True), (8192, False)])
def test_full_range_cs16_against_truth(N, window):
    R = 80
    s = synth.noise_tones_cs16(41, R * N)
    v = synth.cs16_values(s)
    assert int(v.max()) > 16384 and int(v.min()) < -16384, "the stream uses the high byte"
    w = synth.hann_window(N) if window else None
    truth = truth_signed(N, v, R, w)
    with engine(N, "cs16", window=window) as ds:
        got, n, _ = device_run(ds, s)
    assert n == R
    err = float(np.max(np.abs(got - truth) / truth))
    print("N=%d window=%s cs16 vs float64 truth: %.3g (bar VS_TRUTH %.3g)" % (N, window, err, VS_TRUTH))
    assert err < VS_TRUTH


# ---- 5. the catch-all route ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,R", [(500, 64), (2046, 64), (5000, 64), (16384, 12), (65536, 12)])
def test_catch_all_route(N, R):
    u = clamped_cu8(51, R * N)
    s8 = synth.to_cs8(u)
    # the comparator: cu8 on the catch-all path, against the unchanged oracle and float64 truth
    with engine(N, "cu8", flags=CATCH_ALL) as ds:
        ref, n, g0 = device_run(ds, u)
    assert n == R
    truth = truth_f64(N, u, R)
    o32, _ = oracle_accumulate(N, u, R, None, 32)
    e_t, e_o, e_p = max_err_over_mean(ref, truth), max_err_over_mean(ref, o32), abs(ref.sum() / truth.sum() - 1)
    print("N=%d catch-all cu8: vs truth %.3g vs oracle %.3g total power %.3g" % (N, e_t, e_o, e_p))
    assert e_t < PARITY and e_o < PARITY and e_p < TOTAL_POWER_CATCH_ALL
    # cs8 without the flag takes the same kernels after the loader
    with engine(N, "cs8") as ds:
        got8, n, g1 = device_run(ds, s8)
    assert n == R and g1 == g0
    assert np.array_equal(got8, ref)
    # cs16 by identities 2 and 3, over the full int8 range
    f8 = full_range_cs8(52, R * N)
    with engine(N, "cs8") as a, engine(N, "cs16") as b:
        want, _, _ = device_run(a, f8)
        got, n, _ = device_run(b, synth.to_cs16(f8))
        got4, _, _ = device_run(b, synth.to_cs16(f8), misalign=4)
        assert n == R and np.array_equal(got, want) and np.array_equal(got4, want)
        for shift in (8, 3):
            scaled, _, _ = device_run(b, synth.to_cs16(f8, shift))
            assert np.array_equal(scaled, float(4 ** shift) * want), (N, shift)


def test_catch_all_route_overlapped():
    N, R = 5000, 40
    step = N // 2 + 1
    f8 = full_range_cs8(53, N + step * (R - 1))
    with engine(N, "cs8", step) as a, engine(N, "cs16", step) as b, engine(N, "cs8") as flat:
        want, n0, _ = device_run(a, f8)
        got, n1, _ = device_run(b, synth.to_cs16(f8))
        side, n2, _ = device_run(flat, materialise(f8, N, step))
    assert n0 == n1 == n2 == R
    assert np.array_equal(got, want) and np.array_equal(want, side)


# ---- 6. the queue path ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [4096, 5000])
@pytest.mark.parametrize("buf_length", [2732, 16384 + 4, 174764])
def test_queue_path_cs16(N, buf_length):
    R = 37
    s = synth.noise_tones_cs16(61, R * N + N // 3)            # trailing samples that do not fill a frame
    s = s[: s.size - 4]
    assert buf_length % 4 == 0 and buf_length % (4 * N) != 0
    with engine(N, "cs16", buf_length=buf_length, repeats=1 << 40) as ds:
        assert ds.frames_in(s.size) == frames_in(s.size, N, N, 4) == R
        for quota in (1 << 40, R - 11):                       # no quota; one that ends in the middle of a buffer
            want, n, _ = device_run(ds, s, repeats=quota)
            got, done = ds.accumulate(s, quota)
            assert done == n == min(quota, R)
            err = max_rel(got, want)
            print("N=%d buffers of %d bytes quota %d: queue vs device %.3g" % (N, buf_length, quota, err))
            assert err < SAME_KERNELS


def test_submit_of_half_a_sample_is_invalid_argument():
    with engine(4096, "cs16") as ds:
        ds.begin(4)
        buf = ds.acquire()
        with pytest.raises(rpf.RPFError) as e:
            ds.submit(buf, 4 * 100 + 2)
        assert e.value.retval == rpf.ReturnValue.InvalidArgument
        ds.unget(buf)
        assert ds.finish() == 0


# ---- 7. hops ---------------------------------------------------------------------------------------------------------------

def test_cs16_hops_in_one_launch():
    N, H = 4096, 8
    frames = [23 + 5 * h for h in range(H)]
    hops8 = [full_range_cs8(70 + h, frames[h] * N) for h in range(H)]
    hops16 = [synth.to_cs16(x) for x in hops8]

    def scan(ds, hops):
        keeps = [to_device(x) for x in hops]
        out = torch.empty(H * N, dtype=torch.float64, device=DEV)
        done = ds.accumulate_device_hops([p for _, p in keeps], [x.size for x in hops], [1 << 40] * H, out.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        li = ds.launch_info()
        return out.cpu().numpy().reshape(H, N), done, (li["grid"], li["frames_per_wg"])

    with engine(N, "cs8") as a, engine(N, "cs16") as b:
        assert H <= b.max_hops_per_launch()
        want, d0, g0 = scan(a, hops8)
        got, d1, g1 = scan(b, hops16)
        assert d0 == d1 == frames
        assert same(got, want, g1, g0, "scan of %d hops" % H)
        for h in range(H):
            single, n, _ = device_run(b, hops16[h])
            assert n == frames[h]
            assert max_rel(got[h], single) < ADDITIVITY       # (the scan kernel partitions frames differently)


# ---- 8. the CLI --------------------------------------------------------------------------------------------------------------

def test_cli_replays_cs16(tmp_path):
    N, R = 4096, 64
    u = clamped_cu8(81, R * N)
    (tmp_path / "f.cu8").write_bytes(u.tobytes())
    (tmp_path / "f.cs16").write_bytes(synth.to_cs16(synth.to_cs8(u)).tobytes())

    def run(*extra):
        r = subprocess.run([CLI, "-b", str(N), "-n", str(R), "-q"] + list(extra), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return [l for l in r.stdout.split("\n") if l.strip() and not l.startswith("#")]

    a = run("--input", str(tmp_path / "f.cu8"))
    b = run("--input", str(tmp_path / "f.cs16"), "--format", "cs16")
    assert len(a) == len(b) == N
    if a != b:      # another geometry: every printed value within its last printed digit
        for la, lb in zip(a, b):
            fa, fb = la.split(), lb.split()
            assert fa[0] == fb[0]
            digits = len(fa[1].split(".")[1]) if "." in fa[1] else 0
            assert abs(round((float(fa[1]) - float(fb[1])) * 10 ** digits)) <= 1
