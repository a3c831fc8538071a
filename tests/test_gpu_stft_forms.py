"""The phase of the STFT rows on the MI355X at every store kernel, size, format and route (stft_forms_bars.py has the
cases, the bars and the record).  The identity of tests/test_gpu_stft.py -- re^2 + im^2 of a row is the frame's power
-- cannot see a conjugated, swapped, negated or linearly phased spectrum; a comparison with float64 can.

(a) K1's 64 plain kernels with LDS-DMA staging (8 sizes x rect / Hann x cu8 / cs8 / cs16 / cf32) against the numpy
    complex128 transform of the prepared frames, 16 rows from the first iteration, the second, the first ring-fed one
    and the ragged tail; the power identity on the same rows and on the sum of all rows.
(b) The other 192 store kernels by bit equality with (a)'s rows over every row, compared on the device: VGPR staging
    (FLAG_NO_LDS_DMA, and a stream one sample off alignment), the strided kernel at steps N/2 + 1 and N/2 against the
    plain kernel on the materialised frames, and the ties between the formats.
(c) The catch-all route from 2 to 2^22 bins, odd and even log2 N, every value generic_batch takes, against float64.

Out of scope: N above 2^22 (at 2^23 and up a single case costs more than 10 s of host transforms, and the power path
already runs 2^25 through the same batch loop); Bluestein sizes, refused by definition; PFB and the host entry, which
tests/test_gpu_stft.py covers; any timing.  Each test prints the figures it judged."""
import numpy as np
import pytest

from rtl_power_fftw_amd import _lib, synth
import stft_forms_bars as bars
from test_gpu_stft import check_identity, cuda_stream, engine, materialised, resident_grid, stft_rows

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")
NO_DMA = _lib.FLAG_NO_LDS_DMA
_resident = {}


def case_id(case):
    return "%s-%d-%s" % case


def on_device(key, make):
    """A byte stream in HBM, uploaded once per module, with slack behind it."""
    if key not in _resident:
        host = np.ascontiguousarray(make()).reshape(-1).view(np.uint8)
        t = torch.zeros(host.size + 64, dtype=torch.uint8, device=DEV)
        t[:host.size].copy_(torch.from_numpy(host))
        _resident[key] = (host, t)
    return _resident[key]


def k1_resident(fmt):
    return on_device(fmt, lambda: bars.k1_stream(fmt))


def device_rows(ds, d_bytes, nbytes, misalign=0):
    """(F x N x 2 float32 rows in HBM, F) of the first nbytes of the device tensor d_bytes, optionally moved off alignment."""
    assert 0 < nbytes <= d_bytes.numel() - 64         # (every stream here has 64 bytes of slack behind it, as to_device's)
    if misalign:
        moved = torch.zeros(nbytes + 128, dtype=torch.uint8, device=DEV)
        moved[misalign:misalign + nbytes].copy_(d_bytes[:nbytes])
        d_bytes = moved[misalign:]
    F = ds.frames_in(nbytes)
    out = torch.full((F, ds.params.N, 2), -12345.5, dtype=torch.float32, device=DEV)
    n = ds.stft_device(d_bytes.data_ptr(), nbytes, 1 << 40, out.data_ptr(), cuda_stream())
    torch.cuda.synchronize()
    assert n == F
    return out, F


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def as_complex(rows):
    return rows.cpu().numpy().view(np.complex64)[..., 0]


def planned(ds, case):
    """(grid, fpw, F) of a K1 engine; the plain cases must plan the grid the CPU figures were computed for."""
    li = resident_grid(ds)
    assert li["lds_bytes"] > 0 and li["block"] >= 256
    return li["grid"], li["frames_per_wg"], bars.k1_frames(case[0], case[1], li["grid"], li["frames_per_wg"])


def route_of(ds, d_ptr, flags=0):
    """The staging route transform_stft_k1 takes: LDS-DMA where the engine allows it and pointer and pitch are multiples of 16."""
    pitch = ds.sample_bytes * ds.params.frame_step
    return "LDS-DMA" if not (flags & NO_DMA) and d_ptr % 16 == 0 and pitch % 16 == 0 else "VGPR"


def judge(case, got, want, what, check=True):
    """The bars of stft_forms_bars on judged rows; returns the figures (check=False: the recorder, which asserts nothing)."""
    err, row, k = bars.worst(got, want)
    cpu = bars.CPU_F32[case]
    print("%s: err %.3e at judged row %d bin %d, CPU float32 path %.3e, ratio %s (bar 2), COARSE %.0e"
          % (what, err, row, k, cpu, "%.2f" % (err / cpu) if cpu else "-", bars.COARSE))
    assert err <= bars.COARSE or not check, (what, err)
    if check and case not in bars.RECORDED_NOT_ASSERTED:
        assert err <= bars.BAR[case], (what, err, bars.BAR[case])
    return {"err": err, "cpu_f32": cpu, "ratio": err / cpu if cpu else None, "worst_row": row, "worst_bin": k}


# ---- (a) the 64 plain LDS-DMA kernels against float64 -------------------------------------------------------------------

def k1_plain_figures(case, check=True):
    fmt, N, form = case
    host, dev = k1_resident(fmt)
    with engine(N, fmt, form == "hann") as ds:
        grid, fpw, F = planned(ds, case)
        assert (grid, fpw) == bars.GEOMETRY[case], "the device plans another grid than stft_forms_bars.GEOMETRY records"
        nbytes = ds.frame_span(F)
        assert route_of(ds, dev.data_ptr()) == "LDS-DMA"
        d_rows, n = device_rows(ds, dev, nbytes)
        assert n == F and ds.launch_info()["grid"] == grid
        sel = bars.k1_rows(fmt, N, grid, fpw)
        judged = bars.frames_of(host, fmt, N, sel)
        assert np.array_equal(judged, bars.k1_judged_frames(case))
        _, want = bars.references(judged, case)
        what = "N=%d %s %s grid %d x %d, %d frames" % (N, fmt, form, grid, fpw, F)
        fig = judge(case, as_complex(d_rows[sel]), want, what, check)
        check_identity(ds, host[:nbytes], as_complex(d_rows), sel, what)
    fig.update(grid=grid, fpw=fpw, frames=F, staging="LDS-DMA", judged_rows=sel)
    return fig


@pytest.mark.parametrize("case", bars.K1_CASES, ids=case_id)
def test_plain_kernel_rows_against_float64(case):
    """Measured on the MI355X: stft_forms_bars.MEASURED."""
    k1_plain_figures(case)


# ---- (b) the other 192 kernels, bit for bit -----------------------------------------------------------------------------

@pytest.mark.parametrize("case", bars.K1_CASES, ids=case_id)
def test_vgpr_staging_gives_the_lds_dma_rows(case):
    fmt, N, form = case
    host, dev = k1_resident(fmt)
    with engine(N, fmt, form == "hann") as ds:
        grid, fpw, F = planned(ds, case)
        nbytes = ds.frame_span(F)
        want, _ = device_rows(ds, dev, nbytes)
        off = _lib.SAMPLE_BYTES[fmt]
        shifted, _ = device_rows(ds, dev, nbytes, misalign=off)        # off alignment the DMA engine goes the VGPR route
        assert off % 16 and same_bits(shifted, want)
    with engine(N, fmt, form == "hann", flags=NO_DMA) as ds:
        plain, n = device_rows(ds, dev, nbytes)
        assert n == F and ds.launch_info()["grid"] == grid
        assert same_bits(plain, want)
        shifted, _ = device_rows(ds, dev, nbytes, misalign=off)
        assert same_bits(shifted, want)
    print("N=%d %s %s: %d rows, VGPR staging (flagged, and one sample off alignment) bit for bit the LDS-DMA rows" % (N, fmt, form, F))


@pytest.mark.parametrize("case", bars.K1_CASES, ids=case_id)
def test_strided_kernel_gives_the_plain_rows_of_the_materialised_frames(case):
    fmt, N, form = case
    b = _lib.SAMPLE_BYTES[fmt]
    host, dev = k1_resident(fmt)
    routes = []
    for S in (N // 2 + 1, N // 2):
        with engine(N, fmt, form == "hann", step=S) as ds:
            grid, fpw, F = planned(ds, case)
            nbytes = ds.frame_span(F)
            got, n = device_rows(ds, dev, nbytes)
            routes.append("S=%d %s (grid %d x %d, %d frames)" % (S, route_of(ds, dev.data_ptr()), grid, fpw, F))
            if (b * S) % 16 == 0:                  # the LDS-DMA kernel ran: the VGPR one of the same step gives its rows
                with engine(N, fmt, form == "hann", step=S, flags=NO_DMA) as nd:
                    vgpr, _ = device_rows(nd, dev, nbytes)
                assert same_bits(vgpr, got)
                routes[-1] += " and VGPR"
        # the frames side by side, gathered on the device (what `materialised` does on the host, checked on three frames)
        side = torch.zeros(F * b * N + 64, dtype=torch.uint8, device=DEV)
        side[:F * b * N].view(F, b * N).copy_(torch.as_strided(dev, (F, b * N), (b * S, 1)))
        assert np.array_equal(side[:3 * b * N].cpu().numpy(), materialised(host, fmt, N, S, 3))
        with engine(N, fmt, form == "hann") as ds:
            want, m = device_rows(ds, side, F * b * N)
        assert m == F == n and same_bits(got, want)
    print("N=%d %s %s strided, every row bit for bit the plain kernel's: %s" % (N, fmt, form, "; ".join(routes)))


FORM_CASES = [(N, form) for N in bars.K1_SIZES for form in bars.FORMS]


@pytest.mark.parametrize("N,form", FORM_CASES, ids=lambda v: str(v))
def test_formats_that_say_the_same_give_the_same_rows(N, form):
    """cs8 of to_cs8(stream) = cu8; cs16 of the 8-bit values = cs8; cf32 of the int16 values = cs16.  Rows are per frame,
    so the grids do not enter; every tie runs the larger of its two engines' frame counts."""
    def tie(a, b, samples):
        """Rows of engine format a[0] on stream a[1:] against those of b, over the larger frame count that `samples` holds."""
        F = min(max(bars.k1_frames(f, N, *bars.GEOMETRY[(f, N, form)]) for f in (a[0], b[0])), samples // N)
        out = []
        for fmt, key, make in (a, b):
            _, dev = on_device(key, make)
            with engine(N, fmt, form == "hann") as ds:
                rows, n = device_rows(ds, dev, ds.frame_span(F))
            assert n == F
            out.append(rows)
        assert same_bits(*out)
        return F

    cu8 = ("cu8", "cu8", lambda: bars.k1_stream("cu8"))
    cs8 = ("cs8", "cs8", lambda: bars.k1_stream("cs8"))
    cs16 = ("cs16", "cs16", lambda: bars.k1_stream("cs16"))
    cs16_of_cs8 = ("cs16", "cs16 of cs8", lambda: synth.to_cs16(bars.k1_stream("cs8")))
    cf32_of_cs16 = ("cf32", "cf32 of cs16", lambda: synth.to_cf32(bars.k1_stream("cs16")).view(np.uint8))
    F8 = tie(cs8, cu8, bars.k1_samples("cu8"))
    F16 = tie(cs16_of_cs8, cs8, bars.k1_samples("cu8"))
    F32 = tie(cf32_of_cs16, cs16, bars.k1_samples("cs16"))
    print("N=%d %s: cs8 = cu8 over %d rows, cs16 of 8-bit values = cs8 over %d, cf32 of int16 values = cs16 over %d"
          % (N, form, F8, F16, F32))


# ---- (c) the catch-all route against float64 ----------------------------------------------------------------------------

def catch_all_figures(case, check=True):
    fmt, N, form = case
    B, F, sel = bars.generic_batch(N), bars.catch_all_frames(N), bars.catch_all_rows(N)
    stream = bars.catch_all_stream(case)
    judged = bars.frames_of(stream, fmt, N, sel)
    assert np.array_equal(judged, bars.catch_all_judged_frames(case))
    _, want = bars.references(judged, case)
    what = "catch-all N=%d %s %s, %d frames in batches of %d" % (N, fmt, form, F, B)
    with engine(N, fmt, form == "hann") as ds:
        rows, n = stft_rows(ds, stream)
        assert n == F and ds.launch_info()["lds_bytes"] == 0
        fig = judge(case, rows[sel], want, what, check)
    # The power identity holds on the catch-all engine; where another family serves the size for power (cu8: the
    # Bluestein kernels below 64 bins, mixed radix and four-step from 32768 to 262144) the default engine gives the
    # rows of that twin, and everywhere the two engines' rows are the same bits.
    with engine(N, fmt, form == "hann", flags=_lib.FLAG_CATCH_ALL) as ds:
        twin, m = stft_rows(ds, stream)
        assert m == F and ds.launch_info()["lds_bytes"] == 0
        assert np.array_equal(twin.view(np.uint32), rows.view(np.uint32))
        check_identity(ds, stream, twin, sel, what)
    fig.update(frames=F, batch=B, staging="catch-all", judged_rows=sel)
    return fig


@pytest.mark.parametrize("case", bars.CATCH_ALL_CASES, ids=case_id)
def test_catch_all_rows_against_float64(case):
    """Measured on the MI355X: stft_forms_bars.MEASURED."""
    catch_all_figures(case)


def test_overlapped_rows_on_the_catch_all_route_at_an_odd_log():
    N, fmt = 32768, "cu8"
    S, F = N // 2 + 1, 70
    stream = synth.noise_tones_iq(2500, N + S * (F - 1))
    with engine(N, fmt, step=S) as ds:
        got, n = stft_rows(ds, stream)
    with engine(N, fmt, flags=_lib.FLAG_CATCH_ALL) as ds:
        want, m = stft_rows(ds, materialised(stream, fmt, N, S, F))
    assert n == m == F
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
