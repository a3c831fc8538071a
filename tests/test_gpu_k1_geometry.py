"""K1's launch geometry on the MI355X: every size x {cu8, cs8, cs16} x {plain, windowed} x entry kind launches with the
grid, workgroup size, frames per workgroup and dynamic LDS recorded in tests/golden/k1_launch_geometry.json
(tests/golden/make_k1_launch_geometry.py wrote it from the build before the size table became one table).  The
kernels index LDS by compile-time geometry and the host sizes it from the size table: the two have to stay the same
numbers, the statistics kernels' lower occupancies and cs16's doubled ring included.  Exact equality; no spectrum is
looked at (the parity tests do that).

Entry kinds: `single` rpf_accumulate_device; `stats` the same on an engine with RPF_FLAG_BIN_STATS; `overlapped` the
same at frame step N/2 (the strided kernel); `series` rpf_accumulate_device_series with L = 4.  Every stream holds
2 x recorded grid x frames_per_wg frames, so the launched grid is the planned resident grid and not ceil(frames / fpw):
a changed occupancy shows.  `grid` is compared on a device with the fixture's CU count only; the other three always."""
import json
import os

import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import synth
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")

FIXTURE = os.path.join(GOLDEN, "k1_launch_geometry.json")
SIZES = [64, 128, 256, 512, 1024, 2048, 4096, 8192]
FORMATS = ["cu8", "cs8", "cs16"]
KINDS = ["single", "stats", "overlapped", "series"]
SERIES_L = 4
FIELDS = ("grid", "block", "frames_per_wg", "lds_bytes")


def key(N, fmt, window, kind):
    return "n%d_%s_%s_%s" % (N, fmt, "hann" if window else "rect", kind)


def engine_for(kind, N, fmt, window):
    """The engine an entry kind runs on; `single` and `series` share one (engine_key says which)."""
    w = synth.hann_window(N) if window else None
    step = N // 2 if kind == "overlapped" else None
    return rpf.Datastore(rpf.Params(N=N, window=window, frame_step=step, sample_format=fmt, bin_stats=(kind == "stats")), w)


def engine_key(kind):
    return "plain" if kind in ("single", "series") else kind


def launch(ds, kind, frames):
    """launch_info() after one launch of `kind` over `frames` frames of constant bytes."""
    N = ds.params.N
    nbytes = ds.frame_span(frames)
    stream = torch.full((nbytes,), 127, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    if kind == "series":
        K = frames // SERIES_L
        out = torch.empty((K, N), dtype=torch.float64, device=DEV)
        assert ds.accumulate_device_series(stream.data_ptr(), nbytes, SERIES_L, K, out.data_ptr(), s) == K
        assert ds.series_launches() == 1
    else:
        out = torch.empty(N, dtype=torch.float64, device=DEV)
        assert ds.accumulate_device(stream.data_ptr(), nbytes, frames, out.data_ptr(), s) == frames
    torch.cuda.synchronize()
    return ds.launch_info()


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("window", [False, True], ids=["rect", "hann"])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("N", SIZES)
def test_launch_geometry_is_the_recorded_one(recorded, N, fmt, window):
    same_cus = torch.cuda.get_device_properties(0).multi_processor_count == recorded["cu_count"]
    compared = FIELDS if same_cus else FIELDS[1:]
    engines, wrong = {}, []
    try:
        for kind in KINDS:
            want = recorded["records"][key(N, fmt, window, kind)]
            if engine_key(kind) not in engines:
                engines[engine_key(kind)] = engine_for(kind, N, fmt, window)
            got = launch(engines[engine_key(kind)], kind, 2 * want["grid"] * want["frames_per_wg"])
            print("%s: %s%s" % (key(N, fmt, window, kind), got, "" if same_cus else " (another CU count: grid not compared)"))
            if any(got[f] != want[f] for f in compared):
                wrong.append((kind, got, want))
    finally:
        for ds in engines.values():
            ds.close()
    assert not wrong, wrong
