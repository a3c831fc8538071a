"""frame_truth.py (the float64 reference test_gpu_k1_forms.py judges against) says what the project's earlier statements
of the same reference say, bit for bit: test_gpu_spectral_stats.truth_frame_powers / planes on cu8,
test_gpu_sample_formats.truth_signed on cs16, test_gpu_cf32.truth_cf32 on cf32; helpers.truth_f64 adds the same doubles
frame by frame where they add them in a tree, so that one is compared at ADDITIVITY.  Overlapped frames are the
materialised stream's frames.  No GPU: the modules are imported for their CPU functions only."""
import numpy as np
import pytest

from rtl_power_fftw_amd import synth
from frame_truth import planes, row_planes, truth_frame_powers, unpacked
from helpers import max_rel, truth_f64
from parity_bars import ADDITIVITY
from test_frame_overlap import materialise

pytest.importorskip("torch")
import test_gpu_cf32                                  # noqa: E402
import test_gpu_sample_formats                        # noqa: E402
import test_gpu_spectral_stats                        # noqa: E402


@pytest.mark.parametrize("N,window", [(64, False), (128, True), (4096, True)])
def test_cu8_is_the_statistics_tests_reference(N, window):
    frames = 9
    u = synth.noise_tones_iq(3, frames * N)
    w = synth.hann_window(N) if window else None
    p = truth_frame_powers(N, unpacked("cu8", u), frames, w)
    old = test_gpu_spectral_stats.truth_frame_powers(N, u, frames, w)
    assert np.array_equal(p, old)
    assert np.array_equal(planes(p), test_gpu_spectral_stats.planes(old))
    assert max_rel(p.sum(axis=0), truth_f64(N, u, frames, w)) < ADDITIVITY
    rows = row_planes(p, 4, 2)
    assert rows.shape == (2, 3, N)
    assert np.array_equal(rows[1], planes(p[4:8]))


def test_signed_and_float_formats_and_overlap():
    N, frames = 256, 7
    w = synth.hann_window(N)
    s16 = synth.noise_tones_cs16(5, frames * N)
    got = truth_frame_powers(N, unpacked("cs16", s16), frames, w).sum(axis=0)
    assert np.array_equal(got, test_gpu_sample_formats.truth_signed(N, synth.cs16_values(s16), frames, w))
    z = synth.gaussian_cf32(7, frames * N)
    got = truth_frame_powers(N, unpacked("cf32", z), frames, w).sum(axis=0)
    assert np.array_equal(got, test_gpu_cf32.truth_cf32(N, z, frames, w))
    u = np.minimum(synth.noise_tones_iq(9, frames * N), 254).astype(np.uint8)
    assert np.array_equal(unpacked("cs8", synth.to_cs8(u)), unpacked("cu8", u))
    step = N // 2 + 1
    X = synth.noise_tones_iq(11, N + step * (frames - 1))
    assert np.array_equal(truth_frame_powers(N, unpacked("cu8", X), frames, w, step=step),
                          truth_frame_powers(N, unpacked("cu8", materialise(X, N, step)), frames, w))
