"""Short-time Fourier transform (include/rpf_engine.h, rpf_stft_device): the float64 answer, the reference for tests
and users.  Nothing here touches a device."""
import numpy as np

from . import _lib, pfb
from .datastore import frames_in


def reference(stream, N, fmt="cu8", step=None, window=None, taps=1, coeffs=None):
    """Row f = the transform of frame f as the engine defines it, complex128, shape (F, N): the samples converted
    exactly (cu8: v - 127; cs8, cs16, cf32: v), multiplied by the float32 product window[n] * (-1)^n rounded once as the
    engine rounds it (the samples are integers or float32, so the product with them is then formed in double), forward
    and unnormalised, so that bin N/2 is DC.  step: the frame step in samples (None = N).  coeffs (taps x N, with taps
    >= 1): the PFB form, the transform of the folded frames of pfb.fold -- no window, step N."""
    sgn = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    if coeffs is not None:
        z = pfb.fold(stream, N, taps, coeffs, fmt)
        return np.fft.fft(z * sgn, axis=1)
    step = N if step is None else step
    x = pfb.sample_values(stream, fmt)
    b = _lib.SAMPLE_BYTES[fmt]
    F = frames_in(x.size * b, N, step, b)
    if F <= 0:
        return np.zeros((0, N), dtype=np.complex128)
    v = x[np.arange(F)[:, None] * step + np.arange(N)[None, :]]
    if window is None:
        return np.fft.fft(v * sgn, axis=1)
    # one float32 rounding per component, as the kernels apply the window (every sample value is a float32 exactly)
    w32 = np.asarray(window, dtype=np.float32) * sgn.astype(np.float32)
    frames = (v.real.astype(np.float32) * w32).astype(np.float64) + 1j * (v.imag.astype(np.float32) * w32).astype(np.float64)
    return np.fft.fft(frames, axis=1)
