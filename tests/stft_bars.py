"""The bar of the STFT accuracy tests (tests/test_gpu_stft.py: the rows of rpf_stft_device against stft.reference, the
numpy complex128 transform of the same prepared frames, 16 frames), with the record that justifies it.

The figure judged is  err = max over rows f and bins k of |X^[f, k] - X[f, k]| / max(|X[f, k]|, median_k |X[f, k]|):
relative where a bin carries signal, against the row's median magnitude where it does not.

The bar is not a number picked for the GPU: it is twice err of the CPU float32 path on the same prepared frames --
rpf_oracle_fft_f32 over the frames as the kernels prepare them (the exactly converted samples times the float32 product
of (-1)^n and the window; for PFB the emulator's folded frames) -- the project's margin for two float32 implementations
of one calculation.  CPU_F32 holds those CPU figures; tests/test_stft.py recomputes them without a GPU and fails if the
record drifts by more than 2 %.  MEASURED holds what the MI355X gave."""
import ctypes

import numpy as np

from rtl_power_fftw_amd import pfb, stft, synth
from helpers import fp, oracle_lib

ACCURACY_FRAMES = 16
PFB_TAPS = 4
# (format, N, form): form "rect" or "hann" (native K1 sizes and the catch-all sizes 16384 and 65536), or "pfb" (N = 512,
# PFB_TAPS taps of the default prototype)
ACCURACY_CASES = [(fmt, N, form) for fmt in ("cu8", "cf32")
                  for N, form in ((64, "rect"), (512, "rect"), (4096, "rect"), (4096, "hann"), (8192, "rect"),
                                  (16384, "rect"), (65536, "rect"), (512, "pfb"))]


def accuracy_stream(fmt, N, form):
    """Bytes of ACCURACY_FRAMES frames (PFB: of the input frames they fold): synth's noise-and-tone stream, cu8 bytes or
    Gaussian cf32 with full mantissas."""
    samples = (ACCURACY_FRAMES + (PFB_TAPS - 1 if form == "pfb" else 0)) * N
    if fmt == "cu8":
        return synth.noise_tones_iq(600 + N, samples)
    return synth.gaussian_cf32(600 + N, samples).view(np.uint8)


def case_arguments(fmt, N, form):
    """(window, taps, coeffs) of a case, as stft.reference and the engines take them."""
    if form == "pfb":
        return None, PFB_TAPS, pfb.coefficients(N, PFB_TAPS)
    return (synth.hann_window(N) if form == "hann" else None), 1, None


def err(got, want):
    """The figure of the module docstring; got and want (F, N) complex."""
    mag = np.abs(want)
    floor = np.median(mag, axis=1, keepdims=True)
    return float(np.max(np.abs(np.asarray(got, dtype=np.complex128) - want) / np.maximum(mag, floor)))


def prepared_frames(stream, fmt, N, window=None, step=None, folded=None):
    """The frames as the kernels prepare them, (F, N, 2) float32: the exactly converted samples of frame f = samples
    [f S, f S + N) times the float32 product window[n] (-1)^n, one rounding per component.  folded: (F, N, 2) float32
    frames to take instead of the stream's (a PFB engine's folded frames: (-1)^n alone)."""
    sgn = (1 - 2 * (np.arange(N) % 2)).astype(np.float32)
    if folded is not None:
        return np.ascontiguousarray(np.asarray(folded, dtype=np.float32) * sgn[None, :, None])
    v = pfb.sample_values(stream, fmt)
    S = N if step is None else step
    F = 0 if v.size < N else (v.size - N) // S + 1
    x = v[np.arange(F)[:, None] * S + np.arange(N)[None, :]]
    x = np.stack([x.real, x.imag], axis=2).astype(np.float32)              # exact: every format's value is a float32
    w = sgn if window is None else np.asarray(window, dtype=np.float32) * sgn
    return np.ascontiguousarray(x * w[None, :, None])


def cpu_f32_rows(frames):
    """The CPU float32 path: rpf_oracle_fft_f32 over prepared frames, (F, N) complex64."""
    frames = np.ascontiguousarray(frames, dtype=np.float32)
    F, N = frames.shape[0], frames.shape[1]
    orc = oracle_lib()
    plan = orc.rpf_oracle_plan_create(N)
    out = np.zeros((F, N, 2), dtype=np.float32)
    for f in range(F):
        orc.rpf_oracle_fft_f32(plan, frames[f].ctypes.data_as(fp), out[f].ctypes.data_as(fp))
    orc.rpf_oracle_plan_destroy(plan)
    return out.view(np.complex64).reshape(F, N)


def f64_rows(frames):
    """The numpy complex128 transform of prepared frames."""
    frames = np.asarray(frames, dtype=np.float64)
    return np.fft.fft(frames[..., 0] + 1j * frames[..., 1], axis=1)


# (format, N, form) -> err of the CPU float32 path against complex128
CPU_F32 = {('cu8', 64, 'rect'): 2.209e-07, ('cu8', 512, 'rect'): 5.185e-07, ('cu8', 4096, 'rect'): 1.020e-06,
           ('cu8', 4096, 'hann'): 1.495e-06, ('cu8', 8192, 'rect'): 1.772e-06, ('cu8', 16384, 'rect'): 2.940e-06,
           ('cu8', 65536, 'rect'): 4.500e-06, ('cu8', 512, 'pfb'): 6.088e-07, ('cf32', 64, 'rect'): 2.882e-07,
           ('cf32', 512, 'rect'): 7.255e-07, ('cf32', 4096, 'rect'): 2.142e-06, ('cf32', 4096, 'hann'): 1.208e-06,
           ('cf32', 8192, 'rect'): 1.961e-06, ('cf32', 16384, 'rect'): 4.529e-06, ('cf32', 65536, 'rect'): 9.568e-06,
           ('cf32', 512, 'pfb'): 5.794e-07}

BAR = {case: 2.0 * e for case, e in CPU_F32.items()}

# (format, N, form) -> err of rpf_stft_device against stft.reference measured by tests/test_gpu_stft.py
MEASURED = {('cu8', 64, 'rect'): 2.256e-07, ('cu8', 512, 'rect'): 2.979e-07, ('cu8', 4096, 'rect'): 1.018e-06,
            ('cu8', 4096, 'hann'): 1.160e-06, ('cu8', 8192, 'rect'): 1.087e-06, ('cu8', 16384, 'rect'): 2.442e-06,
            ('cu8', 65536, 'rect'): 3.482e-06, ('cu8', 512, 'pfb'): 5.959e-07, ('cf32', 64, 'rect'): 3.262e-07,
            ('cf32', 512, 'rect'): 5.392e-07, ('cf32', 4096, 'rect'): 2.152e-06, ('cf32', 4096, 'hann'): 1.411e-06,
            ('cf32', 8192, 'rect'): 1.581e-06, ('cf32', 16384, 'rect'): 4.530e-06, ('cf32', 65536, 'rect'): 1.309e-05,
            ('cf32', 512, 'pfb'): 4.961e-07}
