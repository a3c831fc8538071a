"""The bar of the correlator's accuracy test (tests/test_gpu_correlate.py: rpf_correlate_device against correlate.reference,
the numpy complex128 visibilities of the same streams, 80 frames), with the record that justifies it.

The figure judged is  err = max over i <= j and bins k of |V^_ij[k] - V_ij[k]| / max(m_ij[k], median_k m_ij),
m_ij = (V_ii + V_jj) / 2 of the float64 truth: the error of a sum of products of float32 spectra scales with the two
powers, not with |V_ij|.

The bar is not a number picked for the GPU: it is twice err of the CPU float32 path on the same streams --
rpf_oracle_fft_f32 over each stream's prepared frames (stft_bars.prepared_frames; for PFB the emulator's folded frames),
then the definition's terms and their sums in float64 -- the project's margin for two float32 implementations of one
calculation.  CPU_F32 holds those CPU figures; tests/test_correlate.py recomputes them without a GPU and fails if the
record drifts by more than 2 %.  MEASURED holds what the MI355X gave."""
import numpy as np

from rtl_power_fftw_amd import correlate, synth
import stft_bars

ACCURACY_FRAMES = 80
PFB_TAPS = stft_bars.PFB_TAPS
# (format, N, form, M): form "rect" or "hann" (16384: the catch-all twin), or "pfb" (PFB_TAPS taps of the default prototype)
ACCURACY_CASES = [("cu8", 64, "rect", 4), ("cu8", 512, "rect", 4), ("cu8", 4096, "rect", 4), ("cu8", 4096, "hann", 4),
                  ("cf32", 512, "rect", 4), ("cf32", 4096, "rect", 4), ("cu8", 16384, "rect", 4), ("cu8", 512, "pfb", 4),
                  ("cu8", 512, "rect", 8)]


def accuracy_streams(fmt, N, form, M):
    """M streams as bytes, ACCURACY_FRAMES frames each (PFB: of the frames they fold): stream m is half a common stream and
    half an independent one of the same kind, rounded to the format (cross_bars.accuracy_streams for M streams) -- mean
    coherence about 0.25 for every pair, so neither the coherent nor the incoherent part of V_ij dominates."""
    samples = (ACCURACY_FRAMES + (PFB_TAPS - 1 if form == "pfb" else 0)) * N
    if fmt == "cu8":
        c = synth.uniform_iq(700 + N, samples).astype(np.float64) - 127.0
        out = []
        for m in range(M):
            n = synth.uniform_iq(800 + 31 * m + N, samples).astype(np.float64) - 127.0
            out.append(np.clip(np.rint(0.5 * c + 0.5 * n) + 127.0, 0, 255).astype(np.uint8))
        return out
    c = synth.gaussian_cf32(700 + N, samples).astype(np.complex128)
    return [np.ascontiguousarray((0.5 * c + 0.5 * synth.gaussian_cf32(800 + 31 * m + N, samples).astype(np.complex128))
                                 .astype(np.complex64)).view(np.uint8) for m in range(M)]


def case_arguments(fmt, N, form, M):
    """(window, taps, coeffs) of a case, as correlate.reference and the engines take them."""
    return stft_bars.case_arguments(fmt, N, form)


def truth(streams, fmt, N, form, M):
    window, taps, coeffs = case_arguments(fmt, N, form, M)
    return correlate.reference(streams, N, fmt, window=window, taps=taps, coeffs=coeffs)


def err(got, want):
    """The figure of the module docstring; got and want (M, M, N) complex."""
    got = np.asarray(got, dtype=np.complex128)
    M = want.shape[0]
    worst = 0.0
    for i in range(M):
        for j in range(i, M):
            m = 0.5 * (want[i, i].real + want[j, j].real)
            worst = max(worst, float(np.max(np.abs(got[i, j] - want[i, j]) / np.maximum(m, np.median(m)))))
    return worst


def terms_sum(rows):
    """V from (M, F, N) complex rows by the definition: per frame the terms ar br + ai bi and ai br - ar bi of float64
    copies, then their sum over the frames in float64 (the lower triangle the conjugate of the upper)."""
    X = np.asarray(rows)
    ar, ai = X.real.astype(np.float64), X.imag.astype(np.float64)
    M, N = X.shape[0], X.shape[2]
    V = np.zeros((M, M, N), dtype=np.complex128)
    for i in range(M):
        for j in range(i, M):
            re = (ar[i] * ar[j] + ai[i] * ai[j]).sum(axis=0)
            im = (ai[i] * ar[j] - ar[i] * ai[j]).sum(axis=0)
            V[i, j].real, V[i, j].imag = re, im
            V[j, i].real, V[j, i].imag = re, -im
    return V


def cpu_f32(streams, fmt, N, form, M):
    """The CPU float32 path of the module docstring: (M, M, N) complex128."""
    from test_pfb import emul_fold
    window, taps, coeffs = case_arguments(fmt, N, form, M)
    rows = []
    for s in streams:
        folded = emul_fold(s, ACCURACY_FRAMES, N, taps, fmt, coeffs) if form == "pfb" else None
        rows.append(stft_bars.cpu_f32_rows(stft_bars.prepared_frames(s, fmt, N, window=window, folded=folded)))
    return terms_sum(np.stack(rows))


# (format, N, form, M) -> err of the CPU float32 path against float64
CPU_F32 = {("cu8", 64, "rect", 4): 1.081e-07, ("cu8", 512, "rect", 4): 1.167e-07, ("cu8", 4096, "rect", 4): 1.514e-07,
           ("cu8", 4096, "hann", 4): 1.523e-07, ("cf32", 512, "rect", 4): 1.244e-07, ("cf32", 4096, "rect", 4): 2.267e-07,
           ("cu8", 16384, "rect", 4): 1.631e-07, ("cu8", 512, "pfb", 4): 1.237e-07, ("cu8", 512, "rect", 8): 1.282e-07}

BAR = {case: 2.0 * e for case, e in CPU_F32.items()}

# (format, N, form, M) -> err of rpf_correlate_device against float64 measured by tests/test_gpu_correlate.py
MEASURED = {("cu8", 64, "rect", 4): 7.57e-08, ("cu8", 512, "rect", 4): 1.06e-07, ("cu8", 4096, "rect", 4): 1.85e-07,
            ("cu8", 4096, "hann", 4): 1.90e-07, ("cf32", 512, "rect", 4): 1.29e-07, ("cf32", 4096, "rect", 4): 2.92e-07,
            ("cu8", 16384, "rect", 4): 1.65e-07, ("cu8", 512, "pfb", 4): 1.26e-07, ("cu8", 512, "rect", 8): 1.23e-07}

# the known answers of test_gpu_correlate.py (cu8, N = 512, 80 frames, judged at BAR[("cu8", 512, "rect", 4)] = 2.33e-7):
# stream 1 = every frame of stream 0 shifted by 3 samples: |coherence - 1| 2.4e-14, phase within 3.0e-8 rad; M = 2 against
# accumulate_device_cross 1.22e-7 (bar 4.79e-7, the sum of the two bars)
MEASURED_KNOWN = {"shift_coherence": 2.39e-14, "shift_phase": 3.02e-08, "vs_cross": 1.22e-07}
