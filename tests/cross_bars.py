"""The bar of the cross-spectrum accuracy test (tests/test_gpu_cross.py: accumulate_device_cross against a numpy
complex128 cross-spectrum of the same two streams, 80 frames), with the record that justifies it.

The figure judged is  err = max_k |S^ab[k] - Sab[k]| / max(m[k], median m),  m = (Saa + Sbb) / 2  from the truth: the
error of the identity's Sab scales with Saa + Sbb, not with |Sab| (include/rpf_engine.h).

The bar is not a number picked for the GPU: it is twice err of the CPU float32 path on the same streams -- the oracle's
float32 transform over a, b and the emulator's u and v (tests/emul/cross_emul.cpp), |X|^2 summed in double, the
emulator's finishing expression -- the project's margin for two float32 implementations of one calculation.  CPU_F32
holds those CPU figures; tests/test_cross.py recomputes them without a GPU and fails if the record drifts by more than
2 %.  MEASURED holds what the MI355X gave."""
import numpy as np

from rtl_power_fftw_amd import synth

ACCURACY_FRAMES = 80
# (format, N, Hann window?)
ACCURACY_CASES = [("cu8", 64, False), ("cu8", 512, False), ("cu8", 4096, False), ("cu8", 4096, True),
                  ("cf32", 64, False), ("cf32", 512, False), ("cf32", 4096, False), ("cf32", 4096, True)]


def accuracy_streams(fmt, N):
    """(a, b) as bytes, ACCURACY_FRAMES frames each: a uniform cu8 bytes or Gaussian cf32 with full mantissas, b half a
    and half an independent stream of the same kind, rounded to the format -- mean coherence about 0.5, so neither the
    coherent nor the incoherent part of Sab dominates."""
    samples = ACCURACY_FRAMES * N
    if fmt == "cu8":
        a, n = synth.uniform_iq(400 + N, samples), synth.uniform_iq(500 + N, samples)
        mix = 0.5 * (a.astype(np.float64) - 127.0) + 0.5 * (n.astype(np.float64) - 127.0)
        return a, np.clip(np.rint(mix) + 127.0, 0, 255).astype(np.uint8)
    a, n = synth.gaussian_cf32(400 + N, samples), synth.gaussian_cf32(500 + N, samples)
    b = (0.5 * a.astype(np.complex128) + 0.5 * n.astype(np.complex128)).astype(np.complex64)
    return a.view(np.uint8), np.ascontiguousarray(b).view(np.uint8)


# (format, N, window) -> err of the CPU float32 path against float64
CPU_F32 = {("cu8", 64, False): 8.134e-8, ("cu8", 512, False): 1.229e-7, ("cu8", 4096, False): 2.074e-7,
           ("cu8", 4096, True): 1.848e-7,
           ("cf32", 64, False): 9.375e-8, ("cf32", 512, False): 1.422e-7, ("cf32", 4096, False): 2.176e-7,
           ("cf32", 4096, True): 3.621e-7}

BAR = {case: 2.0 * err for case, err in CPU_F32.items()}

# (format, N, window) -> err of accumulate_device_cross against float64 measured by test_accuracy_against_float64
MEASURED = {("cu8", 64, False): 8.18e-8, ("cu8", 512, False): 1.52e-7, ("cu8", 4096, False): 2.03e-7,
            ("cu8", 4096, True): 1.84e-7,
            ("cf32", 64, False): 9.60e-8, ("cf32", 512, False): 1.32e-7, ("cf32", 4096, False): 2.18e-7,
            ("cf32", 4096, True): 2.64e-7}

# the known answers of test_gpu_cross.py (cu8, N = 512, 80 frames, judged at BAR[("cu8", 512, False)] = 2.46e-7):
# b = a: Re Sab == Saa bit for bit, |coherence - 1| 5e-15, largest Im Sab / Saa 7.4e-8; b = i a: Im Sab == -Saa bit for
# bit, Re Sab 6.1e-8; b = every frame of a shifted by 3 samples: |coherence - 1| 1.9e-7, phase within 8.2e-8 rad
MEASURED_KNOWN = {"self_im": 7.36e-8, "times_i_re": 6.12e-8, "shift_coherence": 1.85e-7, "shift_phase": 8.18e-8}
