"""The bar of the PFB accuracy test (tests/test_gpu_pfb.py: the PFB engine against pfb.fold and a numpy complex128
transform, per bin over 80 frames, helpers.max_err_over_mean), with the record that justifies it.

The bar is not a number picked for the GPU: it is twice the worst-bin error of the CPU float32 path on the same frames
-- the emulator's fold (tests/emul/pfb_emul.cpp) into the oracle's float32 transform, |X|^2 summed in double -- the
margin the statistics tests use and for the same reason: two float32 implementations of one calculation differ by a
factor of that order in the error of their worst bin.  CPU_F32 holds those CPU figures; tests/test_pfb.py recomputes
them without a GPU and fails if the record drifts.  MEASURED holds what the MI355X gave."""
from rtl_power_fftw_amd import synth

ACCURACY_TAPS = 4
ACCURACY_FRAMES = 80
ACCURACY_CASES = [("cu8", 64), ("cu8", 512), ("cu8", 4096), ("cf32", 64), ("cf32", 512), ("cf32", 4096)]


def accuracy_stream(fmt, N):
    """Uniform cu8 bytes or Gaussian cf32 with full mantissas, as bytes: ACCURACY_FRAMES frames of ACCURACY_TAPS taps."""
    samples = (ACCURACY_FRAMES + ACCURACY_TAPS - 1) * N
    if fmt == "cu8":
        return synth.uniform_iq(300 + N, samples)
    return synth.gaussian_cf32(300 + N, samples).view("uint8")


# (format, N) -> worst-bin error of the CPU float32 path against float64
CPU_F32 = {("cu8", 64): 1.07e-7, ("cu8", 512): 1.25e-7, ("cu8", 4096): 1.36e-7,
           ("cf32", 64): 1.02e-7, ("cf32", 512): 1.14e-7, ("cf32", 4096): 1.60e-7}

BAR = {case: 2.0 * err for case, err in CPU_F32.items()}

# (format, N) -> worst-bin error of the PFB engine against float64 measured by test_accuracy_against_float64
MEASURED = {("cu8", 64): 6.66e-8, ("cu8", 512): 1.13e-7, ("cu8", 4096): 1.82e-7,
            ("cf32", 64): 7.77e-8, ("cf32", 512): 1.05e-7, ("cf32", 4096): 1.95e-7}

# test_leakage_on_the_device (cu8 tone of amplitude 100 at bin N/4 + 0.5, N = 512, T = 4, 40 frames): p[k+3]/p[k] is
# 0.0401 on the plain engine and 6.83e-7 through the filter bank, 1.7e-5 of it (the test asks for less than 1e-3)
MEASURED_LEAKAGE = {"plain": 0.0401, "pfb": 6.83e-7}
