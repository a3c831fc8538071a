"""The bar of the cf32 accuracy test (tests/test_gpu_cf32.py, Gaussian float32 input with full mantissas against numpy
complex128), with the record that justifies it.

The bar is the one the integer-format tests use, parity_bars.VS_TRUTH: per bin, 80 frames, |gpu - truth| / truth.  The
input differs from theirs in that the samples carry 24 significant bits instead of 8 or 16, which costs nothing before
the transform: (-1)^n is exact and the window is one rounding for every format.  Measured on the MI355X (worst bin):
MEASURED below, 0.8 - 2.3e-7; all under the bar, so the fallback of the issue (twice the CPU float32 path's error on the same
frames) is not used."""
from parity_bars import VS_TRUTH

CF32_VS_TRUTH = VS_TRUTH

# (N, windowed) -> worst-bin error against float64 truth measured by test_gaussian_cf32_against_truth
MEASURED = {(64, False): 7.92e-8, (512, False): 1.19e-7, (4096, False): 1.97e-7, (4096, True): 1.75e-7, (8192, False): 2.26e-7}
