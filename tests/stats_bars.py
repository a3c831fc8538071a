"""Thresholds of the per-bin statistics tests (test_spectral_stats.py, test_gpu_spectral_stats.py).  Everything that
parity_bars.py already records is imported from there; what is new is recorded here with its reason."""
from parity_bars import ADDITIVITY, PARITY, SAME_KERNELS, VS_TRUTH  # noqa: F401

# S2 and PK against float64 truth: no number of their own.  What is asserted per case is
#     err(gpu, truth) <= STATS_TIMES_CPU_ERR * err(cpu_f32, truth)
# with err the worst per-bin relative error of that statistic and cpu_f32 the CPU float32 path (rpf_oracle_fft_f32 on the
# exactly unpacked frame, p as the header defines it) evaluated in the same test on the same stream.  2 is the spread
# this project has recorded between two correct float32 transforms with different plans (parity_bars.py section 4: the
# oracle against pocketfft; K1's recorded S1 errors sit at 0.7 - 1.0 x the oracle's).
STATS_TIMES_CPU_ERR = 2.0

# |SK_gpu - SK_truth| <= (M+1)/(M-1) * (M S2/S1^2) * (d2 + 2 d1) * SK_SLACK per bin, with d1, d2 the relative errors
# of S1 and S2 measured for the case: first-order propagation through SK = (M+1)/(M-1) (M S2/S1^2 - 1); the 1 % covers
# the second-order terms (d ~ 1e-7).
SK_SLACK = 1.01

# The host emulator's p against the CPU float32 path's, frame by frame: two float32 transforms with different plans,
# each ~1e-7 x the frame's rms bin from the exact spectrum, so a bin's power differs by at most a few 1e-7 of the
# larger of itself and the frame's mean bin (helpers.max_err_over_mean's metric, FEW_FRAMES_FILLED_BINS' reasoning:
# weak bins of a single periodogram have no relative accuracy in any float32 transform).
EMUL_VS_ORACLE_FRAME = 3e-6

# The detection test (N = 4096, 1000 frames, noise + steady carrier + one-in-ten burst), limits asserted FIRST on the
# float64 truth and then on the CLI's columns.  From SK's distribution for Gaussian noise, 1 +- 2/sqrt(M) = 0.063 at
# M = 1000: [0.6, 1.4] is more than six sigma either way (recorded on the truth: 0.79 ... 1.27 over 4093 bins); a steady
# carrier 4e3 x the noise gives ~4e-4, a carrier in every tenth frame ~9.
SK_NOISE_RANGE = (0.6, 1.4)
SK_STEADY_BELOW = 0.05
SK_BURST_ABOVE = 4.0
PEAK_WITHIN_DB = 1.0          # burst bin's peak hold against the steady bin's (recorded 0.12 dB)
MEAN_LOWER_DB = (9.0, 11.0)   # ... while its mean is ~10 dB lower (recorded 10.0 dB)
