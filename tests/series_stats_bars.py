"""Thresholds of the time-resolved statistics tests (test_gpu_series_stats.py).  Everything stats_bars.py and
parity_bars.py already record is imported from there; what is new is recorded here with its reason."""
from stats_bars import ADDITIVITY, SAME_KERNELS, SK_BURST_ABOVE  # noqa: F401

# The time-resolved detection test (test_gpu_series_stats.py: N = 512, rows of M = 64 frames, noise + a carrier in every
# eighth frame of two rows), limits asserted FIRST on the float64 truth of the same stream and then on the GPU's rows.
# A carrier far above the noise in a fraction f of a row's frames gives SK ~ (M+1)/(M-1) (1/f - 1) = 7.2 at f = 1/8
# (truth: 7.05 and 7.06), above SK_BURST_ABOVE.  For Gaussian noise SK has mean 1 and variance
# 4 M^2 / ((M-1)(M+2)(M+3)) = 0.2425^2 at M = 64, is bounded below by 0 and skewed to the right (skewness ~ 10/sqrt(M)):
# the range is mean - 2.9 sd ... mean + 6.2 sd.  Recorded on the truth: the 22 judged values (the burst bin in the rows
# without a burst) lie in 0.644 ... 1.352; all 12240 noise (row, bin) pairs of the stream in 0.448 ... 3.70 with sd
# 0.244, three of them above 2.5 -- the range is for the judged bin, not a bound for every bin of a spectrogram.
SK_NOISE_RANGE_M64 = (0.3, 2.5)
