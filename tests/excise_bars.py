"""Thresholds of the excised-average tests (test_excise.py, test_gpu_excise.py).  Everything series_stats_bars.py,
stats_bars.py and parity_bars.py already record is imported from there; what is new is recorded here with its reason."""
from series_stats_bars import ADDITIVITY, SAME_KERNELS  # noqa: F401

# mask and kept have no bar: they are compared exactly (the kernels evaluate SK in the order of
# stats.spectral_kurtosis, every operation rounded on its own).  clean and total are sums of the same doubles as the
# reference's in another order: ADDITIVITY, relative to the bin's total (a bin with nothing kept has clean = 0).

# The detection test (test_gpu_excise.py: N = 512, 24 integrations of L = 64 frames, 8-bit Gaussian noise, sigma 20, and a
# carrier of amplitude 30 in every eighth frame of the integrations 7 and 16 at one bin; thresholds stats.sk_limits(64),
# 3 sigma = 0.2726 ... 1.7274).  Every limit is asserted FIRST on the float64 truth of the same stream, then on the GPU.
#
# The burst integrations have SK ~ (M+1)/(M-1) (1/f - 1) = 7.2 at f = 1/8 (truth: 7.0), far above the upper limit: both
# are flagged and kept at that bin is K - 2 (the seed is chosen so that none of the bin's 22 noise integrations is).
#
# The mean power of a bin over its kept integrations, relative to the median of the bins' clean means.  A noise bin's mean
# over ~1500 frames scatters by 1/sqrt(1500) = 2.6 %; over the 510 noise bins the largest excursion expected is about
# 3.3 sd.  The neighbours are the 16 bins either side of the burst bin; the bar is 4.6 sd of the scatter, for them and
# for the burst bin's own clean mean (truth: the neighbours within 0.044, the burst bin at +0.016).  Excision itself
# biases a clean mean down a little (the integrations it drops are the ones with large S2, which have large S1): well
# inside the bar.
NEIGHBOUR_SPREAD = 0.12          # |mean / median - 1| of the neighbours' clean means (truth: at most 0.044)
# Unexcised, the burst bin carries the carrier's power in 16 of its 1536 frames: 30^2 N / (2 sigma^2) = 576 x the noise
# in those frames, 16/1536 x 576 = 6.0 x the noise on average.  The truth shows +6.07; the bar is half of it.
TOTAL_EXCESS_ABOVE = 3.0         # total mean of the burst bin / median - 1 (truth: 6.07)

# Share of the noise (integration, bin) pairs flagged at 3 sigma.  SK for Gaussian noise is skewed to the right, so the
# upper tail beyond 3 sd holds more than a normal distribution's 0.13 %: the truth of this stream (seed chosen on the
# CPU) shows 1.08 %; the cap is the issue's.  Nothing here is a calibrated false-alarm rate.
NOISE_FLAGGED_SHARE_CAP = 0.02
