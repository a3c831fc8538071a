"""The bars of the cf32 statistics tests (tests/test_gpu_cf32_stats.py) and the record of what the MI355X measured.

Nothing here is new but one name: S1 is judged at cf32_bars.CF32_VS_TRUTH, S2 and PK at stats_bars.STATS_TIMES_CPU_ERR
times the CPU float32 path's own error on the same frames, SK at its first-order bound with stats_bars.SK_SLACK, sums
grouped differently at parity_bars.ADDITIVITY."""
from stats_bars import EMUL_VS_ORACLE_FRAME

# The NaN test compares PK of the K1 route with PK of the catch-all route on noise: PK is the power of one frame, and
# the two routes are two float32 transforms with different plans.  That is the situation stats_bars.EMUL_VS_ORACLE_FRAME
# was written down for -- a bin's power of one frame differs by at most a few 1e-7 of the larger of itself and the
# frame's typical bin (helpers.max_err_over_mean's metric) -- so the bar is that one.  (If the two routes pick different
# frames as a bin's loudest, the two maxima still differ by no more than one frame's error.)  On frames that every
# transform computes exactly the test asserts np.array_equal instead.
NAN_ROUTES_PK = EMUL_VS_ORACLE_FRAME

# (N, windowed) -> worst-bin relative errors against float64 truth measured by
# test_gaussian_cf32_statistics_against_truth: (S1, S2, PK) of the GPU, (S1, S2, PK) of the CPU float32 path on the same
# frames, and the spectral kurtosis error over its bound.  On the noise stream of the NaN test the two routes' PK differed
# by 4.2e-7 (rectangular) and 4.6e-7 (Hann) in max_err_over_mean's metric.
MEASURED = {
    (64, False): {"gpu": (7.92e-08, 1.97e-07, 2.77e-07), "cpu_f32": (9.91e-08, 2.8e-07, 2.94e-07), "sk_err_over_bound": 0.222},
    (512, False): {"gpu": (1.19e-07, 2.85e-07, 3.15e-07), "cpu_f32": (1.16e-07, 2.73e-07, 3.5e-07), "sk_err_over_bound": 0.158},
    (1024, True): {"gpu": (1.52e-07, 3.17e-07, 3.62e-07), "cpu_f32": (1.54e-07, 3.34e-07, 3.87e-07), "sk_err_over_bound": 0.243},
    (4096, True): {"gpu": (1.75e-07, 4.52e-07, 5.09e-07), "cpu_f32": (1.47e-07, 3.42e-07, 4.72e-07), "sk_err_over_bound": 0.262},
    (8192, False): {"gpu": (2.26e-07, 5.11e-07, 7.42e-07), "cpu_f32": (2.24e-07, 6.77e-07, 7.4e-07), "sk_err_over_bound": 0.225},
}
