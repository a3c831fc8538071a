"""Per-bin statistics derived from what a stats engine (RPF_FLAG_BIN_STATS) accumulates."""
import numpy as np


def spectral_kurtosis(S1, S2, M):
    """The spectral kurtosis estimator of Nita & Gary from S1 = sum of the frame powers, S2 = sum of their squares
    over M frames:  SK = (M+1)/(M-1) * (M * S2 / S1^2 - 1), evaluated in double in exactly this order (the C++ host,
    host/datastore.h, does the same operations).  1 for Gaussian noise (standard deviation about 2/sqrt(M)), towards 0
    for a steady carrier, above 1 for anything intermittent.  NaN where it is undefined: M < 2, or S1 == 0."""
    S1 = np.asarray(S1, dtype=np.float64)
    S2 = np.asarray(S2, dtype=np.float64)
    out = np.full(np.broadcast(S1, S2).shape, np.nan)
    M = int(M)
    if M < 2:
        return out
    m = np.float64(M)
    ok = np.broadcast_to(S1 != 0.0, out.shape)
    s1 = np.broadcast_to(S1, out.shape)[ok]
    s2 = np.broadcast_to(S2, out.shape)[ok]
    out[ok] = ((m + 1.0) / (m - 1.0)) * (m * s2 / (s1 * s1) - 1.0)
    return out
