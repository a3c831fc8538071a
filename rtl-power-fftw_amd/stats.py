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


def sk_limits(M, sigma=3.0):
    """(lower, upper) = 1 -+ sigma * sqrt(4 M^2 / ((M-1)(M+2)(M+3))), the lower one not below 0: `sigma` standard
    deviations of SK about its mean for Gaussian noise and M independent frames (Nita & Gary's variance).  SK is bounded
    below by 0 and skewed to the right (skewness about 10/sqrt(M)), so at 3 sigma a fraction of a per cent of clean data
    lies above the upper limit: thresholds to start from, not a calibrated false-alarm rate.  Overlapped frames
    (frame step < N) are not independent.  The C++ host's sk_limits (host/datastore.h) does the same operations."""
    M = int(M)
    if M < 2:
        raise ValueError("sk_limits: M must be at least 2, got %d" % M)
    m = np.float64(M)
    sd = np.sqrt(4.0 * m * m / ((m - 1.0) * (m + 2.0) * (m + 3.0)))
    d = np.float64(sigma) * sd
    return float(max(1.0 - d, 0.0)), float(1.0 + d)


def excise(rows, L, sk_lo, sk_hi):
    """The excised average of include/rpf_engine.h (rpf_accumulate_device_excised) stated in numpy, on the (K, 3, N)
    rows of a series of statistics ([k, 0] = S1, [k, 1] = S2; PK is not used): integration k is kept in bin b iff
    sk_lo <= SK_k[b] <= sk_hi with SK = spectral_kurtosis(S1, S2, L) (NaN: flagged).  Returns (out (3, N) = clean, kept,
    total; mask (K, N) uint8, 1 = flagged).  The sums run over k in numpy's order, the engine's in its own: clean and
    total agree to a few ulp, kept and mask exactly."""
    rows = np.asarray(rows, dtype=np.float64)
    K, planes, N = rows.shape
    assert planes == 3
    s1 = rows[:, 0]
    sk = spectral_kurtosis(s1, rows[:, 1], L)
    with np.errstate(invalid="ignore"):
        keep = (sk >= sk_lo) & (sk <= sk_hi)
    out = np.zeros((3, N))
    out[0] = np.where(keep, s1, 0.0).sum(axis=0)
    out[1] = keep.sum(axis=0)
    out[2] = s1.sum(axis=0)
    return out, (~keep).astype(np.uint8)


def coherence(planes):
    """The magnitude-squared coherence of include/rpf_engine.h (rpf_accumulate_device_cross) from the (4, N) planes Saa,
    Sbb, Re Sab, Im Sab:  (re^2 + im^2) / (Saa Sbb), in double in exactly this order (the C++ host's coherence,
    host/datastore.h, does the same operations).  NaN where Saa Sbb == 0; not clamped: rounding can put it a few 1e-7
    above 1.  Of M frames it is a biased estimate: identically 1 for M = 1, about 1/M for unrelated streams."""
    p = np.asarray(planes, dtype=np.float64)
    if p.shape[0] != 4:
        raise ValueError("coherence: planes must be (4, N)")
    den = p[0] * p[1]
    num = p[2] * p[2] + p[3] * p[3]
    out = np.full(den.shape, np.nan)
    ok = den != 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        out[ok] = num[ok] / den[ok]
    return out


def cross_phase(planes):
    """arg Sab = atan2(Im Sab, Re Sab) in radians, from the same (4, N) planes (host/datastore.h: cross_phase)."""
    p = np.asarray(planes, dtype=np.float64)
    if p.shape[0] != 4:
        raise ValueError("cross_phase: planes must be (4, N)")
    return np.arctan2(p[3], p[2])


def coherence_matrix(V):
    """The magnitude-squared coherence of every pair of include/rpf_engine.h (rpf_correlate_device) from the (M, M, N)
    visibilities V:  gamma^2_ij = (re^2 + im^2) / (V_ii V_jj), with V_ii the real diagonal, in double in exactly this order
    (the C++ host's coherence_pair, host/datastore.h, does the same operations).  NaN where V_ii V_jj == 0; not clamped.
    The diagonal is 1 wherever the power is not 0.  Of F frames it is biased: identically 1 for F = 1, about 1/F for
    unrelated streams."""
    V = np.asarray(V)
    if V.ndim != 3 or V.shape[0] != V.shape[1]:
        raise ValueError("coherence_matrix: V must be (M, M, N)")
    re, im = np.real(V).astype(np.float64), np.imag(V).astype(np.float64)
    auto = np.real(np.diagonal(V, axis1=0, axis2=1)).T.astype(np.float64)       # (M, N)
    den = auto[:, None, :] * auto[None, :, :]
    num = re * re + im * im
    out = np.full(num.shape, np.nan)
    ok = den != 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        out[ok] = num[ok] / den[ok]
    return out


def quantiles(rows, q):
    """The per-bin quantiles of include/rpf_engine.h (rpf_quantile_select_device) stated in numpy, on (K, N) rows: with
    v_(0) <= ... <= v_(K-1) the values of a bin in np.sort's order (a NaN last), h = q (K - 1), j = floor(h), g = h - j,
    a = v_(j), b = v_(min(j + 1, K - 1)) and Q = a where g == 0 or a == b, else a + g (b - a) -- float64, one operation
    at a time.  Returns (nq, N); all NaN for K = 0.  q: values in [0, 1]."""
    rows = np.asarray(rows, dtype=np.float64)
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if rows.ndim != 2 or q.ndim != 1:
        raise ValueError("quantiles: rows must be (K, N) and q one-dimensional")
    if not np.all((q >= 0.0) & (q <= 1.0)):
        raise ValueError("quantiles: every q must be in [0, 1]")
    K, N = rows.shape
    out = np.full((q.size, N), np.nan)
    if K == 0:
        return out
    ordered = np.sort(rows, axis=0)
    for i, qi in enumerate(q):
        h = qi * np.float64(K - 1)
        j = int(np.floor(h))
        g = h - np.float64(j)
        a = ordered[j]
        b = ordered[min(j + 1, K - 1)]
        with np.errstate(invalid="ignore", over="ignore"):
            d = b - a
            gd = g * d
            mid = a + gd
            out[i] = np.where((g == 0.0) | (a == b), a, mid)
    return out
