"""Fold of a plane of time series at trial periods (include/rpf_engine.h, rpf_fold_device): the step of a period, the
phase bins, the float64 answer that is the reference for tests and users, and the reduced chi-square of a profile.
Nothing here touches a device."""
import math

import numpy as np

SEGMENTS = 16                # RPF_FOLD_SEGMENTS: the fixed order of the sums
MAX_PHASE_BINS = 128
_TWO64 = 1 << 64


def row_period_steps(periods_rows):
    """The steps of periods given in rows (times of the plane): uint64 array of int(ldexp(1.0 / pr, 64)), the phase
    advance per time in units of 2^-64 turn.  Refused unless every pr is finite and >= 2."""
    pr = np.atleast_1d(np.asarray(periods_rows, dtype=np.float64))
    if not np.all(np.isfinite(pr) & (pr >= 2.0)):
        raise ValueError("period_steps: a period must be finite and at least two rows; got %r rows."
                         % (pr[~(np.isfinite(pr) & (pr >= 2.0))][0],))
    # through Python integers: nothing passes through a signed 64-bit value
    return np.array([int(math.ldexp(1.0 / float(v), 64)) for v in pr], dtype=np.uint64)


def period_steps(periods_s, rate, N, L, step=None):
    """The steps of periods in seconds for rows of L frames at frame step `step` (None = N) of a stream at `rate`
    samples/s: t_row = (L S) / rate, pr = period / t_row, then row_period_steps.  The operations are those of
    include/rpf_engine.h, in double, one rounding each (host/datastore.h's period_steps does the same ones)."""
    S = N if step is None else step
    if N < 1 or L < 1 or S < 1 or not rate > 0:
        raise ValueError("period_steps: N, L, the frame step and the rate must be positive.")
    t_row = (np.float64(L) * np.float64(S)) / np.float64(rate)
    return row_period_steps(np.atleast_1d(np.asarray(periods_s, dtype=np.float64)) / t_row)


def phase_bins(step, T, NB):
    """bin(p, t) for t < T: (((t step) mod 2^64) >> 32) NB >> 32, as int64."""
    step = int(step)
    if not 0 <= step < _TWO64 or NB < 1:
        raise ValueError("phase_bins: the step must fit 64 bits and NB must be positive.")
    t = np.arange(int(T), dtype=np.uint64)
    with np.errstate(over="ignore"):
        phase = t * np.uint64(step)
    return (((phase >> np.uint64(32)) * np.uint64(NB)) >> np.uint64(32)).astype(np.int64)


def segment_bounds(T):
    """The 17 bounds of the 16 segments of T times: min(T, g ceil(T / 16))."""
    G = -(-int(T) // SEGMENTS)
    return [min(int(T), g * G) for g in range(SEGMENTS + 1)]


def reference(x, steps, NB):
    """prof (D, P, NB) float64, hits (P, NB) int32, mom (D, 2) float64 of the definition for x (D, T): per segment one
    np.bincount, in ascending t, the 16 segments then added in order; mom the same two-level sums of x and of x x."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    steps = [int(s) for s in np.atleast_1d(steps)]
    D, T = x.shape
    P = len(steps)
    bounds = segment_bounds(T)
    prof = np.zeros((D, P, NB), dtype=np.float64)
    hits = np.zeros((P, NB), dtype=np.int32)
    mom = np.zeros((D, 2), dtype=np.float64)
    zeros = np.zeros(T, dtype=np.int64)
    for p, step in enumerate(steps):
        bins = phase_bins(step, T, NB)
        hits[p] = np.bincount(bins, minlength=NB)
        for s in range(D):
            acc = np.zeros(NB, dtype=np.float64)
            for g in range(SEGMENTS):
                lo, hi = bounds[g], bounds[g + 1]
                acc = acc + np.bincount(bins[lo:hi], weights=x[s, lo:hi], minlength=NB)
            prof[s, p] = acc
    for s in range(D):
        sq = x[s] * x[s]
        for j, v in enumerate((x[s], sq)):
            acc = np.float64(0.0)
            for g in range(SEGMENTS):
                lo, hi = bounds[g], bounds[g + 1]
                acc = acc + np.bincount(zeros[lo:hi], weights=v[lo:hi], minlength=1)[0]
            mom[s, j] = acc
    return prof, hits, mom


def chi2(prof, hits, mom, T):
    """Reduced chi-square (D, P) of every profile against a flat one: mu = mom[:, 0] / T, v = mom[:, 1] / T - mu mu,
    sum over the bins with hits of hits (prof / hits - mu)^2 / v / (n_used - 1); NaN where fewer than two bins have
    hits or v <= 0."""
    prof = np.asarray(prof, dtype=np.float64)
    hits = np.asarray(hits)
    mom = np.asarray(mom, dtype=np.float64)
    D, P, NB = prof.shape
    out = np.full((D, P), np.nan)
    if T < 1:
        return out
    mu = mom[:, 0] / float(T)
    var = mom[:, 1] / float(T) - mu * mu
    for s in range(D):
        for p in range(P):
            used = hits[p] > 0
            n = int(np.count_nonzero(used))
            if n < 2 or not var[s] > 0:
                continue
            h = hits[p][used].astype(np.float64)
            dev = prof[s, p][used] / h - mu[s]
            out[s, p] = np.sum(h * dev * dev / var[s]) / (n - 1)
    return out
