"""Incoherent dedispersion of the stored integrations (include/rpf_engine.h, rpf_dedisperse_device): the delay table
of a dispersion measure, the float64 answer that is the reference for tests and users, and a robust signal-to-noise
scale of the DM-time plane.  Nothing here touches a device."""
import numpy as np

K_DM = 4.148808e3          # s MHz^2 pc^-1 cm^3


def dm_delays(dms, fc, rate, N, L, step=None):
    """Delay table of the dispersion measures `dms` [pc cm^-3]: (D, N) int32, in integrations of L frames at frame step
    `step` (None = N), for N bins around the tuned frequency fc [Hz] at `rate` samples/s.  The highest bin is the
    reference (delay 0).  The operations are those of include/rpf_engine.h, in double, one rounding each (host/datastore.h's
    dm_delays does the same ones, so the integers agree)."""
    dms = np.atleast_1d(np.asarray(dms, dtype=np.float64))
    S = N if step is None else step
    if N < 1 or L < 1 or S < 1 or not rate > 0:
        raise ValueError("dm_delays: N, L, the frame step and the rate must be positive.")
    if not np.all(np.isfinite(dms) & (dms >= 0)):
        raise ValueError("dm_delays: a dispersion measure must be finite and not negative.")
    b = np.arange(N, dtype=np.int64)
    f = (np.float64(fc) + (b - N // 2).astype(np.float64) * (np.float64(rate) / np.float64(N))) / 1e6
    if not f[0] > 0:
        raise ValueError("dm_delays: the lowest bin's frequency must be positive, got %r MHz." % f[0])
    inv = 1.0 / (f * f)
    t_row = (np.float64(L) * np.float64(S)) / np.float64(rate)
    v = np.floor(((K_DM * dms)[:, None] * (inv - inv[N - 1])[None, :]) / t_row + 0.5)
    if not np.all(v < 2147483648.0):
        raise ValueError("dm_delays: a delay does not fit 32 bits.")
    return v.astype(np.int32)


def times(K, delays):
    """T = max(0, K - Dmax) for K rows and this table."""
    delays = np.asarray(delays)
    return max(0, int(K) - int(delays.max())) if delays.size else int(K)


def reference(rows, delays, weights=None):
    """out[d, t] = sum over the bins b, ascending, of weights[b] rows[t + delays[d, b], b], t < T = max(0, K - Dmax), in
    float64 with every product and every sum rounded on its own; a bin of weight 0 is not read.  rows (K, N), delays
    (D, N) integers >= 0, weights N values or None for all ones.  Returns (D, T)."""
    rows = np.asarray(rows, dtype=np.float64)
    delays = np.atleast_2d(np.asarray(delays)).astype(np.int64)
    K, N = rows.shape
    D = delays.shape[0]
    if delays.shape[1] != N or (delays.size and delays.min() < 0):
        raise ValueError("reference: delays must be (D, N) and not negative.")
    T = times(K, delays)
    # every trial at once: row d of `term` is rows[delays[d, b] : delays[d, b] + T, b]
    acc = np.zeros((D, T), dtype=np.float64)
    t = np.arange(T, dtype=np.int64)[None, :]
    for b in range(N):
        if weights is not None and weights[b] == 0:
            continue
        term = rows[delays[:, b][:, None] + t, b]
        acc = acc + (term if weights is None else np.float64(weights[b]) * term)
    return acc


def snr(plane):
    """(x - median) / (1.4826 MAD) of every trial (row) of the DM-time plane: the deviation in robust sigmas.  A trial
    whose MAD is 0 gives inf or NaN."""
    plane = np.atleast_2d(np.asarray(plane, dtype=np.float64))
    med = np.median(plane, axis=1, keepdims=True)
    mad = np.median(np.abs(plane - med), axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (plane - med) / (1.4826 * mad)
