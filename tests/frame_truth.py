"""The float64 reference of the per-frame quantities, stated once for every sample format and frame step: p[f, b] of
every frame and bin (helpers.truth_f64's evaluation kept per frame), the statistics S1 = sum p, S2 = sum p^2, PK = max p
over a stream, and the same three over the rows [k L, (k + 1) L) of a series.  tests/test_frame_truth.py ties it, bit for
bit, to the cu8-only statement test_gpu_spectral_stats.py keeps and to helpers.truth_f64."""
import numpy as np


def unpacked(fmt, stream):
    """The float32 values (I0, Q0, I1, ...) a stream of sample format `fmt` unpacks to, exactly: cu8 byte - 127, cs8 and
    cs16 the integer as stored, cf32 the float as stored."""
    s = np.ascontiguousarray(stream)
    if fmt == "cu8":
        return s.view(np.uint8).astype(np.float32) - np.float32(127.0)
    if fmt == "cs8":
        return s.view(np.uint8).view(np.int8).astype(np.float32)
    if fmt == "cs16":
        return s.view(np.uint8).view("<i2").astype(np.float32)
    assert fmt == "cf32", fmt
    return s.view(np.uint8).view("<f4").astype(np.float32)


def truth_frame_powers(N, values, frames, window=None, step=None):
    """p[f, b] in float64.  `values` are the unpacked float32 samples (unpacked()); frame f is the samples
    [f step, f step + N) (step = N unless given: overlapped frames); (-1)^n by the index inside the frame, the window as
    one float32 multiply, a numpy complex128 transform per frame."""
    S = N if step is None else step
    v = np.asarray(values)
    assert v.dtype == np.float32, "the samples as the float32 values the format unpacks to"
    v = v.reshape(-1, 2)
    assert v.shape[0] >= S * (frames - 1) + N
    sign = (1 - 2 * (np.arange(N) % 2)).astype(np.float32)
    w = None if window is None else np.asarray(window, dtype=np.float32)
    out = np.empty((frames, N))
    chunk = max(1, (1 << 22) // N)
    for f0 in range(0, frames, chunk):
        f1 = min(frames, f0 + chunk)
        idx = (np.arange(f0, f1) * S)[:, None] + np.arange(N)[None, :]
        x = v[idx] * sign[None, :, None]
        if w is not None:
            x = x * w[None, :, None]
        assert x.dtype == np.float32
        spec = np.fft.fft(x[..., 0].astype(np.float64) + 1j * x[..., 1].astype(np.float64), axis=1)
        out[f0:f1] = spec.real ** 2 + spec.imag ** 2
    return out


def planes(p):
    """S1 = sum, S2 = sum of squares, PK = maximum over the frames of p[f, b]: (3, N)."""
    return np.array([p.sum(axis=0), (p * p).sum(axis=0), p.max(axis=0)])


def row_planes(p, L, K):
    """planes() of the frames [k L, (k + 1) L) for k < K: (K, 3, N)."""
    g = p[:K * L].reshape(K, L, p.shape[1])
    return np.stack([g.sum(axis=1), (g * g).sum(axis=1), g.max(axis=1)], axis=1)
