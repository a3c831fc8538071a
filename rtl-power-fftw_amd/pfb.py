"""Polyphase filter bank front end (include/rpf_engine.h, rpf_engine_create_pfb): the default prototype filter and the
float64 fold, the reference for tests and users.  Nothing here touches a device."""
import numpy as np

from . import _lib
from ._lib import RPFError, ReturnValue

MAX_TAPS = 32


def coefficients(N, taps):
    """The default prototype h[0 .. T N), float32: a sinc whose first zeros lie one channel width from the centre, under
    a Hamming window over the whole length,

        sinc((j - (T N - 1) / 2) / N) * (0.54 - 0.46 cos(2 pi j / (T N - 1))),   j in [0, T N),

    computed in double and scaled so that the sum of h^2 is N -- white noise then sits at the level the plain engine
    gives it -- and rounded to float32 once.  Symmetric: h[j] == h[T N - 1 - j]."""
    if taps < 1 or taps > MAX_TAPS or N < 2 or N % 2:
        raise RPFError("pfb.coefficients: taps must be in 1 .. %d and N a positive even number" % MAX_TAPS,
                       ReturnValue.InvalidArgument)
    M = taps * N
    j = np.arange(M, dtype=np.float64)
    h = np.sinc((j - (M - 1) / 2.0) / N) * (0.54 - 0.46 * np.cos(2.0 * np.pi * j / (M - 1)))
    h *= np.sqrt(N / np.sum(h * h))
    return h.astype(np.float32)


def sample_values(stream, sample_format="cu8"):
    """The samples of a byte stream as the engine converts them (cu8: v - 127; cs8, cs16, cf32: v), complex128."""
    raw = np.ascontiguousarray(stream).reshape(-1).view(np.uint8)
    if sample_format == "cu8":
        v = raw.astype(np.float64) - 127.0
    elif sample_format == "cs8":
        v = raw.view(np.int8).astype(np.float64)
    elif sample_format == "cs16":
        v = raw[:raw.size // 2 * 2].view("<i2").astype(np.float64)
    elif sample_format == "cf32":
        v = raw[:raw.size // 4 * 4].view("<f4").astype(np.float64)
    else:
        raise RPFError("Unknown sample format '%s' (one of: cu8, cs8, cs16, cf32)." % (sample_format,),
                       ReturnValue.InvalidArgument)
    v = v[:v.size // 2 * 2]
    return v[0::2] + 1j * v[1::2]


def fold(stream, N, taps, coeffs, sample_format="cu8"):
    """The fold in float64: z[f, n] = sum over t < T of h[t N + n] x[(f + t) N + n] for every frame the stream holds,
    frames x N complex128 (the (-1)^n is not applied).  stream: bytes of `sample_format` (a complex64 / float32 array
    is taken by its bytes when the format is cf32)."""
    x = sample_values(stream, sample_format)
    h = np.asarray(coeffs, dtype=np.float64).reshape(taps, N)
    frames = frames_in(x.size * _lib.SAMPLE_BYTES[sample_format], N, taps, _lib.SAMPLE_BYTES[sample_format])
    rows = x[:(frames + taps - 1) * N].reshape(-1, N) if frames else np.zeros((0, N), dtype=np.complex128)
    z = np.zeros((frames, N), dtype=np.complex128)
    for t in range(taps):
        z += h[t] * rows[t:t + frames]
    return z


def frames_in(nbytes, N, taps, sample_bytes=2):
    """frames(B) = B < b T N ? 0 : (B - b T N) / (b N) + 1 (rpf_frames_in of a PFB engine)."""
    from .datastore import frames_in as f
    return f(nbytes, N, N, sample_bytes, taps=taps)


def spectrum(z):
    """The float64 spectrum of folded frames as the engine lays it out: sum over the frames of |FFT((-1)^n z)|^2,
    bin N/2 = DC."""
    z = np.asarray(z)
    return np.sum(np.abs(np.fft.fftshift(np.fft.fft(z, axis=1), axes=1)) ** 2, axis=0)
