"""Correlator of up to eight streams (include/rpf_engine.h, rpf_correlate_device): the float64 answer, the reference for
tests and users.  Nothing here touches a device."""
import numpy as np

from . import stft


def reference(streams, N, fmt="cu8", step=None, window=None, taps=1, coeffs=None):
    """V[i, j, k] = sum over the frames f of X_i,f[k] conj(X_j,f[k]), complex128 of shape (M, M, N), with X_m the rows
    of stft.reference of stream m (same arguments); the frames are those every stream holds whole (the shortest
    stream's).  F = 0 gives zeros."""
    rows = [stft.reference(s, N, fmt, step, window, taps, coeffs) for s in streams]
    F = min(r.shape[0] for r in rows)
    X = np.stack([r[:F] for r in rows])
    return np.einsum("ifk,jfk->ijk", X, np.conj(X))
