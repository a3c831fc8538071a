"""Host-side mirror of ``class Datastore`` (/root/reference/src/datastore.h:35-68)
over the C-ABI of include/rpf_engine.h.  Used by tests/ and bench.py; the C++
host wrapper with the same shape lives in rtl-power-fftw_amd/host/."""
import ctypes
import sys

import numpy as np

from . import _lib
from ._lib import RPFError, ReturnValue

BASE_BUF = 16384                # params.h:26
DEFAULT_BUF_MULTIPLIER = 100    # params.h:27


class Params:
    """The Params fields the hot path reads, with the reference's defaults
    (/root/reference/src/params.h:33-66)."""

    def __init__(self, N=512, buffers=5, buf_length=BASE_BUF * DEFAULT_BUF_MULTIPLIER,
                 repeats=None, window=False, sample_rate=2000000, cfreq=1420405752,
                 linear=False, baseline=False, frame_step=None, sample_format="cu8", bin_stats=False,
                 pfb_taps=0, pfb_coeffs=None):
        self.N = N
        # polyphase filter bank front end (rpf_engine_create_pfb): T taps, 0 = none; pfb_coeffs: T x N float32 values,
        # None = pfb.coefficients(N, T), the default prototype
        self.pfb_taps = int(pfb_taps)
        self.pfb_coeffs = pfb_coeffs
        # per-bin statistics beside the power (RPF_FLAG_BIN_STATS): Datastore.sum_sq, Datastore.peak
        self.bin_stats = bool(bin_stats)
        # what one complex sample of the stream is: "cu8" (the reference's), "cs8", "cs16", "cf32" (RPF_FORMAT_*)
        if sample_format not in _lib.FORMATS:
            raise RPFError("Unknown sample format '%s' (one of: cu8, cs8, cs16, cf32)." % (sample_format,),
                           ReturnValue.InvalidArgument)
        self.sample_format = sample_format
        # frame step S in complex samples (rpf_config::frame_step): frame f = samples [f S, f S + N); None = N
        self.frame_step = N if frame_step is None else frame_step
        self.buffers = buffers
        self.buf_length = buf_length
        # params.h:56: repeats = buf_length/(2*N) unless -n/-t say otherwise -- a sample budget, which overlapped
        # frames turn into more frames from the same samples
        self.repeats = (frames_for_budget(buf_length // (_lib.SAMPLE_BYTES[sample_format] * N), N, self.frame_step,
                                          max(self.pfb_taps, 1))
                        if repeats is None
                        else repeats)
        self.window = window
        self.sample_rate = sample_rate
        self.cfreq = cfreq
        self.linear = linear
        self.baseline = baseline


def frames_for_budget(r0, N, step, taps=1):
    """R = floor((R0 - 1) N / S) + 1: the frames at step S the samples of R0 side-by-side frames hold (R0 for S = N).
    With a PFB of `taps` taps a frame spans taps x N samples: R0 - (taps - 1) frames, at least one."""
    if r0 < 1 or not step:
        return r0
    if taps > 1:
        return max(r0 - (taps - 1), 1)
    return (r0 - 1) * N // step + 1


def _as_bytes(stream):
    """The bytes of a host stream: a complex64 or float32 array (cf32 samples) is viewed as its bytes, anything else
    is taken as raw bytes."""
    a = np.asarray(stream)
    if a.dtype in (np.complex64, np.float32):
        return np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return np.ascontiguousarray(a, dtype=np.uint8)


def frames_in(nbytes, N, step, sample_bytes=2, taps=1):
    """frames(B) = B < bTN ? 0 : (B - bTN) / (bS) + 1 (rpf_frames_in); b = sample_bytes, T = taps (a PFB engine's
    frame spans T N samples and its step is N; 1 without PFB)."""
    b = sample_bytes
    return 0 if nbytes < b * taps * N else (nbytes - b * taps * N) // (b * step) + 1


def frame_span(frames, N, step, sample_bytes=2, taps=1):
    """Bytes `frames` frames span: bTN + bS (frames - 1) (rpf_frame_span); b = sample_bytes, T = taps."""
    return 0 if frames < 1 else sample_bytes * (taps * N + step * (frames - 1))


class Datastore:
    """``Datastore(params, window_values)``: buffer pool + FFT/accumulate worker."""

    def __init__(self, params, window_values=None, device=0, flags=0, struct_size=None):
        """struct_size: rpf_config.struct_size to pass (default sizeof; _lib.CONFIG_SIZE_V2_0 = a caller built
        against the config without frame_step)."""
        self.params = params
        self._lib = _lib.load()
        self._handle = ctypes.c_void_p()
        self._window = None
        cfg = _lib.rpf_config()
        cfg.struct_size = ctypes.sizeof(_lib.rpf_config) if struct_size is None else struct_size
        cfg.N = params.N
        if params.window:
            if window_values is None or len(window_values) != params.N:
                raise RPFError("Error reading window function. Expected %d values, found %d."
                               % (params.N, 0 if window_values is None else len(window_values)),
                               ReturnValue.InvalidInput)
            self._window = np.ascontiguousarray(window_values, dtype=np.float32)
            cfg.window = self._window.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        cfg.n_buffers = params.buffers
        cfg.buffer_capacity = params.buf_length
        cfg.device = device
        cfg.flags = flags | _lib.FLAG_SAMPLE_FORMAT(_lib.FORMATS[getattr(params, "sample_format", "cu8")])
        if getattr(params, "bin_stats", False):
            cfg.flags |= _lib.FLAG_BIN_STATS
        cfg.frame_step = getattr(params, "frame_step", params.N)
        taps = getattr(params, "pfb_taps", 0)
        if taps:
            from . import pfb
            coeffs = getattr(params, "pfb_coeffs", None)
            if coeffs is None and 1 <= taps <= pfb.MAX_TAPS:
                coeffs = pfb.coefficients(params.N, taps)
            if coeffs is not None:
                coeffs = np.ascontiguousarray(coeffs, dtype=np.float32).reshape(-1)
                if coeffs.size != taps * params.N and taps >= 1:
                    raise RPFError("Error reading PFB coefficients. Expected %d values, found %d."
                                   % (taps * params.N, coeffs.size), ReturnValue.InvalidInput)
            self._pfb_coeffs = coeffs
            rc = self._lib.rpf_engine_create_pfb(
                ctypes.byref(cfg), taps,
                None if coeffs is None else coeffs.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                ctypes.byref(self._handle))
        else:
            rc = self._lib.rpf_engine_create(ctypes.byref(cfg), ctypes.byref(self._handle))
        if rc != 0:
            self._handle = ctypes.c_void_p()
            raise RPFError(self._lib.rpf_last_global_error().decode(), rc)
        self.pwr = np.zeros(params.N, dtype=np.float64)
        # stats engines (Params(bin_stats=True) or _lib.FLAG_BIN_STATS): S2 and PK of the last acquisition, else None
        self.sum_sq = self.peak = None
        if self.has_bin_stats:
            self.sum_sq = np.zeros(params.N, dtype=np.float64)
            self.peak = np.zeros(params.N, dtype=np.float64)
        self.repeats_done = 0

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "_handle", None):
            self._lib.rpf_engine_destroy(self._handle)
            self._handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise RPFError(self._lib.rpf_last_error(self._handle).decode(), rc)

    # -- the hand-off protocol of Acquisition::run ------------------------
    def begin(self, repeats=None):
        """acquisition.cxx:252-256"""
        self._check(self._lib.rpf_begin(self._handle,
                                        self.params.repeats if repeats is None else repeats))

    def acquire(self):
        """acquisition.cxx:278-285 -> writable uint8 view of a pinned buffer"""
        ptr = ctypes.c_void_p()
        cap = ctypes.c_size_t()
        self._check(self._lib.rpf_buffer_acquire(self._handle, ctypes.byref(ptr), ctypes.byref(cap)))
        arr = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint8)),
                                    shape=(cap.value,))
        return arr

    def submit(self, buf, nbytes):
        """acquisition.cxx:302,320-323"""
        self._check(self._lib.rpf_buffer_submit(self._handle, ctypes.c_void_p(buf.ctypes.data), nbytes))

    def unget(self, buf):
        """acquisition.cxx:310-314"""
        self._check(self._lib.rpf_buffer_unget(self._handle, ctypes.c_void_p(buf.ctypes.data)))

    def finish(self):
        """acquisition.cxx:343-347; afterwards pwr / repeats_done are valid"""
        done = ctypes.c_int64()
        self._check(self._lib.rpf_finish(self._handle, ctypes.byref(done)))
        self.repeats_done = done.value
        self._check(self._lib.rpf_get_power(self._handle,
                                            self.pwr.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        self._fetch_bin_stats()
        return self.repeats_done

    @property
    def has_bin_stats(self):
        """rpf_has_bin_stats: does the engine keep S2 and PK beside the power?"""
        return bool(self._lib.rpf_has_bin_stats(self._handle))

    def _fetch_bin_stats(self):
        if self.sum_sq is not None:
            dp = ctypes.POINTER(ctypes.c_double)
            self._check(self._lib.rpf_get_bin_stats(self._handle, self.sum_sq.ctypes.data_as(dp),
                                                    self.peak.ctypes.data_as(dp)))

    def spectral_kurtosis(self):
        """SK of the last acquisition (stats.spectral_kurtosis of pwr, sum_sq, repeats_done)."""
        from . import stats
        return stats.spectral_kurtosis(self.pwr, self.sum_sq, self.repeats_done)

    @property
    def queue_histogram(self):
        out = (ctypes.c_int * (self.params.buffers + 1))()
        self._check(self._lib.rpf_get_histogram(self._handle, out))
        return list(out)

    def printQueueHistogram(self, file=sys.stderr):
        """datastore.cxx:98-103"""
        file.write("Buffer queue histogram: " + "".join("%d " % v for v in self.queue_histogram) + "\n")

    # -- whole-stream conveniences -----------------------------------------
    def accumulate(self, stream, repeats=None):
        """Run one acquisition over a contiguous host byte stream through the
        buffer queues.  Returns (pwr copy, repeats_done)."""
        stream = _as_bytes(stream)
        done = ctypes.c_int64()
        self._check(self._lib.rpf_accumulate(
            self._handle, ctypes.c_void_p(stream.ctypes.data), stream.size,
            self.params.repeats if repeats is None else repeats,
            self.pwr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(done)))
        self.repeats_done = done.value
        self._fetch_bin_stats()
        return self.pwr.copy(), self.repeats_done

    def register_stream(self, stream):
        """rpf_stream_register: pin a host array that will be replayed more than once; accumulate() on it (or on a slice
        of it) then skips the copy into the pool.  Keep the array alive until unregister_stream / close."""
        assert stream.dtype == np.uint8 and stream.flags["C_CONTIGUOUS"]
        self._check(self._lib.rpf_stream_register(self._handle, ctypes.c_void_p(stream.ctypes.data), stream.size))

    def unregister_stream(self, stream):
        self._check(self._lib.rpf_stream_unregister(self._handle, ctypes.c_void_p(stream.ctypes.data)))

    def accumulate_device(self, d_stream_ptr, nbytes, repeats, d_pwr_ptr, hip_stream=0):
        """Enqueue the fused kernel over a stream resident in HBM (raw device
        pointers; asynchronous).  Returns the number of frames that will be summed."""
        done = ctypes.c_int64()
        self._check(self._lib.rpf_accumulate_device(
            self._handle, ctypes.c_void_p(d_stream_ptr), nbytes, repeats,
            ctypes.c_void_p(d_pwr_ptr), ctypes.c_void_p(hip_stream), ctypes.byref(done)))
        return done.value

    def accumulate_device_stats(self, d_stream_ptr, nbytes, repeats, d_out_ptr, hip_stream=0):
        """rpf_accumulate_device_stats: as accumulate_device, d_out = 3 x N device doubles (S1, S2, PK)."""
        done = ctypes.c_int64()
        self._check(self._lib.rpf_accumulate_device_stats(
            self._handle, ctypes.c_void_p(d_stream_ptr), nbytes, repeats,
            ctypes.c_void_p(d_out_ptr), ctypes.c_void_p(hip_stream), ctypes.byref(done)))
        return done.value

    # -- cross-spectrum of two streams (rpf_accumulate[_device]_cross; include/rpf_engine.h has the definition) -------
    def accumulate_device_cross(self, d_a_ptr, d_b_ptr, nbytes, repeats, d_out_ptr, hip_stream=0):
        """rpf_accumulate_device_cross: two streams of nbytes each resident in HBM, d_out = 4 x N device doubles (Saa,
        Sbb, Re Sab, Im Sab); asynchronous.  Returns the number of frames that will be summed."""
        done = ctypes.c_int64()
        self._check(self._lib.rpf_accumulate_device_cross(
            self._handle, ctypes.c_void_p(d_a_ptr), ctypes.c_void_p(d_b_ptr), nbytes, repeats,
            ctypes.c_void_p(d_out_ptr), ctypes.c_void_p(hip_stream), ctypes.byref(done)))
        return done.value

    def accumulate_cross(self, a, b, repeats=None):
        """rpf_accumulate_cross: the same on two host streams of equal length (not through the buffer queues).  Returns
        ((4, N) array: Saa, Sbb, Re Sab, Im Sab; frames); stats.coherence and stats.cross_phase take the array.
        repeats None = every whole frame the streams hold."""
        a, b = _as_bytes(a), _as_bytes(b)
        if a.size != b.size:
            raise RPFError("accumulate_cross: the two streams must have the same length; got %d and %d bytes."
                           % (a.size, b.size), ReturnValue.InvalidArgument)
        out = np.zeros((4, self.params.N), dtype=np.float64)
        done = ctypes.c_int64()
        self._check(self._lib.rpf_accumulate_cross(
            self._handle, ctypes.c_void_p(a.ctypes.data), ctypes.c_void_p(b.ctypes.data), a.size,
            (1 << 62) if repeats is None else repeats,
            out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(done)))
        return out, done.value

    # -- the frames' spectra themselves (rpf_stft[_device]; include/rpf_engine.h has the definition) ------------------
    def stft_device(self, d_stream_ptr, nbytes, max_frames, d_out_ptr, hip_stream=0):
        """rpf_stft_device: row f of d_out (F x N device complex64, 16-byte aligned) = the float32 transform of frame f
        of a stream resident in HBM; asynchronous.  Returns F."""
        done = ctypes.c_int64()
        self._check(self._lib.rpf_stft_device(
            self._handle, ctypes.c_void_p(d_stream_ptr), nbytes, max_frames, ctypes.c_void_p(d_out_ptr),
            ctypes.byref(done), ctypes.c_void_p(hip_stream)))
        return done.value

    def stft(self, stream, max_frames=None):
        """rpf_stft: the same on a host byte stream.  Returns a complex64 array of shape (F, N); max_frames None = every
        whole frame the stream holds."""
        stream = _as_bytes(stream)
        if max_frames is None:
            max_frames = 1 << 62
        rows = max(min(max_frames, self.frames_in(stream.size)), 0)
        out = np.zeros((max(rows, 1), self.params.N), dtype=np.complex64)
        done = ctypes.c_int64()
        self._check(self._lib.rpf_stft(
            self._handle, ctypes.c_void_p(stream.ctypes.data), stream.size, max_frames,
            ctypes.c_void_p(out.ctypes.data), ctypes.byref(done)))
        return out[:done.value]

    # -- correlator of up to eight streams (rpf_correlate[_device]; include/rpf_engine.h has the definition) ----------
    def correlate_device(self, d_ptrs, nbytes, repeats, d_out_ptr, hip_stream=0):
        """rpf_correlate_device: M = len(d_ptrs) streams of nbytes each resident in HBM, d_out = M x M x 2 x N device
        doubles (the visibilities V_ij, re and im); asynchronous.  Returns F, the number of frames that will be summed."""
        ptrs = (ctypes.c_void_p * max(len(d_ptrs), 1))(*[ctypes.c_void_p(p) for p in d_ptrs])
        done = ctypes.c_int64()
        self._check(self._lib.rpf_correlate_device(
            self._handle, ptrs, len(d_ptrs), nbytes, repeats, ctypes.c_void_p(d_out_ptr), ctypes.c_void_p(hip_stream),
            ctypes.byref(done)))
        return done.value

    def correlate(self, streams, repeats=None):
        """rpf_correlate: the same on M host streams of equal length (not through the buffer queues).  Returns
        (V complex128 of shape (M, M, N), F); stats.coherence_matrix takes V.  repeats None = every whole frame the
        streams hold."""
        streams = [_as_bytes(s) for s in streams]
        sizes = sorted({s.size for s in streams})
        if len(sizes) > 1:
            raise RPFError("correlate: the streams must have the same length; got %s bytes."
                           % ", ".join(str(s.size) for s in streams), ReturnValue.InvalidArgument)
        M, N = len(streams), self.params.N
        out = np.zeros((max(M, 1), max(M, 1), 2, N), dtype=np.float64)
        ptrs = (ctypes.c_void_p * max(M, 1))(*[ctypes.c_void_p(s.ctypes.data) for s in streams])
        done = ctypes.c_int64()
        self._check(self._lib.rpf_correlate(
            self._handle, ptrs, M, sizes[0] if sizes else 0, (1 << 62) if repeats is None else repeats,
            out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(done)))
        v = np.empty((out.shape[0], out.shape[1], N), dtype=np.complex128)
        v.real, v.imag = out[:, :, 0, :], out[:, :, 1, :]          # the doubles as they came, bit for bit
        return v, done.value

    def accumulate_device_series(self, d_stream_ptr, nbytes, frames_per_spectrum, max_spectra, d_out_ptr, hip_stream=0):
        """rpf_accumulate_device_series: consecutive spectra of `frames_per_spectrum` frames of a stream resident in
        HBM, row k of d_out (K x N device doubles) = frames [k L, (k + 1) L); asynchronous.  Returns K."""
        done = ctypes.c_int64()
        self._check(self._lib.rpf_accumulate_device_series(
            self._handle, ctypes.c_void_p(d_stream_ptr), nbytes, frames_per_spectrum, max_spectra,
            ctypes.c_void_p(d_out_ptr), ctypes.c_void_p(hip_stream), ctypes.byref(done)))
        return done.value

    def accumulate_series(self, stream, frames_per_spectrum, max_spectra=None):
        """rpf_accumulate_series: the same on a host byte stream (not through the buffer queues).  Returns
        (K x N array, K); max_spectra None = every whole spectrum the stream holds."""
        stream = _as_bytes(stream)
        if max_spectra is None:
            max_spectra = max(self.frames_in(stream.size) // frames_per_spectrum, 0) if frames_per_spectrum >= 1 else 0
        rows = max(min(max_spectra, self.frames_in(stream.size) // max(frames_per_spectrum, 1)), 0)
        out = np.zeros((max(rows, 1), self.params.N), dtype=np.float64)
        done = ctypes.c_int64()
        self._check(self._lib.rpf_accumulate_series(
            self._handle, ctypes.c_void_p(stream.ctypes.data), stream.size, frames_per_spectrum, max_spectra,
            out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(done)))
        return out[:done.value], done.value

    def accumulate_device_series_stats(self, d_stream_ptr, nbytes, frames_per_spectrum, max_spectra, d_out_ptr, hip_stream=0):
        """rpf_accumulate_device_series_stats (stats engines): as accumulate_device_series, row k of d_out (K x 3 x N
        device doubles) = S1, S2, PK of frames [k L, (k + 1) L); asynchronous.  Returns K."""
        done = ctypes.c_int64()
        self._check(self._lib.rpf_accumulate_device_series_stats(
            self._handle, ctypes.c_void_p(d_stream_ptr), nbytes, frames_per_spectrum, max_spectra,
            ctypes.c_void_p(d_out_ptr), ctypes.c_void_p(hip_stream), ctypes.byref(done)))
        return done.value

    def accumulate_series_stats(self, stream, frames_per_spectrum, max_spectra=None):
        """rpf_accumulate_series_stats: the same on a host byte stream (not through the buffer queues).  Returns
        (K x 3 x N array, K), [k, 0] = S1, [k, 1] = S2, [k, 2] = PK; stats.spectral_kurtosis(out[:, 0], out[:, 1],
        frames_per_spectrum) is the spectral kurtosis of every row.  max_spectra None = every whole spectrum."""
        stream = _as_bytes(stream)
        if max_spectra is None:
            max_spectra = max(self.frames_in(stream.size) // frames_per_spectrum, 0) if frames_per_spectrum >= 1 else 0
        rows = max(min(max_spectra, self.frames_in(stream.size) // max(frames_per_spectrum, 1)), 0)
        out = np.zeros((max(rows, 1), 3, self.params.N), dtype=np.float64)
        done = ctypes.c_int64()
        self._check(self._lib.rpf_accumulate_series_stats(
            self._handle, ctypes.c_void_p(stream.ctypes.data), stream.size, frames_per_spectrum, max_spectra,
            out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(done)))
        return out[:done.value], done.value

    def accumulate_device_excised(self, d_stream_ptr, nbytes, frames_per_spectrum, max_spectra, sk_lo, sk_hi, d_out_ptr,
                                  d_mask_ptr=0, hip_stream=0):
        """rpf_accumulate_device_excised (stats engines): the excised average of a stream resident in HBM, d_out = 3 x N
        device doubles (clean, kept, total), d_mask = K x N device bytes (1 = flagged) or 0; asynchronous.  Returns K."""
        done = ctypes.c_int64()
        self._check(self._lib.rpf_accumulate_device_excised(
            self._handle, ctypes.c_void_p(d_stream_ptr), nbytes, frames_per_spectrum, max_spectra, sk_lo, sk_hi,
            ctypes.c_void_p(d_out_ptr), ctypes.c_void_p(d_mask_ptr or None), ctypes.c_void_p(hip_stream),
            ctypes.byref(done)))
        return done.value

    def accumulate_excised(self, stream, frames_per_spectrum, sk_lo, sk_hi, max_spectra=None, want_mask=False):
        """rpf_accumulate_excised: the same on a host byte stream (not through the buffer queues).  Returns
        (out (3, N): clean, kept, total; mask (K, N) uint8 with 1 = flagged, or None; K).  stats.sk_limits gives
        thresholds; max_spectra None = every whole spectrum the stream holds."""
        stream = _as_bytes(stream)
        if max_spectra is None:
            max_spectra = max(self.frames_in(stream.size) // frames_per_spectrum, 0) if frames_per_spectrum >= 1 else 0
        rows = max(min(max_spectra, self.frames_in(stream.size) // max(frames_per_spectrum, 1)), 0)
        out = np.zeros((3, self.params.N), dtype=np.float64)
        mask = np.zeros((max(rows, 1), self.params.N), dtype=np.uint8) if want_mask else None
        done = ctypes.c_int64()
        self._check(self._lib.rpf_accumulate_excised(
            self._handle, ctypes.c_void_p(stream.ctypes.data), stream.size, frames_per_spectrum, max_spectra, sk_lo, sk_hi,
            out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if want_mask else None, ctypes.byref(done)))
        return out, (mask[:done.value] if want_mask else None), done.value

    # -- per-bin quantiles of the integrations (rpf_quantile_*; include/rpf_engine.h has the definition) ----------
    def quantile_reset(self):
        """rpf_quantile_reset: forget the stored rows (the allocation stays)."""
        self._check(self._lib.rpf_quantile_reset(self._handle))

    @property
    def quantile_rows(self):
        """rpf_quantile_rows: rows the store holds."""
        return self._lib.rpf_quantile_rows(self._handle)

    @property
    def quantile_max_rows(self):
        """rpf_quantile_max_rows: rows the store can hold, max(1, 2^27 / N)."""
        return self._lib.rpf_quantile_max_rows(self._handle)

    def quantile_append_device(self, d_stream_ptr, nbytes, frames_per_spectrum, max_spectra, hip_stream=0):
        """rpf_quantile_append_device: the rows accumulate_device_series would write for this call, appended to the
        engine's row store; asynchronous.  Returns the number of rows appended."""
        done = ctypes.c_int64()
        self._check(self._lib.rpf_quantile_append_device(
            self._handle, ctypes.c_void_p(d_stream_ptr), nbytes, frames_per_spectrum, max_spectra,
            ctypes.c_void_p(hip_stream), ctypes.byref(done)))
        return done.value

    def quantile_append(self, stream, frames_per_spectrum, max_spectra=None):
        """rpf_quantile_append: the same on a host byte stream (not through the buffer queues).  Returns the number of
        rows appended; max_spectra None = every whole spectrum the stream holds."""
        stream = _as_bytes(stream)
        if max_spectra is None:
            max_spectra = max(self.frames_in(stream.size) // frames_per_spectrum, 0) if frames_per_spectrum >= 1 else 0
        done = ctypes.c_int64()
        self._check(self._lib.rpf_quantile_append(
            self._handle, ctypes.c_void_p(stream.ctypes.data), stream.size, frames_per_spectrum, max_spectra,
            ctypes.byref(done)))
        return done.value

    @staticmethod
    def _quantile_list(q):
        q = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=np.float64)))
        return q, q.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def quantile_select_device(self, q, d_out_ptr, hip_stream=0):
        """rpf_quantile_select_device: the quantiles q (host values in [0, 1], at most 8) of the stored rows into
        d_out = len(q) x N device doubles; asynchronous."""
        q, qp = self._quantile_list(q)
        self._check(self._lib.rpf_quantile_select_device(self._handle, qp, q.size, ctypes.c_void_p(d_out_ptr),
                                                         ctypes.c_void_p(hip_stream)))

    def quantile_select(self, q):
        """rpf_quantile_select: the same into a (len(q), N) array; stats.quantiles(rows, q) of the stored rows."""
        q, qp = self._quantile_list(q)
        out = np.zeros((max(q.size, 1), self.params.N), dtype=np.float64)
        self._check(self._lib.rpf_quantile_select(self._handle, qp, q.size,
                                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return out[:q.size]

    # -- incoherent dedispersion of the stored rows (rpf_dedisperse[_device]; include/rpf_engine.h has the definition) --
    def _dedisperse_args(self, delays, weights):
        delays = np.ascontiguousarray(np.atleast_2d(np.asarray(delays)), dtype=np.int32)
        if delays.ndim != 2 or delays.shape[1] != self.params.N:
            raise RPFError("dedisperse: delays must be (D, N) with N = %d; got shape %s." % (self.params.N, delays.shape),
                           ReturnValue.InvalidArgument)
        wp = None
        if weights is not None:
            weights = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
            if weights.size != self.params.N:
                raise RPFError("dedisperse: weights must hold N = %d values; got %d." % (self.params.N, weights.size),
                               ReturnValue.InvalidArgument)
            wp = weights.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        return delays, delays.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), weights, wp

    def dedisperse_times(self, delays):
        """rpf_dedisperse_times: T = max(0, rows stored - largest delay) for this table."""
        delays, dp, _, _ = self._dedisperse_args(delays, None)
        return self._lib.rpf_dedisperse_times(self._handle, dp, delays.shape[0])

    def dedisperse_device(self, delays, weights, d_out_ptr, capacity, hip_stream=0):
        """rpf_dedisperse_device: the DM-time plane of the stored rows for the host table delays (D, N) and the host
        weights (N, or None for ones) into d_out = `capacity` device doubles, D x T of them written; asynchronous.
        Returns T."""
        delays, dp, weights, wp = self._dedisperse_args(delays, weights)
        times = ctypes.c_int64()
        self._check(self._lib.rpf_dedisperse_device(self._handle, dp, wp, delays.shape[0], ctypes.c_void_p(d_out_ptr),
                                                    capacity, ctypes.c_void_p(hip_stream), ctypes.byref(times)))
        return times.value

    def dedisperse(self, delays, weights=None):
        """rpf_dedisperse: the same into a (D, T) array; dedisperse.reference(rows, delays, weights) of the stored rows."""
        delays, dp, weights, wp = self._dedisperse_args(delays, weights)
        D = delays.shape[0]
        T = max(self._lib.rpf_dedisperse_times(self._handle, dp, D), 0)
        out = np.zeros(max(D * T, 1), dtype=np.float64)
        times = ctypes.c_int64()
        self._check(self._lib.rpf_dedisperse(self._handle, dp, wp, D, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                             D * T, ctypes.byref(times)))
        return out[:D * times.value].reshape(D, times.value)

    # -- fold of a plane at trial periods (rpf_fold_device, rpf_dedisperse_fold; include/rpf_engine.h has the definition) --
    @staticmethod
    def _fold_steps(steps, phase_bins):
        steps = np.ascontiguousarray(np.atleast_1d(steps), dtype=np.uint64)
        if steps.ndim != 1:
            raise RPFError("fold: steps must be a list of 64-bit values; got shape %s." % (steps.shape,), ReturnValue.InvalidArgument)
        return steps, steps.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), int(phase_bins)

    def fold_device(self, d_series_ptr, n_series, T, steps, phase_bins, d_prof_ptr, capacity, d_hits_ptr=None, d_mom_ptr=None,
                    hip_stream=0):
        """rpf_fold_device: folds the n_series x T device doubles at d_series at the host `steps` (fold.period_steps)
        into phase_bins bins: d_prof = `capacity` device doubles, n_series x len(steps) x phase_bins written; d_hits
        (len(steps) x phase_bins int32) and d_mom (n_series x 2 doubles) may be None.  Asynchronous on hip_stream."""
        steps, sp, NB = self._fold_steps(steps, phase_bins)
        self._check(self._lib.rpf_fold_device(self._handle, ctypes.c_void_p(d_series_ptr), n_series, T, sp, steps.size, NB,
                                              ctypes.c_void_p(d_prof_ptr), capacity, ctypes.c_void_p(d_hits_ptr),
                                              ctypes.c_void_p(d_mom_ptr), ctypes.c_void_p(hip_stream)))

    def dedisperse_fold(self, delays, weights, steps, phase_bins):
        """rpf_dedisperse_fold: dedisperses the stored rows (as `dedisperse`) and folds the plane on the device at
        `steps`.  Returns prof (D, P, NB), hits (P, NB) int32, mom (D, 2) and T: fold.reference of that plane."""
        delays, dp, weights, wp = self._dedisperse_args(delays, weights)
        steps, sp, NB = self._fold_steps(steps, phase_bins)
        D, P = delays.shape[0], steps.size
        prof = np.zeros(max(D * P * NB, 1), dtype=np.float64)
        hits = np.zeros(max(P * NB, 1), dtype=np.int32)
        mom = np.zeros((D, 2), dtype=np.float64)
        times = ctypes.c_int64()
        self._check(self._lib.rpf_dedisperse_fold(self._handle, dp, wp, D, sp, P, NB, prof.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                  D * P * NB, hits.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                  mom.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(times)))
        return prof[:D * P * max(NB, 0)].reshape(D, P, NB), hits[:P * NB].reshape(P, NB), mom, times.value

    def accumulate_quantiles(self, stream, frames_per_spectrum, q=(0.5,), max_spectra=None):
        """Reset, append, select: the per-bin quantiles q over the integrations of `frames_per_spectrum` frames of a
        host stream.  Returns ((len(q), N) array, K)."""
        self.quantile_reset()
        done = self.quantile_append(stream, frames_per_spectrum, max_spectra)
        return self.quantile_select(q), done

    def series_launches(self):
        """rpf_series_launches: transform launches of the last series call (1 = the one-launch path)."""
        return self._lib.rpf_series_launches(self._handle)

    def device_fused(self, d_stream_ptr, nbytes, repeats, hip_stream=0):
        """K1 only (measurement hook, rpf_device_fused)."""
        done = ctypes.c_int64()
        self._check(self._lib.rpf_device_fused(self._handle, ctypes.c_void_p(d_stream_ptr), nbytes,
                                               repeats, ctypes.c_void_p(hip_stream), ctypes.byref(done)))
        return done.value

    def device_reduce(self, d_pwr_ptr, hip_stream=0):
        """K3 only (measurement hook, rpf_device_reduce)."""
        self._check(self._lib.rpf_device_reduce(self._handle, ctypes.c_void_p(d_pwr_ptr),
                                                ctypes.c_void_p(hip_stream)))

    @staticmethod
    def _hop_arrays(d_stream_ptrs, nbytes, repeats):
        H = len(d_stream_ptrs)
        assert len(nbytes) == H and len(repeats) == H
        return (H, (ctypes.c_void_p * H)(*[int(p) for p in d_stream_ptrs]),
                (ctypes.c_size_t * H)(*[int(b) for b in nbytes]),
                (ctypes.c_int64 * H)(*[int(r) for r in repeats]), (ctypes.c_int64 * H)())

    def accumulate_device_hops(self, d_stream_ptrs, nbytes, repeats, d_pwr_ptr, hip_stream=0):
        """A whole scan of device-resident hops in one call (rpf_accumulate_device_hops): hop h's
        spectrum lands in d_pwr[h*N : (h+1)*N].  Returns the frames summed per hop."""
        H, ptrs, nb, rep, done = self._hop_arrays(d_stream_ptrs, nbytes, repeats)
        self._check(self._lib.rpf_accumulate_device_hops(self._handle, ptrs, nb, rep, H, ctypes.c_void_p(d_pwr_ptr),
                                                         ctypes.c_void_p(hip_stream), done))
        return list(done)

    def device_fused_hops(self, d_stream_ptrs, nbytes, repeats, hip_stream=0):
        """K1 over up to max_hops_per_launch() hops in ONE launch (measurement hook); device_reduce()
        then writes all their spectra."""
        H, ptrs, nb, rep, done = self._hop_arrays(d_stream_ptrs, nbytes, repeats)
        self._check(self._lib.rpf_device_fused_hops(self._handle, ptrs, nb, rep, H, ctypes.c_void_p(hip_stream), done))
        return list(done)

    def frames_in(self, nbytes):
        """rpf_frames_in: frames a stream of nbytes holds at this engine's frame step."""
        return self._lib.rpf_frames_in(self._handle, nbytes)

    def frame_span(self, frames):
        """rpf_frame_span: bytes `frames` frames span at this engine's frame step."""
        return self._lib.rpf_frame_span(self._handle, frames)

    @property
    def pfb_taps(self):
        """rpf_pfb_taps: T of a PFB engine, 0 for an engine without PFB."""
        return self._lib.rpf_pfb_taps(self._handle)

    @property
    def sample_bytes(self):
        """rpf_sample_bytes: bytes per complex sample of this engine's format (2, 2, 4, 8)."""
        return self._lib.rpf_sample_bytes(self._handle)

    @property
    def sample_format(self):
        """rpf_sample_format: the engine's RPF_FORMAT_* value."""
        return self._lib.rpf_sample_format(self._handle)

    def max_hops_per_launch(self):
        return self._lib.rpf_max_hops_per_launch()

    def fused_status(self):
        """rpf_fused_status: is the fused four-step kernel what the next launch runs, how many of its launches gave
        up, how many of those the queue worker ran again on the two-kernel path."""
        active = ctypes.c_int()
        gave_up, recovered = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.rpf_fused_status(self._handle, ctypes.byref(active), ctypes.byref(gave_up),
                                               ctypes.byref(recovered)))
        return {"active": bool(active.value), "gave_up": gave_up.value, "recovered": recovered.value}

    def debug_fused_fault(self, mode, skip=0, count=-1):
        """rpf_debug_fused_fault (test hook)."""
        self._check(self._lib.rpf_debug_fused_fault(self._handle, mode, skip, count))

    def launch_info(self):
        vals = [ctypes.c_int() for _ in range(4)]
        self._check(self._lib.rpf_last_launch_info(self._handle, *[ctypes.byref(v) for v in vals]))
        return dict(zip(("grid", "block", "frames_per_wg", "lds_bytes"), (v.value for v in vals)))
