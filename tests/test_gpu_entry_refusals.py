"""What the engine's entry points answer when they refuse a call, on the MI355X: the return code and the text of
rpf_last_error(handle) for a table of calls through _lib on small engines, against tests/golden/entry_refusals.json
(tests/golden/make_entry_refusals.py recorded it there, from the build before the entries' refusals, inner engines and
piece loops were stated once).  Every call of CASES is refused before any launch; where two checks could fire an
`order_` case trips both, so the order of the checks is part of what is pinned.  Exact equality of code and text.

Each case is preceded by a refusal with a known text (PRIMER), so a case does not depend on the one before it and an
entry that returns without a message shows as such.  A misaligned pointer is a device pointer one sample-byte unit (or
8 bytes, for an output) past an aligned one; no refused call reads it.  `running=True` puts rpf_begin / rpf_finish
around the call.  The "kernel variant other than 0" refusals of the cross, STFT and correlator entries are not here:
rpf_engine_create refuses every variant but 0 in the product build, so no engine exists to make the call on.

OUT_CASES pins what lands in the out-parameters instead: for each entry with a `*_done` / `*times` out-parameter one
refused call and one call on a stream shorter than a frame (or, for the dedispersion, a plane without a time), the
out-parameter prefilled with SENTINEL and the output with 7.0, so that "not written" shows.  A record is [rc, what the
out-parameter holds, the number of leading zeros of the output, whether all the rest still holds 7.0]."""
import ctypes
import json
import os

import numpy as np
import pytest

from rtl_power_fftw_amd import _lib
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "entry_refusals.json")
SENTINEL = -777
FILL = 7.0
PRIMER = "rpf_stream_unregister: not a registered stream"
STORED_ROWS = 5                    # 2-frame integrations in the row store of the engine "stored"
MAX_HOPS = 16                      # rpf_max_hops_per_launch()

CU8, CS16, CF32, STATS = _lib.FORMAT_CU8, _lib.FORMAT_CS16, _lib.FORMAT_CF32, _lib.FLAG_BIN_STATS

# the engines, each created once per module: the smallest that can still go wrong
ENGINES = {
    "cu8": dict(N=64),                               # K1
    "cs16": dict(N=64, fmt=CS16),
    "cf32": dict(N=64, fmt=CF32),
    "stats": dict(N=64, flags=STATS),
    "pfb": dict(N=64, taps=2),
    "n1000": dict(N=1000, step=500),                 # not a power of two, not K1, overlapped frames
    "n1000_stats": dict(N=1000, flags=STATS),        # ... for the order of "power of two" and "not on a stats engine"
    "stored": dict(N=64),                            # STORED_ROWS rows appended to its quantile store
}


class Sym:
    """A pointer of the context by name, `off` bytes on: resolved when the call is made."""

    def __init__(self, kind, off=0):
        self.kind, self.off = kind, off

    def __add__(self, off):
        return Sym(self.kind, self.off + off)


D, D2, O = Sym("d"), Sym("d2"), Sym("o")            # device: two streams (256-byte aligned) and an output
HS, HO = Sym("hs"), Sym("ho")                       # host: a stream and an output of doubles
DELAYS, DELAYS_NEG, DELAYS_BIG = Sym("delays"), Sym("delays_neg"), Sym("delays_big")
WEIGHTS, WEIGHTS_NAN = Sym("weights"), Sym("weights_nan")
Q, Q_BAD, Q_NAN, STEPS = Sym("q"), Sym("q_bad"), Sym("q_nan"), Sym("steps")
FOUR = "four frames"                                # nbytes: rpf_frame_span(handle, 4)
SHORT = "short"                                     # nbytes: one sample less than a frame

_TYPED = {"ho": ctypes.c_double, "delays": ctypes.c_int32, "delays_neg": ctypes.c_int32, "delays_big": ctypes.c_int32,
          "weights": ctypes.c_double, "weights_nan": ctypes.c_double, "q": ctypes.c_double, "q_bad": ctypes.c_double,
          "q_nan": ctypes.c_double, "steps": ctypes.c_uint64}


class Context:
    def __init__(self):
        import torch
        self.torch = torch
        self.lib = _lib.load()
        dev = torch.device("cuda:0")
        self.t_in = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
        self.t_out = torch.zeros(1 << 13, dtype=torch.float64, device=dev)
        self.host = {
            "hs": np.zeros(1 << 16, np.uint8), "ho": np.zeros(1 << 13, np.float64),
            "delays": np.zeros(4 * 64, np.int32), "delays_neg": np.zeros(4 * 64, np.int32),
            "delays_big": np.full(4 * 64, 1000, np.int32),
            "weights": np.ones(64), "weights_nan": np.ones(64),
            "q": np.array([0.5, 0.25]), "q_bad": np.array([0.5, 1.5]), "q_nan": np.array([np.nan, 0.5]),
            "steps": np.full(8, 3 << 32, np.uint64),
        }
        self.host["delays_neg"][64 + 3] = -2                # trial 1, bin 3
        self.host["weights_nan"][5] = np.nan
        self.base = {"d": self.t_in.data_ptr(), "d2": self.t_in.data_ptr() + (1 << 15), "o": self.t_out.data_ptr()}
        assert self.base["d"] % 256 == 0 and self.base["o"] % 256 == 0
        for k, a in self.host.items():
            self.base[k] = a.ctypes.data
        self.handles = {}
        for name, cfg in ENGINES.items():
            self.handles[name] = self.create(**cfg)
        rows = np.random.default_rng(7).integers(0, 256, 2 * 64 * 2 * STORED_ROWS, dtype=np.uint8)
        done = ctypes.c_int64()
        assert self.lib.rpf_quantile_append(self.handles["stored"], rows.ctypes.data, rows.size, 2, 1 << 40, ctypes.byref(done)) == 0
        assert done.value == STORED_ROWS

    def create(self, N, fmt=CU8, flags=0, step=0, taps=0):
        cfg = _lib.rpf_config()
        cfg.struct_size = ctypes.sizeof(_lib.rpf_config)
        cfg.N, cfg.n_buffers, cfg.buffer_capacity, cfg.device = N, 2, 16384, 0
        cfg.flags = flags | _lib.FLAG_SAMPLE_FORMAT(fmt)
        cfg.frame_step = step
        handle = ctypes.c_void_p()
        if taps:
            coeffs = np.ones(taps * N, np.float32)
            rc = self.lib.rpf_engine_create_pfb(ctypes.byref(cfg), taps, coeffs.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                ctypes.byref(handle))
        else:
            rc = self.lib.rpf_engine_create(ctypes.byref(cfg), ctypes.byref(handle))
        assert rc == 0, self.lib.rpf_last_global_error().decode()
        return handle

    def close(self):
        self.torch.cuda.synchronize()
        for h in self.handles.values():
            self.lib.rpf_engine_destroy(h)
        self.handles = {}

    def r(self, v):
        """The argument a Sym stands for: an address, or a typed pointer where the binding wants one."""
        if not isinstance(v, Sym):
            return v
        addr = self.base[v.kind] + v.off
        return ctypes.cast(ctypes.c_void_p(addr), ctypes.POINTER(_TYPED[v.kind])) if v.kind in _TYPED else addr

    def n(self, h, nbytes):
        if nbytes == FOUR:
            return self.lib.rpf_frame_span(h, 4)
        if nbytes == SHORT:
            return self.lib.rpf_frame_span(h, 1) - self.lib.rpf_sample_bytes(h)
        return nbytes

    def ptrs(self, streams):
        return None if streams is None else (ctypes.c_void_p * len(streams))(*[self.r(s) for s in streams])


# ---- one adapter per entry (family): a call every check lets through unless an argument is overridden ----------------

def acc_dev(c, h, entry="rpf_accumulate_device", stream=D, nbytes=FOUR, repeats=4, out=O, done=None):
    return getattr(c.lib, entry)(h, c.r(stream), c.n(h, nbytes), repeats, c.r(out), None, done)


def cross_dev(c, h, a=D, b=D2, nbytes=FOUR, repeats=4, out=O, done=None):
    return c.lib.rpf_accumulate_device_cross(h, c.r(a), c.r(b), c.n(h, nbytes), repeats, c.r(out), None, done)


def cross_host(c, h, a=HS, b=HS, nbytes=FOUR, repeats=4, out=HO, done=None):
    return c.lib.rpf_accumulate_cross(h, c.r(a), c.r(b), c.n(h, nbytes), repeats, c.r(out), done)


def stft_dev(c, h, stream=D, nbytes=FOUR, max_frames=4, out=O, done=None):
    return c.lib.rpf_stft_device(h, c.r(stream), c.n(h, nbytes), max_frames, c.r(out), done, None)


def stft_host(c, h, stream=HS, nbytes=FOUR, max_frames=4, out=Sym("hs", 1 << 15), done=None):
    return c.lib.rpf_stft(h, c.r(stream), c.n(h, nbytes), max_frames, c.r(out), done)


def corr_dev(c, h, streams=(D, D2), n=None, nbytes=FOUR, repeats=4, out=O, done=None):
    n = (len(streams) if streams is not None else 2) if n is None else n
    return c.lib.rpf_correlate_device(h, c.ptrs(streams), n, c.n(h, nbytes), repeats, c.r(out), None, done)


def corr_host(c, h, streams=(HS, HS), n=None, nbytes=FOUR, repeats=4, out=HO, done=None):
    n = (len(streams) if streams is not None else 2) if n is None else n
    return c.lib.rpf_correlate(h, c.ptrs(streams), n, c.n(h, nbytes), repeats, c.r(out), done)


def fused(c, h, stream=D, nbytes=FOUR, repeats=4, done=None):
    return c.lib.rpf_device_fused(h, c.r(stream), c.n(h, nbytes), repeats, None, done)


def reduce(c, h, out=O):
    return c.lib.rpf_device_reduce(h, c.r(out), None)


def hops(c, h, entry="rpf_accumulate_device_hops", streams=(D, D2), nbytes=(FOUR, FOUR), repeats=(4, 4), n=None, out=O, done=None):
    n = (len(streams) if streams is not None else 2) if n is None else n
    nb = None if nbytes is None else (ctypes.c_size_t * len(nbytes))(*[c.n(h, b) for b in nbytes])
    rp = None if repeats is None else (ctypes.c_int64 * len(repeats))(*repeats)
    if entry == "rpf_accumulate_device_hops":
        return c.lib.rpf_accumulate_device_hops(h, c.ptrs(streams), nb, rp, n, c.r(out), None, done)
    return c.lib.rpf_device_fused_hops(h, c.ptrs(streams), nb, rp, n, None, done)


def series_dev(c, h, entry="rpf_accumulate_device_series", stream=D, nbytes=FOUR, L=2, max_spectra=2, out=O, done=None):
    return getattr(c.lib, entry)(h, c.r(stream), c.n(h, nbytes), L, max_spectra, c.r(out), None, done)


def series_host(c, h, entry="rpf_accumulate_series", stream=HS, nbytes=FOUR, L=2, max_spectra=2, out=HO, done=None):
    return getattr(c.lib, entry)(h, c.r(stream), c.n(h, nbytes), L, max_spectra, c.r(out), done)


def excised_dev(c, h, stream=D, nbytes=FOUR, L=2, max_spectra=2, lo=0.5, hi=1.5, out=O, done=None):
    return c.lib.rpf_accumulate_device_excised(h, c.r(stream), c.n(h, nbytes), L, max_spectra, lo, hi, c.r(out), None, None, done)


def excised_host(c, h, stream=HS, nbytes=FOUR, L=2, max_spectra=2, lo=0.5, hi=1.5, out=HO, done=None):
    return c.lib.rpf_accumulate_excised(h, c.r(stream), c.n(h, nbytes), L, max_spectra, lo, hi, c.r(out), None, done)


def q_append_dev(c, h, stream=D, nbytes=FOUR, L=2, max_spectra=2, done=None):
    return c.lib.rpf_quantile_append_device(h, c.r(stream), c.n(h, nbytes), L, max_spectra, None, done)


def q_append(c, h, stream=HS, nbytes=FOUR, L=2, max_spectra=2, done=None):
    return c.lib.rpf_quantile_append(h, c.r(stream), c.n(h, nbytes), L, max_spectra, done)


def q_select_dev(c, h, q=Q, nq=2, out=O):
    return c.lib.rpf_quantile_select_device(h, c.r(q), nq, c.r(out), None)


def q_select(c, h, q=Q, nq=2, out=HO):
    return c.lib.rpf_quantile_select(h, c.r(q), nq, c.r(out))


def dd_dev(c, h, delays=DELAYS, weights=WEIGHTS, n=2, out=O, capacity=1 << 20, times=True, done=None):
    t = done if done is not None else (ctypes.byref(ctypes.c_int64(SENTINEL)) if times else None)
    return c.lib.rpf_dedisperse_device(h, c.r(delays), c.r(weights), n, c.r(out), capacity, None, t)


def dd_host(c, h, delays=DELAYS, weights=WEIGHTS, n=2, out=HO, capacity=1 << 20, times=True, done=None):
    t = done if done is not None else (ctypes.byref(ctypes.c_int64(SENTINEL)) if times else None)
    return c.lib.rpf_dedisperse(h, c.r(delays), c.r(weights), n, c.r(out), capacity, t)


def dd_fold(c, h, delays=DELAYS, weights=WEIGHTS, n=2, steps=STEPS, P=2, NB=4, prof=HO, capacity=1 << 20, times=True, done=None):
    t = done if done is not None else (ctypes.byref(ctypes.c_int64(SENTINEL)) if times else None)
    return c.lib.rpf_dedisperse_fold(h, c.r(delays), c.r(weights), n, c.r(steps), P, NB, c.r(prof), capacity, None, None, t)


def fold_dev(c, h, series=D, n=2, T=16, steps=STEPS, P=2, NB=4, prof=O, capacity=1 << 40, hits=None, mom=None):
    return c.lib.rpf_fold_device(h, c.r(series), n, T, c.r(steps), P, NB, c.r(prof), capacity, c.r(hits), c.r(mom), None)


def register(c, h, stream=HS, nbytes=4096):
    return c.lib.rpf_stream_register(h, c.r(stream), nbytes)


def unregister(c, h, stream=HS):
    return c.lib.rpf_stream_unregister(h, c.r(stream))


def fused_fault(c, h, mode=0, skip=0, count=0):
    return c.lib.rpf_debug_fused_fault(h, mode, skip, count)


def begin(c, h, repeats=4):
    return c.lib.rpf_begin(h, repeats)


def finish(c, h):
    return c.lib.rpf_finish(h, None)


def accumulate(c, h, stream=HS, nbytes=FOUR, repeats=4):
    return c.lib.rpf_accumulate(h, c.r(stream), c.n(h, nbytes), repeats, None, None)


def get_power(c, h, out=HO):
    return c.lib.rpf_get_power(h, c.r(out))


def get_bin_stats(c, h):
    return c.lib.rpf_get_bin_stats(h, None, None)


def copy_power(c, h, out=O):
    return c.lib.rpf_copy_power_device(h, c.r(out), None, 0)


def submit(c, h, how="odd"):
    """rpf_buffer_submit of a buffer of the pool (acquired, and put back afterwards) or of a stranger."""
    if how == "stranger":
        return c.lib.rpf_buffer_submit(h, c.r(HS), 2)
    buf, cap = ctypes.c_void_p(), ctypes.c_size_t()
    assert c.lib.rpf_buffer_acquire(h, ctypes.byref(buf), ctypes.byref(cap)) == 0
    rc = c.lib.rpf_buffer_submit(h, buf, {"odd": 3, "too_large": cap.value + 2, "ragged": 6, "idle": 8, "odd_idle": 3}[how])
    text = c.lib.rpf_last_error(h)
    assert c.lib.rpf_buffer_unget(h, buf) == 0
    assert c.lib.rpf_last_error(h) == text
    return rc


def unget(c, h):
    return c.lib.rpf_buffer_unget(h, c.r(HS))


def acquire(c, h):
    return c.lib.rpf_buffer_acquire(h, None, None)


def C(engine, fn, running=False, **kw):
    return dict(engine=engine, fn=fn, running=running, kw=kw)


ACC, ACC_STATS = "rpf_accumulate_device", "rpf_accumulate_device_stats"
HOPS_FUSED = "rpf_device_fused_hops"
QFULL = 2 * 64 * 2 * ((1 << 21) - STORED_ROWS + 1)       # bytes of one 2-frame integration more than the store of N = 64 has room for

CASES = {
    # ---- rpf_accumulate_device ----
    "accumulate_device.null_out": C("cu8", acc_dev, out=None),
    "accumulate_device.null_stream": C("cu8", acc_dev, stream=None),
    "accumulate_device.running": C("cu8", acc_dev, running=True),
    "accumulate_device.negative_repeats": C("cu8", acc_dev, repeats=-1),
    "accumulate_device.stream_unaligned_cu8": C("cu8", acc_dev, stream=D + 1),
    "accumulate_device.stream_unaligned_cs16": C("cs16", acc_dev, stream=D + 2),
    "accumulate_device.stream_unaligned_cf32": C("cf32", acc_dev, stream=D + 4),
    "accumulate_device.out_unaligned": C("cu8", acc_dev, out=O + 8),
    "accumulate_device.order_null_then_running": C("cu8", acc_dev, out=None, running=True),
    "accumulate_device.order_running_then_repeats": C("cu8", acc_dev, repeats=-1, running=True),
    "accumulate_device.order_repeats_then_stream": C("cu8", acc_dev, repeats=-1, stream=D + 1),
    "accumulate_device.order_stream_then_out": C("cu8", acc_dev, stream=D + 1, out=O + 8),
    # ---- rpf_accumulate_device_stats ----
    "accumulate_device_stats.null_out": C("stats", acc_dev, entry=ACC_STATS, out=None),
    "accumulate_device_stats.without_stats": C("cu8", acc_dev, entry=ACC_STATS),
    "accumulate_device_stats.running": C("stats", acc_dev, entry=ACC_STATS, running=True),
    "accumulate_device_stats.negative_repeats": C("stats", acc_dev, entry=ACC_STATS, repeats=-1),
    "accumulate_device_stats.stream_unaligned": C("stats", acc_dev, entry=ACC_STATS, stream=D + 1),
    "accumulate_device_stats.out_unaligned": C("stats", acc_dev, entry=ACC_STATS, out=O + 8),
    "accumulate_device_stats.order_null_then_without_stats": C("cu8", acc_dev, entry=ACC_STATS, out=None),
    "accumulate_device_stats.order_without_stats_then_running": C("cu8", acc_dev, entry=ACC_STATS, running=True),
    "accumulate_device_stats.order_running_then_repeats": C("stats", acc_dev, entry=ACC_STATS, repeats=-1, running=True),
    "accumulate_device_stats.order_repeats_then_stream": C("stats", acc_dev, entry=ACC_STATS, repeats=-1, stream=D + 1),
    "accumulate_device_stats.order_stream_then_out": C("stats", acc_dev, entry=ACC_STATS, stream=D + 1, out=O + 8),
    # ---- rpf_accumulate_device_cross ----
    "cross_device.null_out": C("cu8", cross_dev, out=None),
    "cross_device.null_b": C("cu8", cross_dev, b=None),
    "cross_device.stats": C("stats", cross_dev),
    "cross_device.pfb": C("pfb", cross_dev),
    "cross_device.running": C("cu8", cross_dev, running=True),
    "cross_device.negative_repeats": C("cu8", cross_dev, repeats=-1),
    "cross_device.ragged_cu8": C("cu8", cross_dev, nbytes=511),
    "cross_device.ragged_cs16": C("cs16", cross_dev, nbytes=1022),
    "cross_device.a_unaligned": C("cu8", cross_dev, a=D + 1),
    "cross_device.b_unaligned_cf32": C("cf32", cross_dev, b=D2 + 4),
    "cross_device.out_unaligned": C("cu8", cross_dev, out=O + 8),
    "cross_device.order_null_then_stats": C("stats", cross_dev, out=None),
    "cross_device.order_null_then_pfb": C("pfb", cross_dev, a=None),
    "cross_device.order_stats_then_running": C("stats", cross_dev, running=True),
    "cross_device.order_pfb_then_running": C("pfb", cross_dev, running=True),
    "cross_device.order_running_then_repeats": C("cu8", cross_dev, repeats=-1, running=True),
    "cross_device.order_repeats_then_ragged": C("cu8", cross_dev, repeats=-1, nbytes=511),
    "cross_device.order_ragged_then_unaligned": C("cu8", cross_dev, nbytes=511, a=D + 1),
    "cross_device.order_unaligned_then_out": C("cu8", cross_dev, b=D2 + 1, out=O + 8),
    # ---- rpf_accumulate_cross ----
    "cross.null_out": C("cu8", cross_host, out=None),
    "cross.null_a": C("cu8", cross_host, a=None),
    "cross.stats": C("stats", cross_host),
    "cross.pfb": C("pfb", cross_host),
    "cross.running": C("cu8", cross_host, running=True),
    "cross.negative_repeats": C("cu8", cross_host, repeats=-1),
    "cross.ragged_cf32": C("cf32", cross_host, nbytes=2044),
    "cross.order_null_then_stats": C("stats", cross_host, out=None),
    "cross.order_stats_then_running": C("stats", cross_host, running=True),
    "cross.order_pfb_then_running": C("pfb", cross_host, running=True),
    "cross.order_running_then_repeats": C("cu8", cross_host, repeats=-1, running=True),
    "cross.order_repeats_then_ragged": C("cu8", cross_host, repeats=-1, nbytes=511),
    # ---- rpf_stft_device ----
    "stft_device.null_out": C("cu8", stft_dev, out=None),
    "stft_device.null_stream_of_no_bytes": C("cu8", stft_dev, stream=None, nbytes=0),
    "stft_device.not_a_power_of_two": C("n1000", stft_dev),
    "stft_device.stats": C("stats", stft_dev),
    "stft_device.running": C("cu8", stft_dev, running=True),
    "stft_device.negative_max_frames": C("cu8", stft_dev, max_frames=-1),
    "stft_device.ragged": C("cs16", stft_dev, nbytes=1022),
    "stft_device.stream_unaligned": C("cu8", stft_dev, stream=D + 1),
    "stft_device.out_unaligned": C("cu8", stft_dev, out=O + 8),
    "stft_device.order_null_then_power_of_two": C("n1000", stft_dev, out=None),
    "stft_device.order_power_of_two_then_stats": C("n1000_stats", stft_dev),
    "stft_device.order_stats_then_running": C("stats", stft_dev, running=True),
    "stft_device.order_running_then_max_frames": C("cu8", stft_dev, max_frames=-1, running=True),
    "stft_device.order_max_frames_then_ragged": C("cu8", stft_dev, max_frames=-1, nbytes=511),
    "stft_device.order_ragged_then_unaligned": C("cu8", stft_dev, nbytes=511, stream=D + 1),
    "stft_device.order_unaligned_then_out": C("cu8", stft_dev, stream=D + 1, out=O + 8),
    # ---- rpf_stft ----
    "stft.null_out": C("cu8", stft_host, out=None),
    "stft.null_stream": C("cu8", stft_host, stream=None),
    "stft.not_a_power_of_two": C("n1000", stft_host),
    "stft.stats": C("stats", stft_host),
    "stft.running": C("cu8", stft_host, running=True),
    "stft.negative_max_frames": C("cu8", stft_host, max_frames=-1),
    "stft.ragged": C("cu8", stft_host, nbytes=511),
    "stft.order_null_then_power_of_two": C("n1000", stft_host, stream=None),
    "stft.order_power_of_two_then_stats": C("n1000_stats", stft_host),
    "stft.order_stats_then_running": C("stats", stft_host, running=True),
    "stft.order_running_then_max_frames": C("cu8", stft_host, max_frames=-1, running=True),
    "stft.order_max_frames_then_ragged": C("cu8", stft_host, max_frames=-1, nbytes=511),
    # ---- rpf_correlate_device ----
    "correlate_device.null_streams": C("cu8", corr_dev, streams=None),
    "correlate_device.null_second_stream": C("cu8", corr_dev, streams=(D, None)),
    "correlate_device.null_out": C("cu8", corr_dev, out=None),
    "correlate_device.one_stream": C("cu8", corr_dev, streams=(D,)),
    "correlate_device.nine_streams": C("cu8", corr_dev, streams=(D,) * 9),
    "correlate_device.not_a_power_of_two": C("n1000", corr_dev),
    "correlate_device.stats": C("stats", corr_dev),
    "correlate_device.running": C("cu8", corr_dev, running=True),
    "correlate_device.negative_repeats": C("cu8", corr_dev, repeats=-1),
    "correlate_device.ragged": C("cs16", corr_dev, nbytes=1022),
    "correlate_device.second_stream_unaligned_cs16": C("cs16", corr_dev, streams=(D, D2 + 2)),
    "correlate_device.out_unaligned": C("cu8", corr_dev, out=O + 8),
    "correlate_device.order_null_then_n_streams": C("cu8", corr_dev, streams=(D,), out=None),
    "correlate_device.order_n_streams_then_power_of_two": C("n1000", corr_dev, streams=(D,)),
    "correlate_device.order_power_of_two_then_stats": C("n1000_stats", corr_dev),
    "correlate_device.order_stats_then_running": C("stats", corr_dev, running=True),
    "correlate_device.order_running_then_repeats": C("cu8", corr_dev, repeats=-1, running=True),
    "correlate_device.order_repeats_then_ragged": C("cu8", corr_dev, repeats=-1, nbytes=511),
    "correlate_device.order_ragged_then_unaligned": C("cu8", corr_dev, nbytes=511, streams=(D + 1, D2)),
    "correlate_device.order_unaligned_then_out": C("cu8", corr_dev, streams=(D, D2 + 1), out=O + 8),
    # ---- rpf_correlate ----
    "correlate.null_streams": C("cu8", corr_host, streams=None),
    "correlate.null_first_stream": C("cu8", corr_host, streams=(None, HS)),
    "correlate.null_out": C("cu8", corr_host, out=None),
    "correlate.one_stream": C("cu8", corr_host, streams=(HS,)),
    "correlate.nine_streams": C("cu8", corr_host, streams=(HS,) * 9),
    "correlate.not_a_power_of_two": C("n1000", corr_host),
    "correlate.stats": C("stats", corr_host),
    "correlate.running": C("cu8", corr_host, running=True),
    "correlate.negative_repeats": C("cu8", corr_host, repeats=-1),
    "correlate.ragged": C("cu8", corr_host, nbytes=511),
    "correlate.order_null_then_n_streams": C("cu8", corr_host, streams=(None,)),
    "correlate.order_n_streams_then_power_of_two": C("n1000", corr_host, streams=(HS,) * 9),
    "correlate.order_power_of_two_then_stats": C("n1000_stats", corr_host),
    "correlate.order_stats_then_running": C("stats", corr_host, running=True),
    "correlate.order_running_then_repeats": C("cu8", corr_host, repeats=-1, running=True),
    "correlate.order_repeats_then_ragged": C("cu8", corr_host, repeats=-1, nbytes=511),
    # ---- rpf_device_fused ----
    "device_fused.null_stream": C("cu8", fused, stream=None),
    "device_fused.pfb": C("pfb", fused),
    "device_fused.stats": C("stats", fused),
    "device_fused.running": C("cu8", fused, running=True),
    "device_fused.stream_unaligned": C("cu8", fused, stream=D + 1),
    "device_fused.overlapped_frames": C("n1000", fused),
    "device_fused.no_whole_frame": C("cu8", fused, nbytes=SHORT),
    "device_fused.negative_repeats": C("cu8", fused, repeats=-1),
    "device_fused.order_null_then_pfb": C("pfb", fused, stream=None),
    "device_fused.order_pfb_then_running": C("pfb", fused, running=True),
    "device_fused.order_stats_then_running": C("stats", fused, running=True),
    "device_fused.order_running_then_unaligned": C("cu8", fused, stream=D + 1, running=True),
    "device_fused.order_unaligned_then_overlapped": C("n1000", fused, stream=D + 1),
    "device_fused.order_overlapped_then_no_whole_frame": C("n1000", fused, nbytes=SHORT),
    # ---- rpf_device_reduce (nothing has been transformed on these engines) ----
    "device_reduce.null_out": C("cf32", reduce, out=None),
    "device_reduce.out_unaligned": C("cf32", reduce, out=O + 8),
    "device_reduce.stats": C("stats", reduce),
    "device_reduce.pfb": C("pfb", reduce),
    "device_reduce.nothing_to_reduce": C("cf32", reduce),
    "device_reduce.order_unaligned_then_stats": C("stats", reduce, out=O + 8),
    "device_reduce.order_unaligned_then_pfb": C("pfb", reduce, out=O + 8),
    # ---- rpf_accumulate_device_hops ----
    "device_hops.null_streams": C("cu8", hops, streams=None),
    "device_hops.null_nbytes": C("cu8", hops, nbytes=None),
    "device_hops.null_repeats": C("cu8", hops, repeats=None),
    "device_hops.no_hop": C("cu8", hops, n=0),
    "device_hops.running": C("cu8", hops, running=True),
    "device_hops.negative_repeats_of_hop_1": C("cu8", hops, repeats=(4, -1)),
    "device_hops.null_stream_of_hop_1": C("cu8", hops, streams=(D, None)),
    "device_hops.stream_unaligned_of_hop_1": C("cu8", hops, streams=(D, D2 + 1)),
    "device_hops.null_out": C("cu8", hops, out=None),
    "device_hops.out_unaligned": C("cu8", hops, out=O + 8),
    "device_hops.order_no_hop_then_running": C("cu8", hops, n=0, running=True),
    "device_hops.order_running_then_repeats": C("cu8", hops, repeats=(-1, 4), running=True),
    "device_hops.order_repeats_then_null_stream": C("cu8", hops, repeats=(-1, 4), streams=(None, D2)),
    "device_hops.order_null_stream_then_unaligned_next_hop": C("cu8", hops, streams=(None, D2 + 1)),
    "device_hops.order_unaligned_hop_0_then_repeats_hop_1": C("cu8", hops, streams=(D + 1, D2), repeats=(4, -1)),
    "device_hops.order_unaligned_then_null_out": C("cu8", hops, streams=(D, D2 + 1), out=None),
    # ---- rpf_device_fused_hops ----
    "fused_hops.null_streams": C("cu8", hops, entry=HOPS_FUSED, streams=None),
    "fused_hops.no_hop": C("cu8", hops, entry=HOPS_FUSED, n=-1),
    "fused_hops.running": C("cu8", hops, entry=HOPS_FUSED, running=True),
    "fused_hops.negative_repeats": C("cu8", hops, entry=HOPS_FUSED, repeats=(-1, 4)),
    "fused_hops.null_stream": C("cu8", hops, entry=HOPS_FUSED, streams=(None, D2)),
    "fused_hops.stream_unaligned_cs16": C("cs16", hops, entry=HOPS_FUSED, streams=(D + 2, D2)),
    "fused_hops.stats": C("stats", hops, entry=HOPS_FUSED),
    "fused_hops.pfb": C("pfb", hops, entry=HOPS_FUSED),
    "fused_hops.not_k1": C("n1000", hops, entry=HOPS_FUSED),
    "fused_hops.too_many_hops": C("cu8", hops, entry=HOPS_FUSED, streams=(D,) * (MAX_HOPS + 1), nbytes=(FOUR,) * (MAX_HOPS + 1),
                                  repeats=(4,) * (MAX_HOPS + 1)),
    "fused_hops.order_running_then_repeats": C("cu8", hops, entry=HOPS_FUSED, repeats=(4, -1), running=True),
    "fused_hops.order_unaligned_then_stats": C("stats", hops, entry=HOPS_FUSED, streams=(D, D2 + 1)),
    "fused_hops.order_unaligned_then_pfb": C("pfb", hops, entry=HOPS_FUSED, streams=(D + 1, D2)),
    "fused_hops.order_pfb_then_not_k1": C("pfb", hops, entry=HOPS_FUSED, streams=(D,) * (MAX_HOPS + 1), nbytes=(FOUR,) * (MAX_HOPS + 1),
                                          repeats=(4,) * (MAX_HOPS + 1)),
    "fused_hops.order_stats_then_not_k1": C("n1000_stats", hops, entry=HOPS_FUSED),
    # ---- rpf_fold_device (no refusal of its own asks what the engine is) ----
    "fold_device.null_series": C("cu8", fold_dev, series=None),
    "fold_device.running": C("cu8", fold_dev, running=True),
    "fold_device.null_steps": C("cu8", fold_dev, steps=None),
    "fold_device.null_prof": C("cu8", fold_dev, prof=None),
    "fold_device.no_series": C("cu8", fold_dev, n=0),
    "fold_device.too_many_series": C("cu8", fold_dev, n=4097),
    "fold_device.no_period": C("cu8", fold_dev, P=0),
    "fold_device.too_many_periods": C("cu8", fold_dev, P=4097),
    "fold_device.no_phase_bin": C("cu8", fold_dev, NB=0),
    "fold_device.too_many_phase_bins": C("cu8", fold_dev, NB=129),
    "fold_device.negative_T": C("cu8", fold_dev, T=-1),
    "fold_device.T_of_2_to_the_31": C("cu8", fold_dev, T=1 << 31),
    "fold_device.cells_above_capacity": C("cu8", fold_dev, capacity=15),
    "fold_device.cells_above_a_call": C("cu8", fold_dev, n=4096, P=4096, NB=2),
    "fold_device.series_unaligned": C("cu8", fold_dev, series=D + 4),
    "fold_device.prof_unaligned": C("cu8", fold_dev, prof=O + 8),
    "fold_device.mom_unaligned": C("cu8", fold_dev, mom=O + 4104),
    "fold_device.hits_unaligned": C("cu8", fold_dev, hits=O + 4098),
    "fold_device.order_null_then_running": C("cu8", fold_dev, series=None, running=True),
    "fold_device.order_running_then_null_steps": C("cu8", fold_dev, steps=None, running=True),
    "fold_device.order_null_steps_then_series": C("cu8", fold_dev, steps=None, n=0),
    "fold_device.order_series_then_periods": C("cu8", fold_dev, n=4097, P=0),
    "fold_device.order_periods_then_phase_bins": C("cu8", fold_dev, P=4097, NB=0),
    "fold_device.order_phase_bins_then_T": C("cu8", fold_dev, NB=129, T=-1),
    "fold_device.order_T_then_cells": C("cu8", fold_dev, T=-1, capacity=15),
    "fold_device.order_cells_then_series_unaligned": C("cu8", fold_dev, capacity=15, series=D + 4),
    "fold_device.order_series_unaligned_then_prof": C("cu8", fold_dev, series=D + 4, prof=O + 8),
    "fold_device.order_prof_then_hits": C("cu8", fold_dev, prof=O + 8, hits=O + 4098),
    # ---- rpf_stream_register, rpf_stream_unregister, rpf_debug_fused_fault ----
    "stream_register.null_stream": C("cu8", register, stream=None),
    "stream_register.empty_stream": C("cu8", register, nbytes=0),
    "stream_register.running": C("cu8", register, running=True),
    "stream_register.order_empty_then_running": C("cu8", register, nbytes=0, running=True),
    "stream_unregister.null_stream": C("cu8", unregister, stream=None),
    "stream_unregister.running": C("cu8", unregister, running=True),
    "stream_unregister.not_registered": C("cu8", unregister, stream=Sym("hs", 64)),
    "stream_unregister.order_null_then_running": C("cu8", unregister, stream=None, running=True),
    "debug_fused_fault.bad_mode": C("cu8", fused_fault, mode=3),
    "debug_fused_fault.negative_skip": C("cu8", fused_fault, skip=-1),
    "debug_fused_fault.running": C("cu8", fused_fault, running=True),
    "debug_fused_fault.order_bad_mode_then_running": C("cu8", fused_fault, mode=-1, running=True),
    # ---- the queue entries and the getters ----
    "begin.already_running": C("cu8", begin, running=True),
    "begin.negative_repeats": C("cu8", begin, repeats=-1),
    "begin.order_running_then_repeats": C("cu8", begin, repeats=-1, running=True),
    "finish.not_running": C("cu8", finish),
    "accumulate.null_stream": C("cu8", accumulate, stream=None),
    "accumulate.already_running": C("cu8", accumulate, running=True),
    "accumulate.negative_repeats": C("cu8", accumulate, repeats=-1),
    "buffer_acquire.null_buf": C("cu8", acquire),
    "buffer_submit.not_an_engine_buffer": C("cu8", submit, how="stranger", running=True),
    "buffer_submit.odd_size": C("cu8", submit, how="odd", running=True),
    "buffer_submit.above_capacity": C("cu8", submit, how="too_large", running=True),
    "buffer_submit.ragged_cf32": C("cf32", submit, how="ragged", running=True),
    "buffer_submit.not_running": C("cu8", submit, how="idle"),
    "buffer_submit.order_size_then_not_running": C("cu8", submit, how="odd_idle"),
    "buffer_unget.not_an_engine_buffer": C("cu8", unget),
    "get_power.null_out": C("cu8", get_power, out=None),
    "get_power.running": C("cu8", get_power, running=True),
    "get_bin_stats.without_stats": C("cu8", get_bin_stats),
    "get_bin_stats.running": C("stats", get_bin_stats, running=True),
    "get_bin_stats.order_without_stats_then_running": C("cu8", get_bin_stats, running=True),
    "copy_power_device.null_out": C("cu8", copy_power, out=None),
    "copy_power_device.running": C("cu8", copy_power, running=True),
}


def _series_cases(prefix, fn, plain, with_stats, device):
    """The refusals of series_check and series_begin for the plain entry and the one with statistics."""
    for tag, entry, own, other in ((prefix, plain, "cu8", "stats"), (prefix + "_stats", with_stats, "stats", "cu8")):
        k = dict(entry=entry)
        CASES.update({
            tag + ".null_out": C(own, fn, out=None, **k),
            tag + ".null_stream": C(own, fn, stream=None, **k),
            tag + ".pfb": C("pfb", fn, **k),
            tag + ".wrong_kind_of_engine": C(other, fn, **k),
            tag + ".running": C(own, fn, running=True, **k),
            tag + ".no_frame_per_spectrum": C(own, fn, L=0, **k),
            tag + ".negative_max_spectra": C(own, fn, max_spectra=-1, **k),
            tag + ".order_null_then_pfb": C("pfb", fn, out=None, **k),
            tag + ".order_pfb_then_running": C("pfb", fn, running=True, **k),
            tag + ".order_wrong_kind_then_running": C(other, fn, running=True, **k),
            tag + ".order_running_then_frames_per_spectrum": C(own, fn, L=0, running=True, **k),
            tag + ".order_frames_per_spectrum_then_max_spectra": C(own, fn, L=-3, max_spectra=-1, **k),
        })
        if device:
            CASES.update({
                tag + ".stream_unaligned": C(own, fn, stream=D + 1, **k),
                tag + ".out_unaligned": C(own, fn, out=O + 8, **k),
                tag + ".order_max_spectra_then_unaligned": C(own, fn, max_spectra=-1, stream=D + 1, **k),
                tag + ".order_stream_then_out": C(own, fn, stream=D + 1, out=O + 8, **k),
            })
    # a PFB engine has no statistics either: the entry with statistics trips both
    CASES[prefix + "_stats.order_pfb_then_without_stats"] = C("pfb", fn, entry=with_stats)


_series_cases("device_series", series_dev, "rpf_accumulate_device_series", "rpf_accumulate_device_series_stats", True)
_series_cases("series", series_host, "rpf_accumulate_series", "rpf_accumulate_series_stats", False)


def _excised_cases(tag, fn, device):
    CASES.update({
        tag + ".null_out": C("stats", fn, out=None),
        tag + ".pfb": C("pfb", fn),
        tag + ".without_stats": C("cu8", fn),
        tag + ".running": C("stats", fn, running=True),
        tag + ".no_frame_per_spectrum": C("stats", fn, L=0),
        tag + ".negative_max_spectra": C("stats", fn, max_spectra=-1),
        tag + ".one_frame_per_spectrum": C("stats", fn, L=1),
        tag + ".threshold_nan": C("stats", fn, hi=float("nan")),
        tag + ".thresholds_crossed": C("stats", fn, lo=1.5, hi=0.5),
        tag + ".order_without_stats_then_running": C("cu8", fn, running=True),
        tag + ".order_max_spectra_then_one_frame": C("stats", fn, max_spectra=-1, L=1),
        tag + ".order_one_frame_then_nan": C("stats", fn, L=1, lo=float("nan")),
    })
    if device:
        CASES.update({
            tag + ".stream_unaligned": C("stats", fn, stream=D + 1),
            tag + ".out_unaligned": C("stats", fn, out=O + 8),
            tag + ".order_thresholds_then_unaligned": C("stats", fn, lo=1.5, hi=0.5, stream=D + 1),
            tag + ".order_stream_then_out": C("stats", fn, stream=D + 1, out=O + 8),
        })


_excised_cases("device_excised", excised_dev, True)
_excised_cases("excised", excised_host, False)


def _quantile_cases():
    for tag, fn, device in (("quantile_append_device", q_append_dev, True), ("quantile_append", q_append, False)):
        CASES.update({
            tag + ".pfb": C("pfb", fn),
            tag + ".stats": C("stats", fn),
            tag + ".running": C("stored", fn, running=True),
            tag + ".null_stream": C("stored", fn, stream=None),
            tag + ".no_frame_per_spectrum": C("stored", fn, L=0),
            tag + ".negative_max_spectra": C("stored", fn, max_spectra=-1),
            tag + ".store_full": C("stored", fn, nbytes=QFULL, max_spectra=1 << 40),
            tag + ".store_full_from_empty": C("cu8", fn, nbytes=QFULL + 2 * 64 * 2 * STORED_ROWS, max_spectra=1 << 40),
            tag + ".order_pfb_then_running": C("pfb", fn, running=True),
            tag + ".order_stats_then_running": C("stats", fn, running=True),
            tag + ".order_running_then_null": C("stored", fn, stream=None, running=True),
            tag + ".order_null_then_frames_per_spectrum": C("stored", fn, stream=None, L=0),
            tag + ".order_frames_per_spectrum_then_max_spectra": C("stored", fn, L=0, max_spectra=-1),
        })
        if device:
            CASES.update({
                tag + ".stream_unaligned": C("stored", fn, stream=D + 1),
                tag + ".order_store_full_then_unaligned": C("stored", fn, nbytes=QFULL, max_spectra=1 << 40, stream=D + 1),
            })
    for tag, fn, device in (("quantile_select_device", q_select_dev, True), ("quantile_select", q_select, False)):
        CASES.update({
            tag + ".pfb": C("pfb", fn),
            tag + ".stats": C("stats", fn),
            tag + ".running": C("stored", fn, running=True),
            tag + ".no_quantile": C("stored", fn, nq=0),
            tag + ".nine_quantiles": C("stored", fn, nq=9),
            tag + ".null_q": C("stored", fn, q=None),
            tag + ".null_out": C("stored", fn, out=None),
            tag + ".q_above_one": C("stored", fn, q=Q_BAD),
            tag + ".q_nan": C("stored", fn, q=Q_NAN),
            tag + ".order_running_then_nq": C("stored", fn, nq=0, running=True),
            tag + ".order_nq_then_null": C("stored", fn, nq=9, q=None),
            tag + ".order_null_out_then_q": C("stored", fn, out=None, q=Q_BAD),
        })
        if device:
            CASES.update({
                tag + ".out_unaligned": C("stored", fn, out=O + 8),
                tag + ".order_q_then_unaligned": C("stored", fn, q=Q_BAD, out=O + 8),
            })


_quantile_cases()


def _dedisperse_cases():
    for tag, fn, out in (("dedisperse_device", dd_dev, "out"), ("dedisperse", dd_host, "out"), ("dedisperse_fold", dd_fold, "prof")):
        CASES.update({
            tag + ".pfb": C("pfb", fn),
            tag + ".stats": C("stats", fn),
            tag + ".running": C("stored", fn, running=True),
            tag + ".null_delays": C("stored", fn, delays=None),
            tag + ".null_out": C("stored", fn, **{out: None}),
            tag + ".null_times": C("stored", fn, times=False),
            tag + ".no_trial": C("stored", fn, n=0),
            tag + ".too_many_trials": C("stored", fn, n=4097),
            tag + ".negative_delay": C("stored", fn, delays=DELAYS_NEG),
            tag + ".weight_not_finite": C("stored", fn, weights=WEIGHTS_NAN),
            tag + ".order_pfb_then_null": C("pfb", fn, delays=None),
            tag + ".order_running_then_null": C("stored", fn, delays=None, running=True),
            tag + ".order_null_then_trials": C("stored", fn, n=0, **{out: None}),
            tag + ".order_trials_then_negative_delay": C("stored", fn, n=4097, delays=DELAYS_NEG),
            tag + ".order_negative_delay_then_weights": C("stored", fn, delays=DELAYS_NEG, weights=WEIGHTS_NAN),
        })
    for tag, fn in (("dedisperse_device", dd_dev), ("dedisperse", dd_host)):
        CASES.update({
            tag + ".capacity": C("stored", fn, capacity=2 * STORED_ROWS - 1),
            tag + ".order_weights_then_capacity": C("stored", fn, weights=WEIGHTS_NAN, capacity=2 * STORED_ROWS - 1),
        })
    CASES.update({
        "dedisperse_device.out_unaligned": C("stored", dd_dev, out=O + 8),
        "dedisperse_device.order_capacity_then_unaligned": C("stored", dd_dev, capacity=2 * STORED_ROWS - 1, out=O + 8),
        "dedisperse_fold.null_steps": C("stored", dd_fold, steps=None),
        "dedisperse_fold.no_period": C("stored", dd_fold, P=0),
        "dedisperse_fold.too_many_periods": C("stored", dd_fold, P=4097),
        "dedisperse_fold.no_phase_bin": C("stored", dd_fold, NB=0),
        "dedisperse_fold.too_many_phase_bins": C("stored", dd_fold, NB=129),
        "dedisperse_fold.cells_above_capacity": C("stored", dd_fold, capacity=15),
        "dedisperse_fold.order_weights_then_null_steps": C("stored", dd_fold, weights=WEIGHTS_NAN, steps=None),
        "dedisperse_fold.order_null_steps_then_periods": C("stored", dd_fold, steps=None, P=0),
        "dedisperse_fold.order_periods_then_phase_bins": C("stored", dd_fold, P=4097, NB=0),
        "dedisperse_fold.order_phase_bins_then_cells": C("stored", dd_fold, NB=129, capacity=15),
    })


_dedisperse_cases()


def OUT(engine, fn, output=None, hops=0, **kw):
    return dict(engine=engine, fn=fn, output=output, hops=hops, kw=kw)


def _out_cases():
    cases = {}

    def pair(tag, engine, fn, output, refused, zero, hops=0):
        cases[tag + ".refused"] = OUT(engine, fn, output, hops, **refused)
        cases[tag + ".no_whole_frame"] = OUT(engine, fn, output, hops, **zero)

    short = dict(nbytes=SHORT)
    pair("accumulate_device", "cu8", acc_dev, "o", dict(out=O + 8), short)
    pair("accumulate_device_stats", "stats", acc_dev, "o", dict(entry=ACC_STATS, out=O + 8), dict(entry=ACC_STATS, nbytes=SHORT))
    pair("cross_device", "cu8", cross_dev, "o", dict(out=O + 8), short)
    pair("cross", "cu8", cross_host, "ho", dict(nbytes=511), short)
    pair("stft_device", "cu8", stft_dev, "o", dict(out=O + 8), short)
    pair("stft", "cu8", stft_host, None, dict(nbytes=511), short)
    pair("correlate_device", "cu8", corr_dev, "o", dict(out=O + 8), short)
    pair("correlate", "cu8", corr_host, "ho", dict(nbytes=511), short)
    pair("device_fused", "cu8", fused, None, dict(stream=D + 1), short)
    # (the hop entries leave their mark on the engine's last launch: on an engine of their own kind, not the one
    # device_reduce's "nothing to reduce" is asked of)
    pair("device_hops", "cs16", hops, "o", dict(out=O + 8), dict(nbytes=(SHORT, SHORT)), hops=2)
    pair("fused_hops", "cs16", hops, None, dict(entry=HOPS_FUSED, streams=(D, D2 + 2)), dict(entry=HOPS_FUSED, nbytes=(SHORT, SHORT)),
         hops=2)
    for tag, fn, output, k in (("device_series", series_dev, "o", {}), ("series", series_host, "ho", {}),
                               ("device_series_stats", series_dev, "o", dict(entry="rpf_accumulate_device_series_stats")),
                               ("series_stats", series_host, "ho", dict(entry="rpf_accumulate_series_stats"))):
        pair(tag, "stats" if "stats" in tag else "cu8", fn, output, dict(max_spectra=-1, **k), dict(nbytes=SHORT, **k))
    pair("device_excised", "stats", excised_dev, "o", dict(out=O + 8), short)
    pair("excised", "stats", excised_host, "ho", dict(lo=1.5, hi=0.5), short)
    pair("quantile_append_device", "stored", q_append_dev, None, dict(stream=D + 1), short)
    pair("quantile_append", "stored", q_append, None, dict(max_spectra=-1), short)
    for tag, fn, output, refused in (("dedisperse_device", dd_dev, "o", dict(out=O + 8)),
                                     ("dedisperse", dd_host, "ho", dict(capacity=2 * STORED_ROWS - 1)),
                                     ("dedisperse_fold", dd_fold, "ho", dict(capacity=15))):
        cases[tag + ".refused"] = OUT("stored", fn, output, **refused)
        cases[tag + ".no_time"] = OUT("stored", fn, output, delays=DELAYS_BIG)
        cases[tag + ".no_row"] = OUT("cu8", fn, output)
    return cases


OUT_CASES = _out_cases()


def answer(c, name):
    """[rc, rpf_last_error(handle)] of case `name`."""
    case = CASES[name]
    h = c.handles[case["engine"]]
    assert c.lib.rpf_stream_unregister(h, c.r(Sym("hs", 128))) == 3 and c.lib.rpf_last_error(h).decode() == PRIMER
    if case["running"]:
        assert c.lib.rpf_begin(h, 4) == 0
    try:
        rc = case["fn"](c, h, **case["kw"])
        text = c.lib.rpf_last_error(h).decode()
    finally:
        if case["running"]:
            assert c.lib.rpf_finish(h, None) == 0
    return [rc, text]


def out_answer(c, name):
    """[rc, out-parameter, leading zeros of the output, the rest untouched] of out-parameter case `name`."""
    case = OUT_CASES[name]
    h = c.handles[case["engine"]]
    done = (ctypes.c_int64 * max(case["hops"], 1))(*[SENTINEL] * max(case["hops"], 1))
    c.t_out.fill_(FILL)
    c.host["ho"][:] = FILL
    c.torch.cuda.synchronize()
    rc = case["fn"](c, h, done=done, **case["kw"])
    c.torch.cuda.synchronize()
    record = [rc, list(done) if case["hops"] else done[0]]
    if case["output"]:
        out = c.t_out.cpu().numpy() if case["output"] == "o" else c.host["ho"]
        zeros = int(np.argmax(out != 0.0)) if (out != 0.0).any() else out.size
        record += [zeros, bool(np.all(out[zeros:] == FILL))]
    return record


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def context():
    c = Context()
    yield c
    c.close()


def test_fixture_covers_the_cases(recorded):
    assert sorted(recorded["refusals"]) == sorted(CASES)
    for name, (rc, text) in recorded["refusals"].items():
        assert rc == 3, name                                 # RPF_ERR_INVALID_ARGUMENT
        assert text, name
    assert sorted(recorded["out_parameters"]) == sorted(OUT_CASES)
    for name, record in recorded["out_parameters"].items():
        # (rpf_device_fused has no launch to make without a frame: it refuses that call too)
        assert record[0] == (3 if name.endswith(".refused") or name == "device_fused.no_whole_frame" else 0), name
        assert len(record) == 2 or record[3], name           # whatever was written is a run of zeros from the front


@pytest.mark.parametrize("name", list(CASES))
def test_refusal_answers_as_recorded(context, recorded, name):
    assert answer(context, name) == recorded["refusals"][name]


@pytest.mark.parametrize("name", list(OUT_CASES))
def test_out_parameters_as_recorded(context, recorded, name):
    assert out_answer(context, name) == recorded["out_parameters"][name]
