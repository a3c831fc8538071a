"""What the engine's entry points answer to a NULL engine handle, before any device is touched: the return code and the
text of rpf_last_global_error(), against tests/golden/entry_refusals_null.json (tests/golden/make_entry_refusals.py
recorded it from the build before the entries' refusals were stated once).  Every entry of rpf_engine.cpp tests the
handle before it reads it, so every one that returns a code is here.  An entry that returns without a message leaves the
text of the call before it: each case is preceded by a refusal with a known text (PRIMER), and the fixture then holds
that text.  The correlator and dedispersion entries write their out-parameter before the checks; the case says what
landed in it.  Exact equality of code, text and out-parameter."""
import ctypes
import json
import os

import pytest

from rtl_power_fftw_amd import _lib
from helpers import GOLDEN

FIXTURE = os.path.join(GOLDEN, "entry_refusals_null.json")
SENTINEL = -777
PRIMER = "rpf_stream_unregister: NULL argument"


def _i64():
    return ctypes.c_int64(SENTINEL)


def _with_done(call):
    """The case's rc and what the call left in an int64 out-parameter that held SENTINEL."""
    def run(lib):
        done = _i64()
        return call(lib, ctypes.byref(done)), done.value
    return run


def _plain(call):
    return lambda lib: (call(lib), None)


# name -> lib -> (rc, out-parameter or None); every pointer but the handle is NULL too: the handle is tested first
CASES = {
    "rpf_begin": _plain(lambda lib: lib.rpf_begin(None, 1)),
    "rpf_buffer_acquire": _plain(lambda lib: lib.rpf_buffer_acquire(None, None, None)),
    "rpf_buffer_submit": _plain(lambda lib: lib.rpf_buffer_submit(None, None, 0)),
    "rpf_buffer_unget": _plain(lambda lib: lib.rpf_buffer_unget(None, None)),
    "rpf_finish": _with_done(lambda lib, d: lib.rpf_finish(None, d)),
    "rpf_get_power": _plain(lambda lib: lib.rpf_get_power(None, None)),
    "rpf_get_bin_stats": _plain(lambda lib: lib.rpf_get_bin_stats(None, None, None)),
    "rpf_copy_power_device": _plain(lambda lib: lib.rpf_copy_power_device(None, None, None, 0)),
    "rpf_get_histogram": _plain(lambda lib: lib.rpf_get_histogram(None, None)),
    "rpf_accumulate": _with_done(lambda lib, d: lib.rpf_accumulate(None, None, 0, 1, None, d)),
    "rpf_accumulate_device": _with_done(lambda lib, d: lib.rpf_accumulate_device(None, None, 0, 1, None, None, d)),
    "rpf_accumulate_device_stats": _with_done(lambda lib, d: lib.rpf_accumulate_device_stats(None, None, 0, 1, None, None, d)),
    "rpf_accumulate_device_cross": _with_done(lambda lib, d: lib.rpf_accumulate_device_cross(None, None, None, 0, 1, None, None, d)),
    "rpf_accumulate_cross": _with_done(lambda lib, d: lib.rpf_accumulate_cross(None, None, None, 0, 1, None, d)),
    "rpf_stft_device": _with_done(lambda lib, d: lib.rpf_stft_device(None, None, 0, 1, None, d, None)),
    "rpf_stft": _with_done(lambda lib, d: lib.rpf_stft(None, None, 0, 1, None, d)),
    "rpf_correlate_device": _with_done(lambda lib, d: lib.rpf_correlate_device(None, None, 2, 0, 1, None, None, d)),
    "rpf_correlate": _with_done(lambda lib, d: lib.rpf_correlate(None, None, 2, 0, 1, None, d)),
    "rpf_device_fused": _with_done(lambda lib, d: lib.rpf_device_fused(None, None, 0, 1, None, d)),
    "rpf_device_reduce": _plain(lambda lib: lib.rpf_device_reduce(None, None, None)),
    "rpf_accumulate_device_hops": _with_done(lambda lib, d: lib.rpf_accumulate_device_hops(None, None, None, None, 1, None, None, d)),
    "rpf_device_fused_hops": _with_done(lambda lib, d: lib.rpf_device_fused_hops(None, None, None, None, 1, None, d)),
    "rpf_accumulate_device_series": _with_done(lambda lib, d: lib.rpf_accumulate_device_series(None, None, 0, 1, 1, None, None, d)),
    "rpf_accumulate_device_series_stats": _with_done(
        lambda lib, d: lib.rpf_accumulate_device_series_stats(None, None, 0, 1, 1, None, None, d)),
    "rpf_accumulate_series": _with_done(lambda lib, d: lib.rpf_accumulate_series(None, None, 0, 1, 1, None, d)),
    "rpf_accumulate_series_stats": _with_done(lambda lib, d: lib.rpf_accumulate_series_stats(None, None, 0, 1, 1, None, d)),
    "rpf_accumulate_device_excised": _with_done(
        lambda lib, d: lib.rpf_accumulate_device_excised(None, None, 0, 2, 1, 0.5, 1.5, None, None, None, d)),
    "rpf_accumulate_excised": _with_done(lambda lib, d: lib.rpf_accumulate_excised(None, None, 0, 2, 1, 0.5, 1.5, None, None, d)),
    "rpf_quantile_reset": _plain(lambda lib: lib.rpf_quantile_reset(None)),
    "rpf_quantile_append_device": _with_done(lambda lib, d: lib.rpf_quantile_append_device(None, None, 0, 1, 1, None, d)),
    "rpf_quantile_append": _with_done(lambda lib, d: lib.rpf_quantile_append(None, None, 0, 1, 1, d)),
    "rpf_quantile_select_device": _plain(lambda lib: lib.rpf_quantile_select_device(None, None, 1, None, None)),
    "rpf_quantile_select": _plain(lambda lib: lib.rpf_quantile_select(None, None, 1, None)),
    "rpf_dedisperse_device": _with_done(lambda lib, d: lib.rpf_dedisperse_device(None, None, None, 1, None, 0, None, d)),
    "rpf_dedisperse": _with_done(lambda lib, d: lib.rpf_dedisperse(None, None, None, 1, None, 0, d)),
    "rpf_dedisperse_fold": _with_done(lambda lib, d: lib.rpf_dedisperse_fold(None, None, None, 1, None, 1, 1, None, 0, None, None, d)),
    "rpf_fold_device": _plain(lambda lib: lib.rpf_fold_device(None, None, 1, 1, None, 1, 1, None, 0, None, None, None)),
    "rpf_stream_register": _plain(lambda lib: lib.rpf_stream_register(None, None, 0)),
    "rpf_stream_unregister": _plain(lambda lib: lib.rpf_stream_unregister(None, None)),
    "rpf_fused_status": _plain(lambda lib: lib.rpf_fused_status(None, None, None, None)),
    "rpf_debug_fused_fault": _plain(lambda lib: lib.rpf_debug_fused_fault(None, 0, 0, 0)),
    "rpf_last_launch_info": _plain(lambda lib: lib.rpf_last_launch_info(None, None, None, None, None)),
}


def answer(name):
    """[rc, rpf_last_global_error(), out-parameter] of case `name`, after a refusal that leaves PRIMER as the text."""
    lib = _lib.load()
    assert lib.rpf_stream_unregister(None, None) == 3 and lib.rpf_last_global_error().decode() == PRIMER
    rc, done = CASES[name](lib)
    return [rc, lib.rpf_last_global_error().decode(), done]


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_the_cases(recorded):
    assert sorted(recorded) == sorted(CASES)
    for name, (rc, text, done) in recorded.items():
        assert rc == 3, name                                             # RPF_ERR_INVALID_ARGUMENT
        assert text == PRIMER or text.startswith(name + ": "), name      # its own message, or none at all
        assert done in (None, 0, SENTINEL), name


@pytest.mark.parametrize("name", list(CASES))
def test_null_handle_answers_as_recorded(recorded, name):
    assert answer(name) == recorded[name]
