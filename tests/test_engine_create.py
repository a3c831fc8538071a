"""What rpf_engine_create and rpf_engine_create_pfb answer before any device is touched: the return code and the text of
rpf_last_global_error() for a list of configurations, against tests/golden/engine_create_errors.json
(tests/golden/make_engine_create_errors.py recorded it, on a machine without a GPU, from the build before
create_engine was taken apart).  A bad configuration gives its message; a good one gives "No HIP device available ...
no CPU path" there, which says that every check passed before the device was asked for.  Where two checks could fire the
list holds a configuration that trips both: the order of the checks is part of what callers see.  Exact equality of
code and text; with a GPU present the good rows are skipped (they would create engines) and the bad ones still hold."""
import ctypes
import json
import os

import numpy as np
import pytest

from rtl_power_fftw_amd import _lib
from helpers import GOLDEN

FIXTURE = os.path.join(GOLDEN, "engine_create_errors.json")
NO_DEVICE = "No HIP device available"

CU8, CS8, CS16, CF32 = _lib.FORMAT_CU8, _lib.FORMAT_CS8, _lib.FORMAT_CS16, _lib.FORMAT_CF32
FUSED, NO_MIXED, CATCH_ALL, STATS = (_lib.FLAG_FOURSTEP_FUSED, _lib.FLAG_NO_MIXED_RADIX, _lib.FLAG_CATCH_ALL,
                                     _lib.FLAG_BIN_STATS)


def VARIANT(k):
    return k << 8


def case(N=4096, step=0, fmt=CU8, flags=0, buffers=5, capacity=16384, size="full", window=False, taps=None, coeffs=True,
         device=0):
    return dict(N=N, step=step, fmt=fmt, flags=flags, buffers=buffers, capacity=capacity, size=size, window=window,
                taps=taps, coeffs=coeffs, device=device)


CASES = {
    # ---- configurations every check lets through ----
    "good_4096": case(),
    "good_short_struct": case(size="short"),
    "good_short_struct_ignores_the_step_field": case(size="short", step=-7),
    "good_step_1": case(step=1),
    "good_step_n": case(step=4096),
    "good_cs16": case(fmt=CS16, capacity=16384),
    "good_cf32_stats_1000": case(N=1000, fmt=CF32, flags=STATS),
    "good_windowed_32768": case(N=32768, window=True),
    "good_two_to_the_26": case(N=1 << 26),
    "good_8388606": case(N=8388606),
    "good_fused_16384": case(N=16384, flags=FUSED),
    "good_device_ordinal_is_asked_after_the_count": case(device=-1),
    "good_pfb_512": case(N=512, taps=4),
    "good_pfb_32_taps": case(N=512, taps=32),
    "good_pfb_catch_all_only_size": case(N=1000, taps=4),
    "good_pfb_taps_x_bins_at_the_limit": case(N=1 << 21, taps=32),
    # ---- one check each ----
    "struct_size_bad": case(size=7),
    "n_odd": case(N=4095),
    "n_zero": case(N=0),
    "n_one": case(N=1),
    "n_negative": case(N=-4096),
    "n_10000000": case(N=10000000),
    "n_two_to_the_27": case(N=1 << 27),
    "step_negative": case(step=-1),
    "step_above_n": case(step=4097),
    "format_3": case(fmt=3),
    "format_5": case(fmt=5),
    "stats_with_fused": case(N=16384, flags=STATS | FUSED),
    "stats_with_variant_1": case(flags=STATS | VARIANT(1)),
    "variant_1_at_4096": case(flags=VARIANT(1)),           # (the product build has variant 0 only)
    "variant_200_at_4096": case(flags=VARIANT(200)),
    "catch_all_with_variant_1": case(flags=CATCH_ALL | VARIANT(1)),
    "cs8_with_variant_1_at_4096": case(fmt=CS8, flags=VARIANT(1)),
    "buffers_zero": case(buffers=0),
    "capacity_odd": case(capacity=16383),
    "capacity_zero": case(capacity=0),
    "capacity_not_whole_cs16_samples": case(fmt=CS16, capacity=16382),
    "capacity_not_whole_cf32_samples": case(fmt=CF32, capacity=16388),
    "pfb_taps_0": case(N=512, taps=0),
    "pfb_taps_33": case(N=512, taps=33),
    "pfb_taps_x_bins_too_many": case(N=1 << 22, taps=32),
    "pfb_null_coeffs": case(N=512, taps=4, coeffs=False),
    "pfb_window": case(N=512, taps=4, window=True),
    "pfb_step": case(N=512, taps=4, step=256),
    "pfb_stats": case(N=512, taps=4, flags=STATS),
    "pfb_fused": case(N=16384, taps=4, flags=FUSED),
    "pfb_variant_1": case(N=512, taps=4, flags=VARIANT(1)),
    "pfb_size_nobody_serves": case(N=10000000, taps=4),
    # ---- two checks at once: the earlier one answers ----
    "order_struct_size_then_n": case(size=7, N=4095),
    "order_n_then_step": case(N=4095, step=-1),
    "order_step_then_format": case(step=4097, fmt=3),
    "order_format_then_stats_fused": case(fmt=3, flags=STATS | FUSED),
    "order_stats_fused_then_stats_variant": case(flags=STATS | FUSED | VARIANT(1)),
    "order_stats_variant_then_pfb_taps": case(N=512, taps=0, flags=STATS | VARIANT(1)),
    "order_stats_fused_then_pfb_stats": case(N=512, taps=4, flags=STATS | FUSED),
    "order_pfb_taps_then_product": case(N=1 << 22, taps=33),
    "order_pfb_product_then_coeffs": case(N=1 << 22, taps=32, coeffs=False),
    "order_pfb_coeffs_then_window": case(N=512, taps=4, coeffs=False, window=True),
    "order_pfb_window_then_step": case(N=512, taps=4, window=True, step=256),
    "order_pfb_step_then_stats": case(N=512, taps=4, step=256, flags=STATS),
    "order_pfb_fused_then_variant": case(N=512, taps=4, flags=FUSED | VARIANT(1)),
    "order_pfb_variant_then_no_kernel": case(N=10000000, taps=4, flags=VARIANT(1)),
    "order_no_kernel_then_buffers": case(N=10000000, buffers=0),
    "order_pfb_no_kernel_then_buffers": case(N=10000000, taps=4, buffers=0),
    "order_buffers_then_capacity": case(buffers=0, capacity=16383),
    "order_capacity_even_then_sample_size": case(fmt=CS16, capacity=16383),
}


def create(c):
    """(return code, rpf_last_global_error()) of the create call of configuration `c`; destroys what it made."""
    lib = _lib.load()
    cfg = _lib.rpf_config()
    cfg.struct_size = {"full": ctypes.sizeof(_lib.rpf_config), "short": _lib.CONFIG_SIZE_V2_0}.get(c["size"], c["size"])
    cfg.N = c["N"]
    window = np.ones(max(c["N"], 1), dtype=np.float32) if c["window"] else None
    if window is not None:
        cfg.window = window.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    cfg.n_buffers = c["buffers"]
    cfg.buffer_capacity = c["capacity"]
    cfg.device = c["device"]
    cfg.flags = c["flags"] | _lib.FLAG_SAMPLE_FORMAT(c["fmt"])
    cfg.frame_step = c["step"]
    handle = ctypes.c_void_p()
    if c["taps"] is None:
        rc = lib.rpf_engine_create(ctypes.byref(cfg), ctypes.byref(handle))
    else:
        # (no check reads the coefficients; a configuration that passes them all is not created where there is a device)
        coeffs = np.zeros(max(1, min(c["taps"] * max(c["N"], 0), 1 << 16)), dtype=np.float32) if c["coeffs"] else None
        rc = lib.rpf_engine_create_pfb(ctypes.byref(cfg), c["taps"],
                                       None if coeffs is None else coeffs.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                       ctypes.byref(handle))
    text = lib.rpf_last_global_error().decode() if rc != 0 else ""
    if handle:
        lib.rpf_engine_destroy(handle)
    return rc, text


def have_gpu():
    try:
        import torch
    except ImportError:
        return False
    return torch.cuda.is_available()


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_the_cases(recorded):
    assert sorted(recorded) == sorted(CASES)
    for name, (rc, text) in recorded.items():
        # a good row is one that got as far as the device, and the names say which they are
        assert name.startswith("good_") == text.startswith(NO_DEVICE), name
        assert rc == (7 if name.startswith("good_") else 3), name       # RPF_ERR_HARDWARE / RPF_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", list(CASES))
def test_create_answers_as_recorded(recorded, name):
    if name.startswith("good_") and have_gpu():
        pytest.skip("a configuration every check lets through: with a device present it is an engine, not an answer")
    assert list(create(CASES[name])) == recorded[name]
