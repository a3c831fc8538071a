"""cf32 with per-bin statistics on K1: everything that needs no GPU -- the rows of k1_size(i, cf32, true) as k1_sizes.h
states them (compiled for the host, tests/emul/cf32_stats_emul.cpp): every row's LDS fits the CU, slab, ring and
workgroup are the plain cf32 kernels', what differs is the stated list and nothing else; and the recorded resource
listing of the new kernels.  geometry() is what tests/test_gpu_cf32_stats.py compares launch_info() with."""
import ast
import ctypes
import functools
import os
import re

from helpers import ROOT

K1_SIZES = [64, 128, 256, 512, 1024, 2048, 4096, 8192]
FIELDS = ("N", "P", "OCC", "OCCW", "RAWD", "TWLDS", "TWLDSW", "WGO", "WG", "fpw", "lds_bytes", "slab_bytes")

# Where a row of the cf32 kernels with statistics may differ from the plain cf32 row (k1_sizes.h, k1_size): the waves
# per SIMD the statistics kernels of every format give up (128, 256: two; windowed 512: three), windowed 1024's one wave,
# and 8192's LDS twiddle table in both window forms, which is 4080 bytes of LDS.
DEPARTURES = {
    128: {"OCC": 2},
    256: {"OCC": 2},
    512: {"OCCW": 3},
    1024: {"OCCW": 1},
    8192: {"TWLDS": 1, "TWLDSW": 1, "lds_bytes": 135168 + 4080},
}


@functools.lru_cache(maxsize=1)
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "librpf_emul_cf32_stats.so"))
    lib.rpf_emul_cf32_stats_row.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    return lib


def row(i, stats):
    out = (ctypes.c_int * len(FIELDS))()
    assert emul().rpf_emul_cf32_stats_row(i, 1 if stats else 0, out) == 0
    return dict(zip(FIELDS, out))


def geometry():
    """{(N, windowed): (WG, fpw, lds_bytes)} of the sixteen size x window forms of the cf32 kernels with statistics; the
    two window forms of a size share one launch geometry."""
    out = {}
    for i in range(emul().rpf_emul_cf32_stats_rows()):
        r = row(i, True)
        for window in (False, True):
            out[(r["N"], window)] = (r["WG"], r["fpw"], r["lds_bytes"])
    return out


def test_the_rows_are_the_size_table():
    lib = emul()
    assert lib.rpf_emul_cf32_stats_rows() == len(K1_SIZES)
    assert [row(i, True)["N"] for i in range(len(K1_SIZES))] == K1_SIZES
    out = (ctypes.c_int * len(FIELDS))()
    assert lib.rpf_emul_cf32_stats_row(len(K1_SIZES), 1, out) == -1


def test_every_row_fits_the_cu():
    cu = emul().rpf_emul_cf32_stats_lds_per_cu()
    assert cu == 160 * 1024
    for i in range(len(K1_SIZES)):
        r = row(i, True)
        assert 0 < r["lds_bytes"] <= cu, r
        # the LDS is the frame slots' slabs and rings, and the twiddle table where a window form has one
        slots = r["fpw"] * (r["slab_bytes"] + r["RAWD"] * 8 * r["N"])
        assert r["lds_bytes"] >= slots and (r["lds_bytes"] == slots) == (not (r["TWLDS"] or r["TWLDSW"])), r


def test_slab_ring_and_workgroup_are_the_plain_rows_and_only_the_stated_departures_differ():
    for i, N in enumerate(K1_SIZES):
        plain, st = row(i, False), row(i, True)
        for k in ("N", "P", "RAWD", "WGO", "WG", "fpw", "slab_bytes"):
            assert st[k] == plain[k], (N, k)
        differ = {k: st[k] for k in FIELDS if st[k] != plain[k]}
        assert differ == DEPARTURES.get(N, {}), (N, differ)


def test_geometry_has_sixteen_forms():
    g = geometry()
    assert sorted(g) == sorted((N, w) for N in K1_SIZES for w in (False, True))
    assert g[(512, False)] == (256, 4, 51200) and g[(8192, True)] == (512, 1, 139248)


def test_recorded_resources_every_kernel_without_scratch():
    """profiles/cf32_stats_resources.txt (make resources on the two new units): single and strided statistics kernels
    and the series kernel with statistics, each x 8 sizes x {plain, windowed} x {LDS-DMA, VGPR staging} = 96 kernels,
    none with scratch or spilled registers, none above the 256 registers a 512-thread workgroup can have."""
    lines = [l for l in open(os.path.join(ROOT, "profiles", "cf32_stats_resources.txt")).read().splitlines() if l.strip()]
    assert len(lines) == 3 * len(K1_SIZES) * 2 * 2 == 96
    forms = {}
    for l in lines:
        m = re.match(r"N=(\d+) P=(\d+) WG=(\d+) OCC=(\d+) win=([01]) dma=([01]) dbuf=0 (\{.*\})$", l)
        assert m, l
        N, P, WG, OCC, win, dma = (int(v) for v in m.groups()[:6])
        res = ast.literal_eval(m.group(7))
        assert res["ScratchSize"] == "0" and res["VGPRs Spill"] == "0", l
        assert int(res["VGPRs"]) + int(res["AGPRs"]) <= (256 if WG == 512 else 512), l
        forms[(N, win, dma)] = forms.get((N, win, dma), 0) + 1
        r = row(K1_SIZES.index(N), True)
        assert (P, WG, OCC) == (r["P"], r["WG"], r["OCCW"] if win else r["OCC"]), l
    assert forms == {(N, w, d): 3 for N in K1_SIZES for w in (0, 1) for d in (0, 1)}
