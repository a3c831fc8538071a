// k1_sizes.h -- K1's per-size geometry, stated once.  Every translation unit that instantiates K1 kernels
// (rpf_kernels.hip, rpf_kernels_formats.hip, rpf_kernels_cf32.hip, rpf_kernels_stats*.hip, rpf_kernels_series*.hip)
// builds its table of variant 0 from this list (k1_kernels.h, find_default_variant); only the tuning build's
// experiments (k1_tuning.inc) name geometries of their own.
#pragma once

#include "fft_core.h"
#include "rpf_device_common.h"

namespace rpf {

// P      points per lane: a frame is owned by T = N / P threads
// OCC    waves per SIMD the register budget must admit (= resident workgroups per CU x WG / 256); OCCW: windowed kernels
// RAWD   depth of the raw-byte ring = iterations staged ahead (k1_kernels.h); kRingSmall: by sample format, below
// TWLDS  the twiddles of the passes after the first in an LDS table instead of registers; TWLDSW: windowed kernels
//        (k1_size sets it: TWLDS, but for one statistics kernel)
// WGO    workgroup size; 0 = max(T, 256).  A larger one runs more frames side by side.
// LDW    loader waves launched behind the WGO threads (k1_loader.h): the single-acquisition kernel that stages by
//        LDS-DMA without a window takes them, every other kernel of the row has none (k1_size sets it)
struct K1Size {
    int N, P, OCC, OCCW, RAWD;
    bool TWLDS;
    int WGO;
    bool TWLDSW = false;
    int LDW = 0;
};

constexpr int kRingSmall = 0;

constexpr K1Size kK1Sizes[] = {
    //  N   P  OCC OCCW  RAWD      TWLDS  WGO
    {64, 8, 4, 4, kRingSmall, false, 0},
    // 128 = 16 x 8 and 256 = 16 x 16: two passes and ONE exchange at 16 points per lane (measured
    // 12-14 % faster than 8 x 8 x 2 / 8 x 8 x 4 -- the LDS stores are what costs)
    {128, 16, 3, 3, kRingSmall, false, 0},
    {256, 16, 3, 3, kRingSmall, false, 0},
    {512, 8, 4, 4, 2, false, 0},
    {1024, 16, 3, 2, 2, true, 0},
    // 2048/4096: one 512-thread workgroup per CU (4 / 2 frames side by side): as fast as three
    // 256-thread workgroups (the kernel is VALU-bound at 8 waves) and a third of the partials.
    {2048, 16, 2, 2, 2, true, 512},
    {4096, 16, 2, 2, 2, true, 512},
    {8192, 16, 2, 2, 2, false, 0},
};
constexpr int kK1SizeCount = sizeof(kK1Sizes) / sizeof(kK1Sizes[0]);

// What the host needs to launch a K1-shaped kernel: workgroup size, frames side by side in it, dynamic LDS.
// WG counts the threads that own frames; `launched` is what the launch asks for, WG + 64 per loader wave (with_loader:
// the geometry of a variant's one entry that has them).
struct K1Geometry {
    int WG, fpw, lds_bytes;
    int launched;
    constexpr K1Geometry with_loader(int ldw) const { return K1Geometry{WG, fpw, lds_bytes, WG + 64 * ldw}; }
};

// The workgroup size and the LDS of its frame slots (slabs and raw ring, all but the twiddle table) from plain values,
// so that k1_size can ask at a run-time row index whether a ring fits.
constexpr int k1_workgroup(int n, int p, int wgo) { return wgo ? wgo : (n / p >= 256 ? n / p : 256); }
constexpr int k1_slots_lds(int n, int p, int wgo, int slabs, int rawd, int fmt)
{
    return k1_workgroup(n, p, wgo) / (n / p) *
           (slabs * (n + n / p) * static_cast<int>(sizeof(cf)) + rawd * sample_bytes_of(fmt) * n);
}
// G: the frame's Geom; wgo: K1Size::WGO; per frame slot `slabs` exchange slabs (1 in every kernel; the host builds of
// tests/emul state it too) and a raw ring of `rawd` frames of format `fmt` (0: no ring, the Bluestein kernel);
// twtable: the LDS twiddle table, one per workgroup.  The kernels index LDS by the same compile-time quantities
// (k1_body.inc).
template <class G>
constexpr K1Geometry k1_geometry(int wgo, int slabs, int rawd, int fmt, bool twtable)
{
    static_assert(G::T == G::N / G::P && G::LDS_CPX == G::N + G::N / G::P, "k1_slots_lds states the slab of Geom");
    const int wg = k1_workgroup(G::N, G::P, wgo);
    return K1Geometry{wg, wg / G::T,
                      k1_slots_lds(G::N, G::P, wgo, slabs, rawd, fmt) +
                          (twtable ? twlds_entries<G>() * static_cast<int>(sizeof(cf)) : 0),
                      wg};
}

// kRingSmall, the tiny frames of N <= 256: four frames in flight with 2-byte samples, two with cs16's 4-byte samples,
// one with cf32's 8-byte samples -- the same bytes in flight and the same LDS, so the same occupancy.  Everywhere else
// every format keeps two where they fit (cf32: below), and cs16's LDS grows by 4N per frame slot (N = 8192: 68 KB slab
// + 64 KB ring of the CU's 160 KB, one workgroup per CU as with cu8).
constexpr int ring_depth(int rawd, int fmt)
{
    return rawd != kRingSmall ? rawd : fmt == kFmtCf32 ? 1 : fmt == kFmtCs16 ? 2 : 4;
}

constexpr int kLdsPerCU = 160 * 1024;
// RPF_K1_LOADER_WAVES (A/B builds, `make kvariant KFLAGS=-DRPF_K1_LOADER_WAVES=1`): the loader waves of the 4096 row.
// Two, one per frame slot: with one, its sixteen pieces per iteration were the new critical path and the gain stayed
// inside the run-to-run range; none is the kernel before the loader (profiles/k1_loader.json).
#ifndef RPF_K1_LOADER_WAVES
#define RPF_K1_LOADER_WAVES 2
#endif
constexpr int kLoaderWaves4096 = RPF_K1_LOADER_WAVES;

// Row i as the kernels of sample format `fmt` take it; stats: the kernels with per-bin statistics
// (RPF_FLAG_BIN_STATS), which depart from the table where the registers run out.  Three double accumulators per bin
// are 6 P registers (96 at P = 16) beside the frame, the twiddles and the window: the sizes whose plain twins run at
// three waves per SIMD (168 registers) take two here (256), and no instantiation spills
// (profiles/spectral_stats_resources.txt): windowed 512 takes three waves instead of four, and windowed 8192, whose
// 512-thread workgroup cannot have more than 256 registers per lane, reads the twiddles of passes 2 and 3 from an LDS
// table (4 KB more LDS for both window forms of that size).  Slab, ring and workgroup are the plain kernels'.
// The series kernels with statistics (rpf_kernels_series_stats.hip) take the same departures and need no further one:
// 102 .. 134 registers at P = 8, 208 .. 252 of 256 at P = 16, no scratch (profiles/series_stats_resources.txt).
// cf32 departs where a workgroup with a two-deep ring of 8-byte samples is more than the CU's 160 KB of LDS: 2048 and
// 4096 (200 KB + the twiddle table) and 8192 (200 KB); 512 (50 KB) and 1024 (102 KB) keep two.  Those three sizes
// take a ring of depth 1, refilled behind the unpack: the same kernel body with RAWD = 1 -- the counted wait at the
// top of the frame loop is vmcnt(0), the refill of the one slot is issued as soon as the unpack's LDS reads have
// returned and has the frame's transform to land in (132 KB + table at 2048 and 4096, 132 KB at 8192).
// cf32 also gives up the third wave per SIMD where three did not compile without scratch: the windowed kernels of 128
// and 256 and the plain ones of 1024 take two (256 registers).  None of them had a third workgroup's LDS on the CU
// to begin with (66 KB, 66 KB and 102 KB per workgroup), so no resident workgroup is lost
// (profiles/cf32_resources.txt).
// cf32 with statistics departs twice more, for the VGPR-staging forms, whose eight 16-byte loads in flight meet the
// three double accumulators per bin: 8192 reads the twiddles of passes 2 and 3 from the LDS table in its plain form
// as well (4 KB more: 136 KB of 160), and windowed 1024 takes one wave per SIMD -- its 102 KB of LDS admit one
// workgroup per CU whatever the registers say, so no resident workgroup is lost and the compiler may use 512
// registers.  The windowed VGPR-staging forms also stop holding the window across the frame (k1_body.inc, WREG).  No
// instantiation spills (profiles/cf32_stats_resources.txt).
constexpr K1Size k1_size(int i, int fmt, bool stats)
{
    K1Size s = kK1Sizes[i];
    s.RAWD = ring_depth(s.RAWD, fmt);
    // (slabs and ring alone decide it: where two frames fit, the twiddle table does too -- default_variant checks)
    if (fmt == kFmtCf32 && s.RAWD > 1 && k1_slots_lds(s.N, s.P, s.WGO, 1, s.RAWD, fmt) > kLdsPerCU) s.RAWD = 1;
    if (fmt == kFmtCf32 && (s.N == 128 || s.N == 256)) s.OCCW = 2;
    if (fmt == kFmtCf32 && s.N == 1024) s.OCC = 2;
    s.TWLDSW = s.TWLDS;
    // The loader wave: measured at 4096 with cu8 alone (profiles/k1_loader.json); every other row, format and kernel
    // keeps the LDS-DMA in its compute waves.
    s.LDW = (s.N == 4096 && fmt == kFmtCu8 && !stats) ? kLoaderWaves4096 : 0;
    if (stats) {
        if (s.N == 128 || s.N == 256 || s.N == 1024) s.OCC = s.OCCW = 2;
        if (s.N == 512) s.OCCW = 3;
        if (s.N == 8192) s.TWLDSW = true;
        if (fmt == kFmtCf32 && s.N == 8192) s.TWLDS = true;
        if (fmt == kFmtCf32 && s.N == 1024) s.OCCW = 1;
    }
    return s;
}

}  // namespace rpf
