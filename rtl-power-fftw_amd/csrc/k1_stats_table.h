// k1_stats_table.h -- K1 (k1_kernels.h) with per-bin statistics (RPF_FLAG_BIN_STATS): the table of one sample
// format, shared by the two translation units that instantiate it (rpf_kernels_stats.hip: unsigned 8-bit;
// rpf_kernels_stats_formats.hip: signed 8- and 16-bit) so that they compile side by side.
//
// Three double accumulators per bin are 6 P registers (96 at P = 16) beside the frame, the twiddles and the window:
// the sizes whose plain twins run at three waves per SIMD (168 registers) take two here (256), and no instantiation
// spills (profiles/spectral_stats_resources.txt): windowed 512 takes three waves instead of four, and windowed 8192,
// whose 512-thread workgroup cannot have more than 256 registers per lane, reads the twiddles of passes 2 and 3 from an
// LDS table (TWLDSW; 4 KB more LDS for both window forms of that size).  Geometry, slab and ring are the plain kernels'.
#pragma once

#include "k1_kernels.h"

namespace rpf {

namespace {

// variant 0 of one size: the single-acquisition and the strided kernel (a scan of a stats engine runs hop by hop)
template <int N, int P, int OCC, int OCCW, int RAWD, bool TWLDS, bool TWLDSW, int WGO, int FMT>
Variant make_stats_variant()
{
    using G = Geom<N, P>;
    constexpr int WG = WGO ? WGO : (G::T >= 256 ? G::T : 256);
    constexpr int FPW = WG / G::T;
    constexpr int LDS = FPW * (G::LDS_CPX * (int)sizeof(cf) + RAWD * sample_bytes_of(FMT) * N) +
                        ((TWLDS || TWLDSW) ? twlds_entries<G>() * (int)sizeof(cf) : 0);
    return Variant{N, 0, P, WG, FPW, LDS, false,
                   {{fft_accum_kernel<G, WG, OCC, false, false, false, 0, false, RAWD, 0, TWLDS, FMT, true>,
                     fft_accum_kernel<G, WG, OCC, false, true, false, 0, false, RAWD, 0, TWLDS, FMT, true>},
                    {fft_accum_kernel<G, WG, OCCW, true, false, false, 0, false, RAWD, 0, TWLDSW, FMT, true>,
                     fft_accum_kernel<G, WG, OCCW, true, true, false, 0, false, RAWD, 0, TWLDSW, FMT, true>}},
                   {{nullptr, nullptr}, {nullptr, nullptr}},
                   {{fft_accum_strided_kernel<G, WG, OCC, false, false, false, 0, false, RAWD, 0, TWLDS, FMT, true>,
                     fft_accum_strided_kernel<G, WG, OCC, false, true, false, 0, false, RAWD, 0, TWLDS, FMT, true>},
                    {fft_accum_strided_kernel<G, WG, OCCW, true, false, false, 0, false, RAWD, 0, TWLDSW, FMT, true>,
                     fft_accum_strided_kernel<G, WG, OCCW, true, true, false, 0, false, RAWD, 0, TWLDSW, FMT, true>}}};
}

template <int FMT>
const Variant* find_in_stats_table(int N)
{
    constexpr int R = FMT == kFmtCs16 ? 2 : 4;     // ring depth of the three smallest sizes (rpf_kernels_formats.hip)
    // Template arguments after <N, P>: OCC, OCCW (windowed), RAWD, TWLDS, TWLDSW (windowed), WGO, FMT
    static const Variant table[] = {
        make_stats_variant<64, 8, 4, 4, R, false, false, 0, FMT>(),
        make_stats_variant<128, 16, 2, 2, R, false, false, 0, FMT>(),
        make_stats_variant<256, 16, 2, 2, R, false, false, 0, FMT>(),
        make_stats_variant<512, 8, 4, 3, 2, false, false, 0, FMT>(),
        make_stats_variant<1024, 16, 2, 2, 2, true, true, 0, FMT>(),
        make_stats_variant<2048, 16, 2, 2, 2, true, true, 512, FMT>(),
        make_stats_variant<4096, 16, 2, 2, 2, true, true, 512, FMT>(),
        make_stats_variant<8192, 16, 2, 2, 2, false, true, 0, FMT>(),
    };
    for (const Variant& v : table)
        if (v.N == N) return &v;
    return nullptr;
}

}  // namespace

}  // namespace rpf
