// rpf_kernels_series_stats_cf32.hip -- K1 for a uniform series of per-bin statistics on float32 I/Q (cf32):
// fft_accum_series_stats_kernel (k1_kernels.h, k1_scan_body.inc under STATS) for variant 0 of every K1 size x {plain,
// windowed} x {LDS-DMA, VGPR staging}.  A translation unit of its own, so that the kernels of
// rpf_kernels_series_stats.hip stay what they are; that unit's finder, plan, launch and format-free fix-up kernel
// serve these kernels too (k1_series_stats_variant asks here for cf32).
#include "k1_kernels.h"

namespace rpf {

const Variant* k1_series_stats_cf32_variant(int N, int fmt)
{
    return fmt == kFmtCf32 ? find_default_variant<kK1SeriesStats, kFmtCf32>(N) : nullptr;
}

}  // namespace rpf
