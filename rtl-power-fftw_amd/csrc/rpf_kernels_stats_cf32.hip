// rpf_kernels_stats_cf32.hip -- K1 with per-bin statistics (k1_kernels.h, kK1Stats) for float32 I/Q (cf32), variant 0
// of every K1 size: single and strided kernels x {plain, windowed} x {LDS-DMA, VGPR staging}.  A translation unit of
// its own, as rpf_kernels_cf32.hip: it compiles beside the others and no existing kernel is touched.
//
// Slab, ring and workgroup are the plain cf32 kernels'; what the statistics change is in k1_sizes.h (k1_size), and the
// windowed VGPR-staging forms read the window per frame instead of holding it (k1_body.inc, WREG).
#include "k1_kernels.h"

namespace rpf {

const Variant* k1_stats_cf32_variant(int N, int fmt)
{
    return fmt == kFmtCf32 ? find_default_variant<kK1Stats, kFmtCf32>(N) : nullptr;
}

}  // namespace rpf
