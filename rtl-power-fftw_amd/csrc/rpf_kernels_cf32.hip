// rpf_kernels_cf32.hip -- K1 (k1_kernels.h) for float32 I/Q (cf32), variant 0 of every K1 size: single, scan and
// strided kernels x {plain, windowed} x {LDS-DMA, VGPR staging}.  A translation unit of its own so that it compiles
// beside the others and no existing kernel is touched.
//
// cf32 stages 8 bytes per sample and unpacks with one 8-byte LDS read per point: no conversion, the stored pair is
// the sample (fft_core.h, phase_unpack).  The raw ring of a frame slot is RAWD x 8N bytes: one frame at N <= 256 (the
// bytes in flight of the other formats), two at 512 and 1024, and one again from 2048 on, where two no longer fit
// the CU's LDS beside the slab (k1_sizes.h, k1_size).
#include "k1_kernels.h"

namespace rpf {

const Variant* k1_cf32_variant(int N, int fmt)
{
    return fmt == kFmtCf32 ? find_default_variant<kK1Plain, kFmtCf32>(N) : nullptr;
}

}  // namespace rpf
