// rpf_kernels_stft_cf32.hip -- K1's store kernels (rpf_kernels_stft.hip) for float32 I/Q (cf32): the ring depths of the
// plain cf32 kernels (k1_sizes.h, k1_size).
#include "k1_kernels.h"

namespace rpf {

const Variant* k1_stft_cf32_variant(int N, int fmt)
{
    return fmt == kFmtCf32 ? find_default_variant<kK1Stft, kFmtCf32>(N) : nullptr;
}

}  // namespace rpf
