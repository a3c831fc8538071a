// rpf_kernels_stft_formats.hip -- K1's store kernels (rpf_kernels_stft.hip) for the signed sample formats, cs8 and cs16.
#include "k1_kernels.h"

namespace rpf {

const Variant* k1_stft_format_variant(int N, int fmt) { return find_signed_variant<kK1Stft>(N, fmt); }

}  // namespace rpf
