// rpf_kernels_stats_formats.hip -- K1 with per-bin statistics (k1_kernels.h, kK1Stats) for the signed sample formats,
// cs8 and cs16; compiled beside rpf_kernels_stats.hip.
#include "k1_kernels.h"

namespace rpf {

const Variant* k1_stats_format_variant(int N, int fmt) { return find_signed_variant<kK1Stats>(N, fmt); }

}  // namespace rpf
