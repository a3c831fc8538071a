// rpf_kernels_stats_formats.hip -- K1 with per-bin statistics (k1_stats_table.h) for the signed sample formats,
// cs8 and cs16; compiled beside rpf_kernels_stats.hip.
#include "k1_stats_table.h"

namespace rpf {

const Variant* find_stats_format_variant(int N, int fmt)
{
    return fmt == kFmtCs8 ? find_in_stats_table<kFmtCs8>(N) : fmt == kFmtCs16 ? find_in_stats_table<kFmtCs16>(N) : nullptr;
}

}  // namespace rpf
