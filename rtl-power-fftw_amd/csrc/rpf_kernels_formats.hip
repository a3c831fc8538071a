// rpf_kernels_formats.hip -- K1 (k1_kernels.h) for the signed sample formats: signed 8-bit (cs8) and signed 16-bit
// little-endian (cs16) I/Q, variant 0 of every K1 size.  A translation unit of its own so that it compiles beside
// rpf_kernels.hip, which keeps the unsigned 8-bit instantiations and the launch code.
//
// cs8 is cu8 with another conversion: same staging, same LDS, same launch geometry.  cs16 stages 4 bytes per sample:
// the raw ring of a frame slot is RAWD x 4N bytes (k1_sizes.h, ring_depth).
#include "k1_kernels.h"

namespace rpf {

const Variant* k1_format_variant(int N, int fmt) { return find_signed_variant<kK1Plain>(N, fmt); }

}  // namespace rpf
