// rpf_kernels_formats.hip -- K1 (k1_kernels.h) for the signed sample formats: signed 8-bit (cs8) and signed 16-bit
// little-endian (cs16) I/Q, variant 0 of every K1 size.  A translation unit of its own so that it compiles beside
// rpf_kernels.hip, which keeps the unsigned 8-bit instantiations and the launch code.
//
// cs8 is cu8 with another conversion: same staging, same LDS, same launch geometry.  cs16 stages 4 bytes per sample:
// the raw ring of a frame slot is RAWD x 4N bytes.  Where cu8 keeps four frames in flight (N <= 256, tiny frames) cs16
// keeps two -- the same bytes in flight and the same LDS, so the same occupancy --; everywhere else both keep two, and
// the workgroup's LDS grows by 4N per frame slot (N = 8192: 68 KB slab + 64 KB ring of the CU's 160 KB, one workgroup
// per CU as with cu8).
#include "k1_kernels.h"

namespace rpf {

namespace {

template <int FMT>
const Variant* find_in_table(int N)
{
    constexpr int R = FMT == kFmtCs16 ? 2 : 4;     // ring depth of the three smallest sizes
    // Template arguments after <N, P>: OCC, OCCW, DBUF, ACCB, PF32, RAWD, ABL, TWLDS, WGO, FMT -- rpf_kernels.hip's defaults
    static const Variant table[] = {
        make_variant<64, 8, 4, 4, false, 0, false, R, 0, false, 0, FMT>(0),
        make_variant<128, 16, 3, 3, false, 0, false, R, 0, false, 0, FMT>(0),
        make_variant<256, 16, 3, 3, false, 0, false, R, 0, false, 0, FMT>(0),
        make_variant<512, 8, 4, 4, false, 0, false, 2, 0, false, 0, FMT>(0),
        make_variant<1024, 16, 3, 2, false, 0, false, 2, 0, true, 0, FMT>(0),
        make_variant<2048, 16, 2, 2, false, 0, false, 2, 0, true, 512, FMT>(0),
        make_variant<4096, 16, 2, 2, false, 0, false, 2, 0, true, 512, FMT>(0),
        make_variant<8192, 16, 2, 2, false, 0, false, 2, 0, false, 0, FMT>(0),
    };
    for (const Variant& v : table)
        if (v.N == N) return &v;
    return nullptr;
}

}  // namespace

const Variant* find_format_variant(int N, int fmt)
{
    return fmt == kFmtCs8 ? find_in_table<kFmtCs8>(N) : fmt == kFmtCs16 ? find_in_table<kFmtCs16>(N) : nullptr;
}

}  // namespace rpf
