// TEST-ONLY host build of k1_sizes.h for the cf32 kernels with per-bin statistics (tests/test_cf32_stats.py): the rows
// of k1_size(i, cf32, true) as the kernels are instantiated with them, their launch geometry, and the rows of the plain
// cf32 kernels beside them, so that the test can say where the two differ.  The geometry is k1_geometry with the
// arguments make_variant (k1_kernels.h) gives it: one slab, the row's ring, the twiddle table if either window form
// has it.
#include <hip/hip_runtime.h>

#include "../../rtl-power-fftw_amd/csrc/k1_sizes.h"

namespace {

constexpr int F = rpf::kFmtCf32;

template <int I, bool STATS>
struct Row {
    static constexpr rpf::K1Size s = rpf::k1_size(I, F, STATS);
    using G = rpf::Geom<s.N, s.P>;
    static constexpr rpf::K1Geometry geo = rpf::k1_geometry<G>(s.WGO, 1, s.RAWD, F, s.TWLDS || s.TWLDSW);
    static constexpr int slab_bytes = static_cast<int>(sizeof(rpf::cf)) * G::LDS_CPX;
};

template <int I, bool STATS>
void fill(int* out)
{
    using R = Row<I, STATS>;
    const int v[12] = {R::s.N, R::s.P, R::s.OCC, R::s.OCCW, R::s.RAWD, R::s.TWLDS ? 1 : 0, R::s.TWLDSW ? 1 : 0, R::s.WGO,
                       R::geo.WG, R::geo.fpw, R::geo.lds_bytes, R::slab_bytes};
    for (int k = 0; k < 12; ++k) out[k] = v[k];
}

template <int... I>
int row(int i, bool stats, int* out, std::integer_sequence<int, I...>)
{
    int found = -1;
    ((I == i ? ((stats ? fill<I, true>(out) : fill<I, false>(out)), found = 0) : 0), ...);
    return found;
}

}  // namespace

extern "C" {
int rpf_emul_cf32_stats_rows(void) { return rpf::kK1SizeCount; }
int rpf_emul_cf32_stats_lds_per_cu(void) { return rpf::kLdsPerCU; }
// out[12] = N, P, OCC, OCCW, RAWD, TWLDS, TWLDSW, WGO, WG, fpw, lds_bytes, slab bytes per frame slot of row i of
// k1_size(i, cf32, stats); -1 past the table's end
int rpf_emul_cf32_stats_row(int i, int stats, int* out)
{
    return row(i, stats != 0, out, std::make_integer_sequence<int, rpf::kK1SizeCount>{});
}
}
