// TEST-ONLY host build of the correlator's core, for tests/test_correlate.py and tests/test_gpu_correlate.py:
// csrc/correlate_core.h -- the same text the kernels and the engine compile -- behind a C interface.  Built with
// -ffp-contract=off.
#include <cstdint>

#include "../../rtl-power-fftw_amd/csrc/correlate_core.h"

using namespace rpf;

extern "C" {

// re[n], im[n] = the term of a[s] = (a[2s], a[2s+1]) and b[s], s < n.  Returns 0, or -1 for a bad argument.
int rpf_emul_correlate_term(const float* a, const float* b, long long n, double* re, double* im)
{
    if (!a || !b || !re || !im || n < 0) return -1;
    for (long long s = 0; s < n; ++s) correlate_term(a[2 * s], a[2 * s + 1], b[2 * s], b[2 * s + 1], re[s], im[s]);
    return 0;
}

int rpf_emul_correlate_plane(int M, int i, int j, int c) { return correlate_plane(M, i, j, c); }
long long rpf_emul_correlate_chunk_frames(int N) { return correlate_chunk_frames(N); }
long long rpf_emul_correlate_groups(int N, int M, long long F) { return correlate_groups(N, M, F); }
long long rpf_emul_correlate_group_begin(long long F, long long G, long long g) { return correlate_group_begin(F, G, g); }
int rpf_emul_correlate_bins_per_group(void) { return kCorrelateBins; }

}  // extern "C"
