// TEST-ONLY host build of the excised average, for tests/test_excise.py: csrc/excise_core.h's element step -- the same
// text the kernels compile -- walked over the rows in the kernels' order (rpf_excise.hip): piece by piece, row k of the
// call into the accumulators of row group k mod G in increasing k, then the combine's lanes and their sum in lane order.
#include <cstddef>
#include <vector>

#include "../../rtl-power-fftw_amd/csrc/excise_core.h"

using namespace rpf;

extern "C" {

int rpf_emul_excise_groups(int N) { return excise_groups(N); }

// rows[K x 3 x N] (S1, S2, PK per row) in pieces of `piece` rows -> out[3 x N] = clean, kept, total and, unless null,
// mask[K x N] (1 = flagged).  Returns the number of pieces, or -1.
long long rpf_emul_excise(const double* rows, long long K, int N, long long L, double sk_lo, double sk_hi, long long piece,
                          double* out, unsigned char* mask)
{
    if (K < 0 || N < 2 || (N & 1) || L < 2 || piece < 1) return -1;
    const int G = excise_groups(N);
    const size_t plane = static_cast<size_t>(N);
    const double m = static_cast<double>(L);
    std::vector<ExciseAcc> state(static_cast<size_t>(G) * plane);       // (valid from the first piece on, as d_state)
    long long pieces = 0;
    for (long long k0 = 0; k0 < K; k0 += piece, ++pieces) {             // excise_rows_kernel, one launch per piece
        const long long kc = piece < K - k0 ? piece : K - k0;
        const double* const piece_rows = rows + static_cast<size_t>(k0) * 3 * plane;
        const int k0_mod_g = static_cast<int>(k0 % G);
        for (int g = 0; g < G; ++g)
            for (int bin = 0; bin < N; ++bin) {
                ExciseAcc a = k0 == 0 ? ExciseAcc{0.0, 0.0, 0.0} : state[static_cast<size_t>(g) * plane + bin];
                long long r = g - k0_mod_g;
                if (r < 0) r += G;
                for (; r < kc; r += G) {
                    const double* const row = piece_rows + static_cast<size_t>(r) * 3 * plane + bin;
                    const unsigned char f = excise_step(a, row[0], row[plane], m, sk_lo, sk_hi);
                    if (mask) mask[static_cast<size_t>(k0 + r) * plane + bin] = f;
                }
                state[static_cast<size_t>(g) * plane + bin] = a;
            }
    }
    for (int bin = 0; bin < N; ++bin) {                                  // excise_combine_kernel
        ExciseAcc tot = {0.0, 0.0, 0.0};
        for (int j = 0; j < kExciseLanes; ++j) {
            ExciseAcc lane = {0.0, 0.0, 0.0};
            if (K > 0)
                for (int g = j; g < G; g += kExciseLanes) lane = excise_add(lane, state[static_cast<size_t>(g) * plane + bin]);
            tot = excise_add(tot, lane);
        }
        out[bin] = tot.clean;
        out[plane + bin] = tot.kept;
        out[2 * plane + bin] = tot.total;
    }
    return pieces;
}

// excise_sk, element by element (the arithmetic the mask rests on).
void rpf_emul_excise_sk(const double* s1, const double* s2, long long L, double* out, long long n)
{
    for (long long i = 0; i < n; ++i) out[i] = excise_sk(s1[i], s2[i], static_cast<double>(L));
}

}  // extern "C"
