// rpf_excise.hip -- the excised average (rpf_accumulate_device_excised): the rows a series of statistics left in HBM,
// S1[N] S2[N] PK[N] each, judged bin by bin with the row's spectral kurtosis and summed where they pass.  Two kernels
// over excise_core.h's element step and addition order:
//   excise_rows_kernel     one piece of rows into the (row group, bin) accumulators, and the piece's mask bytes;
//   excise_combine_kernel  the accumulators of every bin, added in the fixed order, into clean / kept / total.
// Plain C++, memory bound: 16 N bytes read per row (PK is not read).  A translation unit of its own: it compiles
// beside the others and none of their kernels moves.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "excise_core.h"
#include "rpf_kernels.h"

namespace rpf {

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef unsigned char uc2 __attribute__((ext_vector_type(2)));

// Thread (group g, bin pair b) of block (bin tile, group tile): rows r of the piece with (k0 + r) mod G == g, in
// increasing r, into accumulator g of the pair's two bins.  A wave reads two 512-byte runs of a plane per load
// instruction, 16 bytes per lane; rows and state are 16-byte aligned because N is even.  first: the call's first
// piece, the accumulators start from zero instead of from `state`.  Every thread with a bin and a group stores its
// accumulators, rows or not, so after the first piece all of `state` is defined.
template <int PAIRS, int GR>
__global__ __launch_bounds__(PAIRS* GR) void excise_rows_kernel(const double* __restrict__ rows, int kc, int k0_mod_g,
                                                                 int N, int G, double m, double sk_lo, double sk_hi,
                                                                 double* __restrict__ state,
                                                                 unsigned char* __restrict__ mask, int mask_pairs,
                                                                 int first)
{
    const int b = threadIdx.x % PAIRS;
    const int g = static_cast<int>(blockIdx.y) * GR + threadIdx.x / PAIRS;
    const int bin = static_cast<int>(blockIdx.x) * (2 * PAIRS) + 2 * b;     // N is even: a pair never straddles the end
    if (bin >= N || g >= G) return;
    const size_t plane = static_cast<size_t>(N);
    double* const st = state + static_cast<size_t>(g) * kExcisePlanes * plane + bin;
    ExciseAcc x = {0.0, 0.0, 0.0}, y = {0.0, 0.0, 0.0};
    if (!first) {
        const d2 c = *reinterpret_cast<const d2*>(st), k = *reinterpret_cast<const d2*>(st + plane),
                 t = *reinterpret_cast<const d2*>(st + 2 * plane);
        x = ExciseAcc{c.x, k.x, t.x};
        y = ExciseAcc{c.y, k.y, t.y};
    }
    int r = g - k0_mod_g;                                                    // the first row of this group in the piece
    if (r < 0) r += G;
#pragma unroll 4
    for (; r < kc; r += G) {
        const double* const row = rows + static_cast<size_t>(r) * kStatsPlanes * plane + bin;
        const d2 s1 = *reinterpret_cast<const d2*>(row), s2 = *reinterpret_cast<const d2*>(row + plane);
        const unsigned char fx = excise_step(x, s1.x, s2.x, m, sk_lo, sk_hi);
        const unsigned char fy = excise_step(y, s1.y, s2.y, m, sk_lo, sk_hi);
        if (mask) {
            unsigned char* const at = mask + static_cast<size_t>(r) * plane + bin;
            if (mask_pairs) {                                                // an even mask address: one 2-byte store
                *reinterpret_cast<uc2*>(at) = uc2{fx, fy};
            } else {
                at[0] = fx;
                at[1] = fy;
            }
        }
    }
    *reinterpret_cast<d2*>(st) = d2{x.clean, y.clean};
    *reinterpret_cast<d2*>(st + plane) = d2{x.kept, y.kept};
    *reinterpret_cast<d2*>(st + 2 * plane) = d2{x.total, y.total};
}

// Thread (lane j, bin pair b): the accumulators of the groups j, j + LANES, ... in increasing order; lane 0 then adds
// the lanes' sums in lane order (excise_core.h) and stores the three planes of the pair.
template <int PAIRS, int LANES>
__global__ __launch_bounds__(PAIRS* LANES) void excise_combine_kernel(const double* __restrict__ state, int N, int G,
                                                                       double* __restrict__ out)
{
    __shared__ d2 red[kExcisePlanes][LANES][PAIRS + 1];
    const int b = threadIdx.x % PAIRS, j = threadIdx.x / PAIRS;
    const int bin = static_cast<int>(blockIdx.x) * (2 * PAIRS) + 2 * b;
    const size_t plane = static_cast<size_t>(N);
    ExciseAcc x = {0.0, 0.0, 0.0}, y = {0.0, 0.0, 0.0};
    if (bin < N) {
        for (int g = j; g < G; g += LANES) {
            const double* const st = state + static_cast<size_t>(g) * kExcisePlanes * plane + bin;
            const d2 c = *reinterpret_cast<const d2*>(st), k = *reinterpret_cast<const d2*>(st + plane),
                     t = *reinterpret_cast<const d2*>(st + 2 * plane);
            x = excise_add(x, ExciseAcc{c.x, k.x, t.x});
            y = excise_add(y, ExciseAcc{c.y, k.y, t.y});
        }
    }
    red[0][j][b] = d2{x.clean, y.clean};
    red[1][j][b] = d2{x.kept, y.kept};
    red[2][j][b] = d2{x.total, y.total};
    __syncthreads();
    if (j == 0 && bin < N) {
        ExciseAcc tx = {0.0, 0.0, 0.0}, ty = {0.0, 0.0, 0.0};
#pragma unroll
        for (int l = 0; l < LANES; ++l) {
            tx = excise_add(tx, ExciseAcc{red[0][l][b].x, red[1][l][b].x, red[2][l][b].x});
            ty = excise_add(ty, ExciseAcc{red[0][l][b].y, red[1][l][b].y, red[2][l][b].y});
        }
        *reinterpret_cast<d2*>(out + bin) = d2{tx.clean, ty.clean};
        *reinterpret_cast<d2*>(out + plane + bin) = d2{tx.kept, ty.kept};
        *reinterpret_cast<d2*>(out + 2 * plane + bin) = d2{tx.total, ty.total};
    }
}

}  // namespace

size_t excise_state_doubles(int N) { return static_cast<size_t>(excise_groups(N)) * kExcisePlanes * static_cast<size_t>(N); }

hipError_t launch_excise_rows(const double* d_rows, int64_t kc, int64_t k0, int N, int64_t L, double sk_lo, double sk_hi,
                              double* d_state, uint8_t* d_mask, bool first, hipStream_t stream)
{
    if (!d_rows || !d_state || kc < 1 || kc > INT32_MAX || k0 < 0 || N < 2 || (N & 1) || L < 2) return hipErrorInvalidValue;
    constexpr int PAIRS = 32, GR = 8;
    const int G = excise_groups(N);
    const dim3 blocks((N + 2 * PAIRS - 1) / (2 * PAIRS), (G + GR - 1) / GR);
    const int mask_pairs = (reinterpret_cast<uintptr_t>(d_mask) & 1) == 0 ? 1 : 0;
    hipLaunchKernelGGL((excise_rows_kernel<PAIRS, GR>), blocks, dim3(PAIRS * GR), 0, stream, d_rows, static_cast<int>(kc),
                       static_cast<int>(k0 % G), N, G, static_cast<double>(L), sk_lo, sk_hi, d_state, d_mask, mask_pairs,
                       first ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_excise_combine(const double* d_state, int N, double* d_out, hipStream_t stream)
{
    if (!d_state || !d_out || N < 2 || (N & 1)) return hipErrorInvalidValue;
    constexpr int PAIRS = 8;
    hipLaunchKernelGGL((excise_combine_kernel<PAIRS, kExciseLanes>), dim3((N + 2 * PAIRS - 1) / (2 * PAIRS)),
                       dim3(PAIRS * kExciseLanes), 0, stream, d_state, N, excise_groups(N), d_out);
    return hipGetLastError();
}

}  // namespace rpf
