// rpf_quantile.hip -- per-bin quantiles of the rows an engine has stored (rpf_quantile_select_device): K rows of N
// doubles in HBM, read only, and for every bin the order statistics v_(j), v_(j+1) of its K values, found by an
// MSB-first radix select over quantile_core.h's keys and interpolated.  Five kernels:
//   quantile_init_kernel    every (quantile, bin) starts with an empty prefix and the rank j; the counts are zeroed;
//   quantile_count_kernel   one digit pass: a workgroup walks its share of the rows of a 64-bin tile, counts in LDS the
//                           keys that share the prefix by their next digit, and adds its non-zero counts to the
//                           global counts with integer atomics;
//   quantile_narrow_kernel  after each count: the digit joins the prefix, the rank drops, the counts are zeroed again;
//   quantile_above_kernel   the further pass: the smallest key above the prefix, where v_(j+1) is needed and is no tie;
//   quantile_finish_kernel  keys back to doubles, the interpolation, the output planes.
// A lane owns one bin of the tile, a wave reads 64 adjacent bins of a row (512 bytes) per load, the four waves of a
// workgroup take the rows of its share in turn, eight loads in flight each, and the row shares of a tile are spread
// over blockIdx.y: the parallelism is tiles x row shares, whatever N is.  All quantiles of a call share each read of
// the rows.
// Bytes read per call: (kQuantilePasses + 1) K N 8, the last K N 8 only if some (quantile, bin) needs v_(j+1).
// Integer counts and an integer minimum: the result does not depend on the grid.  Plain C++, no scratch memory.  A
// translation unit of its own: it compiles beside the others and none of their kernels moves.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "quantile_core.h"
#include "rpf_kernels.h"

namespace rpf {

namespace {

constexpr int kTile = 64;            // bins of a tile = lanes of a wave
constexpr int kWaves = 4;            // waves of a workgroup = rows in flight per step
constexpr int kBlock = kTile * kWaves;
constexpr int kBatch = 8;            // rows a wave has in flight: eight 512-byte loads before the first is used
constexpr int kMaxChunk = 1 << 15;   // bins whose state the workspace holds at a time (a call walks N in such chunks)
constexpr int kTargetBlocks = 2048;  // about eight workgroups per CU

// The workspace of a chunk of C bins (C = quantile_chunk(N)), for up to kQuantileMaxQ quantiles.
struct Work {
    uint64_t* prefix;     // [q][C]
    uint64_t* above;      // [q][C]   smallest key above the prefix (the further pass)
    uint32_t* counts;     // [q][digit][C]
    uint32_t* rank;       // [q][C]   after the last pass: kQuantileNoAbove, or anything else = `above` is searched
};

__host__ __device__ inline Work work_of(void* base, int C)
{
    Work w;
    const size_t c = static_cast<size_t>(C);
    w.prefix = static_cast<uint64_t*>(base);
    w.above = w.prefix + kQuantileMaxQ * c;
    w.counts = reinterpret_cast<uint32_t*>(w.above + kQuantileMaxQ * c);
    w.rank = w.counts + static_cast<size_t>(kQuantileMaxQ) * kQuantileDigits * c;
    return w;
}

// Thread (quantile q, bin b of the chunk of cb bins).
__global__ __launch_bounds__(kBlock) void quantile_init_kernel(void* work, int C, int cb, QuantileRanks ranks)
{
    const int b = static_cast<int>(blockIdx.x) * kBlock + threadIdx.x, q = blockIdx.y;
    if (b >= cb) return;
    const Work w = work_of(work, C);
    const size_t at = static_cast<size_t>(q) * C + b;
    w.prefix[at] = 0;
    w.above[at] = kQuantileNanKey;
    w.rank[at] = ranks.j[q];
#pragma unroll
    for (int d = 0; d < kQuantileDigits; ++d) w.counts[(static_cast<size_t>(q) * kQuantileDigits + d) * C + b] = 0;
}

// Block (tile, row share): lane = bin bin0 + tile kTile + lane of the chunk, wave v takes the rows r0 + v, r0 + v +
// kWaves, ... of the share [r0, r1).  LDS counts [q][digit][lane]: the lanes of a wave hit 64 consecutive words, so an
// LDS add has no bank conflict; waves meet on a word only through the atomic.
template <int NQ>
__global__ __launch_bounds__(kBlock) void quantile_count_kernel(const double* __restrict__ rows, int K, int N, int bin0,
                                                                int cb, int C, void* work, int shift, uint64_t prefix_mask)
{
    __shared__ uint32_t lds[NQ * kQuantileDigits * kTile];
    const int lane = threadIdx.x % kTile, wave = threadIdx.x / kTile;
    const int b = static_cast<int>(blockIdx.x) * kTile + lane;             // bin of the chunk
    const bool live = b < cb;
    const Work w = work_of(work, C);
    for (int i = threadIdx.x; i < NQ * kQuantileDigits * kTile; i += kBlock) lds[i] = 0;
    uint64_t prefix[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) prefix[q] = live ? w.prefix[static_cast<size_t>(q) * C + b] : 0;
    __syncthreads();
    const int share = (K + static_cast<int>(gridDim.y) - 1) / static_cast<int>(gridDim.y);
    const int r0 = static_cast<int>(blockIdx.y) * share, r1 = min(K, r0 + share);
    if (live) {
        const uint64_t* const col = reinterpret_cast<const uint64_t*>(rows) + bin0 + b;
        // kBatch rows' loads are issued before the first is used: the LDS adds would otherwise fence every load
        for (int r = r0 + wave; r < r1; r += kWaves * kBatch) {
            uint64_t bits[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const int rr = r + u * kWaves;                              // (the same in every lane of the wave)
                bits[u] = rr < r1 ? col[static_cast<size_t>(rr) * N] : 0;
            }
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                if (r + u * kWaves >= r1) break;
                const uint64_t key = quantile_key(bits[u]);
                const int digit = quantile_digit(key, shift);
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                    if (quantile_matches(key, prefix[q], prefix_mask)) atomicAdd(&lds[(q * kQuantileDigits + digit) * kTile + lane], 1u);
            }
        }
    }
    __syncthreads();
    // the tile's counts into the chunk's: word i of the LDS block is (q, digit, lane); zeros add nothing
    for (int i = threadIdx.x; i < NQ * kQuantileDigits * kTile; i += kBlock) {
        const uint32_t n = lds[i];
        const int bb = static_cast<int>(blockIdx.x) * kTile + i % kTile;
        if (n != 0 && bb < cb) atomicAdd(&w.counts[static_cast<size_t>(i / kTile) * C + bb], n);
    }
}

// Thread (quantile q, bin b of the chunk): quantile_narrow on its counts, which are zeroed for the next pass.  After the
// last pass (shift = 0) the rank word says whether the further pass must look for v_(j+1): not when the call does not
// interpolate at this quantile (g = 0), and not when more keys equal to v_(j) are left than the rank uses up -- a tie,
// v_(j+1) is the same key.
__global__ __launch_bounds__(kBlock) void quantile_narrow_kernel(void* work, int C, int cb, int shift, QuantileRanks ranks)
{
    const int b = static_cast<int>(blockIdx.x) * kBlock + threadIdx.x, q = blockIdx.y;
    if (b >= cb) return;
    const Work w = work_of(work, C);
    const size_t at = static_cast<size_t>(q) * C + b;
    uint32_t* const counts = w.counts + static_cast<size_t>(q) * kQuantileDigits * C + b;
    uint64_t prefix = w.prefix[at];
    uint32_t rank = w.rank[at];
    const uint32_t in_digit = quantile_narrow(counts, static_cast<size_t>(C), shift, prefix, rank);
#pragma unroll
    for (int d = 0; d < kQuantileDigits; ++d) counts[static_cast<size_t>(d) * C] = 0;
    w.prefix[at] = prefix;
    if (shift == 0) {
        const bool tie = rank + 1 < in_digit;
        if (ranks.g[q] == 0.0 || tie) {
            rank = kQuantileNoAbove;
            w.above[at] = prefix;
        } else {
            rank = 0;
        }
    }
    w.rank[at] = rank;
}

// The count kernel's walk with a running minimum per quantile in registers: the smallest key above the prefix.  The
// waves' minima meet in LDS, the workgroups' in `above`, both through integer atomics.
template <int NQ>
__global__ __launch_bounds__(kBlock) void quantile_above_kernel(const double* __restrict__ rows, int K, int N, int bin0,
                                                                int cb, int C, void* work)
{
    __shared__ unsigned long long lds[NQ * kTile];
    const int lane = threadIdx.x % kTile, wave = threadIdx.x / kTile;
    const int b = static_cast<int>(blockIdx.x) * kTile + lane;
    const bool live = b < cb;
    const Work w = work_of(work, C);
    for (int i = threadIdx.x; i < NQ * kTile; i += kBlock) lds[i] = kQuantileNanKey;
    uint64_t prefix[NQ], least[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        prefix[q] = live ? w.prefix[static_cast<size_t>(q) * C + b] : 0;
        least[q] = kQuantileNanKey;
    }
    __syncthreads();
    const int share = (K + static_cast<int>(gridDim.y) - 1) / static_cast<int>(gridDim.y);
    const int r0 = static_cast<int>(blockIdx.y) * share, r1 = min(K, r0 + share);
    if (live) {
        const uint64_t* const col = reinterpret_cast<const uint64_t*>(rows) + bin0 + b;
        for (int r = r0 + wave; r < r1; r += kWaves * kBatch) {
            uint64_t bits[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const int rr = r + u * kWaves;
                bits[u] = rr < r1 ? col[static_cast<size_t>(rr) * N] : 0;
            }
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                if (r + u * kWaves >= r1) break;
                const uint64_t key = quantile_key(bits[u]);
#pragma unroll
                for (int q = 0; q < NQ; ++q) least[q] = (key > prefix[q] && key < least[q]) ? key : least[q];
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            if (least[q] != kQuantileNanKey) atomicMin(&lds[q * kTile + lane], static_cast<unsigned long long>(least[q]));
    }
    __syncthreads();
    if (wave == 0 && live) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const size_t at = static_cast<size_t>(q) * C + b;
            const unsigned long long m = lds[q * kTile + lane];
            if (m != kQuantileNanKey && w.rank[at] != kQuantileNoAbove)
                atomicMin(reinterpret_cast<unsigned long long*>(&w.above[at]), m);
        }
    }
}

// Thread (quantile q, bin b of the chunk): out[q N + bin0 + b].  empty: no rows are stored, every output is NaN and
// the workspace is not read.
__global__ __launch_bounds__(kBlock) void quantile_finish_kernel(const void* work, int C, int cb, int N, int bin0,
                                                                 QuantileRanks ranks, double* __restrict__ out, int empty)
{
    const int b = static_cast<int>(blockIdx.x) * kBlock + threadIdx.x, q = blockIdx.y;
    if (b >= cb) return;
    double* const at_out = out + static_cast<size_t>(q) * N + bin0 + b;
    if (empty) {
        *at_out = quantile_double(quantile_unkey(kQuantileNanKey));
        return;
    }
    const Work w = work_of(const_cast<void*>(work), C);
    const size_t at = static_cast<size_t>(q) * C + b;
    const double a = quantile_double(quantile_unkey(w.prefix[at]));
    const double v = quantile_double(quantile_unkey(w.above[at]));
    *at_out = quantile_interp(a, v, ranks.g[q]);
}

template <int NQ>
void launch_count(dim3 grid, hipStream_t s, const double* rows, int K, int N, int bin0, int cb, int C, void* work, int pass)
{
    hipLaunchKernelGGL((quantile_count_kernel<NQ>), grid, dim3(kBlock), 0, s, rows, K, N, bin0, cb, C, work,
                       quantile_shift(pass), quantile_prefix_mask(pass));
}

template <int NQ>
void launch_above(dim3 grid, hipStream_t s, const double* rows, int K, int N, int bin0, int cb, int C, void* work)
{
    hipLaunchKernelGGL((quantile_above_kernel<NQ>), grid, dim3(kBlock), 0, s, rows, K, N, bin0, cb, C, work);
}

#define RPF_QUANTILE_BY_NQ(nq, fn, ...)          \
    switch (nq) {                                \
        case 1: fn<1>(__VA_ARGS__); break;       \
        case 2: fn<2>(__VA_ARGS__); break;       \
        case 3: fn<3>(__VA_ARGS__); break;       \
        case 4: fn<4>(__VA_ARGS__); break;       \
        case 5: fn<5>(__VA_ARGS__); break;       \
        case 6: fn<6>(__VA_ARGS__); break;       \
        case 7: fn<7>(__VA_ARGS__); break;       \
        default: fn<8>(__VA_ARGS__); break;      \
    }

}  // namespace

int quantile_chunk(int N) { return std::min(N, kMaxChunk); }

size_t quantile_work_bytes(int N)
{
    const size_t c = static_cast<size_t>(quantile_chunk(N));
    return kQuantileMaxQ * c * (2 * sizeof(uint64_t) + sizeof(uint32_t) * (kQuantileDigits + 1));
}

hipError_t launch_quantile_select(const double* d_rows, int64_t K, int N, const QuantileRanks& ranks, void* d_work,
                                  double* d_out, hipStream_t stream)
{
    if (!d_out || K < 0 || K > INT32_MAX || N < 2 || (N & 1) || ranks.nq < 1 || ranks.nq > kQuantileMaxQ) return hipErrorInvalidValue;
    if (K > 0 && (!d_rows || !d_work)) return hipErrorInvalidValue;
    const int C = quantile_chunk(N), k = static_cast<int>(K);
    bool interpolates = false;
    for (int q = 0; q < ranks.nq; ++q) {
        if (K > 0 && ranks.j[q] >= static_cast<uint64_t>(K)) return hipErrorInvalidValue;
        interpolates = interpolates || ranks.g[q] != 0.0;
    }
    for (int bin0 = 0; bin0 < N; bin0 += C) {
        const int cb = std::min(C, N - bin0);
        const dim3 per_bin((cb + kBlock - 1) / kBlock, ranks.nq);
        if (K > 0) {
            const int tiles = (cb + kTile - 1) / kTile;
            // row shares: enough workgroups for every CU whatever N is, none with fewer than four rows per wave
            const int shares = std::max(1, std::min((k + 4 * kWaves - 1) / (4 * kWaves), (kTargetBlocks + tiles - 1) / tiles));
            const dim3 grid(tiles, shares);
            hipLaunchKernelGGL(quantile_init_kernel, per_bin, dim3(kBlock), 0, stream, d_work, C, cb, ranks);
            for (int pass = 0; pass < kQuantilePasses; ++pass) {
                RPF_QUANTILE_BY_NQ(ranks.nq, launch_count, grid, stream, d_rows, k, N, bin0, cb, C, d_work, pass);
                hipLaunchKernelGGL(quantile_narrow_kernel, per_bin, dim3(kBlock), 0, stream, d_work, C, cb, quantile_shift(pass),
                                   ranks);
            }
            if (interpolates) { RPF_QUANTILE_BY_NQ(ranks.nq, launch_above, grid, stream, d_rows, k, N, bin0, cb, C, d_work); }
        }
        hipLaunchKernelGGL(quantile_finish_kernel, per_bin, dim3(kBlock), 0, stream, d_work, C, cb, N, bin0, ranks, d_out,
                           K == 0 ? 1 : 0);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

}  // namespace rpf
