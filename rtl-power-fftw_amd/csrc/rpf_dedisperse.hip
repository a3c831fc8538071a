// rpf_dedisperse.hip -- the kernel of the incoherent dedispersion of the stored integrations (include/rpf_engine.h,
// rpf_dedisperse_device): out[d][t] = sum over the bins b, ascending, of weights[b] rows[t + delays[d][b]][b].
//
// The rows are [k][b] with b contiguous, and a lane owns (trial, time): reading the store directly, the 64 lanes of a
// wave would touch 64 different rows for every bin.  So a workgroup owns a tile of kDedispTT consecutive times x
// kDedispDT trials and walks the bins in blocks of kDedispBC, ascending.  Per block it stages rows
// [t0 + lo, t0 + kDedispTT + hi) x kDedispBC of the store into LDS, coalesced along b (256 contiguous bytes per row),
// where lo and hi are the block's span over the tile's trials (dedisperse_core.h; the engine computed them when it
// uploaded the table).  Then every lane adds the block's bins, in order, from LDS: lane time + delay - lo is its row, and
// the odd row pitch makes a wave's ds_read_b64 of one bin at 64 consecutive rows conflict-free.  The delay and the
// weight of (trial, bin) are the same for the whole wave.  The kDedispPerLane accumulators of a lane stay in registers
// for the whole walk; each is its output's sum in ascending b, so the bits do not depend on the grid or the tiling.
//
// A (tile, block) whose span does not fit the LDS tile is read straight from the store by every lane: correct and
// slow.  No scratch, no atomics, no second pass (profiles/dedisperse_resources.txt).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dedisperse_core.h"
#include "rpf_kernels.h"

namespace rpf {

namespace {

constexpr int kBatch = 8;       // bins whose loads are in flight together in the staged walk

__global__ __launch_bounds__(kDedispWG) void dedisperse_kernel(const double* __restrict__ rows, long K, int N,
                                                               const int32_t* __restrict__ delays,
                                                               const double* __restrict__ weights,
                                                               const DedispSpan* __restrict__ spans, int D, long T,
                                                               double* __restrict__ out)
{
    __shared__ double tile[kDedispRows * kDedispPitch];
    const int lane = threadIdx.x, lt = dedisperse_lane_time(lane);
    const long t0 = static_cast<long>(blockIdx.x) * kDedispTT, t = t0 + lt, n = N;
    const int d0 = blockIdx.y * kDedispDT, nblocks = dedisperse_bin_blocks(N);
    double acc[kDedispPerLane];
#pragma unroll
    for (int j = 0; j < kDedispPerLane; ++j) acc[j] = 0.0;

    for (int blk = 0; blk < nblocks; ++blk) {
        const DedispSpan sp = spans[blockIdx.y * nblocks + blk];            // (the same for the whole workgroup)
        if (dedisperse_span_empty(sp)) continue;
        const int c0 = blk * kDedispBC, bc = min(kDedispBC, N - c0);
        const bool staged = dedisperse_span_fits(sp);
        if (staged) {
            const long r0 = t0 + sp.lo, cells = dedisperse_staged_rows(sp, t0, K) * kDedispBC;
            for (long i = lane; i < cells; i += kDedispWG) {
                const int row = static_cast<int>(i / kDedispBC), col = static_cast<int>(i % kDedispBC);
                if (col < bc) tile[dedisperse_lds_index(row, col)] = rows[(r0 + row) * n + c0 + col];
            }
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < kDedispPerLane; ++j) {
            // the same for the whole wave, and said so: the weights and the delays then come by scalar loads
            const int d = __builtin_amdgcn_readfirstlane(d0 + dedisperse_lane_trial(lane, j));
            if (d >= D) continue;
            const int32_t* dl = delays + static_cast<long>(d) * n + c0;
            if (staged) {
                // (a lane at t >= T reads rows of the tile that nothing staged; its sums are never stored)
                const int up = lt - sp.lo;                                   // row = lane time + delay - lo, in [0, kDedispRows)
                int c = 0;
                // kBatch bins at a time: their weights and delays (the same for the whole wave) and their LDS reads are
                // issued together, the additions follow in order.  A bin of weight 0 reads row 0 (its delay lies outside
                // the span) and its value is dropped.
                for (; c + kBatch <= bc; c += kBatch) {
                    double w[kBatch], r[kBatch];
                    int32_t dv[kBatch];
#pragma unroll
                    for (int u = 0; u < kBatch; ++u) {
                        w[u] = weights[c0 + c + u];
                        dv[u] = dl[c + u];
                    }
#pragma unroll
                    for (int u = 0; u < kBatch; ++u) r[u] = tile[dedisperse_lds_index(w[u] != 0.0 ? up + dv[u] : 0, c + u)];
#pragma unroll
                    for (int u = 0; u < kBatch; ++u) acc[j] = w[u] != 0.0 ? dedisperse_term(acc[j], w[u], r[u]) : acc[j];
                }
                for (; c < bc; ++c) {
                    const double w = weights[c0 + c];
                    if (w != 0.0) acc[j] = dedisperse_term(acc[j], w, tile[dedisperse_lds_index(up + dl[c], c)]);
                }
            } else if (t < T) {
                for (int c = 0; c < bc; ++c) {
                    const double w = weights[c0 + c];
                    if (w != 0.0) acc[j] = dedisperse_term(acc[j], w, rows[(t + dl[c]) * n + c0 + c]);
                }
            }
        }
        if (staged) __syncthreads();
    }
    if (t >= T) return;
#pragma unroll
    for (int j = 0; j < kDedispPerLane; ++j) {
        const int d = d0 + dedisperse_lane_trial(lane, j);
        if (d < D) out[static_cast<long>(d) * T + t] = acc[j];
    }
}

}  // namespace

hipError_t launch_dedisperse(const double* d_rows, long K, int N, const int32_t* d_delays, const double* d_weights,
                             const void* d_spans, int D, long T, double* d_out, hipStream_t stream)
{
    if (T < 1) return hipSuccess;
    if (!d_rows || !d_delays || !d_weights || !d_spans || !d_out || N < 1 || D < 1 || D > kDedispMaxTrials || T > K)
        return hipErrorInvalidValue;
    const long tiles = dedisperse_time_tiles(T);
    if (tiles > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(dedisperse_trial_tiles(D)));
    hipLaunchKernelGGL(dedisperse_kernel, grid, dim3(kDedispWG), 0, stream, d_rows, K, N, d_delays, d_weights,
                       static_cast<const DedispSpan*>(d_spans), D, T, d_out);
    return hipGetLastError();
}

}  // namespace rpf
