// rpf_fold.hip -- the kernels of the fold of a D x T plane at trial periods (include/rpf_engine.h, rpf_fold_device):
// prof[s][p][bin(p, t)] += x[s][t], the times of each of 16 segments in ascending order, the segments then added in order.
//
// A wave owns (series s, 64 consecutive periods, segment g); lane = period.  x[s][t] is the same for the whole wave, so
// it comes by scalar loads.  Every lane advances its own 64-bit phase by steps[p] per time (exact: it wraps as the
// product t steps[p] does) and takes its bin with one mul_hi.  The wave's partial profiles live in LDS as part[bin][lane]
// (fold_core.h: a pitch of 64 doubles, conflict-free whatever bin each lane holds); a lane keeps the sum of its
// current bin in a register while consecutive times fall into that bin, writes it back and loads the next bin's sum
// when the bin changes.  Every cell's additions are still in ascending t.  The partials go to scratch [g][s][p][bin],
// transposed through LDS so the stores are contiguous; fold_reduce_kernel adds the 16 segments in order.
//
// The hits are the same walk on a plane of ones in int32 (fold_kernel<false>, no series: one launch per call), and the
// two moments of a series ride along in the waves of the first period chunk.  No atomics, no cross-lane sums, no
// spilled registers (profiles/fold_resources.txt).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "fold_core.h"
#include "rpf_kernels.h"

namespace rpf {

namespace {

constexpr int kBatch = 8;       // times whose x one scalar load brings (s_load_dwordx16)

// kSeries: the sums of x[s][t] in double (and the moments); else the counts in int32.
template <bool kSeries>
__global__ __launch_bounds__(kFoldLanes) void fold_kernel(const double* __restrict__ x, long T, const uint64_t* __restrict__ steps,
                                                          int P, int NB, int series,
                                                          std::conditional_t<kSeries, double, int32_t>* __restrict__ part,
                                                          double* __restrict__ mom_part)
{
    using V = std::conditional_t<kSeries, double, int32_t>;
    extern __shared__ __attribute__((aligned(16))) unsigned char fold_lds[];
    V* const cell = reinterpret_cast<V*>(fold_lds);
    const int lane = threadIdx.x, p0 = blockIdx.x * kFoldLanes, p = p0 + lane, g = blockIdx.y;
    // the same for the whole wave, and said so: x[s][t] then comes by scalar loads
    const int s = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.z));
    const long lo = fold_segment_begin(T, g), hi = fold_segment_begin(T, g + 1);
    const uint64_t step = p < P ? steps[p] : 0;          // (a lane past P walks bin 0 and stores nothing)
    const uint32_t nb = static_cast<uint32_t>(NB);
    for (int b = 0; b < NB; ++b) cell[fold_lds_index(b, lane)] = V(0);

    const double* xs = x + static_cast<long>(s) * T;
    const bool moments = kSeries && blockIdx.x == 0 && mom_part != nullptr;
    uint64_t phase = fold_phase(step, lo);
    uint32_t cur = fold_bin_of_phase(phase, nb);
    V sum = V(0);
    double m0 = 0.0, m1 = 0.0;
    // one time: the lane's bin, its sum swapped through LDS where the bin changes, then the addition
    auto take = [&](double v) {
        const uint32_t bin = fold_bin_of_phase(phase, nb);
        if (bin != cur) {
            cell[fold_lds_index(cur, lane)] = sum;
            sum = cell[fold_lds_index(bin, lane)];
            cur = bin;
        }
        if constexpr (kSeries) {
            sum = fold_add(sum, v);
            if (moments) {
                m0 = fold_add(m0, v);
                m1 = fold_add_square(m1, v);
            }
        } else {
            sum += 1;
        }
        phase += step;
    };
    long t = lo;
    if constexpr (kSeries) {
        // kBatch times at once: one scalar load brings their x, the additions follow in order
        for (; t + kBatch <= hi; t += kBatch) {
            double v[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) v[u] = xs[t + u];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) take(v[u]);
        }
    }
    for (; t < hi; ++t) take(kSeries ? xs[t] : 0.0);
    cell[fold_lds_index(cur, lane)] = sum;
    __syncthreads();
    // out through LDS, transposed: consecutive lanes store consecutive bins of one period
    V* const out = part + (static_cast<long>(g) * series + s) * P * NB;
    for (int i = lane; i < NB * kFoldLanes; i += kFoldLanes) {
        const int pl = i / NB, b = i - pl * NB;
        if (p0 + pl < P) out[static_cast<long>(p0 + pl) * NB + b] = cell[fold_lds_index(b, pl)];
    }
    if (moments && lane == 0) {
        mom_part[(static_cast<long>(g) * series + s) * 2] = m0;
        mom_part[(static_cast<long>(g) * series + s) * 2 + 1] = m1;
    }
}

// The second level: the 16 segments of every cell, ascending.  Thread i: cell i of prof (series x cells), moment i of
// mom (series x 2) and cell i of hits (cells), where those are asked for.
__global__ __launch_bounds__(256) void fold_reduce_kernel(const double* __restrict__ part, long series_cells, double* __restrict__ prof,
                                                          const double* __restrict__ mom_part, long series2, double* __restrict__ mom,
                                                          const int32_t* __restrict__ hit_part, long cells, int32_t* __restrict__ hits)
{
    const long i = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
    if (i < series_cells) {
        double acc = 0.0;
#pragma unroll
        for (int g = 0; g < kFoldSegments; ++g) acc = fold_add(acc, part[g * series_cells + i]);
        prof[i] = acc;
    }
    if (mom && i < series2) {
        double acc = 0.0;
#pragma unroll
        for (int g = 0; g < kFoldSegments; ++g) acc = fold_add(acc, mom_part[g * series2 + i]);
        mom[i] = acc;
    }
    if (hits && i < cells) {
        int32_t n = 0;
#pragma unroll
        for (int g = 0; g < kFoldSegments; ++g) n += hit_part[g * cells + i];
        hits[i] = n;
    }
}

}  // namespace

hipError_t launch_fold(const double* d_x, int series, long T, const uint64_t* d_steps, int P, int NB, void* d_scratch,
                       double* d_prof, int32_t* d_hits, double* d_mom, hipStream_t stream)
{
    if (T < 1) return hipSuccess;
    if (!d_x || !d_steps || !d_scratch || !d_prof || series < 1 || series > kFoldMaxSeries || P < 1 || P > kFoldMaxPeriods ||
        NB < 1 || NB > kFoldMaxBins || T > 0x7fffffffL || fold_scratch(series, P, NB).bytes > kFoldScratchBytes)
        return hipErrorInvalidValue;
    const FoldScratch at = fold_scratch(series, P, NB);
    unsigned char* const base = static_cast<unsigned char*>(d_scratch);
    double* const part = reinterpret_cast<double*>(base + at.part_at);
    double* const mom_part = reinterpret_cast<double*>(base + at.mom_at);
    int32_t* const hit_part = reinterpret_cast<int32_t*>(base + at.hits_at);
    const unsigned chunks = static_cast<unsigned>(fold_period_chunks(P));
    hipLaunchKernelGGL(fold_kernel<true>, dim3(chunks, kFoldSegments, static_cast<unsigned>(series)), dim3(kFoldLanes),
                       fold_lds_bytes(NB), stream, d_x, T, d_steps, P, NB, series, part, d_mom ? mom_part : nullptr);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    if (d_hits) {
        hipLaunchKernelGGL(fold_kernel<false>, dim3(chunks, kFoldSegments, 1), dim3(kFoldLanes),
                           sizeof(int32_t) * static_cast<size_t>(NB) * kFoldLanes, stream, static_cast<const double*>(nullptr), T,
                           d_steps, P, NB, 1, hit_part, static_cast<double*>(nullptr));
        if ((err = hipGetLastError()) != hipSuccess) return err;
    }
    const long cells = static_cast<long>(P) * NB, series_cells = cells * series, series2 = 2L * series;
    const long most = series_cells > series2 ? series_cells : series2;       // (cells <= series_cells)
    hipLaunchKernelGGL(fold_reduce_kernel, dim3(static_cast<unsigned>((most + 255) / 256)), dim3(256), 0, stream, part, series_cells,
                       d_prof, mom_part, series2, d_mom, hit_part, cells, d_hits);
    return hipGetLastError();
}

}  // namespace rpf
