// TEST-ONLY host build of the per-bin quantiles, for tests/test_quantile.py: csrc/quantile_core.h's steps -- the same
// text the kernels compile -- walked in the kernels' order (rpf_quantile.hip): the rows split over `groups` simulated
// workgroups, every digit pass counting per workgroup and adding the workgroups' counts as integers, the narrowing
// step after each pass, the further pass for v_(j+1) as a minimum over the workgroups' minima, then the interpolation.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../rtl-power-fftw_amd/csrc/quantile_core.h"

using namespace rpf;

extern "C" {

int rpf_emul_quantile_passes(void) { return kQuantilePasses; }

// key and back, element by element (what the order rests on).
void rpf_emul_quantile_keys(const double* v, long long n, unsigned long long* keys, double* back)
{
    for (long long i = 0; i < n; ++i) {
        keys[i] = quantile_key(quantile_bits(v[i]));
        back[i] = quantile_double(quantile_unkey(keys[i]));
    }
}

// rows[K x N], q[nq] -> out[nq x N].  Returns the passes over the rows that were needed (counting passes, plus one
// if some (quantile, bin) had to look for v_(j+1)), or -1.
long long rpf_emul_quantile(const double* rows, long long K, int N, const double* q, int nq, int groups, double* out)
{
    if (K < 0 || N < 1 || nq < 1 || nq > kQuantileMaxQ || groups < 1) return -1;
    const size_t plane = static_cast<size_t>(N);
    if (K == 0) {
        for (size_t i = 0; i < static_cast<size_t>(nq) * plane; ++i) out[i] = quantile_double(quantile_unkey(kQuantileNanKey));
        return 0;
    }
    QuantileRanks ranks;
    ranks.nq = nq;
    for (int i = 0; i < nq; ++i) {
        int64_t j = 0;
        quantile_rank(q[i], K, j, ranks.g[i]);
        ranks.j[i] = static_cast<uint32_t>(j);
    }
    const long long share = (K + groups - 1) / groups;                     // quantile_count_kernel's row shares
    std::vector<uint64_t> prefix(nq * plane, 0), above(nq * plane, kQuantileNanKey);
    std::vector<uint32_t> rank(nq * plane), counts(static_cast<size_t>(nq) * kQuantileDigits * plane, 0);
    for (int i = 0; i < nq; ++i)
        for (size_t b = 0; b < plane; ++b) rank[i * plane + b] = ranks.j[i];           // quantile_init_kernel
    long long passes = 0;
    for (int pass = 0; pass < kQuantilePasses; ++pass, ++passes) {
        const int shift = quantile_shift(pass);
        const uint64_t mask = quantile_prefix_mask(pass);
        for (int g = 0; g < groups; ++g) {                                 // quantile_count_kernel, one workgroup
            std::vector<uint32_t> lds(static_cast<size_t>(nq) * kQuantileDigits * plane, 0);
            const long long r0 = g * share, r1 = r0 + share < K ? r0 + share : K;
            for (long long r = r0; r < r1; ++r)
                for (size_t b = 0; b < plane; ++b) {
                    const uint64_t key = quantile_key(quantile_bits(rows[static_cast<size_t>(r) * plane + b]));
                    const int digit = quantile_digit(key, shift);
                    for (int i = 0; i < nq; ++i)
                        if (quantile_matches(key, prefix[i * plane + b], mask)) ++lds[(static_cast<size_t>(i) * kQuantileDigits + digit) * plane + b];
                }
            for (size_t i = 0; i < lds.size(); ++i) counts[i] += lds[i];
        }
        for (int i = 0; i < nq; ++i)                                       // quantile_narrow_kernel
            for (size_t b = 0; b < plane; ++b) {
                const size_t at = i * plane + b;
                uint32_t* const c = counts.data() + static_cast<size_t>(i) * kQuantileDigits * plane + b;
                const uint32_t in_digit = quantile_narrow(c, plane, shift, prefix[at], rank[at]);
                for (int d = 0; d < kQuantileDigits; ++d) c[d * plane] = 0;
                if (shift == 0) {
                    const bool tie = rank[at] + 1 < in_digit;
                    if (ranks.g[i] == 0.0 || tie) {
                        rank[at] = kQuantileNoAbove;
                        above[at] = prefix[at];
                    } else {
                        rank[at] = 0;
                    }
                }
            }
    }
    bool interpolates = false;
    for (int i = 0; i < nq; ++i) interpolates = interpolates || ranks.g[i] != 0.0;
    if (interpolates) {                                                    // quantile_above_kernel
        ++passes;
        for (int g = 0; g < groups; ++g) {
            std::vector<uint64_t> least(nq * plane, kQuantileNanKey);
            const long long r0 = g * share, r1 = r0 + share < K ? r0 + share : K;
            for (long long r = r0; r < r1; ++r)
                for (size_t b = 0; b < plane; ++b) {
                    const uint64_t key = quantile_key(quantile_bits(rows[static_cast<size_t>(r) * plane + b]));
                    for (int i = 0; i < nq; ++i) {
                        uint64_t& m = least[i * plane + b];
                        m = (key > prefix[i * plane + b] && key < m) ? key : m;
                    }
                }
            for (size_t at = 0; at < nq * plane; ++at)
                if (least[at] != kQuantileNanKey && rank[at] != kQuantileNoAbove && least[at] < above[at]) above[at] = least[at];
        }
    }
    for (int i = 0; i < nq; ++i)                                           // quantile_finish_kernel
        for (size_t b = 0; b < plane; ++b) {
            const size_t at = i * plane + b;
            out[at] = quantile_interp(quantile_double(quantile_unkey(prefix[at])), quantile_double(quantile_unkey(above[at])), ranks.g[i]);
        }
    return passes;
}

}  // extern "C"
