// TEST-ONLY host build of fft_core.h's cf32 code (tests/test_cf32.py): the wave-local raw layout of 8-byte samples
// (raw_source <-> phase_unpack) for every K1 geometry, the unpack arithmetic, and a cf32 frame of int16 values
// against the cs16 frame of the same values through the emulated transform (the phase functions of fft_core.h run
// thread by thread, as tests/emul/fft_emul.cpp runs them for cu8).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../rtl-power-fftw_amd/csrc/k1_sizes.h"

namespace {

using rpf::cf;
constexpr int F = rpf::kFmtCf32;

// Row I of K1's size table as the cf32 kernels take it: k1_sizes.h itself (compiled for the host), so that what is
// checked here is the geometry the kernels are instantiated with.
template <int I>
struct Row {
    static constexpr rpf::K1Size s = rpf::k1_size(I, F, false);
    using G = rpf::Geom<s.N, s.P>;
    static constexpr int WG = rpf::k1_workgroup(s.N, s.P, s.WGO);
    static_assert(WG == rpf::k1_geometry<G>(s.WGO, 1, s.RAWD, F, s.TWLDS).WG, "");
};

// The waves of a workgroup stage their areas through raw_source: every byte of every frame slot exactly once, in
// 16-byte pieces contiguous and 16-byte aligned in the source.  Returns the number of violations.
template <class R>
long coverage_violations()
{
    using G = typename R::G;
    constexpr int FPW = R::WG / G::T, AREA = rpf::raw_chunk_of(F) * G::P, FRAME = rpf::sample_bytes_of(F) * G::N;
    static_assert(rpf::sample_bytes_of(F) == 8 && rpf::raw_chunk_of(F) == 512, "");
    std::vector<int> seen(static_cast<size_t>(FPW) * FRAME, 0);
    long bad = 0;
    for (int w = 0; w < R::WG / 64; ++w)
        for (int j = 0; j < AREA; j += 16) {
            int slot0, off0;
            rpf::raw_source<G, F>(w, j, &slot0, &off0);
            if (off0 % 16 != 0) ++bad;
            for (int k = 0; k < 16; ++k) {
                int slot, off;
                rpf::raw_source<G, F>(w, j + k, &slot, &off);
                if (slot != slot0 || off != off0 + k) ++bad;
                if (slot < 0 || slot >= FPW || off < 0 || off >= FRAME) { ++bad; continue; }
                ++seen[static_cast<size_t>(slot) * FRAME + off];
            }
        }
    for (int c : seen)
        if (c != 1) ++bad;
    return bad;
}

// One workgroup stages FPW frames (`frames`: FPW x N complex floats) and every lane unpacks: register a of thread t of
// slot fs must hold v * sgn exactly, or fl(v * (w * sgn)) with the window.  Returns the components that do not.
template <class R>
long unpack_mismatches(const float* frames, const float* window)
{
    using G = typename R::G;
    constexpr int AREA = rpf::raw_chunk_of(F) * G::P, FRAME = 8 * G::N;
    const uint8_t* src = reinterpret_cast<const uint8_t*>(frames);
    std::vector<uint8_t> raw(static_cast<size_t>(R::WG / 64) * AREA);
    for (int w = 0; w < R::WG / 64; ++w)
        for (int j = 0; j < AREA; ++j) {
            int slot, off;
            rpf::raw_source<G, F>(w, j, &slot, &off);
            raw[static_cast<size_t>(w) * AREA + j] = src[static_cast<size_t>(slot) * FRAME + off];
        }
    long bad = 0;
    for (int tid = 0; tid < R::WG; ++tid) {
        const int fs = tid / G::T, t = tid % G::T;
        const float sgn = (t & 1) ? -1.0f : 1.0f;
        float wsgn[G::P];
        for (int a = 0; a < G::P; ++a) wsgn[a] = window ? window[t + G::T * a] * sgn : 0.0f;
        cf x[G::P];
        const uint8_t* lane_raw = raw.data() + static_cast<size_t>(tid / 64) * AREA + 8 * (tid % 64);
        if (window) rpf::phase_unpack<G, true, F>(lane_raw, sgn, wsgn, x);
        else rpf::phase_unpack<G, false, F>(lane_raw, sgn, wsgn, x);
        for (int a = 0; a < G::P; ++a) {
            const float* v = frames + 2 * (static_cast<size_t>(fs) * G::N + t + G::T * a);
            const float m = window ? wsgn[a] : sgn;
            // volatile: the products are rounded to float here whatever the compiler would like to contract
            volatile float wi = v[0] * m, wq = v[1] * m;
            const float got[2] = {x[a].x, x[a].y}, want[2] = {wi, wq};
            if (std::memcmp(got, want, 8)) ++bad;
        }
    }
    return bad;
}

template <class G, int J>
void load_tw(int t, const std::vector<cf>& twN, cf* tw)
{
    if constexpr (J < G::NPASS) {
        for (int r = 1; r < G::P; ++r) tw[(J - 1) * (G::P - 1) + r - 1] = twN[rpf::twiddle_index<G, J>(t, r)];
        load_tw<G, J + 1>(t, twN, tw);
    }
}
template <class G, int J>
void middle(std::vector<std::vector<cf>>& regs, std::vector<cf>& slab, const std::vector<std::vector<cf>>& tws)
{
    if constexpr (J < G::NPASS) {
        for (int t = 0; t < G::T; ++t)
            if constexpr (J > 1) rpf::phase_fetch<G, J>(t, regs[t].data(), slab.data());
        for (int t = 0; t < G::T; ++t) {
            rpf::phase_butterfly_twiddle<G>(regs[t].data(), tws[t].data() + (J - 1) * (G::P - 1));
            rpf::phase_store<G, J>(t, regs[t].data(), slab.data());
        }
        middle<G, J + 1>(regs, slab, tws);
    }
}

// One frame of format FMT through the emulated kernel: staging, unpack, passes, |X|^2 into pwr[N].
template <class G, int FMT>
void transform(const uint8_t* frame, const float* window, double* pwr)
{
    constexpr int T = G::T, P = G::P, N = G::N, WAVES = T >= 64 ? T / 64 : 1, AREA = rpf::raw_chunk_of(FMT) * P;
    constexpr int SB = rpf::sample_bytes_of(FMT);
    std::vector<cf> twN(N);
    const long double two_pi = 6.283185307179586476925286766559005768L;
    for (int k = 0; k < N; ++k) twN[k] = {(float)cosl(two_pi * k / N), (float)(-sinl(two_pi * k / N))};
    std::vector<std::vector<cf>> tws(T, std::vector<cf>((G::NPASS - 1) * (P - 1)));
    for (int t = 0; t < T; ++t) load_tw<G, 1>(t, twN, tws[t].data());
    std::vector<std::vector<cf>> regs(T, std::vector<cf>(P));
    std::vector<cf> slab(G::LDS_CPX, cf{NAN, NAN});
    std::vector<uint8_t> raw(static_cast<size_t>(WAVES) * AREA);
    for (int w = 0; w < WAVES; ++w)
        for (int j = 0; j < AREA; ++j) {
            int slot, off;
            rpf::raw_source<G, FMT>(w, j, &slot, &off);
            raw[static_cast<size_t>(w) * AREA + j] = slot == 0 ? frame[off] : 0;
        }
    for (int t = 0; t < T; ++t) {
        const float sgn = (t & 1) ? -1.0f : 1.0f;
        float wsgn[P];
        for (int a = 0; a < P; ++a) wsgn[a] = window ? window[t + T * a] * sgn : 0.0f;
        const uint8_t* lane_raw = raw.data() + static_cast<size_t>(t / 64) * AREA + SB * (t % 64);
        if (window) rpf::phase_unpack<G, true, FMT>(lane_raw, sgn, wsgn, regs[t].data());
        else rpf::phase_unpack<G, false, FMT>(lane_raw, sgn, wsgn, regs[t].data());
    }
    middle<G, 1>(regs, slab, tws);
    for (int t = 0; t < T; ++t) {
        double acc[P] = {};
        rpf::phase_fetch<G, G::NPASS>(t, regs[t].data(), slab.data());
        rpf::phase_last<G>(regs[t].data());
        rpf::phase_accumulate(regs[t].data(), acc, P);
        for (int a = 0; a < P; ++a) pwr[rpf::bin_of<G>(t, a)] = acc[a];
    }
}

// fn(Row<I>{}) for the row of size N, or -1
template <class Fn, int... I>
long at_row(int N, Fn fn, std::integer_sequence<int, I...>)
{
    long r = -1;
    ((Row<I>::G::N == N ? (r = fn(Row<I>{}), 0) : 0), ...);
    return r;
}
template <class Fn>
long at_row(int N, Fn fn)
{
    return at_row(N, fn, std::make_integer_sequence<int, rpf::kK1SizeCount>{});
}

template <class R>
long both_formats(const uint8_t* cs16_frame, const uint8_t* cf32_frame, const float* window, double* pwr16, double* pwr32)
{
    transform<typename R::G, rpf::kFmtCs16>(cs16_frame, window, pwr16);
    transform<typename R::G, F>(cf32_frame, window, pwr32);
    return 0;
}

}  // namespace

extern "C" {
int rpf_emul_cf32_sample_bytes(void) { return rpf::sample_bytes_of(F); }
int rpf_emul_cf32_format(void) { return F; }
// the sizes of K1's table: N of row i, or -1 past its end
int rpf_emul_cf32_size(int i) { return i >= 0 && i < rpf::kK1SizeCount ? rpf::kK1Sizes[i].N : -1; }
// frames side by side in the workgroup of size N, or -1
long rpf_emul_cf32_fpw(int N)
{
    return at_row(N, [](auto row) -> long { return decltype(row)::WG / decltype(row)::G::T; });
}
long rpf_emul_cf32_coverage_violations(int N)
{
    return at_row(N, [](auto row) { return coverage_violations<decltype(row)>(); });
}
long rpf_emul_cf32_unpack_mismatches(int N, const float* frames, const float* window)
{
    return at_row(N, [&](auto row) { return unpack_mismatches<decltype(row)>(frames, window); });
}
long rpf_emul_cf32_vs_cs16(int N, const uint8_t* cs16_frame, const uint8_t* cf32_frame, const float* window,
                           double* pwr16, double* pwr32)
{
    return at_row(N, [&](auto row) { return both_formats<decltype(row)>(cs16_frame, cf32_frame, window, pwr16, pwr32); });
}
}
