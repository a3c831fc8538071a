// TEST-ONLY host build of fft_core.h's sample-format code (tests/test_sample_formats.py): the signed unpacks over every
// bit pattern, and the wave-local raw layout of the 16-bit format (raw_source <-> phase_unpack) for one wave.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../rtl-power-fftw_amd/csrc/fft_core.h"

namespace {

using G = rpf::Geom<512, 8>;     // T = 64: one frame is exactly one wave

// Unpacks `count` samples (I = pattern k, Q = pattern count - 1 - k) eight at a time through phase_unpack and counts
// the components that are not exactly sgn * float(v) (* w when windowed, w a power of two: no rounding).
template <int FMT, typename INT>
long unpack_mismatches(long count)
{
    constexpr int SB = rpf::sample_bytes_of(FMT), CH = rpf::raw_chunk_of(FMT);
    std::vector<uint8_t> raw(CH * G::P);
    long bad = 0;
    for (long k0 = 0; k0 < count; k0 += G::P) {
        INT want_i[G::P], want_q[G::P];
        for (int a = 0; a < G::P; ++a) {
            const INT vi = static_cast<INT>(k0 + a), vq = static_cast<INT>(count - 1 - (k0 + a));
            want_i[a] = vi;
            want_q[a] = vq;
            std::memcpy(raw.data() + CH * a, &vi, SB / 2);          // little-endian host
            std::memcpy(raw.data() + CH * a + SB / 2, &vq, SB / 2);
        }
        for (int mode = 0; mode < 3; ++mode) {
            const float sgn = mode == 1 ? -1.0f : 1.0f;
            float wsgn[G::P];
            for (int a = 0; a < G::P; ++a) wsgn[a] = 0.25f * sgn;
            rpf::cf x[G::P];
            if (mode == 2) rpf::phase_unpack<G, true, FMT>(raw.data(), sgn, wsgn, x);
            else rpf::phase_unpack<G, false, FMT>(raw.data(), sgn, wsgn, x);
            const float scale = mode == 2 ? 0.25f : sgn;
            for (int a = 0; a < G::P; ++a) {
                if (x[a].x != scale * static_cast<float>(want_i[a])) ++bad;
                if (x[a].y != scale * static_cast<float>(want_q[a])) ++bad;
            }
        }
    }
    return bad;
}

// One wave stages frame `frame` (N samples of FMT) through raw_source and every lane unpacks: register a of lane t
// must hold sample t + T a.  Returns the number of components that do not.
template <int FMT, typename INT>
long layout_mismatches(const uint8_t* frame)
{
    constexpr int SB = rpf::sample_bytes_of(FMT), CH = rpf::raw_chunk_of(FMT);
    std::vector<uint8_t> raw(CH * G::P);
    for (int j = 0; j < CH * G::P; ++j) {
        int slot, off;
        rpf::raw_source<G, FMT>(0, j, &slot, &off);
        if (slot != 0 || off < 0 || off >= SB * G::N) return -1;
        raw[j] = frame[off];
    }
    long bad = 0;
    for (int t = 0; t < G::T; ++t) {
        rpf::cf x[G::P];
        rpf::phase_unpack<G, false, FMT>(raw.data() + SB * t, 1.0f, nullptr, x);
        for (int a = 0; a < G::P; ++a) {
            INT v[2];
            std::memcpy(v, frame + SB * (t + G::T * a), SB);
            if (x[a].x != static_cast<float>(v[0]) || x[a].y != static_cast<float>(v[1])) ++bad;
        }
    }
    return bad;
}

}  // namespace

extern "C" {
long rpf_emul_cs8_unpack_mismatches(void) { return unpack_mismatches<rpf::kFmtCs8, int8_t>(256); }
long rpf_emul_cs16_unpack_mismatches(void) { return unpack_mismatches<rpf::kFmtCs16, int16_t>(65536); }
long rpf_emul_cs8_layout_mismatches(const uint8_t* frame) { return layout_mismatches<rpf::kFmtCs8, int8_t>(frame); }
long rpf_emul_cs16_layout_mismatches(const uint8_t* frame) { return layout_mismatches<rpf::kFmtCs16, int16_t>(frame); }
int rpf_emul_formats_n(void) { return G::N; }
}
