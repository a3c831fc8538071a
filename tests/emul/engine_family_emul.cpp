// csrc/engine_family.h's select_family for tests/test_engine_family.py (which compiles this file): the query's bools
// travel as bits, in FamilyQuery's order from `cu8` (bit 0) to `generic` (bit 12); returns the enumerator (None = no kernel).
// With -DENGINE_FAMILY_MAIN it is a stand-alone program that walks the test's enumeration itself and prints how often
// each family won -- what a sanitizer build runs:
//   g++ -std=c++11 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DENGINE_FAMILY_MAIN engine_family_emul.cpp
#include "../../rtl-power-fftw_amd/csrc/engine_family.h"

extern "C" int rpf_emul_select_family(int N, int variant, unsigned bits)
{
    auto bit = [&](int k) { return ((bits >> k) & 1u) != 0; };
    const rpf::FamilyQuery q{N,      variant, bit(0), bit(1), bit(2),  bit(3),  bit(4), bit(5),
                             bit(6), bit(7),  bit(8), bit(9), bit(10), bit(11), bit(12)};
    return static_cast<int>(rpf::select_family(q));
}

#ifdef ENGINE_FAMILY_MAIN
#include <cstdio>
#include <initializer_list>

int main()
{
    long won[7] = {};      // [enumerator]
    long total = 0;
    for (int N : {32768, 4096})
        for (int variant : {0, 1})
            for (unsigned bits = 0; bits < (1u << 13); ++bits) {
                const unsigned three = (bits >> 9) & 7u;                      // fourstep, bluestein, bigblu
                if (three & (three - 1)) continue;                            // at most one of them
                if (variant == 0 && ((bits >> 6) & 1u) != ((bits >> 7) & 1u)) continue;   // k1 is k1_v0 at variant 0
                ++won[rpf_emul_select_family(N, variant, bits)];
                ++total;
            }
    std::printf("%ld queries:", total);
    for (int f = 0; f < 7; ++f) std::printf(" %d:%ld", f, won[f]);
    std::printf("\n");
    return 0;
}
#endif
