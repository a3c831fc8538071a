// stft_core.h -- how a K1 frame slot's spectrum leaves the store kernels (k1_stft_body.inc; include/rpf_engine.h,
// rpf_stft_device): the staging index map, stated once.  Plain C++ over fft_core.h's geometry, so that the CPU emulator
// (tests/emul/stft_emul.cpp) compiles the same functions the kernels do.
//
// After the last pass lane t of a frame holds the bins bin_of<G>(t, a), a < P, scattered over the row.  The frame slot
// parks them in its own exchange slab (N + N/P complex values, free once every lane has fetched its last-pass inputs):
//     bin k  ->  slab[stft_stage_index<G>(k)],   stft_stage_index(k) = k + 2 (k >> log2(2P))
// two spare values after every 2P bins, N + N/P - 3 at the most.  The row is then read back in natural order, lane t in
// round i taking the bins stft_read_bin<G>(t, i) and the next one: the pair is 16 bytes, 16-byte aligned in the slab
// (an even bin has an even index and the spare values never part a pair) and in the row, so it is one 16-byte LDS read
// and one 16-byte store, and the T lanes of a round write 16 T contiguous bytes (1 KB per wave from T = 64 on).
//
// LDS bank conflicts under the banking rules tools/lds_bank_model.py states (8-byte stores: groups of 16 contiguous
// lanes, bank = dword mod 32; 16-byte reads: four groups of 16 lanes, bank = dword mod 64), as the largest number of
// distinct addresses on one bank in a group -- tests/test_stft.py recomputes them from these functions:
//     stores   1 (none) at N = 64, 256, 512, 1024, 2048;  2 at N = 128 and 4096;  4 at N = 8192
//     reads    2 at every size: the spare pair shifts the second half of a group by four banks
// Measured (profiles/stft.json), a call moves 3.7 - 5.3 TB/s of reads and writes together, at or near what HBM gives a
// stream; what these conflict cycles cost beside that has not been measured.
#pragma once

#include "fft_core.h"

namespace rpf {

template <class G>
RPF_HD int stft_stage_index(int bin)
{
    return bin + 2 * (bin >> (G::LOG2P + 1));
}

// rounds of the read-back of one row, and the first bin of lane t's pair in round i
template <class G>
constexpr int stft_read_rounds() { return G::P / 2; }
template <class G>
RPF_HD int stft_read_bin(int t, int i)
{
    return 2 * t + 2 * G::T * i;
}

// the conflict degrees stated above, for the test
constexpr int stft_store_conflicts(int N) { return N == 8192 ? 4 : (N == 128 || N == 4096) ? 2 : 1; }
constexpr int stft_read_conflicts(int) { return 2; }

}  // namespace rpf
