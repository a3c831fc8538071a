// TEST-ONLY: the schedule of K1's loader waves (rtl-power-fftw_amd/csrc/k1_loader.h) as the kernel compiles it, handed
// to tests/test_k1_loader_schedule.py value by value.  Built by k1_loader.mk into librpf_emul_k1_loader.so.
#include "../../rtl-power-fftw_amd/csrc/k1_loader.h"

using namespace rpf::k1_loader;

extern "C" {
int rpf_emul_k1_loader_prologue_barriers() { return kPrologueBarriers; }
int rpf_emul_k1_loader_barriers_per_iteration() { return kBarriersPerIteration; }
int rpf_emul_k1_loader_refill_barrier() { return kRefillBarrier; }
int rpf_emul_k1_loader_landed_barrier() { return kLandedBarrier; }
int rpf_emul_k1_loader_flush_barriers(int stats) { return flush_barriers(stats != 0); }
int rpf_emul_k1_loader_slot_of(int it, int rawd) { return slot_of(it, rawd); }
int rpf_emul_k1_loader_refill_iteration(int it, int rawd) { return refill_iteration(it, rawd); }
int rpf_emul_k1_loader_pieces_per_iteration(int compute_waves, int ldw, int pieces)
{
    return pieces_per_iteration(compute_waves, ldw, pieces);
}
int rpf_emul_k1_loader_prologue_wait(int rawd, int ppi) { return prologue_wait(rawd, ppi); }
int rpf_emul_k1_loader_loop_wait(int rawd, int ppi) { return loop_wait(rawd, ppi); }
int rpf_emul_k1_loader_flush_wait() { return kFlushWait; }
int rpf_emul_k1_loader_max_counted_wait() { return kMaxCountedWait; }
}
