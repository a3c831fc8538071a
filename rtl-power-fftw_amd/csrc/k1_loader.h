// k1_loader.h -- the schedule of K1's loader waves (k1_body.inc, LDW > 0), stated once: the kernel compiles these
// functions and tests/test_k1_loader_schedule.py walks them on the host (tests/emul/k1_loader_emul.cpp).  Plain C++.
//
// A workgroup with loader waves has WG / 64 compute waves, which own the frames and never issue LDS-DMA, and LDW
// loader waves behind them, which do nothing else.  Loader l stages the raw bytes of the compute waves
// [l S, (l + 1) S), S = WG / 64 / LDW, into those waves' own ring slots (fft_core.h raw_source: the layout a compute
// wave would have staged for itself).  The two roles meet at the workgroup's s_barriers only, and every wave of the
// workgroup arrives at every one of them:
//
//   prologue   loader: the pieces of iterations 0 .. RAWD-1, wait(prologue_wait)      compute: twiddles, LDS table
//              ---- barrier (kPrologueBarriers: the one after fill_twlds) ----
//   iteration  compute: unpack slot_of(it), lgkmcnt(0)
//              ---- barrier 0 of the iteration, top of frame (kRefillBarrier) ----
//              loader: refill slot_of(it) with the frames of iteration refill_iteration(it), wait(loop_wait)
//              compute: pass 1
//              ---- barrier 1 of the iteration, pass-1 exchange (kLandedBarrier) ----
//              compute: the other passes, accumulate
//   flush      loader: wait(kFlushWait)
//              ---- flush_barriers(stats) barriers ----
//
// What orders the bytes: a loader's pieces complete in the order it issued them, so its counted wait leaves only the
// newest `wait` pieces outstanding; the barrier it arrives at next publishes the landed bytes to the compute waves
// (RAW), and the top-of-frame barrier, which a compute wave reaches only after its unpack reads have returned, frees
// the slot for the refill (WAR).  Frames past the end are clamped, not skipped (stage_raw), so every iteration issues
// the same number of pieces and the waits are the same constants from the first iteration to the last.
#pragma once

namespace rpf {
namespace k1_loader {

constexpr int kPrologueBarriers = 1;      // the exchange_sync<true> after fill_twlds (the loader needs TWLDS)
constexpr int kBarriersPerIteration = 2;  // top of frame, pass-1 exchange
constexpr int kRefillBarrier = 0;         // the refill is issued after this barrier of the iteration ...
constexpr int kLandedBarrier = 1;         // ... and the next iteration's bytes have landed before the loader arrives here
// the barriers of the flush: one before the accumulators are staged and one after; with statistics, per plane
constexpr int flush_barriers(bool stats) { return stats ? 6 : 2; }

// the ring slot iteration `it` unpacks, and the iteration whose frames go into it after barrier kRefillBarrier of `it`
constexpr int slot_of(int it, int rawd) { return it % rawd; }
constexpr int refill_iteration(int it, int rawd) { return it + rawd; }

// LDS-DMA instructions one loader issues per iteration: `pieces` for each compute wave it serves
constexpr int waves_served(int compute_waves, int ldw) { return compute_waves / ldw; }
constexpr int pieces_per_iteration(int compute_waves, int ldw, int pieces)
{
    return waves_served(compute_waves, ldw) * pieces;
}

// The counted waits (s_waitcnt vmcnt), in pieces of one loader that may still be outstanding.
// Prologue: iterations 0 .. rawd-1 issued, iteration 0 must have landed.
constexpr int prologue_wait(int rawd, int ppi) { return (rawd - 1) * ppi; }
// In iteration `it`, after the refill: iterations it+1 .. it+rawd are the only ones that can be outstanding (it landed
// before the previous kLandedBarrier), iteration it+1 must have landed.
constexpr int loop_wait(int rawd, int ppi) { return (rawd - 1) * ppi; }
// Before the flush reuses the LDS: nothing.
constexpr int kFlushWait = 0;
constexpr int kMaxCountedWait = 63;       // vmcnt is a 6-bit field

}  // namespace k1_loader
}  // namespace rpf
