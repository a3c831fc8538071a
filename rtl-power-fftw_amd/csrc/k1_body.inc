// k1_body.inc -- the body of K1 (rpf_kernels.hip), included by its two kernels: fft_accum_kernel (frame f at byte
// 2N f) and fft_accum_strided_kernel (frame f at byte f * pitch, overlapped frames).  The includer declares
// `constexpr bool STRIDED` and `pitch`: a constexpr long in the plain kernel, the kernel argument `long pitch` in the
// strided one.  An include rather than a force-inlined device function: the plain kernels then compile to the
// instruction stream they had before the strided form existed (an inlined body changed their schedules).  `STATS` (a
// template argument of both, false everywhere but in rpf_kernels_stats*.hip) adds the per-bin statistics; with it
// false nothing below changes what the plain kernels compile to (tools/kernel_streams.py compares the instruction
// streams of two builds).
    RPF_SEAM_MARK(0);                            // (timing builds only)
    constexpr int P = G::P, T = G::T, N = G::N, NPASS = G::NPASS;
    constexpr int FPW = WG / T;
    constexpr bool BLOCK_SYNC = (T > 64);
    static_assert(WG % T == 0 && WG % 64 == 0, "");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    cf* const slab_base = reinterpret_cast<cf*>(smem);                        // [FPW][LDS_CPX]
    uint8_t* const raw_base = smem + FPW * G::LDS_CPX * sizeof(cf);          // [WG/64][RAWD][RAW_SLOT] bytes

    const int tid = threadIdx.x;
    const int fs = tid / T, t = tid % T;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    constexpr int RAW_SLOT = raw_chunk_of(FMT) * P;   // bytes one wave stages per frame (FMT: the sample format)
    constexpr int PIECES = P / 8 * (sample_bytes_of(FMT) / 2);   // DMA instructions per wave per frame
    // WREG: the window values stay in registers across the frame loop, and a frame's raw bytes are staged all at once.
    // Everywhere but in the windowed VGPR-staging cf32 kernels with statistics at P = 16, where eight 16-byte loads in
    // flight, three double accumulators per bin and the window are more than 256 registers: those read the P window values
    // again for every frame (L1 hits; the same products, so the same bits) and stage in two batches (stage_raw,
    // BATCH).  With WREG true -- every other instantiation -- nothing here changes what the kernel compiles to.
    constexpr bool WREG = !(FMT == kFmtCf32 && STATS && !DMA && WINDOW && P == 16);
    constexpr int SBATCH = WREG ? 0 : P / 4;
    static_assert((RAWD - 1) * PIECES <= 63, "the counted wait below: vmcnt is a 6-bit field");
    uint8_t* const wave_raw = raw_base + wave * (RAWD * RAW_SLOT);

    // First thing: get the first frames' bytes moving (HBM latency overlaps the
    // constant loads below).  RAWREG keeps the next frame's 2P bytes per lane in
    // VGPRs instead of issuing LDS-DMA (two global_load_dwordx4 cost a few issue
    // cycles, an LDS-DMA instruction ~100-200).
    const long stride = static_cast<long>(gridDim.x) * FPW;
    long fb = static_cast<long>(blockIdx.x) * FPW;
    // LDW > 0: loader waves behind the WG / 64 compute waves stage every frame's bytes, and the compute waves issue no
    // LDS-DMA and wait for none; the two roles meet at the workgroup's barriers only (k1_loader.h has the schedule).
    static_assert(LDW == 0 || (DMA && TWLDS && BLOCK_SYNC && !STRIDED && !STATS && ABL == 0 && (WG / 64) % LDW == 0),
                  "the loader takes the place of the LDS-DMA of a kernel with the barriers of k1_loader.h");
    if constexpr (LDW > 0) {
        if (wave >= WG / 64) {
            constexpr int SERVED = k1_loader::waves_served(WG / 64, LDW);
            constexpr int PPI = k1_loader::pieces_per_iteration(WG / 64, LDW, PIECES);
            static_assert(k1_loader::prologue_wait(RAWD, PPI) <= k1_loader::kMaxCountedWait &&
                          k1_loader::loop_wait(RAWD, PPI) <= k1_loader::kMaxCountedWait, "vmcnt is a 6-bit field");
            const int w0 = (wave - WG / 64) * SERVED;      // the compute waves this loader stages for
            if (fb < nframes) {
#pragma unroll
                for (int d = 0; d < RAWD; ++d)
#pragma unroll
                    for (int k = 0; k < SERVED; ++k)
                        stage_raw<G, DMA, long, FMT>(stream, fb + d * stride, nframes, pitch,
                                                     raw_base + (w0 + k) * (RAWD * RAW_SLOT) + d * RAW_SLOT, w0 + k, lane);
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(k1_loader::prologue_wait(RAWD, PPI)) : "memory");
            }
#pragma unroll
            for (int b = 0; b < k1_loader::kPrologueBarriers; ++b) exchange_sync<true>();
            for (int it = 0; fb < nframes; fb += stride, ++it) {
                static_assert(k1_loader::kBarriersPerIteration == 2 && k1_loader::kRefillBarrier == 0 &&
                              k1_loader::kLandedBarrier == 1, "the two barriers of the frame loop below");
                exchange_sync<true>();                   // top of frame: every compute wave's unpack reads have returned
                const int slot = k1_loader::slot_of(it, RAWD);
#pragma unroll
                for (int k = 0; k < SERVED; ++k)
                    stage_raw<G, DMA, long, FMT>(stream, fb + (k1_loader::refill_iteration(it, RAWD) - it) * stride, nframes,
                                                 pitch, raw_base + (w0 + k) * (RAWD * RAW_SLOT) + slot * RAW_SLOT, w0 + k, lane);
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(k1_loader::loop_wait(RAWD, PPI)) : "memory");
                exchange_sync<true>();                   // pass-1 exchange: the next iteration's bytes have landed
            }
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(k1_loader::kFlushWait) : "memory");   // nothing lands in the flush's LDS
#pragma unroll
            for (int b = 0; b < k1_loader::flush_barriers(STATS); ++b) exchange_sync<true>();
            return;
        }
    }
    if (LDW == 0 && fb < nframes) {
#pragma unroll
        for (int d = 0; d < RAWD; ++d)
            stage_raw<G, DMA, long, FMT, SBATCH>(stream, fb + d * stride, nframes, pitch, wave_raw + d * RAW_SLOT, wave, lane);
    }

    // Loop-invariant per-thread constants: twiddles, sign, window.
    cf tw[NPASS - 1][P - 1];
    load_twiddles<G, 1, TWLDS>(t, twN, tw);
    cf* const twtable = reinterpret_cast<cf*>(raw_base + (WG / 64) * RAWD * RAW_SLOT);
    if constexpr (TWLDS) {
        fill_twlds<G, 1>(tid, WG, twN, twtable);
        exchange_sync<true>();
    }
    const float sgn = (t & 1) ? -1.0f : 1.0f;
    float wsgn[P];
    if constexpr (WINDOW && WREG) {
#pragma unroll
        for (int a = 0; a < P; ++a) wsgn[a] = window[t + T * a] * sgn;
    }
    double acc[P];
#pragma unroll
    for (int a = 0; a < P; ++a) acc[a] = 0.0;
    // STATS: the sum of the squared powers and the peak power of every bin beside acc (fft_core.h,
    // phase_accumulate_stats); the peak starts from 0, which no power is below.
    static_assert(!STATS || ABL == 0, "the ablations do not combine with the statistics");
    double acc_s2[STATS ? P : 1], acc_pk[STATS ? P : 1];
    if constexpr (STATS) {
#pragma unroll
        for (int a = 0; a < P; ++a) acc_s2[a] = acc_pk[a] = 0.0;
    }

    PhaseClock clk;
    clk.start();
    for (int it = 0; fb < nframes; fb += stride, ++it) {
        const bool active = (fb + fs) < nframes;
        cf* const slab = slab_base + fs * G::LDS_CPX;
        uint8_t* const ring_slot = wave_raw + (it % RAWD) * RAW_SLOT;
        cf x[P];

        {
            // this frame's bytes have landed: every iteration issues exactly PIECES DMA
            // instructions per wave, so all but the newest (RAWD-1) frames' worth are done
            // (LDW > 0: they landed before the loader arrived at the barrier this wave passed last)
            if constexpr (DMA && !(ABL & 8) && LDW == 0)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"((RAWD - 1) * PIECES) : "memory");
            if constexpr (LDW == 0) exchange_sync<false>();
            RPF_STAMP(clk, 0);                   // waiting for the staged bytes
            if constexpr (WINDOW && !WREG) {
                const float* wp = window + t;
                asm volatile("" : "+v"(wp));      // (opaque: the loads stay inside the frame loop)
#pragma unroll
                for (int a = 0; a < P; ++a) wsgn[a] = wp[T * a] * sgn;
            }
            phase_unpack<G, WINDOW, FMT>(ring_slot + sample_bytes_of(FMT) * lane, sgn, wsgn, x);
            // The slot is refilled next: its LDS reads must have RETURNED first (a DMA
            // that hits in L2/MALL can land before queued LDS reads execute -- seen as
            // sporadic 1e-3 errors), so wait for this wave's LDS reads, not just issue.
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if constexpr (LDW == 0) exchange_sync<false>();
            RPF_STAMP(clk, 1);                   // unpack
#ifdef RPF_PHASE_TIMING
            if (it == 0) RPF_SEAM_MARK(1);
#endif
            // the slot has been consumed: refill it with the frame RAWD iterations ahead (LDW > 0: the loader does,
            // behind the top-of-frame barrier below)
            if constexpr (!(ABL & 8) && LDW == 0)
                stage_raw<G, DMA, long, FMT, SBATCH>(stream, fb + RAWD * stride, nframes, pitch, ring_slot, wave, lane);
            RPF_STAMP(clk, 3);                   // DMA issue
        }

        // one slab: every wave must be done with the previous frame's slab
        exchange_sync<BLOCK_SYNC>();
        RPF_STAMP(clk, 2);                       // top-of-frame barrier
        middle_passes<G, 1, ABL, TWLDS>(t, x, tw, slab, clk, twtable);   // stamps 4J..4J+3
        if constexpr (!(ABL & 4)) phase_fetch<G, NPASS>(t, x, slab);
        asm volatile("" : "+v"(x[0]));
        RPF_STAMP(clk, 12);                      // last fetch
        if constexpr (!(ABL & 2)) phase_last<G>(x);
        RPF_STAMP(clk, 13);                      // last butterfly
        if constexpr (ABL & 1) {
#pragma unroll
            for (int a = 0; a < P; ++a) asm volatile("" ::"v"(x[a]));
        } else if constexpr (STATS) {
            if (active) phase_accumulate_stats(x, acc, acc_s2, acc_pk, P);     // (an inactive slot leaves the peak alone)
        } else {
            if (active) phase_accumulate(x, acc, P);
        }
        RPF_STAMP(clk, 14);                      // accumulate
    }
    RPF_SEAM_MARK(2);
    if constexpr (DMA && LDW == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // trailing (clamped) prefetches

    // One partial spectrum per workgroup (the FPW frame slots are summed here);
    // every workgroup writes its partial, zeros included.  The accumulators go
    // through LDS (now free) so that the bin-scattered registers leave as fully
    // coalesced 512-byte rows: stage at a padded bin index (one spare double per
    // 16, conflict-free for the stride-16 bin pattern of bin_of), then stream out.
    exchange_sync<true>();
    double* const stage = reinterpret_cast<double*>(smem);          // [FPW][N + N/16]
    constexpr int SN = N + N / 16;
    static_assert(sizeof(double) * SN <= sizeof(cf) * G::LDS_CPX + 2 * N, "stage fits the LDS");
    if constexpr (STATS) {
        // Three planes per workgroup, partial[(3 w + plane) N ..): S1, S2, PK, one after the other through the same
        // staging area; the frame slots combine by +, +, max (stats_combine), plane 0 exactly as the plain flush.
#pragma unroll
        for (int plane = 0; plane < kStatsPlanes; ++plane) {
            if (plane > 0) exchange_sync<true>();         // every wave has read the previous plane
            const double* const src = plane == 0 ? acc : plane == 1 ? acc_s2 : acc_pk;
#pragma unroll
            for (int a = 0; a < P; ++a) {
                const int bin = bin_of<G>(t, a);
                stage[fs * SN + bin + (bin >> 4)] = src[a];
            }
            exchange_sync<true>();
            double* const out = partial + (static_cast<size_t>(blockIdx.x) * kStatsPlanes + plane) * N;
            for (int bin = 2 * tid; bin < N; bin += 2 * WG) {
                partial2_t v = {0.0, 0.0};
#pragma unroll
                for (int k = 0; k < FPW; ++k) {
                    v.x = stats_combine(plane, v.x, stage[k * SN + bin + (bin >> 4)]);
                    v.y = stats_combine(plane, v.y, stage[k * SN + bin + 1 + (bin >> 4)]);
                }
                store_partial2(out + bin, v);
            }
        }
    } else {
#pragma unroll
        for (int a = 0; a < P; ++a) {
            const int bin = bin_of<G>(t, a);
            stage[fs * SN + bin + (bin >> 4)] = acc[a];
        }
        exchange_sync<true>();
        // two neighbouring bins per lane = one 16-byte store: an 8-byte-per-lane store tail is
        // issue-bound at ~7 B/clk/CU (MI355X_MICROARCH.md), and every workgroup ends in one.
        // Written through (store_partial2): 32 KB per workgroup that K3 reads from another XCD.
        for (int bin = 2 * tid; bin < N; bin += 2 * WG) {
            partial2_t v = {0.0, 0.0};
#pragma unroll
            for (int k = 0; k < FPW; ++k) {
                v.x += stage[k * SN + bin + (bin >> 4)];
                v.y += stage[k * SN + bin + 1 + (bin >> 4)];
            }
            store_partial2(partial + static_cast<size_t>(blockIdx.x) * N + bin, v);
        }
    }
    RPF_SEAM_DRAIN();
    RPF_SEAM_MARK(3);
    clk.publish(lane);                           // (timing builds: its atomics after the marks)
