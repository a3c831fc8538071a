// k1_stft_body.inc -- the body of K1's store kernels (rpf_kernels_stft*.hip), included by fft_stft_kernel (frame f at
// byte bN f) and fft_stft_strided_kernel (frame f at byte f * pitch): the plain kernel's frame loop (k1_body.inc) up to
// and including the last pass, phase for phase, and then the frame's spectrum itself leaves -- row f of `out`, N
// interleaved float32 (re, im) in natural bin order (include/rpf_engine.h, rpf_stft_device) -- where the plain kernel
// squares it.  No double accumulators, no flush, no partial spectra.  The includer has `pitch`: a constexpr long in
// fft_stft_kernel, the kernel argument `long pitch` in fft_stft_strided_kernel.
    constexpr int P = G::P, T = G::T, N = G::N, NPASS = G::NPASS;
    constexpr int FPW = WG / T;
    constexpr bool BLOCK_SYNC = (T > 64);
    static_assert(WG % T == 0 && WG % 64 == 0, "");
    static_assert(N - 1 + 2 * ((N - 1) >> (G::LOG2P + 1)) < G::LDS_CPX, "a staged row fits the frame slot's slab");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    cf* const slab_base = reinterpret_cast<cf*>(smem);                  // [FPW][LDS_CPX]
    uint8_t* const raw_base = smem + FPW * G::LDS_CPX * sizeof(cf);     // [WG/64][RAWD][RAW_SLOT] bytes

    const int tid = threadIdx.x;
    const int fs = tid / T, t = tid % T;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    constexpr int RAW_SLOT = raw_chunk_of(FMT) * P;
    constexpr int PIECES = P / 8 * (sample_bytes_of(FMT) / 2);
    static_assert((RAWD - 1) * PIECES <= 63, "the counted wait below: vmcnt is a 6-bit field");
    uint8_t* const wave_raw = raw_base + wave * (RAWD * RAW_SLOT);

    const long stride = static_cast<long>(gridDim.x) * FPW;
    long fb = static_cast<long>(blockIdx.x) * FPW;
    if (fb < nframes) {
#pragma unroll
        for (int d = 0; d < RAWD; ++d)
            stage_raw<G, DMA, long, FMT>(stream, fb + d * stride, nframes, pitch, wave_raw + d * RAW_SLOT, wave, lane);
    }

    cf tw[NPASS - 1][P - 1];
    load_twiddles<G, 1, TWLDS>(t, twN, tw);
    cf* const twtable = reinterpret_cast<cf*>(raw_base + (WG / 64) * RAWD * RAW_SLOT);
    if constexpr (TWLDS) {
        fill_twlds<G, 1>(tid, WG, twN, twtable);
        exchange_sync<true>();
    }
    const float sgn = (t & 1) ? -1.0f : 1.0f;
    float wsgn[P];
    if constexpr (WINDOW) {
#pragma unroll
        for (int a = 0; a < P; ++a) wsgn[a] = window[t + T * a] * sgn;
    }

    PhaseClock clk;
    cf* const slab = slab_base + fs * G::LDS_CPX;
    for (int it = 0; fb < nframes; fb += stride, ++it) {
        const bool active = (fb + fs) < nframes;
        uint8_t* const ring_slot = wave_raw + (it % RAWD) * RAW_SLOT;
        cf x[P];

        // This frame's bytes have landed.  The wave's vector-memory operations retire in the order they were issued, and
        // the row stores below are issued between the DMA instructions: with all but the newest (RAWD - 1) x PIECES
        // operations done, every DMA of this frame is done, whatever number of stores the earlier iterations issued
        // (a wave of inactive slots issues none).  The stores of the iteration before are waited for with it.
        if constexpr (DMA) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((RAWD - 1) * PIECES) : "memory");
        exchange_sync<false>();
        phase_unpack<G, WINDOW, FMT>(ring_slot + sample_bytes_of(FMT) * lane, sgn, wsgn, x);
        // the slot is refilled next: its LDS reads must have RETURNED first (k1_body.inc has the story)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        exchange_sync<false>();
        stage_raw<G, DMA, long, FMT>(stream, fb + RAWD * stride, nframes, pitch, ring_slot, wave, lane);

        // every wave is done with the slab: the read-back of the frame before this one
        exchange_sync<BLOCK_SYNC>();
        middle_passes<G, 1, 0, TWLDS>(t, x, tw, slab, clk, twtable);
        phase_fetch<G, NPASS>(t, x, slab);
        asm volatile("" : "+v"(x[0]));
        phase_last<G>(x);

        // The row leaves through the frame slot's slab (stft_core.h): every lane of the frame has fetched its last-pass
        // inputs, the bins are parked, and the row is read back in natural order, 16 bytes per lane.
        // Parked under `active`, as the plain kernel accumulates under it: the last pass then ends its basic block in both
        // kernels and compiles to the same float32 operations.  (Parked unconditionally, the 16-point last pass of 256 and
        // 4096 was compiled with three more fused multiply-adds than the plain kernel's, and the rows missed the bit
        // identity with the power by an ulp; with the branch every store kernel has its plain twin's float32 operations.)
        exchange_sync<BLOCK_SYNC>();
        if (active) {
#pragma unroll
            for (int a = 0; a < P; ++a) slab[stft_stage_index<G>(bin_of<G>(t, a))] = x[a];
        }
        exchange_sync<BLOCK_SYNC>();
        if (active) {
            cf* const row = out + static_cast<size_t>(fb + fs) * N;
#pragma unroll
            for (int i = 0; i < stft_read_rounds<G>(); ++i) {
                const int bin = stft_read_bin<G>(t, i);
                *reinterpret_cast<stft_pair_t*>(row + bin) =
                    *reinterpret_cast<const stft_pair_t*>(slab + stft_stage_index<G>(bin));
            }
        }
    }
    if constexpr (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // trailing (clamped) prefetches
