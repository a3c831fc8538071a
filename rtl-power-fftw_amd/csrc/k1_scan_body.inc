// k1_scan_body.inc -- the body of K1's multi-acquisition form (k1_kernels.h), included by its two kernels:
// fft_accum_scan_kernel (up to kMaxHops hops, tables in lanes: HopLanes) and fft_accum_series_kernel (a uniform series
// of spectra cut from one stream, arithmetic table: series_partition.h).  The includer declares `using TABLE`, the type
// that answers it_begin / nframes / stream / hop_of, and `constexpr bool SERIES`; its kernel argument `hops` is what
// TABLE::load takes and carries q, r and step.  An include rather than a force-inlined device function, as k1_body.inc:
// the scan kernel compiles to the instruction stream it had before the series form existed (tools/kernel_streams.py).
// What SERIES changes is where a segment goes (the hand-over below): a complete spectrum straight to its output row,
// a cut one to partial slot 2w or 2w + 1.  The includer also declares `constexpr bool STATS` (true in
// fft_accum_series_stats_kernel alone): the per-bin statistics of k1_body.inc beside the power, and rows and slots of
// three planes each.  With it false nothing below changes what the two other kernels compile to.
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
    constexpr int RAW_SLOT = raw_chunk_of(FMT) * P;   // bytes one wave stages per frame
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

    // This workgroup's iterations: `count` of them, `step` apart from `first` on (hop_partition.h).
    // The host launches at most one workgroup per iteration (launch_fft_accum checks it), so
    // count >= 1 -- deliberately not tested here: a branch on q and r would put their scalar
    // load in front of the table loads instead of beside them.
    TABLE tbl;
    tbl.load(hops);
    const int step = hops.step;
    int first, count;
    hop_share(static_cast<int>(blockIdx.x), hops.q, hops.r, step, &first, &count);

    // First thing: get the first iterations' bytes moving (HBM latency overlaps the constant
    // loads below).  The staging cursor `ahead` runs RAWD iterations in front of the compute
    // cursor, across hop boundaries; every iteration issues PIECES DMAs.  The frame loop sees
    // of it only a frame index that advances and a countdown: `ahead_run` stagings stay inside
    // the hop the cursor stands in (scans have step = 1, an interleaved single acquisition
    // never leaves its hop), then ahead_turn() moves the cursor on -- or, when nothing is left
    // to stage, parks it on the launch's iteration 0 with no advance: the same 2N FPW bytes
    // for every workgroup, an L2 hit, so the surplus (never read) stagings that keep the DMA
    // count per iteration constant cost no memory traffic.
    const int fstep = FPW * step;                  // frames between a workgroup's iterations
    HopCursor ahead;
    ahead.seek(tbl, first);
    int ahead_fb = (ahead.j - ahead.begin) * FPW, ahead_fstep = fstep;
    int ahead_left = count;                        // real iterations not staged yet
    auto run_length = [&](const HopCursor& c, int left) {
        const int in_hop = step == 1 ? c.end - c.j : left;
        return in_hop < left ? in_hop : left;
    };
    int ahead_run = run_length(ahead, ahead_left);
    ahead_left -= ahead_run;
    auto ahead_turn = [&]() {
        if (ahead_left > 0) {
            ahead.seek(tbl, ahead.end);            // (step == 1 here: the next hop starts where this one ended)
            ahead_fb = 0;
            ahead_run = run_length(ahead, ahead_left);
            ahead_left -= ahead_run;
        } else {
            ahead.seek(tbl, 0);
            ahead_fb = 0;
            ahead_fstep = 0;
            ahead_run = 0x7fffffff;
        }
    };
    auto stage_next = [&](uint8_t* dst) {
        stage_raw<G, DMA, int, FMT, SBATCH>(ahead.stream, ahead_fb, ahead.nframes,
                                            static_cast<long>(sample_bytes_of(FMT)) * G::N, dst, wave, lane);
        ahead_fb += ahead_fstep;
        if (--ahead_run == 0) ahead_turn();
    };
    if constexpr (!(ABL & 8)) {
#pragma unroll
        for (int d = 0; d < RAWD; ++d) stage_next(wave_raw + d * RAW_SLOT);
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
    // STATS: the sum of the squared powers and the peak power of every bin beside acc (fft_core.h,
    // phase_accumulate_stats), zeroed with it at every spectrum; the peak starts from 0, which no power is below.
    static_assert(!STATS || (SERIES && ABL == 0), "the statistics: series kernels only, no ablations");
    double acc_s2[STATS ? P : 1], acc_pk[STATS ? P : 1];

    PhaseClock clk;
    clk.start();
    HopCursor cur;
    cur.seek(tbl, first);
    int it = 0;                                    // iterations done: the ring slot
    while (true) {
        // ---- one segment: this workgroup's iterations inside hop cur.h ------------------------
        const int seg = run_length(cur, count - it);
#pragma unroll
        for (int a = 0; a < P; ++a) acc[a] = 0.0;
        if constexpr (STATS) {
#pragma unroll
            for (int a = 0; a < P; ++a) acc_s2[a] = acc_pk[a] = 0.0;
        }
        int fb = (cur.j - cur.begin) * FPW;        // slot-0 frame of the iteration, within the hop
        for (int n = seg; n > 0; --n, ++it, fb += fstep) {
            const bool active = (fb + fs) < cur.nframes;
            cf* const slab = slab_base + fs * G::LDS_CPX;
            uint8_t* const ring_slot = wave_raw + (it % RAWD) * RAW_SLOT;
            cf x[P];

            // this iteration's bytes have landed: every iteration issues exactly PIECES DMA
            // instructions per wave, so all but the newest (RAWD-1) iterations' worth are done
            if constexpr (DMA && !(ABL & 8))
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"((RAWD - 1) * PIECES) : "memory");
            exchange_sync<false>();
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
            exchange_sync<false>();
            RPF_STAMP(clk, 1);                   // unpack
            // the slot has been consumed: refill it with the iteration RAWD ahead
            if constexpr (!(ABL & 8)) stage_next(ring_slot);
            RPF_STAMP(clk, 3);                   // DMA issue

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
                if (active) phase_accumulate_stats(x, acc, acc_s2, acc_pk, P);   // (an inactive slot leaves the peak alone)
            } else {
                if (active) phase_accumulate(x, acc, P);
            }
            RPF_STAMP(clk, 14);                      // accumulate
        }

        // ---- hand the segment over: one partial spectrum (the FPW frame slots summed) ----------
        // The accumulators go through the slab (free between frames; the raw ring with its
        // in-flight prefetches is not touched) so that the bin-scattered registers leave as
        // fully coalesced 512-byte rows: stage at a padded bin index (one spare double per
        // 16, conflict-free for the stride-16 bin pattern of bin_of), then stream out.
        exchange_sync<true>();
        double* const stage = reinterpret_cast<double*>(smem);          // [FPW][N + N/16]
        constexpr int SN = N + N / 16;
        static_assert(sizeof(double) * SN <= sizeof(cf) * G::LDS_CPX, "the stage stays inside the slab");
        // (opaque copies of the thread indices: the hand-over runs once per hop, its sixteen
        // stage addresses must not be hoisted into registers that live across the frame loop)
        int ft = t, ftid = tid, ffs = fs;
        asm volatile("" : "+v"(ft), "+v"(ftid), "+v"(ffs));
        if constexpr (STATS) {
            // Three planes per row or slot, S1, S2, PK at p N: one after the other through the same staging area, the
            // frame slots combined by +, +, max (stats_combine), plane 0 exactly as the plain hand-over below.
            const int w = static_cast<int>(blockIdx.x);
            double* const row3 = series_segment_complete(cur.j, first + it, cur.begin, cur.end)
                                     ? series_rows(hops) + static_cast<size_t>(cur.h) * (kStatsPlanes * N)
                                     : partial + static_cast<size_t>(series_segment_slot(w, cur.j, cur.begin)) * (kStatsPlanes * N);
#pragma unroll
            for (int plane = 0; plane < kStatsPlanes; ++plane) {
                if (plane > 0) exchange_sync<true>();     // every wave has read the previous plane
                const double* const src = plane == 0 ? acc : plane == 1 ? acc_s2 : acc_pk;
#pragma unroll
                for (int a = 0; a < P; ++a) {
                    const int bin = bin_of<G>(ft, a);
                    stage[ffs * SN + bin + (bin >> 4)] = src[a];
                }
                exchange_sync<true>();
                for (int bin = 2 * ftid; bin < N; bin += 2 * WG) {
                    partial2_t v = {0.0, 0.0};
#pragma unroll
                    for (int k = 0; k < FPW; ++k) {
                        v.x = stats_combine(plane, v.x, stage[k * SN + bin + (bin >> 4)]);
                        v.y = stats_combine(plane, v.y, stage[k * SN + bin + 1 + (bin >> 4)]);
                    }
                    store_partial2(row3 + plane * N + bin, v);
                }
            }
        } else {
#pragma unroll
            for (int a = 0; a < P; ++a) {
                const int bin = bin_of<G>(ft, a);
                stage[ffs * SN + bin + (bin >> 4)] = acc[a];
            }
            exchange_sync<true>();
            size_t slot = 0;
            double* row = nullptr;           // SERIES: where this segment goes
            if constexpr (SERIES) {
                // (cur.j is still the segment's first iteration; first + it the one after its last)
                const int w = static_cast<int>(blockIdx.x);
                row = series_segment_complete(cur.j, first + it, cur.begin, cur.end)
                          ? series_rows(hops) + static_cast<size_t>(cur.h) * N
                          : partial + static_cast<size_t>(series_segment_slot(w, cur.j, cur.begin)) * N;
            } else {
                slot = static_cast<size_t>(tbl.slot_bias(cur.h) + static_cast<int>(blockIdx.x));
            }
            // two neighbouring bins per lane = one 16-byte store: an 8-byte-per-lane store tail is
            // issue-bound at ~7 B/clk/CU (MI355X_MICROARCH.md), and every workgroup ends in one.
            // Written through (store_partial2), as K1's flush.
            for (int bin = 2 * ftid; bin < N; bin += 2 * WG) {
                partial2_t v = {0.0, 0.0};
#pragma unroll
                for (int k = 0; k < FPW; ++k) {
                    v.x += stage[k * SN + bin + (bin >> 4)];
                    v.y += stage[k * SN + bin + 1 + (bin >> 4)];
                }
                if constexpr (SERIES)
                    store_partial2(row + bin, v);
                else
                    store_partial2(partial + slot * N + bin, v);
            }
        }
        if (it >= count) break;
        // next hop: the slab is reused by its first frame once every wave has read the stage
        exchange_sync<true>();
        cur.seek(tbl, cur.end);                    // (a segment that is not the last ends with its hop)
    }
    clk.publish(lane);
    if constexpr (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // trailing (repeated) prefetches
