// k1_tuning.inc -- K1's lab equipment: the experimental variants and ablations of RPF_FLAG_VARIANT(k).  Included by
// rpf_kernels.hip, inside namespace rpf { namespace {, under RPF_TUNING only: never part of the product.

// Template arguments after <N, P>: OCC, OCCW, RAWD, ABL, TWLDS, WGO, FMT, TWLDSW, KERNELS, LDW
// (k1_kernels.h, make_variant)
const Variant kTuningVariants[] = {
    // Lab equipment, compiled only into the -DRPF_TUNING build (make tuning ->
    // librpf_engine_tuning.so, used by tools/): in the shipped library every N has exactly
    // one kernel and RPF_FLAG_VARIANT(k != 0) fails rpf_engine_create with
    // RPF_ERR_INVALID_ARGUMENT.  Every variant is exact unless it says ablation.
    // (Round 2's de-phasing experiments -- alternating frame groups, skewed workgroup starts,
    // register prefetch instead of LDS-DMA -- measured slower and were removed in round 3;
    // their numbers stay in profiles/r02_k1_dephasing.txt and DESIGN.md.  So were, later, the
    // double-buffered slab (3, 26), the float32 pre-accumulate and partials (4, 22, 23, 24) and
    // the matrix-pipe first pass (60): DESIGN.md, K1, has their numbers.)
    make_variant<4096, 16, 3, 2, 2>(1),                       // all twiddles in registers
    make_variant<4096, 16, 3, 2, 1, 0, true>(2),              // one frame ahead only
    make_variant<4096, 8, 4, 4, 2>(5),                        // 8 points per lane, 512 threads
    make_variant<4096, 16, 3, 3, 2, 0, true, 768>(8),         // one 768-thread workgroup per CU, 3 frames side by side
    make_variant<4096, 16, 3, 2, 2, 0, true>(9),              // 256 threads, 3 (windowed: 2) workgroups per CU
    make_variant<4096, 16, 2, 2, 2, 0, true>(10),             // 256 threads, 2 workgroups per CU
    // round 3: deeper raw rings for HBM-resident input (one workgroup per CU leaves the LDS for it),
    // pass-2 twiddles back in registers (the 512-thread form has the registers)
    make_variant<4096, 16, 2, 2, 3, 0, true, 512>(50),
    make_variant<4096, 16, 2, 2, 4, 0, true, 512>(51),
    make_variant<4096, 16, 2, 2, 6, 0, true, 512>(52),
    make_variant<4096, 16, 2, 2, 2, 0, false, 512>(53),
    make_variant<4096, 16, 2, 2, 4, 0, false, 512>(54),
    make_variant<2048, 16, 2, 2, 4, 0, true, 512>(51),
    // loader waves behind the eight compute waves (k1_loader.h): one, and one per frame slot -- the size table's own
    // kernel under a number of its own (profiles/k1_loader.json)
    make_variant<4096, 16, 2, 2, 2, 0, true, 512, kFmtCu8, true, kK1Plain, 1>(70),
    make_variant<4096, 16, 2, 2, 2, 0, true, 512, kFmtCu8, true, kK1Plain, 2>(71),
    make_variant<4096, 16, 2, 2, 2, 0, true, 512, kFmtCu8, true, kK1Plain, 0>(72),    // no loader: variant 0 before it
    make_variant<512, 8, 4, 4, 4>(1),   make_variant<512, 8, 4, 4, 8>(2),
    make_variant<512, 16, 3, 3, 2>(3),
    make_variant<128, 8, 4, 4, 4>(3),   make_variant<256, 8, 4, 4, 4>(3),     // 8 points per lane, three passes
    make_variant<1024, 8, 4, 4, 4>(1),  make_variant<2048, 8, 4, 4, 4>(1),
    make_variant<1024, 16, 3, 3, 2>(2), make_variant<2048, 16, 3, 3, 2>(2),
    make_variant<1024, 16, 2, 2, 2, 0, true, 512>(9),
    make_variant<2048, 16, 3, 2, 2, 0, true>(9),
    make_variant<512, 8, 2, 2, 2, 0, false, 512>(9),
    make_variant<8192, 16, 2, 2, 2, 0, true>(1),
    // measurement-only ablations of the default N=4096 kernel (results are garbage)
    make_variant<4096, 16, 2, 2, 2, 1, true, 512>(31),    // no accumulate
    make_variant<4096, 16, 2, 2, 2, 2, true, 512>(32),    // no butterfly arithmetic
    make_variant<4096, 16, 2, 2, 2, 4, true, 512>(34),    // no LDS exchanges
    make_variant<4096, 16, 2, 2, 2, 8, true, 512>(38),    // no HBM staging
    make_variant<4096, 16, 2, 2, 2, 13, true, 512>(36),   // butterflies only
    make_variant<4096, 16, 2, 2, 2, 12, true, 512>(37),   // butterflies + accumulate only
};
