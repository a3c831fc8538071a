"""The row-store and pair kernels below one tile of bins and past one chunk of them, on the MI355X.

Every kernel that post-processes spectra partitions the bins by a constant of its own: the 64-bin tile of the quantile
selection, of the correlator's X-engine and of the excised average, the 32-bin block of the dedispersion, the
32768-bin state chunk of the quantile selection, the 2^18 / N row groups of the excised average, the 64 MB rows chunk of
the cross-spectrum.  The family modules drive them at 64 .. 8192 bins (and a few sizes beside); this module drives them
where a tile has dead lanes, where the chunk loop runs a second and a third time, where there is one row group, two, or
131072 of them, and where a rows chunk is a few frames.

Nothing here is judged by a bar of its own.  Every comparison is the one its family module makes, through that
module's helpers: equality of doubles with stats.quantiles / dedisperse.reference of the engine's own rows, mask and
kept exact and clean / total at ADDITIVITY for the excised average, bit identity with the definition for the
cross-spectrum, the terms of the device's own rows for the correlator.  The rows themselves come from the series entries
on the spectrum-by-spectrum route at all of these sizes, so for every new N of sections 1 to 3 row k is first held,
bit for bit, to rpf_accumulate_device of the same engine on the frames [k L, (k + 1) L).  Each test prints the figures
it judged."""
import os
import re

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, dedisperse, stats, synth
from helpers import ROOT, max_rel
from parity_bars import ADDITIVITY
from test_correlate import emul as correlate_emul
from test_dedisperse import DT, TT, direct_share, same_bits
from test_dedisperse_edge_sizes import expected_direct_pairs
from test_excise import err_over_total
from test_seams import QUANTILE_CHUNK, gather_chunk
from test_gpu_correlate import (Resident, check_against_rows as correlate_check, check_layout, corr, device_rows,
                                engine as correlate_engine, rows_case, streams_of)
from test_gpu_cross import (ADDITIVITY as CROSS_ADDITIVITY, cf32, cross_run, engine as cross_engine,  # noqa: F401 (cf32: a fixture)
                            identity_case, in_units_of_the_powers)
from test_gpu_dedisperse import fill, make_table, make_weights
from test_gpu_excise import (check_against_rows as excise_check, engine as excise_engine, excised,
                             series_rows as stats_rows, truth_rows)
from test_gpu_quantile import (Q8, check_against_rows as quantile_check, current, engine, noise, same, select_device,
                               series_rows, to_device)
from test_gpu_sample_formats import device_run
from test_gpu_series import slice_rows
from test_gpu_series_stats import slice_rows as stats_slice_rows

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")


# ---- the rows are on tested ground ---------------------------------------------------------------------------------------

def rows_equal_the_slices(ds, stream, L, K, what):
    """Row k of rpf_accumulate_device_series equals rpf_accumulate_device on the frames [k L, (k + 1) L), bit for bit:
    the spectrum-by-spectrum route makes the same launches.  Returns the rows."""
    rows, launches = series_rows(ds, to_device(stream), stream.size, L, K)
    want = slice_rows(ds, stream, L, K)
    differ = int(np.count_nonzero(~((rows == want) | (np.isnan(rows) & np.isnan(want)))))
    print("%s: L=%d K=%d launches=%d: %d of %d row values differ from rpf_accumulate_device on the row's frames"
          % (what, L, K, launches, differ, rows.size))
    assert launches == K, what                                      # spectrum by spectrum
    assert same(rows, want), what
    return rows


def stats_rows_equal_the_slices(ds, stream, L, K, what):
    """The same for a stats engine: S1, S2, PK of row k against rpf_accumulate_device_stats on the row's frames, and S1
    against rpf_accumulate_device, all bit for bit."""
    rows, launches = stats_rows(ds, to_device(stream), stream.size, L, K)
    want = stats_slice_rows(ds, stream, L, K)
    plain = slice_rows(ds, stream, L, K)
    differ = [int(np.count_nonzero(rows[:, p] != want[:, p])) for p in range(3)]
    print("%s: L=%d K=%d launches=%d: S1 / S2 / PK differ from rpf_accumulate_device_stats on the row's frames in %s of %d, "
          "S1 from rpf_accumulate_device in %d" % (what, L, K, launches, differ, K * ds.params.N,
                                                   int(np.count_nonzero(rows[:, 0] != plain))))
    assert launches == K, what
    assert np.array_equal(rows, want), what
    assert np.array_equal(rows[:, 0], plain), what
    return rows


# ---- 1. quantile selection below one tile ----------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K", [(2, 1), (2, 2), (2, 37), (6, 37), (34, 37), (62, 37)])
def test_quantiles_below_one_tile(N, K):
    """One tile with 62 .. 2 dead lanes (34: the second wave half holds two bins): `live` and `bb < cb` do real work."""
    L = 1
    stream = noise("cu8", 200 + N + K, N * K * L)
    with engine(N) as ds:
        rows_equal_the_slices(ds, stream, L, K, "N=%d" % N)
        quantile_check(ds, stream, L, K, "N=%d K=%d" % (N, K), K)    # (no K1 size: K launches)


# ---- 2. quantile selection past one chunk of bins ----------------------------------------------------------------------------

def bin_chunks(N):
    return [(b0, min(b0 + QUANTILE_CHUNK, N)) for b0 in range(0, N, QUANTILE_CHUNK)]


def check_chunk_by_chunk(got, rows, what):
    """got against stats.quantiles of the rows, one chunk of bins at a time: a failure says where it is."""
    wrong = []
    for c, (b0, b1) in enumerate(bin_chunks(rows.shape[1])):
        want = stats.quantiles(rows[:, b0:b1], Q8)
        part = got[:, b0:b1]
        n = int(np.count_nonzero(~((part == want) | (np.isnan(part) & np.isnan(want)))))
        print("%s: chunk %d, bins [%d, %d): %d of %d values differ from stats.quantiles of the engine's rows"
              % (what, c, b0, b1, n, want.size))
        if n:
            wrong.append("chunk %d (bins [%d, %d)): %d of %d values" % (c, b0, b1, n, want.size))
    assert not wrong, "%s: differs from stats.quantiles in %s" % (what, "; ".join(wrong))


def stored(ds, stream, L, K):
    """The selection of Q8 after the stream's K rows were appended to an empty store."""
    d = to_device(stream)
    ds.quantile_reset()
    assert ds.quantile_append_device(d.data_ptr(), stream.size, L, K, current()) == K and ds.quantile_rows == K
    return select_device(ds, Q8)


@pytest.mark.parametrize("N,chunks", [(32770, [32768, 2]), (40010, [32768, 7242]), (65536, [32768, 32768]),
                                      (65538, [32768, 32768, 2])])
def test_quantiles_past_one_chunk(N, chunks):
    """32770: the second chunk is one tile with two live lanes; 40010: a ragged last tile of 10; 65536: two full chunks;
    65538: three chunks, the last of 2 bins."""
    L, K = 1, 9
    assert [b1 - b0 for b0, b1 in bin_chunks(N)] == chunks
    stream = noise("cu8", 300 + N % 97, N * K * L)
    assert stream.size < 1200000
    with engine(N) as ds:
        rows = rows_equal_the_slices(ds, stream, L, K, "N=%d" % N)
        check_chunk_by_chunk(stored(ds, stream, L, K), rows, "N=%d" % N)
        quantile_check(ds, stream, L, K, "N=%d" % N, K)


def test_exact_ties_past_one_chunk():
    """Frames A B A B ... A at 65536 bins: every bin holds two values, 6 and 5 times: the `tie` branch of the narrow
    kernel in a chunk with bin0 > 0."""
    N, L, K = 65536, 1, 11
    two = synth.noise_tones_iq(371, 2 * N).reshape(2, 2 * N)
    stream = np.ascontiguousarray(two[np.arange(K) % 2]).reshape(-1)
    with engine(N) as ds:
        rows = rows_equal_the_slices(ds, stream, L, K, "N=%d ties" % N)
        assert np.all(rows[0::2] == rows[0]) and np.all(rows[1::2] == rows[1])
        assert np.count_nonzero(rows[0, QUANTILE_CHUNK:] != rows[1, QUANTILE_CHUNK:]) > QUANTILE_CHUNK // 2
        got = stored(ds, stream, L, K)
        check_chunk_by_chunk(got, rows, "N=%d ties" % N)
        lo, hi = np.minimum(rows[0], rows[1]), np.maximum(rows[0], rows[1])
        assert same(got[0], lo) and same(got[7], hi) and np.all((got == lo) | (got == hi))


def test_a_nan_sample_past_one_chunk():
    """cf32 at 65536 bins, one NaN sample in integration 5: it is the largest value of every bin of both chunks, and
    q = 0.99 interpolates towards it (the `above` pass in a chunk with bin0 > 0)."""
    N, L, K = 65536, 1, 9
    z = synth.gaussian_cf32(381, N * K * L, sigma=20.0).copy()
    z[5 * L * N + 40000] = np.nan
    stream = z.view(np.uint8).reshape(-1)
    with engine(N, "cf32") as ds:
        rows = rows_equal_the_slices(ds, stream, L, K, "N=%d cf32 NaN" % N)
        assert np.all(np.isnan(rows[5])) and not np.isnan(np.delete(rows, 5, axis=0)).any()
        got = stored(ds, stream, L, K)
        check_chunk_by_chunk(got, rows, "N=%d cf32 NaN" % N)
        # nine rows: q <= 0.75 lies at or below v_(6); 0.9, 0.99 and 1 reach v_(8), the NaN
        assert np.all(np.isnan(got[5:])) and not np.isnan(got[:5]).any()


# ---- 3. the excised average with one row group, two, and very many -----------------------------------------------------------

EXCISE = {          # N: (L, K, G, seed)
    2: (2, 600, 131072, 11),              # tiny N, huge G: one bin pair per 64-bin block
    6: (3, 200, 43690, 12),               # G no multiple of the 8 groups of a block: a ragged group tile
    131072: (2, 7, 2, 13),                # 3 and 4 rows per group
    200000: (2, 5, 1, 14),                # one group, no power of two
    262144: (2, 12, 1, 15),               # one group and a piece seam (excise_pieces)
}


def excise_groups(N):
    src = open(os.path.join(ROOT, "rtl-power-fftw_amd", "csrc", "excise_core.h")).read()
    m = re.search(r"constexpr int kExciseGroupBins = 1 << (\d+);", src)
    assert m
    return max(1, (1 << int(m.group(1))) // N)


def excise_pieces(N, K):
    """(rows per piece, pieces) of a call of K rows: as many rows of 3 N doubles as fit kExciseRowBytes, at least one."""
    src = open(os.path.join(ROOT, "rtl-power-fftw_amd", "csrc", "rpf_engine.cpp")).read()
    m = re.search(r"constexpr size_t kExciseRowBytes = static_cast<size_t>\((\d+)\) << (\d+);", src)
    assert m and "kExciseRowBytes / (sizeof(double) * rpf::kStatsPlanes * e->N)" in src
    cap = max(1, (int(m.group(1)) << int(m.group(2))) // (8 * 3 * N))
    return cap, -(-K // cap)


def excise_stream(N):
    L, K, _, seed = EXCISE[N]
    return noise("cu8", seed, N * K * L)


@pytest.mark.parametrize("N", [2, 6])
def test_the_tiny_streams_take_both_branches_in_float64(N):
    """What check_against_rows requires of a stream (0 < flagged < all at 1 sigma), on a float64 model of the rows: if
    this fails the seed is wrong, not the kernel."""
    L, K, _, _ = EXCISE[N]
    lo, hi = stats.sk_limits(L, 1.0)
    _, mask = stats.excise(truth_rows(excise_stream(N), N, L, K), L, lo, hi)
    print("N=%d L=%d K=%d: the float64 model flags %d of %d pairs at 1 sigma" % (N, L, K, int(mask.sum()), mask.size))
    assert K * N // 10 < mask.sum() < 9 * K * N // 10


@pytest.mark.parametrize("N", sorted(EXCISE))
def test_excised_average_at_every_group_count(N):
    L, K, G, _ = EXCISE[N]
    assert excise_groups(N) == G
    stream = excise_stream(N)
    with excise_engine(N) as ds:
        stats_rows_equal_the_slices(ds, stream, L, K, "N=%d" % N)
        excise_check(ds, stream, L, K, "N=%d G=%d" % (N, G), K)      # (spectrum by spectrum: K launches)


def test_the_second_piece_continues_the_one_accumulator():
    """N = 262144: a row of statistics is 6 MB, a piece holds 10 and K = 12 is two pieces; with G = 1 the second piece
    goes on from the state the first left (first == 0).  The host entry cuts the same pieces: its bits are the device
    entry's."""
    N = 262144
    L, K, G, _ = EXCISE[N]
    cap, pieces = excise_pieces(N, K)
    assert G == 1 and K == cap + 2 and pieces == 2
    stream = excise_stream(N)
    lo, hi = stats.sk_limits(L, 1.0)
    with excise_engine(N) as ds:
        d = to_device(stream)
        dev, dmask, dk = excised(ds, d, stream.size, L, lo, hi)
        assert ds.series_launches() == K
        head, hmask, hk = excised(ds, d, stream.size, L, lo, hi, max_spectra=cap)        # the first piece alone
        rows, _ = stats_rows(ds, d, stream.size, L, K)
        host, host_mask, host_k = ds.accumulate_excised(stream, L, lo, hi, want_mask=True)
        assert ds.series_launches() == K
    assert dk == host_k == K and hk == cap
    want, want_mask = stats.excise(rows, L, lo, hi)
    tail, tail_mask = stats.excise(rows[cap:], L, lo, hi)
    e_clean, e_total = err_over_total(dev[0], want[0], want[2]), err_over_total(dev[2], want[2], want[2])
    s_clean, s_total = (err_over_total(dev[0], head[0] + tail[0], want[2]), err_over_total(dev[2], head[2] + tail[2], want[2]))
    print("N=%d K=%d in pieces of %d and %d: %d of %d flagged; vs stats.excise clean %.3g total %.3g, vs the first piece "
          "plus stats.excise of the second piece's rows clean %.3g total %.3g (bar %g); host vs device: mask unequal in %d, "
          "clean / kept / total unequal in %d / %d / %d"
          % (N, K, cap, K - cap, int(dmask.sum()), dmask.size, e_clean, e_total, s_clean, s_total, ADDITIVITY,
             int(np.count_nonzero(host_mask != dmask)), int(np.count_nonzero(host[0] != dev[0])),
             int(np.count_nonzero(host[1] != dev[1])), int(np.count_nonzero(host[2] != dev[2]))))
    assert np.array_equal(dmask, want_mask) and np.array_equal(dev[1], want[1])
    assert e_clean < ADDITIVITY and e_total < ADDITIVITY
    # the seam: the first piece's mask is the quota's, and the second piece added its rows to what the first left
    assert np.array_equal(dmask[:cap], hmask) and np.array_equal(dmask[cap:], tail_mask)
    assert np.array_equal(dev[1], head[1] + tail[1])
    assert s_clean < ADDITIVITY and s_total < ADDITIVITY
    assert 0 < dmask[cap:].sum() < dmask[cap:].size
    # the host entry, bit for bit
    assert np.array_equal(host_mask, dmask) and host.tobytes() == dev.tobytes()


# ---- 4. dedispersion below one block of bins ------------------------------------------------------------------------------------

DEDISP_SIZES = [2, 10, 34]           # a block of 2, a block of 10, one full block and a block of 2
DEDISP_L = 2


@pytest.fixture(scope="module")
def small_engines():
    """One engine, one noise stream and its rows tied to the slices per size, for the whole module."""
    made = {}

    def get(N):
        if N not in made:
            ds = rpf.Datastore(rpf.Params(N=N))
            stream = synth.noise_tones_iq(400 + N, N * DEDISP_L * 400)
            rows_equal_the_slices(ds, stream[:2 * N * DEDISP_L * 50], DEDISP_L, 50, "N=%d" % N)
            made[N] = (ds, stream)
        return made[N]
    yield get
    for ds, _ in made.values():
        ds.close()


@pytest.mark.parametrize("weights", ["none", "zeros"])
@pytest.mark.parametrize("kind", ["zero", "random", "random_direct"])
@pytest.mark.parametrize("N", DEDISP_SIZES)
def test_dedispersion_below_one_block(small_engines, N, kind, weights):
    """N < 32: a single, partial bin block -- the staged copy's `col < bc` guard and the tail loop after the batches of 8
    are the whole walk (N = 2: no batch at all; N = 10: one batch and two; N = 34: a full block, then a block of 2)."""
    ds, stream = small_engines(N)
    L, D = DEDISP_L, DT() + 1
    rng = np.random.default_rng([N, len(kind), len(weights)])
    delays, w = make_table(kind, rng, D, N, L), make_weights(weights, rng, N)
    if w is not None:                                                  # a bin of non-zero weight is left
        assert np.count_nonzero(w) >= 1 and np.count_nonzero(w == 0) >= 1
        if N == 2:
            assert np.count_nonzero(w == 0) == 1
    T = 2 * TT() + 3
    K = int(delays.max()) + T
    rows = fill(ds, stream, L, K)
    assert ds.dedisperse_times(delays) == T
    took, pairs = direct_share(delays, w, N)
    assert (took, pairs) == expected_direct_pairs(delays, w, N) and pairs >= 1
    assert took >= 1 if kind == "random_direct" else took == 0
    got = ds.dedisperse(delays, w)
    want = dedisperse.reference(rows, delays, w)
    assert got.shape == want.shape == (D, T)
    wrong = int(np.count_nonzero(got != want))
    print("N=%d %s weights=%s: K=%d Dmax=%d, %d of %d (tile, block) pairs direct, %d of %d outputs differ"
          % (N, kind, weights, K, delays.max(), took, pairs, wrong, want.size))
    assert same_bits(got, want) and np.isfinite(got).all()
    assert ds.quantile_rows == K


# ---- 5. the correlator below one wave of bins ----------------------------------------------------------------------------------

CORR_FRAMES = 130                    # one X-engine workgroup along the bins, two frame groups of 65


@pytest.mark.parametrize("N", [2, 16, 32])
def test_correlator_below_one_wave(N):
    """`if (k >= N) return` of the X-engine, the reduce and the finish with 62, 48 and 32 idle lanes."""
    F = CORR_FRAMES
    with correlate_engine(N) as ds:
        for M in (2, 8):
            assert correlate_emul().rpf_emul_correlate_groups(N, M, F) == 2
            vis, res = rows_case(ds, streams_of("cu8", 500 + N, M, N * F), F, "cu8 N=%d M=%d" % (N, M))
            check_layout(vis)
            one, n = corr(ds, res, repeats=1)                                        # F = 1: the terms themselves
            assert n == 1 and correlate_emul().rpf_emul_correlate_groups(N, M, 1) == 1
            correlate_check(one, device_rows(ds, res, 1), 1, "cu8 N=%d M=%d, one frame" % (N, M))
            print("cu8 N=%d M=%d, one frame: V equals the terms of the device's own rows as doubles" % (N, M))


def test_correlator_below_one_wave_cf32():
    N, M, F = 32, 3, CORR_FRAMES
    with correlate_engine(N, "cf32") as ds:
        vis, _ = rows_case(ds, streams_of("cf32", 540, M, N * F), F, "cf32 N=%d M=%d" % (N, M))
        check_layout(vis)


def test_correlator_reversal_identity_at_16():
    """test_reversing_the_streams_calling_twice_and_the_autos at N = 16, M = 5."""
    N, F, M = 16, CORR_FRAMES, 5
    streams = streams_of("cu8", 550, M, N * F)
    with correlate_engine(N) as ds:
        res = Resident(streams)
        vis, n = corr(ds, res)
        again, _ = corr(ds, res)
        rev, _ = corr(ds, Resident(streams[::-1]))
        assert n == F
        check_layout(vis)
        assert np.array_equal(again.view(np.int64), vis.view(np.int64))                     # the same bits
        for i in range(M):
            for j in range(M):
                assert np.array_equal(rev[i, j], vis[M - 1 - i, M - 1 - j]), (i, j)
        one, _ = corr(ds, res, repeats=1)
    # The autos.  Below 64 bins the rows come from the catch-all transform whatever family serves the size for power
    # (include/rpf_engine.h, rpf_stft_device: Routes), so the power path that shares the rows' arithmetic is the
    # catch-all engine's: one frame bit for bit, F frames in another grouping of the same double additions.
    worst = 0.0
    with correlate_engine(N, flags=_lib.FLAG_CATCH_ALL) as twin:
        for m in range(M):
            p1, n1, _ = device_run(twin, streams[m], repeats=1)
            pF, nF, _ = device_run(twin, streams[m])
            assert n1 == 1 and nF == F
            assert np.array_equal(one[m, m, 0], p1), m                                        # one frame: bit for bit
            worst = max(worst, max_rel(vis[m, m, 0], pF))
    print("N=%d M=%d: reversed streams give the reversed matrix, a second call the same bits; autos over %d frames vs "
          "accumulate_device of the catch-all engine: %.3g (bar 1e-12)" % (N, M, F, worst))
    assert worst < 1e-12


# ---- 6. the cross-spectrum at both ends -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["cu8", "cf32"])
@pytest.mark.parametrize("N", [2, 32])
def test_cross_bit_identity_below_one_workgroup(cf32, N, fmt):  # noqa: F811
    identity_case(cf32, N, fmt, [1, 3, 37], seed=620 + N)
    print("N=%d %s, 1 / 3 / 37 frames: the four planes equal the definition bit for bit" % (N, fmt))


def test_cross_chunk_seam_where_a_chunk_is_a_few_frames():
    """N = 262144: a chunk of cf32 rows (64 MB per stream) is 32 frames, so 33 frames cross a seam; judged as
    test_gpu_cross.test_more_than_one_chunk judges 8192."""
    N = 262144
    first = gather_chunk("cf32", N)
    frames = first + 1
    assert first * 8 * N == 64 << 20 and first < 64
    a, b = synth.uniform_iq(640, N * frames), synth.uniform_iq(641, N * frames)
    with cross_engine(N, "cu8") as ds:
        got, n, _ = cross_run(ds, a, b)
        cut = 2 * N * first
        head, n0, _ = cross_run(ds, a[:cut], b[:cut])               # each slice is one chunk: the definition, bit for bit
        tail, n1, _ = cross_run(ds, a[cut:], b[cut:])
        assert n == frames and n0 == first and n1 == frames - first
        err = in_units_of_the_powers(got, head + tail)
        print("N=%d, %d frames in chunks of %d and %d vs the sum of its single-chunk slices: %.3g (bar %g)"
              % (N, frames, first, frames - first, err, CROSS_ADDITIVITY))
        assert err < CROSS_ADDITIVITY
        # a quota that cuts inside the first chunk: the slice's bits
        q = first // 2
        part, n2, _ = cross_run(ds, a, b, repeats=q)
        want, n3, _ = cross_run(ds, a[:2 * N * q], b[:2 * N * q])
        assert n2 == n3 == q and np.array_equal(part, want)
        whole, n4, _ = cross_run(ds, a, b, repeats=first)           # ... and one that ends on the seam
        assert n4 == first and np.array_equal(whole, head)
