"""The dedisperser's tile walk below one block of bins, on the host emulator (tests/emul/dedisperse_emul.cpp over
csrc/dedisperse_core.h): test_dedisperse.test_the_tile_walk_equals_the_reference_bit_for_bit at N = 2, 10 and 34, the
sizes tests/test_gpu_edge_sizes.py runs on the device -- a block of 2 bins, a block of 10, one full block and a block
of 2 --, so that the CPU suite sees the shapes as well.

The walk is judged as there: the bits of dedisperse.reference, every (trial, time, bin) of non-zero weight visited
once and in order, no LDS cell read that was not staged.  What differs is the route.  At 64 and 500 bins the table kinds
decide it (`random_large` is read straight from the store, the others are staged); over one or two blocks they cannot:
a block with a single bin of non-zero weight has a span of 0 and is staged whatever its delays, and the DM grid over two
bins sweeps far more rows than the LDS tile holds.  So the route is held to the span rule itself, restated in numpy
(expected_direct_pairs), for every table."""
import numpy as np
import pytest

from rtl_power_fftw_amd import dedisperse
from test_dedisperse import BC, DT, TT, direct_share, emul, emul_dedisperse, same_bits, table

SIZES = [2, 10, 34]


def expected_direct_pairs(delays, weights, N):
    """direct_share by the rule of dedisperse_core.h, in numpy: a (trial tile, bin block) with a bin of non-zero weight
    is read straight from the store where its largest delay minus its smallest, plus TT, is beyond the LDS tile's rows."""
    delays = np.asarray(delays)
    live = np.ones(N, bool) if weights is None else np.asarray(weights) != 0
    direct = pairs = 0
    for d0 in range(0, delays.shape[0], DT()):
        for b0 in range(0, N, BC()):
            sel = delays[d0:d0 + DT(), b0:b0 + BC()][:, live[b0:b0 + BC()]]
            if sel.size:
                pairs += 1
                direct += int(int(sel.max()) - int(sel.min()) + TT() > emul().rpf_emul_dedisperse_rows())
    return direct, pairs


@pytest.mark.parametrize("N", [64, 500])
def test_the_span_rule_in_numpy_is_the_emulators_at_the_sizes_of_the_family_module(N):
    """Where the kinds do decide the route, the numpy rule says what test_dedisperse asserts."""
    rng = np.random.default_rng(N)
    for kind, all_direct in (("zero", False), ("dm", False), ("random_small", False), ("random_large", True)):
        delays = table(kind, rng, DT() + 1, N, 0)
        for w in (None, np.where(rng.uniform(size=N) < 0.2, 0.0, 1.5)):
            took, pairs = expected_direct_pairs(delays, w, N)
            assert (took, pairs) == direct_share(delays, w, N) and pairs > 0
            assert took == (pairs if all_direct else 0), (kind, took, pairs)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kind", ["zero", "dm", "random_small", "random_large"])
@pytest.mark.parametrize("weights", ["none", "positive", "zeros"])
def test_the_tile_walk_equals_the_reference_bit_for_bit_below_one_block(N, kind, weights):
    rng = np.random.default_rng([N, len(kind), len(weights)])
    D = DT() + 1
    delays = table(kind, rng, D, N, 0)
    K = int(delays.max()) + 2 * TT() + 3                       # T = 2 TT + 3: three time tiles, the last one ragged
    rows = rng.standard_normal((K, N)) ** 2 * 10.0 ** rng.uniform(-3, 3, (K, N))
    w = None
    if weights != "none":
        w = rng.uniform(0.25, 4.0, N)
    if weights == "zeros":
        w[N // 2] = 0.0
        w[rng.integers(0, N, N // 5)] = 0.0
        w[BC():2 * BC()] = 0.0                                 # (N = 34: the block of 2 is left without a bin and skipped)
        assert np.count_nonzero(w) >= 1                        # a bin of non-zero weight is left (N = 2: bin 0)
        rows[:, w == 0] = np.nan                               # a bin of weight 0 is not read
    want = dedisperse.reference(rows, delays, w)
    got, visits, disorder, direct = emul_dedisperse(rows, delays, w)
    assert want.shape == (D, 2 * TT() + 3)
    assert same_bits(got, want) and not np.isnan(got).any()
    # every (d, t, b) of non-zero weight exactly once, in ascending b; no LDS cell read that was not staged
    assert disorder == 0
    assert np.all(visits == (N if w is None else np.count_nonzero(w)))
    took, pairs = direct_share(delays, w, N)
    print("N=%d %s weights=%s: K=%d, %d of %d (tile, block) pairs direct, %d direct terms"
          % (N, kind, weights, K, took, pairs, direct))
    assert (took, pairs) == expected_direct_pairs(delays, w, N) and pairs > 0
    assert (direct > 0) == (took > 0)
    if kind in ("zero", "random_small"):                       # spans of at most TT + 8 rows fit the tile at any N
        assert took == 0
