"""Incoherent dedispersion of the stored integrations on the device (include/rpf_engine.h, rpf_dedisperse_device).  The
rows come from accumulate_series of the same engine and stream, the store is filled by quantile_append, and every
comparison with dedisperse.reference is equality of doubles: the order of every sum is defined, so there is no tolerance.
TT and DT come from the emulator library (csrc/dedisperse_core.h)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import dedisperse, synth
from helpers import ROOT, dp
from test_dedisperse import BC, DT, TT, cli_weights, direct_share, emul, format_block, same_bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
i32p = ctypes.POINTER(ctypes.c_int32)
SENTINEL = -12345.5
SIZES = {64: 2, 512: 2, 500: 2, 8192: 1}          # N: frames per integration (500: the catch-all route, no multiple of BC)


def current():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def engines():
    """One engine and one noise stream per size for the whole module."""
    made = {}

    def get(N):
        if N not in made:
            made[N] = (rpf.Datastore(rpf.Params(N=N)), synth.noise_tones_iq(300 + N, N * SIZES[N] * 400))
        return made[N]
    yield get
    for ds, _ in made.values():
        ds.close()


def fill(ds, stream, L, K):
    """The first K integrations of `stream`: the engine's own rows, and the same in the store."""
    sub = stream[:2 * ds.params.N * L * K]
    rows, done = ds.accumulate_series(sub, L)
    assert done == K
    ds.quantile_reset()
    assert ds.quantile_append(sub, L) == K and ds.quantile_rows == K
    return rows


def make_table(kind, rng, D, N, L):
    if kind == "zero":
        return np.zeros((D, N), dtype=np.int32)
    if kind == "dm":                                   # a DM grid whose last trial sweeps about 60 rows
        per_dm = dedisperse.dm_delays([1.0e4], 408e6, 2.4e6, N, L).max() / 1.0e4
        return dedisperse.dm_delays(np.arange(D) * (60.0 / (per_dm * (D - 1))), 408e6, 2.4e6, N, L)
    dmax = TT() + 26 if kind == "random" else emul().rpf_emul_dedisperse_rows() + 40
    t = rng.integers(0, dmax + 1, (D, N)).astype(np.int32)
    t[D - 1, N - 1] = dmax
    return t


def make_weights(kind, rng, N):
    if kind == "none":
        return None
    w = rng.uniform(0.25, 4.0, N)
    if kind == "zeros":
        w[N // 2] = 0.0
        w[rng.integers(0, N, N // 5)] = 0.0
        w[BC():2 * BC()] = 0.0                         # a whole block without a bin
    return w


# ---- 1. equals the reference on the series' own rows, bit for bit -----------------------------------------------------------

@pytest.mark.parametrize("weights", ["none", "positive", "zeros"])
@pytest.mark.parametrize("kind", ["zero", "dm", "random", "random_direct"])
@pytest.mark.parametrize("N", sorted(SIZES))
def test_equals_the_reference_bit_for_bit(engines, N, kind, weights):
    ds, stream = engines(N)
    L, D = SIZES[N], DT() + 1
    rng = np.random.default_rng([N, len(kind), len(weights)])
    delays, w = make_table(kind, rng, D, N, L), make_weights(weights, rng, N)
    T = 2 * TT() + 3
    K = int(delays.max()) + T
    rows = fill(ds, stream, L, K)
    assert ds.dedisperse_times(delays) == T
    took, pairs = direct_share(delays, w, N)
    assert (took == pairs) if kind == "random_direct" else (took == 0)
    if kind == "dm":
        assert delays.max() > 40
    if kind == "random":
        assert delays.max() > TT()
    got = ds.dedisperse(delays, w)
    want = dedisperse.reference(rows, delays, w)
    assert got.shape == want.shape == (D, T)
    wrong = int(np.count_nonzero(got != want))
    print("N=%d %s weights=%s: K=%d Dmax=%d, %d of %d (tile, block) pairs direct, %d of %d outputs differ"
          % (N, kind, weights, K, delays.max(), took, pairs, wrong, want.size))
    assert same_bits(got, want) and np.isfinite(got).all()
    assert ds.quantile_rows == K


@pytest.mark.parametrize("N", [64, 500])
def test_one_time_and_no_time(engines, N):
    ds, stream = engines(N)
    L, D, K = SIZES[N], DT() + 1, 37
    rng = np.random.default_rng(N)
    rows = fill(ds, stream, L, K)
    delays = rng.integers(0, K, (D, N)).astype(np.int32)
    delays[3, 7] = K - 1                                                      # Dmax = K - 1: T = 1
    got = ds.dedisperse(delays)
    assert got.shape == (D, 1) and same_bits(got, dedisperse.reference(rows, delays))
    for dmax in (K, K + 1000):                                                # Dmax >= K: T = 0, nothing is written
        delays[3, 7] = dmax
        assert ds.dedisperse_times(delays) == 0 and ds.dedisperse(delays).shape == (D, 0)
        out = torch.full((D * 4,), SENTINEL, dtype=torch.float64, device=DEV)
        assert ds.dedisperse_device(delays, None, out.data_ptr(), out.numel(), current()) == 0
        host = np.full(D * 4, SENTINEL)
        times = ctypes.c_int64(-1)
        assert ds._lib.rpf_dedisperse(ds._handle, delays.ctypes.data_as(i32p), None, D, host.ctypes.data_as(dp), host.size,
                                      ctypes.byref(times)) == 0 and times.value == 0
        torch.cuda.synchronize()
        assert np.all(out.cpu().numpy() == SENTINEL) and np.all(host == SENTINEL)


# ---- 2. NaN -------------------------------------------------------------------------------------------------------------------

def test_a_nan_row_reaches_exactly_the_outputs_that_read_it():
    N, L, D = 512, 2, DT() + 1
    rng = np.random.default_rng(21)
    delays = rng.integers(0, 29, (D, N)).astype(np.int32)
    delays[:, N - 1] = 0
    delays[5, 100] = delays[9, 200] = 29                                      # the largest delay: two trials, one bin each
    T = 2 * TT() + 3
    K = int(delays.max()) + T
    z = synth.gaussian_cf32(22, N * K * L, sigma=20.0).copy()
    bad = K - 1                                                               # read only at t = T - 1 through a delay of Dmax
    z[bad * L * N + 300] = np.nan
    stream = z.view(np.uint8).reshape(-1)
    w = make_weights("zeros", rng, N)
    w[100], w[200] = 1.5, 0.0                                                 # trial 9 reads the row through a bin of weight 0
    assert delays.max() == 29
    with rpf.Datastore(rpf.Params(N=N, sample_format="cf32")) as ds:
        rows, done = ds.accumulate_series(stream, L)
        assert done == K and np.all(np.isnan(rows[bad])) and not np.isnan(np.delete(rows, bad, axis=0)).any()
        assert ds.quantile_append(stream, L) == K
        for weights in (None, w):
            live = np.ones(N, bool) if weights is None else weights != 0
            reads = ((delays[:, None, :] + np.arange(T)[None, :, None]) == bad) & live[None, None, :]
            expect_nan = reads.any(axis=2)                                    # (D, T)
            assert np.argwhere(expect_nan).tolist() == ([[5, T - 1], [9, T - 1]] if weights is None else [[5, T - 1]])
            got = ds.dedisperse(delays, weights)
            assert np.array_equal(np.isnan(got), expect_nan)
            assert same_bits(got, dedisperse.reference(rows, delays, weights))
        # the bins through which some output reads that row weighted 0: it is not read, nothing is NaN
        w2 = w.copy()
        w2[(delays == delays.max()).any(axis=0)] = 0.0
        got = ds.dedisperse(delays, w2)
        assert np.isfinite(got).all() and same_bits(got, dedisperse.reference(rows, delays, w2))


# ---- 3. the store is only read ------------------------------------------------------------------------------------------------

def test_the_store_and_the_selection_are_untouched_and_appends_stack(engines):
    N = 512
    ds, stream = engines(N)
    L, D, K1, K2 = SIZES[N], DT() + 1, 150, 90
    rng = np.random.default_rng(31)
    delays, w = make_table("random", rng, D, N, L), make_weights("positive", rng, N)
    q = [0.0, 0.5, 0.9]
    rows1 = fill(ds, stream, L, K1)
    before = ds.quantile_select(q)
    first = ds.dedisperse(delays, w)
    assert ds.quantile_rows == K1 and same_bits(ds.quantile_select(q), before)
    assert same_bits(ds.dedisperse(delays, w), first)                          # a second identical call
    assert same_bits(first, dedisperse.reference(rows1, delays, w))
    # append, dedisperse again: the reference over all rows
    more = stream[2 * N * L * K1:2 * N * L * (K1 + K2)]
    rows2, done = ds.accumulate_series(more, L)
    assert done == K2 and ds.quantile_append(more, L) == K2 and ds.quantile_rows == K1 + K2
    both = ds.dedisperse(delays, w)
    assert both.shape == (D, K1 + K2 - int(delays.max()))
    assert same_bits(both, dedisperse.reference(np.concatenate([rows1, rows2]), delays, w))
    assert same_bits(ds.quantile_select([0.5])[0], np.median(np.concatenate([rows1, rows2]), axis=0))


def test_device_entry_equals_host_entry(engines):
    N = 500
    ds, stream = engines(N)
    L, D = SIZES[N], DT() + 1
    rng = np.random.default_rng(41)
    delays, w = make_table("dm", rng, D, N, L), make_weights("zeros", rng, N)
    T = 2 * TT() + 3
    rows = fill(ds, stream, L, int(delays.max()) + T)
    out = torch.full((D * T + 6,), SENTINEL, dtype=torch.float64, device=DEV)
    assert ds.dedisperse_device(delays, w, out.data_ptr(), out.numel(), current()) == T
    # a second table straight after it on the same stream: the first call's tables are not overwritten under it
    K = T + int(delays.max())
    out2 = torch.full((D * K,), SENTINEL, dtype=torch.float64, device=DEV)
    assert ds.dedisperse_device(np.zeros_like(delays), None, out2.data_ptr(), out2.numel(), current()) == K
    torch.cuda.synchronize()
    assert same_bits(out2.cpu().numpy().reshape(D, K), dedisperse.reference(rows, np.zeros_like(delays)))
    got = out.cpu().numpy()
    assert np.all(got[D * T:] == SENTINEL)
    assert same_bits(got[:D * T].reshape(D, T), ds.dedisperse(delays, w))
    assert same_bits(got[:D * T].reshape(D, T), dedisperse.reference(rows, delays, w))


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------

def test_every_refusal_returns_its_code_and_leaves_the_output(engines):
    N = 64
    ds, stream = engines(N)
    L, D, K = SIZES[N], 3, 40
    fill(ds, stream, L, K)
    lib, bad_arg = ds._lib, rpf.ReturnValue.InvalidArgument
    good = np.zeros((D, N), dtype=np.int32)
    ones = np.ones(N)
    d_out = torch.full((D * K + 2,), SENTINEL, dtype=torch.float64, device=DEV)
    h_out = np.full(D * K, SENTINEL)
    times = ctypes.c_int64(-1)

    def call(device, e=None, delays=good, weights=None, n=D, out="own", cap=D * K, tp="own"):
        e = ds._handle if e is None else e
        t = ctypes.byref(times) if tp == "own" else tp
        d = None if delays is None else delays.ctypes.data_as(i32p)
        wp = None if weights is None else weights.ctypes.data_as(dp)
        times.value = -1
        if device:
            o = d_out.data_ptr() if out == "own" else out
            return lib.rpf_dedisperse_device(e, d, wp, n, ctypes.c_void_p(o), cap, ctypes.c_void_p(current()), t)
        o = h_out.ctypes.data_as(dp) if out == "own" else out
        return lib.rpf_dedisperse(e, d, wp, n, o, cap, t)

    def refused(word, **kw):
        for device in (True, False):
            assert call(device, **kw) == bad_arg, (word, device)
            if kw.get("e", 1) != 0:
                assert word in lib.rpf_last_error(ds._handle).decode(), (word, lib.rpf_last_error(ds._handle).decode())
            if kw.get("tp", "own") == "own":
                assert times.value == 0

    refused("NULL", e=0)
    refused("NULL", delays=None)
    refused("NULL", out=None)
    refused("NULL", tp=None)
    refused("n_trials", n=0)
    refused("n_trials", n=4097)
    negative = good.copy()
    negative[2, 5] = -1
    refused("negative delay", delays=negative)
    for v in (np.nan, np.inf, -np.inf):
        w = ones.copy()
        w[9] = v
        refused("not finite", weights=w)
    refused("capacity", cap=D * K - 1)
    assert call(True, out=d_out.data_ptr() + 8) == bad_arg and "16-byte" in lib.rpf_last_error(ds._handle).decode()
    assert lib.rpf_dedisperse_times(ds._handle, negative.ctypes.data_as(i32p), D) == -1
    assert lib.rpf_dedisperse_times(ds._handle, None, D) == -1 and lib.rpf_dedisperse_times(ds._handle, good.ctypes.data_as(i32p), 0) == -1
    ds.begin(4)
    refused("acquisition running")
    ds.finish()
    torch.cuda.synchronize()
    assert np.all(d_out.cpu().numpy() == SENTINEL) and np.all(h_out == SENTINEL)
    # ... and the engine still works, the store as it was
    assert call(False) == 0 and times.value == K and ds.quantile_rows == K and not np.any(h_out == SENTINEL)
    # the store's own refusals
    wide = np.zeros((D, 512), dtype=np.int32)
    for kw, word in ((dict(bin_stats=True), "RPF_FLAG_BIN_STATS"), (dict(pfb_taps=4), "PFB")):
        with rpf.Datastore(rpf.Params(N=512, **kw)) as other:
            for fn in (lambda: other.dedisperse(wide), lambda: other.dedisperse_device(wide, None, d_out.data_ptr(), D * K, current())):
                with pytest.raises(rpf.RPFError) as err:
                    fn()
                assert err.value.retval == bad_arg and word in str(err.value), str(err.value)
    with pytest.raises(rpf.RPFError):
        ds.dedisperse(np.zeros((2, N + 1), dtype=np.int32))
    with pytest.raises(rpf.RPFError):
        ds.dedisperse(good, np.ones(N - 1))


# ---- 5. what it is for: a dispersed pulse in noise ------------------------------------------------------------------------------

PULSE = dict(N=64, L=4, K=256, fc=408000000, rate=2400000, dm=15, at=100)


def pulse_stream(seed):
    """cu8 Gaussian noise of sigma 20 per component and, for every bin but DC, a bin-centred tone of amplitude 6 with a
    random phase in the L frames of row at + delays[dm][b]: a pulse of DM 15 that arrives at the top of the band in row 100."""
    N, L, K = PULSE["N"], PULSE["L"], PULSE["K"]
    rng = np.random.default_rng(seed)
    delays = dedisperse.dm_delays(np.arange(31.0), PULSE["fc"], PULSE["rate"], N, L)
    z = 20.0 * (rng.standard_normal(N * L * K) + 1j * rng.standard_normal(N * L * K))
    z = z.reshape(K, L * N)
    n = np.arange(L * N)
    for b in range(N):
        if b != N // 2:
            z[PULSE["at"] + delays[PULSE["dm"], b]] += 6.0 * np.exp(1j * (2 * np.pi * (b - N // 2) * n / N + rng.uniform(0, 2 * np.pi)))
    z = z.reshape(-1)
    u = np.empty(2 * z.size, dtype=np.float64)
    u[0::2], u[1::2] = z.real, z.imag
    u = np.rint(u + 127.0)
    assert u.min() >= 0 and u.max() <= 255                                    # no sample saturates
    return u.astype(np.uint8), delays


def test_the_pulse_is_found_at_its_dm_and_time():
    N, L, K = PULSE["N"], PULSE["L"], PULSE["K"]
    stream, delays = pulse_stream(0)
    assert delays.max() == 81
    with rpf.Datastore(rpf.Params(N=N)) as ds:
        assert ds.quantile_append(stream, L) == K
        w = cli_weights(ds.quantile_select([0.5])[0])
        plane = ds.dedisperse(delays, w)
    assert plane.shape == (31, 175)
    s = dedisperse.snr(plane)
    d, t = np.unravel_index(np.argmax(s), s.shape)
    others = np.delete(s, PULSE["dm"], axis=0).max()
    print("strongest sample: trial %d, t %d, snr %.1f; any other trial at most %.1f; DM 0 at most %.1f"
          % (d, t, s[d, t], others, s[0].max()))
    assert (d, t) == (PULSE["dm"], PULSE["at"])


def test_cli_end_to_end_on_the_pulse(tmp_path):
    N, L, K, rate = PULSE["N"], PULSE["L"], PULSE["K"], PULSE["rate"]
    stream, delays = pulse_stream(1)
    path = tmp_path / "rec.cu8"
    stream.tofile(str(path))
    with rpf.Datastore(rpf.Params(N=N, sample_rate=rate, cfreq=PULSE["fc"])) as ds:
        assert ds.quantile_append(stream, L) == K
        w = cli_weights(ds.quantile_select([0.5])[0])
        plane = ds.dedisperse(delays, w)
    nb = int(np.count_nonzero(w))
    assert nb == N - 1
    for extra in ((), ("-l",)):
        r = subprocess.run([CLI, "--input", str(path), "-f", str(PULSE["fc"]), "-r", str(rate), "-b", str(N), "--dedisperse", str(L),
                            "--dm", "0:30:1", *extra], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        want = []
        for d in range(31):
            block = format_block(plane[d], nb, L, N, rate, bool(extra), float(d), int(delays[d].max()))
            want += [ln for ln in block if ln.strip() and not ln.startswith("# Acquisition")]
        lines = r.stdout.split("\n")
        got = [ln for ln in lines[lines.index("# rtl-power-fftw output"):] if ln.strip() and not ln.startswith("# Acquisition")]
        assert r.stdout.count("# rtl-power-fftw output") == 31
        assert got == want, [(g, x) for g, x in zip(got, want) if g != x][:3]
        note = [ln for ln in r.stderr.split("\n") if ln.startswith("Dedispersed:")]
        assert len(note) == 1 and "%d integrations of %d frames" % (K, L) in note[0] and "175 times of 31 trials" in note[0]
        assert "DM 15 (trial 15) at %g s" % (100 * L * N / rate) in note[0], note[0]


def test_cli_refuses_a_replay_whose_medians_are_all_zero(tmp_path):
    """cu8 samples of 127 are zeros: every bin's median is 0, no bin keeps a weight, and the run says so instead of
    writing blocks of 0 / 0."""
    N, L, K = 64, 2, 8
    path = tmp_path / "zeros.cu8"
    np.full(2 * N * L * K, 127, dtype=np.uint8).tofile(str(path))
    r = subprocess.run([CLI, "--input", str(path), "-b", str(N), "--dedisperse", str(L), "--dm", "0:3:1"], capture_output=True, text=True)
    assert r.returncode == 5 and "--dedisperse" in r.stderr and "median of 0" in r.stderr, r.stderr
    assert "# DM" not in r.stdout
