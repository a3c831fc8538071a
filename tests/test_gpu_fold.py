"""Fold of a plane at trial periods on the device (include/rpf_engine.h, rpf_fold_device, rpf_dedisperse_fold).  Every
comparison with fold.reference is equality of doubles: the order of every sum is defined, so there is no tolerance.  The
helpers, the shapes and the detection case come from tests/test_fold.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import dedisperse, fold, synth
from helpers import ROOT, dp
from test_dedisperse import cli_weights
from test_fold import (BINS, PULSAR, PULSAR_DMS, TIMES, best_cell, cpp_chi2, emul, emul_fold, essential, i32p,
                       pulsar_steps, pulsar_stream, python_blocks, same_bits, make_series, make_steps,
                       u64p)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
SENTINEL = -12345.5
HIT_SENTINEL = -77


def current():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def engine():
    with rpf.Datastore(rpf.Params(N=64)) as ds:
        yield ds


class Outputs:
    """Device outputs full of sentinels, `extra` cells behind what a call writes."""
    def __init__(self, D, P, NB, extra=6):
        self.shape, self.extra = (D, P, NB), extra
        self.prof = torch.full((D * P * NB + extra,), SENTINEL, dtype=torch.float64, device=DEV)
        self.hits = torch.full((P * NB + extra,), HIT_SENTINEL, dtype=torch.int32, device=DEV)
        self.mom = torch.full((2 * D + extra,), SENTINEL, dtype=torch.float64, device=DEV)

    def read(self):
        """(prof, hits, mom) on the host; what lies behind them is still the sentinel."""
        D, P, NB = self.shape
        torch.cuda.synchronize()
        prof, hits, mom = self.prof.cpu().numpy(), self.hits.cpu().numpy(), self.mom.cpu().numpy()
        assert np.all(prof[D * P * NB:] == SENTINEL) and np.all(hits[P * NB:] == HIT_SENTINEL) and np.all(mom[2 * D:] == SENTINEL)
        return prof[:D * P * NB].reshape(D, P, NB), hits[:P * NB].reshape(P, NB), mom[:2 * D].reshape(D, 2)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.prof == SENTINEL).all() and (self.hits == HIT_SENTINEL).all() and (self.mom == SENTINEL).all())


def fold_on_device(ds, x, steps, NB, hits=True, mom=True, extra=6):
    """ds.fold_device of the host array x (D, T) through a torch double tensor: (prof, hits, mom) with None where not asked."""
    D, T = x.shape
    d_x = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    out = Outputs(D, len(steps), NB, extra)
    ds.fold_device(d_x.data_ptr(), D, T, steps, NB, out.prof.data_ptr(), out.prof.numel() - extra,
                   out.hits.data_ptr() if hits else None, out.mom.data_ptr() if mom else None, current())
    prof, h, m = out.read()
    if not hits:
        assert np.all(h == HIT_SENTINEL)
    if not mom:
        assert np.all(m == SENTINEL)
    return prof, h if hits else None, m if mom else None


# ---- 1. equals the reference, bit for bit ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("NB", BINS)
@pytest.mark.parametrize("T", TIMES)
def test_fold_device_equals_the_reference_bit_for_bit(engine, T, NB):
    for P in (1, 64, 65):                                    # the seam between two waves of periods
        for D in (1, 3):
            rng = np.random.default_rng([T, NB, P, D])
            steps, x = make_steps(rng, P), make_series(rng, D, T)
            want_prof, want_hits, want_mom = fold.reference(x, steps, NB)
            prof, hits, mom = fold_on_device(engine, x, steps, NB)
            wrong = int(np.count_nonzero(prof != want_prof))
            print("T=%d NB=%d P=%d D=%d: %d of %d cells differ" % (T, NB, P, D, wrong, prof.size))
            assert prof.tobytes() == want_prof.tobytes(), (T, NB, P, D)
            assert np.array_equal(hits, want_hits) and hits.dtype == np.int32 and np.all(hits.sum(axis=1) == T)
            assert mom.tobytes() == want_mom.tobytes()
    # a second identical call gives the same bits; hits and mom are optional
    again, no_hits, no_mom = fold_on_device(engine, x, steps, NB, hits=False, mom=False)
    assert again.tobytes() == prof.tobytes() and no_hits is None and no_mom is None


def test_two_calls_back_to_back_on_one_stream_do_not_disturb_each_other(engine):
    rng = np.random.default_rng(11)
    T, D = 4099, 3
    x = make_series(rng, D, T)
    d_x = torch.from_numpy(x).to(DEV)
    first, second = (make_steps(rng, 65), 64), (fold.row_period_steps([40.3, 2.0, 1000.5]), 7)
    outs = []
    for steps, NB in (first, second):                        # no synchronise between the two
        out = Outputs(D, len(steps), NB)
        engine.fold_device(d_x.data_ptr(), D, T, steps, NB, out.prof.data_ptr(), D * len(steps) * NB, out.hits.data_ptr(),
                           out.mom.data_ptr(), current())
        outs.append(out)
    for out, (steps, NB) in zip(outs, (first, second)):
        prof, hits, mom = out.read()
        want = fold.reference(x, steps, NB)
        assert prof.tobytes() == want[0].tobytes() and np.array_equal(hits, want[1]) and mom.tobytes() == want[2].tobytes()


def test_series_in_groups_when_the_partials_exceed_the_scratch(engine):
    """5 series x 4096 periods x 128 bins: 64 MB of partials per series, so the engine runs groups of 3 and 2 series."""
    D, P, NB, T = 5, 4096, 128, 33
    assert emul().rpf_emul_fold_group_series(D, P, NB) == 3
    rng = np.random.default_rng(17)
    steps, x = make_steps(rng, P), make_series(rng, D, T)
    prof, hits, mom = fold_on_device(engine, x, steps, NB)
    e_prof, e_hits, e_mom, disorder, groups = emul_fold(x, steps, NB)
    assert disorder == 0 and groups == 2
    assert prof.tobytes() == e_prof.tobytes() and np.array_equal(hits, e_hits) and mom.tobytes() == e_mom.tobytes()
    some = [0, 1, 63, 64, 2047, 4095]                        # the reference itself at periods of the first and the last wave
    want = fold.reference(x, steps[some], NB)
    assert prof[:, some].tobytes() == want[0].tobytes() and np.array_equal(hits[some], want[1]) and mom.tobytes() == want[2].tobytes()


# ---- 2. special cases --------------------------------------------------------------------------------------------------------------

def test_a_nan_reaches_exactly_the_cells_of_its_bins_and_its_moments(engine):
    rng = np.random.default_rng(7)
    T, NB, at = 1000, 7, 613
    steps, x = make_steps(rng, 65), make_series(rng, 3, T)
    x[1, at] = np.nan
    prof, hits, mom = fold_on_device(engine, x, steps, NB)
    expect = np.zeros(prof.shape, bool)
    for p, step in enumerate(steps):
        expect[1, p, fold.phase_bins(step, T, NB)[at]] = True
    assert np.array_equal(np.isnan(prof), expect)
    assert np.isnan(mom[1]).all() and np.isfinite(mom[[0, 2]]).all()
    want = fold.reference(x, steps, NB)
    assert same_bits(prof, want[0]) and np.array_equal(hits, want[1]) and same_bits(mom, want[2])


def test_no_time_writes_nothing(engine):
    steps = make_steps(np.random.default_rng(1), 5)
    d_x = torch.zeros(8, dtype=torch.float64, device=DEV)
    out = Outputs(3, 5, 16)
    engine.fold_device(d_x.data_ptr(), 3, 0, steps, 16, out.prof.data_ptr(), 3 * 5 * 16, out.hits.data_ptr(), out.mom.data_ptr(), current())
    assert out.untouched()


# ---- 3. dedisperse_fold -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [64, 500])
def test_dedisperse_fold_equals_the_reference_of_the_plane(N):
    L, D, K, NB = 2, 5, 700, 16
    rng = np.random.default_rng(N)
    stream = synth.noise_tones_iq(900 + N, N * L * K)
    delays = dedisperse.dm_delays(np.arange(D) * 6.0, 408e6, 2.4e6, N, L)
    w = rng.uniform(0.25, 4.0, N)
    w[N // 2] = 0.0
    steps = np.concatenate([fold.row_period_steps([40.3, 2.0, 77.7]), make_steps(rng, 64)])
    q = [0.1, 0.5]
    with rpf.Datastore(rpf.Params(N=N)) as ds:
        assert ds.quantile_append(stream, L) == K
        before_q, plane = ds.quantile_select(q), ds.dedisperse(delays, w)
        T = plane.shape[1]
        assert 0 < T == K - int(delays.max())
        prof, hits, mom, times = ds.dedisperse_fold(delays, w, steps, NB)
        assert times == T and prof.shape == (D, steps.size, NB) and hits.shape == (steps.size, NB) and mom.shape == (D, 2)
        want = fold.reference(plane, steps, NB)
        assert prof.tobytes() == want[0].tobytes() and np.array_equal(hits, want[1]) and mom.tobytes() == want[2].tobytes()
        # the store, the selection and the plain dedispersion are as they were; a second call gives the same bits
        assert ds.quantile_rows == K and same_bits(ds.quantile_select(q), before_q) and same_bits(ds.dedisperse(delays, w), plane)
        again = ds.dedisperse_fold(delays, None, steps[:3], 7)
        assert again[0].tobytes() == fold.reference(ds.dedisperse(delays), steps[:3], 7)[0].tobytes()
        assert ds.dedisperse_fold(delays, w, steps, NB)[0].tobytes() == prof.tobytes()
        # T = 0: RPF_OK, nothing written
        far = delays.copy()
        far[0, 0] = K
        h_prof, times = np.full(D * 3 * 7, SENTINEL), ctypes.c_int64(-1)
        assert ds._lib.rpf_dedisperse_fold(ds._handle, far.ctypes.data_as(i32p), None, D, steps.ctypes.data_as(u64p), 3, 7,
                                           h_prof.ctypes.data_as(dp), h_prof.size, None, None, ctypes.byref(times)) == 0
        assert times.value == 0 and np.all(h_prof == SENTINEL)


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------

def test_every_refusal_returns_its_code_and_leaves_the_output(engine):
    ds, lib, bad_arg = engine, engine._lib, rpf.ReturnValue.InvalidArgument
    D, T, P, NB = 3, 100, 5, 16
    x = torch.zeros(D * T + 2, dtype=torch.float64, device=DEV)
    out = Outputs(D, P, NB)
    steps = make_steps(np.random.default_rng(2), P)
    sp = steps.ctypes.data_as(u64p)
    cells = D * P * NB

    def call(e="own", series="own", n=D, t=T, st=sp, p=P, nb=NB, prof="own", cap=cells, hits="own", mom="own"):
        e = ds._handle if e == "own" else e
        series = x.data_ptr() if series == "own" else series
        prof = out.prof.data_ptr() if prof == "own" else prof
        hits = out.hits.data_ptr() if hits == "own" else hits
        mom = out.mom.data_ptr() if mom == "own" else mom
        return lib.rpf_fold_device(e, ctypes.c_void_p(series), n, t, st, p, nb, ctypes.c_void_p(prof), cap, ctypes.c_void_p(hits),
                                   ctypes.c_void_p(mom), ctypes.c_void_p(current()))

    def refused(word, **kw):
        assert call(**kw) == bad_arg, word
        if kw.get("e", 1) is not None:
            assert word in lib.rpf_last_error(ds._handle).decode(), (word, lib.rpf_last_error(ds._handle).decode())

    refused("NULL", e=None)
    refused("NULL", series=None)
    refused("NULL", st=None)
    refused("NULL", prof=None)
    for n in (0, -1, 4097):
        refused("n_series", n=n)
        refused("n_periods", p=n)
    for nb in (0, -1, 129):
        refused("phase_bins", nb=nb)
    refused("T must be", t=-1)
    refused("T must be", t=1 << 31)
    refused("capacity", cap=cells - 1)
    refused("at most 16777216", n=4096, p=4096, nb=2, cap=1 << 40)
    refused("8-byte", series=x.data_ptr() + 4)
    refused("16-byte", prof=out.prof.data_ptr() + 8)
    refused("16-byte", mom=out.mom.data_ptr() + 8)
    ds.begin(4)
    refused("acquisition running")
    ds.finish()
    assert out.untouched()
    # ... and the engine still works
    assert call() == 0
    prof, hits, mom = out.read()
    assert np.all(prof == 0.0) and np.all(hits.sum(axis=1) == T) and np.all(mom == 0.0)

    # rpf_dedisperse_fold: its own refusals and those of rpf_dedisperse, the host outputs untouched
    N, K = 64, 40
    stream = synth.noise_tones_iq(5, N * 2 * K)
    ds.quantile_reset()
    assert ds.quantile_append(stream, 2) == K
    good = np.zeros((D, N), dtype=np.int32)
    h_prof, h_hits, h_mom = np.full(cells, SENTINEL), np.full(P * NB, HIT_SENTINEL, dtype=np.int32), np.full(2 * D, SENTINEL)
    times = ctypes.c_int64(-1)

    def host(e="own", delays=good, weights=None, n=D, st=sp, p=P, nb=NB, prof="own", cap=cells, tp="own"):
        e = ds._handle if e == "own" else e
        prof = h_prof.ctypes.data_as(dp) if prof == "own" else prof
        return lib.rpf_dedisperse_fold(e, None if delays is None else delays.ctypes.data_as(i32p),
                                       None if weights is None else weights.ctypes.data_as(dp), n, st, p, nb, prof, cap,
                                       h_hits.ctypes.data_as(i32p), h_mom.ctypes.data_as(dp), ctypes.byref(times) if tp == "own" else tp)

    negative = good.copy()
    negative[1, 3] = -1
    weights = np.ones(N)
    weights[7] = np.inf
    for word, kw in (("NULL", dict(e=None)), ("NULL", dict(delays=None)), ("NULL", dict(st=None)), ("NULL", dict(prof=None)),
                     ("NULL", dict(tp=None)), ("n_trials", dict(n=0)), ("n_trials", dict(n=4097)), ("n_periods", dict(p=0)),
                     ("n_periods", dict(p=4097)), ("phase_bins", dict(nb=0)), ("phase_bins", dict(nb=129)),
                     ("capacity", dict(cap=cells - 1)), ("negative delay", dict(delays=negative)), ("not finite", dict(weights=weights))):
        assert host(**kw) == bad_arg, word
        if kw.get("e", 1) is not None:
            assert word in lib.rpf_last_error(ds._handle).decode(), (word, lib.rpf_last_error(ds._handle).decode())
    ds.begin(4)
    assert host() == bad_arg and "acquisition running" in lib.rpf_last_error(ds._handle).decode()
    ds.finish()
    assert np.all(h_prof == SENTINEL) and np.all(h_hits == HIT_SENTINEL) and np.all(h_mom == SENTINEL)
    assert host() == 0 and times.value == K and not np.any(h_prof == SENTINEL) and np.all(h_hits.reshape(P, NB).sum(axis=1) == K)
    wide = np.zeros((D, 512), dtype=np.int32)
    for kw, word in ((dict(bin_stats=True), "RPF_FLAG_BIN_STATS"), (dict(pfb_taps=4), "PFB")):
        with rpf.Datastore(rpf.Params(N=512, **kw)) as other:
            with pytest.raises(rpf.RPFError) as err:
                other.dedisperse_fold(wide, None, steps, NB)
            assert err.value.retval == bad_arg and word in str(err.value), str(err.value)
            # ... while the device entry reads no store and works on any engine
            got = fold_on_device(other, np.ones((1, 50)), steps, NB)
            assert got[0].tobytes() == fold.reference(np.ones((1, 50)), steps, NB)[0].tobytes()


# ---- 5. what it is for: the pulsar of tests/test_fold.py, through the engine and through the CLI ----------------------------------

def engine_search(stream, delays, N, L, rate, fc):
    with rpf.Datastore(rpf.Params(N=N, sample_rate=rate, cfreq=fc)) as ds:
        assert ds.quantile_append(stream, L) == PULSAR["K"]
        w = cli_weights(ds.quantile_select([0.5])[0])
        prof, hits, mom, T = ds.dedisperse_fold(delays, w, pulsar_steps(), PULSAR["NB"])
    return w, prof, hits, mom, T


def test_the_pulsar_is_found_at_its_dm_and_period():
    N, L = PULSAR["N"], PULSAR["L"]
    stream, delays = pulsar_stream(0)
    w, prof, hits, mom, T = engine_search(stream, delays, N, L, PULSAR["rate"], PULSAR["fc"])
    assert T == 1967 and prof.shape == (11, 9, 16)
    c = fold.chi2(prof, hits, mom, T)
    order = np.sort(c.ravel())
    print("strongest cell %s, reduced chi2 %.1f, second %.1f, DM 0 at most %.1f" % (best_cell(c), order[-1], order[-2], c[0].max()))
    assert best_cell(c) == (PULSAR["dm_index"], 4)
    assert np.all(c.max() > 2 * c[0])


def test_cli_end_to_end_on_the_pulsar(tmp_path):
    N, L, K, rate, fc, NB = PULSAR["N"], PULSAR["L"], PULSAR["K"], PULSAR["rate"], PULSAR["fc"], PULSAR["NB"]
    stream, delays = pulsar_stream(1)
    path = tmp_path / "rec.cu8"
    stream.tofile(str(path))
    t_row = (float(L) * float(N)) / float(rate)
    # periods as text the CLI parses back to lo + i step: 40.3 - 0.4 rows and a step of 0.1 row, in seconds
    lo, step = "%.12g" % (39.9 * t_row), "%.12g" % (0.1 * t_row)
    periods = np.array([float(lo) + i * float(step) for i in range(9)])
    steps = fold.period_steps(periods, rate, N, L)
    with rpf.Datastore(rpf.Params(N=N, sample_rate=rate, cfreq=fc)) as ds:
        assert ds.quantile_append(stream, L) == K
        w = cli_weights(ds.quantile_select([0.5])[0])
        prof, hits, mom, T = ds.dedisperse_fold(delays, w, steps, NB)
    nb = int(np.count_nonzero(w))
    c = fold.chi2(prof, hits, mom, T)
    assert nb == N - 1 and T == 1967 and best_cell(c) == (PULSAR["dm_index"], 4)
    c_cpp = cpp_chi2(prof, hits, mom, T)
    assert np.max(np.abs(c_cpp - c) / c) < 1e-9 and best_cell(c_cpp) == best_cell(c)
    for extra in ((), ("-l",)):
        r = subprocess.run([CLI, "--input", str(path), "-f", str(fc), "-r", str(rate), "-b", str(N), "--dedisperse", str(L), "--dm",
                            "0:30:3", "--fold", "%s:%s:%s" % (lo, "%.12g" % (periods[8] + 0.5 * float(step)), step), "--phase-bins",
                            str(NB), *extra], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout.count("# rtl-power-fftw output") == 2 and "# time [s]" not in r.stdout
        lines = r.stdout.split("\n")
        got = essential(lines[lines.index("# rtl-power-fftw output"):])
        # (Python's formatting of the C++ statistic: the two sum in different orders, so their sixth digit may differ)
        want = python_blocks(PULSAR_DMS, periods, NB, T, c_cpp, prof, hits, nb, bool(extra))
        assert got == want, [(g, x) for g, x in zip(got, want) if g != x][:3]
        # the DMs are separated by blank lines: 11 DMs of 9 lines
        body = lines[lines.index("# DM [pc cm^-3] period [s] reduced chi2") + 1:]
        assert [i for i, ln in enumerate(body[:11 * 10 + 1]) if ln == ""] == [10 * d + 9 for d in range(11)] + [110]
        note = [ln for ln in r.stderr.split("\n") if ln.startswith("Folded:")]
        assert len(note) == 1, r.stderr
        assert "%d integrations of %d frames, 1967 times of 11 trials at 9 periods" % (K, L) in note[0], note[0]
        assert note[0].endswith("strongest cell: DM 15 (trial 5), period %.9g s (trial 4), reduced chi2 %.6g" % (periods[4], c_cpp[5, 4])), note[0]
    # without --fold every byte of --dedisperse output is what it was: the blocks of time and power
    r = subprocess.run([CLI, "--input", str(path), "-f", str(fc), "-r", str(rate), "-b", str(N), "--dedisperse", str(L), "--dm", "0:30:15"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count("# time [s] power [median units]") == 3 and "# fold" not in r.stdout
    assert "Dedispersed:" in r.stderr and "Folded:" not in r.stderr
