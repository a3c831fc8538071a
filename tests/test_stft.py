"""Short-time Fourier transform, everything that needs no GPU: the two symbols at the boundary, the staging index map of
the store kernels (csrc/stft_core.h through tests/emul/stft_emul.cpp), the piece rule of the host entry, the float64
reference (rtl_power_fftw_amd/stft.py), the CLI's option, and the CPU float32 figures behind the GPU test's bar
(stft_bars.py).  tests/test_gpu_stft.py has the rest."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, pfb, stft, synth
from helpers import ROOT
import frame_truth
import stft_bars
from test_pfb import emul_fold, make_stream

sys.path.insert(0, os.path.join(ROOT, "tools"))
from lds_bank_model import B128, G16       # noqa: E402  (the lane groups of the banking rules stft_core.h quotes)

HEADER = os.path.join(ROOT, "include", "rpf_engine.h")
CLI = os.path.join(ROOT, "rtl-power-fftw_amd", "host", "rpf_power")
K1_SIZES = [64, 128, 256, 512, 1024, 2048, 4096, 8192]
ip = ctypes.POINTER(ctypes.c_int)
_emul = None


def emul():
    global _emul
    if _emul is None:
        lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emul", "librpf_emul_stft.so"))
        lib.rpf_emul_stft_map.argtypes = [ctypes.c_int, ctypes.c_int, ip]
        lib.rpf_emul_stft_pieces.argtypes = [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_longlong,
                                             ctypes.POINTER(ctypes.c_longlong)]
        _emul = lib
    return _emul


# ---- header, binding and library -----------------------------------------------------------------------------------------

def test_header_binding_and_library_agree_on_the_two_symbols():
    text = open(HEADER).read()
    assert re.search(r"\bint rpf_stft_device\(rpf_engine\* e, const void\* d_stream, size_t nbytes, int64_t max_frames,\s+"
                     r"void\* d_out[^;]*, int64_t\* frames_done, void\* hip_stream\);", text)
    assert re.search(r"\bint rpf_stft\(rpf_engine\* e, const uint8_t\* stream, size_t nbytes, int64_t max_frames,\s+"
                     r"void\* out[^;]*, int64_t\* frames_done\);", text)
    m = re.search(r"#define RPF_ABI_VERSION 2(.*?)\*/", text, re.S)
    assert m and "rpf_stft_device" in m.group(1) and "rpf_stft" in m.group(1)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in ("rpf_stft_device", "rpf_stft"):
        assert name in _lib.symbol_names()
        assert re.search(r"\bT %s$" % name, exported, re.M), name
    lib = rpf.load()
    assert lib.rpf_abi_version() == 2
    out = np.zeros(4, dtype=np.float32)
    assert lib.rpf_stft(None, None, 0, 0, out.ctypes.data, None) == rpf.ReturnValue.InvalidArgument
    assert lib.rpf_stft_device(None, None, 0, 0, None, None, None) == rpf.ReturnValue.InvalidArgument
    assert hasattr(rpf.Datastore, "stft") and hasattr(rpf.Datastore, "stft_device")


# ---- the staging index map -----------------------------------------------------------------------------------------------

def staging_map(row):
    g = np.zeros(7, dtype=np.int32)
    assert emul().rpf_emul_stft_map(row, 0, g.ctypes.data_as(ip)) == 0
    N, P, T, cpx, rounds = (int(v) for v in g[:5])
    st = np.zeros((T, P, 2), dtype=np.int32)
    rd = np.zeros((T, rounds, 2), dtype=np.int32)
    assert emul().rpf_emul_stft_map(row, 1, st.ctypes.data_as(ip)) == 0
    assert emul().rpf_emul_stft_map(row, 2, rd.ctypes.data_as(ip)) == 0
    return N, P, T, cpx, rounds, int(g[5]), int(g[6]), st, rd


def conflict_degree(dword_of_lane, groups, nbanks, width):
    """The largest number of distinct addresses on one bank in a lane group (tools/lds_bank_model.py's rules)."""
    worst = 0
    for grp in groups:
        banks = {}
        for l in grp:
            for w in range(width):
                d = dword_of_lane[l] + w
                banks.setdefault(d % nbanks, set()).add(d)
        worst = max(worst, max(len(v) for v in banks.values()))
    return worst


def test_the_size_table_is_the_k1_sizes():
    assert emul().rpf_emul_stft_rows() == len(K1_SIZES)
    assert [staging_map(r)[0] for r in range(len(K1_SIZES))] == K1_SIZES
    assert emul().rpf_emul_stft_map(len(K1_SIZES), 0, np.zeros(7, dtype=np.int32).ctypes.data_as(ip)) == -1


@pytest.mark.parametrize("row", range(len(K1_SIZES)))
def test_every_bin_is_written_once_and_read_once_inside_the_slab(row):
    N, P, T, cpx, rounds, _, _, st, rd = staging_map(row)
    assert cpx == N + N // P and rounds == P // 2
    # written: every bin by exactly one (lane, register), at an index of its own inside the slab
    assert sorted(st[..., 0].ravel().tolist()) == list(range(N))
    assert len(set(st[..., 1].ravel().tolist())) == N and 0 <= st[..., 1].min() and st[..., 1].max() < cpx
    index_of = dict(zip(st[..., 0].ravel().tolist(), st[..., 1].ravel().tolist()))
    # read: the pairs (bin, bin + 1) tile the row, each pair 16 bytes, 16-byte aligned in the slab and in the row
    firsts = rd[..., 0].ravel()
    assert sorted(firsts.tolist()) == list(range(0, N, 2))
    for b, i in zip(firsts.tolist(), rd[..., 1].ravel().tolist()):
        assert i == index_of[b] and i % 2 == 0 and index_of[b + 1] == i + 1
    # a round's lanes write contiguous bytes: lane t takes the pair after lane t - 1's
    assert np.all(np.diff(rd[..., 0], axis=0) == 2)


@pytest.mark.parametrize("row", range(len(K1_SIZES)))
def test_bank_conflicts_are_what_the_header_states(row):
    N, P, T, cpx, rounds, stated_store, stated_read, st, rd = staging_map(row)
    waves = max(1, T // 64)
    store = read = 0
    for w in range(waves):
        # lane l of wave w: frame slot and lane of the frame (T < 64: several slots per wave, each with a slab of its own)
        lanes = [((64 * w + l) // T, (64 * w + l) % T) for l in range(64)]
        for a in range(P):
            store = max(store, conflict_degree([2 * (fs * cpx + int(st[t, a, 1])) for fs, t in lanes], G16, 32, 2))
        for i in range(rounds):
            read = max(read, conflict_degree([2 * (fs * cpx + int(rd[t, i, 1])) for fs, t in lanes], B128, 64, 4))
    print("N=%d: 8-byte stores %d-way (stated %d), 16-byte reads %d-way (stated %d)" % (N, store, stated_store, read, stated_read))
    assert store == stated_store and read == stated_read
    assert stated_store <= 4 and stated_read <= 2


# ---- the piece rule of the host entry ------------------------------------------------------------------------------------

@pytest.mark.parametrize("b", [2, 8])
@pytest.mark.parametrize("N", [64, 8192, 1 << 20])
def test_pieces_tile_the_frames_within_both_bounds(N, b):
    budget = 64 << 20
    for S in (1, N // 2 + 1, N):
        frame, pitch = b * N, b * S
        for F in (1, 2, 1000, 123457):
            out = (ctypes.c_longlong * 3)()
            emul().rpf_emul_stft_pieces(frame, pitch, N, F, out)
            per, nbytes, hop = out[0], out[1], out[2]
            assert per >= 1 and hop == pitch and nbytes == frame + pitch * (per - 1)
            # both bounds, unless a single frame is already more than the budget
            assert per == 1 or (nbytes <= budget and per * 8 * N <= budget)
            # as many as fit: one more frame would break a bound (or there are no more)
            assert per == F or frame + pitch * per > budget or (per + 1) * 8 * N > budget
            # the pieces tile the frames exactly
            starts = list(range(0, F, per))
            assert sum(min(per, F - k0) for k0 in starts) == F and all(min(per, F - k0) >= 1 for k0 in starts)
        # with a frame step of one sample the rows, not the input, are the bound
        if S == 1 and N >= 8192:
            emul().rpf_emul_stft_pieces(frame, pitch, N, 1 << 40, out)
            assert out[0] == max(1, budget // (8 * N)) and out[1] < budget // 4


# ---- the float64 reference -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["cu8", "cs8", "cs16", "cf32"])
@pytest.mark.parametrize("N,step,hann", [(64, None, False), (512, 257, True), (1024, 512, False)])
def test_reference_rows_square_to_the_float64_power(fmt, N, step, hann):
    F = 7
    S = N if step is None else step
    stream = make_stream(fmt, 40 + N, N + S * (F - 1))
    w = synth.hann_window(N) if hann else None
    rows = stft.reference(stream, N, fmt, step=step, window=w)
    assert rows.shape == (F, N) and rows.dtype == np.complex128
    want = frame_truth.truth_frame_powers(N, frame_truth.unpacked(fmt, stream), F, window=w, step=step)
    got = rows.real ** 2 + rows.imag ** 2
    assert np.array_equal(got, want)
    assert np.allclose(got.sum(axis=0), want.sum(axis=0), rtol=1e-13, atol=0)
    # bin N/2 is DC: a constant stream lands there alone
    if fmt == "cu8" and not hann:
        const = np.full(2 * N, 137, dtype=np.uint8)
        r = stft.reference(const, N, fmt)
        assert abs(r[0, N // 2] - N * (10 + 10j)) < 1e-9 and np.abs(np.delete(r[0], N // 2)).max() < 1e-9


@pytest.mark.parametrize("fmt", ["cu8", "cf32"])
def test_reference_pfb_form_at_one_tap_is_the_plain_form(fmt):
    N, F = 256, 5
    stream = make_stream(fmt, 77, F * N)
    plain = stft.reference(stream, N, fmt)
    one = stft.reference(stream, N, fmt, taps=1, coeffs=np.ones(N, dtype=np.float32))
    assert np.array_equal(plain, one)
    h = pfb.coefficients(N, 4)
    four = stft.reference(stream, N, fmt, taps=4, coeffs=h)
    assert four.shape == (F - 3, N)
    assert stft.reference(stream[:10], N, fmt).shape == (0, N)


# ---- the CPU float32 figures behind the GPU test's bar -------------------------------------------------------------------

@pytest.mark.parametrize("fmt,N,form", stft_bars.ACCURACY_CASES)
def test_recorded_cpu_float32_error_is_what_the_cpu_path_gives(fmt, N, form):
    """stft_bars.CPU_F32 (half the GPU test's bar) against a fresh run of the path it records."""
    case = (fmt, N, form)
    stream = stft_bars.accuracy_stream(*case)
    window, taps, h = stft_bars.case_arguments(*case)
    folded = emul_fold(stream, stft_bars.ACCURACY_FRAMES, N, taps, fmt, h) if form == "pfb" else None
    frames = stft_bars.prepared_frames(stream, fmt, N, window=window, folded=folded)
    want = stft.reference(stream, N, fmt, window=window, taps=taps, coeffs=h)
    assert frames.shape[0] == want.shape[0] == stft_bars.ACCURACY_FRAMES
    if form != "pfb":
        assert np.array_equal(stft_bars.f64_rows(frames), want)      # the reference IS the transform of the prepared frames
    err = stft_bars.err(stft_bars.cpu_f32_rows(frames), want)
    print("CPU float32 path %s N=%d %s: err %.3e (recorded %.3e)" % (fmt, N, form, err, stft_bars.CPU_F32[case]))
    assert abs(err / stft_bars.CPU_F32[case] - 1.0) < 0.02
    assert stft_bars.BAR[case] == 2.0 * stft_bars.CPU_F32[case]


def test_every_accuracy_case_has_a_bar():
    assert set(stft_bars.CPU_F32) == set(stft_bars.ACCURACY_CASES) == set(stft_bars.BAR)
    assert set(stft_bars.MEASURED) <= set(stft_bars.ACCURACY_CASES)
    for case, got in stft_bars.MEASURED.items():
        assert got <= stft_bars.BAR[case], case


# ---- the CLI -------------------------------------------------------------------------------------------------------------

def run_cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True)


def test_cli_parses_the_option():
    r = run_cli("--help")
    assert r.returncode == 0 and "--stft <file>" in r.stdout
    # good command lines: what fails next is not the option (there is no device here, or the file is empty)
    for extra in (("-w", "/dev/null"), ("--frame-overlap", "50"), ("--pfb", "4"), ("--format", "cf32")):
        r = run_cli("--input", "/dev/null", "--stft", "/dev/null", "-b", "512", "-q", *extra)
        assert r.returncode != 3 or "--stft" not in r.stderr, r.stderr
    r = run_cli("--input", "/dev/null", "--stft")
    assert r.returncode == 4


@pytest.mark.parametrize("other,shown", [(("-n", "10"), "--repeats"), (("-t", "1"), "--time"), (("-c",), "--continue"),
                                         (("-e", "10"), "--elapsed"), (("-f", "100M:200M"), "frequency range"),
                                         (("-m", "out"), "-m"), (("--gpus", "0,1"), "--gpus"), (("--stats",), "--stats"),
                                         (("--series", "4"), "--series"), (("--series-stats", "4"), "--series-stats"),
                                         (("--excise", "4"), "--excise"), (("--quantile", "4"), "--quantile"),
                                         (("--cross", "/dev/null"), "--cross")])
def test_cli_refuses_what_stft_does_not_combine_with(other, shown):
    r = run_cli("--input", "/dev/null", "--stft", "/dev/null", *other)
    assert r.returncode == 3, r.stderr
    assert "--stft" in r.stderr and shown in r.stderr, r.stderr
    assert r.stdout == ""


def test_cli_stft_needs_input_and_a_power_of_two():
    r = run_cli("--stft", "/dev/null")
    assert r.returncode == 3 and "--stft" in r.stderr and "--input" in r.stderr, r.stderr
    r = run_cli("--input", "/dev/null", "--stft", "/dev/null", "-b", "500")
    assert r.returncode == 3 and "--stft" in r.stderr and "power-of-two" in r.stderr, r.stderr
