"""The piece rule of the series family's host routes, the parts that need no GPU: the plan of csrc/series_pieces.h
against a brute-force count (tests/emul/series_pieces_emul.cpp, compiled here), and the CLI's file reader
(host/piece_reader.h) walked over small files with a budget of a few hundred bytes (through librpf_host.so)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT
from test_host import host  # noqa: F401  (the fixture that loads librpf_host.so)


@pytest.fixture(scope="module")
def pieces(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("series_pieces") / "librpf_emul_series_pieces.so")
    subprocess.run(["g++", "-std=c++11", "-O1", "-fPIC", "-shared", "-o", lib,
                    os.path.join(ROOT, "tests", "emul", "series_pieces_emul.cpp")], check=True)
    lib = ctypes.CDLL(lib)
    lib.rpf_emul_series_pieces.argtypes = [ctypes.c_int] * 4 + [ctypes.c_longlong] * 4 + [ctypes.POINTER(ctypes.c_longlong)]
    lib.rpf_emul_series_pieces.restype = None
    return lib


# ---- the pieces of a host call (series_pieces.h) ------------------------------------------------------------------------
def frames_that_fit(frame, pitch, budget):
    """Brute force: the most frames f whose span (f - 1) pitch + frame is within the budget."""
    f = 0
    while f * pitch + frame <= budget:          # f + 1 frames still fit
        f += 1
    return f


def test_piece_plan_against_a_brute_force_count(pieces):
    out = (ctypes.c_longlong * 3)()
    checked = 0
    for b in (2, 4, 8):
        for N in (64, 500):
            for S in (N, N // 2, N // 2 + 1, 1):
                for taps in (0, 4) if S == N else (0,):          # (a PFB engine's frames advance by N)
                    frame, pitch = b * N * max(taps, 1), b * S
                    span = lambda frames: 0 if frames < 1 else frame + pitch * (frames - 1)
                    for L in (1, 3, 16):
                        budgets = [frame - 1, frame, span(L) - 1, span(L), span(L) + 1, 3 * L * pitch - 1, 3 * L * pitch,
                                   3 * L * pitch + 1, span(3 * L) - 1, span(3 * L), span(3 * L) + 2 * pitch + 1,
                                   span(3 * L + 3), 5 * L * pitch + 3 * pitch + b]
                        for budget in budgets:
                            fit = frames_that_fit(frame, pitch, budget) // L
                            full = max(1, fit)
                            for row_cap in (0, 1, 2, 1 << 40):          # 0: the series rule, else the excised rule
                                rows = full if row_cap == 0 else min(full, row_cap)
                                for K in sorted({1, max(1, rows - 1), rows, rows + 1, 3 * rows, 3 * rows + 1}):
                                    pieces.rpf_emul_series_pieces(b, N, S, taps, L, K, budget, row_cap, out)
                                    per_piece, nbytes, hop = list(out)
                                    assert per_piece == min(K, rows), (b, N, S, taps, L, K, budget, row_cap)
                                    assert 1 <= per_piece <= K
                                    assert nbytes == span(per_piece * L)
                                    assert fit == 0 or nbytes <= budget
                                    assert hop == L * b * S
                                    # the engine's loop, k0 = 0, per_piece, ...: the pieces tile [0, K), all full but the last
                                    starts = list(range(0, K, per_piece))
                                    sizes = [min(per_piece, K - k0) for k0 in starts]
                                    assert sum(sizes) == K and all(n == per_piece for n in sizes[:-1]) and 1 <= sizes[-1]
                                    assert [k0 * hop for k0 in starts] == [i * per_piece * L * b * S for i in range(len(starts))]
                                    # ... and every piece lies inside the bytes K integrations span
                                    assert starts[-1] * hop + span(sizes[-1] * L) == span(K * L)
                                    checked += 1
    assert checked > 10000


# ---- the series modes' file reader (piece_reader.h) -----------------------------------------------------------------
def piece_walk(host, path, frame, pitch, L, budget):
    """[(file offset, bytes held, integrations credited, the bytes handed over)] per piece and the reader's per_piece, or
    the shim's refusal: (-(exit code), message)."""
    ll = ctypes.c_longlong
    host.rpf_host_piece_walk.argtypes = [ctypes.c_char_p, ll, ll, ll, ll, ctypes.POINTER(ll), ctypes.POINTER(ll), ctypes.c_int,
                                         ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    host.rpf_host_piece_walk.restype = ll
    cap_pieces, cap_bytes = 64, 1 << 16
    per_piece, out4, got, msg = ll(), (ll * (4 * cap_pieces))(), ctypes.create_string_buffer(cap_bytes), ctypes.create_string_buffer(256)
    n = host.rpf_host_piece_walk(str(path).encode(), frame, pitch, L, budget, ctypes.byref(per_piece), out4, cap_pieces, got,
                                 cap_bytes, msg, 256)
    if n < 0:
        return n, msg.value.decode()
    span = lambda frames: 0 if frames < 1 else frame + pitch * (frames - 1)
    pieces = []
    for i in range(n):
        offset, have, done, at = out4[4 * i:4 * i + 4]
        pieces.append((offset, have, done, got.raw[at:at + span(done * L)]))
    return pieces, per_piece.value


@pytest.mark.parametrize("pitch", [16, 10])           # frames side by side, and overlapped: a carry-over at every seam
def test_piece_reader_hands_over_the_file_in_whole_integrations(host, tmp_path, pitch):
    frame, L, budget = 16, 3, 256                     # N = 8, cu8
    span = lambda frames: 0 if frames < 1 else frame + pitch * (frames - 1)
    frames_in = lambda nbytes: 0 if nbytes < frame else (nbytes - frame) // pitch + 1
    full = frames_in(budget) // L                     # integrations of a full piece: 5 side by side, 8 overlapped
    assert full >= 2
    rng = np.random.default_rng(20261019)
    tail = 3 * full * L * pitch + span(L) - 2         # three pieces and all but one sample of another integration
    sizes = [0, span(L) - 1, span(full * L), span(3 * full * L), tail, tail + 1]     # the last ends inside a sample
    assert tail % 2 == 0 and tail > span(3 * full * L) and frames_in(tail + 1) // L == 3 * full
    for size in sizes:
        data = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
        path = tmp_path / ("in_%d.bin" % size)
        path.write_bytes(data)
        for bud in (budget, span(L) - 1, 1):          # ... and a budget below one integration: one integration a piece
            pieces, per_piece = piece_walk(host, path, frame, pitch, L, bud)
            assert per_piece == (full if bud == budget else 1)
            total, offset = frames_in(size) // L, 0
            for i, (at, have, done, handed) in enumerate(pieces):
                assert at == offset                                          # the sum of done L pitch of the pieces before
                assert handed == data[at:at + span(done * L)] and len(handed) == span(done * L)
                assert at + have <= size and have <= span(per_piece * L)     # nothing from beyond the file, or the buffer
                assert done == (per_piece if i + 1 < len(pieces) else total - per_piece * (len(pieces) - 1))
                offset += done * L * pitch
            assert sum(done for _, _, done, _ in pieces) == total
            assert len(pieces) == -(-total // per_piece)


def test_piece_reader_refuses_a_missing_file(host, tmp_path):
    path = tmp_path / "absent.bin"
    assert piece_walk(host, path, 16, 16, 3, 256) == (-5, "Could not open %s." % path)
