"""The CLI's series modes across a piece seam on the MI355X: a file above 64 MB read in two pieces."""
import subprocess

import pytest

from test_gpu_series import CLI, blocks_of, one_unit_of_the_last_digit, random_bytes

pytestmark = pytest.mark.gpu


def test_cli_series_across_a_piece_seam(tmp_path):
    """A file above 64 MB goes through the CLI's reader in two pieces, of four integrations and of one; the half
    integration at its end is dropped.  16 MB per integration: a multiple of 16384 bytes, so -c stays contiguous."""
    N, L, K = 8192, 1024, 5
    assert (L * 2 * N) % 16384 == 0 and 4 * L * 2 * N == 64 << 20
    path = tmp_path / "rec.bin"
    random_bytes(53, 2 * N * (K * L + L // 2)).tofile(str(path))
    common = [CLI, "-b", str(N), "--input", str(path)]
    a = subprocess.run(common + ["--series", str(L)], capture_output=True, text=True)
    r = subprocess.run(common + ["-q", "-c", "-n", str(L)], capture_output=True, text=True)
    assert a.returncode == 0, a.stderr
    assert r.returncode == 0, r.stderr
    assert "Spectra written: %d, %d frames each (one launch per piece)" % (K, L) in a.stderr
    got, want = blocks_of(a.stdout), blocks_of(r.stdout)[:K]      # (-c goes on to average the half integration that is left)
    assert len(got) == len(want) == K
    worst = 0.0
    for g, w in zip(got, want):
        assert len(g) == len(w) == N
        assert [x[0] for x in g] == [x[0] for x in w]                    # the frequency column
        for (_, pg), (_, pw) in zip(g, w):
            unit = max(one_unit_of_the_last_digit(pg), one_unit_of_the_last_digit(pw))
            worst = max(worst, abs(float(pg) - float(pw)) / unit)
            assert abs(float(pg) - float(pw)) <= unit * (1 + 1e-9), (pg, pw)
    print("pieces of 4 and 1: %d blocks, worst difference %.3g units of the last printed digit" % (K, worst))
