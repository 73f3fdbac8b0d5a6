"""The band form's host side (no GPU): the theorem the band form rests on,
checked on random pairs with the tests' own matrices (tests/align_util.py,
tests/align_band_util.py); the per-pair decision on hand figures; the `-L` flag,
its refusals and its lines of the manual."""
import io
import os

import numpy as np
import pytest

from align_band_util import INF, band_cells, band_matrix, band_pair, decide, reference_align_band
from align_util import NO_DISTANCE, PAIR_COLS, PRIM_COLS, REPL, align_pair, check_properties, matrix, reference_align, trim, walk
from pangenome_amd.kmer import align_arg, band_arg, parse_args
from seq_util import fasta_records, make_fasta
from test_align_host import _refused_rank, mutate, site_records
from variants_util import reference_variants

THRESHOLDS = (1, 2, 4, 8, 16, 32, 64)


def random_pairs(n, seed):
    """Mutated pairs of 1 to 48 letters, a third over AC (many ties), edit
    rates from 3 % to 60 % and every fifth with a block inserted, trimmed to
    their cores."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        i = len(out)
        alpha = b"AC" if i % 3 == 0 else b"ACGT"
        T = bytes(alpha[x] for x in rng.integers(0, len(alpha), int(rng.integers(1, 49))))
        Q = bytearray(mutate(rng, T, (0.03, 0.1, 0.3, 0.6)[i % 4]))
        if i % 5 == 0:
            at = int(rng.integers(0, len(Q) + 1))
            Q[at:at] = bytes(alpha[x] for x in rng.integers(0, len(alpha), int(rng.integers(1, 20))))
        p, q = trim(T, bytes(Q))
        t, u = T[p:len(T) - q], bytes(Q)[p:len(Q) - q]
        if t and u:
            out.append((t, u))
    return out


def test_the_band_is_exact_on_random_pairs():
    """3,000 cores, every threshold t that holds |a - b|: B >= D everywhere,
    B[a][b] <= t iff D[a][b] <= t, and then the two walks are equal."""
    hold = fail = 0
    for t, u in random_pairs(3000, 17):
        a, b = len(t), len(u)
        D = matrix(t, u)
        ops = walk(D, t, u)
        for th in THRESHOLDS:
            if th < abs(a - b):
                continue
            B = band_matrix(t, u, th)
            assert (B[a][b] <= th) == (D[a][b] <= th)
            if D[a][b] <= th:
                assert B[a][b] == D[a][b] and walk(B, t, u) == ops
                hold += 1
            else:
                fail += 1
        th = THRESHOLDS[len(t) % 7]
        B = band_matrix(t, u, th)
        for i in range(a + 1):
            lo, hi = max(0, i - th), min(b, i + th)
            assert all(x == INF for x in B[i][:lo]) and all(x == INF for x in B[i][hi + 1:])
            assert all(x >= y for x, y in zip(B[i], D[i]))
    assert hold > 5000 and fail > 2000


def test_decide():
    assert band_cells(10, 20, 2) == 50 and band_cells(10, 4, 2) == 40
    # |a - b| = 3 needs t = 4 (k = 2); the distance 9 needs t = 16 (k = 4): three attempts of 90, 130, 130 cells
    assert decide(10, 13, 9, 1, 1 << 26) == (True, 3, 10 * 9 + 10 * 13 + 10 * 13)
    assert decide(10, 13, 4, 1, 1 << 26) == (True, 1, 90)
    # band_cap 100: t = 4 fits (90 cells), t = 8 does not (130): one attempt, not aligned
    assert decide(10, 13, 9, 1, 100) == (False, 1, 90)
    assert decide(10, 13, 9, 1, 89) == (False, 0, 0)
    assert decide(10, 13, 9, 1, 129) == (False, 1, 90) and decide(10, 13, 9, 1, 130) == (True, 3, 350)
    assert decide(100, 100, 0, 64, 1) == (False, 0, 0) and decide(100, 100, 0, 64, 10 ** 4) == (True, 1, 10 ** 4)


def test_band_pair_and_reference():
    T, Q = b"GGACGTACGTACCC", b"GGTCGTACGAACCC"                                # core ACGTACGT / TCGTACGA: 2 SNVs
    assert align_pair(T, Q, 1)["status"] == 1
    r, over, banded, attempts, cells = band_pair(T, Q, 1, 1, 1 << 26)
    assert (r, over, banded, attempts) == (align_pair(T, Q), 1, 1, 2) and cells == 8 * 3 + 8 * 5
    r, over, banded, attempts, cells = band_pair(T, Q, 1, 1, 8 * 3)
    assert (r["status"], r["distance"], r["prims"][0][0], over, banded, attempts) == (1, NO_DISTANCE, REPL, 1, 0, 1)
    assert band_pair(T, Q, 1, 1, 8 * 3 - 1)[1:] == (1, 0, 0, 0)
    assert band_pair(T, Q, 1 << 24, 1, 1)[1:] == (0, 0, 0, 0)                     # (below the cap: untouched)
    r, over, banded, attempts, cells = band_pair(b"GGATACC", b"GGCC", 1, 1, 1)  # an empty core side
    assert (r["status"], r["runs"], r["distance"], over, banded, attempts) == (0, [("=", 2), ("D", 3), ("=", 2)], 3, 1, 1, 0)
    sites = [[(T, 0, 1), (Q, 1, 1), (b"GGCC", 1, -1)], [(b"ACGT", 0, 1), (b"ACGT", 1, 1)]]
    recs, rows, grp = site_records(sites)
    names, seqs = fasta_records(make_fasta(recs))
    ref = reference_variants(rows, grp, 2, 2, seqs, 0)
    res = reference_align_band(ref, seqs, 1, 1, 1 << 26)
    band = res.pop("band")
    assert band == dict(n_over=2, n_banded=2, n_attempts=2, band_cells=64, attempts=[2, 0, 0])
    whole = reference_align(ref, seqs, 1 << 62)
    assert all(res[k] == whole[k] for k in PAIR_COLS + PRIM_COLS + ("op", "len", "lines"))
    check_properties(res)
    assert reference_align_band(ref, seqs, 1, 1, 24)["status"] == [1, 0, 0]
    assert reference_align(ref, seqs, 1)["status"] == [1, 1, 0]                  # (align_util is as it was)


# ------------------------------------------------------------ the flag
def test_parse_args_L():
    assert parse_args(["x", "-i", "f.fa"])["-L"] == "0"
    assert parse_args(["x", "-L", "1"])["-L"] == "1" and parse_args(["x", "-L1"])["-L"] == "1"
    assert band_arg({"-L": "0"}, False) is False and band_arg({"-L": "0"}, True) is False
    assert band_arg({"-L": "1"}, True) is True
    assert band_arg({"-L": "1"}, False) is None and band_arg({"-L": "1"}, None) is None
    assert band_arg({"-L": "2"}, True) is None and band_arg({"-L": "x"}, True) is None
    assert band_arg({"-L": "1"}, align_arg({"-A": "2"}, "g0")) is None


FULL = ["-V", "g0", "-g", "record", "-b", "5"]


@pytest.mark.parametrize("extra", [["-L", "1"], ["-L", "1"] + FULL, ["-L", "1", "-A", "0"] + FULL,
                                   ["-L", "1", "-A", "1", "-g", "record", "-b", "5"], ["-L", "1", "-A", "2"] + FULL,
                                   ["-L", "2", "-A", "1"] + FULL, ["-Lx", "-A", "1"] + FULL])
def test_bad_L_is_usage(tmp_path, extra):
    """Refused before anything is read or built: the manual, then SystemExit."""
    from pangenome_amd import kmer
    out = io.StringIO()
    with pytest.raises(SystemExit):
        kmer.entry_point(["x", "-i", str(tmp_path / "missing.fa"), "-k27", "-c3", "-a", "cc"] + extra, out=out)
    lines = out.getvalue().splitlines()
    assert lines[0] == "Usage:" and lines[-2].startswith("  -a:") and lines[-1].startswith("  -w:")
    assert os.listdir(str(tmp_path)) == []


def test_manual_has_two_L_lines():
    from pangenome_amd import kmer
    out = io.StringIO()
    kmer.manual_print(out)
    lines = out.getvalue().splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("  -L:")]
    assert len(at) == 1 and lines[at[0] - 1].startswith("  -d:") and lines[at[0] + 2].startswith("  -r:")
    assert "with -A 1" in lines[at[0]] and "band" in lines[at[0]]
    assert lines[at[0] + 1].startswith("      ") and "0 (off) or 1" in lines[at[0] + 1]
    assert [ln[:5] for ln in lines[-3:]] == ["  -c:", "  -a:", "  -w:"]


def test_dist_entry_point_refuses_L(tmp_path):
    """The multi-process CLI refuses -L as it refuses -A: the manual on rank
    0, then SystemExit, before anything is built."""
    from dist_util import spawn_ranks
    from golden_util import Fixture
    fx = Fixture("pan8_k27_c3")
    q = tmp_path / "input.fsa"
    q.write_bytes(fx.fasta)
    argv = ["kmer_numba.py", "-i", str(q), "-k", str(fx.k), "-c", str(fx.c), "-a", "cc", "-w", "4", "-L", "1"]
    exited, text = spawn_ranks(1, _refused_rank, (argv,))[0]
    lines = text.splitlines()
    assert exited and lines[0] == "Usage:" and sum(ln.startswith("  -L:") for ln in lines) == 1
    assert os.listdir(str(tmp_path)) == ["input.fsa"]
