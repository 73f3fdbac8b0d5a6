"""The band form of pg_region_align (PG_TUNE_ALIGN_BAND; k_al_fill_band in
pangenome_amd/csrc/pg_align.hip): the pairs above the cells cap aligned in a
band of diagonals whose threshold doubles.

Every case compares the device exactly - counts, the four tables, both texts -
with the list-based reference: tests/align_util.py at an unlimited cells cap,
which the band form promises to equal, or tests/align_band_util.py where pairs
are given up.  With PG_TUNE_ALIGN_CELLS at 1 every pair with a letter in its
core is above the cap, and with PG_TUNE_ALIGN_BAND_T0 at 1 the band's edges and
its doubling show on cores of a few letters.  Every tune is put back in a
`finally`."""
import contextlib
import os

import numpy as np
import pytest

from align_band_util import BAND_CAP, UNLIMITED, band_cells, check_align_band, cores_of, figures_of
from align_util import (DEL, INS, NO_DISTANCE, REPL, assert_same, check_align, check_properties, check_vcf, cigar,
                        device_state, reference_align)
from golden_util import Fixture
from pangenome_rows_util import BORDERS, other
from seq_util import make_fasta, parse
from test_align_host import HAND, mutate, site_records
from test_gpu_align import _run, acgt, border_site, tie_sites
from variants_util import reference_variants

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pangenome_amd._lib import Context
    c = Context(27, 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def km():
    from pangenome_amd import kmer
    return kmer


@contextlib.contextmanager
def tuned(c, band=1, cells=0, t0=0, band_cap=0, scratch=0):
    """The five tunes of the alignment set, and all back at their defaults after."""
    from pangenome_amd import _lib
    ids = (_lib.PG_TUNE_ALIGN_BAND, _lib.PG_TUNE_ALIGN_CELLS, _lib.PG_TUNE_ALIGN_BAND_T0,
           _lib.PG_TUNE_ALIGN_BAND_CELLS, _lib.PG_TUNE_ALIGN_SCRATCH)
    try:
        for what, v in zip(ids, (band, cells, t0, band_cap, scratch)):
            c.tune(what, v)
        yield
    finally:
        for what in ids:
            c.tune(what, 0)


def counts_of(res):
    return res["n_pairs"], res["n_aligned"], res["n_ops_all"], res["n_prims_all"], res["n_lines"]


def equals_full(c, sites, ref_group, G=2, t0s=(1, 4, 64)):
    """Every pair above the cap (cells_cap 1), the band on: at every t0 the
    device equals the reference at an unlimited cap, and region_align_band()'s
    counts are the decision's.  Returns the reference."""
    from pangenome_amd._lib import PG_TUNE_ALIGN_BAND_T0
    recs, rows, grp = site_records(sites)
    names, seqs = parse(c, make_fasta(recs))
    with tuned(c, cells=1, t0=t0s[0]):
        res, _, _ = check_align(c, rows, grp, G, 2, names, seqs, ref_group, cells_cap=UNLIMITED)
        for t0 in t0s:
            c.tune(PG_TUNE_ALIGN_BAND_T0, t0)
            assert c.region_align() == counts_of(res)
            assert_same(c, res, names, seqs)
            want = figures_of(res, 1, t0, BAND_CAP)
            assert c.region_align_band()[:4] == want[:4] and want[0] == want[1] and not any(want[5])
    return res


# ------------------------------------------------------------ 1. equals the unlimited full form
def test_hand_cases_banded(ctx):
    """tests/test_align_host.py's hand cases, one site each, with the CIGARs
    typed out there."""
    res = equals_full(ctx, [[(T, 0, 1), (Q, 1, 1)] for T, Q, _, _, _ in HAND], 0)
    assert [cigar(res, j) for j in range(res["n_pairs"])] == [h[2] for h in HAND]
    assert figures_of(res, 1, 1)[0] == 7                  # (all but the two pairs with nothing in their cores)


@pytest.mark.parametrize("shift", range(16))
def test_strip_and_word_borders_banded(ctx, shift):
    """test_gpu_align.py's border site: cores of 1 to 129 letters (and the
    empty ones) at every offset mod 16, related and unrelated by turns."""
    res = equals_full(ctx, border_site(shift), 0, G=3)
    assert res["n_pairs"] == 144 == res["n_aligned"] and figures_of(res, 1, 1)[0] == 143
    assert set(cores_of(res)) >= {(a, b) for a in BORDERS for b in BORDERS if a * b != 1}
    assert max(figures_of(res, 1, 1)[4]) >= 7             # doubled from 1 to 64 and beyond


@pytest.mark.parametrize("unit", [b"A", b"AC", b"ACG"])
def test_ties_banded(ctx, unit):
    """Every place of the gap co-optimal: the leftmost one, |a - b| = len(unit)
    columns from the main diagonal, which is the band's edge at t0 = 1 for AC
    (t = 2) and at t0 = 4 for none - the rule must hold on and off the edge."""
    res = equals_full(ctx, tie_sites(unit), 0)
    assert res["prefix"] == [0] * res["n_pairs"] == res["suffix"] and max(res["t_len"]) >= 68
    u = len(unit)
    for j in range(res["n_pairs"]):
        n = res["op_off"][j]
        assert chr(res["op"][n]) == ("D" if res["q_len"][j] < res["t_len"][j] else "I") and res["len"][n] == u


# ------------------------------------------------------------ 2. band edges and doubling
def snvs(T, places):
    Q = bytearray(T)
    for x in places:
        Q[x] = other(T[x])
    return bytes(Q)


def edge_sites():
    """Cores with nothing to trim (first and last columns differ).  A path on
    the edge diagonal itself would need every edit to be that one gap and
    leave equal letters behind it to trim, so the longest run beside the edge
    is on diagonal t - 1, with one SNV at the far end."""
    S, L = acgt(24, 500), acgt(140, 501)
    gg = lambda n, seed: bytes(other(x) for x in acgt(n, seed))
    sites = []
    # |a - b| = 4 = D = t: the end cell on the last diagonal, reached by insertions (deletions) at both ends
    sites.append([(S, 0, 1), (snvs(S, [0])[:1] * 2 + S + snvs(S, [23])[-1:] * 2, 1, 1)])
    sites.append([(snvs(S, [0])[:1] * 2 + S + snvs(S, [23])[-1:] * 2, 0, 1), (S, 1, 1)])
    # D = 4, a threshold, and 5, a threshold plus one; 8 and 9
    W = acgt(40, 502)
    sites.append([(W, 0, 1), (snvs(W, [0, 13, 27, 39]), 1, 1), (snvs(W, [0, 13, 14, 27, 39]), 2, 1),
                  (snvs(W, [0, 3, 9, 13, 20, 27, 33, 39]), 1, 1), (snvs(W, [0, 3, 9, 13, 20, 21, 27, 33, 39]), 2, -1)])
    # 140 rows beside the edge: 7 letters inserted (deleted) at the start and an SNV at the end, D = 8 = t
    ins = gg(7, 503)
    sites.append([(L, 0, 1), (bytes([other(L[0])]) + ins[1:] + snvs(L, [139]), 1, 1)])
    sites.append([(bytes([other(L[0])]) + ins[1:] + L, 0, 1), (snvs(L, [139]), 1, 1)])
    # |a - b| = 8 = D = t over three strips: 4 letters at either end, the end cell on the last diagonal
    sites.append([(L, 0, 1), (bytes([other(L[0])]) * 4 + L + bytes([other(L[-1])]) * 4, 1, 1)])
    return sites


def test_band_edges_and_doubling(ctx):
    recs, rows, grp = site_records(edge_sites())
    names, seqs = parse(ctx, make_fasta(recs))
    with tuned(ctx, cells=1, t0=1):
        res, _, vcf = check_align_band(ctx, rows, grp, 3, 2, names, seqs, 0, cells_cap=1, t0=1)
    assert res["prefix"] == [0] * 9 == res["suffix"] and res["status"] == [0] * 9
    assert res["distance"] == [4, 4, 4, 5, 8, 9, 8, 8, 8] and res["band"]["attempts"] == [1, 1, 3, 4, 4, 5, 1, 1, 1]
    assert cores_of(res) == [(24, 28), (28, 24)] + [(40, 40)] * 4 + [(140, 147), (147, 140), (140, 148)]
    assert [cigar(res, j) for j in (0, 1, 6, 7, 8)] == [b"2I24=2I", b"2D24=2D", b"7I139=1X", b"7D139=1X", b"4I140=4I"]
    check_properties(res)
    check_vcf(res, vcf, names, seqs)


# ------------------------------------------------------------ 3. an empty core side above the cap
def test_empty_core_side(ctx):
    A = acgt(30, 510)
    sites = [[(A, 0, 1), (A[:10] + A[17:], 1, 1), (A[:10] + b"GATTACA" + A[10:], 2, -1)],
             [(b"", 0, 1), (b"ACG", 1, 1)], [(b"ACG", 0, 1), (b"", 1, -1)]]
    recs, rows, grp = site_records(sites)
    names, seqs = parse(ctx, make_fasta(recs))
    with tuned(ctx, cells=1):
        res, tsv, _ = check_align_band(ctx, rows, grp, 3, 2, names, seqs, 0, cells_cap=1)
    assert res["status"] == [0, 0, 0, 0] and res["type"] == [DEL, INS, INS, DEL] and REPL not in res["type"]
    assert [cigar(res, j) for j in range(4)] == [b"10=7D13=", b"9=7I21=", b"3I", b"3D"]
    assert res["distance"] == [7, 7, 3, 3] and res["band"] == dict(n_over=4, n_banded=4, n_attempts=0, band_cells=0,
                                                                   attempts=[0] * 4)
    with tuned(ctx, band=0, cells=1):                      # (off: the same pairs are replacements)
        off = check_align(ctx, rows, grp, 3, 2, names, seqs, 0, cells_cap=1)[0]
    assert off["status"] == [1] * 4 and off["type"] == [REPL] * 4


# ------------------------------------------------------------ 4. band_cap
def test_band_cap(ctx):
    """Three pairs that need t = 8 at t0 = 1, whose bands there take 63, 64
    and 65 cells, at band_cap 64: aligned, aligned, given up - before its
    first attempt, because |a - b| = 8 lets it join at t = 8 only."""
    sites = [[(b"ACACTCA", 0, 1), (b"GCGATCTTG", 1, 1)], [(b"ACGTTGCA", 0, 1), (b"CAGTACAT", 1, 1)],
             [(b"ACACA", 0, 1), (b"GACACAGGGGGGG", 1, 1)]]
    recs, rows, grp = site_records(sites)
    names, seqs = parse(ctx, make_fasta(recs))
    whole = reference_align(reference_variants(rows, grp, 2, 2, seqs, 0), seqs, UNLIMITED)
    assert cores_of(whole) == [(7, 9), (8, 8), (5, 13)] and all(4 < d <= 8 for d in whole["distance"])
    assert [band_cells(a, b, 8) for a, b in cores_of(whole)] == [63, 64, 65]
    with tuned(ctx, cells=1, t0=1, band_cap=64):
        res, tsv, _ = check_align_band(ctx, rows, grp, 2, 2, names, seqs, 0, cells_cap=1, t0=1, band_cap=64)
        assert res["status"] == [0, 0, 1] and res["band"]["attempts"] == [3, 4, 0]
        given_up = device_state(ctx, names, 2)
    assert (res["distance"][2], res["n_prims"][2], res["type"][-1]) == (NO_DISTANCE, 1, REPL)
    assert tsv.split(b"\n")[3].split(b"\t")[8:] == [b".", b"0", b"0", b"13", b"5", b"5D13I"]
    with tuned(ctx, band=0, cells=1):                      # today's form of that pair, byte for byte
        ctx.region_align()
        plain = device_state(ctx, names, 2)
    own = [k for k in plain[0][0] if k not in ("op_off", "prim_off")]    # (the offsets count the other pairs' entries)
    assert [plain[0][0][k][2] for k in own] == [given_up[0][0][k][2] for k in own]
    assert [plain[0][2][k][-1] for k in plain[0][2]] == [given_up[0][2][k][-1] for k in given_up[0][2]]
    assert plain[1].split(b"\n")[3] == given_up[1].split(b"\n")[3]
    with tuned(ctx, cells=1, t0=1, band_cap=65):
        res = check_align_band(ctx, rows, grp, 2, 2, names, seqs, 0, cells_cap=1, t0=1, band_cap=65)[0]
        assert res["status"] == [0, 0, 0]
    with tuned(ctx, cells=1, t0=1, band_cap=63):
        res = check_align_band(ctx, rows, grp, 2, 2, names, seqs, 0, cells_cap=1, t0=1, band_cap=63)[0]
        assert res["status"] == [0, 1, 1] and res["band"]["attempts"] == [3, 2, 0]


# ------------------------------------------------------------ 5. a drifting diagonal over many strips
def test_drifting_diagonal(ctx):
    """1,500 against about 1,650 letters at 1 % edits with two insertions of
    80 letters and a deletion of 10: the path drifts 150 columns off the main
    diagonal over 24 strips, and |a - b| alone asks for t = 256.  Beside it
    1,500 unrelated letters against 1,500, which band_cap 2^20 gives up after
    the attempts at 64, 128 and 256."""
    rng = np.random.default_rng(21)
    T = acgt(1500, 520)
    Q = bytearray(mutate(rng, T, 0.01))
    Q[1100:1110] = b""
    Q[900:900] = acgt(80, 521)
    Q[300:300] = acgt(80, 522)
    Q[0], Q[-1] = other(T[0]), other(T[-1])
    sites = [[(T, 0, 1), (bytes(Q), 1, -1)], [(b"A" + acgt(1498, 523) + b"A", 0, 1), (b"C" + acgt(1498, 524) + b"C", 1, 1)]]
    recs, rows, grp = site_records(sites)
    names, seqs = parse(ctx, make_fasta(recs))
    with tuned(ctx, cells=1 << 16, t0=64, band_cap=1 << 20):
        res, _, vcf = check_align_band(ctx, rows, grp, 2, 2, names, seqs, 0, cells_cap=1 << 16, t0=64, band_cap=1 << 20)
        cells, ms = ctx.region_align_band()[3:]
    assert res["prefix"] == [0, 0] == res["suffix"] and res["status"] == [0, 1]
    assert 128 < res["distance"][0] <= 256 and 1640 <= res["q_len"][0] <= 1660
    assert res["band"]["attempts"] == [1, 3] and cells == 1500 * 513 + 1500 * (129 + 257 + 513) and ms > 0
    check_properties(res)
    check_vcf(res, vcf, names, seqs)
    print("drifting diagonal: %d band cells in %.3f ms" % (cells, ms))


# ------------------------------------------------------------ 6. the product setting
def test_product_setting(ctx):
    """One pair of 4,200 letters against about 4,200 with about 20 edits and
    differing ends: just above the default cells cap, so that today it is one
    replacement; with the band on and every other tune at its default it is
    what the full matrix gives, in one attempt at t = 64."""
    rng = np.random.default_rng(22)
    T = acgt(4200, 530)
    Q = bytearray(mutate(rng, T, 0.005))
    Q[0], Q[-1] = other(T[0]), other(T[-1])
    recs, rows, grp = site_records([[(T, 0, 1), (bytes(Q), 1, 1)]])
    names, seqs = parse(ctx, make_fasta(recs))
    with tuned(ctx):
        res, _, vcf = check_align_band(ctx, rows, grp, 2, 2, names, seqs, 0)
        n_over, n_banded, attempts, cells, ms = ctx.region_align_band()
        assert ctx.region_align_time() == (0.0, 0)         # (the full form filled nothing)
    a, b = cores_of(res)[0]
    assert a == 4200 and (a + 1) * (b + 1) > 1 << 24 and res["status"] == [0] and 10 <= res["distance"][0] <= 40
    assert (n_over, n_banded, attempts) == (1, 1, 1) and cells == 4200 * 129 < 1 << 21 and ms > 0
    check_properties(res)
    check_vcf(res, vcf, names, seqs)
    print("product setting: %d band cells in %.3f ms" % (cells, ms))
    with tuned(ctx, band=0):
        assert ctx.region_align()[1] == 0 and ctx.region_align_band() == (0, 0, 0, 0, 0.0)


# ------------------------------------------------------------ 7. batches and rounds
def test_batches_and_rounds(ctx):
    """432 pairs, 363 of them candidates that leave in rounds from t = 1 to t
    = 128: one pair per batch, a few, and all in one give the same state."""
    sites = border_site(7) + border_site(2) + border_site(12)
    recs, rows, grp = site_records(sites)
    names, seqs = parse(ctx, make_fasta(recs))
    ctx.region_bubbles(grp, 3, 2, rows=rows)
    ctx.region_variants(grp, 3, 0, rows=rows)
    states = []
    for scratch in (0, 1, 1 << 12):
        with tuned(ctx, cells=1, t0=1, scratch=scratch):
            assert ctx.region_align()[:2] == (432, 432)
            states.append((device_state(ctx, names, 3), ctx.region_align_band()[:4]))
    assert states[0] == states[1] == states[2]
    n_over, n_banded, attempts, _ = states[0][1]
    assert n_over == n_banded == 429 and attempts > 600


# ------------------------------------------------------------ 8. poison
@pytest.mark.parametrize("t0", [1, 64])
def test_poison_banded(t0):
    """Case 1's borders in a fresh context whose every new device buffer is
    filled with 0xA5 first: a row value, a choice word or a letter read from
    outside the band, where nothing wrote, would show."""
    from pangenome_amd._lib import PG_TUNE_POISON, Context
    c = Context(27, 0)
    try:
        c.tune(PG_TUNE_POISON, 0xA5)
        for ref_group in (0, None):
            res = equals_full(c, border_site(3), ref_group, G=3, t0s=(t0,))
            assert res["n_pairs"] == 144
    finally:
        c.tune(PG_TUNE_POISON, -1)
        c.close()


# ------------------------------------------------------------ 9. off is off
def test_off_is_off(ctx):
    from pangenome_amd import _lib
    from pangenome_amd._lib import Context, PangenomeError
    recs, rows, grp = site_records(border_site(7))
    names, seqs = parse(ctx, make_fasta(recs))
    with tuned(ctx, band=1, cells=64):
        ctx.tune(_lib.PG_TUNE_ALIGN_BAND, 0)
        capped = check_align(ctx, rows, grp, 3, 2, names, seqs, 0, cells_cap=64)[0]
        assert 0 < capped["n_aligned"] < 144 and capped["type"].count(REPL) == 144 - capped["n_aligned"]
        assert ctx.region_align_band() == (0, 0, 0, 0, 0.0)
        ctx.tune(_lib.PG_TUNE_ALIGN_BAND, 1)
        assert ctx.region_align()[1] == 144 and ctx.region_align_band()[0] == 144 - capped["n_aligned"]
    for what, bad in ((_lib.PG_TUNE_ALIGN_BAND, (-1, 2)), (_lib.PG_TUNE_ALIGN_BAND_CELLS, (-1, (1 << 34) + 1)),
                      (_lib.PG_TUNE_ALIGN_BAND_T0, (-1, (1 << 20) + 1))):
        for v in bad:
            with pytest.raises(PangenomeError, match=r"pg_tune failed \(-22\)"):
                ctx.tune(what, v)
    ctx.tune(_lib.PG_TUNE_ALIGN_BAND_CELLS, 1 << 34)
    ctx.tune(_lib.PG_TUNE_ALIGN_BAND_T0, 1 << 20)
    ctx.tune(_lib.PG_TUNE_ALIGN_BAND_CELLS, 0)
    ctx.tune(_lib.PG_TUNE_ALIGN_BAND_T0, 0)
    assert ctx.lib.pg_region_align_band(ctx.h, None, None, None, None, None) == 0
    assert ctx.lib.pg_region_align_band(None, None, None, None, None, None) == -22
    fresh = Context(27, 0)
    try:
        with pytest.raises(PangenomeError, match=r"pg_region_align_band failed \(-22\)"):
            fresh.region_align_band()
    finally:
        fresh.close()


# ------------------------------------------------------------ 10. the CLI
def test_cli_L(km, tmp_path):
    """Nothing of pan8_k27_c3 comes near the cap: -L 1 writes -A 1's files."""
    fx = Fixture("pan8_k27_c3")
    first = fx.fasta.split(b"\n", 1)[0][1:].split()[0].decode()
    base = ["-g", "record", "-b", "5", "-V", first, "-A", "1"]
    q0, plain = _run(km, tmp_path / "plain", fx.fasta, base)
    q, lines = _run(km, tmp_path / "band", fx.fasta, base + ["-L", "1"])
    assert lines == plain and sorted(os.listdir(os.path.dirname(q))) == sorted(os.listdir(os.path.dirname(q0)))
    for f in ("_fr_align.tsv", "_fr_primitives.vcf"):
        assert open(q + f, "rb").read() == open(q0 + f, "rb").read() != b""
    d = tmp_path / "bad"
    with pytest.raises(SystemExit):
        _run(km, d, fx.fasta, ["-g", "record", "-b", "5", "-V", first, "-L", "1"])
    assert os.listdir(str(d)) == ["pan8.fsa"]
