"""What the three passes over the region rows refuse, once for all of them
(pg_freq, pg_region_graph, pg_region_seqs share row_input, pangenome_amd/csrc/
pg_region.hip): the return code, the message, and the previous result left in
place.  Every case is refused on the host before any launch.

9 records (pan8 and its first record once more), 4 groups, 500 host rows that
lie inside their records; the context has gone through a parse and a row pass,
so the device rows and the bases are there too.
"""
import ctypes as C

import numpy as np
import pytest

from golden_util import Fixture

pytestmark = pytest.mark.gpu

PASSES = ("pg_freq", "pg_region_graph", "pg_region_seqs")
N_OUT = {"pg_freq": 3, "pg_region_graph": 4, "pg_region_seqs": 3}
NAMES = [b"r%d" % r for r in range(9)]


def fasta9():
    fasta = Fixture("pan8_k27_c3").fasta
    first = fasta.split(b">")[1]
    return fasta + b">again " + first


@pytest.fixture(scope="module")
def ctx():
    from pangenome_amd._lib import Context
    c = Context(27, 0)
    c.parse_host(np.frombuffer(fasta9(), np.uint8))
    assert c.n_records == 9
    c.build_dbg(None, 0, True)
    c.build_rdbg()
    c.edges_count(None, True)
    c.cluster_cc(None, None, 4)
    assert c.rows_count(None, True) > 0
    yield c
    c.close()


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(21)
    n = 500
    start = rng.integers(0, 1000, n)
    rows = np.stack([np.sort(rng.integers(0, 9, n)), start, start + rng.integers(1, 500, n), rng.choice([1, -1], n),
                     rng.integers(0, 20, n)], axis=1).astype(np.int64)
    rows[rng.integers(0, n, 10), 4] = -1
    return np.ascontiguousarray(rows), rng.permutation(np.arange(9) % 4).astype(np.int32)


def call(c, name, rows, n_rows, group, n_records, G):
    """The pass through the ABI with no outputs: 0, or (code, PangenomeError's text)."""
    from pangenome_amd._lib import PangenomeError, check, ptr
    rc = getattr(c.lib, name)(c.h, ptr(rows), n_rows, ptr(group), n_records, G, *[None] * N_OUT[name])
    if rc == 0:
        return 0
    with pytest.raises(PangenomeError) as e:
        check(rc, name)
    return rc, str(e.value)


def text_of(c, name):
    if name == "pg_freq":
        return c.freq_text()
    return c.region_links_text() if name == "pg_region_graph" else c.region_fasta_text(NAMES)


@pytest.mark.parametrize("name", PASSES)
def test_refusals(ctx, case, name):
    from pangenome_amd._lib import Context
    rows, group = case

    assert call(ctx, name, rows, 500, group, 9, 4) == 0
    kept = text_of(ctx, name)
    assert kept.count(b"\n") > 1

    def refused(what, *args, c=ctx):
        assert call(c, name, *args) == (-22, "%s failed (-22): %s: %s" % (name, name, what))
        assert text_of(ctx, name) == kept                # the previous result is in place

    refused("rec_group is NULL", rows, 500, None, 9, 4)
    for bad in (4, -2):
        g2 = group.copy()
        g2[3] = bad
        refused("rec_group[3] = %d is outside [-1, 4)" % bad, rows, 500, g2, 9, 4)
    for bad in (-1, 9):
        r2 = rows.copy()
        r2[17, 0] = bad
        refused("row 17 names record %d of 9" % bad, r2, 500, group, 9, 4)
    refused("n_groups is 0 with rows", rows, 500, np.full(9, -1, np.int32), 9, 0)
    fresh = Context(27, 0)
    try:
        if name == "pg_region_seqs":
            refused("no parse (the bases come from the context's parse)", None, 0, group, 9, 4, c=fresh)
            fresh.parse_host(np.frombuffer(fasta9(), np.uint8))
        refused("no row pass (call pg_rows first, or pass rows)", None, 0, group, 9, 4, c=fresh)
    finally:
        fresh.close()
    # the record count: with the device rows it must be the context's
    refused("8 records, the context has 9", None, 0, group[:8].copy(), 8, 4)
    # ... with host rows only pg_region_seqs insists (its bases are the context's); the other two take
    # any count that covers the rows' records
    g10 = np.append(group, np.int32(-1))
    if name == "pg_region_seqs":
        refused("10 records, the context has 9", rows, 500, g10, 10, 4)
    else:
        assert call(ctx, name, rows, 500, g10, 10, 4) == 0
    assert text_of(ctx, name) == kept
