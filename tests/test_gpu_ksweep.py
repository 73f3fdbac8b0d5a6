"""The device at every k-mer length from 1 to 27, bit-exact against the CPU
oracle on tests/ksweep_util.py's sweep input (tests/test_ksweep_util.py pins
that oracle to a numpy restatement at the same k and shows that the input
sees a wrong coverage pass at k >= 8).

k reshapes the hot path: init_keys splits the base-5 key at 13 digits (k = 14
is the first with a high part, k = 27 has a kernel of its own); the packed
coverage pass smears mismatches over 16/8/4/2 bases and folds by
2 * (k + 2 - P) bits (P changes at k = 2, 6, 14, where the fold is by 0); the
table's bucket bits are clamped to [max(cbits, kb - 38), kb]; the walks and the
persistence use 5^(k-1) and 5^k; the routed exchange rotates h by as many bits
as there are owner bits, all kb of them with 8 owners at k = 1 and 32 at k = 2.
"""
import numpy as np
import pytest

import ksweep_util as ku
from test_gpu_parity import run_stages

pytestmark = pytest.mark.gpu

EXCHANGE_KS = (1, 2, 3, 6, 13, 14, 20, 27)
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _shared():
    """The inputs and the oracle's runs over them, shared by this module's
    tests and freed with it."""
    yield
    _cache.clear()


@pytest.fixture(scope="module")
def km():
    from pangenome_amd import kmer
    return kmer


def sweep(k):
    if ("fasta", k) not in _cache:
        _cache["fasta", k] = ku.sweep_fasta(k)
    return _cache["fasta", k]


class Ref:
    def __init__(self, oracle, k, c):
        self.run = oracle.OracleRun(sweep(k), k, c)
        self.keys, self.masks = self.run.dbg()
        self.rdbg = self.run.rdbg()


def ref_of(oracle, k, c):
    """The oracle's dBG and rdBG of sweep_fasta(k) at strand bits c (computed once)."""
    if ("ref", k, c) not in _cache:
        _cache["ref", k, c] = Ref(oracle, k, c)
    return _cache["ref", k, c]


def key_bits(k):
    return max(1, (5 ** k - 1).bit_length())


def check_graph(ctx, ref, what, st=None):
    keys, masks = ctx.dbg()
    assert np.array_equal(keys, ref.keys), what
    assert np.array_equal(masks, ref.masks), what
    assert np.array_equal(ctx.rdbg(), ref.rdbg), what
    if st is not None:
        assert (st.n_dbg, st.n_rdbg) == (ref.keys.shape[0], ref.rdbg.shape[0]), what


# ------------------------------------------------------------ 1: the pipeline
@pytest.mark.parametrize("k", ku.KS)
def test_pipeline(km, oracle_mod, tmp_path, k):
    """seq2rdbg, dbg2rdbg and seq2graph against oracle.run_pipeline: dBG keys
    and masks, rdBG, `.xyz` text and region rows."""
    fasta = sweep(k)
    if ("pipe", k) not in _cache:
        _cache["pipe", k] = oracle_mod.run_pipeline(fasta, k, 3)
    ref = _cache["pipe", k]
    got = run_stages(km, fasta, k, 3, None, "", tmp_path)
    assert np.array_equal(got["dbg_keys"], ref["dbg_keys"])
    assert np.array_equal(got["dbg_masks"], ref["dbg_masks"])
    assert np.array_equal(got["rdbg_keys"], ref["rdbg_keys"])
    assert got["xyz"] == ref["xyz"]
    assert got["rows"] == ref["rows"]


# ------------------------------------------------------- 2: every build form
@pytest.mark.parametrize("rc0", (True, False))
@pytest.mark.parametrize("k", ku.KS)
def test_build_paths(oracle_mod, k, rc0):
    """Every way into the build on one context: pg_build_host in 16 KiB upload
    chunks on the fresh context (cold) and again (warm: sized from the first),
    the three-call path, pg_build, pg_build_device, pg_build with the tile list
    in four chunks and with a table 8x smaller than sized."""
    import torch
    from pangenome_amd._lib import Context, PG_TUNE_BUCKET_SHIFT, PG_TUNE_H2D_CHUNK, PG_TUNE_K3_CHUNKS
    fasta = sweep(k)
    ref = ref_of(oracle_mod, k, 2 * int(rc0))
    dev = torch.frombuffer(bytearray(fasta), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    ctx = Context(k)
    try:
        ctx.tune(PG_TUNE_H2D_CHUNK, 16384)
        for what in ("build_host cold", "build_host warm"):
            check_graph(ctx, ref, what, ctx.build_host(fasta, rc0))
        ctx.tune(PG_TUNE_H2D_CHUNK, 0)
        ctx.set_fasta(fasta)
        ctx.parse()
        st = ctx.build_dbg(None, 0, rc0)
        assert st.n_dbg == ref.keys.shape[0]
        check_graph(ctx, ref, "parse + build_dbg + build_rdbg", ctx.build_rdbg())
        check_graph(ctx, ref, "build", ctx.build(None, 0, rc0))
        check_graph(ctx, ref, "build_device", ctx.build_device(dev.data_ptr(), dev.numel(), rc0, keepalive=dev))
        ctx.tune(PG_TUNE_K3_CHUNKS, 4)
        check_graph(ctx, ref, "build, 4 chunks", ctx.build(None, 0, rc0))
        ctx.tune(PG_TUNE_K3_CHUNKS, 0)
        ctx.tune(PG_TUNE_BUCKET_SHIFT, 3)
        check_graph(ctx, ref, "build, bucket shift 3", ctx.build(None, 0, rc0))
    finally:
        ctx.close()


# ------------------------------------------------ 3: coverage did something
@pytest.mark.parametrize("k", ku.KS)
def test_coverage_skips_what_the_lead_holds(oracle_mod, k):
    """The coverage pass skips follower windows the lead holds: stage A emits
    fewer records for sweep_fasta(k) than for records of the same lengths that
    are unrelated to the lead (at k >= 8; below, random records share most
    short contexts anyway and nothing is asserted).  Both builds give the
    oracle's graph.  Prints the counts and the table's buckets (-s)."""
    from pangenome_amd._lib import Context
    other = ku.unrelated_fasta(k)
    run = oracle_mod.OracleRun(other, k, 2)
    ctx = Context(k)
    try:
        ctx.set_fasta(sweep(k))
        ctx.parse()
        st = ctx.build(None, 0, True)
        check_graph(ctx, ref_of(oracle_mod, k, 2), "related", st)
        related, cap = st.n_records_a, st.table_capacity
        ctx.set_fasta(other)
        ctx.parse()
        st = ctx.build(None, 0, True)
        keys, masks = ctx.dbg()
        assert np.array_equal(keys, run.dbg()[0]) and np.array_equal(masks, run.dbg()[1])
        assert np.array_equal(ctx.rdbg(), run.rdbg())
        unrelated = st.n_records_a
    finally:
        ctx.close()
    print("k=%2d kb=%2d table_capacity=%d (unrelated %d) n_dbg=%d stage A records: related %d unrelated %d"
          % (k, key_bits(k), cap, st.table_capacity, ref_of(oracle_mod, k, 2).keys.shape[0], related, unrelated))
    if k >= 8:
        assert related < unrelated, (related, unrelated)


# ------------------------------------------------------- 4: dump and reload
@pytest.mark.parametrize("k", ku.KS)
def test_dump_load(oracle_mod, k):
    """pg_dbg_dump against the oracle's oakht (keys, masks, saturating counts,
    capacity); then those slots staged on a fresh context (pg_dbg_load) and a
    build with every record unflagged: the same dBG and rdBG."""
    from pangenome_amd._lib import Context
    fasta = sweep(k)
    ref = ref_of(oracle_mod, k, 2)
    rk, rm, rcnt = ref.run.dbg_counts()
    ctx, fresh = Context(k), Context(k)
    try:
        ctx.set_fasta(fasta)
        R, _ = ctx.parse()
        ctx.build(None, 0, True)
        cap, size, keys, vals, cnts = ctx.dbg_dump()
        assert cap == ref.run.dbg_capacity() and size == rk.shape[0]
        sel = cnts > 0
        o = np.argsort(keys[sel], kind="stable")
        assert np.array_equal(keys[sel][o], rk)
        assert np.array_equal(vals[sel][o], rm)
        assert np.array_equal(cnts[sel][o], rcnt)
        fresh.set_fasta(fasta)
        assert fresh.parse()[0] == R
        fresh.dbg_load(keys[sel], vals[sel], cnts[sel])
        st = fresh.build(np.zeros(R, np.uint8), 0, True)
        check_graph(fresh, ref, "reloaded", st)
    finally:
        ctx.close()
        fresh.close()


# ------------------------------------------------------------ 5: the exchange
def _union(parts):
    """(keys, masks, rdbg) of the owners' exports, sorted; the owners'
    key sets must be disjoint."""
    keys = np.concatenate([p[0] for p in parts])
    masks = np.concatenate([p[1] for p in parts])
    rdbg = np.concatenate([p[2] for p in parts])
    assert np.unique(keys).shape[0] == keys.shape[0] and np.unique(rdbg).shape[0] == rdbg.shape[0]
    o = np.argsort(keys, kind="stable")
    return keys[o], masks[o], np.sort(rdbg)


def _owner(dst):
    dst.build_rdbg()
    return (*dst.dbg(), dst.rdbg())


@pytest.mark.parametrize("k", EXCHANGE_KS)
def test_exchange(oracle_mod, k):
    """Both exchanges in one process, a sender and an owner context: the
    built table partitioned into 1, 3 and 8 runs of 16-byte records and each
    run merged (pg_dbg_partition / pg_dbg_merge); stage A held and routed to
    2 and to 2^min(6, kb) owners - at k = 1 and 2 as many owner bits as key
    bits, the rotation by kb - and each owner's rows merged (pg_route_stage_a /
    pg_route_scatter / pg_route_merge, one owner through pg_route_merge_segs in
    two segments); pg_route_finish for one owner.  The owners' dBGs are
    disjoint, their union is the oracle's dBG and rdBG, and the senders' sums,
    the receivers' checksums and what the merges read agree."""
    import torch
    from pangenome_amd._lib import Context
    from pangenome_amd.dist import row_check_sum
    ref = ref_of(oracle_mod, k, 2)
    want = (ref.keys, ref.masks, ref.rdbg)
    src, dst = Context(k), Context(k)
    try:
        src.set_fasta(sweep(k))
        src.parse()
        built = src.build_dbg(None, 0, True)
        sentinel = bool(built.sentinel)
        assert sentinel                                           # (the tail's records shorter than k)
        for nparts in (1, 3, 8):
            counts = src.partition(nparts).astype(np.int64)
            total = int(counts.sum())
            assert total == built.n_slots                         # the canonical entries; the sentinel goes as a flag
            buf = torch.zeros((total, 2), dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            assert np.array_equal(src.partition(nparts, buf.data_ptr(), total).astype(np.int64), counts)
            sums = src.partition_sums(nparts)
            off = np.concatenate([[0], np.cumsum(counts)])
            assert np.array_equal(src.rows_checksum(buf.data_ptr(), off), sums)
            host = buf.cpu().numpy()
            parts = []
            for p in range(nparts):
                assert row_check_sum(host[off[p]:off[p + 1]]) == int(sums[p])
                dst.merge(buf.data_ptr() + 16 * int(off[p]), int(counts[p]), 0, sentinel and p == 0)
                assert dst.merge_check() == (int(counts[p]), int(sums[p]))
                parts.append(_owner(dst))
            for g, w in zip(_union(parts), want):
                assert np.array_equal(g, w), nparts
        for nparts in (2, 2 ** min(6, key_bits(k))):
            counts, sent = src.route_stage_a(None, 0, True, nparts)
            counts = counts.astype(np.int64)
            total = int(counts.sum())
            assert sent and total > 0
            buf = torch.zeros((total, 3), dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            sums = src.route_scatter(nparts, buf.data_ptr(), total)
            off = np.concatenate([[0], np.cumsum(counts)])
            assert np.array_equal(src.route_rows_checksum(buf.data_ptr(), off), sums)
            host = buf.cpu().numpy()
            parts = []
            for o in range(nparts):
                n, at = int(counts[o]), buf.data_ptr() + 12 * int(off[o])
                assert row_check_sum(host[off[o]:off[o + 1]]) == int(sums[o])
                if nparts == 2 and o == 1:
                    st = dst.route_merge_segs([(at, n // 2), (at + 12 * (n // 2), n - n // 2)], nparts, False)
                else:
                    st = dst.route_merge(at, n, nparts, sent and o == 0)
                assert dst.merge_check() == (n, int(sums[o]))
                parts.append(_owner(dst))
                assert st.n_dbg == parts[-1][0].shape[0] and st.n_rdbg == parts[-1][2].shape[0]
            for g, w in zip(_union(parts), want):
                assert np.array_equal(g, w), nparts
        counts, sent = src.route_stage_a(None, 0, True, 1)
        assert sent and int(counts[0]) == total
        check_graph(src, ref, "route_finish", src.route_finish())
    finally:
        src.close()
        dst.close()


# ------------------------------------------------------------- 6: refusals
@pytest.mark.parametrize("k,nparts", [(1, 16), (2, 64)])
def test_more_owners_than_coarse_bins_are_refused(k, nparts):
    """One owner more than doubles the coarse bins of k (2^kb: 8 at k = 1, 32
    at k = 2): refused with PG_EINVAL by every routed entry point before
    anything runs, on a context that has not built yet and on one that has."""
    from pangenome_amd._lib import Context, PangenomeError
    refused = r" failed \(-22\): %s: more owners than coarse bins"
    ctx = Context(k)
    try:
        for state in ("fresh", "parsed", "built"):
            if state == "parsed":
                ctx.set_fasta(sweep(k))
                ctx.parse()
            if state == "built":
                ctx.build(None, 0, True)
            with pytest.raises(PangenomeError, match=refused % "pg_route_stage_a"):
                ctx.route_stage_a(None, 0, True, nparts)
            with pytest.raises(PangenomeError, match=refused % "pg_route_scatter"):
                ctx.route_scatter(nparts, 0, 0)
            with pytest.raises(PangenomeError, match=refused % "pg_route_merge"):
                ctx.route_merge(0, 0, nparts)
            with pytest.raises(PangenomeError, match=refused % "pg_route_merge_segs"):
                ctx.route_merge_segs([(0, 0)], nparts)
        assert ctx.stats().n_dbg > 0                              # the build is still there
    finally:
        ctx.close()
