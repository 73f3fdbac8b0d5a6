"""The edge walk, the label dictionary, the greedy region merge and the two
device text formatters (pangenome_amd/csrc/pg_walk.hip), driven directly
through the C ABI and compared exactly, integers and bytes, with the CPU
oracle.

The inputs come from tests/walk_util.py (tests/test_walk_util.py checks them
against the oracle alone): one FASTA per k whose record lengths sit on every
boundary of the walks, and label tables made from the oracle's dBG that turn
every window into a hit, so the row merge runs on dense hits, long merges
and arbitrary labels instead of the one-hit rows the pipelines give.  A pass
over rec_flags is compared with the oracle over the FASTA of the flagged
records alone.
"""
import ctypes as C

import numpy as np
import pytest

import walk_util as wu

pytestmark = pytest.mark.gpu

# the edges of k: the smallest and the largest keys; 13 and 14, where 5^k (pow5(k), pow5(k - 1) in the walks)
# passes 2^32 and init_keys gets its high part; 6 and 14, where the coverage pass of the build under the walks
# changes its smear; 11 and 20 in between (tests/test_gpu_ksweep.py has every k)
KS = (1, 2, 6, 11, 13, 14, 20, 27)
PATTERNS = ("alternate", "last", "short", "none", "all")
# every pattern at k = 11 and 27, "alternate" and "all" at the other k
FLAG_CASES = [(k, p) for p in PATTERNS for k in (11, 27)] + \
             [(k, p) for p in ("alternate", "all") for k in KS if k not in (11, 27)]
TABLES = ("const", "three", "distinct", "cross31", "negative", "minus1", "sparse", "absent", "empty")


@pytest.fixture(scope="module")
def ctxs():
    """One context per k, made on first use."""
    from pangenome_amd._lib import Context
    made = {}

    def get(k):
        if k not in made:
            made[k] = Context(k, 0)
        return made[k]
    yield get
    for c in made.values():
        c.close()


class Input:
    """One FASTA with what the oracle says about it (computed once)."""

    def __init__(self, oracle, fasta, k):
        self.oracle, self.fasta, self.k = oracle, fasta, k
        self.arr = np.frombuffer(fasta, np.uint8)
        self.names = wu.names_of(fasta)
        self.n_records = len(self.names)
        self.run = oracle.OracleRun(fasta, k, 3)
        self.true_members = self.run.rdbg()
        self.dbg_keys, self.dbg_masks = self.run.dbg()
        self._dense = None
        self._tables = {}

    def members(self, which):
        return self.true_members if which == "true" else self.dbg_keys

    @property
    def dense(self):
        if self._dense is None:
            self._dense = wu.dense_table(self.dbg_keys, self.dbg_masks)
        return self._dense

    def table(self, name):
        """(keys, vals, ids) of the synthetic label tables."""
        if name not in self._tables:
            k, v = self.dense
            n = k.shape[0]
            if name == "const":
                t = k, v, np.full(n, 7, np.int64)
            elif name == "three":
                t = k, v, wu.hash_ids(k, v, 3)
            elif name == "distinct":
                t = k, v, np.arange(n, dtype=np.int64)
            elif name == "cross31":          # ids on both sides of 2^31: the int32 output wraps the upper ones
                t = k, v, 2 ** 31 - n // 2 + np.arange(n, dtype=np.int64)
            elif name == "negative":
                t = k, v, -2 - 1000003 * wu.hash_ids(k, v, 5, salt=3)
            elif name == "minus1":           # -1 is the merge's label before a walk's first hit (:1529-1531)
                t = k, v, wu.hash_ids(k, v, 3, salt=5) - 1
            elif name == "sparse":
                sel = wu.hash_ids(k, v, 3, salt=9) == 0
                t = k[sel], v[sel], wu.hash_ids(k[sel], v[sel], 4, salt=1)
            elif name == "absent":           # values past the 12 bits a window can give
                t = k, v + 4096, wu.hash_ids(k, v, 3)
            else:
                t = tuple(np.zeros(0, np.int64) for _ in range(3))
            self._tables[name] = tuple(np.ascontiguousarray(a) for a in t)
        return self._tables[name]

    # ---- the oracle's answers
    def rows(self, labels, rc1, flags=None):
        run = self.run
        if flags is not None:
            sub = wu.subset_fasta(self.fasta, flags)
            if not sub:
                return []
            run = self.oracle.OracleRun(sub, self.k, 2)
        run.c = 2 | int(bool(rc1))
        return run.rows(labels)

    def edges(self, which, rc1, flags=None):
        run = self.run
        if flags is not None:
            sub = wu.subset_fasta(self.fasta, flags)
            if not sub:
                return np.zeros((0, 4), np.uint64), np.zeros(0, np.int64)
            run = self.oracle.OracleRun(sub, self.k, 2)
        run.set_rdbg(self.members(which))
        run.c = 2 | int(bool(rc1))
        return run.edges()


_inputs = {}


@pytest.fixture(scope="module", autouse=True)
def _shared_inputs():
    """The inputs and the oracle's runs over them are shared by the tests of
    this module and freed with it."""
    yield
    _inputs.clear()


def standard(oracle, k):
    if ("std", k) not in _inputs:
        _inputs["std", k] = Input(oracle, wu.standard_fasta(k), k)
    return _inputs["std", k]


def parse(ctx, inp):
    ctx.set_fasta(inp.arr)
    assert ctx.parse()[0] == inp.n_records


def stage(ctx, inp, which):
    """Parse the input and make `which` member set the context's rdBG: the true
    one by a build over every record, or every dBG key (the -D form: the keys
    staged with mask 0, no record inserted)."""
    parse(ctx, inp)
    if which == "true":
        ctx.dbg_load(np.zeros(0, np.uint64))
        ctx.build_dbg(None, 0, True)
    else:
        ctx.dbg_load(inp.members(which))
        ctx.build_dbg(np.zeros(inp.n_records, np.uint8), 0, True)
        ctx.dbg_load(np.zeros(0, np.uint64))          # (the stage is merged into every following build)
    ctx.build_rdbg()
    assert np.array_equal(ctx.rdbg(), np.sort(inp.members(which)))


def text_of(lines):
    return "".join(x + "\n" for x in lines).encode()


def check_rows(ctx, inp, labels, rc1, flags=None):
    """set_labels + rows + rows_text against the oracle; returns the lines."""
    want = inp.rows(labels, rc1, flags)
    ctx.set_labels(*labels)
    rows = ctx.rows(flags, rc1)
    assert wu.row_lines(rows, inp.names) == want
    assert ctx.rows_text(inp.names) == text_of(want)
    return want


def check_edges(ctx, inp, which, rc1, flags=None):
    from pangenome_amd import host
    wt, wc = inp.edges(which, rc1, flags)
    t, c, walk = ctx.edges(flags, rc1)
    assert t.shape == wt.shape and np.array_equal(t, wt)
    assert np.array_equal(c, wc)
    assert np.all(np.diff(walk) >= 0)
    assert ctx.edges_text() == host.xyz_text(wt, wc).encode()
    return t, c, walk


# ------------------------------------------------------------------ 1: rows
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("k", KS)
def test_rows_synthetic_labels(ctxs, oracle_mod, k, table):
    inp, ctx = standard(oracle_mod, k), ctxs(k)
    parse(ctx, inp)
    labels = inp.table(table)
    for rc1 in (True, False):
        lines = check_rows(ctx, inp, labels, rc1)
        walks = int((wu.record_table(inp.fasta)[0] > k).sum()) * (2 if rc1 else 1)
        if table == "const":
            assert len(lines) == walks
        elif table in ("three", "distinct", "cross31", "negative", "sparse"):
            assert len(lines) > 4 * walks                   # merges interleaved with breaks
        elif table in ("absent", "empty"):
            assert lines == []
        if table == "cross31":
            labs = [int(x.rsplit("\t", 1)[1]) for x in lines]
            assert min(labs) < -2 ** 30 and max(labs) > 2 ** 30
        if table == "negative":
            assert all(x.rsplit("\t", 1)[1].startswith("-") for x in lines)
        if table == "minus1":
            assert any(x.endswith("\t-1") for x in lines)


def test_rows_minus_one_everywhere(ctxs, oracle_mod):
    """Every hit labelled -1: the label a walk starts with, so no row opens."""
    inp, ctx = standard(oracle_mod, 11), ctxs(11)
    parse(ctx, inp)
    k, v = inp.dense
    assert check_rows(ctx, inp, (k, v, np.full(k.shape[0], -1, np.int64)), True) == []


# -------------------------------------------------------- 2: rows, rec_flags
@pytest.mark.parametrize("k,pattern", FLAG_CASES)
def test_rows_rec_flags(ctxs, oracle_mod, k, pattern):
    inp, ctx = standard(oracle_mod, k), ctxs(k)
    parse(ctx, inp)
    flags = wu.flag_patterns(inp.fasta, k)[pattern]
    for rc1 in (True, False):
        lines = check_rows(ctx, inp, inp.table("three"), rc1, flags)
        assert bool(lines) == (pattern != "none")
    if pattern == "alternate":                              # leading -1 hits of a walk after unwalked records
        check_rows(ctx, inp, inp.table("minus1"), True, flags)


# ------------------------------------------------- 3: edges, dense members
@pytest.mark.parametrize("rc1", (True, False))
@pytest.mark.parametrize("k", KS)
def test_edges_every_key_a_member(ctxs, oracle_mod, k, rc1):
    inp, ctx = standard(oracle_mod, k), ctxs(k)
    stage(ctx, inp, "all")
    t, c, _ = check_edges(ctx, inp, "all", rc1)
    if k == 2:
        assert t.shape[0] > 1024          # past the edge table's floor: the x4 re-run
    assert c.max() > 1


def test_edge_counts_are_walks_not_occurrences(ctxs, oracle_mod):
    """A period-4 repeat: 227 windows, a handful of distinct edges, each
    counted once per walk (ACGT is its own reverse complement: twice with
    the other strand walked)."""
    fasta = wu.fasta_bytes([r for r in wu.standard_records(11) if r[0].startswith("period4")])
    inp, ctx = Input(oracle_mod, fasta, 11), ctxs(11)
    stage(ctx, inp, "all")
    for rc1 in (False, True):
        t, c, _ = check_edges(ctx, inp, "all", rc1)
        assert t.shape[0] <= 8 and c.max() == (2 if rc1 else 1)


# ------------------------------------------------ 4: counts and contention
@pytest.mark.parametrize("which", ("true", "all"))
def test_edges_contended_claims(ctxs, oracle_mod, which):
    """64 copies of one record: every walk of a launch claims the same edge
    slots.  Twice on one context: the same arrays."""
    if "rep" not in _inputs:
        _inputs["rep"] = Input(oracle_mod, wu.repeats_fasta(), 11)
    inp, ctx = _inputs["rep"], ctxs(11)
    stage(ctx, inp, which)
    t, c, w = check_edges(ctx, inp, which, True)
    assert c.max() in (64, 65) and t.shape[0] > 100         # walks holding the edge, of 65 per strand
    t2, c2, w2 = check_edges(ctx, inp, which, True)
    assert np.array_equal(t, t2) and np.array_equal(c, c2) and np.array_equal(w, w2)


# ------------------------------------------------------- 5: edges, rec_flags
@pytest.mark.parametrize("which", ("true", "all"))
@pytest.mark.parametrize("k,pattern", FLAG_CASES)
def test_edges_rec_flags(ctxs, oracle_mod, k, pattern, which):
    inp, ctx = standard(oracle_mod, k), ctxs(k)
    stage(ctx, inp, which)
    flags = wu.flag_patterns(inp.fasta, k)[pattern]
    walked = np.arange(inp.n_records) if flags is None else np.flatnonzero(flags)
    for rc1 in (True, False):
        t, c, walk = check_edges(ctx, inp, which, rc1, flags)
        if pattern in ("alternate", "all", "none"):
            assert bool(t.shape[0]) == (pattern != "none")
        assert set((walk // 2).tolist()) <= set(walked.tolist())
        if not rc1:
            assert np.all(walk % 2 == 0)
        # first_walk = 2 * record + strand: the edges first seen up to record r
        # are the edge list of the input that ends after record r
        for r in sorted({int(walked[i]) for i in (0, walked.size // 2, -1)} if walked.size else ()):
            upto = (np.arange(inp.n_records) <= r).astype(np.uint8)
            if flags is not None:
                upto &= flags
            wt, _ = inp.edges(which, rc1, upto)
            assert np.array_equal(t[walk <= 2 * r + 1], wt)


# ---------------------------------------------------- 6: labels from edges
def _mcl_over(nodes, rng, extra=()):
    """A `.mcl` over a random third of `nodes` (lines of 1 to 4 members)
    and, line by line, the `extra` nodes: ([(key, value, line)], lines)."""
    pick = rng.permutation(len(nodes))[:len(nodes) // 3].tolist()
    members = [nodes[i] for i in pick] + list(extra)
    ent, line, i = [], 0, 0
    while i < len(members):
        m = int(rng.integers(1, 5))
        ent += [(a, b, line) for a, b in members[i:i + m]]
        i += m
        line += 1
    return ent, line


def _nodes_of(t):
    return list(dict.fromkeys((a, b) for row in np.asarray(t, np.uint64).tolist()
                              for a, b in (row[:2], row[2:])))


def check_labels(ctx, tuples, device_tuples, ent, next_label):
    """pg_labels_from_edges (tuples given, or None: the last edge pass, whose
    export is device_tuples) against the restated dictionary."""
    want = wu.label_dict(device_tuples if tuples is None else tuples, ent, next_label)
    mk, mv, mi = wu.mcl_arrays(ent)
    n = ctx.labels_from_edges(tuples, mk, mv, mi, next_label)
    got = ctx.labels()
    assert n == want[0].shape[0]
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    return want


@pytest.mark.parametrize("case", ("no_mcl", "third", "absent", "next_above"))
def test_labels_from_edges_after_an_edge_pass(ctxs, oracle_mod, case):
    inp, ctx = standard(oracle_mod, 11), ctxs(11)
    stage(ctx, inp, "all")
    t, c, _ = check_edges(ctx, inp, "all", True)
    rng = np.random.default_rng(11)
    nodes = _nodes_of(t)
    absent = [(5 ** 11 + 17 * i, 3 + i % 5) for i in range(40)]
    ent, lines = {"no_mcl": ([], 0), "third": _mcl_over(nodes, rng), "absent": _mcl_over(nodes, rng, absent),
                  "next_above": _mcl_over(nodes, rng)}[case]
    next_label = lines + (1000 if case == "next_above" else 0)
    for tuples in (None, t):
        labels = check_labels(ctx, tuples, t, ent, next_label)
        assert labels[0].shape[0] == len(nodes) + (40 if case == "absent" else 0)
        want = inp.rows(labels, True)
        assert want and wu.row_lines(ctx.rows(None, True), inp.names) == want
    # a node value of 2^32 is refused before any device work: the table stays
    bad = np.array([[1, 2, 3, 2 ** 32]], np.uint64)
    mk, mv, mi = wu.mcl_arrays(ent or [(1, 2, 0)])
    from pangenome_amd._lib import ptr
    n = C.c_uint64()
    assert ctx.lib.pg_labels_from_edges(ctx.h, ptr(bad), 1, ptr(mk), ptr(mv), ptr(mi), mk.shape[0], 0,
                                        C.byref(n)) == -22
    for g, w in zip(ctx.labels(), labels):
        assert np.array_equal(g, w)
    assert wu.row_lines(ctx.rows(None, True), inp.names) == want


def test_labels_from_synthetic_edges(ctxs):
    """50,000 edges over 3,000 nodes: three values per key (0, 2^32 - 1 and a
    small one), keys below 2^63, every node repeated many times."""
    ctx = ctxs(27)
    rng = np.random.default_rng(6)
    i = np.arange(3000, dtype=np.uint64)
    key = ((i // np.uint64(3) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(1)
    val = np.where(i % np.uint64(3) == 0, np.uint64(0),
                   np.where(i % np.uint64(3) == 1, np.uint64(2 ** 32 - 1), np.uint64(1) + i % np.uint64(1000)))
    e = rng.integers(0, 3000, (50_000, 2))
    t = np.ascontiguousarray(np.stack([key[e[:, 0]], val[e[:, 0]], key[e[:, 1]], val[e[:, 1]]], axis=1))
    nodes = _nodes_of(t)
    assert len(nodes) == 3000 and int(t[:, 0].max()) < 2 ** 63
    absent = [(2 ** 62 + 5 * j, 2 ** 32 - 1 - j) for j in range(100)]
    ent, lines = _mcl_over(nodes, rng, absent)
    for mcl, nxt in (([], 0), (ent, lines), (ent, lines + 12345)):
        labels = check_labels(ctx, t, t, mcl, nxt)
        assert labels[0].shape[0] == 3000 + (100 if mcl else 0)


def test_labels_from_no_edges(ctxs, oracle_mod):
    """Zero edges with a non-empty `.mcl`, host tuples and device edges: the
    table is the `.mcl`'s, and the rows use it."""
    inp, ctx = standard(oracle_mod, 11), ctxs(11)
    stage(ctx, inp, "true")
    k, v, ids = inp.table("sparse")
    ent = list(zip(k.view(np.uint64).tolist()[:700], v.tolist()[:700], ids.tolist()[:700]))
    none = np.zeros(inp.n_records, np.uint8)
    assert ctx.edges_count(none, True) == 0 and ctx.edges_text() == b""
    for tuples in (None, np.zeros((0, 4), np.uint64)):
        labels = check_labels(ctx, tuples, np.zeros((0, 4), np.uint64), ent, 4)
        assert labels[0].shape[0] == 700
        want = inp.rows(labels, True)
        assert want and wu.row_lines(ctx.rows(None, True), inp.names) == want
    assert ctx.labels_from_edges(np.zeros((0, 4), np.uint64)) == 0
    assert ctx.rows(None, True).shape == (0, 5) and ctx.rows_text(inp.names) == b""


# -------------------------------------------------------------- 7: row text
def test_rows_text_takes_each_call_s_names(ctxs, oracle_mod):
    from pangenome_amd import _lib
    recs = wu.standard_records(11)
    recs = [recs[2], ("", recs[0][1][:400]), recs[7], ("long " + "x" * 4995, recs[0][1][350:900]), recs[16]]
    inp, ctx = Input(oracle_mod, wu.fasta_bytes(recs), 11), ctxs(11)
    assert [len(x) for x in inp.names][1::2] == [0, 5000]
    stage(ctx, inp, "true")
    check_edges(ctx, inp, "true", True)
    xyz = ctx.edges_text()
    labels = (*inp.dense, wu.hash_ids(*inp.dense, 3) * 1000003 - 1000003)
    want = check_rows(ctx, inp, labels, True)
    rows = ctx.rows(None, True)
    assert len(want) > 50 and any(x.startswith("\t") for x in want) and any(x.endswith("\t-1000003") for x in want)
    first = ctx.rows_text(inp.names)
    assert first == _lib.format_rows(rows, inp.names) == text_of(wu.row_lines(rows, inp.names))
    # other names, of other lengths and more of them, after the same pg_rows
    other = [b"second-" + bytes([65 + i]) * (7 * i + 1) for i in range(inp.n_records)]
    other[0], other[3] = b"", b"y" * 3000
    second = ctx.rows_text(other + [b"spare"])
    assert second == text_of(wu.row_lines(rows, other)) == _lib.format_rows(rows, other)
    assert ctx.rows_text(inp.names) == first
    # the edge text shares the offsets buffer: each format in turn, unchanged
    assert ctx.edges_text() == xyz and ctx.rows_text(other) == second and ctx.edges_text() == xyz
    # a size query, another call's size query, then the fill
    na, oa = _lib._names_blob(inp.names)
    nb, ob = _lib._names_blob(other)
    n = C.c_uint64()
    p = _lib.ptr
    assert ctx.lib.pg_rows_format(ctx.h, p(na), p(oa), len(inp.names), None, 0, C.byref(n)) == 0
    assert n.value == len(first)
    assert ctx.lib.pg_rows_format(ctx.h, p(nb), p(ob), len(other), None, 0, C.byref(n)) == 0
    assert n.value == len(second) != len(first)
    buf = np.zeros(len(first), np.uint8)
    assert ctx.lib.pg_rows_format(ctx.h, p(na), p(oa), len(inp.names), p(buf), len(first), C.byref(n)) == 0
    assert n.value == len(first) and buf.tobytes() == first


# ---------------------------------------------------------------- 8: errors
def test_argument_and_state_errors(ctxs, oracle_mod):
    """Refused before any launch: no device fault is involved."""
    from pangenome_amd._lib import Context, _names_blob, ptr
    inp = standard(oracle_mod, 11)
    n = C.c_uint64(99)
    fresh = Context(11, 0)
    try:
        lib, h = fresh.lib, fresh.h
        assert lib.pg_rows(h, None, 1, C.byref(n)) == -22                 # no parse
        parse(fresh, inp)
        assert lib.pg_edges(h, None, 1, C.byref(n)) == -22                # no rdBG (no build yet)
        assert n.value == 99
        assert lib.pg_rows(h, None, 1, C.byref(n)) == 0 and n.value == 0  # no label pass: no rows
        assert fresh.rows(None, True).shape == (0, 5) and fresh.rows_text(inp.names) == b""
    finally:
        fresh.close()
    ctx = ctxs(11)
    stage(ctx, inp, "true")
    t, c, w = check_edges(ctx, inp, "true", True)
    lines = check_rows(ctx, inp, inp.table("three"), True)
    lib, h = ctx.lib, ctx.h
    m, nl, nr = t.shape[0], inp.table("three")[0].shape[0], len(lines)
    assert m > 1 and nr > 1
    assert lib.pg_edges_export(h, ptr(t), ptr(c), ptr(w), m - 1) == -34
    assert lib.pg_edges_export(h, ptr(t), ptr(c), ptr(w), m) == 0
    rows = np.zeros((nr, 5), np.int64)
    assert lib.pg_rows_export(h, ptr(rows), nr - 1) == -34
    assert lib.pg_rows_export(h, ptr(rows), nr) == 0 and wu.row_lines(rows, inp.names) == lines
    lab = [np.zeros(nl, np.int64) for _ in range(3)]
    assert lib.pg_labels_export(h, ptr(lab[0]), ptr(lab[1]), ptr(lab[2]), nl - 1) == -34
    assert lib.pg_labels_export(h, ptr(lab[0]), ptr(lab[1]), ptr(lab[2]), nl) == 0
    assert all(np.array_equal(a, b) for a, b in zip(lab, inp.table("three")))
    xyz, txt = ctx.edges_text(), text_of(lines)
    buf = np.zeros(max(len(xyz), len(txt)), np.uint8)
    assert lib.pg_edges_format(h, ptr(buf), len(xyz) - 1, C.byref(n)) == -34
    assert lib.pg_edges_format(h, ptr(buf), len(xyz), C.byref(n)) == 0 and buf[:n.value].tobytes() == xyz
    nb, off = _names_blob(inp.names)
    assert lib.pg_rows_format(h, ptr(nb), ptr(off), len(inp.names), ptr(buf), len(txt) - 1, C.byref(n)) == -34
    assert lib.pg_rows_format(h, ptr(nb), ptr(off), len(inp.names), ptr(buf), len(txt), C.byref(n)) == 0
    assert buf[:n.value].tobytes() == txt
    assert lib.pg_rows_format(h, ptr(nb), ptr(off), len(inp.names) - 1, None, 0, C.byref(n)) == -22
