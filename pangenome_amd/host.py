"""Host-side logic of the drop-in: which records each pass visits, the label
dictionary, the `.xyz` text and the printed rows.

The device does every per-base step; what stays here is what is plain Python
(or loop control) in the reference too:

* the record loops of the three passes with their `-n` limit, their
  2**33-base checkpoints and what resuming from a checkpoint does
  (seq2rdbg :1251-1266 + seq2dbg_jit_ :1204-1230; seq2graph :1876-1890 +
  rdbg_edge_weight_jit_ :1809-1827; seqs2path_jit_ :1831-1849);
* the `.xyz` writer (:1893-1904), the label dictionary (:1918-1944) and the
  row printer (:1946-1949).
"""
from __future__ import annotations

import ast
import io
import operator
import os

import numpy as np

CHUNK = 2 ** 33          # entry_point :2073
NEVER = 2 ** 63


# ------------------------------------------------------------------ -n parsing
_OPS = {ast.Add: operator.add, ast.Sub: operator.sub, ast.Mult: operator.mul,
        ast.Div: operator.truediv, ast.Pow: operator.pow, ast.FloorDiv: operator.floordiv,
        ast.USub: operator.neg, ast.UAdd: operator.pos}


def eval_number(text: str) -> int:
    """``int(eval(args['-n']))`` (:1997) for the numeric expressions it is given
    ('5e8', '2**63', '10**9'), without evaluating arbitrary code."""
    def ev(node):
        if isinstance(node, ast.Expression):
            return ev(node.body)
        if isinstance(node, ast.Constant) and isinstance(node.value, (int, float)):
            return node.value
        if isinstance(node, ast.BinOp) and type(node.op) in _OPS:
            return _OPS[type(node.op)](ev(node.left), ev(node.right))
        if isinstance(node, ast.UnaryOp) and type(node.op) in _OPS:
            return _OPS[type(node.op)](ev(node.operand))
        raise ValueError("unsupported -n expression: %r" % text)
    return int(ev(ast.parse(text, mode="eval")))


def ns_hit(N: int, Ns: int) -> bool:
    # numba compares int64 N with Ns; Ns >= 2**63 arrives as uint64 and the
    # mixed comparison never succeeds
    return Ns < NEVER and N > Ns


# ----------------------------------------------------------------- pass plans
class FileShape:
    """What the pass planner needs to know about the FASTA beyond the records."""

    def __init__(self, first_byte: int, last_line_has_nl: bool, first_header_at: int,
                 record_header_is_last_unterminated: bool):
        self.first_byte = first_byte
        self.last_line_has_nl = last_line_has_nl
        self.first_header_at = first_header_at            # byte offset of record 0's header
        self.last_header_unterminated = record_header_is_last_unterminated

    @classmethod
    def from_bytes(cls, buf, hdr_start: np.ndarray, hdr_len: np.ndarray):
        n = len(buf)
        first = buf[0] if n else -1
        last_nl = n > 0 and buf[n - 1] == 10
        R = hdr_start.shape[0]
        fh = int(hdr_start[0]) if R else -1
        # the last record's header is the file's final, newline-less line
        lhu = bool(R) and int(hdr_start[-1] + hdr_len[-1]) >= n - 1 and not last_nl
        return cls(first, last_nl, fh, lhu)


def _resumed_records(pos: int, R: int, shape: FileShape):
    """Records one seqio_jit_ call yields when restarted at the `ptr` of record
    pos-1 (:1240, :1860): readline_jit_ starts its first line at byte 0, so
    that line is the file's prefix up to the end of record pos's header line.
    If the file does not start with '>', that prefix is a sequence line, qid
    is never set and record pos is lost; when record pos-1 was the last one the
    prefix runs to EOF and, starting with '>', yields one extra empty record.
    A first line without '\\n' is never yielded (`end > start > 0`)."""
    if pos < R:
        if pos == R - 1 and shape.last_header_unterminated:
            return []                                  # no '\n' after ptr: nothing at all
        lost = shape.first_byte != ord(">")
        return list(range(pos + (1 if lost else 0), R))
    if shape.last_line_has_nl and shape.first_byte == ord(">"):
        return ["extra"]
    return []


def plan_dbg(seq_len: np.ndarray, shape: FileShape, rc0: bool, Ns: int, chunk: int = CHUNK,
             resume: int | None = None, checkpoint: bool = False):
    """seq2rdbg (:1251-1266) over seq2dbg_jit_ (:1204-1230): which records the
    dBG pass inserts, and how many extra empty records it meets.  `resume`
    is the record a -r checkpoint restarts at (resume_position).  With
    `checkpoint`, also the state of the last `<in>_db_brkpt.npz` dump
    (:1255-1259; each dump overwrites the previous one): (flags, extra,
    record) of the records inserted when it was written and the record whose
    seqio ptr is its offset - or None when no pass crossed `chunk`."""
    R = seq_len.shape[0]
    flags = np.zeros(R, np.uint8)
    extra = 0
    ckpt = None
    mult = 2 if rc0 else 1
    recs = list(range(R)) if not resume else _resumed_records(resume, R, shape)
    N = 0
    while True:
        Nl = chk = 0
        done, last = 1, None
        for r in recs:
            n = 0 if r == "extra" else int(seq_len[r])
            if r == "extra":
                extra += 1
            else:
                flags[r] = 1
            Nl += n * mult
            chk += n * mult
            if chk > chunk:
                done, last = -1, r
                break
            if ns_hit(Nl, Ns):
                break
        if done != -1:
            break
        ckpt = (flags.copy(), extra, last)
        recs = _resumed_records(last + 1, R, shape)
        N += Nl
        if ns_hit(N, Ns):
            break
    return (flags, extra, ckpt) if checkpoint else (flags, extra)


def plan_edges(seq_len: np.ndarray, shape: FileShape, Ns: int, chunk: int = CHUNK, resume: int | None = None,
               checkpoint: bool = False):
    """seq2graph (:1876-1890) over rdbg_edge_weight_jit_ (:1809-1827): walked
    records and, per record, the checkpoint segment it belongs to.  `resume`
    is the record a -R checkpoint restarts at (resume_position).  With
    `checkpoint`, also the record whose seqio ptr is the offset of the last
    `<in>_rdb_brkpt.npz` dump (:1880-1887), or None (no checkpoint)."""
    R = seq_len.shape[0]
    flags = np.zeros(R, np.uint8)
    segment = np.full(R, -1, np.int64)
    ckpt = None
    recs = list(range(R)) if not resume else _resumed_records(resume, R, shape)
    N = 0
    seg = 0
    n_checkpoints = 0
    while True:
        chk = 0
        done, last = 1, None
        for r in recs:
            n = 0 if r == "extra" else int(seq_len[r])
            if r != "extra":
                flags[r] = 1
                segment[r] = seg
            N += n
            if ns_hit(N, Ns):
                break
            chk += n
            if chk > chunk:
                done, last = -1, r
                break
        if done != -1:
            break
        n_checkpoints += 1
        ckpt = last
        seg += 1
        recs = _resumed_records(last + 1, R, shape)
    return (flags, segment, n_checkpoints, ckpt) if checkpoint else (flags, segment, n_checkpoints)


def plan_rows(seq_len: np.ndarray, shape: FileShape, buf, Ns: int):
    """seqs2path_jit_ (:1831-1849).  It hands `isfasta` (True) to seqio_jit_'s
    offset slot (:1833), so line scanning starts at byte 1; that differs from
    byte 0 only when the file starts with '\\n' and record 0's header is the
    next line — that record is then lost."""
    R = seq_len.shape[0]
    flags = np.zeros(R, np.uint8)
    first = 0
    if R and len(buf) > 1 and buf[0] == 10 and shape.first_header_at == 1:
        first = 1
    N = 0
    for r in range(first, R):
        flags[r] = 1
        N += int(seq_len[r])
        if ns_hit(N, Ns):
            break
    return flags


def edge_order(walk_first: np.ndarray, segment_of_record: np.ndarray, n_checkpoints: int) -> np.ndarray:
    """Iteration order of the edge Dict: first occurrence, reversed at every
    dump/reload checkpoint (dict2array pops LIFO, :229; array2dict re-inserts,
    :264-286).  Input rows are in first-occurrence order; returns the
    permutation into the reference's order."""
    m = walk_first.shape[0]
    idx = np.arange(m, dtype=np.int64)
    if m == 0 or n_checkpoints == 0:
        return idx
    seg = segment_of_record[walk_first // 2]
    order = np.zeros(0, np.int64)
    for s in range(n_checkpoints + 1):
        order = np.concatenate([order, idx[seg == s]])
        if s < n_checkpoints:
            order = order[::-1]
    return order


# -------------------------------------------------------------------- text
def xyz_text(tuples: np.ndarray, counts: np.ndarray) -> str:
    """`"%d_%d\\t%d_%d\\t%d\\n"` per edge (:1901)."""
    return "".join("%d_%d\t%d_%d\t%d\n" % (a, b, c, d, e)
                   for (a, b, c, d), e in zip(tuples.tolist(), counts.tolist()))


def label_dict(mcl_text: str, xyz_lines) -> dict:
    """seq2graph :1918-1944: `.mcl` line index, then unseen `.xyz` nodes."""
    lab = {}
    flag = 0
    for line in mcl_text.splitlines(keepends=True):
        for tok in line[:-1].split("\t"):
            lab[tuple(map(int, tok.split("_")[:2]))] = flag
        flag += 1
    for line in xyz_lines:
        j, k = line[:-1].split("\t")[:2]
        kj = tuple(map(int, j.split("_")[:2]))
        if kj not in lab:
            lab[kj] = flag
            flag += 1
        kk = tuple(map(int, k.split("_")[:2]))
        if kk not in lab:
            lab[kk] = flag
            flag += 1
    return lab


def mcl_labels(mcl_text: str):
    """The `.mcl` part of seq2graph's label dictionary (:1918-1929): every
    token's line index, a later line winning as dict assignment does.
    Returns (keys, vals, ids) as int64 (keys carry the uint64 key's bits) and
    the number of lines (the next label)."""
    seen = {}
    flag = 0
    for line in mcl_text.splitlines(keepends=True):
        for tok in line[:-1].split("\t"):
            p = tok.split("_")[:2]
            seen[(int(p[0]), int(p[1]))] = flag
        flag += 1
    mk = np.array([k for k, _ in seen.keys()], dtype=np.uint64).view(np.int64)
    mv = np.array([v for _, v in seen.keys()], dtype=np.uint64).view(np.int64)
    mi = np.fromiter(seen.values(), dtype=np.int64, count=len(seen))
    return mk, mv, mi, flag


def _node_ids(t: np.ndarray):
    """The nodes of the edges t [E, 4], E > 0: the distinct (key, value) pairs
    numbered by first appearance (n0_v0, then n1_v1 of each edge, in edge
    order).  Returns the node ids of each edge's ends [E, 2] and the nodes
    [U, 2]."""
    nodes = np.ascontiguousarray(t.reshape(-1, 2))           # slot 2e is (n0, v0), slot 2e + 1 is (n1, v1)
    vv = nodes.view(np.dtype((np.void, 16))).ravel()
    _, first, inv = np.unique(vv, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                 # groups by first appearance
    rank = np.empty(order.shape[0], np.int64)
    rank[order] = np.arange(order.shape[0])
    return rank[inv.ravel()].reshape(-1, 2), nodes[first[order]]


def cluster_cc(tuples: np.ndarray, counts: np.ndarray, min_weight: int = 1):
    """The built-in clusterer's specification (pg_cluster_cc computes the same
    on the device): the `.xyz` edges with count < min_weight dropped, the
    connected components of the rest (reference README step 4).  Nodes are the
    distinct (key, value) pairs, numbered by first appearance (n0_v0, then
    n1_v1 of each edge, in edge order); light edges and self-loops join
    nothing, but their endpoints are nodes.  Clusters by size descending, ties
    by their smallest node id; members by node id.  Returns the `.mcl` text
    (one line per cluster, "<key>_<value>" tokens separated by tabs) and the
    label table (keys, vals, ids) in file order, ids = line indices: what
    mcl_labels(text) gives."""
    if int(min_weight) < 1:
        raise ValueError("cluster_cc: min_weight below 1")
    t = np.ascontiguousarray(tuples, dtype=np.uint64).reshape(-1, 4)
    cnt = np.ascontiguousarray(counts, dtype=np.int64)
    if cnt.shape[0] != t.shape[0]:
        raise ValueError("cluster_cc: %d tuples, %d counts" % (t.shape[0], cnt.shape[0]))
    if t.shape[0] == 0:
        z = np.zeros(0, np.int64)
        return "", z, z.copy(), z.copy()
    ids, uniq = _node_ids(t)
    U = uniq.shape[0]
    parent = list(range(U))
    keep = cnt >= int(min_weight)
    for a, b in ids[keep].tolist():
        while parent[a] != a:                                # find with path halving
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a != b:                                           # the larger root under the smaller
            if a < b:
                a, b = b, a
            parent[a] = b
    members = {}
    for i in range(U):                                       # roots are their component's smallest id
        r = i
        while parent[r] != r:
            r = parent[r]
        parent[i] = r
        members.setdefault(r, []).append(i)
    clusters = sorted(members.items(), key=lambda kv: (-len(kv[1]), kv[0]))
    names = ["%d_%d" % (a, b) for a, b in uniq.tolist()]
    text = "".join("\t".join(names[i] for i in m) + "\n" for _, m in clusters)
    file_order = np.fromiter((i for _, m in clusters for i in m), dtype=np.int64, count=U)
    line = np.repeat(np.arange(len(clusters), dtype=np.int64), [len(m) for _, m in clusters])
    return text, uniq[file_order, 0].view(np.int64), uniq[file_order, 1].view(np.int64), line


MK_ONE = 1 << 31                 # pg_cluster_markov's fixed point: 1.0
MK_CUT = MK_ONE // 10000         # entries below it are pruned (a column's first entry stays)
MK_STOP = MK_ONE // 1000         # the iteration stops at this chaos
MK_SELECT, MK_MAX_ITER = 64, 200 # what the command line runs with


def markov_note(n_iter, chaos):
    """the line -a markov prints before the rows when the iteration cap was reached, else None"""
    if n_iter >= MK_MAX_ITER and chaos > MK_STOP:
        return "# -a markov: not converged after %d iterations (chaos %.6f)" % (MK_MAX_ITER, chaos / MK_ONE)
    return None


def _mk_isqrt(x):
    """floor(sqrt(x)) of a uint64 array, exact: the double root, then fixed down and up."""
    one = np.uint64(1)
    s = np.sqrt(x.astype(np.float64)).astype(np.uint64)
    while True:
        m = s * s > x
        if not m.any():
            break
        s[m] -= one
    while True:
        m = (s + one) * (s + one) <= x
        if not m.any():
            break
        s[m] += one
    return s


def _mk_prune(col, row, f, U, select):
    """prune() of every column at once.  col, row (int64) and f (uint64, positive) list the candidates in
    any order, every column at least one; returns (col, row, value) by (col, row) and the columns' starts."""
    o = np.lexsort((row, col))
    col, row, f = col[o], row[o], f[o]
    start = np.searchsorted(col, np.arange(U))
    n = (f << np.uint64(31)) // np.add.reduceat(f, start)[col]
    o = np.lexsort((row, np.uint64(1 << 32) - n, col))       # n descending, then row ascending
    col, row, n = col[o], row[o], n[o]
    rank = np.arange(col.shape[0]) - start[col]
    keep = (rank == 0) | ((n >= np.uint64(MK_CUT)) & (rank < select))
    col, row, n = col[keep], row[keep], n[keep]
    start = np.searchsorted(col, np.arange(U))
    v = (n << np.uint64(31)) // np.add.reduceat(n, start)[col]
    o = np.lexsort((row, col))
    return col[o], row[o], v[o], start


def _mk_chaos(v, start):
    if not v.shape[0]:
        return 0
    return int((np.maximum.reduceat(v, start) - (np.add.reduceat(v * v, start) >> np.uint64(31))).max())


def _mk_step(col, row, val, start, U, inflation2, select):
    """one iteration: expansion, scaling, inflation, prune"""
    u31 = np.uint64(31)
    length = np.diff(np.append(start, col.shape[0]))
    reps = length[row]                                       # entry (k = row, j = col) meets column k whole
    e_of = np.repeat(np.arange(col.shape[0]), reps)
    src = start[row[e_of]] + (np.arange(e_of.shape[0]) - np.repeat(np.cumsum(reps) - reps, reps))
    cc, cr, prod = col[e_of], row[src], val[src] * val[e_of]
    o = np.lexsort((cr, cc))
    cc, cr, prod = cc[o], cr[o], prod[o]
    head = np.flatnonzero(np.append(True, (cc[1:] != cc[:-1]) | (cr[1:] != cr[:-1])))
    cc, cr, e = cc[head], cr[head], np.add.reduceat(prod, head) >> u31
    cstart = np.searchsorted(cc, np.arange(U))
    x = (e << u31) // np.maximum.reduceat(e, cstart)[cc]
    y = np.full(x.shape[0], MK_ONE, np.uint64)
    for _ in range(inflation2 // 2):
        y = (y * x) >> u31
    if inflation2 & 1:
        y = (y * _mk_isqrt(x << u31)) >> u31
    live = y > 0
    return _mk_prune(cc[live], cr[live], y[live], U, select)


def cluster_markov(tuples, counts, min_weight: int = 1, inflation2: int = 3, select: int = 64, max_iter: int = 200):
    """Markov clustering's specification (pg_cluster_markov computes the same
    on the device, bit for bit): the definition of include/pangenome.h in
    unsigned integers, 1.0 = MK_ONE.  Nodes as cluster_cc; w(i, j) = the summed
    counts >= min_weight of the edges between i != j, a loop of the column's
    largest weight (1 without an edge); columns pruned to `select` entries;
    per iteration the expansion M x M, the scaling to the column's largest,
    the inflation by inflation2 / 2 and the prune, until the chaos is at most
    MK_STOP or max_iter iterations ran.  Clusters: the components of the last
    matrix's stored entries, ordered and written as cluster_cc does.  Returns
    cluster_cc's four values, then n_iter, chaos and the matrix (col_len
    uint32 [U], rows and vals uint32 [U, select], zero beyond a column's
    length).  Also the fallback of a shard backend without a device."""
    min_weight, inflation2, select, max_iter = int(min_weight), int(inflation2), int(select), int(max_iter)
    if min_weight < 1:
        raise ValueError("cluster_markov: min_weight below 1")
    if not 3 <= inflation2 <= 40:
        raise ValueError("cluster_markov: inflation2 outside [3, 40]")
    if not 1 <= select <= 64:
        raise ValueError("cluster_markov: select outside [1, 64]")
    if not 0 <= max_iter <= 10000:
        raise ValueError("cluster_markov: max_iter outside [0, 10000]")
    t = np.ascontiguousarray(tuples, dtype=np.uint64).reshape(-1, 4)
    cnt = np.ascontiguousarray(counts, dtype=np.int64)
    if cnt.shape[0] != t.shape[0]:
        raise ValueError("cluster_markov: %d tuples, %d counts" % (t.shape[0], cnt.shape[0]))
    if t.shape[0] == 0:
        z = np.zeros(0, np.int64)
        return "", z, z.copy(), z.copy(), 0, 0, (np.zeros(0, np.uint32), np.zeros((0, select), np.uint32),
                                                 np.zeros((0, select), np.uint32))
    ids, uniq = _node_ids(t)
    U = uniq.shape[0]
    # ---- the weights: undirected pairs summed, then both directions and the loops
    keep = (cnt >= min_weight) & (ids[:, 0] != ids[:, 1])
    a, b = ids[keep].min(axis=1), ids[keep].max(axis=1)
    o = np.lexsort((b, a))
    a, b, w = a[o], b[o], cnt[keep][o].astype(object)        # (Python integers: the sum has no limit here)
    head = np.flatnonzero(np.append(True, (a[1:] != a[:-1]) | (b[1:] != b[:-1]))) if a.shape[0] else np.zeros(0, np.int64)
    w = np.add.reduceat(w, head) if a.shape[0] else w
    if any(int(x) >= 1 << 32 for x in w):
        raise OverflowError("cluster_markov: a summed weight of 2^32 or more")
    a, b, w = a[head], b[head], w.astype(np.uint64)
    loop = np.ones(U, np.uint64)
    big = np.zeros(U, np.uint64)
    np.maximum.at(big, a, w)
    np.maximum.at(big, b, w)
    loop = np.maximum(loop, big)
    col = np.concatenate([a, b, np.arange(U)]).astype(np.int64)
    row = np.concatenate([b, a, np.arange(U)]).astype(np.int64)
    col, row, val, start = _mk_prune(col, row, np.concatenate([w, w, loop]), U, select)
    chaos, n_iter = _mk_chaos(val, start), 0
    while n_iter < max_iter:
        col, row, val, start = _mk_step(col, row, val, start, U, inflation2, select)
        chaos, n_iter = _mk_chaos(val, start), n_iter + 1
        if chaos <= MK_STOP:
            break
    col_len = np.diff(np.append(start, col.shape[0])).astype(np.uint32)
    rows = np.zeros((U, select), np.uint32)
    vals = np.zeros((U, select), np.uint32)
    at = np.arange(col.shape[0]) - start[col]
    rows[col, at] = row
    vals[col, at] = val
    # ---- the clusters: components of the stored entries, cluster_cc's order and text
    edges = np.zeros((col.shape[0], 4), np.uint64)
    edges[:, 0:2] = uniq[col]
    edges[:, 2:4] = uniq[row]
    # (cluster_cc numbers nodes by first appearance: lead with every node in id order, as loops)
    lead = np.concatenate([uniq, uniq], axis=1)
    text, k, v, line = cluster_cc(np.concatenate([lead, edges]), np.ones(U + col.shape[0], np.int64), 1)
    return text, k, v, line, n_iter, chaos, (col_len, rows, vals)


SWEEP_MAX_LEVELS = 4096          # pg_cluster_sweep's limit


def cluster_sweep(tuples: np.ndarray, counts: np.ndarray, thresholds):
    """The cluster curve's specification (pg_cluster_sweep computes the same
    on the device): for every threshold T of the strictly ascending list,
    the edges with count >= T (self-loops included) and the number of
    clusters cluster_cc(min_weight=T) forms, the size of the largest (0
    without nodes) and how many have one node.  One union-find goes from the
    highest threshold down: the components at T are those at the next higher
    threshold plus the unions of the edges between the two.  Returns a dict
    of arrays: w (int64), edges, clusters, largest, singletons (uint64)."""
    thr = np.ascontiguousarray(thresholds, dtype=np.int64).reshape(-1)
    if thr.shape[0] > SWEEP_MAX_LEVELS:
        raise ValueError("cluster_sweep: more than %d thresholds" % SWEEP_MAX_LEVELS)
    if thr.shape[0] and (thr[0] < 1 or np.any(np.diff(thr) <= 0)):
        raise ValueError("cluster_sweep: thresholds must be at least 1 and strictly ascending")
    t = np.ascontiguousarray(tuples, dtype=np.uint64).reshape(-1, 4)
    cnt = np.ascontiguousarray(counts, dtype=np.int64)
    if cnt.shape[0] != t.shape[0]:
        raise ValueError("cluster_sweep: %d tuples, %d counts" % (t.shape[0], cnt.shape[0]))
    n = thr.shape[0]
    out = {"w": thr, "edges": np.zeros(n, np.uint64), "clusters": np.zeros(n, np.uint64),
           "largest": np.zeros(n, np.uint64), "singletons": np.zeros(n, np.uint64)}
    if t.shape[0] == 0 or n == 0:
        return out
    ids, uniq = _node_ids(t)
    U = uniq.shape[0]
    level = np.searchsorted(thr, cnt, side="right") - 1      # the last threshold <= count (-1: below them all)
    parent, size = list(range(U)), [1] * U
    clusters, largest, singles, kept = U, 1, U, 0
    for i in range(n - 1, -1, -1):
        sel = level == i
        kept += int(sel.sum())
        for a, b in ids[sel].tolist():
            while parent[a] != a:                            # find with path halving
                parent[a] = parent[parent[a]]
                a = parent[a]
            while parent[b] != b:
                parent[b] = parent[parent[b]]
                b = parent[b]
            if a != b:                                       # the larger root under the smaller
                if a < b:
                    a, b = b, a
                parent[a] = b
                singles -= (size[a] == 1) + (size[b] == 1)
                size[b] += size[a]
                largest = max(largest, size[b])
                clusters -= 1
        out["edges"][i], out["clusters"][i], out["largest"][i], out["singletons"][i] = kept, clusters, largest, singles
    return out


def sweep_thresholds(max_weight: int):
    """-w auto's thresholds for edges whose largest count is max_weight: every
    integer 1 .. min(max_weight + 1, 64); past 64 the powers of two 128, 256,
    ... up to max_weight, then max_weight + 1.  The last is always above every
    count: the row of single nodes."""
    top = int(max_weight) + 1
    thr = list(range(1, min(top, 64) + 1))
    if top > 64:
        p = 128
        while p <= int(max_weight):
            thr.append(p)
            p *= 2
        thr.append(top)
    return thr


def sweep_choice(table) -> int:
    """-w auto's rule: the threshold whose row has the most clusters of two
    or more nodes (clusters - singletons); among equals the smallest; 1
    without rows or when no row has any."""
    w = np.asarray(table["w"], np.int64)
    multi = np.asarray(table["clusters"], np.int64) - np.asarray(table["singletons"], np.int64)
    if w.shape[0] == 0 or multi.max() <= 0:
        return 1
    return int(w[int(np.argmax(multi))])                     # (argmax: the first of equals; w ascends)


def sweep_text(table, chosen: int) -> str:
    """`<in>_rdbg_weight.xyz.sweep.tsv`: a header, one line of unsigned
    decimals per threshold (multi = clusters - singletons), `#auto`."""
    cols = [np.asarray(table[k]).tolist() for k in ("w", "edges", "clusters", "largest", "singletons")]
    return ("#w\tedges\tclusters\tlargest\tsingletons\tmulti\n"
            + "".join("%d\t%d\t%d\t%d\t%d\t%d\n" % (w, e, c, l, s, c - s) for w, e, c, l, s in zip(*cols))
            + "#auto\t%d\n" % chosen)


def write_sweep_file(qry: str, table, chosen: int):
    """sweep_text as `<qry>_rdbg_weight.xyz.sweep.tsv` (renamed when whole)."""
    name = qry + "_rdbg_weight.xyz.sweep.tsv"
    with open(name + ".tmp", "w") as f:
        f.write(sweep_text(table, chosen))
    os.replace(name + ".tmp", name)


def label_table(mcl_text: str, tuples: np.ndarray):
    """label_dict + label_arrays without the text round trip: the `.mcl` line
    index of every token (a later line wins, as dict assignment does), then
    every `.xyz` node (n0_v0 then n1_v1 of each edge, in edge order) not seen
    yet, numbered in first-appearance order.  Returns (keys, vals, ids) as
    int64 (keys carry the uint64 key's bits)."""
    seen = {}
    flag = 0
    for line in mcl_text.splitlines(keepends=True):
        for tok in line[:-1].split("\t"):
            p = tok.split("_")[:2]
            seen[(int(p[0]), int(p[1]))] = flag
        flag += 1
    t = np.ascontiguousarray(tuples, dtype=np.uint64).reshape(-1, 4)
    nodes = np.empty((2 * t.shape[0], 2), np.uint64)
    nodes[0::2] = t[:, 0:2]
    nodes[1::2] = t[:, 2:4]
    if nodes.shape[0]:
        vv = np.ascontiguousarray(nodes).view(np.dtype((np.void, 16))).ravel()
        _, first = np.unique(vv, return_index=True)
        uniq = nodes[np.sort(first)]
    else:
        uniq = nodes
    if seen:
        keep = np.fromiter(((int(a), int(b)) not in seen for a, b in uniq.tolist()), dtype=bool, count=uniq.shape[0])
        uniq = uniq[keep]
    mk = np.array([k for k, _ in seen.keys()], dtype=np.uint64)
    mv = np.array([v for _, v in seen.keys()], dtype=np.uint64)
    mi = np.fromiter(seen.values(), dtype=np.int64, count=len(seen))
    keys = np.concatenate([mk, uniq[:, 0]]).view(np.int64)
    vals = np.concatenate([mv, uniq[:, 1]]).view(np.int64)
    ids = np.concatenate([mi, flag + np.arange(uniq.shape[0], dtype=np.int64)])
    return keys, vals, ids


def label_arrays(lab: dict):
    n = len(lab)
    keys = np.fromiter((a for a, _ in lab.keys()), dtype=np.int64, count=n)
    vals = np.fromiter((b for _, b in lab.keys()), dtype=np.int64, count=n)
    ids = np.fromiter(lab.values(), dtype=np.int64, count=n)
    return keys, vals, ids


def format_rows(rows: np.ndarray, buf, hdr_start: np.ndarray, hdr_len: np.ndarray):
    """`print('%s\\t%d\\t%d\\t%s\\t%d')` (:1947-1949); qid = header line minus '>'."""
    names = {}
    out = []
    for r, s, e, strand, lab in rows.tolist():
        q = names.get(r)
        if q is None:
            hs, hl = int(hdr_start[r]), int(hdr_len[r])
            q = names[r] = bytes(buf[hs:hs + hl]).decode()[1:]
        out.append("%s\t%d\t%d\t%s\t%d" % (q, s, e, "+" if strand == 1 else "-", lab))
    return out


# ------------------------------------------------------------ npz side files
DB_LOAD = 750000000            # int(0.75 * 1e9): oakht's load factor as dump() stores it (:252)
NPZ_PIECE = 32 << 20           # bytes per CRC / write task of savez_stored


def _crc32_combine():
    """zlib's crc32_combine (libz, not exposed by Python's zlib module)."""
    import ctypes
    f = getattr(_crc32_combine, "f", None)
    if f is None:
        z = ctypes.CDLL("libz.so.1")
        f = z.crc32_combine
        f.restype = ctypes.c_ulong
        f.argtypes = [ctypes.c_ulong, ctypes.c_ulong, ctypes.c_long]
        _crc32_combine.f = f
    return f


class Deferred:
    """A savez_stored member whose data a native writer puts into the file:
    `n` elements of `dtype` (a 1-D array)."""

    def __init__(self, dtype, n: int):
        self.dtype = np.dtype(dtype)
        self.n = int(n)


def savez_stored(fn: str, fill=None, **arrays) -> None:
    """np.savez(fn, **arrays) (a zip of stored .npy members, what np.load and
    the reference's load_on_disk read, :289-335), written in parallel: every
    member's bytes go to the file in NPZ_PIECE pieces by a thread pool
    (os.pwrite at their final offsets) while the same threads CRC them
    (zlib.crc32, GIL released; pieces joined with crc32_combine); then the
    local headers, the central directory and the ZIP64 end records.  The
    single-threaded zipfile CRC and write of np.savez took 0.67 s for C3's
    dump (0.45 s of it CRC).  A `Deferred` member's data is written by
    `fill(fd, offsets)` (its data offsets in member order), which returns
    their CRC-32s."""
    import struct
    import zlib
    from concurrent.futures import ThreadPoolExecutor
    fn = fn if fn.endswith(".npz") else fn + ".npz"
    comb = _crc32_combine()
    members = []
    off = 0
    for name, arr in arrays.items():
        if isinstance(arr, Deferred):
            hd = {"descr": np.lib.format.dtype_to_descr(arr.dtype), "fortran_order": False, "shape": (arr.n,)}
            body, blen = None, arr.n * arr.dtype.itemsize
        else:
            a = np.ascontiguousarray(arr)
            hd = np.lib.format.header_data_from_array_1_0(a)
            body = a.reshape(-1).view(np.uint8) if a.size else np.zeros(0, np.uint8)
            blen = body.shape[0]
        hb = io.BytesIO()
        np.lib.format.write_array_header_1_0(hb, hd)
        head = hb.getvalue()
        zname = (name + ".npy").encode()
        lh = 30 + len(zname) + 20                       # local header + ZIP64 extra (sizes)
        members.append([zname, head, body, off, lh, blen])
        off += lh + len(head) + blen
    fd = os.open(fn, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        tasks = []
        for mi, (zname, head, body, moff, lh, blen) in enumerate(members):
            d0 = moff + lh + len(head)
            if body is not None:
                for p in range(0, blen, NPZ_PIECE):
                    tasks.append((mi, p, body[p:p + NPZ_PIECE], d0 + p))

        def work(t):
            mi, p, piece, at = t
            mv = memoryview(piece)
            done = 0
            while done < len(mv):
                done += os.pwrite(fd, mv[done:], at + done)
            return mi, p, zlib.crc32(mv), len(mv)
        crcs = {}
        if tasks:
            with ThreadPoolExecutor(max_workers=min(16, len(tasks), os.cpu_count() or 4)) as ex:
                for mi, p, c, n in ex.map(work, tasks):
                    crcs[(mi, p)] = (c, n)
        deferred = [mi for mi, m in enumerate(members) if m[2] is None]
        if deferred:
            got = fill(fd, [members[mi][3] + members[mi][4] + len(members[mi][1]) for mi in deferred])
            for mi, c in zip(deferred, got):
                crcs[(mi, 0)] = (int(c), members[mi][5])
        cdir = bytearray()
        dt = (0 << 11) | (0 << 5), (1 << 5) | 1        # 00:00:00, 1980-01-01
        for mi, (zname, head, body, moff, lh, blen) in enumerate(members):
            crc = zlib.crc32(head)
            for p in (range(0, blen, NPZ_PIECE) if body is not None else [0] if blen else []):
                c, n = crcs[(mi, p)]
                crc = comb(crc, c, n)
            size = len(head) + blen
            local = struct.pack("<IHHHHHIIIHH", 0x04034B50, 45, 0, 0, dt[0], dt[1], crc, 0xFFFFFFFF, 0xFFFFFFFF,
                                len(zname), 20) + zname + struct.pack("<HHQQ", 1, 16, size, size) + head
            done = 0
            while done < len(local):
                done += os.pwrite(fd, local[done:], moff + done)
            cdir += struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 45, 45, 0, 0, dt[0], dt[1], crc, 0xFFFFFFFF,
                                0xFFFFFFFF, len(zname), 28, 0, 0, 0, 0, 0xFFFFFFFF) + zname + \
                struct.pack("<HHQQQ", 1, 24, size, size, moff)
        n = len(members)
        tail = bytes(cdir) + struct.pack("<IQHHIIQQQQ", 0x06064B50, 44, 45, 45, 0, 0, n, n, len(cdir), off) + \
            struct.pack("<IIQI", 0x07064B50, 0, off + len(cdir), 1) + \
            struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, min(n, 0xFFFF), min(n, 0xFFFF), 0xFFFFFFFF, 0xFFFFFFFF, 0)
        done = 0
        while done < len(tail):
            done += os.pwrite(fd, tail[done:], off + done)
    finally:
        os.close(fd)


def write_db_npz(fn: str, capacity: int, size: int, keys, values, counts, offset: int = 0):
    """dump() for an oakht (:243-261): parameters [capacity, load * 1e9, size,
    ksize, vsize, offset] and the keys / values / counts slot arrays."""
    fn = fn[:-4] if fn.endswith(".npz") else fn
    params = np.asarray([capacity, DB_LOAD, size, 1, 1, offset], dtype=np.uint64)
    # members stored (np.savez's format) rather than the reference's
    # savez_compressed: the same zip of .npy members, read identically by
    # np.load / the reference's load_on_disk, ~1.4x the bytes, but deflate ran
    # at ~30 MB/s on the slot arrays (C3: 26 s of a 42 s CLI run)
    savez_stored(fn, parameters=params, keys=keys, values=values, counts=counts)


def write_db_npz_from(fn: str, capacity: int, size: int, fill, offset: int = 0):
    """write_db_npz with the slot arrays written by `fill(fd, offsets)` (the
    device's pg_dbg_dump_fd): the same file, no host copy of the arrays."""
    fn = fn[:-4] if fn.endswith(".npz") else fn
    params = np.asarray([capacity, DB_LOAD, size, 1, 1, offset], dtype=np.uint64)
    savez_stored(fn, fill, parameters=params, keys=Deferred(np.uint64, capacity),
                 values=Deferred(np.uint16, capacity), counts=Deferred(np.uint8, capacity))


def read_db_npz(fn: str):
    """load_on_disk (:289-335) of an oakht dump: (offset, keys, values, counts)
    of the occupied (counts > 0) slots, the entries iteritems yields (:623-631).
    The file is read with numpy's non-pickling loader."""
    with np.load(fn, allow_pickle=False) as z:
        params = np.asarray(z["parameters"])
        if params.shape[0] != 6:
            raise ValueError("%s: not an oakht dump (parameters %r)" % (fn, params.tolist()))
        if int(params[3]) != 1 or int(params[4]) != 1:
            raise ValueError("%s: ksize/vsize %d/%d, the dBG uses 1/1" % (fn, int(params[3]), int(params[4])))
        counts = np.asarray(z["counts"])
        sel = counts > 0
        keys = np.asarray(z["keys"])[sel].astype(np.uint64)
        values = np.asarray(z["values"])[sel].astype(np.uint16)
        return int(params[5]), keys, values, np.minimum(counts[sel], 255).astype(np.uint8)


def resume_position(offset: int, rec_ptr: np.ndarray) -> int:
    """The record a checkpoint's `offset` (seqio's ptr when record r was
    yielded, :1255-1259) restarts at: r + 1.  Offset 0 is a fresh start."""
    if offset == 0:
        return 0
    hit = np.flatnonzero(rec_ptr == offset)
    if hit.shape[0] == 0:
        raise ValueError("checkpoint offset %d is not a record boundary of this input" % offset)
    return int(hit[0]) + 1


def write_edge_npz(fn: str, tuples, counts, offset: int):
    """dump(jit=True, ksize=4, vsize=1) of the edge Dict (:243-250): parameters
    [4, 1, offset], then dict2array's popitem order (:221-235) - the Dict's
    iteration order reversed.  `tuples` / `counts` are in iteration order."""
    fn = fn[:-4] if fn.endswith(".npz") else fn
    t = np.ascontiguousarray(np.asarray(tuples, dtype=np.uint64)[::-1]).reshape(-1)
    c = np.ascontiguousarray(np.asarray(counts)[::-1]).astype(np.uint64)
    savez_stored(fn, parameters=np.asarray([4, 1, offset], dtype=np.uint64), keys=t, values=c)


def read_edge_npz(fn: str):
    """load_on_disk(jit=True) (:305-309) of an edge checkpoint: (offset,
    tuples[N, 4] uint64, counts[N]) in file order — array2dict's insertion
    order (:264-286)."""
    with np.load(fn, allow_pickle=False) as z:
        params = np.asarray(z["parameters"])
        if params.shape[0] != 3 or int(params[0]) != 4 or int(params[1]) != 1:
            raise ValueError("%s: not an edge checkpoint (parameters %r)" % (fn, params.tolist()))
        keys = np.asarray(z["keys"]).astype(np.uint64)
        values = np.asarray(z["values"])
        n = min(keys.shape[0] // 4, values.shape[0])
        return int(params[2]), keys[:4 * n].reshape(n, 4), values[:n].astype(np.int64)


def merge_edges(loaded_t, loaded_c, tuples, counts, walk_first, segment_of_record, n_checkpoints):
    """The edge Dict of a resumed seq2graph (:1859-1887): the loaded items in
    file order, then the walks' edges by first occurrence — a known edge adds
    its walk count in place, a new one is appended — and the whole Dict
    reversed at every further checkpoint dump/reload."""
    d = {}
    for t, c in zip(map(tuple, loaded_t.tolist()), loaded_c.tolist()):
        d[t] = c
    seg = segment_of_record[walk_first // 2] if walk_first.shape[0] else np.zeros(0, np.int64)
    tl, cl = tuples.tolist(), counts.tolist()
    for s in range(n_checkpoints + 1):
        for i in np.flatnonzero(seg == s).tolist():
            t = tuple(tl[i])
            d[t] = d.get(t, 0) + cl[i]
        if s < n_checkpoints:
            d = dict(reversed(list(d.items())))
    out_t = np.array(list(d.keys()), dtype=np.uint64).reshape(-1, 4)
    out_c = np.array(list(d.values()), dtype=np.int64)
    return out_t, out_c


# ------------------------------------------------------------ frequency table
FREQ_HEADER = "#label\tgenomes\trows\tplus\tbp\tmin\tmax\n"
_U64 = np.uint64


def _popcount_rows(bits: np.ndarray) -> np.ndarray:
    """Set bits of each row of a uint64 [n, W] array."""
    if bits.shape[0] == 0 or bits.shape[1] == 0:
        return np.zeros(bits.shape[0], np.uint32)
    b = np.unpackbits(np.ascontiguousarray(bits).view(np.uint8).reshape(bits.shape[0], -1), axis=1)
    return b.sum(axis=1).astype(np.uint32)


def _freq_derive(t: dict) -> dict:
    """n_genomes, the spectrum and the per-genome sums of a table from its
    per-label columns and its (label, genome, rows, bases) pairs."""
    G = int(t["n_groups"])
    ng = _popcount_rows(t["bits"])
    t["n_genomes"] = ng
    sl, sb = np.zeros(G + 1, _U64), np.zeros(G + 1, _U64)
    np.add.at(sl, ng, _U64(1))
    np.add.at(sb, ng, t["bp"])
    t["spectrum_labels"], t["spectrum_bp"] = sl, sb
    p = t["pairs"]
    g = p[:, 1].astype(np.int64)
    png = ng[np.searchsorted(t["labels"], p[:, 0].astype(np.int64))] if p.shape[0] else np.zeros(0, np.uint32)
    core = png == G
    uniq = (png == 1) & ~core
    for name, sel, col in (("g_rows", slice(None), 2), ("g_bp", slice(None), 3), ("g_core", core, 3),
                           ("g_unique", uniq, 3)):
        a = np.zeros(G, _U64)
        np.add.at(a, g[sel], p[sel, col])
        t[name] = a
    t["g_shell"] = t["g_bp"] - t["g_core"] - t["g_unique"]
    return t


def freq_table(rows5, rec_group, n_groups: int) -> dict:
    """The frequency table's specification (pg_freq computes the same on the
    device): rows (record, start, end, strand, label) grouped by rec_group
    (record -> genome in [0, n_groups), or -1).  A row is used iff its label
    is >= 0 and its record has a genome.  Per label with a used row, labels
    ascending: rows, plus (strand +1), bp = sum |end - start|, min_len,
    max_len, the presence bits (uint64 [n, ceil(n_groups / 64)], genome g =
    bit g % 64 of word g / 64) and n_genomes; spectrum_labels / spectrum_bp
    [n_groups + 1] by n_genomes; g_rows, g_bp, g_core, g_shell, g_unique per
    genome (unique only when n_groups > 1); n_used, n_skipped.  `pairs` holds
    (label, genome, rows, bp) per label and genome, which freq_merge needs to
    class a genome's bases by labels other ranks saw too."""
    r = np.ascontiguousarray(rows5, dtype=np.int64).reshape(-1, 5)
    grp = np.ascontiguousarray(rec_group, dtype=np.int32).reshape(-1)
    G = int(n_groups)
    if G < 0 or (G == 0 and r.shape[0]):
        raise ValueError("freq_table: n_groups is %d with %d rows" % (G, r.shape[0]))
    if grp.shape[0] and (grp.min() < -1 or grp.max() >= G):
        raise ValueError("freq_table: a rec_group entry is outside [-1, %d)" % G)
    if r.shape[0] and (r[:, 0].min() < 0 or r[:, 0].max() >= grp.shape[0]):
        raise ValueError("freq_table: a row's record is outside [0, %d)" % grp.shape[0])
    W = (G + 63) // 64
    g = grp[r[:, 0]].astype(np.int64) if r.shape[0] else np.zeros(0, np.int64)
    used = (r[:, 4] >= 0) & (g >= 0)
    u, g = r[used], g[used]
    s, e = u[:, 1].view(_U64), u[:, 2].view(_U64)
    length = np.where(u[:, 2] >= u[:, 1], e - s, s - e)
    labels, inv = np.unique(u[:, 4], return_inverse=True)
    inv = inv.reshape(-1)
    n = labels.shape[0]
    t = {"n_groups": G, "n_used": int(used.sum()), "n_skipped": int(r.shape[0] - used.sum()),
         "labels": labels.astype(np.int64),
         "rows": np.bincount(inv, minlength=n).astype(_U64),
         "plus": np.bincount(inv[u[:, 3] == 1], minlength=n).astype(_U64),
         "bp": np.zeros(n, _U64), "min_len": np.full(n, ~_U64(0)), "max_len": np.zeros(n, _U64),
         "bits": np.zeros((n, W), _U64)}
    np.add.at(t["bp"], inv, length)
    np.minimum.at(t["min_len"], inv, length)
    np.maximum.at(t["max_len"], inv, length)
    np.bitwise_or.at(t["bits"], (inv, g >> 6), _U64(1) << (g & 63).astype(_U64))
    pk, pinv = np.unique(inv * max(G, 1) + g, return_inverse=True)
    pinv = pinv.reshape(-1)
    pairs = np.zeros((pk.shape[0], 4), _U64)
    pairs[:, 0] = labels[pk // max(G, 1)].astype(_U64)
    pairs[:, 1] = (pk % max(G, 1)).astype(_U64)
    pairs[:, 2] = np.bincount(pinv, minlength=pk.shape[0]).astype(_U64)
    np.add.at(pairs[:, 3], pinv, length)
    t["pairs"] = pairs
    return _freq_derive(t)


def freq_pairs(rows5, rec_group, n_groups: int) -> np.ndarray:
    """The (label, genome, rows, bp) pairs of freq_table alone (a shard whose
    device made the per-label columns adds them for freq_merge)."""
    return freq_table(rows5, rec_group, n_groups)["pairs"]


def freq_text(table: dict) -> str:
    """The text pg_freq_format writes: the header, then one line per entry."""
    cols = [table[k].tolist() for k in ("labels", "n_genomes", "rows", "plus", "bp", "min_len", "max_len")]
    return FREQ_HEADER + "".join("%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % x for x in zip(*cols))


def freq_merge(parts: list, n_groups: int) -> dict:
    """Per-rank tables (freq_table's dicts, over one global genome numbering)
    merged: rows / plus / bp add, min_len takes the minimum, max_len the
    maximum, the presence bits are ORed (a genome's records may lie on two
    ranks), the pairs add; n_genomes, the spectrum and the per-genome sums are
    derived again from the merged table."""
    G = int(n_groups)
    W = (G + 63) // 64
    lab = np.concatenate([p["labels"] for p in parts]) if parts else np.zeros(0, np.int64)
    labels, inv = np.unique(lab, return_inverse=True)
    inv = inv.reshape(-1)
    n = labels.shape[0]
    cat = lambda k: np.concatenate([p[k] for p in parts]) if parts else np.zeros(0, _U64)
    t = {"n_groups": G, "n_used": sum(int(p["n_used"]) for p in parts),
         "n_skipped": sum(int(p["n_skipped"]) for p in parts), "labels": labels.astype(np.int64),
         "rows": np.zeros(n, _U64), "plus": np.zeros(n, _U64), "bp": np.zeros(n, _U64),
         "min_len": np.full(n, ~_U64(0)), "max_len": np.zeros(n, _U64), "bits": np.zeros((n, W), _U64)}
    for k in ("rows", "plus", "bp"):
        np.add.at(t[k], inv, cat(k))
    np.minimum.at(t["min_len"], inv, cat("min_len"))
    np.maximum.at(t["max_len"], inv, cat("max_len"))
    if parts and W:
        np.bitwise_or.at(t["bits"], inv, np.concatenate([p["bits"].reshape(-1, W) for p in parts]))
    pp = np.concatenate([p["pairs"].reshape(-1, 4) for p in parts]) if parts else np.zeros((0, 4), _U64)
    pk, pinv = np.unique(pp[:, 0] * _U64(max(G, 1)) + pp[:, 1], return_inverse=True)
    pinv = pinv.reshape(-1)
    pairs = np.zeros((pk.shape[0], 4), _U64)
    pairs[:, 0], pairs[:, 1] = pk // _U64(max(G, 1)), pk % _U64(max(G, 1))
    np.add.at(pairs[:, 2], pinv, pp[:, 2])
    np.add.at(pairs[:, 3], pinv, pp[:, 3])
    t["pairs"] = pairs
    return _freq_derive(t)


# ---------------------------------------------------------- genome comparison
def compare_orders(G: int, P: int) -> np.ndarray:
    """The genome orders of `-p P`, int32 [P, G]: order 0 is the identity,
    order p >= 1 a Fisher-Yates shuffle of arange(G) drawn from
    synth.splitmix64(DEFAULT_SEED, p, G - 1): for t, i in enumerate(G-1 .. 1),
    j = r[t] % (i + 1) and a[i], a[j] are swapped."""
    from . import synth
    G, P = int(G), int(P)
    out = np.tile(np.arange(G, dtype=np.int32), (P, 1)).reshape(P, G)
    for p in range(1, P):
        r = synth.splitmix64(synth.DEFAULT_SEED, p, max(G - 1, 0)).tolist()
        a = out[p]
        for t, i in enumerate(range(G - 1, 0, -1)):
            j = r[t] % (i + 1)
            a[i], a[j] = a[j], a[i]
    return out


def _popcount_sum(a: np.ndarray) -> np.ndarray:
    """Set bits of each row of a uint64 [m, w] array, as uint64 [m]."""
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(a).sum(axis=1, dtype=_U64)
    return _popcount_rows(a).astype(_U64)


def freq_compare(bits, n_groups: int, orders):
    """The genome comparison's specification (pg_freq_compare computes the
    same on the device).  bits: uint64 [n, W] presence words (genome g = bit
    g % 64 of word g / 64); orders: int32 [P, G], every row a permutation.
    Returns (shared, pan, core): shared[g][h] = the labels in both g and h,
    uint64 [G, G]; pan[p][i] / core[p][i] = the labels in at least one / in
    every one of the first i + 1 genomes of order p, uint64 [P, G].
    As the device does: the bits are transposed to genome-major rows (64 Ki
    labels at a time, whose 0 / 1 matrix also gives that slice's share of
    `shared` as an exact float32 product), and the curves are the popcounts of
    the running OR / AND of the rows taken in the order, all orders at once."""
    G = int(n_groups)
    W = (G + 63) // 64
    b = np.ascontiguousarray(bits, dtype=_U64)
    n = b.shape[0]
    b = b.reshape(n, W)
    o = np.ascontiguousarray(orders, dtype=np.int32) if orders is not None else np.zeros((0, G), np.int32)
    o = o.reshape(-1, G) if G else o.reshape(o.shape[0], 0)
    P = o.shape[0]
    if G == 0 and n:
        raise ValueError("freq_compare: n_groups is 0 with %d labels" % n)
    if P and G and not np.array_equal(np.sort(o, axis=1), np.tile(np.arange(G, dtype=np.int32), (P, 1))):
        raise ValueError("freq_compare: an order is not a permutation of 0..%d" % (G - 1))
    if G & 63 and n and (b[:, W - 1] >> _U64(G & 63)).any():
        raise ValueError("freq_compare: a row has a bit at or above genome %d" % G)
    step = 1 << 16
    NW = (n + 63) // 64
    T = np.zeros((G, NW), _U64)
    shared = np.zeros((G, G), _U64)
    for lo in range(0, n, step):
        hi = min(lo + step, n)
        u = np.unpackbits(b[lo:hi].view(np.uint8).reshape(hi - lo, W * 8), axis=1, bitorder="little")[:, :G]
        f = u.astype(np.float32)
        shared += (f.T @ f).astype(_U64)                      # (sums below 2^16: exact in float32)
        ut = np.zeros((G, (hi - lo + 63) // 64 * 64), np.uint8)
        ut[:, :hi - lo] = u.T
        T[:, lo // 64:lo // 64 + ut.shape[1] // 64] = np.packbits(ut, axis=1, bitorder="little").view(_U64)
    pan, core = np.zeros((P, G), _U64), np.zeros((P, G), _U64)
    if P and G:
        valid = np.full(NW, ~_U64(0))
        if n & 63:
            valid[NW - 1] = (_U64(1) << _U64(n & 63)) - _U64(1)
        run_or, run_and = np.zeros((P, NW), _U64), np.tile(valid, (P, 1))
        for i in range(G):
            x = T[o[:, i]]
            run_or |= x
            run_and &= x
            pan[:, i], core[:, i] = _popcount_sum(run_or), _popcount_sum(run_and)
    return shared, pan, core


def write_compare_files(prefix: str, names, shared, orders, pan, core, tag: str = "_fr_", curve: bool = True) -> None:
    """The four `-p` files of `prefix` (the input's path): `_fr_shared.tsv`
    (the matrix), `_fr_jaccard.tsv` (1 - shared / union, six decimals; 0 for an
    empty union), `_fr_curve.tsv` (per number of genomes the sum, minimum and
    maximum of pan and core over the orders) and `_fr_compare.npz`; each is
    written to `.tmp` and renamed when whole.  tag: what stands for `_fr_` in
    the names (`_km_`: the k-mer colours' files); curve False: no curve file."""
    s = np.asarray(shared, _U64)
    G = s.shape[0]
    o = np.asarray(orders, np.int32).reshape(-1, G) if G else np.zeros((len(orders), 0), np.int32)
    pan, core = np.asarray(pan, _U64).reshape(o.shape), np.asarray(core, _U64).reshape(o.shape)
    nm = [bytes(x) for x in names]

    def whole(suffix, fill):
        fn = prefix + suffix
        with open(fn + ".tmp", "wb") as f:
            fill(f)
        os.replace(fn + ".tmp", fn)
    head = b"#genome" + b"".join(b"\t" + x for x in nm) + b"\n"
    sl = s.tolist()
    whole(tag + "shared.tsv", lambda f: f.write(head + b"".join(
        nm[g] + "".join("\t%d" % v for v in sl[g]).encode() + b"\n" for g in range(G))))

    def jac(g, h):
        u = sl[g][g] + sl[h][h] - sl[g][h]
        return "\t%.6f" % (1.0 - sl[g][h] / u if u else 0.0)
    whole(tag + "jaccard.tsv", lambda f: f.write(head + b"".join(
        nm[g] + "".join(jac(g, h) for h in range(G)).encode() + b"\n" for g in range(G))))
    P = o.shape[0]
    cols = [[[int(x) for x in a[:, i].tolist()] for i in range(G)] for a in (pan, core)]
    stat = lambda v: (sum(v), min(v) if v else 0, max(v) if v else 0)
    curve and whole(tag + "curve.tsv", lambda f: f.write((
        "#genomes\torders\tpan_sum\tpan_min\tpan_max\tcore_sum\tcore_min\tcore_max\n" + "".join(
            "%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % ((i + 1, P) + stat(cols[0][i]) + stat(cols[1][i]))
            for i in range(G))).encode()))
    gn = np.array(nm, dtype=np.bytes_) if nm else np.zeros(0, "S1")
    whole(tag + "compare.npz", lambda f: np.savez(f, genomes=gn, shared=s, orders=o, pan=pan, core=core))


# -------------------------------------------------------------- k-mer colours
def kmer_colors(key_sets, n_groups: int, keys=None) -> dict:
    """The k-mer colours' specification (pg_kmer_colors computes the same on
    the device; include/pangenome.h, "k-mer colours", has the definition).
    key_sets: per genome 0 .. n_groups - 1 a sorted uint64 key array, the keys
    of the dBG of that genome's records alone; keys: the table's keys (None:
    the union of the sets; a key of no set is uncoloured; a set's key that the
    table lacks colours nothing).  Returns keys (ascending), bits (uint64
    [n, ceil(n_groups / 64)], genome g = bit g % 64 of word g / 64),
    n_genomes, kmers_by_g [n_groups + 1], g_kmers, g_core, g_shell, g_unique
    (unique only when n_groups > 1) and shared (freq_compare's, over the keys)."""
    G = int(n_groups)
    if len(key_sets) != G:
        raise ValueError("kmer_colors: %d key sets for %d genomes" % (len(key_sets), G))
    W = (G + 63) // 64
    sets = [np.unique(np.asarray(k, dtype=_U64).reshape(-1)) for k in key_sets]
    if keys is None:
        keys = np.unique(np.concatenate(sets)) if sets else np.zeros(0, _U64)
    else:
        keys = np.unique(np.asarray(keys, dtype=_U64).reshape(-1))
    n = keys.shape[0]
    bits = np.zeros((n, W), _U64)
    for g, ks in enumerate(sets):
        i = np.searchsorted(keys, ks)
        i = i[(i < n) & (keys[np.minimum(i, max(n - 1, 0))] == ks)] if n else i[:0]
        bits[i, g >> 6] |= _U64(1) << _U64(g & 63)
    ng = _popcount_rows(bits)
    t = {"n_groups": G, "keys": keys, "bits": bits, "n_genomes": ng,
         "kmers_by_g": np.bincount(ng, minlength=G + 1).astype(_U64)}
    core, uniq = ng == G, (ng == 1) & (G > 1)
    for name, sel in (("g_kmers", slice(None)), ("g_core", core), ("g_unique", uniq)):
        b = bits[sel]
        t[name] = np.array([int(((b[:, g >> 6] >> _U64(g & 63)) & _U64(1)).sum()) for g in range(G)], dtype=_U64)
    t["g_shell"] = t["g_kmers"] - t["g_core"] - t["g_unique"]
    t["shared"] = freq_compare(bits, G, None)[0]
    return t


def kmer_distance(shared) -> np.ndarray:
    """d[g][h] = shared[g][g] + shared[h][h] - 2 shared[g][h]: the keys in
    exactly one of the two genomes, as pg_tree_nj takes a host matrix;
    ValueError, naming the limit, for an entry above pg_tree_nj's 2^31."""
    s = np.asarray(shared, _U64)
    dg = s.diagonal()
    d = dg[:, None] + dg[None, :] - _U64(2) * s
    if d.size and int(d.max()) > TREE_MAX_DIST:
        raise ValueError("-K with -T: a k-mer distance of %d is above pg_tree_nj's limit of 2^31 = %d"
                         % (int(d.max()), TREE_MAX_DIST))
    return d


def write_kmer_files(prefix: str, table: dict, genome_names) -> None:
    """The first two `-K` files of `prefix` (the input's path): `_km_spectrum.tsv`
    (`#genomes kmers`, one line for each of 0 .. G) and `_km_genomes.tsv`
    (`#genome kmers core shell unique`) from kmers_by_g and the g_ columns of
    table; each is written to `.tmp` and renamed when whole."""
    def whole(suffix, fill):
        fn = prefix + suffix
        with open(fn + ".tmp", "wb") as f:
            fill(f)
        os.replace(fn + ".tmp", fn)
    by_g = [int(x) for x in table["kmers_by_g"]]
    whole("_km_spectrum.tsv", lambda f: f.write(("#genomes\tkmers\n" + "".join(
        "%d\t%d\n" % (g, v) for g, v in enumerate(by_g))).encode()))
    cols = [[int(x) for x in table[k]] for k in ("g_kmers", "g_core", "g_shell", "g_unique")]
    whole("_km_genomes.tsv", lambda f: f.write(b"#genome\tkmers\tcore\tshell\tunique\n" + b"".join(
        bytes(nm) + ("\t%d\t%d\t%d\t%d\n" % x).encode() for nm, x in zip(genome_names, zip(*cols)))))


# ---------------------------------------------------------------- genome tree
TREE_FRAC_BITS = 16
TREE_MAX_LEAVES = 16384
TREE_MAX_DIST = 1 << 31


def tree_nj(dist):
    """The genome tree's specification (pg_tree_nj computes the same on the
    device; include/pangenome.h, "genome tree", has the definition).  dist:
    [n, n] non-negative integers, symmetric, zero diagonal, no entry above
    2^31, n <= 16384 (ValueError otherwise).  Returns (joins, root): joins a
    dict of left, right (uint32 [J], J = max(n - 3, 0)) and left_len, right_len
    (uint64 [J], 16 fractional bits); root = (child uint32 [<= 3], len uint64).
    Integers only: the matrix and the row sums are int64 arrays, which the
    header's bound (|Q| < 2^63) keeps exact, `>>` and `//` round towards minus
    infinity, and the scalars of a join are Python integers.  The live slots
    are kept dense in their order (a dead slot's row and column are deleted),
    so the first minimum of the row-major upper triangle is the smallest
    (i, j) among equal Q."""
    d = np.ascontiguousarray(dist, dtype=_U64)
    n = d.shape[0]
    if n > TREE_MAX_LEAVES:
        raise ValueError("tree_nj: %d leaves, at most %d" % (n, TREE_MAX_LEAVES))
    d = d.reshape(n, n)
    if n and int(d.max()) > TREE_MAX_DIST:
        raise ValueError("tree_nj: an entry above 2^31")
    if d.diagonal().any():
        raise ValueError("tree_nj: a non-zero diagonal")
    if not np.array_equal(d, d.T):
        raise ValueError("tree_nj: the matrix is not symmetric")
    S = TREE_FRAC_BITS
    D = d.astype(np.int64) << S
    r = D.sum(axis=1)
    node = np.arange(n, dtype=np.int64)
    J = max(n - 3, 0)
    joins = {"left": np.zeros(J, np.uint32), "right": np.zeros(J, np.uint32),
             "left_len": np.zeros(J, _U64), "right_len": np.zeros(J, _U64)}
    low = np.tri(n, dtype=bool) if J else None           # (on and below the diagonal: no pair)
    big = np.iinfo(np.int64).max
    for t in range(J):
        m = n - t
        Q = (m - 2) * D - r[:, None] - r[None, :]
        Q[low[:m, :m]] = big
        i, j = divmod(int(np.argmin(Q)), m)
        dij = int(D[i, j])
        li = min(max((dij + (int(r[i]) - int(r[j])) // (m - 2)) >> 1, 0), dij)
        joins["left"][t], joins["right"][t] = node[i], node[j]
        joins["left_len"][t], joins["right_len"][t] = li, dij - li
        new = np.maximum(0, (D[i] + D[j] - dij) >> 1)
        new[i] = new[j] = 0
        r += new - D[i] - D[j]
        r[i] = int(new.sum())
        D[i, :] = new
        D[:, i] = new
        node[i] = n + t
        D = np.delete(np.delete(D, j, axis=0), j, axis=1)
        r, node = np.delete(r, j), np.delete(node, j)
    D = [[int(v) for v in row] for row in D.tolist()]
    if n >= 3:
        (a, b, c) = (0, 1, 2)
        ln = [max(0, (D[a][b] + D[a][c] - D[b][c]) >> 1), max(0, (D[a][b] + D[b][c] - D[a][c]) >> 1),
              max(0, (D[a][c] + D[b][c] - D[a][b]) >> 1)]
    elif n == 2:
        ln = [D[0][1] >> 1, D[0][1] - (D[0][1] >> 1)]
    else:
        ln = [0] * n
    return joins, (node.astype(np.uint32), np.array(ln, dtype=_U64))


def tree_len_text(v: int) -> bytes:
    """A length of 16 fractional bits as the tree files print it: six
    decimals, cut and not rounded."""
    v = int(v)
    return b"%d.%06d" % (v >> TREE_FRAC_BITS, ((v & 65535) * 1000000) >> TREE_FRAC_BITS)


def tree_name_text(name) -> bytes:
    """A leaf's name as the Newick text holds it: verbatim, or in single
    quotes with the inner quotes doubled if it has one of ()[]{}:;,'" or
    white space."""
    nm = name.encode() if isinstance(name, str) else bytes(name)
    if any(ch in b"()[]{}:;,'\" \t\n\r\x0b\x0c" for ch in nm):
        return b"'" + nm.replace(b"'", b"''") + b"'"
    return nm


def tree_newick(names, joins, root, support=None) -> bytes:
    """The Newick text of tree_nj's (or the device's) tables over the leaves
    called names: `(<child>:<len>,<child>:<len>,<child>:<len>);` and a line
    feed, nested, each join's left child before its right.  No leaf: empty.
    support: None, or (counts [J], replicates) of tree_bootstrap - every
    join's closing parenthesis is then followed by floor(100 * count /
    replicates) as the node's label; the root's carries none."""
    n = len(names)
    if not n:
        return b""
    pct = None
    if support is not None:
        pct = [b"%d" % (100 * int(s) // int(support[1])) for s in support[0]]
    left, right = [int(x) for x in joins["left"]], [int(x) for x in joins["right"]]
    ll, rl = [int(x) for x in joins["left_len"]], [int(x) for x in joins["right_len"]]
    out = []
    # (an explicit stack: a comb of 16384 leaves is as deep as it is long)
    stack = [b");\n"]
    kids = list(zip([int(x) for x in root[0]], [int(x) for x in root[1]]))
    for k, (c, v) in reversed(list(enumerate(kids))):
        stack.append(b":" + tree_len_text(v) + (b"," if k + 1 < len(kids) else b""))
        stack.append(c)
    out.append(b"(")
    while stack:
        x = stack.pop()
        if isinstance(x, bytes):
            out.append(x)
        elif x < n:
            out.append(tree_name_text(names[x]))
        else:
            t = x - n
            stack.append(b":" + tree_len_text(rl[t]) + b")" + (pct[t] if pct else b""))
            stack.append(right[t])
            stack.append(b":" + tree_len_text(ll[t]) + b",")
            stack.append(left[t])
            out.append(b"(")
    return b"".join(out)


def write_tree_files(prefix: str, names, dist, joins, root, var: bool = False, tag: str = "_fr_") -> None:
    """The `-T` files of `prefix` (the input's path): `_fr_dist.tsv` (the
    distance matrix in `_fr_shared.tsv`'s layout), `_fr_tree.nwk`,
    `_fr_tree.tsv` (per join the node it makes, its two children and their
    lengths as the Newick prints them, then one `#root` line: the children,
    then their lengths) and `_fr_tree.npz`; var: the tree of the differences,
    `_fr_vardist.tsv` and `_fr_vartree.nwk` alone.  Each is written to `.tmp`
    and renamed when whole.  tag: what stands for `_fr_` in the names (`_km_`:
    the k-mer tree's files)."""
    d = np.asarray(dist, _U64)
    n = d.shape[0]
    nm = [bytes(x) for x in names]

    def whole(suffix, fill):
        fn = prefix + suffix
        with open(fn + ".tmp", "wb") as f:
            fill(f)
        os.replace(fn + ".tmp", fn)
    head = b"#genome" + b"".join(b"\t" + x for x in nm) + b"\n"
    dl = d.tolist()
    whole(tag + ("vardist.tsv" if var else "dist.tsv"), lambda f: f.write(head + b"".join(
        nm[g] + "".join("\t%d" % v for v in dl[g]).encode() + b"\n" for g in range(n))))
    whole(tag + ("vartree.nwk" if var else "tree.nwk"), lambda f: f.write(tree_newick(nm, joins, root)))
    if var:
        return
    cols = [[int(x) for x in joins[k]] for k in ("left", "right", "left_len", "right_len")]
    child, ln = [int(x) for x in root[0]], [int(x) for x in root[1]]
    whole(tag + "tree.tsv", lambda f: f.write(
        b"#node\tleft\tright\tleft_len\tright_len\n" + b"".join(
            b"%d\t%d\t%d\t%s\t%s\n" % (n + t, a, b, tree_len_text(x), tree_len_text(y))
            for t, (a, b, x, y) in enumerate(zip(*cols))) +
        b"#root" + b"".join(b"\t%d" % c for c in child) + b"".join(b"\t" + tree_len_text(v) for v in ln) + b"\n"))
    gn = np.array(nm, dtype=np.bytes_) if nm else np.zeros(0, "S1")
    whole(tag + "tree.npz", lambda f: np.savez(
        f, genomes=gn, dist=d, left=np.asarray(joins["left"], np.uint32), right=np.asarray(joins["right"], np.uint32),
        left_len=np.asarray(joins["left_len"], _U64), right_len=np.asarray(joins["right_len"], _U64),
        root_child=np.asarray(root[0], np.uint32), root_len=np.asarray(root[1], _U64),
        frac_bits=np.int64(TREE_FRAC_BITS)))


# --------------------------------------------------------------- tree support
BOOT_MAX_REPS = 4096
BOOT_MAX_LABELS = 1 << 31


def boot_index(x, L: int) -> np.ndarray:
    """idx = ((x >> 32) * L) >> 32 of 64-bit outputs x, in unsigned 64 bits:
    in [0, L), and the product does not wrap while L <= 2^31."""
    L = int(L)
    if not 0 <= L <= BOOT_MAX_LABELS:
        raise ValueError("boot_index: %d labels, at most 2^31" % L)
    return ((np.asarray(x, _U64) >> _U64(32)) * _U64(L)) >> _U64(32)


def boot_draws(seed: int, b: int, L: int) -> np.ndarray:
    """Replicate b's drawn rows, uint64 [L]: idx(b, t) = boot_index of output
    t of synth.splitmix64(seed, b + 1, L)."""
    from . import synth
    return boot_index(synth.splitmix64(int(seed), int(b) + 1, int(L)), L)


def tree_splits(joins, n: int) -> list:
    """The split of every join of a tree over n leaves, as Python integers
    (bit g = genome g): the join's clade - a leaf's is itself, a node's the
    union of its children's - if leaf 0 is not in it, otherwise the
    complement within 0 .. n - 1."""
    left, right = [int(x) for x in joins["left"]], [int(x) for x in joins["right"]]
    full = (1 << n) - 1
    clade = [1 << i for i in range(n)]
    out = []
    for a, b in zip(left, right):
        c = clade[a] | clade[b]
        clade.append(c)
        out.append(full ^ c if c & 1 else c)
    return out


def tree_clade_sizes(joins, n: int) -> list:
    """The number of leaves below every join (its clade, not its split)."""
    size = [1] * n
    for a, b in zip(joins["left"], joins["right"]):
        size.append(size[int(a)] + size[int(b)])
    return size[n:]


def tree_bootstrap(bits, n_groups: int, joins, n_reps: int, seed: int, dist=None, rep_dist: bool = False) -> dict:
    """Tree support's specification (pg_tree_bootstrap computes the same on
    the device; include/pangenome.h, "tree support", has the definition).
    bits: uint64 [L, W] presence words; joins: the rated tree's (tree_nj's
    dict, or the device's); n_reps in [1, 4096].  dist: None, or the matrix
    the rated tree was built from - ValueError if it is not the Hamming
    matrix of bits (the guard).  Returns support uint32 [J] (the replicates
    whose tree has join t's split), rep_left and rep_right uint32 [R, J] (the
    replicate trees' joins) and, asked for, rep_dist uint64 [R, n, n].
    A replicate's matrix: with c[l] = how often row l was drawn and u the 0 / 1
    table, s = u^T diag(c) u in float64 (exact: sums at most 2^31) and
    d(g, h) = s[g][g] + s[h][h] - 2 s[g][h]."""
    G, R = int(n_groups), int(n_reps)
    W = (G + 63) // 64
    b = np.ascontiguousarray(bits, dtype=_U64)
    L = b.shape[0]
    b = b.reshape(L, W)
    if not 1 <= R <= BOOT_MAX_REPS:
        raise ValueError("tree_bootstrap: %d replicates: 1 to %d" % (R, BOOT_MAX_REPS))
    if L > BOOT_MAX_LABELS:
        raise ValueError("tree_bootstrap: %d labels, at most 2^31" % L)
    if G & 63 and L and (b[:, W - 1] >> _U64(G & 63)).any():
        raise ValueError("tree_bootstrap: a row has a bit at or above genome %d" % G)
    J = max(G - 3, 0)
    if len(joins["left"]) != J:
        raise ValueError("tree_bootstrap: the tree has %d joins, %d genomes have %d" % (len(joins["left"]), G, J))
    u = np.unpackbits(b.view(np.uint8).reshape(L, W * 8), axis=1, bitorder="little")[:, :G].astype(np.float64)

    def hamming(count):
        s = (u * count[:, None]).T @ u
        dg = np.diag(s)
        return (dg[:, None] + dg[None, :] - 2 * s).astype(_U64)
    if dist is not None and not np.array_equal(hamming(np.ones(L)), np.asarray(dist, _U64).reshape(G, G)):
        raise ValueError("tree_bootstrap: the tree was not built from this table")
    where = {}
    for t, s in enumerate(tree_splits(joins, G)):
        where[s] = t
    out = {"support": np.zeros(J, np.uint32), "rep_left": np.zeros((R, J), np.uint32),
           "rep_right": np.zeros((R, J), np.uint32)}
    if rep_dist:
        out["rep_dist"] = np.zeros((R, G, G), _U64)
    for r in range(R):
        count = np.bincount(boot_draws(seed, r, L).astype(np.int64), minlength=L).astype(np.float64)
        d = hamming(count)
        if rep_dist:
            out["rep_dist"][r] = d
        rj, _ = tree_nj(d)
        out["rep_left"][r], out["rep_right"][r] = rj["left"], rj["right"]
        for s in tree_splits(rj, G):
            if s in where:
                out["support"][where[s]] += 1
    return out


def write_tree_support_files(prefix: str, names, joins, root, boot: dict, seed: int, var: bool = False) -> None:
    """The `-B` files of `prefix`: `_fr_tree_support.nwk` (`_fr_tree.nwk` with
    every join's support as an integer percentage behind its closing
    parenthesis), `_fr_tree_support.tsv` (per join its node, the raw count,
    the replicates and the clade's leaves) and `_fr_tree_boot.npz`; var: the
    tree of the differences, `_fr_vartree_support.nwk` and `.tsv` alone.  boot:
    tree_bootstrap's dict (or the device's).  Each is written to `.tmp` and
    renamed when whole."""
    nm = [bytes(x) for x in names]
    n = len(nm)
    sup = np.asarray(boot["support"], np.uint32)
    R = int(np.asarray(boot["rep_left"]).shape[0])
    stem = "_fr_vartree_support" if var else "_fr_tree_support"

    def whole(suffix, fill):
        fn = prefix + suffix
        with open(fn + ".tmp", "wb") as f:
            fill(f)
        os.replace(fn + ".tmp", fn)
    whole(stem + ".nwk", lambda f: f.write(tree_newick(nm, joins, root, support=(sup, R))))
    whole(stem + ".tsv", lambda f: f.write(b"#node\tsupport\treplicates\tleaves\n" + b"".join(
        b"%d\t%d\t%d\t%d\n" % (n + t, int(s), R, k) for t, (s, k) in enumerate(zip(sup, tree_clade_sizes(joins, n))))))
    if var:
        return
    gn = np.array(nm, dtype=np.bytes_) if nm else np.zeros(0, "S1")
    whole("_fr_tree_boot.npz", lambda f: np.savez(
        f, genomes=gn, support=sup, replicates=np.int64(R), seed=np.uint64(seed),
        rep_left=np.asarray(boot["rep_left"], np.uint32), rep_right=np.asarray(boot["rep_right"], np.uint32)))


REGION_COLS = (("labels", np.int64), ("rows", np.uint64), ("max_len", np.uint64), ("n_out", np.uint32),
               ("n_in", np.uint32), ("link_from", np.int64), ("link_to", np.int64), ("link_count", np.uint64),
               ("link_genomes", np.uint32), ("path_record", np.int64), ("path_strand", np.int64),
               ("path_lo", np.int64), ("path_hi", np.int64), ("path_steps", np.uint64))


def write_region_files(prefix: str, write_links, write_gfa, table: dict, genome_names) -> None:
    """The four `-l` files of `prefix` (the input's path): `_fr_links.tsv` and
    `_fr_graph.gfa` (write_links(file) / write_gfa(file) write the texts),
    `_fr_nodes.tsv` from the table's node columns and `_fr_graph.npz` (every
    column of REGION_COLS and the genome names); each is written to `.tmp`
    and renamed when whole."""
    def whole(suffix, fill):
        fn = prefix + suffix
        with open(fn + ".tmp", "wb") as f:
            fill(f)
        os.replace(fn + ".tmp", fn)
    whole("_fr_links.tsv", write_links)
    cols = [np.asarray(table[k]).tolist() for k in ("labels", "rows", "max_len", "n_out", "n_in")]
    whole("_fr_nodes.tsv", lambda f: f.write(("#label\trows\tmax\tout\tin\n" + "".join(
        "%d\t%d\t%d\t%d\t%d\n" % x for x in zip(*cols))).encode()))
    whole("_fr_graph.gfa", write_gfa)
    arrays = {k: np.ascontiguousarray(table[k], dtype=t).reshape(-1) for k, t in REGION_COLS}
    arrays["genomes"] = (np.array([bytes(x) for x in genome_names], dtype=np.bytes_) if genome_names
                         else np.zeros(0, "S1"))
    whole("_fr_graph.npz", lambda f: np.savez(f, **arrays))


REGION_SEQ_COLS = ("label", "row", "record", "start", "end", "strand", "len", "gc", "amb")


def write_region_seq_files(prefix: str, write_fasta, table: dict, ids, write_gfa=None) -> None:
    """The `-s` files of `prefix` (the input's path): `_fr_regions.fa`
    (write_fasta(file) writes the text), `_fr_regions.tsv` from the table's
    columns (a record is printed by its seqid, ids[record]) and, with
    write_gfa, `_fr_graph_seq.gfa`; each is written to `.tmp` and renamed
    when whole."""
    def whole(suffix, fill):
        fn = prefix + suffix
        with open(fn + ".tmp", "wb") as f:
            fill(f)
        os.replace(fn + ".tmp", fn)
    whole("_fr_regions.fa", write_fasta)
    cols = [np.asarray(table[k]).tolist() for k in REGION_SEQ_COLS]
    whole("_fr_regions.tsv", lambda f: f.write(b"#label\trow\tseqid\tstart\tend\tstrand\tlen\tgc\tamb\n" + b"".join(
        b"%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (l, r, bytes(ids[rec]), s, e, st, n, gc, amb)
        for l, r, rec, s, e, st, n, gc, amb in zip(*cols))))
    if write_gfa is not None:
        whole("_fr_graph_seq.gfa", write_gfa)


SITES_COLS = (("site_from", np.int64), ("site_to", np.int64), ("site_alleles", np.uint32), ("site_first", np.uint64),
              ("site_count", np.uint64), ("site_genomes", np.uint32), ("allele_site", np.uint64),
              ("allele_via", np.int64), ("allele_count", np.uint64), ("allele_genomes", np.uint32),
              ("allele_min", np.uint64), ("allele_max", np.uint64), ("genome_sites", np.uint64),
              ("genome_alleles", np.uint64), ("genome_private", np.uint64))


def write_sites_files(prefix: str, write_sites, table: dict, genome_names) -> None:
    """The three `-v` files of `prefix` (the input's path): `_fr_sites.tsv`
    (write_sites(file) writes the text), `_fr_sites_genomes.tsv` from the
    table's per-genome columns and `_fr_sites.npz` (every column of
    SITES_COLS, `bits` as uint64 [alleles, W] and the genome names); each is
    written to `.tmp` and renamed when whole."""
    def whole(suffix, fill):
        fn = prefix + suffix
        with open(fn + ".tmp", "wb") as f:
            fill(f)
        os.replace(fn + ".tmp", fn)
    nm = [bytes(x) for x in genome_names]
    whole("_fr_sites.tsv", write_sites)
    cols = [np.asarray(table[k]).tolist() for k in ("genome_sites", "genome_alleles", "genome_private")]
    whole("_fr_sites_genomes.tsv", lambda f: f.write(b"#genome\tsites\talleles\tprivate\n" + b"".join(
        b"%s\t%d\t%d\t%d\n" % x for x in zip(nm, *cols))))
    arrays = {k: np.ascontiguousarray(table[k], dtype=t).reshape(-1) for k, t in SITES_COLS}
    n = arrays["allele_site"].shape[0]
    arrays["bits"] = np.ascontiguousarray(table["bits"], dtype=_U64).reshape(n, (len(nm) + 63) // 64)
    arrays["genomes"] = np.array(nm, dtype=np.bytes_) if nm else np.zeros(0, "S1")
    whole("_fr_sites.npz", lambda f: np.savez(f, **arrays))


BUBBLES_COLS = (("site_from", np.int64), ("site_to", np.int64), ("site_alleles", np.uint32),
                ("site_first", np.uint64), ("site_count", np.uint64), ("site_genomes", np.uint32),
                ("allele_site", np.uint64), ("allele_regions", np.uint64), ("allele_first_row", np.uint64),
                ("allele_count", np.uint64), ("allele_genomes", np.uint32), ("allele_min_bp", np.uint64),
                ("allele_max_bp", np.uint64), ("allele_inner_off", np.uint64), ("inner", np.int64),
                ("genome_sites", np.uint64), ("genome_alleles", np.uint64), ("genome_private", np.uint64),
                ("anchors", np.int64), ("anchor_genomes", np.uint32))


def write_bubbles_files(prefix: str, write_bubbles, table: dict, genome_names, min_genomes: int) -> None:
    """The three `-b` files of `prefix` (the input's path): `_fr_bubbles.tsv`
    (write_bubbles(file) writes the text), `_fr_bubbles_genomes.tsv` from the
    table's per-genome columns and `_fr_bubbles.npz` (every column of
    BUBBLES_COLS, `bits` as uint64 [alleles, W], the genome names and
    min_genomes); each is written to `.tmp` and renamed when whole."""
    def whole(suffix, fill):
        fn = prefix + suffix
        with open(fn + ".tmp", "wb") as f:
            fill(f)
        os.replace(fn + ".tmp", fn)
    nm = [bytes(x) for x in genome_names]
    whole("_fr_bubbles.tsv", write_bubbles)
    cols = [np.asarray(table[k]).tolist() for k in ("genome_sites", "genome_alleles", "genome_private")]
    whole("_fr_bubbles_genomes.tsv", lambda f: f.write(b"#genome\tsites\talleles\tprivate\n" + b"".join(
        b"%s\t%d\t%d\t%d\n" % x for x in zip(nm, *cols))))
    arrays = {k: np.ascontiguousarray(table[k], dtype=t).reshape(-1) for k, t in BUBBLES_COLS}
    n = arrays["allele_site"].shape[0]
    arrays["bits"] = np.ascontiguousarray(table["bits"], dtype=_U64).reshape(n, (len(nm) + 63) // 64)
    arrays["genomes"] = np.array(nm, dtype=np.bytes_) if nm else np.zeros(0, "S1")
    arrays["min_genomes"] = np.array(int(min_genomes), np.int64)
    whole("_fr_bubbles.npz", lambda f: np.savez(f, **arrays))


VCF_NS = b'##INFO=<ID=NS,Number=1,Type=Integer,Description="Genomes with an allele at the site">\n'
VCF_GT = (b'##FORMAT=<ID=GT,Number=.,Type=String,Description="Every allele of the site found in the genome, '
          b'unphased; . if none">\n')


def vcf_header(ref_name, contigs, genome_names) -> bytes:
    """The header of `_fr_variants.vcf`: the file format, the source, the
    reference genome's name, a contig line per (seqid, length) of contigs -
    the walked records of that genome - the NS and GT meta lines and the
    column line with the genome names."""
    out = [b"##fileformat=VCFv4.2\n", b"##source=pangenome_amd\n", b"##reference=%s\n" % bytes(ref_name)]
    out += [b"##contig=<ID=%s,length=%d>\n" % (bytes(i), int(n)) for i, n in contigs]
    out += [VCF_NS, VCF_GT, b"\t".join([b"#CHROM", b"POS", b"ID", b"REF", b"ALT", b"QUAL", b"FILTER", b"INFO",
                                        b"FORMAT"] + [bytes(x) for x in genome_names]) + b"\n"]
    return b"".join(out)


VCF_AC = b'##INFO=<ID=AC,Number=1,Type=Integer,Description="Alleles of the site that carry the difference">\n'
VCF_GT_PRIM = (b'##FORMAT=<ID=GT,Number=.,Type=String,Description="1: an allele of the site in the genome carries the '
               b'difference, 0: one does not, 0/1: both, unphased; . if the genome has no allele">\n')


def primitives_vcf_header(ref_name, contigs, genome_names) -> bytes:
    """The header of `_fr_primitives.vcf`: vcf_header's lines with an AC meta
    line after NS and the GT description of a line per difference."""
    return vcf_header(ref_name, contigs, genome_names).replace(VCF_GT, VCF_AC + VCF_GT_PRIM)


def write_align_files(prefix: str, write_tsv, header: bytes, write_vcf) -> None:
    """The two `-A` files of `prefix` (the input's path): `_fr_align.tsv`
    (write_tsv(file) writes the text) and `_fr_primitives.vcf`: header, then
    the body write_vcf(file) writes; each is written to `.tmp` and renamed
    when whole."""
    def whole(suffix, fill):
        fn = prefix + suffix
        with open(fn + ".tmp", "wb") as f:
            fill(f)
        os.replace(fn + ".tmp", fn)
    whole("_fr_align.tsv", write_tsv)

    def vcf(f):
        f.write(header)
        write_vcf(f)
    whole("_fr_primitives.vcf", vcf)


VARIANT_COLS = ("from", "to", "allele", "regions", "record", "lo", "hi", "strand", "len", "gc", "amb")


def write_variants_files(prefix: str, write_fasta, table: dict, ids, header: bytes, write_vcf) -> None:
    """The three `-V` files of `prefix` (the input's path): `_fr_alleles.fa`
    (write_fasta(file) writes the text), `_fr_alleles.tsv` from the table's
    columns (VARIANT_COLS; a record is printed by its seqid, ids[record]) and
    `_fr_variants.vcf`: header, then the body write_vcf(file) writes; each is
    written to `.tmp` and renamed when whole."""
    def whole(suffix, fill):
        fn = prefix + suffix
        with open(fn + ".tmp", "wb") as f:
            fill(f)
        os.replace(fn + ".tmp", fn)
    whole("_fr_alleles.fa", write_fasta)
    cols = [np.asarray(table[k]).tolist() for k in VARIANT_COLS]
    whole("_fr_alleles.tsv", lambda f: f.write(
        b"#from\tto\tallele\tregions\tseqid\tstart\tend\tstrand\tlen\tgc\tamb\n" + b"".join(
            b"%d\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (a, c, k, r, bytes(ids[rec]), lo, hi, st, n, gc, amb)
            for a, c, k, r, rec, lo, hi, st, n, gc, amb in zip(*cols))))

    def vcf(f):
        f.write(header)
        write_vcf(f)
    whole("_fr_variants.vcf", vcf)


def seqid(name: bytes) -> bytes:
    """A record's id: its header without '>' up to the first whitespace."""
    p = bytes(name).split(None, 1)
    return p[0] if p else b""


def read_group_file(path: str) -> dict:
    """`seqid<TAB>genome` lines -> {seqid: genome} (bytes); blank lines and
    lines starting with '#' are skipped, a later line for a seqid wins."""
    m = {}
    with open(path, "rb") as f:
        for ln in f:
            ln = ln.rstrip(b"\r\n")
            if not ln.strip() or ln.startswith(b"#"):
                continue
            p = ln.split(b"\t")
            if len(p) < 2 or not p[1].strip():
                raise ValueError("%s: not a seqid<TAB>genome line: %r" % (path, ln[:80]))
            m[p[0].strip()] = p[1].strip()
    return m


def read_groups(path: str, record_ids) -> list:
    """The genome name of every id in record_ids from a `-g` file; ids the
    file does not hold are a ValueError naming up to five of them."""
    m = read_group_file(path)
    ids = [bytes(x) for x in record_ids]
    missing = [x for x in ids if x not in m]
    if missing:
        raise ValueError("%s: no genome for %d record(s): %s%s" % (
            path, len(missing), ", ".join(x.decode("utf-8", "replace") for x in missing[:5]),
            ", ..." if len(missing) > 5 else ""))
    return [m[x] for x in ids]


def assign_groups(names, flags, groups: str):
    """-g: the genome of every record.  names[r] = record r's header without
    '>'; flags = the records the row pass walks (plan_rows).  groups ==
    "record": every walked record is its own genome, named by its seqid;
    otherwise a `seqid<TAB>genome` file (read_groups).  Genomes are numbered
    by first appearance over the walked records; the others get -1.  Returns
    (rec_group int32 [R], genome names)."""
    walked = np.flatnonzero(np.asarray(flags)).tolist()
    ids = [seqid(names[r]) for r in walked]
    gn = ids if groups == "record" else read_groups(groups, ids)
    rec_group = np.full(len(names), -1, np.int32)
    number, order = {}, []
    for r, nm in zip(walked, gn):
        key = (r, nm) if groups == "record" else nm
        if key not in number:
            number[key] = len(order)
            order.append(nm)
        rec_group[r] = number[key]
    return rec_group, order


def rows_from_text(text: bytes, names, flags) -> np.ndarray:
    """The [n, 5] rows of a printed row text whose records are names[r]
    (a backend without device rows): rows come in record order, so each
    line's qid is matched forward from the last record seen."""
    out = []
    walked = np.flatnonzero(np.asarray(flags)).tolist()
    w = 0
    for ln in bytes(text).split(b"\n"):
        if not ln:
            continue
        q, s, e, st, lab = ln.rsplit(b"\t", 4)
        while w < len(walked) and names[walked[w]] != q:
            w += 1
        if w == len(walked):
            raise ValueError("row text: record %r is not among the walked records in order" % q[:80])
        out.append((walked[w], int(s), int(e), 1 if st == b"+" else -1, int(lab)))
    return np.array(out, np.int64).reshape(-1, 5)


def write_freq_files(prefix: str, write_text, table: dict, genome_names) -> None:
    """The four `-g` files of `prefix` (the input's path): `_fr_freq.tsv`
    (write_text(file) writes the table's text), `_fr_spectrum.tsv`,
    `_fr_genomes.tsv` and `_fr_presence.npz`; each is written to `.tmp` and
    renamed when whole."""
    G = int(table["n_groups"])

    def whole(suffix, fill):
        fn = prefix + suffix
        with open(fn + ".tmp", "wb") as f:
            fill(f)
        os.replace(fn + ".tmp", fn)
    whole("_fr_freq.tsv", write_text)
    sl, sb = table["spectrum_labels"].tolist(), table["spectrum_bp"].tolist()
    whole("_fr_spectrum.tsv", lambda f: f.write(("#genomes\tlabels\tbp\n" + "".join(
        "%d\t%d\t%d\n" % (g, sl[g], sb[g]) for g in range(1, G + 1))).encode()))
    cols = [table[k].tolist() for k in ("g_rows", "g_bp", "g_core", "g_shell", "g_unique")]
    whole("_fr_genomes.tsv", lambda f: f.write(b"#genome\trows\tbp\tcore\tshell\tunique\n" + b"".join(
        bytes(nm) + ("\t%d\t%d\t%d\t%d\t%d\n" % x).encode() for nm, x in zip(genome_names, zip(*cols)))))
    gn = np.array([bytes(x) for x in genome_names], dtype=np.bytes_) if genome_names else np.zeros(0, "S1")
    whole("_fr_presence.npz", lambda f: np.savez(f, labels=np.asarray(table["labels"], np.int64),
                                                 bits=np.asarray(table["bits"], _U64), genomes=gn))
