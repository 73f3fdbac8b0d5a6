"""An independent restatement of Markov clustering (include/pangenome.h,
pg_cluster_markov) for the tests: dense U x U matrices of Python integers for
graphs of at most 64 nodes, nothing shared with pangenome_amd/; and the graph
builders of the Markov tests."""
import hashlib
import math

import numpy as np

ONE = 1 << 31
CUT = ONE // 10000
STOP = ONE // 1000

GRID = [(i2, sel, w) for i2 in (3, 4, 5) for sel in (2, 64) for w in (1, 2)]


def _prune(f, select):
    """f: {row: positive value} -> {row: stored value}"""
    total = sum(f.values())
    n = {i: (v << 31) // total for i, v in f.items()}
    order = sorted(n, key=lambda i: (-n[i], i))
    kept = [order[0]]
    for i in order[1:]:
        if n[i] >= CUT and len(kept) < select:
            kept.append(i)
    t = sum(n[i] for i in kept)
    return {i: (n[i] << 31) // t for i in sorted(kept)}


def _chaos(cols):
    return max((max(c.values()) - (sum(v * v for v in c.values()) >> 31) for c in cols), default=0)


def dense_markov(tuples, counts, min_weight=1, inflation2=3, select=64, max_iter=200):
    """(text, n_iter, chaos, matrix) with matrix = (col_len, rows, vals) as
    lists of lists, by the definition's own words."""
    names, ids = [], {}
    edges = []
    for (a, b, c, d), n in zip(np.asarray(tuples, np.uint64).reshape(-1, 4).tolist(), np.asarray(counts).tolist()):
        for tok in ((a, b), (c, d)):
            if tok not in ids:
                ids[tok] = len(names)
                names.append("%d_%d" % tok)
        edges.append((ids[(a, b)], ids[(c, d)], n))
    U = len(names)
    assert U <= 64
    w = [[0] * U for _ in range(U)]
    for i, j, n in edges:
        if i != j and n >= min_weight:
            w[i][j] += n
            w[j][i] += n
    if any(x >= 1 << 32 for r in w for x in r):
        raise OverflowError("weight sum")
    for j in range(U):
        w[j][j] = max(max(w[i][j] for i in range(U)), 1)
    cols = [_prune({i: w[i][j] for i in range(U) if w[i][j]}, select) for j in range(U)]
    chaos, n_iter = _chaos(cols), 0
    while U and n_iter < max_iter:
        new = []
        for j in range(U):
            acc = {}
            for k, m in cols[j].items():
                for i, v in cols[k].items():
                    acc[i] = acc.get(i, 0) + v * m
            e = {i: a >> 31 for i, a in acc.items()}
            top = max(e.values())
            y = {}
            for i, ei in e.items():
                x = (ei << 31) // top
                yi = ONE
                for _ in range(inflation2 // 2):
                    yi = (yi * x) >> 31
                if inflation2 % 2:
                    yi = (yi * math.isqrt(x << 31)) >> 31
                if yi:
                    y[i] = yi
            new.append(_prune(y, select))
        cols = new
        chaos, n_iter = _chaos(cols), n_iter + 1
        if chaos <= STOP:
            break
    # components of the stored entries; clusters by (size descending, smallest id), members by id
    comp = list(range(U))

    def root(x):
        while comp[x] != x:
            x = comp[x]
        return x
    for j in range(U):
        for i in cols[j]:
            a, b = root(i), root(j)
            if a != b:
                comp[max(a, b)] = min(a, b)
    groups = {}
    for i in range(U):
        groups.setdefault(root(i), []).append(i)
    order = sorted(groups.values(), key=lambda m: (-len(m), m[0]))
    text = "".join("\t".join(names[i] for i in m) + "\n" for m in order)
    matrix = ([len(c) for c in cols], [list(c.keys()) for c in cols], [list(c.values()) for c in cols])
    return text, n_iter, chaos, matrix


def matrix_lists(matrix):
    """host.cluster_markov's / the binding's padded arrays -> dense_markov's lists"""
    col_len, rows, vals = matrix
    return ([int(n) for n in col_len], [rows[j, :n].tolist() for j, n in enumerate(col_len)],
            [vals[j, :n].tolist() for j, n in enumerate(col_len)])


def matrix_digest(matrix):
    col_len, rows, vals = matrix
    h = hashlib.sha256()
    for a in (col_len, rows, vals):
        h.update(np.ascontiguousarray(a, np.uint32).tobytes())
    return h.hexdigest()


def tuples_of(pairs):
    """Edges between abstract node numbers -> (key, value) tuples: distinct
    64-bit keys (an odd multiplier is a bijection mod 2^64), small values."""
    p = np.asarray(pairs, np.uint64).reshape(-1, 2)
    key = p * np.uint64(0x9E3779B97F4A7C15)
    val = p % np.uint64(7)
    return np.stack([key[:, 0], val[:, 0], key[:, 1], val[:, 1]], axis=1)


def star(n):
    return tuples_of([[0, i] for i in range(1, n + 1)]), np.ones(n, np.int64)


def clique(n):
    e = [[i, j] for i in range(n) for j in range(i + 1, n)]
    return tuples_of(e), np.ones(len(e), np.int64)


def ring(n):
    return tuples_of([[i, (i + 1) % n] for i in range(n)]), np.ones(n, np.int64)


def bigcol(n=4500, reach=32, seed=20):
    """node i linked to i +- 1 .. i +- reach modulo n, weights 1..5 from a fixed seed"""
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(n), reach)
    j = (i + np.tile(np.arange(1, reach + 1), n)) % n
    return tuples_of(np.stack([i, j], axis=1)), rng.integers(1, 6, i.shape[0]).astype(np.int64)


def two_triangles():
    e = [[0, 1], [1, 2], [2, 0], [3, 4], [4, 5], [5, 3], [2, 3]]
    return tuples_of(e), np.array([5] * 6 + [1], np.int64)


def candidates(matrix):
    """per column, the bound on its next expansion's candidates: the summed lengths of its stored columns"""
    col_len, rows, _ = matrix
    ln = np.asarray(col_len, np.int64)
    mask = np.arange(rows.shape[1])[None, :] < ln[:, None]
    return np.where(mask, ln[rows.astype(np.int64)], 0).sum(axis=1)


def token(i):
    """the `.mcl` token of abstract node i (tuples_of's key and value)"""
    return "%d_%d" % ((i * 0x9E3779B97F4A7C15) % 2 ** 64, i % 7)


def text_of(clusters):
    return "".join("\t".join(token(i) for i in m) + "\n" for m in clusters)


def hand_cases():
    """name -> (tuples, counts, the clusters at the defaults, written out by hand)"""
    tri_t, tri_c = two_triangles()
    return {
        "no_edges": (np.zeros((0, 4), np.uint64), np.zeros(0, np.int64), []),
        "one_edge": (tuples_of([[0, 1]]), np.array([1], np.int64), [[0, 1]]),
        "self_loop": (tuples_of([[3, 3]]), np.array([9], np.int64), [[3]]),
        "path3": (tuples_of([[0, 1], [1, 2]]), np.array([1, 1], np.int64), [[0, 1, 2]]),
        "two_triangles": (tri_t, tri_c, [[0, 1, 2], [3, 4, 5]]),
        "both_directions": (tuples_of([[0, 1], [1, 0], [1, 2]]), np.array([1, 1, 1], np.int64), [[0, 1, 2]]),
    }


def scaled_values(matrix):
    """the x of the next iteration from a small matrix (dense, Python integers): every expanded value scaled
    to its column's largest"""
    col_len, rows, vals = matrix
    U = len(col_len)
    D = [[0] * U for _ in range(U)]
    for j in range(U):
        for a in range(int(col_len[j])):
            D[int(rows[j, a])][j] = int(vals[j, a])
    xs = []
    for j in range(U):
        e = [sum(D[i][k] * D[k][j] for k in range(U)) >> 31 for i in range(U)]
        xs += [(v << 31) // max(e) for v in e if v]
    return xs


def inflation_graph():
    """weights from 1 to 2^31 around one hub and along a chain of its leaves"""
    w = [1, 2, 3, 4, 9, 16, 17, 255, 256, 65535, 65536, 2 ** 20 + 1, 2 ** 24, 2 ** 30, 2 ** 31 - 1, 2 ** 31]
    e = [[0, i + 1] for i in range(len(w))] + [[i + 1, i + 2] for i in range(len(w) - 1)]
    return tuples_of(e), np.array(w + w[:-1][::-1], np.int64)
