"""An independent reference for the tree support (pg_tree_bootstrap,
host.tree_bootstrap): the loops of the definition in include/pangenome.h,
"tree support", on Python integers and sets; nothing of pangenome_amd.host is
imported (the replicate trees are tree_util.reference_nj's).  Also the inputs
the support tests share and a Newick parser that accepts inner labels."""
import numpy as np

from tree_util import reference_nj

MASK = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15
STREAM = 0xD1B54A32D192ED03


def splitmix_one(seed, stream, t):
    """Output t (from 0) of splitmix64 started at seed ^ (stream * STREAM)."""
    z = (((seed ^ (stream * STREAM)) & MASK) + (t + 1) * GAMMA) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def index_of(x, L):
    """idx = ((x >> 32) * L) >> 32; the product must not pass 64 bits."""
    p = (x >> 32) * L
    assert p <= MASK
    return p >> 32


def draw(seed, b, t, L):
    return index_of(splitmix_one(seed, b + 1, t), L)


def rows_as_ints(bits, G):
    """uint64 [L, W] presence words -> one Python integer per row (bit g = genome g)."""
    b = np.asarray(bits, np.uint64).reshape(-1, (G + 63) // 64)
    return [sum(int(w) << (64 * k) for k, w in enumerate(row)) for row in b]


def hamming_by_counting(rows, G):
    d = [[0] * G for _ in range(G)]
    for row in rows:
        for g in range(G):
            for h in range(G):
                if ((row >> g) ^ (row >> h)) & 1:
                    d[g][h] += 1
    return d


def clades(joins, n):
    """Per join the set of leaves below it."""
    below = [frozenset([i]) for i in range(n)]
    for left, right in joins:
        below.append(below[left] | below[right])
    return below[n:]


def splits(joins, n):
    """Per join its clade if leaf 0 is not in it, else the complement."""
    every = frozenset(range(n))
    return [every - c if 0 in c else c for c in clades(joins, n)]


def reference_bootstrap(rows, G, joins, R, seed):
    """rows: integers (rows_as_ints); joins: the rated tree's (left, right)
    pairs.  Returns (support list [J], rep_joins [R] lists of (left, right),
    rep_dist [R] matrices)."""
    L = len(rows)
    rated = splits(joins, G)
    assert len(set(rated)) == len(rated)
    support = [0] * len(rated)
    rep_joins, rep_dist = [], []
    for b in range(R):
        drawn = [rows[draw(seed, b, t, L)] for t in range(L)]
        d = hamming_by_counting(drawn, G)
        rj = [(a, c) for a, c, _, _ in reference_nj(d)[0]]
        rep_dist.append(d)
        rep_joins.append(rj)
        mine = splits(rj, G)
        assert len(set(mine)) == len(mine)
        for t, s in enumerate(rated):
            if s in mine:
                support[t] += 1
    return support, rep_joins, rep_dist


# ------------------------------------------------------------------ inputs
def pack_rows(u):
    """A 0 / 1 table [L, G] -> uint64 [L, W] presence words."""
    u = np.asarray(u, np.uint8)
    L, G = u.shape
    W = (G + 63) // 64
    full = np.zeros((L, W * 64), np.uint8)
    full[:, :G] = u
    return np.packbits(full, axis=1, bitorder="little").view(np.uint64).reshape(L, W)


def coin_table(L, G, seed=0, p=0.5):
    rng = np.random.default_rng([seed, L, G])
    return pack_rows(rng.random((L, G)) < p)


def clean_table(n, per, seed=0):
    """A random unrooted binary tree of n leaves as presence rows: every
    clade of the tree is backed by `per` identical labels and every leaf by
    `per` private ones, so the Hamming distances are `per` times the tree's
    path lengths in edges.  The rows are shuffled."""
    rng = np.random.default_rng([seed, n, per])
    groups = [[i] for i in range(n)]
    rows = [[i] for i in range(n)]
    while len(groups) > 3:
        a, b = sorted(rng.choice(len(groups), 2, replace=False).tolist())
        merged = groups[a] + groups[b]
        groups = [x for k, x in enumerate(groups) if k not in (a, b)] + [merged]
        rows.append(merged)
    u = np.zeros((len(rows) * per, n), np.uint8)
    for k, members in enumerate(rows):
        u[k * per:(k + 1) * per, members] = 1
    return pack_rows(u[rng.permutation(u.shape[0])])


def mixed_table(seed=0):
    """The clean 20-leaf table at 3 labels per clade with 150 coin-flip rows appended."""
    return np.concatenate([clean_table(20, 3, seed), coin_table(150, 20, seed)])


def star_table(G, L=40):
    """Rows that are in every genome or in none: every replicate distance is
    equal (0), whatever is drawn, so the tie rule alone decides every tree."""
    u = np.zeros((L, G), np.uint8)
    u[::2] = 1
    return pack_rows(u)


def table_dist(bits, G):
    """The Hamming matrix of a table, uint64 [G, G] (exact in float64)."""
    W = (G + 63) // 64
    b = np.asarray(bits, np.uint64).reshape(-1, W)
    u = np.unpackbits(b.view(np.uint8).reshape(b.shape[0], W * 8), axis=1, bitorder="little")[:, :G].astype(np.float64)
    s = u.T @ u
    dg = np.diag(s)
    return (dg[:, None] + dg[None, :] - 2 * s).astype(np.uint64)


# ------------------------------------------------------------------ Newick
def parse_newick_labels(text):
    """A Newick text whose inner nodes may carry a label between `)` and `:`
    -> (edges, leaves, labels): edges (parent, child, length text) over node
    numbers in order of appearance (the root is 0), leaves {node: name},
    labels {inner node: label text} for the labelled ones.  Names may be
    quoted in single quotes, an inner quote doubled."""
    if isinstance(text, bytes):
        text = text.decode()
    assert text.endswith(";\n"), text[-10:]
    pos = 0
    edges, leaves, labels, edge_to = [], {}, {}, {}

    def name():
        nonlocal pos
        if text[pos] == "'":
            out = []
            pos += 1
            while True:
                if text[pos] == "'":
                    if text[pos + 1] == "'":
                        out.append("'")
                        pos += 2
                        continue
                    pos += 1
                    return "".join(out)
                out.append(text[pos])
                pos += 1
        st = pos
        while text[pos] not in "():,;":
            pos += 1
        return text[st:pos]

    def length():
        nonlocal pos
        assert text[pos] == ":", (pos, text[pos])
        pos += 1
        st = pos
        while text[pos] not in "(),;":
            pos += 1
        return text[st:pos]
    assert text[pos] == "("
    stack, count = [0], 1
    pos += 1
    while stack:
        if text[pos] == "(":
            edges.append([stack[-1], count, None])
            edge_to[count] = edges[-1]
            stack.append(count)
            count += 1
            pos += 1
            continue
        if text[pos] == ")":
            me = stack.pop()
            pos += 1
            lab = name()
            if lab:
                labels[me] = lab
            if not stack:
                break
            edge_to[me][2] = length()
        else:
            leaves[count] = name()
            edges.append([stack[-1], count, length()])
            count += 1
        if text[pos] == ",":
            pos += 1
    assert text[pos:] == ";\n", text[pos:]
    return [tuple(e) for e in edges], leaves, labels


def labels_by_clade(text):
    """{frozenset of leaf names below an inner non-root node: (its label or
    None, its length text)} of a Newick text."""
    edges, leaves, labels = parse_newick_labels(text)
    kids, length = {}, {}
    for a, b, w in edges:
        kids.setdefault(a, []).append(b)
        length[b] = w
    below, out = {}, {}
    for x in reversed([b for _, b, _ in edges]):             # (children appear after their parents)
        below[x] = frozenset([leaves[x]]) if x in leaves else frozenset().union(*[below[k] for k in kids[x]])
        if x not in leaves:
            out[below[x]] = (labels.get(x), length[x])
    return out
