"""An independent reference for the genome tree (pg_tree_nj, host.tree_nj):
the loops of the definition in include/pangenome.h, "genome tree", on Python
integers; nothing of pangenome_amd.host is imported.  Also the inputs the tree
tests share (random Hamming matrices, random additive trees) and a small
Newick parser."""
import numpy as np

S = 16
ONE = 1 << S


def reference_nj(dist):
    """(joins, root) of the definition: joins a list of (left, right, left_len,
    right_len), root a list of (child, len)."""
    n = len(dist)
    D = [[int(dist[i][j]) << S for j in range(n)] for i in range(n)]
    node = list(range(n))
    live = list(range(n))
    joins = []
    while len(live) > 3:
        m = len(live)
        r = {i: sum(D[i][k] for k in live) for i in live}
        best = None
        for a in range(m):
            for b in range(a + 1, m):
                i, j = live[a], live[b]
                q = (m - 2) * D[i][j] - r[i] - r[j]
                if best is None or q < best[0]:               # (ascending (i, j): the first of equal Q stays)
                    best = (q, i, j)
        _, i, j = best
        dij = D[i][j]
        li = (dij + (r[i] - r[j]) // (m - 2)) >> 1
        li = min(max(li, 0), dij)
        joins.append((node[i], node[j], li, dij - li))
        for k in live:
            if k != i and k != j:
                D[i][k] = D[k][i] = max(0, (D[i][k] + D[j][k] - dij) >> 1)
        node[i] = n + len(joins) - 1
        live.remove(j)
    if len(live) == 3:
        a, b, c = live
        root = [(node[a], max(0, (D[a][b] + D[a][c] - D[b][c]) >> 1)),
                (node[b], max(0, (D[a][b] + D[b][c] - D[a][c]) >> 1)),
                (node[c], max(0, (D[a][c] + D[b][c] - D[a][b]) >> 1))]
    elif len(live) == 2:
        a, b = live
        root = [(node[a], D[a][b] >> 1), (node[b], D[a][b] - (D[a][b] >> 1))]
    else:
        root = [(node[a], 0) for a in live]
    return joins, root


def as_lists(joins, root):
    """The tables of host.tree_nj or of the device (dict of arrays, (child,
    len)) in reference_nj's form."""
    return ([tuple(int(x) for x in row) for row in zip(joins["left"], joins["right"], joins["left_len"],
                                                        joins["right_len"])],
            [(int(c), int(v)) for c, v in zip(*root)])


def hamming(n, labels=300, p=0.4, seed=0):
    """The Hamming distances of n random presence columns, uint64 [n, n]:
    `labels` labels, each in a genome with probability p."""
    rng = np.random.default_rng([seed, n, labels])
    b = (rng.random((labels, n)) < p).astype(np.float64)
    s = (b.T @ b).astype(np.int64)                           # (counts below 2^53: exact)
    dg = np.diag(s)
    return (dg[:, None] + dg[None, :] - 2 * s).astype(np.uint64)


def star(n, v=2):
    d = np.full((n, n), v, np.uint64)
    np.fill_diagonal(d, 0)
    return d


def additive(n, seed=0):
    """A random unrooted binary tree of n >= 3 leaves with integer edges 1 .. 9:
    (dist uint64 [n, n] between the leaves, the sum of the edges)."""
    rng = np.random.default_rng([seed, n])
    # grow it: start from a star of three leaves, then split a random edge for every next leaf
    edges = [[n, 0, int(rng.integers(1, 10))], [n, 1, int(rng.integers(1, 10))], [n, 2, int(rng.integers(1, 10))]]
    nxt = n + 1
    for leaf in range(3, n):
        e = edges[int(rng.integers(0, len(edges)))]
        b = e[1]
        e[1], e[2] = nxt, int(rng.integers(1, 10))           # a - nxt, nxt - b, nxt - leaf
        edges.append([nxt, b, int(rng.integers(1, 10))])
        edges.append([nxt, leaf, int(rng.integers(1, 10))])
        nxt += 1
    perm = rng.permutation(n)                                # (the leaves in no order of growth)
    edges = [[int(perm[a]) if a < n else a, int(perm[b]) if b < n else b, w] for a, b, w in edges]
    return tree_dist(edges, n), sum(w for _, _, w in edges)


def tree_dist(edges, n):
    """Leaf-to-leaf path lengths, uint64 [n, n], of an edge list (a, b, w)
    whose leaves are 0 .. n - 1."""
    adj = {}
    for a, b, w in edges:
        adj.setdefault(a, []).append((b, w))
        adj.setdefault(b, []).append((a, w))
    d = np.zeros((n, n), np.uint64)
    for s in range(n):
        seen, stack = {s: 0}, [s]
        while stack:
            x = stack.pop()
            for y, w in adj.get(x, ()):
                if y not in seen:
                    seen[y] = seen[x] + w
                    stack.append(y)
        for t in range(n):
            d[s, t] = seen[t]
    return d


def parse_newick(text):
    """A Newick text -> (edges, leaves): edges a list of (parent, child,
    length text) over node numbers in order of appearance (the root is 0),
    leaves {node: name}.  Names may be quoted in single quotes, an inner
    quote doubled."""
    if isinstance(text, bytes):
        text = text.decode()
    assert text.endswith(";\n"), text[-10:]
    pos, count = 0, 0
    edges, leaves, edge_to = [], {}, {}

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
    # (no recursion: a comb is as deep as it is long)
    assert text[pos] == "("
    stack = [0]
    count = 1
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
    return [tuple(e) for e in edges], leaves


def length_value(text):
    """`<int>.<six digits>` as a multiple of 10^-6."""
    a, b = text.split(".")
    assert len(b) == 6
    return int(a) * 1000000 + int(b)


def newick_leaf_dist(text, names):
    """The leaf-to-leaf path lengths read back from a Newick text, in units
    of 10^-6, uint64 [n, n] in the order of names."""
    edges, leaves = parse_newick(text)
    idx = {nm: i for i, nm in enumerate(names)}
    n = len(names)
    assert sorted(leaves.values()) == sorted(names)
    ren = {node: idx[nm] for node, nm in leaves.items()}
    e2 = [(ren.get(a, a + n), ren.get(b, b + n), length_value(w)) for a, b, w in edges]
    return tree_dist(e2, n)


def joins_of_newick(text, names):
    """The tree of a Newick text as a set of leaf-name sets, one per internal
    non-root node (what joins it names, whatever their order)."""
    edges, leaves = parse_newick(text)
    kids = {}
    for a, b, _ in edges:
        kids.setdefault(a, []).append(b)
    out = set()
    order = [b for _, b, _ in edges]
    below = {}
    for x in reversed(order):                                # (children appear after their parents)
        below[x] = frozenset([leaves[x]]) if x in leaves else frozenset().union(*[below[k] for k in kids[x]])
        if x not in leaves:
            out.add(below[x])
    return out


def joins_as_sets(names, joins, n):
    """The same sets from a join table (rows of left, right, ..)."""
    below = {i: frozenset([names[i]]) for i in range(n)}
    out = set()
    for t, row in enumerate(joins):
        below[n + t] = below[int(row[0])] | below[int(row[1])]
        out.add(below[n + t])
    return out
