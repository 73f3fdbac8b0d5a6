"""An independent reference of the built-in clusterer for the tests: a
dict-based union-find over `<key>_<value>` tokens (nothing shared with
pangenome_amd/host.py), and helpers to read the committed expectations
(tests/golden/cc/*.mcl.gz, made by tests/golden/make_cc_goldens.py)."""
import glob
import gzip
import os

import numpy as np

from golden_util import GOLDEN


def reference_mcl(tuples, counts, w):
    """The `.mcl` text the clusterer must write for these edges at threshold w."""
    first, parent = {}, {}

    def root(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:                        # compress the path walked
            parent[x], x = r, parent[x]
        return r
    for (a, b, c, d), n in zip(np.asarray(tuples, np.uint64).reshape(-1, 4).tolist(), np.asarray(counts).tolist()):
        s, t = "%d_%d" % (a, b), "%d_%d" % (c, d)
        for tok in (s, t):
            if tok not in first:
                first[tok] = len(first)
                parent[tok] = tok
        if n >= w:
            rs, rt = root(s), root(t)
            if rs != rt:
                parent[rs] = rt
    groups = {}
    for tok in first:                                # (first-appearance order: members come sorted)
        groups.setdefault(root(tok), []).append(tok)
    order = sorted(groups.values(), key=lambda m: (-len(m), first[m[0]]))
    return "".join("\t".join(m) + "\n" for m in order)


def cc_cases():
    """(fixture name, W) of every committed expectation."""
    out = []
    for p in sorted(glob.glob(os.path.join(GOLDEN, "cc", "*.mcl.gz"))):
        name, w = os.path.basename(p)[:-len(".mcl.gz")].rsplit("_w", 1)
        out.append((name, int(w)))
    return out


def cc_text(name, w):
    return gzip.open(os.path.join(GOLDEN, "cc", "%s_w%d.mcl.gz" % (name, w))).read().decode()


def xyz_arrays(xyz_text):
    """(tuples uint64 [n, 4], counts int64 [n]) of a `.xyz` text."""
    t, c = [], []
    for line in xyz_text.splitlines():
        j, k, n = line.split("\t")
        t.append([int(x) for x in j.split("_") + k.split("_")])
        c.append(int(n))
    return np.array(t, np.uint64).reshape(-1, 4), np.array(c, np.int64)


def random_graph(seed, U, E, wmax=5):
    """E random edges over U nodes (64-bit keys, small values), weights 1..wmax."""
    rng = np.random.default_rng(seed)
    nodes = np.stack([rng.integers(0, 2 ** 63, U, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
                      rng.integers(0, 4096, U, dtype=np.uint64)], axis=1)
    e = rng.integers(0, U, (E, 2))
    return np.concatenate([nodes[e[:, 0]], nodes[e[:, 1]]], axis=1), rng.integers(1, wmax + 1, E).astype(np.int64)
