"""An independent reference of the genome comparison for the tests: Python
sets and integers (nothing shared with pangenome_amd/host.py), a numpy form
for the larger cases, the expected file texts, and the comparisons every test
uses."""
import os

import numpy as np


def members(bits, G):
    """[n][G] 0 / 1 lists from presence words [n][W], by integer shifts."""
    rows = np.asarray(bits, np.uint64).reshape(len(bits), (G + 63) // 64).tolist()
    return [[(r[g // 64] >> (g % 64)) & 1 for g in range(G)] for r in rows]


def reference_compare(bits, G, orders):
    """(shared, pan, core) as lists of lists, from one set of labels per genome."""
    m = members(bits, G)
    sets = [{l for l, r in enumerate(m) if r[g]} for g in range(G)]
    shared = [[len(sets[g] & sets[h]) for h in range(G)] for g in range(G)]
    pan, core = [], []
    for order in np.asarray(orders).reshape(-1, G).tolist() if G else [[] for _ in orders]:
        union, inter, a, b = set(), None, [], []
        for g in order:
            union = union | sets[g]
            inter = set(sets[g]) if inter is None else inter & sets[g]
            a.append(len(union))
            b.append(len(inter))
        pan.append(a)
        core.append(b)
    return shared, pan, core


def reference_compare_fast(bits, G, orders):
    """The same for the larger cases: a float64 product for shared (exact
    below 2^53) and logical accumulates along each order for the curves."""
    b = np.asarray(bits, np.uint64).reshape(len(bits), (G + 63) // 64)
    g = np.arange(G)
    m = ((b[:, g // 64] >> (g % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)          # [n][G]
    f = m.astype(np.float64)
    shared = (f.T @ f).astype(np.uint64).tolist()
    pan, core = [], []
    for order in np.asarray(orders).reshape(-1, G):
        rows = m[:, order].T                                                                  # [G][n]
        pan.append(np.logical_or.accumulate(rows, axis=0).sum(axis=1).tolist())
        core.append(np.logical_and.accumulate(rows, axis=0).sum(axis=1).tolist())
    return shared, pan, core


def check_identities(bits, G, orders, shared, pan, core):
    """The three identities of the definitions, from the bits alone."""
    m = members(bits, G)
    any_g, all_g = sum(1 for r in m if any(r)), sum(1 for r in m if all(r))
    for p, order in enumerate(np.asarray(orders).reshape(-1, G).tolist()):
        assert pan[p][G - 1] == any_g and core[p][G - 1] == all_g
        assert pan[p][0] == core[p][0] == shared[order[0]][order[0]]
    for g in range(G):
        assert shared[g][g] == sum(r[g] for r in m)
        assert [shared[g][h] for h in range(G)] == [shared[h][g] for h in range(G)]


def random_bits(n, G, density=0.4, seed=1, ones_row=True, zeros_row=True):
    """Presence words [n][W] with each bit set with `density`; row 0 all ones
    and row n - 1 all zeros when asked (and n allows)."""
    rng = np.random.default_rng(seed)
    m = rng.random((n, G)) < density
    if ones_row and n > 0:
        m[0] = True
    if zeros_row and n > 1:
        m[n - 1] = False
    return pack(m)


def pack(m):
    """[n][G] booleans -> uint64 [n][W] presence words."""
    m = np.asarray(m, bool)
    n, G = m.shape
    W = (G + 63) // 64
    out = np.zeros((n, W), np.uint64)
    for g in range(G):
        out[:, g // 64] |= m[:, g].astype(np.uint64) << np.uint64(g % 64)
    return out


def random_orders(G, P, seed=2):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(G) for _ in range(P)]).astype(np.int32) if P else np.zeros((0, G), np.int32)


def as_lists(shared, pan, core):
    return tuple(np.asarray(x).tolist() for x in (shared, pan, core))


def files_of(names, shared, orders, pan, core):
    """The three text files `-p` writes, from lists."""
    G, P = len(names), len(orders)
    head = "#genome" + "".join("\t" + x for x in names) + "\n"
    out = {"_fr_shared.tsv": head + "".join(
        names[g] + "".join("\t%d" % shared[g][h] for h in range(G)) + "\n" for g in range(G))}
    lines = []
    for g in range(G):
        cells = []
        for h in range(G):
            u = shared[g][g] + shared[h][h] - shared[g][h]
            cells.append("0.000000" if u == 0 else "%.6f" % (1.0 - shared[g][h] / u))
        lines.append(names[g] + "".join("\t" + c for c in cells) + "\n")
    out["_fr_jaccard.tsv"] = head + "".join(lines)
    curve = "#genomes\torders\tpan_sum\tpan_min\tpan_max\tcore_sum\tcore_min\tcore_max\n"
    for i in range(G):
        a, b = [pan[p][i] for p in range(P)], [core[p][i] for p in range(P)]
        curve += "%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (i + 1, P, sum(a), min(a), max(a), sum(b), min(b), max(b))
    out["_fr_curve.tsv"] = curve
    return out


def assert_compare_files(prefix, names, shared, orders, pan, core):
    """The four `-p` files of `prefix` against lists (names: str)."""
    orders = np.asarray(orders).tolist()
    for suffix, want in files_of(names, shared, orders, pan, core).items():
        assert open(prefix + suffix).read() == want, suffix
    z = np.load(prefix + "_fr_compare.npz")
    G, P = len(names), len(orders)
    assert [x.decode() for x in z["genomes"].tolist()] == list(names)
    assert z["shared"].dtype == np.uint64 and z["shared"].shape == (G, G) and z["shared"].tolist() == shared
    assert z["orders"].dtype == np.int32 and z["orders"].shape == (P, G) and z["orders"].tolist() == orders
    for k, want in (("pan", pan), ("core", core)):
        assert z[k].dtype == np.uint64 and z[k].shape == (P, G) and z[k].tolist() == want, k
    assert not [f for f in os.listdir(os.path.dirname(prefix)) if f.endswith(".tmp")]


def fr_files(prefix):
    d, base = os.path.split(prefix)
    return sorted(f[len(base):] for f in os.listdir(d) if f.startswith(base + "_fr_"))


NEW_FILES = ["_fr_compare.npz", "_fr_curve.tsv", "_fr_jaccard.tsv", "_fr_shared.tsv"]
OLD_FILES = ["_fr_freq.tsv", "_fr_genomes.tsv", "_fr_presence.npz", "_fr_spectrum.tsv"]
