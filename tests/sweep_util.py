"""An independent reference of the cluster curve for the tests: one dict-based
union-find over `<key>_<value>` tokens per threshold, each from scratch
(nothing shared with pangenome_amd/, nothing kept from level to level), and
the committed expectation tests/golden/cc/pan8_k27_c3_sweep.json."""
import json
import os

import numpy as np

from golden_util import GOLDEN

COLUMNS = ("w", "edges", "clusters", "largest", "singletons")


def reference_sweep(tuples, counts, thresholds):
    """The rows the sweep must give for these edges: a dict of lists."""
    edges = list(zip(np.asarray(tuples, np.uint64).reshape(-1, 4).tolist(), np.asarray(counts).tolist()))
    out = {k: [] for k in COLUMNS}
    for w in [int(x) for x in thresholds]:
        parent = {}

        def root(x):
            r = x
            while parent[r] != r:
                r = parent[r]
            while parent[x] != r:                        # compress the path walked
                parent[x], x = r, parent[x]
            return r
        kept = 0
        for (a, b, c, d), n in edges:
            s, t = "%d_%d" % (a, b), "%d_%d" % (c, d)
            parent.setdefault(s, s)
            parent.setdefault(t, t)
            if n >= w:
                kept += 1
                rs, rt = root(s), root(t)
                if rs != rt:
                    parent[rs] = rt
        sizes = {}
        for tok in parent:
            r = root(tok)
            sizes[r] = sizes.get(r, 0) + 1
        out["w"].append(w)
        out["edges"].append(kept)
        out["clusters"].append(len(sizes))
        out["largest"].append(max(sizes.values(), default=0))
        out["singletons"].append(sum(1 for v in sizes.values() if v == 1))
    return out


def as_lists(table):
    """A sweep result (dict of arrays or lists) as plain lists of ints."""
    return {k: [int(x) for x in np.asarray(table[k]).tolist()] for k in COLUMNS}


def golden_sweep():
    """pan8_k27_c3's curve over thresholds 1..8, as committed."""
    with open(os.path.join(GOLDEN, "cc", "pan8_k27_c3_sweep.json")) as f:
        return json.load(f)


def sweep_file_text(table, chosen):
    """The bytes of `<in>_rdbg_weight.xyz.sweep.tsv` for these rows."""
    t = as_lists(table)
    lines = ["#w\tedges\tclusters\tlargest\tsingletons\tmulti\n"]
    for i in range(len(t["w"])):
        row = [t[k][i] for k in COLUMNS] + [t["clusters"][i] - t["singletons"][i]]
        lines.append("\t".join(str(x) for x in row) + "\n")
    lines.append("#auto\t%d\n" % chosen)
    return "".join(lines)
