"""Expected `.mcl` files of the built-in clusterer (tests/golden/cc/*.mcl.gz).

Independent of the package: the graph of a fixture's `rdbg_weight.xyz.gz` is
built with networkx as the reference's other/test_net.py builds it (one node
per `<key>_<value>` token, one edge per line), keeping only edges of weight
>= W but every node, and networkx.connected_components gives the clusters.
They are then written in the order the clusterer documents: clusters by size
descending, ties by the first appearance of their earliest node in the .xyz
(token 0, then token 1 of each line, in file order); members by that first
appearance; one line per cluster, tab-separated.

Run from the repository root:  python tests/golden/make_cc_goldens.py
"""
import gzip
import os
import sys

try:
    import networkx as nx
except ImportError:
    sys.exit("make_cc_goldens.py needs networkx (it is the independent reference of these fixtures)")

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("pan8_k27_c3", 1), ("pan8_k27_c3", 4), ("pan8_k27_c2", 2), ("pan8_k15", 4), ("edge_k27", 1),
         ("edge_k27", 2), ("polya_k27", 1), ("edge_k5", 1), ("test_k27", 1)]


def cc_text(xyz: str, w: int) -> str:
    g = nx.Graph()
    first = {}
    for line in xyz.splitlines():
        j, k, cnt = line.split("\t")[:3]
        for tok in (j, k):
            first.setdefault(tok, len(first))
            g.add_node(tok)
        if int(cnt) >= w:
            g.add_edge(j, k)
    comps = [sorted(c, key=first.__getitem__) for c in nx.connected_components(g)]
    comps.sort(key=lambda c: (-len(c), first[c[0]]))
    return "".join("\t".join(c) + "\n" for c in comps)


def main():
    out = os.path.join(HERE, "cc")
    os.makedirs(out, exist_ok=True)
    for name, w in CASES:
        xyz = gzip.open(os.path.join(HERE, name, "rdbg_weight.xyz.gz")).read().decode()
        text = cc_text(xyz, w)
        with open(os.path.join(out, "%s_w%d.mcl.gz" % (name, w)), "wb") as f:
            with gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as z:
                z.write(text.encode())
        lines = text.splitlines()
        sizes = sorted((l.count("\t") + 1 for l in lines), reverse=True)
        print("%s W=%d: %d clusters, %d with more than one node, largest %s"
              % (name, w, len(lines), sum(s > 1 for s in sizes), sizes[:5]))


if __name__ == "__main__":
    main()
