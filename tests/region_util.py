"""An independent reference of the region graph for the tests: plain Python
dicts and lists (nothing shared with pangenome_amd/), its two texts, and the
comparison every test uses."""
import json
import os

import numpy as np

from golden_util import GOLDEN

LINKS_HEADER = "#from\tto\tcount\tgenomes\n"
GFA_HEADER = "H\tVN:Z:1.0\n"
NODE_COLS = ("labels", "rows", "max_len", "n_out", "n_in")
LINK_COLS = ("link_from", "link_to", "link_count", "link_genomes")
PATH_COLS = ("path_record", "path_strand", "path_lo", "path_hi", "path_steps")
DTYPES = dict(labels=np.int64, rows=np.uint64, max_len=np.uint64, n_out=np.uint32, n_in=np.uint32,
              link_from=np.int64, link_to=np.int64, link_count=np.uint64, link_genomes=np.uint32,
              path_record=np.int64, path_strand=np.int64, path_lo=np.int64, path_hi=np.int64, path_steps=np.uint64)


def reference_region(rows5, rec_group, G):
    """Nodes, links, paths and counts as plain lists.  A row is used iff its
    label >= 0 and its record has a genome; a run is a maximal stretch of
    consecutive used rows of one record and strand; a link is two adjacent
    rows of a run."""
    rows = np.asarray(rows5, np.int64).reshape(-1, 5).tolist()
    grp = [int(x) for x in np.asarray(rec_group).reshape(-1).tolist()]
    assert all(-1 <= g < G for g in grp)
    nodes, links, paths, skipped = {}, {}, [], 0
    run = None                                           # the path the previous row belongs to, if it was used
    for rec, s, e, strand, lab in rows:
        g = grp[rec]
        if lab < 0 or g < 0:
            skipped += 1
            run = None
            continue
        nd = nodes.setdefault(lab, [0, 0])
        nd[0] += 1
        nd[1] = max(nd[1], abs(e - s))
        if run is not None and run["record"] == rec and run["strand"] == strand:
            lk = links.setdefault((run["labels"][-1], lab), [0, set()])
            lk[0] += 1
            lk[1].add(g)
            run["labels"].append(lab)
            run["last"] = (s, e)
        else:
            run = {"record": rec, "strand": strand, "first": (s, e), "last": (s, e), "labels": [lab]}
            paths.append(run)
    labels, pairs = sorted(nodes), sorted(links)
    return {"n_skipped": skipped, "labels": labels,
            "rows": [nodes[l][0] for l in labels], "max_len": [nodes[l][1] for l in labels],
            "n_out": _degree(labels, pairs, 0), "n_in": _degree(labels, pairs, 1),
            "link_from": [a for a, b in pairs], "link_to": [b for a, b in pairs],
            "link_count": [links[p][0] for p in pairs], "link_genomes": [len(links[p][1]) for p in pairs],
            "path_record": [p["record"] for p in paths], "path_strand": [p["strand"] for p in paths],
            "path_lo": [min(p["first"][0], p["last"][0]) for p in paths],
            "path_hi": [max(p["first"][1], p["last"][1]) for p in paths],
            "path_steps": [len(p["labels"]) for p in paths], "path_labels": [p["labels"] for p in paths]}


def _degree(labels, pairs, end):
    """Per label the distinct links that leave (end 0) or enter (end 1) it."""
    d = {}
    for p in pairs:
        d[p[end]] = d.get(p[end], 0) + 1
    return [d.get(l, 0) for l in labels]


def reference_links_text(ref):
    return LINKS_HEADER + "".join("%d\t%d\t%d\t%d\n" % x for x in zip(*[ref[k] for k in LINK_COLS]))


def reference_gfa(ref, names):
    """The GFA 1 text (bytes: a record's name is copied verbatim)."""
    out = [GFA_HEADER.encode()]
    out += [b"S\t%d\t*\tLN:i:%d\n" % (l, m) for l, m in zip(ref["labels"], ref["max_len"])]
    out += [b"L\t%d\t+\t%d\t+\t0M\tRC:i:%d\tgn:i:%d\n" % x for x in zip(*[ref[k] for k in LINK_COLS])]
    for rec, strand, lo, hi, labs in zip(ref["path_record"], ref["path_strand"], ref["path_lo"], ref["path_hi"],
                                         ref["path_labels"]):
        out.append(b"P\t%s:%d-%d:%s\t%s\t*\n" % (bytes(names[rec]), lo, hi, b"+" if strand == 1 else b"-",
                                                 ",".join("%d+" % l for l in labs).encode()))
    return b"".join(out)


def device_tables(ctx):
    """The three exports of the context's graph as one dict of arrays."""
    t = ctx.region_nodes()
    t.update(ctx.region_links())
    t.update(ctx.region_paths())
    return t


def assert_same(got, ref):
    for k in NODE_COLS + LINK_COLS + PATH_COLS:
        assert got[k].dtype == DTYPES[k] and got[k].ndim == 1, k
        assert got[k].tolist() == ref[k], k


def check_device(ctx, rows, rec_group, G, names, rows_on_device=False):
    """region_graph() on the device against reference_region, exactly: the
    four returned counts, the three exports and both texts.  Returns (ref,
    links text, GFA text)."""
    ref = reference_region(rows, rec_group, G)
    counts = ctx.region_graph(rec_group, G, rows=None if rows_on_device else rows)
    assert counts == (len(ref["labels"]), len(ref["link_from"]), len(ref["path_record"]), ref["n_skipped"])
    assert_same(device_tables(ctx), ref)
    text = ctx.region_links_text()
    assert text.decode() == reference_links_text(ref)
    gfa = ctx.region_gfa_text(names)
    assert gfa == reference_gfa(ref, names)
    return ref, text, gfa


def summary(ref):
    """The figures tests/golden/region/*.json record."""
    pairs = set(zip(ref["link_from"], ref["link_to"]))
    return {"n_rows": sum(ref["rows"]), "n_paths": len(ref["path_record"]), "n_nodes": len(ref["labels"]),
            "n_links": len(pairs), "n_pairs": sum(ref["link_count"]), "max_count": max(ref["link_count"], default=0),
            "max_out": max(ref["n_out"], default=0), "max_in": max(ref["n_in"], default=0),
            "links_one_genome": sum(1 for g in ref["link_genomes"] if g == 1),
            "links_with_reverse": sum(1 for a, b in pairs if a != b and (b, a) in pairs),
            "self_links": sum(1 for a, b in pairs if a == b)}


def golden(name):
    return json.load(open(os.path.join(GOLDEN, "region", name + ".json")))


def files_of(ref, names):
    """The three text files of a graph (as `-l` writes them); names[r] = record r's seqid."""
    nodes = "#label\trows\tmax\tout\tin\n" + "".join("%d\t%d\t%d\t%d\t%d\n" % x for x in zip(*[ref[k] for k in NODE_COLS]))
    return {"_fr_links.tsv": reference_links_text(ref).encode(), "_fr_nodes.tsv": nodes.encode(),
            "_fr_graph.gfa": reference_gfa(ref, names)}


def assert_files(prefix, ref, names, genome_names):
    for suffix, want in files_of(ref, names).items():
        assert open(prefix + suffix, "rb").read() == want, suffix
    z = np.load(prefix + "_fr_graph.npz")
    assert sorted(z.files) == sorted(NODE_COLS + LINK_COLS + PATH_COLS + ("genomes",))
    assert_same(z, ref)
    assert [x.decode() for x in z["genomes"].tolist()] == list(genome_names)
    assert not [f for f in os.listdir(os.path.dirname(prefix)) if f.endswith(".tmp")]
