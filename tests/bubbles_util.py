"""An independent reference of the variable sites between anchor regions for
the tests: plain Python dicts and lists (nothing shared with pangenome_amd/),
the text, and the comparison every test uses.

Definition (stated here on its own, not copied from include/pangenome.h):
a row (record, start, end, strand, label) is used iff label >= 0 and its
record has a genome.  A run is a maximal stretch of consecutive used rows of
one record and strand.  A label is an anchor when its used rows lie in at
least min_genomes distinct genomes.  Inside a run, two anchor rows with no
anchor row between them bound a segment: flanks (a, c) = their labels in walk
order, inner path = the labels of the rows strictly between them (possibly
none), bp = the sum of |end - start| of those rows, genome = the record's.
An allele of a flank pair is a distinct inner path; a site is a flank pair
with two alleles or more.  Alleles are listed by site and, inside a site, by
the row index of the `a` row of their earliest segment."""
import json
import os

import numpy as np

from golden_util import GOLDEN

HEADER = "#from\tto\tinner\tregions\tcount\tgenomes\tmin\tmax\n"
COUNTS = ("n_anchors", "n_segments", "n_sites", "n_alleles", "n_skipped")
SITE_COLS = ("site_from", "site_to", "site_alleles", "site_first", "site_count", "site_genomes")
ALLELE_COLS = ("allele_site", "allele_regions", "allele_first_row", "allele_count", "allele_genomes", "allele_min_bp",
               "allele_max_bp", "allele_inner_off")
GENOME_COLS = ("genome_sites", "genome_alleles", "genome_private")
ANCHOR_COLS = ("anchors", "anchor_genomes")
DTYPES = dict(site_from=np.int64, site_to=np.int64, site_alleles=np.uint32, site_first=np.uint64,
              site_count=np.uint64, site_genomes=np.uint32, allele_site=np.uint64, allele_regions=np.uint64,
              allele_first_row=np.uint64, allele_count=np.uint64, allele_genomes=np.uint32, allele_min_bp=np.uint64,
              allele_max_bp=np.uint64, allele_inner_off=np.uint64, genome_sites=np.uint64, genome_alleles=np.uint64,
              genome_private=np.uint64, anchors=np.int64, anchor_genomes=np.uint32, inner=np.int64)
M64 = 2 ** 64 - 1


def reference_bubbles(rows5, rec_group, G, min_genomes):
    """Every table and count as plain lists; "bits" is a list of W Python ints
    per allele, "pairs" the flank pairs with any segment, "anchor_steps" the
    used rows that carry an anchor, "outside" the used rows in no segment and
    on no anchor."""
    rows = np.asarray(rows5, np.int64).reshape(-1, 5).tolist()
    grp = [int(x) for x in np.asarray(rec_group).reshape(-1).tolist()]
    assert all(-1 <= g < G for g in grp) and min_genomes >= 1
    runs, skipped, prev, where = [], 0, None, {}
    for i, (rec, s, e, strand, lab) in enumerate(rows):
        if lab < 0 or grp[rec] < 0:
            skipped += 1
            prev = None
            continue
        if prev != (rec, strand):
            runs.append((grp[rec], []))
            prev = (rec, strand)
        runs[-1][1].append((lab, abs(e - s), i))
        where.setdefault(lab, set()).add(grp[rec])
    anchors = {lab: len(gs) for lab, gs in where.items() if len(gs) >= min_genomes}
    pairs, n_segments, anchor_steps, outside = {}, 0, 0, 0       # (a, c) -> inner path -> [count, genomes, min, max, row]
    for g, steps in runs:
        at = [k for k, st in enumerate(steps) if st[0] in anchors]
        anchor_steps += len(at)
        outside += len(steps) - (at[-1] - at[0] + 1) if at else len(steps)
        for p, q in zip(at, at[1:]):
            path = tuple(st[0] for st in steps[p + 1:q])
            bp = sum(st[1] for st in steps[p + 1:q]) & M64
            n_segments += 1
            al = pairs.setdefault((steps[p][0], steps[q][0]), {}).setdefault(path, [0, set(), bp, bp, steps[p][2]])
            al[0] += 1
            al[1].add(g)
            al[2], al[3], al[4] = min(al[2], bp), max(al[3], bp), min(al[4], steps[p][2])
    W = (G + 63) // 64
    ref = {k: [] for k in SITE_COLS + ALLELE_COLS}
    ref.update(n_anchors=len(anchors), n_segments=n_segments, n_skipped=skipped, n_runs=len(runs), pairs=len(pairs),
               anchor_steps=anchor_steps, outside=outside, bits=[], inner=[], min_genomes=min_genomes,
               anchors=sorted(anchors), anchor_genomes=[anchors[a] for a in sorted(anchors)],
               genome_sites=[0] * G, genome_alleles=[0] * G, genome_private=[0] * G)
    for (a, c) in sorted(pairs):
        alleles = pairs[(a, c)]
        if len(alleles) < 2:
            continue
        site, everyone = len(ref["site_from"]), set()
        ref["site_from"].append(a)
        ref["site_to"].append(c)
        ref["site_alleles"].append(len(alleles))
        ref["site_first"].append(len(ref["allele_site"]))
        ref["site_count"].append(sum(v[0] for v in alleles.values()))
        for path in sorted(alleles, key=lambda p: alleles[p][4]):
            count, genomes, lo, hi, row = alleles[path]
            everyone |= genomes
            ref["allele_site"].append(site)
            ref["allele_regions"].append(len(path))
            ref["allele_first_row"].append(row)
            ref["allele_count"].append(count)
            ref["allele_genomes"].append(len(genomes))
            ref["allele_min_bp"].append(lo)
            ref["allele_max_bp"].append(hi)
            ref["allele_inner_off"].append(len(ref["inner"]))
            ref["inner"].extend(path)
            mask = sum(1 << g for g in genomes)
            ref["bits"].append([(mask >> (64 * w)) & M64 for w in range(W)])
            for g in genomes:
                ref["genome_alleles"][g] += 1
                if len(genomes) == 1:
                    ref["genome_private"][g] += 1
        ref["site_genomes"].append(len(everyone))
        for g in everyone:
            ref["genome_sites"][g] += 1
    ref["n_sites"], ref["n_alleles"] = len(ref["site_from"]), len(ref["allele_site"])
    return ref


def inner_of(ref, i):
    """Allele i's inner path."""
    at = ref["allele_inner_off"][i]
    return list(ref["inner"][at:at + ref["allele_regions"][i]])


def reference_text(ref):
    out = [HEADER]
    for i, site in enumerate(ref["allele_site"]):
        path = inner_of(ref, i)
        out.append("%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\n" % (
            ref["site_from"][site], ref["site_to"][site], ",".join("%d" % x for x in path) if path else "*", len(path),
            ref["allele_count"][i], ref["allele_genomes"][i], ref["allele_min_bp"][i], ref["allele_max_bp"][i]))
    return "".join(out)


def device_tables(ctx):
    """The five exports of the context's bubbles as one dict of arrays."""
    t = ctx.region_bubbles_table()
    t.update(ctx.region_bubbles_alleles())
    t["inner"] = ctx.region_bubbles_inner()
    t.update(ctx.region_bubbles_groups())
    t.update(ctx.region_bubbles_anchors())
    return t


def assert_same(got, ref, G):
    for k in SITE_COLS + ALLELE_COLS + GENOME_COLS + ANCHOR_COLS + ("inner",):
        assert got[k].dtype == DTYPES[k] and got[k].ndim == 1, k
        assert got[k].tolist() == list(ref[k]), k
    assert got["bits"].dtype == np.uint64 and got["bits"].shape == (len(ref["allele_site"]), (G + 63) // 64)
    assert got["bits"].tolist() == [list(b) for b in ref["bits"]]


def check_device(ctx, rows, rec_group, G, min_genomes, rows_on_device=False):
    """region_bubbles() on the device against reference_bubbles, exactly: the
    five returned counts, the five exports with the bits and the inner paths,
    and the text byte for byte.  Returns (ref, text)."""
    ref = reference_bubbles(rows, rec_group, G, min_genomes)
    counts = ctx.region_bubbles(rec_group, G, min_genomes, rows=None if rows_on_device else rows)
    assert tuple(counts) == tuple(ref[k] for k in COUNTS)
    assert_same(device_tables(ctx), ref, G)
    text = ctx.region_bubbles_text()
    assert text.decode() == reference_text(ref)
    return ref, text


def summary(ref):
    """The figures tests/golden/bubbles/*.json record."""
    n, reg, na = ref["site_alleles"], ref["allele_regions"], len(ref["allele_site"])
    direct = {ref["allele_site"][i] for i in range(na) if reg[i] == 0}
    long_sites = {ref["allele_site"][i] for i in range(na) if reg[i] >= 2}
    out = {"n_paths": ref["n_runs"], "n_anchors": ref["n_anchors"], "anchor_steps": ref["anchor_steps"],
           "steps_outside": ref["outside"], "n_segments": ref["n_segments"], "n_pairs": ref["pairs"],
           "n_sites": len(n), "n_alleles": na, "sites_with_direct": len(direct),
           "sites_reaching_2_regions": len(long_sites), "alleles_2_regions": sum(1 for r in reg if r >= 2),
           "longest_inner": max(reg) if reg else 0,
           "alleles_in_2_genomes": sum(1 for g in ref["allele_genomes"] if g >= 2),
           "largest_max_bp": max(ref["allele_max_bp"]) if na else 0}
    for k in range(2, 7):
        out["sites_%d_alleles" % k] = sum(1 for x in n if x == k)
    return out


def golden(name):
    return json.load(open(os.path.join(GOLDEN, "bubbles", name + ".json")))


def files_of(ref, genome_names):
    """The two text files of `-b`; genome_names as bytes."""
    genomes = b"#genome\tsites\talleles\tprivate\n" + b"".join(
        b"%s\t%d\t%d\t%d\n" % x for x in zip(genome_names, *[ref[k] for k in GENOME_COLS]))
    return {"_fr_bubbles.tsv": reference_text(ref).encode(), "_fr_bubbles_genomes.tsv": genomes}


def assert_files(prefix, ref, genome_names):
    G = len(genome_names)
    for suffix, want in files_of(ref, [x.encode() for x in genome_names]).items():
        assert open(prefix + suffix, "rb").read() == want, suffix
    z = np.load(prefix + "_fr_bubbles.npz")
    assert sorted(z.files) == sorted(SITE_COLS + ALLELE_COLS + GENOME_COLS + ANCHOR_COLS +
                                     ("inner", "bits", "genomes", "min_genomes"))
    assert_same(z, ref, G)
    assert [x.decode() for x in z["genomes"].tolist()] == list(genome_names)
    assert int(z["min_genomes"]) == ref["min_genomes"]
    assert not [f for f in os.listdir(os.path.dirname(prefix)) if f.endswith(".tmp")]
