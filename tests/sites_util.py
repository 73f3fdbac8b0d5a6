"""An independent reference of the variable sites for the tests: plain Python
dicts and lists (nothing shared with pangenome_amd/), the text, and the
comparison every test uses.

Definition (stated here on its own, not copied from include/pangenome.h):
a row (record, start, end, strand, label) is used iff label >= 0 and its
record has a genome.  A run is a maximal stretch of consecutive used rows of
one record and strand.  Inside a run every two neighbours (a, c) are a direct
record of the flank pair (a, c) with via -1 and length 0, and every three
neighbours (a, x, c) a via record of the flank pair (a, c) with via x and the
length |end - start| of the middle row.  An allele of a flank pair is a
distinct via; a site is a flank pair with two alleles or more."""
import json
import os

import numpy as np

from golden_util import GOLDEN

HEADER = "#from\tto\tvia\tcount\tgenomes\tmin\tmax\n"
SITE_COLS = ("site_from", "site_to", "site_alleles", "site_first", "site_count", "site_genomes")
ALLELE_COLS = ("allele_site", "allele_via", "allele_count", "allele_genomes", "allele_min", "allele_max")
GENOME_COLS = ("genome_sites", "genome_alleles", "genome_private")
DTYPES = dict(site_from=np.int64, site_to=np.int64, site_alleles=np.uint32, site_first=np.uint64,
              site_count=np.uint64, site_genomes=np.uint32, allele_site=np.uint64, allele_via=np.int64,
              allele_count=np.uint64, allele_genomes=np.uint32, allele_min=np.uint64, allele_max=np.uint64,
              genome_sites=np.uint64, genome_alleles=np.uint64, genome_private=np.uint64)


def reference_sites(rows5, rec_group, G):
    """The three tables and the counts as plain lists; "bits" is a list of W
    Python ints per allele, "pairs" the flank pairs with any record."""
    rows = np.asarray(rows5, np.int64).reshape(-1, 5).tolist()
    grp = [int(x) for x in np.asarray(rec_group).reshape(-1).tolist()]
    assert all(-1 <= g < G for g in grp)
    runs, skipped, prev = [], 0, None
    for rec, s, e, strand, lab in rows:
        if lab < 0 or grp[rec] < 0:
            skipped += 1
            prev = None
            continue
        if prev != (rec, strand):
            runs.append((grp[rec], []))
            prev = (rec, strand)
        runs[-1][1].append((lab, abs(e - s)))
    pairs, n_records = {}, 0                             # (a, c) -> via -> [count, genomes, min, max]
    for g, steps in runs:
        recs = [(steps[i][0], steps[i + 1][0], -1, 0) for i in range(len(steps) - 1)]
        recs += [(steps[i][0], steps[i + 2][0], steps[i + 1][0], steps[i + 1][1]) for i in range(len(steps) - 2)]
        n_records += len(recs)
        for a, c, via, ln in recs:
            al = pairs.setdefault((a, c), {}).setdefault(via, [0, set(), ln, ln])
            al[0] += 1
            al[1].add(g)
            al[2], al[3] = min(al[2], ln), max(al[3], ln)
    W = (G + 63) // 64
    ref = {k: [] for k in SITE_COLS + ALLELE_COLS}
    ref.update(n_skipped=skipped, n_records=n_records, n_runs=len(runs), pairs=len(pairs), bits=[],
               genome_sites=[0] * G, genome_alleles=[0] * G, genome_private=[0] * G)
    for (a, c) in sorted(pairs):
        alleles = pairs[(a, c)]
        if len(alleles) < 2:
            continue
        site, everyone = len(ref["site_from"]), set()
        ref["site_from"].append(a)
        ref["site_to"].append(c)
        ref["site_alleles"].append(len(alleles))
        ref["site_first"].append(len(ref["allele_via"]))
        ref["site_count"].append(sum(v[0] for v in alleles.values()))
        for via in sorted(alleles):
            count, genomes, lo, hi = alleles[via]
            everyone |= genomes
            ref["allele_site"].append(site)
            ref["allele_via"].append(via)
            ref["allele_count"].append(count)
            ref["allele_genomes"].append(len(genomes))
            ref["allele_min"].append(lo)
            ref["allele_max"].append(hi)
            mask = sum(1 << g for g in genomes)
            ref["bits"].append([(mask >> (64 * w)) & (2 ** 64 - 1) for w in range(W)])
            for g in genomes:
                ref["genome_alleles"][g] += 1
                if len(genomes) == 1:
                    ref["genome_private"][g] += 1
        ref["site_genomes"].append(len(everyone))
        for g in everyone:
            ref["genome_sites"][g] += 1
    return ref


def reference_text(ref):
    out = [HEADER]
    for site, via, count, genomes, lo, hi in zip(*[ref[k] for k in ALLELE_COLS]):
        out.append("%d\t%d\t%s\t%d\t%d\t%d\t%d\n" % (ref["site_from"][site], ref["site_to"][site],
                                                   "*" if via < 0 else "%d" % via, count, genomes, lo, hi))
    return "".join(out)


def device_tables(ctx):
    """The three exports of the context's sites as one dict of arrays."""
    t = ctx.region_sites_table()
    t.update(ctx.region_sites_alleles())
    t.update(ctx.region_sites_groups())
    return t


def assert_same(got, ref, G):
    for k in SITE_COLS + ALLELE_COLS + GENOME_COLS:
        assert got[k].dtype == DTYPES[k] and got[k].ndim == 1, k
        assert got[k].tolist() == ref[k], k
    assert got["bits"].dtype == np.uint64 and got["bits"].shape == (len(ref["allele_via"]), (G + 63) // 64)
    assert got["bits"].tolist() == ref["bits"]


def check_device(ctx, rows, rec_group, G, rows_on_device=False):
    """region_sites() on the device against reference_sites, exactly: the four
    returned counts, the three exports with the bits, and the text byte for
    byte.  Returns (ref, text)."""
    ref = reference_sites(rows, rec_group, G)
    counts = ctx.region_sites(rec_group, G, rows=None if rows_on_device else rows)
    assert counts == (len(ref["site_from"]), len(ref["allele_via"]), ref["n_records"], ref["n_skipped"])
    assert_same(device_tables(ctx), ref, G)
    text = ctx.region_sites_text()
    assert text.decode() == reference_text(ref)
    return ref, text


def summary(ref):
    """The figures tests/golden/sites/*.json record."""
    n = ref["site_alleles"]
    direct = {s for s, v in zip(ref["allele_site"], ref["allele_via"]) if v < 0}
    return {"n_paths": ref["n_runs"], "n_pairs": ref["pairs"], "n_sites": len(n),
            "sites_2_alleles": sum(1 for x in n if x == 2), "sites_3_alleles": sum(1 for x in n if x == 3),
            "sites_4_alleles": sum(1 for x in n if x == 4), "n_alleles": len(ref["allele_via"]),
            "sites_with_direct": len(direct), "sites_in_2_genomes": sum(1 for g in ref["site_genomes"] if g >= 2)}


def golden(name):
    return json.load(open(os.path.join(GOLDEN, "sites", name + ".json")))


def files_of(ref, genome_names):
    """The two text files of `-v`; genome_names as bytes."""
    genomes = b"#genome\tsites\talleles\tprivate\n" + b"".join(
        b"%s\t%d\t%d\t%d\n" % x for x in zip(genome_names, *[ref[k] for k in GENOME_COLS]))
    return {"_fr_sites.tsv": reference_text(ref).encode(), "_fr_sites_genomes.tsv": genomes}


def assert_files(prefix, ref, genome_names):
    G = len(genome_names)
    for suffix, want in files_of(ref, [x.encode() for x in genome_names]).items():
        assert open(prefix + suffix, "rb").read() == want, suffix
    z = np.load(prefix + "_fr_sites.npz")
    assert sorted(z.files) == sorted(SITE_COLS + ALLELE_COLS + GENOME_COLS + ("bits", "genomes"))
    assert_same(z, ref, G)
    assert [x.decode() for x in z["genomes"].tolist()] == list(genome_names)
    assert not [f for f in os.listdir(os.path.dirname(prefix)) if f.endswith(".tmp")]
