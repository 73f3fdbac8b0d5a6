"""An independent reference of the frequency table for the tests: plain
Python dicts and integers (nothing shared with pangenome_amd/host.py), its
text, and the comparison every test uses."""
import json
import os

import numpy as np

from golden_util import GOLDEN

HEADER = "#label\tgenomes\trows\tplus\tbp\tmin\tmax\n"
LABEL_COLS = ("labels", "n_genomes", "rows", "plus", "bp", "min_len", "max_len")
GROUP_COLS = ("g_rows", "g_bp", "g_core", "g_shell", "g_unique")


def reference_freq(rows5, rec_group, G):
    """The table as plain lists: per-label columns (labels ascending), bits as
    a list of W-word lists, the spectrum, the per-genome sums, the counts."""
    rows = np.asarray(rows5, np.int64).reshape(-1, 5).tolist()
    grp = [int(x) for x in np.asarray(rec_group).reshape(-1).tolist()]
    W = (G + 63) // 64
    per, used_rows, skipped = {}, [], 0
    for rec, s, e, strand, lab in rows:
        g = grp[rec]
        if lab < 0 or g < 0:
            skipped += 1
            continue
        ln = abs(e - s)
        d = per.setdefault(lab, {"rows": 0, "plus": 0, "bp": 0, "min": None, "max": 0, "set": set()})
        d["rows"] += 1
        d["plus"] += strand == 1
        d["bp"] += ln
        d["min"] = ln if d["min"] is None else min(d["min"], ln)
        d["max"] = max(d["max"], ln)
        d["set"].add(g)
        used_rows.append((g, lab, ln))
    labels = sorted(per)
    out = {"n_groups": G, "n_used": len(used_rows), "n_skipped": skipped, "labels": labels,
           "n_genomes": [len(per[l]["set"]) for l in labels], "rows": [per[l]["rows"] for l in labels],
           "plus": [per[l]["plus"] for l in labels], "bp": [per[l]["bp"] for l in labels],
           "min_len": [per[l]["min"] for l in labels], "max_len": [per[l]["max"] for l in labels],
           "bits": [[sum(1 << (g % 64) for g in per[l]["set"] if g // 64 == w) for w in range(W)] for l in labels]}
    out["spectrum_labels"], out["spectrum_bp"] = [0] * (G + 1), [0] * (G + 1)
    for l in labels:
        out["spectrum_labels"][len(per[l]["set"])] += 1
        out["spectrum_bp"][len(per[l]["set"])] += per[l]["bp"]
    for k in GROUP_COLS:
        out[k] = [0] * G
    for g, lab, ln in used_rows:
        n = len(per[lab]["set"])
        out["g_rows"][g] += 1
        out["g_bp"][g] += ln
        out["g_core" if n == G else ("g_unique" if n == 1 else "g_shell")][g] += ln
    return out


def reference_text(ref):
    return HEADER + "".join("%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % x for x in zip(*[ref[k] for k in LABEL_COLS]))


def as_lists(table):
    """A table of arrays (host.freq_table, or the Context's three exports
    put together) in reference_freq's form, for the keys it holds."""
    out = {}
    for k, v in table.items():
        if k == "pairs":
            continue
        out[k] = v.tolist() if hasattr(v, "tolist") else v
    return out


def assert_same(got, ref):
    got = as_lists(got)
    for k in ref:
        if k in got:
            assert got[k] == ref[k], k
    assert set(LABEL_COLS + GROUP_COLS + ("bits", "spectrum_labels", "spectrum_bp")) <= set(got)


def device_table(ctx):
    """Everything the context holds after freq(), as one dict."""
    t = ctx.freq_table()
    t["spectrum_labels"], t["spectrum_bp"] = ctx.freq_spectrum()
    t.update(ctx.freq_groups())
    return t


def check_device(ctx, rows5, rec_group, G, rows_on_device=False):
    """freq() on the device against reference_freq, exactly: the table, the
    spectrum, the per-genome sums, the text and the returned counts."""
    ref = reference_freq(rows5, rec_group, G)
    counts = ctx.freq(rec_group, G, rows=None if rows_on_device else rows5)
    assert counts == (len(ref["labels"]), ref["n_used"], ref["n_skipped"])
    assert_same(device_table(ctx), ref)
    text = ctx.freq_text()
    assert text.decode() == reference_text(ref)
    return ref, text


def golden(name):
    return json.load(open(os.path.join(GOLDEN, "freq", name + ".json")))


def rows_of(text):
    return [ln for ln in text.split("\n") if len(ln.split("\t")) == 5 and ln.split("\t")[3] in ("+", "-")]


def rows5_of(lines, names):
    """Printed rows -> [n, 5] int64 with record names mapped back to indices."""
    idx = {n: i for i, n in enumerate(names)}
    out = []
    for ln in lines:
        q, s, e, st, lab = ln.rsplit("\t", 4)
        out.append((idx[q], int(s), int(e), 1 if st == "+" else -1, int(lab)))
    return np.array(out, np.int64).reshape(-1, 5)


def fasta_names(fasta):
    return [ln[1:].decode() for ln in fasta.split(b"\n") if ln.startswith(b">")]


def files_of(ref, genome_names):
    """The three text files of a table (as `-g` writes them)."""
    G = ref["n_groups"]
    spectrum = "#genomes\tlabels\tbp\n" + "".join(
        "%d\t%d\t%d\n" % (g, ref["spectrum_labels"][g], ref["spectrum_bp"][g]) for g in range(1, G + 1))
    genomes = "#genome\trows\tbp\tcore\tshell\tunique\n" + "".join(
        "%s\t%d\t%d\t%d\t%d\t%d\n" % ((genome_names[g],) + tuple(ref[k][g] for k in GROUP_COLS)) for g in range(G))
    return {"_fr_freq.tsv": reference_text(ref), "_fr_spectrum.tsv": spectrum, "_fr_genomes.tsv": genomes}


def assert_files(prefix, ref, genome_names):
    for suffix, want in files_of(ref, genome_names).items():
        assert open(prefix + suffix).read() == want, suffix
    z = np.load(prefix + "_fr_presence.npz")
    assert z["labels"].dtype == np.int64 and z["labels"].tolist() == ref["labels"]
    assert z["bits"].dtype == np.uint64 and z["bits"].shape == (len(ref["labels"]), (ref["n_groups"] + 63) // 64)
    assert z["bits"].tolist() == ref["bits"]
    assert [x.decode() for x in z["genomes"].tolist()] == list(genome_names)
    d = os.path.dirname(prefix)
    assert not [f for f in os.listdir(d) if f.endswith(".tmp")]
