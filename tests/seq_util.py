"""An independent reference of the region sequences for the tests: the FASTA
lines of a record joined, a 256-entry translate table, Python slices and
`max` (nothing shared with pangenome_amd/), its texts, and the comparison
every test uses.  Inputs use "\\n" line ends only and end with one."""
import hashlib
import json
import os

import numpy as np

from golden_util import GOLDEN
from region_util import GFA_HEADER, LINK_COLS, reference_region

LETTER = bytes(ord(chr(b).upper()) if chr(b) in "ACGTacgt" else ord("N") for b in range(256))
COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")
INT_COLS = ("label", "row", "record", "start", "end", "strand")
UINT_COLS = ("len", "gc", "amb", "offset")
TSV_HEADER = b"#label\trow\tseqid\tstart\tend\tstrand\tlen\tgc\tamb\n"


def fasta_records(fasta):
    """(names, sequences): per record its header without '>' and its lines
    joined and translated (ACGT in either case -> upper case, all else -> N)."""
    names, seqs = [], []
    for ln in bytes(fasta).split(b"\n"):
        if ln.startswith(b">"):
            names.append(ln[1:])
            seqs.append([])
        elif names:
            seqs[-1].append(ln)
    return names, [b"".join(s).translate(LETTER) for s in seqs]


def make_fasta(seqs, width=60, names=None):
    """Records named r0, r1, ... (or names) with their sequences in lines of `width`."""
    out = []
    for i, s in enumerate(seqs):
        out.append(b">" + (names[i] if names else b"r%d" % i) + b"\n")
        out += [s[j:j + width] + b"\n" for j in range(0, len(s), width)]
    return b"".join(out)


def reference_seqs(rows5, rec_group, G, seqs):
    """The table, the sequences and the counts as plain lists.  A row is used
    iff its label >= 0 and its record has a genome; a label's representative
    is its longest used row, the first in list order among equals."""
    rows = np.asarray(rows5, np.int64).reshape(-1, 5).tolist()
    grp = [int(x) for x in np.asarray(rec_group).reshape(-1).tolist()]
    assert len(grp) == len(seqs) and all(-1 <= g < G for g in grp)
    per, skipped = {}, 0
    for i, (rec, s, e, strand, lab) in enumerate(rows):
        if lab < 0 or grp[rec] < 0:
            skipped += 1
            continue
        per.setdefault(lab, []).append((abs(e - s), i))
    out = {k: [] for k in INT_COLS + UINT_COLS}
    out.update(n_skipped=skipped, seqs=[])
    total = 0
    for lab in sorted(per):
        ln, i = max(per[lab], key=lambda t: t[0])           # (max keeps the first of equals)
        rec, s, e, strand, _ = rows[i]
        lo, hi = min(s, e), max(s, e)
        assert 0 <= lo and hi <= len(seqs[rec])
        f = seqs[rec][lo:hi]
        if strand != 1:
            f = f[::-1].translate(COMPLEMENT)
        assert len(f) == ln
        for k, v in zip(INT_COLS + UINT_COLS, (lab, i, rec, s, e, strand, ln, f.count(b"C") + f.count(b"G"),
                                               f.count(b"N"), total)):
            out[k].append(v)
        out["seqs"].append(f)
        total += ln
    out["bases"] = b"".join(out["seqs"])
    return out


def reference_fasta(ref, names):
    return b"".join(b">%d %s:%d-%d:%s len=%d\n%s\n" % (l, bytes(names[r]), min(s, e), max(s, e),
                                                      b"+" if st == 1 else b"-", n, f)
                    for l, r, s, e, st, n, f in zip(ref["label"], ref["record"], ref["start"], ref["end"],
                                                    ref["strand"], ref["len"], ref["seqs"]))


def reference_tsv(ref, ids):
    return TSV_HEADER + b"".join(b"%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (l, i, bytes(ids[r]), s, e, st, n, gc, amb)
                                 for l, i, r, s, e, st, n, gc, amb in zip(*[ref[k] for k in INT_COLS + UINT_COLS[:3]]))


def reference_gfa_seq(graph, ref, names):
    """The GFA 1 text of region_util.reference_region's graph with the
    sequences on the S lines."""
    assert graph["labels"] == ref["label"] and graph["max_len"] == ref["len"]
    out = [GFA_HEADER.encode()]
    out += [b"S\t%d\t%s\tLN:i:%d\n" % (l, f, m) for l, f, m in zip(graph["labels"], ref["seqs"], graph["max_len"])]
    out += [b"L\t%d\t+\t%d\t+\t0M\tRC:i:%d\tgn:i:%d\n" % x for x in zip(*[graph[k] for k in LINK_COLS])]
    for rec, strand, lo, hi, labs in zip(graph["path_record"], graph["path_strand"], graph["path_lo"],
                                         graph["path_hi"], graph["path_labels"]):
        out.append(b"P\t%s:%d-%d:%s\t%s\t*\n" % (bytes(names[rec]), lo, hi, b"+" if strand == 1 else b"-",
                                                 ",".join("%d+" % l for l in labs).encode()))
    return b"".join(out)


def assert_table(got, ref):
    assert list(got) == list(INT_COLS + UINT_COLS)
    for k in INT_COLS + UINT_COLS:
        assert got[k].dtype == (np.int64 if k in INT_COLS else np.uint64) and got[k].ndim == 1, k
        assert got[k].tolist() == ref[k], k


def device_state(ctx, names):
    """Everything the context holds after region_seqs(): table (as lists), bases, FASTA text."""
    return ({k: v.tolist() for k, v in ctx.region_seqs_table().items()}, ctx.region_seqs_bases(),
            ctx.region_fasta_text(names))


def parse(ctx, fasta):
    """Parse `fasta` in the context; returns (names, sequences) of the
    reference after checking that both sides mean the same coordinates."""
    ctx.parse_host(np.frombuffer(bytes(fasta), np.uint8))
    names, seqs = fasta_records(fasta)
    assert ctx.records()["seq_len"].tolist() == [len(s) for s in seqs]
    return names, seqs


def check_device(ctx, rows, rec_group, G, names, seqs, rows_on_device=False, graph=False):
    """region_seqs() on the device against reference_seqs, exactly: the three
    returned counts, the table with its dtypes, the bases and the FASTA text;
    with graph, region_graph() of the same rows and the GFA with sequences
    too.  Returns (ref, FASTA text)."""
    ref = reference_seqs(rows, rec_group, G, seqs)
    counts = ctx.region_seqs(rec_group, G, rows=None if rows_on_device else rows)
    assert counts == (len(ref["label"]), len(ref["bases"]), ref["n_skipped"])
    assert_table(ctx.region_seqs_table(), ref)
    assert ctx.region_seqs_bases() == ref["bases"]
    text = ctx.region_fasta_text(names)
    assert text == reference_fasta(ref, names)
    if graph:
        ctx.region_graph(rec_group, G, rows=None if rows_on_device else rows)
        gfa = ctx.region_gfa_seq_text(names)
        assert gfa == reference_gfa_seq(reference_region(rows, rec_group, G), ref, names)
        plain = ctx.region_gfa_text(names).split(b"\n")
        for a, b in zip(gfa.split(b"\n"), plain):
            if a.startswith(b"S\t"):
                f = a.split(b"\t")
                assert len(f[2]) == int(f[3][5:]) and b.split(b"\t") == [f[0], f[1], b"*", f[3]]
            else:
                assert a == b
        assert len(plain) == gfa.count(b"\n") + 1
    return ref, text


def summary(ref, ids):
    """The figures tests/golden/regionseq/*.json record; ids[r] = record r's seqid."""
    return {"n_regions": len(ref["label"]), "n_bases": len(ref["bases"]), "gc": sum(ref["gc"]),
            "amb": sum(ref["amb"]), "fasta_sha256": hashlib.sha256(reference_fasta(ref, ids)).hexdigest()}


def golden(name):
    return json.load(open(os.path.join(GOLDEN, "regionseq", name + ".json")))


def assert_files(prefix, ref, ids, graph=None):
    """The files `-s` writes; graph: reference_region's result when `-l` ran too."""
    assert open(prefix + "_fr_regions.fa", "rb").read() == reference_fasta(ref, ids)
    assert open(prefix + "_fr_regions.tsv", "rb").read() == reference_tsv(ref, ids)
    assert os.path.isfile(prefix + "_fr_graph_seq.gfa") == (graph is not None)
    if graph is not None:
        assert open(prefix + "_fr_graph_seq.gfa", "rb").read() == reference_gfa_seq(graph, ref, ids)
    assert not [f for f in os.listdir(os.path.dirname(prefix)) if f.endswith(".tmp")]
