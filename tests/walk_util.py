"""Inputs and restatements for the direct tests of the edge, label and row
walks (tests/test_gpu_walks.py; checked against the oracle alone by
tests/test_walk_util.py).

* standard_fasta   one FASTA per k whose record lengths sit on every boundary
                   of the walks (n < k, n = k, n <= k + 1, one and two
                   16-window thread runs) next to records that share k-mers;
* record_table / names_of / subset_fasta
                   the record table (dist_util.seqio_records), the qids the
                   rows print, and the FASTA of the flagged records only (the
                   oracle's input for a rec_flags pass);
* dense_table      a label table that makes every window a hit;
* hash_ids         a few label ids spread over a table by a hash;
* label_dict       seq2graph's label dictionary (oracle.label_table) over
                   arrays instead of the two texts.
"""
import numpy as np

from dist_util import seqio_records

SENTINEL = 2 ** 64 - 1
M64 = 2 ** 64 - 1


def _dna(rng, n, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n).tolist())


def fasta_bytes(records, width=70):
    """[(header without '>', sequence)] -> FASTA bytes, sequences wrapped."""
    out = []
    for hdr, seq in records:
        out.append(">" + hdr + "\n")
        for i in range(0, len(seq), width):
            out.append(seq[i:i + width] + "\n")
    return "".join(out).encode()


def standard_records(k, seed=0):
    rng = np.random.default_rng(1000 * k + seed)
    base = _dna(rng, 3000)
    snp = list(base[300:1500])
    for i in range(25, len(snp), 97):
        snp[i] = "ACGT"[("ACGT".index(snp[i]) + 1) % 4]
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    recs = [
        ("base the 3,000-base record", base),
        ("insertion base with 40 bases inserted", base[:1500] + _dna(rng, 40) + base[1500:]),
        ("shifted a slice of base", base[700:2300]),
        ("len0 no sequence at all", ""),
        ("len1 one base", base[5:6]),
        ("km1 n = k - 1", base[10:10 + k - 1]),
        ("k0 n = k", base[20:20 + k]),
        ("kp1 n = k + 1", base[30:30 + k + 1]),
        ("kp2 n = k + 2", base[40:40 + k + 2]),
        ("w15 15 windows", base[100:100 + k + 14]),
        ("w16 16 windows", base[200:200 + k + 15]),
        ("w17 17 windows", base[300:300 + k + 16]),
        ("w32 32 windows", base[400:400 + k + 31]),
        ("w33 33 windows", base[500:500 + k + 32]),
        ("polyA key 0", "A" * 200),
        ("period4 a repeat cut at an odd length", ("ACGT" * 60)[:237]),
        ("mixed N, $ and lowercase",
         _dna(rng, 90) + "NNNN$" + _dna(rng, 70).lower() + "nn" + base[900:960] + _dna(rng, 420, "ACGTN$") +
         base[2000:2050].lower()),
        ("snps a slice of base with substitutions", "".join(snp)),
        ("revcomp the other strand of a slice", "".join(comp[c] for c in reversed(base[1800:2400]))),
        ("other unrelated bases", _dna(rng, 500)),
    ]
    return recs


def standard_fasta(k, seed=0):
    """The standard input of the walk tests for k-mer length k."""
    return fasta_bytes(standard_records(k, seed))


def repeats_fasta(n_copies=64, length=2000, seed=7):
    """One record `n_copies` times under different names, then a copy with a
    substitution every 50 bases: every walk of the first launch claims the
    same edge slots."""
    rng = np.random.default_rng(seed)
    base = _dna(rng, length)
    snp = list(base)
    for i in range(17, length, 50):
        snp[i] = "ACGT"[("ACGT".index(snp[i]) + 2) % 4]
    recs = [("copy%02d the same bases" % i, base) for i in range(n_copies)] + [("snp one change every 50", "".join(snp))]
    return fasta_bytes(recs)


# ----------------------------------------------------------------- records
def record_table(fasta):
    """(seq_len, hdr_start, hdr_len) int64 arrays of the FASTA's records."""
    recs = seqio_records(fasta)
    cols = list(zip(*recs)) if recs else [(), (), (), ()]
    return tuple(np.asarray(c, np.int64) for c in cols[:3])


def names_of(fasta):
    """qid of every record: its header line without the '>' (:1946-1949)."""
    _, hs, hl = record_table(fasta)
    return [bytes(fasta[int(s) + 1:int(s) + int(l)]) for s, l in zip(hs, hl)]


def subset_fasta(fasta, flags):
    """The FASTA of the flagged records only, each cut at its header's start
    (as dist_util.OracleShard.build cuts a chunk)."""
    _, hs, _ = record_table(fasta)
    flags = np.asarray(flags)
    assert flags.shape[0] == hs.shape[0]
    ends = np.append(hs[1:], len(fasta))
    return b"".join(fasta[int(hs[r]):int(ends[r])] for r in np.flatnonzero(flags).tolist())


def flag_patterns(fasta, k):
    """rec_flags of the walk tests: name -> uint8 array (None: every record)."""
    n, _, _ = record_table(fasta)
    R = n.shape[0]
    short = np.flatnonzero(n == k + 1)
    assert short.size, "the input has a record with n = k + 1"
    one = lambda r: (np.arange(R) == r).astype(np.uint8)                      # noqa: E731
    return {
        "alternate": (np.arange(R) % 2 == 1).astype(np.uint8),
        "last": one(R - 1),
        "short": one(int(short[0])),
        "none": np.zeros(R, np.uint8),
        "all": None,
    }


# ------------------------------------------------------------------ labels
def dense_table(dbg_keys, dbg_masks):
    """(keys, vals) int64: for every dBG key but the n < k sentinel, one
    entry per (pred, succ) with pred in {0} + the bits of mask >> 6 and succ in
    {0} + the bits of mask & 63, value (pred << 6) | succ.  The lastc codes are
    one-hot, so every window's (key, value) is among them."""
    K, V = [], []
    for x, m in zip(np.asarray(dbg_keys, np.uint64).tolist(), np.asarray(dbg_masks).tolist()):
        if x == SENTINEL:
            continue
        preds = [0] + [1 << b for b in range(6) if (m >> 6) >> b & 1]
        succs = [0] + [1 << b for b in range(6) if m >> b & 1]
        for p in preds:
            for s in succs:
                K.append(x)
                V.append((p << 6) | s)
    return np.array(K, np.uint64).view(np.int64), np.array(V, np.int64)


def hash_ids(keys, vals, mod, salt=0):
    """A label id in [0, mod) per entry from a hash of (key, value)."""
    out = []
    for x, v in zip(np.asarray(keys, np.int64).view(np.uint64).tolist(), np.asarray(vals, np.int64).tolist()):
        h = (x * 0x9E3779B97F4A7C15 + (v + salt + 1) * 0xC2B2AE3D27D4EB4F) & M64
        h ^= h >> 29
        h = (h * 0xBF58476D1CE4E5B9) & M64
        out.append((h >> 32) % mod)
    return np.array(out, np.int64)


def mcl_entries(mcl_text):
    """([(key, value, line index)] in file order, number of lines) of a `.mcl`."""
    ent, flag = [], 0
    for line in mcl_text.splitlines(keepends=True):
        for tok in line[:-1].split("\t"):
            a = tok.split("_")[:2]
            ent.append((int(a[0]), int(a[1]), flag))
        flag += 1
    return ent, flag


def label_dict(tuples, mcl=(), next_label=0):
    """seq2graph :1918-1944 over arrays: the `.mcl` entries (key, value, id) in
    file order (a later one replaces an earlier one's id in place, as dict
    assignment does), then every node of the edges, n0_v0 then n1_v1 in
    list order, that has no label yet: next_label, next_label + 1, ...
    Returns (keys, vals, ids) int64 in insertion order."""
    lab = {}
    for a, b, i in mcl:
        lab[(int(a), int(b))] = int(i)
    flag = int(next_label)
    for a, b, c, d in np.asarray(tuples, np.uint64).reshape(-1, 4).tolist():
        for node in ((a, b), (c, d)):
            if node not in lab:
                lab[node] = flag
                flag += 1
    keys = np.array([a for a, _ in lab], np.uint64).view(np.int64)
    vals = np.array([b for _, b in lab], np.uint64).view(np.int64)
    ids = np.array(list(lab.values()), np.int64)
    return keys, vals, ids


def mcl_arrays(mcl):
    """The `.mcl` part of label_dict alone, as pg_labels_from_edges takes it
    (distinct entries)."""
    return label_dict(np.zeros((0, 4), np.uint64), mcl, 0)


# -------------------------------------------------------------------- rows
def row_lines(rows5, names):
    """The printed rows (:1946-1949) of (record, start, end, strand, label)."""
    return ["%s\t%d\t%d\t%s\t%d" % (names[r].decode(), s, e, "+" if st == 1 else "-", lab)
            for r, s, e, st, lab in np.asarray(rows5).reshape(-1, 5).tolist()]
