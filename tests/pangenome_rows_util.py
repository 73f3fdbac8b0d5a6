"""Rows and records shaped the way the row pass writes them, for the tests of
pg_region_bubbles, pg_region_variants and pg_region_align: whole records tiled
by rows, one long run per record with anchor after anchor, many sites per run,
alleles that descend from one another by small edits, both strands, `N` and
lower case, genomes on either side of the 64-genome word boundary
(block_pangenome); and the one-site grid of cores around the strip and word
borders with low-complexity letters (site_frame, lowcx_site).  Nothing here
reads a fixture or imports pangenome_amd/; the generators use
np.random.default_rng(seed) alone and are deterministic in their arguments."""
import functools

import numpy as np

from seq_util import fasta_records, make_fasta
from variants_util import segments

PAD = b"GATTC"                                           # before and behind every record's blocks
LENGTHS = (0, 1, 5, 17, 40, 64, 65, 90)                  # variant 0's length: one of these or `longest`
REVCOMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
BORDERS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129)
KINDS = ("two", "homo", "tandem", "near")


def pick(rng, alphabet, n):
    return bytes(alphabet[x] for x in rng.integers(0, len(alphabet), int(n)))


def edited(rng, seq, alphabet=b"ACGT"):
    """seq after 1 to 3 edits: a substitution, a deletion or an insertion of 1
    to 5 letters, a tandem copy (a unit of 1 to 3 letters repeated 1 to 3 more
    times next to itself), one letter set to N, one set to lower case.  An
    empty sequence can only take an insertion."""
    s = bytearray(seq)
    for _ in range(int(rng.integers(1, 4))):
        what = int(rng.integers(0, 6)) if s else 2
        at = int(rng.integers(0, len(s))) if s else 0
        if what == 0:
            s[at] = next(x for x in pick(rng, alphabet, 1) * 2 + bytes(alphabet) if x != bytes(s[at:at + 1]).upper()[0])
        elif what == 1:
            del s[at:at + int(rng.integers(1, 6))]
        elif what == 2:
            at = int(rng.integers(0, len(s) + 1))
            s[at:at] = pick(rng, alphabet, rng.integers(1, 6))
        elif what == 3:
            unit = s[at:at + int(rng.integers(1, 4))]
            s[at:at] = unit * int(rng.integers(1, 4))
        elif what == 4:
            s[at] = ord("N")
        else:
            s[at] = bytes(s[at:at + 1]).lower()[0]
    return bytes(s)


def block_pangenome(seed, G, slots, longest, alphabet=b"ACGT"):
    """(records, rows5, rec_group): an ancestor of slots + 1 anchor blocks
    (labels 2 s + 1, 4 to 24 letters) with one variable slot between
    neighbours.  A slot has 2 to 5 variants: variant 0 is random letters,
    every later one an earlier one of the slot after edited(); each is cut
    into up to 3 inner blocks (an empty one into none) with fresh labels above
    the anchors', so variants that read alike still differ in their paths.  A
    genome takes every anchor - an inner one is dropped with probability 0.04 -
    and in every slot variant min(geometric(0.5) - 1, last); with probability
    0.5 its block list is cut into two records, and with probability 0.5 it
    has one more record, a second copy of 2 to 6 neighbouring slots with
    variants drawn anew - two alleles of one site in one genome, the GT cell
    `0/1`; a record lies on `+` with probability 0.7, and on `-` it stores the reverse complement.  A record is
    PAD + its blocks + PAD, one row per block in walk order and no unused
    rows: [rec, o, o + len, 1, label] upward, [rec, hi, hi - len, -1, label]
    downward.  rec_group[r] is the record's genome; the last record has group
    -1 and two rows with anchor labels, which must not count."""
    rng = np.random.default_rng(seed)
    anchors = [(2 * s + 1, pick(rng, alphabet, rng.integers(4, 25))) for s in range(slots + 1)]
    label = 2 * slots + 2
    variants = []
    for s in range(slots):
        seqs = [pick(rng, alphabet, (LENGTHS + (longest,))[int(rng.integers(0, len(LENGTHS) + 1))])]
        for _ in range(int(rng.integers(1, 5))):
            seqs.append(edited(rng, seqs[int(rng.integers(0, len(seqs)))], alphabet))
        cut = []
        for f in seqs:
            n = min(len(f), int(rng.integers(1, 4)))
            at = [0] + sorted(rng.choice(np.arange(1, len(f)), n - 1, replace=False).tolist()) + [len(f)] if n else [0]
            cut.append([(label + i, f[x:y]) for i, (x, y) in enumerate(zip(at, at[1:]))])
            label += n
        variants.append(cut)
    records, rows, grp = [], [], []

    def record(blocks, strand, g):
        body = b"".join(f for _, f in blocks)
        rec, at = len(records), len(PAD) if strand == 1 else len(PAD) + len(body)
        for lab, f in blocks:
            rows.append([rec, at, at + strand * len(f), strand, lab])
            at += strand * len(f)
        records.append(PAD + (body if strand == 1 else body[::-1].translate(REVCOMP)) + PAD)
        grp.append(g)

    for g in range(G):
        blocks = []
        for s in range(slots + 1):
            if not (0 < s < slots and rng.random() < 0.04):
                blocks.append(anchors[s])
            if s < slots:
                blocks += variants[s][min(int(rng.geometric(0.5)) - 1, len(variants[s]) - 1)]
        parts = [blocks]
        if rng.random() < 0.5:
            c = int(rng.integers(1, len(blocks)))
            parts = [blocks[:c], blocks[c:]]
        if rng.random() < 0.5:                           # a second copy of a few slots, its variants drawn anew
            s0, dup = int(rng.integers(0, slots - 1)), []
            s1 = min(s0 + int(rng.integers(2, 7)), slots)
            for s in range(s0, s1):
                dup += [anchors[s]] + variants[s][min(int(rng.geometric(0.5)) - 1, len(variants[s]) - 1)]
            parts.append(dup + [anchors[s1]])
        for part in parts:
            record(part, 1 if rng.random() < 0.7 else -1, g)
    record(anchors[:2], 1, -1)
    return records, np.asarray(rows, np.int64).reshape(-1, 5), grp


# ------------------------------------------------------------ the shapes and their floors
# (seed, G, slots, longest, alphabet); every shape runs with min_genomes_of(G)
SHAPES = [(3, 12, 40, 120, b"ACGT"),                     # baseline
          (4, 70, 30, 130, b"ACGT"),                     # two presence words
          (5, 9, 40, 200, b"AC"),                        # low complexity
          (1, 130, 24, 70, b"ACGT"),                     # three presence words
          (2, 3, 60, 257, b"AC")]                        # low complexity, long variants
FLOORS = dict(sites=30, alleles=90, minus_alleles=5, n_alleles=20, placed=10, placed_not_first=5, unplaced=1,
              lines=40, lines_shared=5, long_cores=3, segments_in_a_run=10)
GT_CELLS = {b"0/1", b"1", b"0", b"."}


def min_genomes_of(G):
    """Three quarters of the genomes: the anchors stay anchors although 4 % of
    them are dropped."""
    return max(2, G - G // 4)


@functools.lru_cache(maxsize=None)
def shape_input(i):
    """Shape i's (rows, rec_group, G, names, sequences, FASTA, ref_group): the
    reference genome is the first from G // 2 upward whose records are not all
    on `-`.  Shared by the tests: nobody changes it."""
    _, G = SHAPES[i][:2]
    records, rows, grp = block_pangenome(*SHAPES[i])
    rows.setflags(write=False)
    fasta = make_fasta(records)
    names, seqs = fasta_records(fasta)
    plus = {grp[r] for r, _, _, strand, _ in rows.tolist() if strand == 1}
    return rows, tuple(grp), G, names, seqs, fasta, next(g for g in range(G // 2, G) if g in plus)


def figures(res, vcf, rows, grp):
    """What FLOORS bounds, of align_util.reference_align's result res and the
    primitives' VCF body, plus the GT cells found."""
    ref, bub = res["ref"], res["ref"]["bubbles"]
    per_run = {}
    for i, _ in segments(rows.tolist(), grp, set(bub["anchors"])):
        per_run[rows[i][0]] = per_run.get(rows[i][0], 0) + 1
    cores = [(n - p - q, m - p - q) for n, m, p, q in zip(res["t_len"], res["q_len"], res["prefix"], res["suffix"])]
    cells = {c for ln in vcf.split(b"\n")[:-1] for c in ln.split(b"\t")[9:]}
    return dict(sites=bub["n_sites"], alleles=bub["n_alleles"], minus_alleles=ref["strand"].count(-1),
                n_alleles=sum(1 for x in ref["amb"] if x), placed=ref["n_placed"],
                placed_not_first=sum(1 for k in ref["ref_allele"] if k), unplaced=ref["n_unplaced"],
                lines=res["n_lines"], lines_shared=sum(1 for ln in res["lines"] if ln["ac"] > 1),
                long_cores=sum(1 for a, b in cores if max(a, b) > 64),
                segments_in_a_run=max(per_run.values(), default=0)), cells


def assert_floors(res, vcf, rows, grp):
    got, cells = figures(res, vcf, rows, grp)
    for k, least in FLOORS.items():
        assert got[k] >= least, (k, got[k], least)
    assert cells >= GT_CELLS, cells
    return got


# ------------------------------------------------------------ one site around the strip and word borders
def other(ch):
    return b"ACGT"[(b"ACGT".index(ch) + 1) % 4]


def site_frame(T, shift, core):
    """One site: the target T, and for every (a, b) of BORDERS x BORDERS, the
    k-th of them, a query that shares T's first p = shift + 16 (k % 3) letters,
    replaces the next a by core(k, those a letters, b) - b letters whose ends
    are then forced to differ from the replaced ones', so that nothing more is
    trimmed - and shares the rest; genomes 1 and 2 by turns, every third query
    on `-`.  Returns [alleles] as test_align_host.site_records takes it."""
    alleles, k = [(T, 0, 1)], 0
    for a in BORDERS:
        for b in BORDERS:
            p = shift + 16 * (k % 3)
            t = T[p:p + a]
            u = bytearray(core(k, t, b))
            assert len(u) == b
            if a and b:
                u[0], u[-1] = (other(t[0]), other(t[-1])) if b > 1 else (other(t[0]),) * 2
                if b == 1 and a > 1 and u[0] == t[-1]:
                    u[0] = next(x for x in b"ACGT" if x not in (t[0], t[-1]))
            alleles.append((T[:p] + bytes(u) + T[p + a:], 1 + k % 2, 1 if k % 3 else -1))
            k += 1
    return [alleles]


def homopolymers(rng, n):
    """Runs of one letter, 1 to 40 long, no two neighbours of the same letter."""
    out, last = bytearray(), None
    while len(out) < n:
        last = next(x for x in pick(rng, b"ACGT", 1) * 2 + b"ACGT" if x != last)
        out += bytes([last]) * int(rng.integers(1, 41))
    return bytes(out[:n])


def lowcx_site(shift, kind, seed):
    """site_frame with letters of low complexity, where co-optimal paths
    abound and the tie rule decides every cell.  "two": target and cores
    uniform over AC.  "homo": both runs of one letter.  "tandem": the target a
    unit of 2 to 5 letters repeated, a core the same unit at another phase,
    so with another repeat count.  "near": a core is the replaced letters
    themselves after edited(), cut or filled to its length, over AC.  Forcing
    the ends brings in G or T where it needs a third letter."""
    rng = np.random.default_rng([seed, shift, KINDS.index(kind)])
    if kind == "two":
        T = pick(rng, b"AC", 200)
        core = lambda k, t, b: pick(rng, b"AC", b)
    elif kind == "homo":
        T = homopolymers(rng, 200)
        core = lambda k, t, b: homopolymers(rng, b)
    elif kind == "tandem":
        unit = pick(rng, b"ACGT", rng.integers(2, 6))
        while len(set(unit)) < 2:
            unit = pick(rng, b"ACGT", len(unit))
        T = (unit * 200)[:200]
        core = lambda k, t, b: (unit * (b + 2))[int(rng.integers(0, len(unit))):][:b]
    else:
        T = pick(rng, b"AC", 200)
        core = lambda k, t, b: (edited(rng, t, b"AC") + pick(rng, b"AC", b))[:b]
    return site_frame(T, shift, core)

