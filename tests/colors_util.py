"""Inputs and yardsticks of the k-mer colour tests (test_kmer_colors_host.py,
test_gpu_kmer_colors.py).

Every input is a list of per-genome byte strings, each made of whole records
and ending in a newline; the file is their concatenation.  The independent
yardstick is the oracle: genome g's key set is OracleRun(piece_g, k, c).dbg()[0],
the dBG of that genome's records alone.  The n < k sentinel (key 2^64 - 1) is
no key of the table, so the colour comparisons leave it out of both sides
(the precondition - union of the pieces' keys == the whole file's keys - is
checked with it)."""
import functools
import os

import numpy as np

from golden_util import GOLDEN

SENTINEL = np.uint64(2 ** 64 - 1)
INPUTS = os.path.join(GOLDEN, "inputs")


def _read(name):
    return open(os.path.join(INPUTS, name), "rb").read()


def split_records(fasta: bytes):
    """The records of a FASTA whose first byte is '>' (header line included)."""
    assert fasta[:1] == b">"
    return [b">" + r for r in fasta[1:].split(b"\n>")]


def letters(record: bytes) -> bytes:
    return b"".join(record.split(b"\n")[1:]).replace(b"\r", b"")


def substitute(seq: bytes, index: int, rate: float = 0.03) -> bytes:
    """seq with about `rate` of its ACGT letters substituted (synth's
    generator: the positions from uniform(), the new letter from splitmix64)."""
    from pangenome_amd import synth
    a = np.frombuffer(seq.upper(), np.uint8).copy()
    code = np.full(256, 255, np.uint8)
    code[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4, dtype=np.uint8)
    d = code[a]
    s = synth.DEFAULT_SEED + 7919 * (index + 1)
    pos = np.flatnonzero((synth.uniform(s, 2, a.shape[0]) < rate) & (d < 4))
    shift = (synth.splitmix64(s, 3, pos.shape[0]) % np.uint64(3)).astype(np.uint8) + 1
    a[pos] = synth.ACGT[(d[pos] + shift) & 3]
    return a.tobytes()


def record(name: bytes, seq: bytes, width: int = 60) -> bytes:
    body = b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))
    return b">" + name + b"\n" + body


def base_letters(n: int, seed_off: int = 0) -> bytes:
    from pangenome_amd import synth
    return synth.ACGT[synth.base_genome(n, synth.DEFAULT_SEED + seed_off)].tobytes()


@functools.lru_cache(maxsize=None)
def pieces(name: str):
    """The per-genome byte strings of the input called `name`."""
    if name == "pan8":                                   # one genome per record
        recs = split_records(_read("pan8.fsa"))
        return tuple(r if r.endswith(b"\n") else r + b"\n" for r in recs)
    if name == "edge":                                   # edge.fsa, then two mutated copies of its longest record
        edge = _read("edge.fsa")
        recs = split_records(edge[edge.index(b"\n>") + 1:])
        longest = max((letters(r) for r in recs), key=len)
        return (edge + b"\n", record(b"copy1", substitute(longest, 1)), record(b"copy2", substitute(longest, 2)))
    if name == "smallk":                                 # 6 genomes of 400 bases
        base = base_letters(400, 1)
        return tuple(record(b"s%d" % g, substitute(base, 10 + g)) for g in range(6))
    if name.startswith("runs"):                          # window-run boundaries at k = int(name[4:])
        k = int(name[4:])
        base = base_letters(200, 2)
        lens = [k - 1, k, k + 1, k + 2, k + 15, k + 16, k + 17, 3 * 16 + k]
        recs = [record(b"r%d_%d" % (j, n), substitute(base[3 * j:3 * j + n], 20 + j, 0.05)) for j, n in enumerate(lens)]
        return tuple(b"".join(recs[g::3]) for g in range(3))         # three genomes, several records each
    if name.startswith("word"):                          # the word boundary: G = int(name[4:]) genomes of 300 bases
        base = base_letters(300, 3)
        return tuple(record(b"w%d" % g, base if g == 0 else substitute(base, 100 + g)) for g in range(int(name[4:])))
    if name == "excl":                                   # three genomes of two records of 200 bases
        base = base_letters(200, 4)
        return tuple(record(b"x%da" % g, substitute(base, 200 + 2 * g)) + record(b"x%db" % g, substitute(base, 201 + 2 * g))
                     for g in range(3))
    raise KeyError(name)


def fasta(name: str) -> bytes:
    return b"".join(pieces(name))


# (input, k, c) of every comparison against the oracle; c = 2: both strands (rc0 = 1), c = 0: the forward one
CASES = ([("pan8", 27, 2), ("pan8", 27, 0), ("edge", 5, 2), ("edge", 27, 2)] +
         [("smallk", k, 2) for k in (1, 2, 3)] + [("runs27", 27, 2), ("runs4", 4, 2)] +
         [("word65", 11, 2), ("word64", 11, 2), ("word1", 11, 2), ("excl", 11, 2)])


def oracle_keys(fa: bytes, k: int, c: int) -> np.ndarray:
    from oracle import oracle
    oracle.build()
    return np.unique(oracle.OracleRun(fa, k, c).dbg()[0])


@functools.lru_cache(maxsize=None)
def yardstick(name: str, k: int, c: int):
    """(per-genome oracle key sets, the oracle's keys of the whole file), the
    sentinel still in them; computed once and shared."""
    sets = tuple(oracle_keys(p, k, c) for p in pieces(name))
    for s in sets:
        s.setflags(write=False)
    whole = oracle_keys(fasta(name), k, c)
    whole.setflags(write=False)
    return sets, whole


def no_sentinel(keys: np.ndarray) -> np.ndarray:
    return keys[keys != SENTINEL]


def records_per_piece(name: str, n_records: int):
    """Records of every piece given the parse's record count of the whole
    file: a piece after the first starts with '>' and holds one record per
    header line; the first piece has the rest (a line before its first header
    may be a record of its own)."""
    later = [p.count(b"\n>") + 1 for p in pieces(name)[1:]]
    return [n_records - sum(later)] + later


def rec_group_of(name: str, n_records: int) -> np.ndarray:
    return np.repeat(np.arange(len(pieces(name)), dtype=np.int32), records_per_piece(name, n_records))


DIGIT = {65: 0, 67: 2, 71: 1, 84: 3}                     # A0 C2 G1 T3 (include/pangenome.h)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def window_keys(seq: bytes, k: int, rc: bool):
    """The key of every window of an ACGT-only record longer than k + 1, both
    strands if rc, with multiplicity (digit j has weight 5^j)."""
    assert len(seq) > k + 1 and set(seq) <= set(b"ACGT")
    out = []
    for s in ([seq, seq.translate(COMP)[::-1]] if rc else [seq]):
        d = [DIGIT[b] for b in s]
        out += [sum(d[q + j] * 5 ** j for j in range(k)) for q in range(len(s) - k + 1)]
    return out


def brute_colors(key_sets, G, keys=None):
    """host.kmer_colors with Python sets and loops."""
    sets = [set(int(x) for x in s) for s in key_sets]
    allk = sorted(set().union(*sets) if keys is None else set(int(x) for x in keys)) if (sets or keys is not None) else []
    W = (G + 63) // 64
    bits = [[0] * W for _ in allk]
    for i, x in enumerate(allk):
        for g in range(G):
            if x in sets[g]:
                bits[i][g // 64] |= 1 << (g % 64)
    ng = [sum(bin(w).count("1") for w in row) for row in bits]
    by_g = [sum(1 for v in ng if v == g) for g in range(G + 1)]
    has = lambda i, g: (bits[i][g // 64] >> (g % 64)) & 1
    kmers = [sum(has(i, g) for i in range(len(allk))) for g in range(G)]
    core = [sum(1 for i in range(len(allk)) if has(i, g) and ng[i] == G) for g in range(G)]
    uniq = [sum(1 for i in range(len(allk)) if has(i, g) and ng[i] == 1 and G > 1) for g in range(G)]
    shell = [a - b - c for a, b, c in zip(kmers, core, uniq)]
    shared = [[sum(1 for i in range(len(allk)) if has(i, g) and has(i, h)) for h in range(G)] for g in range(G)]
    return {"keys": allk, "bits": bits, "kmers_by_g": by_g, "g_kmers": kmers, "g_core": core, "g_shell": shell,
            "g_unique": uniq, "shared": shared}
