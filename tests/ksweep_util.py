"""Inputs and host restatements for the sweep over every k-mer length
(tests/test_ksweep_util.py on the CPU, tests/test_gpu_ksweep.py on the device).

sweep_fasta(k) is built so that a follower window the coverage pass wrongly
skips shows in the dBG: record 0 is the unmutated base genome and every
follower's differences from it are its own (synth.pangenome mutates the lead
too, so half of a follower's differences are shared by all followers and a
skipped window is hidden by another record about half the time).
witness_share() measures how many of the windows that differ from the lead
would be seen; numpy_dbg() restates the dBG rule without the oracle.
"""
import numpy as np

from pangenome_amd import synth

KS = tuple(range(1, 28))
SEED = 4242
GENOME = 20_000            # four 4096-window tiles and a ragged one
FOLLOWERS = 5
WIDTH = 61                 # odd: record starts move through the 16-base word alignments
SENTINEL = np.uint64(2 ** 64 - 1)

# the reference's tables (kmer_numba.py alpha :763-768, lastc :736-743, tab_rev_bytes :191-195)
ALPHA = np.full(256, 4, np.uint64)
LASTC = np.zeros(256, np.uint16)
TABREV = np.full(256, ord("N"), np.uint8)
CODE2 = np.full(256, 4, np.uint8)          # A0 C1 G2 T3 in either case (3 - code complements), 4: not ACGT
for _i, _c in enumerate(b"AGCT"):
    ALPHA[_c] = ALPHA[_c | 0x20] = _i
for _i, _c in enumerate(b"ATGCN"):
    LASTC[_c] = LASTC[_c | 0x20] = 1 << _i
    TABREV[_c] = TABREV[_c | 0x20] = b"TACGN"[_i]
for _i, _c in enumerate(b"ACGT"):
    CODE2[_c] = CODE2[_c | 0x20] = _i
LASTC[ord("$")] = 32


def _tail(k, seed):
    """The k-dependent tail: every length class around k, and one record with
    an N run and a lowercase stretch."""
    recs = []
    for j, n in enumerate((0, 1, k - 1, k, k + 1, k + 2, k + 3)):
        recs.append((b"len%d_%d" % (j, n), synth.ACGT[synth.base_genome(n, seed + 100 + j)].tobytes()))
    odd = bytearray(synth.ACGT[synth.base_genome(300, seed + 200)].tobytes())
    odd[100:130] = b"N" * 30
    odd[200:240] = bytes(odd[200:240]).lower()
    recs.append((b"odd", bytes(odd)))
    return b"".join(b">" + name + b"\n" + (seq + b"\n" if seq else b"") for name, seq in recs)


def sweep_fasta(k, seed=SEED):
    """The unmutated base, FOLLOWERS variants of it whose differences are all
    private, and the tail."""
    base = synth.base_genome(GENOME, seed)
    parts = [synth.to_fasta_lines(b"lead", base, width=WIDTH)]
    for i in range(FOLLOWERS):
        v = synth.variant(base, i, snp=0.01, indel=1e-3, seed=seed)
        parts.append(synth.to_fasta_lines(b"f%d" % i, v, width=WIDTH))
    return b"".join(parts) + _tail(k, seed)


def unrelated_fasta(k, seed=SEED):
    """sweep_fasta(k) with every follower replaced by an unrelated random
    record of the same length: nothing for the coverage pass to skip."""
    base = synth.base_genome(GENOME, seed)
    parts = [synth.to_fasta_lines(b"lead", base, width=WIDTH)]
    for i in range(FOLLOWERS):
        n = synth.variant(base, i, snp=0.01, indel=1e-3, seed=seed).shape[0]
        parts.append(synth.to_fasta_lines(b"u%d" % i, synth.base_genome(n, seed + 7000 + i), width=WIDTH))
    return b"".join(parts) + _tail(k, seed)


def records_of(fasta):
    """The sequences (uint8 arrays, line ends removed) of a FASTA that starts
    with a header and ends with a newline."""
    assert fasta[:1] == b">" and fasta[-1:] == b"\n"
    out = []
    for rec in fasta[1:].split(b"\n>"):
        out.append(np.frombuffer(b"".join(rec.split(b"\n")[1:]), np.uint8))
    return out


def reverse(s):
    return TABREV[s[::-1]]


def _windows(s, k):
    """(keys, masks) of one walk (build_dbg :1052-1090): base-5 keys, the
    predecessor's lastc bits << 6 | the successor's; '#' before the first
    window, '$' after the last; the last window's predecessor is the base
    two before it (:1078-1080), and at n == k+1 numba's never-entered loop
    leaves i = 0 (key digit and predecessor s[1])."""
    n = s.shape[0]
    if n < k:
        return np.array([SENTINEL]), np.array([32], np.uint16)
    a, nw = ALPHA[s], n - k + 1
    keys = np.zeros(nw, np.uint64)
    for t in range(k):
        keys += a[t:t + nw] * np.uint64(5 ** t)
    hd = np.concatenate([[ord("#")], s[:nw - 1]]).astype(np.uint8)
    nt = np.concatenate([s[k:], [ord("$")]]).astype(np.uint8)
    if n == k + 1:
        keys[1] = keys[0] // np.uint64(5) + a[1] * np.uint64(5 ** (k - 1))
        hd[1] = s[1]
    elif n > k + 1:
        hd[nw - 1] = s[n - k - 2]
    return keys, (LASTC[hd] << 6) | LASTC[nt]


def numpy_dbg(fasta, k, rc):
    """The dBG as sorted unique keys with OR-ed masks."""
    walks = [w for s in records_of(fasta) for w in ([s, reverse(s)] if rc else [s])]
    kk, mm = zip(*[_windows(s, k) for s in walks])
    keys, inv = np.unique(np.concatenate(kk), return_inverse=True)
    masks = np.zeros(keys.shape[0], np.uint16)
    np.bitwise_or.at(masks, inv, np.concatenate(mm))
    return keys, masks


def _mers(s, m):
    """(packed 2-bit m-mers at every start, whether each is all ACGT)."""
    c = CODE2[s]
    nw = s.shape[0] - m + 1
    if nw <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, bool)
    bad = np.concatenate([[0], np.cumsum(c == 4)])
    v = np.zeros(nw, np.uint64)
    for t in range(m):
        v |= (c[t:t + nw] & 3).astype(np.uint64) << np.uint64(2 * t)
    return v, bad[m:m + nw] == bad[:nw]


def witness_share(fasta, k, rc=False):
    """Of the interior windows of records 1.. whose k+2-base context (the
    window, its predecessor and its successor) does not occur in record 0,
    the share a wrong skip of which would change the dBG: those whose (key,
    predecessor) or (key, successor) pair occurs exactly once in the whole
    input - on the forward strands, or with rc on both (the reverse walk of
    another place can contribute the same key and bit).  Exactly once, not
    merely absent from the lead: the pass depends on each record's start
    modulo 16, so a fault may hit one follower only.  (The pairs are counted
    as k+1-base strings; the one shifted predecessor at each record's last
    window is not.)  Returns (share, windows that differ from the lead)."""
    recs = records_of(fasta)
    walks = recs + ([reverse(s) for s in recs] if rc else [])
    pool = np.concatenate([v[ok] for v, ok in (_mers(s, k + 1) for s in walks)])
    uniq, cnt = np.unique(pool, return_counts=True)
    lead_ctx, ok = _mers(recs[0], k + 2)
    lead_ctx = np.unique(lead_ctx[ok])
    seen = total = 0
    for s in recs[1:]:
        ctx, ok = _mers(s, k + 2)                       # context j: window j + 1
        if not ctx.shape[0]:
            continue
        pair, _ = _mers(s, k + 1)                       # pair j: [pred, key] of window j + 1, [key, succ] of window j
        differs = ok & ~np.isin(ctx, lead_ctx)
        once = cnt[np.searchsorted(uniq, pair[differs.nonzero()[0][:, None] + np.arange(2)])] == 1
        seen += int(once.any(axis=1).sum())
        total += int(differs.sum())
    return (seen / total if total else 0.0), total
