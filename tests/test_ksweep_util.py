"""tests/ksweep_util.py on the CPU: the sweep input can see a wrong coverage
pass at every k >= 8, and the oracle that tests/test_gpu_ksweep.py compares
the device with gives, at every k from 1 to 27, the dBG of a numpy
restatement of the rule."""
import numpy as np
import pytest

import ksweep_util as ku


def test_sweep_input_shape():
    for k in (1, 2, 14, 27):
        fasta = ku.sweep_fasta(k)
        recs = ku.records_of(fasta)
        lens = [r.shape[0] for r in recs]
        assert lens[0] == ku.GENOME and len(recs) == 1 + ku.FOLLOWERS + 8 and len(fasta) < 130_000
        assert all(abs(n - ku.GENOME) < 200 for n in lens[1:1 + ku.FOLLOWERS])
        assert lens[1 + ku.FOLLOWERS:-1] == [0, 1, k - 1, k, k + 1, k + 2, k + 3]
        assert (recs[-1] == ord("N")).sum() == 30 and sum(97 <= c <= 122 for c in recs[-1].tolist()) == 40
        assert (ku.GENOME - k + 1 + 4095) // 4096 == 5                 # four full tiles and a ragged one
        starts = [fasta.index(b">" + n + b"\n") + len(n) + 2 for n in (b"lead", b"f0", b"f1", b"f2", b"f3", b"f4")]
        assert len({s % 16 for s in starts}) >= 4                      # record starts at several word alignments
        other = ku.records_of(ku.unrelated_fasta(k))
        assert [r.shape[0] for r in other] == lens and np.array_equal(other[0], recs[0])
        assert all(np.array_equal(a, b) for a, b in zip(other[1 + ku.FOLLOWERS:], recs[1 + ku.FOLLOWERS:]))


def test_witness_share_counts_by_hand():
    """Lead ACGTACGTAC, follower with one substitution, k = 2: the four
    interior windows around the substitution differ from the lead; the
    (key, predecessor) and (key, successor) strings that occur once are
    counted by hand."""
    fasta = b">a\nACGTACGTAC\n>b\nACGTTCGTAC\n"
    # follower 4-base contexts: ACGT CGTT GTTC TTCG TCGT CGTA GTAC; the lead has ACGT CGTA GTAC TACG
    # differing: CGTT GTTC TTCG TCGT (windows 2..5); 3-base strings of the whole input, counted:
    # ACG 3, CGT 4, GTA 3, TAC 3, GTT 1, TTC 1, TCG 1
    # CGTT: CGT 4, GTT 1 -> seen; GTTC: GTT, TTC -> seen; TTCG: TTC, TCG -> seen; TCGT: TCG 1 -> seen
    assert ku.witness_share(fasta, 2) == (1.0, 4)
    # a second copy of the follower: nothing of it occurs once any more
    assert ku.witness_share(fasta + b">c\nACGTTCGTAC\n", 2) == (0.0, 8)


def test_witness_share_cap():
    """The cap: at every k >= 8 at least 0.95 of the follower windows that
    differ from the lead are visible in the dBG if skipped.  Below, the dBG
    saturates (every short key occurs many times) and the share is printed
    only: a coverage error cannot change the result there."""
    shares = {}
    for k in ku.KS:
        fasta = ku.sweep_fasta(k)
        shares[k] = ku.witness_share(fasta, k), ku.witness_share(fasta, k, rc=True)
        print("k=%2d  witness share %.3f (both strands %.3f) of %d windows" % (k, shares[k][0][0], shares[k][1][0],
                                                                              shares[k][0][1]))
    for k in range(8, 28):
        fw, n = shares[k][0]
        assert n > 10_000, (k, n)                       # (about 1 % SNPs x k + 2 bases x 100 k follower windows)
        assert fw >= 0.95, (k, fw)


@pytest.mark.parametrize("k", ku.KS)
def test_oracle_is_the_numpy_rule(oracle_mod, k):
    """oracle.run_pipeline on sweep_fasta(k) gives the dBG of numpy_dbg: the
    sweep's reference is pinned by the goldens and by this."""
    fasta = ku.sweep_fasta(k)
    out = oracle_mod.run_pipeline(fasta, k, 3)
    keys, masks = ku.numpy_dbg(fasta, k, True)
    assert np.array_equal(out["dbg_keys"], keys)
    assert np.array_equal(out["dbg_masks"], masks)
    assert np.array_equal(out["rdbg_keys"], keys[oracle_mod.rdbg_member(masks)])
    fw = oracle_mod.OracleRun(fasta, k, 0)
    k0, m0 = ku.numpy_dbg(fasta, k, False)
    assert np.array_equal(fw.dbg()[0], k0) and np.array_equal(fw.dbg()[1], m0)
