"""The band form of the alleles' alignments for the tests (PG_TUNE_ALIGN_BAND):
the band matrix in plain Python, the per-pair decision, and reference_align_band
on top of the unchanged align_util.  Nothing here imports pangenome_amd/.

Definition (stated on its own): with the band on, only a pair with (a + 1)(b +
1) > cells_cap changes.  With an empty core side it is aligned as it stands
(`bI` or `aD`, distance a + b).  Otherwise t_k = t0 2^k and band_cells(t) = a
min(b, 2 t + 1); k_lo is the smallest k with t_k >= |a - b|, k* the smallest
with t_k >= D[a][b], k_hi the largest with band_cells(t_k) <= band_cap (-1: none);
the pair is aligned iff k* <= k_hi, and then reads exactly as the full matrix
gives it at an unlimited cells_cap; else it stays as align_util.align_pair
leaves a pair above the cap.  Its attempts: max(0, min(k*, k_hi) - k_lo + 1).

The band matrix B fills the cells with |j - i| <= t (borders included) by the
same recurrence and holds INF everywhere else."""
import align_util
from align_util import CELLS_CAP, assert_same, reference_align
from variants_util import reference_variants

INF = 1 << 30
BAND_CAP = 1 << 26
T0 = 64
UNLIMITED = 1 << 62
FOREVER = 1 << 40                                        # k_hi of a pair whose whole matrix is within band_cap


def band_matrix(t, u, th):
    """B as a list of rows, INF outside the band."""
    a, b = len(t), len(u)
    B = [[INF] * (b + 1) for _ in range(a + 1)]
    for j in range(min(b, th) + 1):
        B[0][j] = j
    for i in range(1, a + 1):
        prev, row = B[i - 1], B[i]
        if i <= th:
            row[0] = i
        for j in range(max(1, i - th), min(b, i + th) + 1):
            row[j] = min(prev[j - 1] + (t[i - 1] != u[j - 1]), prev[j] + 1, row[j - 1] + 1)
    return B


def band_cells(a, b, th):
    return a * min(b, 2 * th + 1)


def decide(a, b, dist, t0=T0, band_cap=BAND_CAP):
    """(aligned, attempts, the attempts' band cells) of a pair with two core
    sides above the cap whose true distance is dist."""
    first = lambda x: next(k for k in range(64) if t0 << k >= x)
    k_lo, k_star = first(abs(a - b)), first(dist)
    if a * b <= band_cap:
        k_hi = FOREVER
    else:
        k_hi = max((k for k in range(64) if band_cells(a, b, t0 << k) <= band_cap), default=-1)
    tried = range(k_lo, min(k_star, k_hi) + 1)
    return k_star <= k_hi, len(tried), sum(band_cells(a, b, t0 << k) for k in tried)


def band_pair(T, Q, cells_cap=CELLS_CAP, t0=T0, band_cap=BAND_CAP, full=align_util.align_pair):
    """(align_pair's result with the band on, over, banded, attempts, cells)."""
    r = full(T, Q, cells_cap)
    if not r["status"]:
        return r, 0, 0, 0, 0
    a, b = len(T) - r["prefix"] - r["suffix"], len(Q) - r["prefix"] - r["suffix"]
    if not a or not b:
        return full(T, Q, UNLIMITED), 1, 1, 0, 0
    # (a band that never fits needs no distance: k_lo alone decides)
    if band_cells(a, b, t0 << next(k for k in range(64) if t0 << k >= abs(a - b))) > band_cap:
        return r, 1, 0, 0, 0
    whole = full(T, Q, UNLIMITED)
    ok, attempts, cells = decide(a, b, whole["distance"], t0, band_cap)
    return (whole if ok else r), 1, int(ok), attempts, cells


def reference_align_band(ref, seqs, cells_cap=CELLS_CAP, t0=T0, band_cap=BAND_CAP):
    """align_util.reference_align's tables with the band on, plus "band":
    n_over, n_banded, n_attempts, band_cells and every pair's attempts."""
    full = align_util.align_pair
    sums, per_pair = [0, 0, 0, 0], []

    def pair(T, Q, cap=CELLS_CAP):
        r, *figures = band_pair(T, Q, cap, t0, band_cap, full)
        for k, v in enumerate(figures):
            sums[k] += v
        per_pair.append(figures[2])
        return r
    try:
        align_util.align_pair = pair
        res = reference_align(ref, seqs, cells_cap)
    finally:
        align_util.align_pair = full
    res["band"] = dict(n_over=sums[0], n_banded=sums[1], n_attempts=sums[2], band_cells=sums[3], attempts=per_pair)
    return res


def figures_of(whole, cells_cap=CELLS_CAP, t0=T0, band_cap=BAND_CAP):
    """(n_over, n_banded, n_attempts, band_cells, every pair's attempts, every
    pair's status) with the band on, from reference_align's result at an
    unlimited cells_cap, which has every pair's distance."""
    sums, per_pair, status = [0, 0, 0, 0], [], []
    for (a, b), d in zip(cores_of(whole), whole["distance"]):
        figures = (0, 0, 0, 0)
        if (a + 1) * (b + 1) > cells_cap:
            figures = (1, 1, 0, 0) if not a or not b else (1,) + tuple(int(x) for x in decide(a, b, d, t0, band_cap))
        sums = [x + y for x, y in zip(sums, figures)]
        per_pair.append(figures[2])
        status.append(figures[0] - figures[1])
    return tuple(sums) + (per_pair, status)


def check_align_band(ctx, rows, rec_group, G, min_genomes, names, seqs, ref_group=None, cells_cap=CELLS_CAP, t0=T0,
                     band_cap=BAND_CAP):
    """align_util.check_align with the band on (the caller has set the tunes):
    the device against reference_align_band, exactly, and the four counts of
    region_align_band().  Returns (res, tsv, VCF body)."""
    ref = reference_variants(rows, rec_group, G, min_genomes, seqs, ref_group)
    res = reference_align_band(ref, seqs, cells_cap, t0, band_cap)
    ctx.region_bubbles(rec_group, G, min_genomes, rows=rows)
    ctx.region_variants(rec_group, G, ref_group, rows=rows)
    counts = ctx.region_align()
    assert counts == (res["n_pairs"], res["n_aligned"], res["n_ops_all"], res["n_prims_all"], res["n_lines"])
    tsv, vcf = assert_same(ctx, res, names, seqs)
    band = res["band"]
    assert ctx.region_align_band()[:4] == (band["n_over"], band["n_banded"], band["n_attempts"], band["band_cells"])
    return res, tsv, vcf


def cores_of(res):
    return [(n - p - q, m - p - q) for n, m, p, q in zip(res["t_len"], res["q_len"], res["prefix"], res["suffix"])]

