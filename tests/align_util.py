"""An independent reference of the alleles' alignments for the tests: plain
Python lists on top of variants_util.reference_variants (nothing shared with
pangenome_amd/), both texts, and the comparison every test uses.

Definition (stated here on its own, not copied from include/pangenome.h):
every site has a target T - a placed site's is the reference record's letters
[pos0, pos0 + ref_len) and its ref_allele is skipped, any other site's is the
sequence of its allele 0, which is skipped - and every other allele of the site
is a query Q; pairs come by site, then allele.  The common suffix is trimmed
first (q letters), then the common prefix (p letters) of what is left; the
cores t and u have a and b letters.  D[i][0] = i, D[0][j] = j, D[i][j] =
min(D[i-1][j-1] + (t[i-1] != u[j-1]), D[i-1][j] + 1, D[i][j-1] + 1).  The path
goes back from (a, b): diagonal (`=` or `X`) if i, j > 0 and D[i][j] is the
diagonal's value, else `D` if i > 0 and D[i][j] == D[i-1][j] + 1, else `I`.
The CIGAR is p `=`, the core's runs, q `=`, empty runs left out.  A pair with
(a + 1)(b + 1) > cells_cap is not aligned: status 1, `aD bI`, no distance, one
REPL primitive.  Primitives: every X column an SNV, every D run a DEL, every I
run an INS, in target order.  The primitives of a placed site with equal
(tpos, type, tlen, qlen) and equal query letters are one line; lines come by
(record, pos, site, type, tlen, qlen, first primitive)."""
import hashlib
import json
import os

import numpy as np

from golden_util import GOLDEN
from variants_util import reference_variants

SNV, DEL, INS, REPL = 0, 1, 2, 3
CELLS_CAP = 1 << 24
NUMPY_FROM = 100_000                                     # cells from which D is filled by anti-diagonals
NO_DISTANCE = 2 ** 64 - 1
PAIR_COLS = ("site", "allele", "placed", "t_len", "q_len", "prefix", "suffix", "status", "distance", "n_eq", "n_sub",
             "n_ins", "n_del", "op_off", "n_ops", "prim_off", "n_prims")
PRIM_COLS = ("pair", "type", "tpos", "qpos", "tlen", "qlen")
LINE_COLS = ("site", "pos", "type", "tpos", "tlen", "qlen", "first_prim", "ac", "n_genomes", "bits")
TSV_HEADER = b"#from\tto\tallele\ttarget\ttlen\tqlen\tprefix\tsuffix\tdist\teq\tsub\tins\tdel\tcigar\n"
VCF_NS = b'##INFO=<ID=NS,Number=1,Type=Integer,Description="Genomes with an allele at the site">\n'
VCF_AC = b'##INFO=<ID=AC,Number=1,Type=Integer,Description="Alleles of the site that carry the difference">\n'
VCF_GT = (b'##FORMAT=<ID=GT,Number=.,Type=String,Description="1: an allele of the site in the genome carries the '
          b'difference, 0: one does not, 0/1: both, unphased; . if the genome has no allele">\n')


def trim(T, Q):
    """(p, q): the suffix first."""
    lim, q, p = min(len(T), len(Q)), 0, 0
    while q < lim and T[len(T) - 1 - q] == Q[len(Q) - 1 - q]:
        q += 1
    while p < lim - q and T[p] == Q[p]:
        p += 1
    return p, q


def matrix(t, u):
    """D as a list of rows, or as an array for a large core."""
    a, b = len(t), len(u)
    if (a + 1) * (b + 1) < NUMPY_FROM:
        D = [list(range(b + 1))]
        for i in range(1, a + 1):
            prev, row = D[-1], [i] + [0] * b
            for j in range(1, b + 1):
                row[j] = min(prev[j - 1] + (t[i - 1] != u[j - 1]), prev[j] + 1, row[j - 1] + 1)
            D.append(row)
        return D
    ta, ua = np.frombuffer(bytes(t), np.uint8), np.frombuffer(bytes(u), np.uint8)
    D = np.zeros((a + 1, b + 1), np.int64)
    D[:, 0] = np.arange(a + 1)
    D[0, :] = np.arange(b + 1)
    for d in range(2, a + b + 1):
        i = np.arange(max(1, d - b), min(a, d - 1) + 1)
        j = d - i
        D[i, j] = np.minimum(np.minimum(D[i - 1, j - 1] + (ta[i - 1] != ua[j - 1]), D[i - 1, j] + 1), D[i, j - 1] + 1)
    return D


def walk(D, t, u):
    """The core's ops from (0, 0) to (a, b), one letter per column."""
    i, j, ops = len(t), len(u), []
    while i or j:
        if i and j and D[i][j] == D[i - 1][j - 1] + (t[i - 1] != u[j - 1]):
            ops.append("=" if t[i - 1] == u[j - 1] else "X")
            i, j = i - 1, j - 1
        elif i and D[i][j] == D[i - 1][j] + 1:
            ops.append("D")
            i -= 1
        else:
            ops.append("I")
            j -= 1
    return ops[::-1]


def runs_of(ops):
    out = []
    for c in ops:
        if out and out[-1][0] == c:
            out[-1][1] += 1
        else:
            out.append([c, 1])
    return [(c, n) for c, n in out]


def align_pair(T, Q, cells_cap=CELLS_CAP):
    """One pair: prefix, suffix, status, distance, the runs over all of T and
    Q, the primitives (type, tpos, qpos, tlen, qlen) and the four sums."""
    p, q = trim(T, Q)
    t, u = T[p:len(T) - q], Q[p:len(Q) - q]
    a, b = len(t), len(u)
    ends = lambda core: ([("=", p)] if p else []) + core + ([("=", q)] if q else [])
    if (a + 1) * (b + 1) > cells_cap:
        core = ([("D", a)] if a else []) + ([("I", b)] if b else [])
        return dict(prefix=p, suffix=q, status=1, distance=NO_DISTANCE, runs=ends(core), prims=[(REPL, p, p, a, b)],
                    n_eq=p + q, n_sub=0, n_ins=b, n_del=a)
    D = matrix(t, u)
    core = runs_of(walk(D, t, u))
    prims, tp, qp = [], p, p
    for c, n in core:
        if c == "X":
            prims += [(SNV, tp + x, qp + x, 1, 1) for x in range(n)]
        elif c == "D":
            prims.append((DEL, tp, qp, n, 0))
        elif c == "I":
            prims.append((INS, tp, qp, 0, n))
        tp += n if c != "I" else 0
        qp += n if c != "D" else 0
    count = lambda c: sum(n for x, n in core if x == c)
    return dict(prefix=p, suffix=q, status=0, distance=int(D[a][b]), runs=ends(core), prims=prims,
                n_eq=p + q + count("="), n_sub=count("X"), n_ins=count("I"), n_del=count("D"))


def apply_prims(T, Q, prims):
    """T with the primitives applied (the tests: it must be Q)."""
    out, at = [], 0
    for _, tpos, qpos, tlen, qlen in prims:
        out += [T[at:tpos], Q[qpos:qpos + qlen]]
        at = tpos + tlen
    return b"".join(out + [T[at:]])


def reference_align(ref, seqs, cells_cap=CELLS_CAP):
    """Every table of the alignment of reference_variants' result ref."""
    bub, G = ref["bubbles"], ref["G"]
    placed = {s: (rec, pos0, k0, n) for s, rec, pos0, k0, n in zip(ref["site"], ref["placed_record"], ref["pos0"],
                                                                   ref["ref_allele"], ref["ref_len"])}
    out = {k: [] for k in PAIR_COLS + PRIM_COLS}
    out.update(op=[], len=[], T=[], Q=[], G=G, ref=ref, placed_at=placed)
    for s in range(bub["n_sites"]):
        first, nal = bub["site_first"][s], bub["site_alleles"][s]
        if s in placed:
            rec, pos0, skip, n = placed[s]
            T = seqs[rec][pos0:pos0 + n]
        else:
            T, skip = ref["seqs"][first], 0
        for k in range(nal):
            if k == skip:
                continue
            Q = ref["seqs"][first + k]
            r = align_pair(T, Q, cells_cap)
            row = dict(site=s, allele=k, placed=int(s in placed), t_len=len(T), q_len=len(Q), prefix=r["prefix"],
                       suffix=r["suffix"], status=r["status"], distance=r["distance"], n_eq=r["n_eq"],
                       n_sub=r["n_sub"], n_ins=r["n_ins"], n_del=r["n_del"], op_off=len(out["op"]),
                       n_ops=len(r["runs"]), prim_off=len(out["pair"]), n_prims=len(r["prims"]))
            j = len(out["site"])
            for key in PAIR_COLS:
                out[key].append(row[key])
            out["op"] += [ord(c) for c, _ in r["runs"]]
            out["len"] += [n for _, n in r["runs"]]
            for prim in r["prims"]:
                for key, v in zip(PRIM_COLS, (j,) + prim):
                    out[key].append(v)
            out["T"].append(T)
            out["Q"].append(Q)
    # the lines of the placed sites
    groups = {}
    for i, j in enumerate(out["pair"]):
        s = out["site"][j]
        if s not in placed:
            continue
        letters = out["Q"][j][out["qpos"][i]:out["qpos"][i] + out["qlen"][i]]
        key = (s, out["tpos"][i], out["type"][i], out["tlen"][i], out["qlen"][i], letters)
        groups.setdefault(key, []).append(i)
    lines = []
    for (s, tpos, typ, tlen, qlen, _), members in groups.items():
        rec, pos0 = placed[s][:2]
        carriers = sorted(bub["site_first"][s] + out["allele"][out["pair"][i]] for i in members)
        assert len(set(carriers)) == len(carriers)
        bits = [0] * ((G + 63) // 64)
        for al in carriers:
            bits = [x | y for x, y in zip(bits, bub["bits"][al])]
        lines.append(dict(record=rec, pos=pos0 + tpos + (typ == SNV), site=s, type=typ, tlen=tlen, qlen=qlen,
                          first_prim=min(members), tpos=tpos, ac=len(members), carriers=carriers, bits=bits,
                          n_genomes=sum(bin(x).count("1") for x in bits)))
    lines.sort(key=lambda x: (x["record"], x["pos"], x["site"], x["type"], x["tlen"], x["qlen"], x["first_prim"]))
    out["lines"] = lines
    out.update(n_pairs=len(out["site"]), n_aligned=out["status"].count(0), n_ops_all=len(out["op"]),
               n_prims_all=len(out["pair"]), n_lines=len(lines))
    return out


def cigar(res, j):
    k0, n = res["op_off"][j], res["n_ops"][j]
    return b"".join(b"%d%c" % (res["len"][k], res["op"][k]) for k in range(k0, k0 + n)) or b"*"


def reference_tsv(res):
    bub, out = res["ref"]["bubbles"], [TSV_HEADER]
    for j, s in enumerate(res["site"]):
        out.append(b"\t".join(
            [b"%d" % bub["site_from"][s], b"%d" % bub["site_to"][s], b"%d" % res["allele"][j],
             b"ref" if res["placed"][j] else b"0", b"%d" % res["t_len"][j], b"%d" % res["q_len"][j],
             b"%d" % res["prefix"][j], b"%d" % res["suffix"][j], b"." if res["status"][j] else b"%d" % res["distance"][j],
             b"%d" % res["n_eq"][j], b"%d" % res["n_sub"][j], b"%d" % res["n_ins"][j], b"%d" % res["n_del"][j],
             cigar(res, j)]) + b"\n")
    return b"".join(out)


def reference_primitives_vcf(res, names, seqs):
    """The body: one line per merged primitive."""
    bub, G, out = res["ref"]["bubbles"], res["G"], []
    for ln in res["lines"]:
        s, i, rec = ln["site"], ln["first_prim"], ln["record"]
        pos0, tpos = res["placed_at"][s][1], ln["tpos"]
        Q = res["Q"][res["pair"][i]]
        alt = Q[res["qpos"][i]:res["qpos"][i] + ln["qlen"]]
        if ln["type"] == SNV:
            REF, ALT = seqs[rec][pos0 + tpos:pos0 + tpos + 1], alt
        else:
            anchor = seqs[rec][pos0 + tpos - 1:pos0 + tpos]
            REF, ALT = anchor + seqs[rec][pos0 + tpos:pos0 + tpos + ln["tlen"]], anchor + alt
        cells = []
        for g in range(G):
            have = [al for al in range(bub["site_first"][s], bub["site_first"][s] + bub["site_alleles"][s])
                    if (bub["bits"][al][g // 64] >> (g % 64)) & 1]
            carry = [al for al in have if al in ln["carriers"]]
            cells.append(b"/".join(([b"0"] if len(have) > len(carry) else []) + ([b"1"] if carry else [])) or b".")
        out.append(b"\t".join([bytes(names[rec]), b"%d" % ln["pos"], b"%d_%d" % (bub["site_from"][s], bub["site_to"][s]),
                               REF, ALT, b".", b".", b"NS=%d;AC=%d" % (bub["site_genomes"][s], ln["ac"]), b"GT"] +
                              cells) + b"\n")
    return b"".join(out)


def reference_header(ref_name, contigs, genome_names):
    out = [b"##fileformat=VCFv4.2\n", b"##source=pangenome_amd\n", b"##reference=" + bytes(ref_name) + b"\n"]
    out += [b"##contig=<ID=%s,length=%d>\n" % (bytes(i), n) for i, n in contigs]
    cols = [b"#CHROM", b"POS", b"ID", b"REF", b"ALT", b"QUAL", b"FILTER", b"INFO", b"FORMAT"]
    return b"".join(out) + VCF_NS + VCF_AC + VCF_GT + b"\t".join(cols + [bytes(x) for x in genome_names]) + b"\n"


def device_state(ctx, names, G):
    """Everything the context holds after region_align(), as lists and bytes."""
    return ([{k: v.tolist() for k, v in t.items()} for t in (ctx.region_align_pairs(), ctx.region_align_ops(),
                                                             ctx.region_align_prims(), ctx.region_align_lines(G))],
            ctx.region_align_text(), ctx.region_primitives_vcf_text(names))


def assert_same(ctx, res, names, seqs):
    """The exports and both texts of the context against res, exactly."""
    got = ctx.region_align_pairs()
    assert list(got) == list(PAIR_COLS)
    for k in PAIR_COLS:
        assert got[k].dtype == np.uint64 and got[k].tolist() == res[k], k
    got = ctx.region_align_ops()
    assert got["op"].dtype == np.uint8 and got["op"].tolist() == res["op"]
    assert got["len"].dtype == np.uint64 and got["len"].tolist() == res["len"]
    got = ctx.region_align_prims()
    assert list(got) == list(PRIM_COLS)
    for k in PRIM_COLS:
        assert got[k].dtype == (np.uint8 if k == "type" else np.uint64) and got[k].tolist() == res[k], k
    got = ctx.region_align_lines(res["G"])
    assert list(got) == list(LINE_COLS)
    for k in LINE_COLS:
        assert got[k].tolist() == [ln[k] for ln in res["lines"]], k
    tsv, vcf = ctx.region_align_text(), ctx.region_primitives_vcf_text(names)
    assert tsv == reference_tsv(res)
    assert vcf == reference_primitives_vcf(res, names, seqs)
    return tsv, vcf


def check_align(ctx, rows, rec_group, G, min_genomes, names, seqs, ref_group=None, rows_on_device=False,
                cells_cap=CELLS_CAP):
    """region_bubbles(), region_variants() and region_align() on the device
    against reference_align, exactly: the five returned counts, the four
    tables and both texts.  Returns (res, tsv, VCF body)."""
    ref = reference_variants(rows, rec_group, G, min_genomes, seqs, ref_group)
    res = reference_align(ref, seqs, cells_cap)
    pass_rows = None if rows_on_device else rows
    ctx.region_bubbles(rec_group, G, min_genomes, rows=pass_rows)
    ctx.region_variants(rec_group, G, ref_group, rows=pass_rows)
    counts = ctx.region_align()
    assert counts == (res["n_pairs"], res["n_aligned"], res["n_ops_all"], res["n_prims_all"], res["n_lines"])
    tsv, vcf = assert_same(ctx, res, names, seqs)
    return res, tsv, vcf


def check_properties(res):
    """What follows from the definition, pair by pair: the core's first and
    last ops are never `=`, no D run touches an I run, the primitives applied
    to T give Q, and their lengths sum to the distance."""
    for j in range(res["n_pairs"]):
        k0, n = res["op_off"][j], res["n_ops"][j]
        ops = [(chr(res["op"][k]), res["len"][k]) for k in range(k0, k0 + n)]
        p, q = res["prefix"][j], res["suffix"][j]
        core = ops[1 if p else 0:len(ops) - (1 if q else 0)]
        assert (not p or ops[0] == ("=", p)) and (not q or ops[-1] == ("=", q))
        assert all(n > 0 for _, n in ops) and all(x[0] != y[0] for x, y in zip(ops, ops[1:]))
        assert sum(n for c, n in ops if c != "I") == res["t_len"][j]
        assert sum(n for c, n in ops if c != "D") == res["q_len"][j]
        r0, rn = res["prim_off"][j], res["n_prims"][j]
        prims = [tuple(res[k][i] for k in PRIM_COLS[1:]) for i in range(r0, r0 + rn)]
        assert apply_prims(res["T"][j], res["Q"][j], prims) == res["Q"][j]
        if res["status"][j]:
            continue
        assert not core or (core[0][0] != "=" and core[-1][0] != "=")
        assert all({x[0], y[0]} != {"D", "I"} for x, y in zip(core, core[1:]))
        assert sum(max(tl, ql) for _, _, _, tl, ql in prims) == res["distance"][j]


def check_vcf(res, vcf, names, seqs):
    """What a VCF reader relies on: one line per line entry, sorted by
    (record, POS), every REF equal to the record's letters at POS, and REF and
    ALT sharing their first letter except in SNVs."""
    lines = vcf.split(b"\n")[:-1]
    assert len(lines) == res["n_lines"]
    keys = []
    for ln in lines:
        f = ln.split(b"\t")
        rec, pos = [bytes(x) for x in names].index(f[0]), int(f[1])
        assert pos >= 1 and seqs[rec][pos - 1:pos - 1 + len(f[3])] == f[3]
        if len(f[3]) == 1 and len(f[4]) == 1:
            assert f[3] != f[4]
        else:
            assert f[3][:1] == f[4][:1] and b"," not in f[4]
        assert len(f) == 9 + res["G"]
        keys.append((rec, pos))
    assert keys == sorted(keys)


def summary(res, ids, seqs):
    """The figures tests/golden/align/*.json record."""
    by_type = [res["type"].count(t) for t in (SNV, DEL, INS, REPL)]
    return {"n_pairs": res["n_pairs"], "n_aligned": res["n_aligned"], "n_ops": res["n_ops_all"],
            "n_prims": dict(zip(("snv", "del", "ins", "repl"), by_type)), "n_lines": res["n_lines"],
            "sum_distance": sum(d for d, st in zip(res["distance"], res["status"]) if not st),
            "tsv_sha256": hashlib.sha256(reference_tsv(res)).hexdigest(),
            "vcf_sha256": hashlib.sha256(reference_primitives_vcf(res, ids, seqs)).hexdigest()}


def golden(name):
    return json.load(open(os.path.join(GOLDEN, "align", name + ".json")))


def assert_files(prefix, res, ids, seqs, ref_name, contigs, genome_names):
    """The two files `-A 1` writes."""
    assert open(prefix + "_fr_align.tsv", "rb").read() == reference_tsv(res)
    assert open(prefix + "_fr_primitives.vcf", "rb").read() == (reference_header(ref_name, contigs, genome_names) +
                                                                  reference_primitives_vcf(res, ids, seqs))
    assert not [f for f in os.listdir(os.path.dirname(prefix)) if f.endswith(".tmp")]
