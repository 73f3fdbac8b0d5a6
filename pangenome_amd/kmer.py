"""Drop-in for kmer_numba.py's k-mer -> dBG -> rdBG -> region-table path.

Same names, arguments and side files as the reference; every per-base step
runs in libpangenome_hip.so on an MI355X (pangenome_amd/csrc).  Mirrors:

  seq_chk      kmer_numba.py:873-885     file type sniffing
  seq2bytes    :117-119                  memory-map the input
  seq2rdbg     :1234-1268                dBG build (K1 parse + K3 insert)
  dbg2rdbg     :1313-1321                rdBG (K5 degree scan + compaction)
  seq2graph    :1853-1951                edges -> .xyz -> mcl -> labels -> rows
  dump / load_on_disk  :243-335         `<in>_db.npz` (oakht slot layout)
  entry_point  :1971-2146                CLI (-i -k -n -c -r -d -R -D; ours: -a -w -g -p -l -s -v -b -V -A -L -T -B -K)

Usage:  python -m pangenome_amd -i genomes.fa -k 27 > result.tab
"""
from __future__ import annotations

import mmap
import os
import sys
from time import time

import numpy as np

from collections.abc import Mapping

from . import host
from ._lib import PG_TUNE_ALIGN_BAND, Context, format_xyz


class LabelTable(Mapping):
    """seq2graph's label dictionary {(key, value): label} (:1918-1944), kept as
    arrays (or on the device, fetched by `loader` when first needed); the
    Python dict is built only if it is looked into."""

    def __init__(self, keys=None, vals=None, ids=None, loader=None):
        self._arrays = None if loader is not None else (keys, vals, ids)
        self._loader = loader
        self._d = None

    @property
    def keys_(self):
        return self._get()[0]

    @property
    def vals_(self):
        return self._get()[1]

    @property
    def ids_(self):
        return self._get()[2]

    def _get(self):
        if self._arrays is None:
            self._arrays = self._loader()
            self._loader = None
        return self._arrays

    def _dict(self):
        if self._d is None:
            k = self.keys_.view(np.uint64).tolist()
            self._d = dict(zip(zip(k, self.vals_.tolist()), self.ids_.tolist()))
        return self._d

    def __getitem__(self, key):
        return self._dict()[key]

    def __iter__(self):
        return iter(self._dict())

    def __len__(self):
        return int(self.ids_.shape[0])


# --------------------------------------------------------------- input files
def seq_chk(qry):
    """:873-885 — 'fasta' if a header starts the first 40 characters."""
    with open(qry, "r") as f:
        seq = f.read(2 * 20)
    if seq[0].startswith(">") or "\n>" in seq:
        return "fasta"
    if seq[0].startswith("@") or "\n@" in seq:
        return "fastq"
    return None


def seq2bytes(fn, populate=True):
    """:117-119 (read-only here: nothing is written back to the input).  The
    mapping's page tables are filled when it is made (MAP_POPULATE: one pass
    in the kernel, ~8 ms per GB of page-cache-warm file), so the staging
    threads that copy it to the GPU never stop on a page fault (demand faults
    from 8 threads at once took 3.7 s for C4's 5 GB)."""
    if not os.path.getsize(fn):
        return np.zeros(0, np.uint8)
    flags = mmap.MAP_SHARED | (getattr(mmap, "MAP_POPULATE", 0) if populate else 0)
    with open(fn, "rb") as f:
        mm = mmap.mmap(f.fileno(), 0, flags=flags, prot=mmap.PROT_READ)
    return np.frombuffer(mm, dtype=np.uint8)


def populate(buf, start: int, end: int):
    """Fill the page tables of bytes [start, end) of a seq2bytes(...,
    populate=False) mapping (madvise MADV_POPULATE_READ, Linux 5.14+;
    silently nothing elsewhere)."""
    mm = getattr(buf, "base", None)
    if not isinstance(mm, mmap.mmap) or end <= start:
        return
    a = start - start % mmap.PAGESIZE
    try:
        mm.madvise(22, a, end - a)                       # MADV_POPULATE_READ
    except (OSError, ValueError, AttributeError):
        pass


class DeviceGraph:
    """The device-resident dBG/rdBG of one input (what the reference keeps in
    its `oakht` tables), plus the parsed record table the later passes reuse.
    With `build_rc` set, the input is parsed and its dBG built in one call
    (pg_build_host: the build's first stage streamed under the upload), for a
    pass that inserts every record; otherwise it is only parsed."""

    def __init__(self, qry, kmer, device=0, data=None, build_rc=None, ctx=None):
        self.qry = qry
        self.k = min(max(1, int(kmer)), 27)                    # :1236
        self.buf = seq2bytes(qry) if data is None else data
        self.ctx = ctx if ctx is not None else Context(self.k, device)
        self.stats = None
        if build_rc is None:
            self.ctx.parse_host(self.buf)        # H2D in chunks, pipelined with K1
        else:
            self.stats = self.ctx.build_host(self.buf, bool(build_rc))
        rec = self.ctx.records()
        self.seq_len, self.hdr_start, self.hdr_len = rec["seq_len"], rec["hdr_start"], rec["hdr_len"]
        self.rec_ptr = rec["ptr"]
        self.shape = host.FileShape.from_bytes(self.buf, self.hdr_start, self.hdr_len)
        self.reduced = False
        self.dbg_flags = None                    # the record flags of the dBG pass (seq2rdbg; -K walks the same records)

    @property
    def size(self):
        return self.stats.n_dbg if self.stats else 0

    def dbg_items(self):
        """(keys, masks) sorted by key — dump()'s content (:243-261)."""
        return self.ctx.dbg()

    def rdbg_keys(self):
        return self.ctx.rdbg()


# ------------------------------------------------------------------- passes
def seq2rdbg(qry, kmer=13, bits=5, Ns=1e6, chunk=2 ** 32, brkpt="./breakpoint", saved="dBG_disk",
             hashfunc=None, jit=True, rc=True, device=0, ctx=None, on_parsed=None):
    """:1234-1268.  Returns the device dBG.  An existing `brkpt` npz (-r) is
    the table so far plus the offset to resume at (:1239-1241).  When a pass
    crosses `chunk` bases the reference dumps the table so far to
    `<in>_db_brkpt.npz` (:1255-1259, each dump replacing the last); here the
    last such state is built, dumped and written once, then the whole build
    runs.  `ctx`: a Context to build in (the CLI creates it before its
    stage timer starts, so the timer excludes HIP runtime start-up).
    `on_parsed(g)`: called once the records are known and before anything is
    built (-g checks its group file there); the parse and the build are then
    two calls."""
    if seq_chk(qry) != "fasta":
        raise ValueError("%s: only FASTA input is supported (the reference's FASTQ branch is "
                         "broken, kmer_numba.py:174-186)" % qry)
    mult = 2 if rc else 1
    nbytes = os.path.getsize(qry)
    if on_parsed is None and not (brkpt and os.path.isfile(brkpt)) and nbytes * mult <= int(chunk) \
            and not host.ns_hit(nbytes * mult, int(Ns)):
        # no -r resume, and no -n limit or 2^33-base checkpoint can touch a
        # file this size (bases <= bytes): every record is in the pass, so
        # parse and build in one call with the build streamed under the upload
        g = DeviceGraph(qry, kmer, device, build_rc=bool(rc), ctx=ctx)
        flags, extra = host.plan_dbg(g.seq_len, g.shape, bool(rc), int(Ns), int(chunk))
        if extra or not flags.all():                      # (cannot happen: bases <= bytes)
            g.stats = g.ctx.build_dbg(flags, extra, bool(rc))
        g.dbg_flags = flags
        return g
    g = DeviceGraph(qry, kmer, device, ctx=ctx)
    if on_parsed is not None:
        on_parsed(g)
    resume = None
    if brkpt and os.path.isfile(brkpt):
        offset, keys, values, counts = host.read_db_npz(brkpt)
        g.ctx.dbg_load(keys, values, counts)
        resume = host.resume_position(offset, g.rec_ptr)
    flags, extra, ckpt = host.plan_dbg(g.seq_len, g.shape, bool(rc), int(Ns), int(chunk), resume=resume,
                                       checkpoint=True)
    if ckpt is not None:
        cf, ce, last = ckpt
        g.ctx.build_dbg(cf, ce, bool(rc))
        # the checkpoint file streamed from the device (pg_dbg_dump_fd: no
        # host copy of the slot arrays; C4: ~2.7 GB of them), then the pass
        cap, size = g.ctx.dbg_dump_size()
        host.write_db_npz_from(qry + "_db_brkpt", cap, size, lambda fd, offs: g.ctx.dbg_dump_fd(fd, offs, cap),
                               offset=int(g.rec_ptr[last]))
    g.stats = g.ctx.build_dbg(flags, extra, bool(rc))
    g.dbg_flags = flags
    return g


def dump(g: DeviceGraph, fn="./tmp"):
    """:243-261 — `fn`.npz as an oakht the reference's load_on_disk accepts."""
    cap, size = g.ctx.dbg_dump_size()
    host.write_db_npz_from(fn, cap, size, lambda fd, offs: g.ctx.dbg_dump_fd(fd, offs, cap))
    return 0


def load_graph(qry, kmer, fn, device=0, rdbg=False, rc=True, on_parsed=None):
    """load_on_disk (:289-335) into a device graph over `qry`: -d (a dBG,
    reduced next) or -D (rdBG keys: staged with mask 0, so every key passes
    the rdBG rule and membership is exactly the file's key set)."""
    _, keys, values, counts = host.read_db_npz(fn)
    g = DeviceGraph(qry, kmer, device)
    if on_parsed is not None:
        on_parsed(g)
    g.ctx.dbg_load(keys, None if rdbg else values, counts)
    g.stats = g.ctx.build_dbg(np.zeros(g.seq_len.shape[0], np.uint8), 0, bool(rc))
    return g


def dbg2rdbg(kmer_dict):
    """:1313-1321.  Reduces in place on the device and returns the same graph."""
    kmer_dict.stats = kmer_dict.ctx.build_rdbg()
    kmer_dict.reduced = True
    return kmer_dict


def rdbg_edges(g: DeviceGraph, Ns, chunk, rc, brkpt="", keep_on_device=False):
    """Edge Dict of rdbg_edge_weight_jit_ (:1808-1827) in its iteration order;
    an existing `brkpt` (-R) is the Dict so far and the offset to resume at.
    With keep_on_device and neither a -R resume nor a checkpoint (the order is
    then the device's first-occurrence order), the edges stay on the device
    and None is returned."""
    loaded, resume = None, None
    if brkpt and os.path.isfile(brkpt):
        offset, lt, lc = host.read_edge_npz(brkpt)
        loaded, resume = (lt, lc), host.resume_position(offset, g.rec_ptr)
    flags, segment, ncp, ckpt = host.plan_edges(g.seq_len, g.shape, int(Ns), int(chunk), resume=resume,
                                                checkpoint=True)
    if keep_on_device and loaded is None and ncp == 0:
        g.ctx.edges_count(flags, bool(rc))
        return None

    def state(fl, upto):                          # the Dict after segments 0..upto, in iteration order
        tuples, counts, walk_first = g.ctx.edges(fl, bool(rc))
        if loaded is not None:
            return host.merge_edges(loaded[0], loaded[1], tuples, counts, walk_first, segment, upto)
        order = host.edge_order(walk_first, segment, upto)
        return tuples[order], counts[order]
    if ckpt is not None:
        # the last `<in>_rdb_brkpt.npz` dump (:1880-1887): the Dict after the
        # segments before the last checkpoint, each dump replacing the last
        last_seg = ncp - 1
        t, c = state((flags.astype(bool) & (segment <= last_seg)).astype(np.uint8), last_seg)
        host.write_edge_npz(g.qry + "_rdb_brkpt", t, c, int(g.rec_ptr[ckpt]))
    return state(flags, ncp)


def seq2graph(qry, kmer=13, bits=5, Ns=1e6, brkpt="./breakpoint_rdbg.npz", rdbg_dict=None, saved=None,
              hashfunc=None, jit=True, chunk=2 ** 33, rc=False, cluster=True, out=None, min_weight=1, groups=None,
              orders=0, links=False, seqs=False, inflation2=3, sites=False, bubbles=0, variants="", align=False,
              align_band=False, tree=False, boot=0, kmers=False, rc0=True):
    """:1853-1951: edge weights -> `<qry>_rdbg_weight.xyz` -> mcl (or reuse)
    -> label dictionary -> print the region rows.  The edges, the label
    table, the rows and both texts are made on the device; the host writes
    the files and runs (or reuses) mcl.  cluster="cc": instead of running
    mcl, the built-in clusterer (pg_cluster_cc: edges lighter than min_weight
    dropped, connected components of the rest) writes the `.mcl`; an existing
    `.mcl` is reused either way.  cluster="markov": the built-in Markov
    clustering (pg_cluster_markov on the device edges where they lie: edges
    lighter than min_weight dropped, inflation inflation2 / 2, 64 entries per
    column, at most 200 iterations) writes the `.mcl` the same way; a run
    that reaches the cap prints one `# -a markov: not converged` line before
    the rows.  min_weight="auto" (with cluster="cc"): the
    cluster curve of the `.xyz` over host.sweep_thresholds is made first
    (pg_cluster_sweep, on the device edges where they lie), written as
    `<qry>_rdbg_weight.xyz.sweep.tsv`, and host.sweep_choice's threshold is
    the weight cut.  groups (-g; "record" or a `seqid<TAB>genome`
    file): after the rows are written, their frequency table is made where
    they lie on the device (pg_freq) and the four `<qry>_fr_*` files written;
    nothing more is printed.  orders (-p, with groups): the genomes are then
    compared on the device table (pg_freq_compare) over that many genome
    orders and four more `<qry>_fr_*` files written.  links (-l, with groups):
    the region graph of the device rows (pg_region_graph) is made with the
    same genomes and its four `<qry>_fr_*` files written.  seqs (-s, with
    groups): one representative sequence per label is decoded on the device
    (pg_region_seqs) and `<qry>_fr_regions.fa`, `_fr_regions.tsv` and, with
    links, `_fr_graph_seq.gfa` written.  sites (-v, with groups): the variable
    sites of the device rows (pg_region_sites) are made with the same genomes
    and `<qry>_fr_sites.tsv`, `_fr_sites_genomes.tsv` and `_fr_sites.npz`
    written.  bubbles (-b, with groups; 0: off): the variable sites between
    anchor regions - labels carried by that many genomes, at most all of them
    - are made the same way (pg_region_bubbles) and `<qry>_fr_bubbles.tsv`,
    `_fr_bubbles_genomes.tsv` and `_fr_bubbles.npz` written.  variants (-V,
    with bubbles; "": off): a genome's name; the bases of every allele are
    decoded and the sites placed on that genome's walks (pg_region_variants),
    and `<qry>_fr_alleles.fa`, `_fr_alleles.tsv` and `_fr_variants.vcf` written.
    align (-A, with variants): every allele is then aligned against its
    site's reference on the device (pg_region_align) and `<qry>_fr_align.tsv`
    and `_fr_primitives.vcf` written.  align_band (-L, with align): the pairs
    above pg_region_align's cells cap are aligned in a band of diagonals
    (PG_TUNE_ALIGN_BAND) instead of standing as one replacement; the same two
    files.  tree (-T, with groups): after the frequency and the comparison
    files a neighbour-joining tree of the genomes is built on the device
    (pg_tree_nj) from the comparison's shared matrix where it lies
    (pg_freq_compare with no orders is run first if orders has not) and
    `<qry>_fr_dist.tsv`, `_fr_tree.nwk`, `_fr_tree.tsv` and `_fr_tree.npz`
    written; with align as well, a second tree from the primitive VCF lines'
    carrier bits as `<qry>_fr_vartree.nwk` and `_fr_vardist.tsv`.  boot (-B,
    with tree): that many bootstrap replicates rate every join of each tree
    (pg_tree_bootstrap) right after its files, as `<qry>_fr_tree_support.nwk`,
    `_fr_tree_support.tsv` and `_fr_tree_boot.npz`, and for the second tree
    `_fr_vartree_support.nwk` and `_fr_vartree_support.tsv`.  kmers (-K, with
    groups; rc0: the dBG's strands): last of all the dBG still in the context
    is coloured (pg_kmer_colors: the genomes of every k-mer, over the records
    the dBG pass inserted) and the `<qry>_km_*` files written (write_kmers);
    nothing is printed and no other file changes."""
    out = out or sys.stdout
    g = rdbg_dict
    res = rdbg_edges(g, Ns, chunk, rc, brkpt=brkpt, keep_on_device=True)
    oname = qry + "_rdbg_weight.xyz"
    with open(oname, "wb") as f:                      # "%d_%d\t%d_%d\t%d\n" (:1893-1904)
        if res is None:
            f.flush()
            g.ctx.edges_write(f.fileno())             # formatted on the device, streamed into the file
        else:
            f.write(format_xyz(*res))
    if cluster == "cc" and min_weight == "auto":
        # -w auto: the cluster curve of the `.xyz` just written, its file, and the weight cut it points to
        if res is None:
            table = g.ctx.cluster_sweep(host.sweep_thresholds(g.ctx.cluster_weights()[1]))
        else:
            table = g.ctx.cluster_sweep(host.sweep_thresholds(int(res[1].max()) if len(res[1]) else 0), *res)
        min_weight = host.sweep_choice(table)
        host.write_sweep_file(qry, table, min_weight)
        if not os.path.isfile("%s.mcl" % oname):      # (an existing `.mcl` is reused whatever made it)
            print("# -w auto: %d" % min_weight, file=out)
    clustered = False
    if cluster:
        if os.path.isfile("%s.mcl" % oname):
            print("# the mcl has been ran", file=out)
        elif cluster == "cc":
            # the label table is made with the clusters: no .mcl parse, no labels_from_edges
            g.ctx.cluster_cc(None if res is None else res[0], None if res is None else res[1], int(min_weight))
            with open(oname + ".mcl.tmp", "wb") as f:           # (renamed when whole: the file is reused if present)
                g.ctx.clusters_write(f.fileno())
            os.replace(oname + ".mcl.tmp", oname + ".mcl")
            clustered = True
        elif cluster == "markov":
            _, _, n_iter, chaos = g.ctx.cluster_markov(None if res is None else res[0], None if res is None else res[1],
                                                       int(min_weight), int(inflation2), host.MK_SELECT, host.MK_MAX_ITER)
            with open(oname + ".mcl.tmp", "wb") as f:
                g.ctx.clusters_write(f.fileno())
            os.replace(oname + ".mcl.tmp", oname + ".mcl")
            note = host.markov_note(n_iter, chaos)
            if note:
                print(note, file=out)
            clustered = True
        else:
            out.flush()
            os.system("mcl %s --abc -I 1.5 -te 8 -o %s.mcl -q x -V all" % (oname, oname))
    if not clustered:
        with open(oname + ".mcl", "r") as f:
            mcl_text = f.read()
        mk, mv, mi, nxt = host.mcl_labels(mcl_text)              # :1918-1929
        g.ctx.labels_from_edges(None if res is None else res[0], mk, mv, mi, nxt)     # :1932-1944
    flags = host.plan_rows(g.seq_len, g.shape, g.buf, int(Ns))
    g.ctx.rows_count(flags, bool(rc))
    names = record_names(g)
    fd = _fileno(out)                                 # print('%s\t%d\t%d\t%s\t%d') (:1946-1949)
    if fd is not None:
        out.flush()
        out.buffer.flush()
        g.ctx.rows_write(names, fd)                   # formatted on the device, streamed to the descriptor
    else:
        text = g.ctx.rows_text(names)
        if text:
            if hasattr(out, "buffer"):
                out.flush()
                out.buffer.write(text)
                out.buffer.flush()
            else:
                out.write(text.decode())
    if groups:
        gnames = write_freq(g, qry, names, flags, groups)
        if orders:
            write_compare(g, qry, gnames, int(orders))
        if tree:
            write_tree(g, qry, gnames, compared=bool(orders), boot=int(boot))
        if links:
            write_region(g, qry, names, flags, groups)
        if seqs:
            write_region_seqs(g, qry, names, flags, groups, bool(links))
        if sites:
            write_sites(g, qry, names, flags, groups)
        if bubbles:
            write_bubbles(g, qry, names, flags, groups, int(bubbles))
            if variants:
                write_variants(g, qry, names, flags, groups, variants)
                if align:
                    write_align(g, qry, names, flags, groups, variants, bool(align_band))
                    if tree:
                        write_var_tree(g, qry, gnames, boot=int(boot))
        if kmers:
            write_kmers(g, qry, names, flags, groups, bool(rc0), int(orders), bool(tree))
    gen = g.ctx.label_gen
    return LabelTable(loader=lambda: g.ctx.labels(gen))           # (raises once a later label pass replaced it)


def record_names(g):
    """Every record's header line without '>' (the rows' qid)."""
    return [bytes(g.buf[int(hs) + 1:int(hs) + int(hl)]) for hs, hl in zip(g.hdr_start, g.hdr_len)]


def check_groups(g, Ns, groups, variants=""):
    """-g's group file against the records the row pass will walk (raises
    ValueError for a walked record the file does not name), and -V's name
    against the genomes (ValueError if it is none of them)."""
    _, gnames = host.assign_groups(record_names(g), host.plan_rows(g.seq_len, g.shape, g.buf, int(Ns)), groups)
    if variants:
        ref_genome(gnames, variants)


def ref_genome(gnames, name):
    """The number of -V's genome: the first genome called `name`."""
    want = name.encode() if isinstance(name, str) else bytes(name)
    for i, nm in enumerate(gnames):
        if bytes(nm) == want:
            return i
    raise ValueError("-V: no genome is called %r (%d genomes)" % (want.decode("utf-8", "replace"), len(gnames)))


def write_freq(g, qry, names, flags, groups):
    """-g: the frequency table of the row pass just run (pg_freq on the
    device rows) as `<qry>_fr_freq.tsv` (the device text), `_fr_spectrum.tsv`,
    `_fr_genomes.tsv` and `_fr_presence.npz`.  Returns the genome names."""
    rec_group, gnames = host.assign_groups(names, flags, groups)
    g.ctx.freq(rec_group, len(gnames))
    table = g.ctx.freq_table()
    table["n_groups"] = len(gnames)
    table["spectrum_labels"], table["spectrum_bp"] = g.ctx.freq_spectrum()
    table.update(g.ctx.freq_groups())

    def text(f):
        f.flush()
        g.ctx.freq_write(f.fileno())
    host.write_freq_files(qry, text, table, gnames)
    return gnames


def write_compare(g, qry, gnames, n_orders):
    """-p: the genomes compared over the frequency table just made, where it
    lies on the device (pg_freq_compare), in host.compare_orders' orders, as
    `<qry>_fr_shared.tsv`, `_fr_jaccard.tsv`, `_fr_curve.tsv` and
    `_fr_compare.npz`."""
    orders = host.compare_orders(len(gnames), n_orders)
    g.ctx.freq_compare(orders)
    pan, core = g.ctx.freq_curves()
    host.write_compare_files(qry, gnames, g.ctx.freq_shared(), orders, pan, core)


def write_tree(g, qry, gnames, compared, boot=0):
    """-T: the neighbour-joining tree of the genomes (pg_tree_nj) from the
    shared matrix of the comparison where it lies on the device - write_compare's
    (compared), or one made here over no orders - as `<qry>_fr_dist.tsv`,
    `_fr_tree.nwk`, `_fr_tree.tsv` and `_fr_tree.npz`.  boot (-B): then its
    joins rated by that many bootstrap replicates over the frequency table
    where it still lies on the device (write_tree_support)."""
    if not compared:
        g.ctx.freq_compare(None)
    g.ctx.tree_nj()
    joins, root = g.ctx.tree_joins(), g.ctx.tree_root()
    host.write_tree_files(qry, gnames, g.ctx.tree_dist(), joins, root)
    if boot:
        write_tree_support(g, qry, gnames, joins, root, boot)


def write_tree_support(g, qry, gnames, joins, root, boot, bits=None):
    """-B: the tree just built rated by `boot` bootstrap replicates
    (pg_tree_bootstrap, seed synth.DEFAULT_SEED) over the device's frequency
    table (bits None) or the host rows the tree of the differences came from,
    as host.write_tree_support_files' files."""
    from . import synth
    g.ctx.tree_bootstrap(boot, synth.DEFAULT_SEED, bits=bits, n_groups=len(gnames))
    left, right = g.ctx.tree_bootstrap_joins()
    res = {"support": g.ctx.tree_support()[0], "rep_left": left, "rep_right": right}
    host.write_tree_support_files(qry, gnames, joins, root, res, synth.DEFAULT_SEED, var=bits is not None)


def write_var_tree(g, qry, gnames, boot=0):
    """-T with -A: a second tree, from the differences: the carrier bits of
    the primitive VCF lines just written (write_align) compared as presence
    rows (pg_freq_compare, no orders; this replaces the device's comparison,
    whose files are written by now), d(g, h) = the lines carried by exactly
    one of the two genomes - a genome with no allele at a site carries none of
    its lines - as `<qry>_fr_vartree.nwk` and `_fr_vardist.tsv`."""
    G = len(gnames)
    bits = g.ctx.region_align_lines(G)["bits"]
    g.ctx.freq_compare(None, bits=bits, n_groups=G)
    g.ctx.tree_nj()
    joins, root = g.ctx.tree_joins(), g.ctx.tree_root()
    host.write_tree_files(qry, gnames, g.ctx.tree_dist(), joins, root, var=True)
    if boot:
        write_tree_support(g, qry, gnames, joins, root, boot, bits=bits)


def write_kmers(g, qry, names, flags, groups, rc0, n_orders, tree):
    """-K: the dBG in the context coloured by write_freq's genomes
    (pg_kmer_colors) over the records the dBG pass inserted (g.dbg_flags)
    that have a genome - the ones the row pass walks, flags - as
    `<qry>_km_spectrum.tsv` and `_km_genomes.tsv`; the colours compared where they lie (pg_kmer_compare,
    write_compare's orders) as `_km_shared.tsv`, `_km_jaccard.tsv`,
    `_km_compare.npz` and, with n_orders, `_km_curve.tsv`; tree: the
    neighbour-joining tree of d = the k-mers in exactly one of two genomes
    (formed here from the shared matrix; this replaces the context's tree,
    whose files are written by now) as `_km_dist.tsv`, `_km_tree.nwk`,
    `_km_tree.tsv` and `_km_tree.npz`.  The colours are dropped afterwards."""
    dflags = g.dbg_flags if g.dbg_flags is not None else np.ones(len(names), np.uint8)
    rec_group, gnames = host.assign_groups(names, flags, groups)
    G = len(gnames)
    try:
        g.ctx.kmer_colors(rec_group, G, rec_flags=dflags, rc0=rc0)
        host.write_kmer_files(qry, g.ctx.kmer_colors_spectrum(), gnames)
        orders = host.compare_orders(G, n_orders)
        shared, pan, core = g.ctx.kmer_compare(orders)
        host.write_compare_files(qry, gnames, shared, orders, pan, core, tag="_km_", curve=bool(n_orders))
    finally:
        g.ctx.kmer_colors_drop()
    if tree:
        g.ctx.tree_nj(host.kmer_distance(shared), G)
        host.write_tree_files(qry, gnames, g.ctx.tree_dist(), g.ctx.tree_joins(), g.ctx.tree_root(), tag="_km_")


def write_region(g, qry, names, flags, groups):
    """-l: the region graph of the row pass just run (pg_region_graph on the
    device rows, write_freq's genomes) as `<qry>_fr_links.tsv` and
    `_fr_graph.gfa` (the device texts; a path is named by its record's seqid),
    `_fr_nodes.tsv` and `_fr_graph.npz`."""
    rec_group, gnames = host.assign_groups(names, flags, groups)
    g.ctx.region_graph(rec_group, len(gnames))
    table = g.ctx.region_nodes()
    table.update(g.ctx.region_links())
    table.update(g.ctx.region_paths())
    ids = [host.seqid(x) for x in names]

    def links(f):
        f.flush()
        g.ctx.region_links_write(f.fileno())

    def gfa(f):
        f.flush()
        g.ctx.region_gfa_write(ids, f.fileno())
    host.write_region_files(qry, links, gfa, table, gnames)


def write_region_seqs(g, qry, names, flags, groups, with_graph):
    """-s: one representative sequence per label of the row pass just run
    (pg_region_seqs on the device rows, write_freq's genomes) as
    `<qry>_fr_regions.fa` (the device text; a record is named by its seqid),
    `_fr_regions.tsv` and, after write_region (-l), `_fr_graph_seq.gfa`: the
    graph with the sequences on its S lines."""
    rec_group, gnames = host.assign_groups(names, flags, groups)
    g.ctx.region_seqs(rec_group, len(gnames))
    ids = [host.seqid(x) for x in names]

    def fasta(f):
        f.flush()
        g.ctx.region_fasta_write(ids, f.fileno())

    def gfa(f):
        f.flush()
        g.ctx.region_gfa_seq_write(ids, f.fileno())
    host.write_region_seq_files(qry, fasta, g.ctx.region_seqs_table(), ids, gfa if with_graph else None)


def write_sites(g, qry, names, flags, groups):
    """-v: the variable sites of the row pass just run (pg_region_sites on the
    device rows, write_freq's genomes) as `<qry>_fr_sites.tsv` (the device
    text), `_fr_sites_genomes.tsv` and `_fr_sites.npz`."""
    rec_group, gnames = host.assign_groups(names, flags, groups)
    g.ctx.region_sites(rec_group, len(gnames))
    table = g.ctx.region_sites_table()
    table.update(g.ctx.region_sites_alleles())
    table.update(g.ctx.region_sites_groups())

    def text(f):
        f.flush()
        g.ctx.region_sites_write(f.fileno())
    host.write_sites_files(qry, text, table, gnames)


def write_bubbles(g, qry, names, flags, groups, min_genomes):
    """-b: the variable sites between anchor regions of the row pass just run
    (pg_region_bubbles on the device rows, write_freq's genomes; an anchor is
    a label in min_genomes genomes, at most all of them) as
    `<qry>_fr_bubbles.tsv` (the device text), `_fr_bubbles_genomes.tsv` and
    `_fr_bubbles.npz`."""
    rec_group, gnames = host.assign_groups(names, flags, groups)
    m = max(1, min(int(min_genomes), len(gnames)))
    g.ctx.region_bubbles(rec_group, len(gnames), m)
    table = g.ctx.region_bubbles_table()
    table.update(g.ctx.region_bubbles_alleles())
    table["inner"] = g.ctx.region_bubbles_inner()
    table.update(g.ctx.region_bubbles_groups())
    table.update(g.ctx.region_bubbles_anchors())

    def text(f):
        f.flush()
        g.ctx.region_bubbles_write(f.fileno())
    host.write_bubbles_files(qry, text, table, gnames, m)


def write_variants(g, qry, names, flags, groups, ref_name):
    """-V: the bubbles just made (write_bubbles) as sequences and against the
    genome ref_name (pg_region_variants on the device rows, write_freq's
    genomes) as `<qry>_fr_alleles.fa` and the body of `_fr_variants.vcf` (the
    device texts; a record is named by its seqid) and `_fr_alleles.tsv`."""
    rec_group, gnames = host.assign_groups(names, flags, groups)
    ref = ref_genome(gnames, ref_name)
    g.ctx.region_variants(rec_group, len(gnames), ref)
    ids = [host.seqid(x) for x in names]
    sites, alleles = g.ctx.region_bubbles_table(), g.ctx.region_bubbles_alleles()
    site = alleles["allele_site"].astype(np.int64)
    table = g.ctx.region_variants_alleles()
    table.update({"from": sites["site_from"][site], "to": sites["site_to"][site],
                  "allele": np.arange(site.shape[0], dtype=np.int64) - sites["site_first"][site].astype(np.int64),
                  "regions": alleles["allele_regions"]})
    contigs = [(ids[r], int(g.seq_len[r])) for r in np.flatnonzero(rec_group == ref).tolist()]

    def fasta(f):
        f.flush()
        g.ctx.region_alleles_fasta_write(ids, f.fileno())

    def vcf(f):
        f.flush()
        g.ctx.region_vcf_write(ids, f.fileno())
    host.write_variants_files(qry, fasta, table, ids, host.vcf_header(gnames[ref], contigs, gnames), vcf)


def write_align(g, qry, names, flags, groups, ref_name, band=False):
    """-A: the alleles just decoded (write_variants) aligned against their
    site's reference (pg_region_align) as `<qry>_fr_align.tsv` and the body
    of `_fr_primitives.vcf` (the device texts; a record is named by its
    seqid), behind write_variants' header with an AC line.  band (-L): with
    the pairs above the cells cap aligned in a band."""
    rec_group, gnames = host.assign_groups(names, flags, groups)
    ref = ref_genome(gnames, ref_name)
    if band:
        g.ctx.tune(PG_TUNE_ALIGN_BAND, 1)
    try:
        g.ctx.region_align()
    finally:
        if band:
            g.ctx.tune(PG_TUNE_ALIGN_BAND, 0)
    ids = [host.seqid(x) for x in names]
    contigs = [(ids[r], int(g.seq_len[r])) for r in np.flatnonzero(rec_group == ref).tolist()]

    def tsv(f):
        f.flush()
        g.ctx.region_align_write(f.fileno())

    def vcf(f):
        f.flush()
        g.ctx.region_primitives_vcf_write(ids, f.fileno())
    host.write_align_files(qry, tsv, host.primitives_vcf_header(gnames[ref], contigs, gnames), vcf)


def _fileno(out):
    """The descriptor under a text stream's binary buffer (stdout, a file),
    or None (a stand-in with no descriptor)."""
    try:
        return out.buffer.fileno()
    except (AttributeError, OSError, ValueError):   # (io.UnsupportedOperation is an OSError)
        return None


# ---------------------------------------------------------------------- CLI
def manual_print(out=None):
    out = out or sys.stdout
    for line in ("Usage:", "  pyhton this.py -i qry.fsa -k 10 -n 1000000", "Parameters:",
                 "  -i: query sequences in fasta format", "  -k: kmer length",
                 "  -A: with -V, every allele aligned against the reference: CIGARs, and the SNVs and indels one per VCF line. 0 (off)",
                 "      or 1; single process only. writes <in>_fr_align.tsv, _fr_primitives.vcf",
                 "  -d: the de bruijn graph",
                 "  -L: with -A 1, the alleles too long for a whole alignment matrix (more than 2^24 cells) aligned in a band of",
                 "      diagonals that doubles until it holds their distance, instead of one replacement. 0 (off) or 1",
                 "  -r: break point of de bruijn graph",
                 "  -T: with -g, a neighbour-joining tree of the genomes from the regions they share. 0 (off) or 1; single process only.",
                 "      writes <in>_fr_dist.tsv, _fr_tree.nwk (Newick), _fr_tree.tsv, _fr_tree.npz and, with -A 1, a second tree from",
                 "      the primitive VCF lines: <in>_fr_vartree.nwk, _fr_vardist.tsv",
                 "  -B: with -T 1, bootstrap support for the tree's branches from this many replicates (0: off, at most 4096): the regions",
                 "      are resampled and every branch rated by the share of replicate trees that split the genomes the same way. single",
                 "      process only. writes <in>_fr_tree_support.nwk (Newick, percentages as node labels), _fr_tree_support.tsv,",
                 "      _fr_tree_boot.npz and, with -A 1, <in>_fr_vartree_support.nwk, _fr_vartree_support.tsv",
                 "  -K: with -g, colour the de bruijn graph: the genomes that hold every k-mer, hence the exact k-mer spectrum, the k-mers",
                 "      every pair of genomes shares and, with -p, the k-mer pan and core growth; no clustering is involved. 0 (off) or 1;",
                 "      single process only, not with -D. writes <in>_km_spectrum.tsv, _km_genomes.tsv, _km_shared.tsv, _km_jaccard.tsv,",
                 "      _km_compare.npz, with -p _km_curve.tsv and, with -T 1, _km_dist.tsv, _km_tree.nwk, _km_tree.tsv, _km_tree.npz",
                 "  -D: the reduced de bruijn graph", "  -R: break point of reduced de bruijn graph",
                 "  -v: with -g, the variable sites: pairs of regions joined in two or more ways, directly or through one region.",
                 "      0 (off) or 1; single process only. writes <in>_fr_sites.tsv, _fr_sites_genomes.tsv, _fr_sites.npz",
                 "  -I: with -a markov, the inflation. a multiple of 0.5 from 1.5 to 20. default 1.5",
                 "  -b: with -g, the variable sites between anchors, regions found in at least this many genomes (0: off), however",
                 "      many regions lie between two. single process only. writes <in>_fr_bubbles.tsv, _fr_bubbles_genomes.tsv, _fr_bubbles.npz",
                 "  -n: length of query sequences for pan-genomic analysis",
                 "  -s: with -g, one representative sequence per region. 0 (off) or 1; single process only. writes",
                 "      <in>_fr_regions.fa, _fr_regions.tsv and, with -l 1, _fr_graph_seq.gfa (GFA 1 with sequences)",
                 "  -g: frequency table of the regions across genomes. record (each record a genome) or a file of",
                 "      seqid<TAB>genome lines; writes <in>_fr_freq.tsv, _fr_spectrum.tsv, _fr_genomes.tsv, _fr_presence.npz",
                 "  -V: with -g and -b, this genome as the reference: the alleles of the sites between anchors as sequences, and a VCF",
                 "      against it. single process only. writes <in>_fr_alleles.fa, _fr_alleles.tsv, _fr_variants.vcf",
                 "  -p: with -g, compare the genomes over this many genome orders (0: off). writes <in>_fr_shared.tsv,",
                 "      _fr_jaccard.tsv (pairs), _fr_curve.tsv (pan and core genome growth), _fr_compare.npz",
                 "  -l: with -g, the graph of the regions along the genomes. 0 (off) or 1; single process only. writes",
                 "      <in>_fr_links.tsv, _fr_nodes.tsv, _fr_graph.gfa (GFA 1, the genomes as paths), _fr_graph.npz",
                 "  -c: complementary reverse sequence. 00,01,10,11",
                 "  -a: clustering of the rdBG. mcl (run or reuse mcl), cc (built-in connected components) or markov "
                 "(built-in Markov clustering)",
                 "  -w: with -a cc or markov, drop edges lighter than this weight. default 1. auto: the weight with the most clusters of "
                 "2+ nodes, from the cluster curve written to <in>_rdbg_weight.xyz.sweep.tsv (auto: -a cc only)"):
        print(line, file=out)


def parse_args(argv):
    """:1983-1997 — same flag handling, including `-k27` and skipped unknowns."""
    args = {"-i": "", "-k": "50", "-n": "2**63", "-r": "", "-d": "", "-R": "", "-D": "", "-c": "2", "-a": "mcl",
            "-w": "1", "-g": "", "-p": "0", "-l": "0", "-s": "0", "-I": "1.5", "-v": "0", "-b": "0",
            "-V": "", "-A": "0", "-L": "0", "-T": "0", "-B": "0", "-K": "0"}
    N = len(argv)
    for i in range(1, N):
        k = argv[i]
        if k in args:
            args[k] = argv[i + 1]
        elif k[:2] in args and len(k) > 2:
            args[k[:2]] = k[2:]
    return args


def weight_arg(args):
    """-w's value with -a cc: "auto" or an integer (anything else raises
    ValueError, as int() does)."""
    return "auto" if args["-w"] == "auto" else int(args["-w"])


def inflation_arg(args):
    """-I's value as pg_cluster_markov's inflation2 = 2 r: r a decimal multiple
    of 0.5 in [1.5, 20]; None for anything else."""
    import re
    m = re.fullmatch(r"(\d+)(?:\.([05])0*)?", args["-I"])
    if not m:
        return None
    i2 = 2 * int(m.group(1)) + (m.group(2) == "5")
    return i2 if 3 <= i2 <= 40 else None


def cluster_args(args):
    """seq2graph's clustering keywords from -a, -w and -I, or None for a
    combination that is refused (-I is read with -a markov alone)."""
    if args["-a"] == "cc":
        return dict(cluster="cc", min_weight=weight_arg(args))
    if args["-a"] == "markov":
        i2 = inflation_arg(args)
        if i2 is None or args["-w"] == "auto":
            return None
        return dict(cluster="markov", min_weight=int(args["-w"]), inflation2=i2)
    return {} if args["-a"] == "mcl" else None


def compare_orders_arg(args):
    """-p's value: the number of genome orders (0: off), or None for a value
    that is refused - not a non-negative integer, or >= 1 without -g."""
    try:
        p = int(args["-p"])
    except ValueError:
        return None
    return None if p < 0 or (p and not args["-g"]) else p


def links_arg(args):
    """-l's value: False (0) or True (1), or None for a value that is refused
    - anything else, or 1 without -g."""
    if args["-l"] not in ("0", "1"):
        return None
    return None if args["-l"] == "1" and not args["-g"] else args["-l"] == "1"


def seqs_arg(args):
    """-s's value: False (0) or True (1), or None for a value that is refused
    - anything else, or 1 without -g."""
    if args["-s"] not in ("0", "1"):
        return None
    return None if args["-s"] == "1" and not args["-g"] else args["-s"] == "1"


def sites_arg(args):
    """-v's value: False (0) or True (1), or None for a value that is refused
    - anything else, or 1 without -g."""
    if args["-v"] not in ("0", "1"):
        return None
    return None if args["-v"] == "1" and not args["-g"] else args["-v"] == "1"


def bubbles_arg(args):
    """-b's value: min_genomes (0: off), or None for a value that is refused
    - not a non-negative decimal integer, or >= 1 without -g."""
    if not args["-b"].isascii() or not args["-b"].isdigit():
        return None
    b = int(args["-b"])
    return None if b and not args["-g"] else b


def variants_arg(args, bubbles):
    """-V's value: the reference genome's name ("": off), or None when it is
    refused - given without -g or without -b >= 1."""
    if not args["-V"]:
        return ""
    return args["-V"] if args["-g"] and bubbles else None


def align_arg(args, variants):
    """-A's value: False (0) or True (1), or None for a value that is refused
    - anything else, or 1 without an accepted -V."""
    if args["-A"] not in ("0", "1"):
        return None
    return None if args["-A"] == "1" and not variants else args["-A"] == "1"


def band_arg(args, align):
    """-L's value: False (0) or True (1), or None for a value that is refused
    - anything else, or 1 without an accepted -A 1."""
    if args["-L"] not in ("0", "1"):
        return None
    return None if args["-L"] == "1" and not align else args["-L"] == "1"


def tree_arg(args):
    """-T's value: False (0) or True (1), or None for a value that is refused
    - anything else, or 1 without -g."""
    if args["-T"] not in ("0", "1"):
        return None
    return None if args["-T"] == "1" and not args["-g"] else args["-T"] == "1"


def boot_arg(args, tree):
    """-B's value: the bootstrap replicates (0: off), or None for a value that
    is refused - not a decimal integer in [0, 4096], or >= 1 without an
    accepted -T 1."""
    if not args["-B"].isascii() or not args["-B"].isdigit() or int(args["-B"]) > host.BOOT_MAX_REPS:
        return None
    b = int(args["-B"])
    return None if b and not tree else b


def kmers_arg(args):
    """-K's value: False (0) or True (1), or None for a value that is refused
    - anything else, or 1 without -g, or 1 with -D (no dBG is loaded then)."""
    if args["-K"] not in ("0", "1"):
        return None
    return None if args["-K"] == "1" and (not args["-g"] or args["-D"]) else args["-K"] == "1"


def entry_point(argv, out=None, device=0):
    out = out or sys.stdout
    args = parse_args(argv)
    qry, kmer, Ns = args["-i"], int(args["-k"]), host.eval_number(args["-n"])
    bkt, dbs, rbk, rc, rdb = args["-r"], args["-d"], args["-R"], int(args["-c"]), args["-D"]
    n_orders, links, seqs, sites = compare_orders_arg(args), links_arg(args), seqs_arg(args), sites_arg(args)
    bubbles = bubbles_arg(args)
    variants = variants_arg(args, bubbles)
    align = align_arg(args, variants)
    band = band_arg(args, align)
    tree = tree_arg(args)
    boot = boot_arg(args, tree)
    kmers = kmers_arg(args)
    bad = (kmers is None or tree is None or boot is None or not qry or n_orders is None or links is None or seqs is None or sites is None or bubbles is None or
           variants is None or align is None or band is None)
    clu = None if bad else cluster_args(args)
    if clu is None:
        manual_print(out)
        raise SystemExit()
    grp = args["-g"]
    if grp:
        clu["groups"] = grp
    if n_orders:
        clu["orders"] = n_orders
    if links:
        clu["links"] = True
    if seqs:
        clu["seqs"] = True
    if sites:
        clu["sites"] = True
    if bubbles:
        clu["bubbles"] = bubbles
    if variants:
        clu["variants"] = variants
    if align:
        clu["align"] = True
    if band:
        clu["align_band"] = True
    if tree:
        clu["tree"] = True
    if boot:
        clu["boot"] = boot
    # a group file, and -V's genome, are checked against the records before anything is built
    chk = (lambda g: check_groups(g, Ns, grp, variants)) if grp and (grp != "record" or variants) else None
    chunk = 2 ** 33
    rc0, rc1 = (rc >> 1) == 1, (rc & 1) == 1
    if kmers:
        clu["kmers"] = True
        clu["rc0"] = rc0
    if dbs or rdb:                                    # :2073-2101
        if not rdb:
            print("load dBG from disk", file=out)
            kmer_dict = load_graph(qry, kmer, dbs, device, rdbg=False, rc=rc0, on_parsed=chk)
            # (-K walks the records a build over this input would insert)
            kmer_dict.dbg_flags = host.plan_dbg(kmer_dict.seq_len, kmer_dict.shape, rc0, Ns, chunk)[0]
            print("# build the reduced dBG", file=out)
            rdbg_dict = dbg2rdbg(kmer_dict)
        else:
            rdbg_dict = dbg2rdbg(load_graph(qry, kmer, rdb, device, rdbg=True, rc=rc0, on_parsed=chk))
        print("# find fr", file=out)
        seq2graph(qry, kmer=kmer, bits=5, Ns=Ns, rdbg_dict=rdbg_dict, chunk=chunk, brkpt=rbk, rc=rc1, out=out, **clu)
        return 0
    ctx = Context(min(max(1, kmer), 27), device)     # HIP runtime start-up before the stage timer
    print("# build the dBG", file=out)
    st = time()
    kmer_dict = seq2rdbg(qry, kmer, 5, Ns, brkpt=bkt, chunk=chunk, rc=rc0, device=device, ctx=ctx, on_parsed=chk)
    print("# finished in", time() - st, "seconds", file=out)
    print("# save dBG to disk", file=out)
    st = time()
    dump(kmer_dict, qry + "_db")
    print("# finished in", time() - st, "seconds", file=out)
    # the reference reloads the file it just wrote (:2120-2126); the device
    # table is that same dBG, so nothing is read back
    print("# load dBG from disk", file=out)
    st = time()
    print("# finished in", time() - st, "seconds", file=out)
    print("# build the reduced dBG", file=out)
    st = time()
    rdbg_dict = dbg2rdbg(kmer_dict)
    print("# finished in", time() - st, "seconds", file=out)
    print("# find fr", file=out)
    st = time()
    seq2graph(qry, kmer=kmer, bits=5, Ns=Ns, rdbg_dict=rdbg_dict, chunk=chunk, brkpt=rbk, rc=rc1, out=out, **clu)
    print("# finished in", time() - st, "seconds", file=out)
    return 0


def main():
    return entry_point(sys.argv)
