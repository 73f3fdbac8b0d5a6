// pg_variants.hip — the bases of the bubbles' alleles and the sites placed on
// a reference genome: the alleles table and their letters, an allele FASTA and
// the body of a VCF.  pg_region_bubbles says which label paths join two
// anchors; this pass says what they read, and where they lie on the walks of
// one genome.
//
// Rows, rec_group, the rule for a used row and the run are pg_region_bubbles'
// (pg_region.hip); the tables read are its result (pg_bubbles.h).  A segment at
// the used anchor row i ends at the next anchor row j of i's run; its span is
// [hi(i), lo(j)) of the record if the strand is 1 and [hi(j), lo(i)) otherwise
// (lo / hi: the smaller / larger of a row's start and end), read in walk
// direction.  An allele's sequence is that of the segment at its first_row.
// Two alleles of a site may read the same: different label paths can have the
// same bases, and they are not merged.
//
// Steps, each its own launch on c.stream (no hand-shake inside a kernel):
//   a. k_row_scan   the shared front end: the flag byte of every row, the rows
//                   that leave their record refused; k_vr_anchor adds the
//                   anchor bit (a search in the bubbles' anchors)
//   b. k_vr_verify  one thread per step of every allele's representative
//                   segment: the row is in the list, used, of the first row's
//                   record and strand, and carries from / the inner label / to
//   c. k_vr_spans   per allele its span, as an entry of the decoder's table
//   d. k_vr_refscan every strand-1 anchor row of a ref_group record walks to
//                   the next anchor of its run (each step of a run is walked
//                   once), finds its flank pair in the sites table (sorted by
//                   (from, to): a binary search) and takes the site's smallest
//                   row with a 64-bit atomic min;  k_vr_reflen walks the chosen
//                   segment once more for its length in regions
//   e. k_vr_mismatch one thread per allele and per inner label of every allele
//                   of a site with a reference segment: the lengths, then the
//                   labels position by position; k_vr_refal the allele nothing
//                   spoke against (alleles are distinct paths: at most one)
//   f. k_vr_place   pos0, the REF span and the placed bit per site; a select of
//                   the placed sites and two stable radix sorts (pos0, then the
//                   record) give the VCF's order; k_vr_placed fills the table
//                   and one decoder entry per placed site: the padding base and
//                   the reference's own letters, [pos0 - 1, pos0 + ref_len)
//   g. k_rs_decode  (pg_seqdec.h) every entry's letters, gc and amb
//   h. the texts, made by every call with its own names through pg_text.h:
//      AlleleFastaLine one thread per header; VcfLine one thread per item - a
//      site's head (CHROM POS ID and the gap of REF), one item per ALT entry,
//      the fixed columns, one item per GT cell; the item and byte offsets come
//      from scans.  k_rs_copy moves the letters into the gaps in 16-byte
//      pieces; the entries a text does not show are left out.
//
// Device bytes while the call runs: 1 per row (and 40 for rows from the host);
// per allele 96 and 1; per site 45, and 32 more per placed site while they are
// sorted.  The result: 88 per allele and 132 per placed site, and per base 1
// (every sequence starts at a multiple of 16).  A text call: its bytes, 8 per
// item and 8 per entry.
//
// Every sum is an integer and every atomic commutes: the result depends on
// the input alone, whatever the schedule.
#include "pg_bubbles.h"
#include "pg_seqdec.h"

namespace pg {

#define VR_ANCHOR 4u               // flag byte of a row, beside RG_USED and RG_HEAD: its label is an anchor
#define VR_BAD_ALLELE 1ull         // what a kernel found wrong: an allele's rows are not the bubbles'
#define VR_BAD_SPAN 2ull           //   a representative segment's flank rows overlap or are out of order
#define VR_BAD_REFSPAN 4ull        //   a reference segment's
#define VR_BAD_NOREF 8ull          //   a reference segment matches no allele
#define VR_NONE32 0xFFFFFFFFu

__device__ __forceinline__ long long vr_lo(const long long* q) { return q[1] < q[2] ? q[1] : q[2]; }
__device__ __forceinline__ long long vr_hi(const long long* q) { return q[1] < q[2] ? q[2] : q[1]; }
// row j goes on the run of the row before it
__device__ __forceinline__ bool vr_follows(uint32_t f) { return (f & (RG_USED | RG_HEAD)) == RG_USED; }

// ------------------------------------------------------------ a. the anchor bit
__global__ void k_vr_anchor(const long long* __restrict__ rows, uint64_t n, const long long* __restrict__ anchors,
                            uint64_t nanc, uint8_t* __restrict__ rf) {
  RG_LOOP(i, n) {
    const uint32_t f = rf[i];
    if (!(f & RG_USED)) continue;
    const long long lab = rows[5 * i + 4];
    uint64_t lo = 0, hi = nanc;                            // the first anchor >= lab
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (anchors[mid] < lab) lo = mid + 1; else hi = mid;
    }
    if (lo < nanc && anchors[lo] == lab) rf[i] = (uint8_t)(f | VR_ANCHOR);
  }
}

// ------------------------------------------------------------ b. the alleles' rows
// item i of all: step k of allele al, the row first_row + k (k = 0: from, 1 .. regions: the inner path,
// regions + 1: to)
__global__ void k_vr_verify(const long long* __restrict__ rows, uint64_t n, const uint8_t* __restrict__ rf, BbSites T,
                            BbAlleles A, const long long* __restrict__ inner, uint64_t na, uint64_t total, ull* bad) {
  RG_LOOP(i, total) {
    const uint64_t al = bb_find(A.ioff, na, 2, i);
    const ull k = i - (A.ioff[al] + 2ull * al), r = A.regions[al], f = A.frow[al];
    bool ok = f < n && r + 1ull < n - f;
    if (ok) {
      const ull site = A.site[al];
      const long long *q = rows + 5 * (f + k), *q0 = rows + 5 * f;
      const long long want = k == 0 ? T.from[site] : k <= r ? inner[A.ioff[al] + k - 1ull] : T.to[site];
      ok = (rf[f + k] & RG_USED) && q[0] == q0[0] && q[3] == q0[3] && q[4] == want;
    }
    if (!ok) RG_OR(bad, VR_BAD_ALLELE);
  }
}

// ------------------------------------------------------------ c. the alleles' spans
__global__ void k_vr_spans(const long long* __restrict__ rows, BbAlleles A, uint64_t na, RsTab V,
                           ull* __restrict__ plen, ull* bad) {
  RG_LOOP(al, na) {
    const ull f = A.frow[al];
    const long long *qi = rows + 5 * f, *qj = rows + 5 * (f + A.regions[al] + 1ull);
    const bool fw = qi[3] == 1;
    long long lo = fw ? vr_hi(qi) : vr_hi(qj), hi = fw ? vr_lo(qj) : vr_lo(qi);
    if (lo > hi) {
      RG_OR(bad, VR_BAD_SPAN);
      hi = lo;
    }
    const ull len = (ull)(hi - lo);
    V.label[al] = (long long)al;
    V.row[al] = (long long)f;
    V.rec[al] = qi[0];
    V.start[al] = lo;
    V.end[al] = hi;
    V.strand[al] = qi[3];
    V.len[al] = len;
    V.gc[al] = 0;
    V.amb[al] = 0;
    plen[al] = (len + 15ull) & ~15ull;
  }
}

// ------------------------------------------------------------ d. the reference scan
// refrow[s] (all ones before): the smallest strand-1 anchor row of a ref_group record whose segment has
// site s's flanks
__global__ void k_vr_refscan(const long long* __restrict__ rows, uint64_t n, const int* __restrict__ rec_group,
                             const uint8_t* __restrict__ rf, int ref_group, BbSites T, uint64_t ns, ull* refrow) {
  RG_LOOP(i, n) {
    const uint32_t f = rf[i];
    if ((f & (RG_USED | VR_ANCHOR)) != (RG_USED | VR_ANCHOR)) continue;
    const long long* q = rows + 5 * i;
    if (q[3] != 1 || rec_group[q[0]] != ref_group) continue;
    uint64_t j = i + 1;                                    // (rf[n] = 0 ends every walk)
    while (vr_follows(rf[j]) && !(rf[j] & VR_ANCHOR)) ++j;
    if (!vr_follows(rf[j])) continue;                      // the run ended before another anchor
    const long long a = q[4], b = rows[5 * j + 4];
    uint64_t lo = 0, hi = ns;                              // the first site >= (a, b)
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (T.from[mid] < a || (T.from[mid] == a && T.to[mid] < b)) lo = mid + 1; else hi = mid;
    }
    if (lo < ns && T.from[lo] == a && T.to[lo] == b) RG_MIN(refrow + lo, (ull)i);
  }
}
// rr[s]: the regions between the reference segment's flank rows
__global__ void k_vr_reflen(const uint8_t* __restrict__ rf, uint64_t ns, const ull* __restrict__ refrow,
                            ull* __restrict__ rr) {
  RG_LOOP(s, ns) {
    const ull i = refrow[s];
    ull j = i + 1;
    if (i != RS_NONE)
      while (!(rf[j] & VR_ANCHOR)) ++j;                    // (k_vr_refscan reached that anchor)
    rr[s] = i != RS_NONE ? j - i - 1ull : 0ull;
  }
}

// ------------------------------------------------------------ e. the ref allele
// item i of all: allele al's length (k = 0) or its inner label k - 1 against the reference segment's;
// mism[al] (zero before) = 1 if anything differs
__global__ void k_vr_mismatch(const long long* __restrict__ rows, BbAlleles A, const long long* __restrict__ inner,
                              uint64_t na, uint64_t total, const ull* __restrict__ refrow, const ull* __restrict__ rr,
                              uint8_t* __restrict__ mism) {
  RG_LOOP(i, total) {
    const uint64_t al = bb_find(A.ioff, na, 1, i);
    const ull k = i - (A.ioff[al] + al), s = A.site[al], row = refrow[s];
    if (row == RS_NONE) continue;
    const bool same_len = A.regions[al] == rr[s];
    if (k == 0 ? !same_len : same_len && inner[A.ioff[al] + k - 1ull] != rows[5 * (row + k) + 4]) mism[al] = 1;
  }
}
// refal[s] (all ones before): the index inside the site of the allele that equals the reference segment
__global__ void k_vr_refal(BbSites T, BbAlleles A, uint64_t na, const ull* __restrict__ refrow,
                           const uint8_t* __restrict__ mism, uint32_t* __restrict__ refal) {
  RG_LOOP(al, na) {
    const ull s = A.site[al];
    if (refrow[s] != RS_NONE && !mism[al]) refal[s] = (uint32_t)(al - T.first[s]);
  }
}

// ------------------------------------------------------------ f. placement
// keep[s]: the site is placed; pos[s], rec[s]: its sort keys (0 for a site without a reference segment)
__global__ void k_vr_place(const long long* __restrict__ rows, uint64_t ns, const ull* __restrict__ refrow,
                           const ull* __restrict__ rr, const uint32_t* __restrict__ refal, uint8_t* __restrict__ keep,
                           ull* __restrict__ pos, ull* __restrict__ rec, ull* bad) {
  RG_LOOP(s, ns) {
    const ull i = refrow[s];
    ull p = 0, r = 0;
    bool placed = false;
    if (i != RS_NONE) {
      const long long *qi = rows + 5 * i, *qj = rows + 5 * (i + rr[s] + 1ull);
      if (refal[s] == VR_NONE32) RG_OR(bad, VR_BAD_NOREF);
      if (vr_lo(qj) < vr_hi(qi)) RG_OR(bad, VR_BAD_REFSPAN);
      p = (ull)vr_hi(qi);                                  // (k_row_scan: lo >= 0)
      r = (ull)qi[0];
      placed = p >= 1ull;
    }
    keep[s] = placed;
    pos[s] = p;
    rec[s] = r;
  }
}
// the placed table in the VCF's order, and entry na + p of the decoder's table: the padding base and REF
__global__ void k_vr_placed(const long long* __restrict__ rows, const ull* __restrict__ ord, uint64_t np,
                            const ull* __restrict__ refrow, const ull* __restrict__ rr,
                            const uint32_t* __restrict__ refal, VrPlaced P, RsTab V, uint64_t na,
                            ull* __restrict__ plen) {
  RG_LOOP(p, np) {
    const ull s = ord[p], i = refrow[s];
    const long long *qi = rows + 5 * i, *qj = rows + 5 * (i + rr[s] + 1ull);
    const long long pos0 = vr_hi(qi);
    const ull len = (ull)(vr_lo(qj) - pos0);
    P.site[p] = s;
    P.row[p] = i;
    P.len[p] = len;
    P.rec[p] = qi[0];
    P.pos[p] = pos0;
    P.refal[p] = refal[s];
    const uint64_t e = na + p;
    V.label[e] = (long long)s;
    V.row[e] = (long long)i;
    V.rec[e] = qi[0];
    V.start[e] = pos0 - 1;
    V.end[e] = pos0 + (long long)len;
    V.strand[e] = 1;
    V.len[e] = len + 1ull;
    V.gc[e] = 0;
    V.amb[e] = 0;
    plen[e] = (len + 1ull + 15ull) & ~15ull;
  }
}

// ------------------------------------------------------------ h. texts
// ><from>_<to>_<k> <name>:<lo>-<hi>:<+|-> regions=<r> genomes=<g> len=<len>\n<sequence>\n; the line leaves a
// gap for the letters (sdst[al]: where it starts in the text)
struct AlleleFastaLine {
  RsTab V;
  BbSites T;
  BbAlleles A;
  const char* names;
  const long long* name_off;
  ull* sdst;
  template <class S>
  __device__ __forceinline__ void operator()(S& s, uint64_t al) const {
    const ull site = A.site[al];
    const long long r = V.rec[al];
    s.ch('>'); s.dec((ull)T.from[site]); s.ch('_'); s.dec((ull)T.to[site]); s.ch('_'); s.dec(al - T.first[site]);
    s.ch(' '); s.bytes(names + name_off[r], (ull)(name_off[r + 1] - name_off[r]));
    s.ch(':'); s.sdec(V.start[al]); s.ch('-'); s.sdec(V.end[al]);
    s.ch(':'); s.ch(V.strand[al] == 1 ? '+' : '-');
    s.lit(" regions="); s.dec(A.regions[al]);
    s.lit(" genomes="); s.dec(A.ngen[al]);
    s.lit(" len="); s.dec(V.len[al]); s.ch('\n');
    const ull at = s.gap(V.len[al]);
    if constexpr (S::writes) sdst[al] = at;
    s.ch('\n');
  }
};
// items[p] = the items of placed site p's line: its head, an ALT entry per other allele, the fixed
// columns and a cell per genome
__global__ void k_vr_items(VrPlaced P, BbSites T, uint64_t np, uint32_t G, ull* __restrict__ items) {
  RG_LOOP(p, np) items[p] = (ull)T.nal[P.site[p]] + (ull)G + 1ull;
}
// <name> <pos0> <from>_<to> <REF> <ALT> . . NS=<n> GT <cell> ... - tab separated.  Item k of placed
// site p: 0 its head, 1 .. nal - 1 the ALT entries, nal the fixed columns, then the cells.  REF and the
// ALT letters are gaps (dst[entry]: where an entry of the decoder's table goes; all ones before)
struct VcfLine {
  RsTab V;
  VrPlaced P;
  BbSites T;
  BbAlleles A;
  const ull* bits;
  const ull* ioff;                 // [np + 1] the items before each placed site
  const char* blob;
  const char* names;
  const long long* name_off;
  ull* dst;
  uint64_t na, np;
  uint32_t G, W;
  template <class S>
  __device__ __forceinline__ void operator()(S& s, uint64_t i) const {
    const uint64_t p = bb_find(ioff, np, 0, i);
    const ull k = i - ioff[p], site = P.site[p], first = T.first[site];
    const uint32_t nal = T.nal[site], ra = P.refal[p];
    if (k == 0) {
      const long long r = P.rec[p];
      s.bytes(names + name_off[r], (ull)(name_off[r + 1] - name_off[r]));
      s.ch('\t'); s.sdec(P.pos[p]); s.ch('\t');
      s.dec((ull)T.from[site]); s.ch('_'); s.dec((ull)T.to[site]); s.ch('\t');
      const ull at = s.gap(P.len[p] + 1ull);
      if constexpr (S::writes) dst[na + p] = at;
    } else if (k < nal) {
      const ull a = k - 1ull < ra ? k - 1ull : k, al = first + a;   // the k-th allele that is not the ref allele
      char pad = 'N';
      if constexpr (S::writes) pad = blob[V.poff[na + p]];
      s.ch(k == 1 ? '\t' : ','); s.ch(pad);
      const ull at = s.gap(V.len[al]);
      if constexpr (S::writes) dst[al] = at;
    } else if (k == nal) {
      s.lit("\t.\t.\tNS="); s.dec(T.ngen[site]); s.lit("\tGT");
    } else {
      const uint32_t g = (uint32_t)(k - nal - 1ull);
      const ull bit = 1ull << (g & 63u);
      const ull* b = bits + first * W + (g >> 6);
      bool any = (b[(size_t)ra * W] & bit) != 0;
      s.ch('\t');
      if (any) s.ch('0');
      for (uint32_t a = 0; a < nal; ++a) {
        if (a == ra || !(b[(size_t)a * W] & bit)) continue;
        if (any) s.ch('/');
        s.dec(a < ra ? a + 1u : a);
        any = true;
      }
      if (!any) s.ch('.');
      if (g + 1u == G) s.ch('\n');
    }
  }
};

static ull read_flags(Ctx& c, const DevBuf& bad) {
  ull h = 0;
  PG_HIP(hipMemcpyAsync(&h, bad.p, 8, hipMemcpyDeviceToHost, c.stream));
  c.sync();
  return h;
}

void region_variants(Ctx& c, const int64_t* h_rows5, uint64_t n_rows, const int32_t* rec_group, uint64_t n_records,
                     uint32_t G, uint32_t ref_group, uint64_t* n_alleles, uint64_t* n_bases, uint64_t* n_placed,
                     uint64_t* n_unplaced) {
  const char* what = "pg_region_variants";
  const std::string w = std::string(what) + ": ";
  // ---- arguments, a parse and the bubbles: everything refused here leaves the previous result in place
  if (rec_group && !c.parsed) throw Error(-22, w + "no parse (the bases come from the context's parse)");
  const RowInput in = row_input(c, what, h_rows5, n_rows, rec_group, n_records, G, true);
  need(c.bb_ready, what, NEED_BUBBLES);
  if (G != c.bb_groups)
    throw Error(-22, w + std::to_string(G) + " groups, the bubbles have " + std::to_string(c.bb_groups));
  const bool has_ref = ref_group != 0xFFFFFFFFu;
  if (has_ref && ref_group >= G)
    throw Error(-22, w + "ref_group = " + std::to_string(ref_group) + " is outside [0, " + std::to_string(G) + ")");
  const uint64_t n = in.n, ns = c.bb_ns, na = c.bb_na, nin = c.bb_nin;
  const long long* rows = in.rows;

  // ---- a. the flags; the rows that leave their record are refused before anything is allocated
  DevBuf rf, bad;
  rf.reserve(n + 16);
  row_scan(c, what, in, rf.as<uint8_t>(), c.rec_len.as<long long>());
  if (!n) PG_HIP(hipMemsetAsync(rf.p, 0, 1, c.stream));
  bad.reserve(16);
  PG_HIP(hipMemsetAsync(bad.p, 0, 8, c.stream));
  const BbSites T(c.bb_sites, ns);
  const BbAlleles A(c.bb_alleles, na);
  const long long* inner = c.bb_inner.as<long long>();

  DevBuf tab, plen, blob, place, refrow, rr, refal, mism, keep, pos, rec, sidx, ord, ord2, kin, kout, cnt;
  uint64_t np = 0;
  if (na) {
    // ---- b. every allele's rows are the ones the bubbles were made of
    if (c.bb_nanc && n)
      RG_LAUNCH(k_vr_anchor, grid_for(n, RG_BLOCK, 8192), rows, n, c.bb_anchors.as<long long>(), c.bb_nanc,
                rf.as<uint8_t>());
    RG_LAUNCH(k_vr_verify, grid_for(nin + 2 * na, RG_BLOCK, 8192), rows, n, rf.as<uint8_t>(), T, A, inner, na,
              nin + 2 * na, bad.as<ull>());
    if (read_flags(c, bad))
      throw Error(-22, w + "the bubbles are not of these rows (an allele's rows are outside the list, not used, "
                           "of two records or strands, or carry other labels)");
    // ---- d. e. the reference segments and their alleles
    refrow.reserve(8 * (ns + 1));
    rr.reserve(8 * (ns + 1));
    refal.reserve(4 * (ns + 1));
    mism.reserve(na + 16);
    keep.reserve(ns + 16);
    pos.reserve(8 * (ns + 1));
    rec.reserve(8 * (ns + 1));
    PG_HIP(hipMemsetAsync(refrow.p, 0xFF, 8 * ns, c.stream));
    PG_HIP(hipMemsetAsync(refal.p, 0xFF, 4 * ns, c.stream));
    PG_HIP(hipMemsetAsync(mism.p, 0, na, c.stream));
    PG_HIP(hipMemsetAsync(keep.as<uint8_t>() + ns, 0, 1, c.stream));
    const unsigned gs = grid_for(ns, RG_BLOCK, 8192);
    if (has_ref) {
      RG_LAUNCH(k_vr_refscan, grid_for(n, RG_BLOCK, 8192), rows, n, in.group, rf.as<uint8_t>(), (int)ref_group, T, ns,
                refrow.as<ull>());
      RG_LAUNCH(k_vr_reflen, gs, rf.as<uint8_t>(), ns, refrow.as<ull>(), rr.as<ull>());
      RG_LAUNCH(k_vr_mismatch, grid_for(nin + na, RG_BLOCK, 8192), rows, A, inner, na, nin + na, refrow.as<ull>(),
                rr.as<ull>(), mism.as<uint8_t>());
      RG_LAUNCH(k_vr_refal, grid_for(na, RG_BLOCK, 8192), T, A, na, refrow.as<ull>(), mism.as<uint8_t>(),
                refal.as<uint32_t>());
    } else {
      PG_HIP(hipMemsetAsync(rr.p, 0, 8 * ns, c.stream));
    }
    // ---- f. the placed sites, in (record, pos0, site) order
    RG_LAUNCH(k_vr_place, gs, rows, ns, refrow.as<ull>(), rr.as<ull>(), refal.as<uint32_t>(), keep.as<uint8_t>(),
              pos.as<ull>(), rec.as<ull>(), bad.as<ull>());
    sidx.reserve(8 * (ns + 1));
    np = select_flagged(c, rocprim::counting_iterator<ull>(0), keep.as<uint8_t>(), sidx.as<ull>(), ns, cnt);
    // ---- c. the alleles' spans (and what k_vr_place found)
    tab.reserve(RsTab::bytes(na + np));
    plen.reserve(8 * (na + np + 1));
    RsTab V(tab, na + np);
    RG_LAUNCH(k_vr_spans, grid_for(na, RG_BLOCK, 8192), rows, A, na, V, plen.as<ull>(), bad.as<ull>());
    const ull h = read_flags(c, bad);
    if (h & VR_BAD_NOREF)
      throw Error(-22, w + "the bubbles are not of these rows (a reference segment's inner path is no allele of "
                           "its site)");
    if (h & (VR_BAD_SPAN | VR_BAD_REFSPAN))
      throw Error(-22, w + "the flank rows of a" + ((h & VR_BAD_SPAN) ? "n allele's first" : " reference") +
                           " segment overlap or are out of order (its span starts after its end)");
    place.reserve(VrPlaced::bytes(np));
    if (np) {
      ord.reserve(8 * np);
      ord2.reserve(8 * np);
      kin.reserve(8 * np);
      kout.reserve(8 * np);
      const unsigned gp = grid_for(np, RG_BLOCK, 8192);
      hipLaunchKernelGGL(k_gather_key, dim3(gp), dim3(RG_BLOCK), 0, c.stream, pos.as<ull>(), sidx.as<ull>(), np,
                         kin.as<ull>());
      PG_HIP(hipGetLastError());
      sort_pairs(c, kin.as<ull>(), kout.as<ull>(), sidx.as<ull>(), ord2.as<ull>(), np, bits_for(c.n_cls));
      hipLaunchKernelGGL(k_gather_key, dim3(gp), dim3(RG_BLOCK), 0, c.stream, rec.as<ull>(), ord2.as<ull>(), np,
                         kin.as<ull>());
      PG_HIP(hipGetLastError());
      sort_pairs(c, kin.as<ull>(), kout.as<ull>(), ord2.as<ull>(), ord.as<ull>(), np, bits_for(c.n_records));
      RG_LAUNCH(k_vr_placed, gp, rows, ord.as<ull>(), np, refrow.as<ull>(), rr.as<ull>(), refal.as<uint32_t>(),
                VrPlaced(place, np), V, na, plen.as<ull>());
    }
  } else {
    tab.reserve(RsTab::bytes(0));
    place.reserve(VrPlaced::bytes(0));
  }
  // ---- g. the letters
  const uint64_t nt = na + np;
  uint64_t bases = 0, pad = 0, pad_al = 0;
  if (nt) {
    RsTab V(tab, nt);
    excl_scan_total(c, V.len, V.off, nt);
    pad = excl_scan_total(c, plen.as<ull>(), V.poff, nt);
    ull h2[2] = {0, 0};
    PG_HIP(hipMemcpyAsync(h2, V.off + na, 8, hipMemcpyDeviceToHost, c.stream));
    PG_HIP(hipMemcpyAsync(h2 + 1, V.poff + na, 8, hipMemcpyDeviceToHost, c.stream));
    c.sync();
    bases = h2[0];
    pad_al = h2[1];
  }
  blob.reserve(pad + 16);
  if (pad) {
    const uint64_t nchunks = pad / 16;
    c.t_vr.init();
    c.t_vr.start(c.stream);
    RG_LAUNCH(k_rs_decode, grid_for(nchunks, RG_BLOCK, RS_DECODE_GRID), packed_cls(c), c.rec_start.as<long long>(),
              (ull)((c.n_cls - 1) >> 4), RsTab(tab, nt), nt, nchunks, blob.as<uint4>());
    c.t_vr.stop(c.stream);
  }
  c.sync();
  c.ms_vr_decode = pad ? c.t_vr.ms() : 0.0;
  c.vr_chunks = pad / 16;
  // ---- the new result replaces the previous one
  c.vr_tab.swap(tab);
  c.vr_blob.swap(blob);
  c.vr_place.swap(place);
  c.vr_na = na;
  c.vr_np = np;
  c.vr_unplaced = ns - np;
  c.vr_bases = bases;
  c.vr_pad_al = pad_al;
  c.vr_pad = pad;
  c.vr_ready = true;
  c.al_ready = false;                                      // (the alignments described the old alleles)
  if (n_alleles) *n_alleles = na;
  if (n_bases) *n_bases = bases;
  if (n_placed) *n_placed = np;
  if (n_unplaced) *n_unplaced = ns - np;
}

void region_variants_alleles(Ctx& c, int64_t* record, int64_t* lo, int64_t* hi, int64_t* strand, uint64_t* len,
                             uint64_t* gc, uint64_t* amb, uint64_t* offset, uint64_t cap) {
  need(c.vr_ready, "pg_region_variants_alleles", NEED_VARIANTS);
  const uint64_t n = c.vr_na;
  if (cap < n) throw Error(-34, "pg_region_variants_alleles: buffer too small");
  if (!n) return;
  RsTab V(c.vr_tab, n + c.vr_np);
  get(c, record, V.rec, 8 * n);
  get(c, lo, V.start, 8 * n);
  get(c, hi, V.end, 8 * n);
  get(c, strand, V.strand, 8 * n);
  get(c, len, V.len, 8 * n);
  get(c, gc, V.gc, 8 * n);
  get(c, amb, V.amb, 8 * n);
  get(c, offset, V.off, 8 * n);
  c.sync();
}

// the alleles' letters one after another: their number (out null), or copied into out
uint64_t region_variants_bases(Ctx& c, uint8_t* out, uint64_t cap) {
  need(c.vr_ready, "pg_region_variants_bases", NEED_VARIANTS);
  if (!out) return c.vr_bases;
  if (cap < c.vr_bases) throw Error(-34, "pg_region_variants_bases: buffer too small");
  if (!c.vr_bases) return 0;
  DevBuf flat;
  flat.reserve(c.vr_bases + 16);
  const RsTab V(c.vr_tab, c.vr_na + c.vr_np);
  const uint64_t nchunks = c.vr_pad_al / 16;
  RG_LAUNCH(k_rs_copy, grid_for(nchunks, RG_BLOCK, RS_DECODE_GRID), c.vr_blob.as<uint4>(), V, c.vr_na, nchunks, V.off,
            flat.as<char>());
  PG_HIP(hipMemcpyAsync(out, flat.p, c.vr_bases, hipMemcpyDeviceToHost, c.stream));
  c.sync();
  return c.vr_bases;
}

void region_variants_placed(Ctx& c, uint64_t* site, int64_t* record, int64_t* pos0, uint64_t* ref_row,
                            uint32_t* ref_allele, uint64_t* ref_len, uint64_t cap) {
  need(c.vr_ready, "pg_region_variants_placed", NEED_VARIANTS);
  const uint64_t n = c.vr_np;
  if (cap < n) throw Error(-34, "pg_region_variants_placed: buffer too small");
  if (!n) return;
  VrPlaced P(c.vr_place, n);
  get(c, site, P.site, 8 * n);
  get(c, record, P.rec, 8 * n);
  get(c, pos0, P.pos, 8 * n);
  get(c, ref_row, P.row, 8 * n);
  get(c, ref_allele, P.refal, 4 * n);
  get(c, ref_len, P.len, 8 * n);
  c.sync();
}

// the allele FASTA of the last region_variants with this call's record names: its size (out null, fd < 0),
// copied into out, or written to fd
uint64_t format_region_alleles_fasta(Ctx& c, const char* names, const int64_t* name_off, uint64_t n_names, char* out,
                                     uint64_t cap, int fd) {
  const char* what = fd >= 0 ? "pg_region_alleles_fasta_fd" : "pg_region_alleles_fasta";
  need(c.vr_ready && c.bb_ready, what, NEED_VARIANTS);
  const DevNames nm = names_upload(c, what, names, name_off, n_names, c.n_records, "alleles");
  const uint64_t na = c.vr_na;
  const RsTab V(c.vr_tab, na + c.vr_np);
  DevBuf toff, sdst, text;
  AlleleFastaLine line{V, BbSites(c.bb_sites, c.bb_ns), BbAlleles(c.bb_alleles, na), nm.bytes, nm.off, nullptr};
  const uint64_t total = text_measure(c, line, na, toff);
  if (!text_wanted(total, out, cap, fd, what) || !total) return total;
  text.reserve(total + 16);
  sdst.reserve(8 * (na + 1));
  line.sdst = sdst.as<ull>();
  text_write(c, line, na, toff, text.as<char>());
  if (c.vr_pad_al) {
    const uint64_t nchunks = c.vr_pad_al / 16;
    RG_LAUNCH(k_rs_copy, grid_for(nchunks, RG_BLOCK, RS_DECODE_GRID), c.vr_blob.as<uint4>(), V, na, nchunks,
              sdst.as<ull>(), text.as<char>());
  }
  return text_out(c, text.p, total, out, cap, fd, what, what);
}

// the VCF body of the last region_variants, the same three ways
uint64_t format_region_vcf(Ctx& c, const char* names, const int64_t* name_off, uint64_t n_names, char* out,
                           uint64_t cap, int fd) {
  const char* what = fd >= 0 ? "pg_region_vcf_fd" : "pg_region_vcf";
  need(c.vr_ready && c.bb_ready, what, NEED_VARIANTS);
  const DevNames nm = names_upload(c, what, names, name_off, n_names, c.n_records, "placed sites");
  const uint64_t na = c.vr_na, np = c.vr_np, nt = na + np;
  if (!np) return 0;
  const RsTab V(c.vr_tab, nt);
  const VrPlaced P(c.vr_place, np);
  const BbSites T(c.bb_sites, c.bb_ns);
  DevBuf items, toff, dst, text;
  items.reserve(8 * (np + 1));
  RG_LAUNCH(k_vr_items, grid_for(np, RG_BLOCK, 8192), P, T, np, c.bb_groups, items.as<ull>());
  const uint64_t ni = excl_scan_total(c, items.as<ull>(), items.as<ull>(), np);
  VcfLine line{V, P, T, BbAlleles(c.bb_alleles, na), c.bb_bits.as<ull>(), items.as<ull>(), c.vr_blob.as<char>(),
               nm.bytes, nm.off, nullptr, na, np, c.bb_groups, c.bb_words};
  const uint64_t total = text_measure(c, line, ni, toff);
  if (!text_wanted(total, out, cap, fd, what) || !total) return total;
  text.reserve(total + 16);
  dst.reserve(8 * (nt + 1));
  PG_HIP(hipMemsetAsync(dst.p, 0xFF, 8 * nt, c.stream));
  line.dst = dst.as<ull>();
  text_write(c, line, ni, toff, text.as<char>());
  const uint64_t nchunks = c.vr_pad / 16;
  RG_LAUNCH(k_rs_copy, grid_for(nchunks, RG_BLOCK, RS_DECODE_GRID), c.vr_blob.as<uint4>(), V, nt, nchunks,
            dst.as<ull>(), text.as<char>());
  return text_out(c, text.p, total, out, cap, fd, what, what);
}

}  // namespace pg
