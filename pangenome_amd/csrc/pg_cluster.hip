// pg_cluster.hip — the built-in clusterer of the rdBG (reference README step
// 4: "remove weak edges in rdBG and index the connect components"): edges of
// the `.xyz` with count < min_weight dropped, the connected components of the
// rest labelled, and the result written in the `.mcl` text format.
//
// Nodes are the distinct (key, value) pairs of the edge list, numbered in
// order of first appearance (n0_v0, then n1_v1 of each edge, list order).
// Components come from a lock-free union-find over those ids (one thread per
// edge), in which the larger root is always linked under the smaller, so a
// component's root is its smallest node id whatever the schedule; pointer
// jumping then flattens the trees, and a sort of the roots gives the sizes.  Clusters
// are ordered by (size descending, smallest id ascending), members by id; the
// result depends on the input alone.  Integer only.
//
// Coherence: k_cc_hook runs on all 8 XCDs and their L2s are not coherent for
// plain loads, so inside it every access to parent[] is an agent-scope
// atomic (relaxed load / relaxed store / CAS); a failed CAS goes on from the
// value it returned.  No loop waits for another thread: find() ends because
// parents strictly decrease, and a union retries only after it has observed
// that its root got a parent.  Every other phase is its own launch on
// c.stream and reads what earlier launches wrote.
//
// pg_cluster.h declares what pg_markov.hip shares with this file: the call's edge list (cc_edges), the node
// ids (cc_node_ids), the union (cc_union) and the steps from a hooked parent[] to the text and the label
// table (cc_finish).
//
// pg_cluster_sweep (the k_sw_* kernels) asks what the clusterer would form at every weight cut of a
// list: the same node ids and the same hook, run level by level from the highest threshold down on one
// parent[] that is flattened in place between levels.
#include <algorithm>
#include <climits>
#include <cstring>

#include "pg_cluster.h"
#include "pg_internal.h"
#include "pg_region.h"
#include "pg_text.h"

namespace pg {

// ------------------------------------------------------------ node ids
// slots sorted by (key, value), stably: a group's first slot is the node's first appearance
__global__ void k_cc_heads(const unsigned long long* __restrict__ skey, const unsigned long long* __restrict__ pos,
                           const unsigned* __restrict__ val0, uint64_t n, uint8_t* __restrict__ head,
                           unsigned* __restrict__ head32) {
  RG_LOOP(t, n) {
    const bool h = t == 0 || skey[t - 1] != skey[t] || val0[pos[t - 1]] != val0[pos[t]];
    head[t] = h;
    head32[t] = h;
  }
}
__global__ void k_cc_iota32(unsigned* __restrict__ out, uint64_t n) {
  RG_LOOP(i, n) out[i] = (unsigned)i;
}
// groups ordered by first appearance: group gsorted[r] is node r
__global__ void k_cc_rank(const unsigned long long* __restrict__ fsorted, const unsigned* __restrict__ gsorted,
                          uint64_t nu, const unsigned long long* __restrict__ tup, unsigned* __restrict__ rank_of_group,
                          unsigned long long* __restrict__ nkey, unsigned long long* __restrict__ nval) {
  RG_LOOP(r, nu) {
    rank_of_group[gsorted[r]] = (unsigned)r;
    if (!nkey) continue;                       // (the sweep needs the ids alone)
    const unsigned long long t = fsorted[r];
    nkey[r] = tup[2 * t];
    nval[r] = tup[2 * t + 1];
  }
}
__global__ void k_cc_ids(const unsigned long long* __restrict__ pos, const unsigned* __restrict__ gx,
                         const unsigned* __restrict__ head32, uint64_t nn, const unsigned* __restrict__ rank_of_group,
                         unsigned* __restrict__ id) {
  RG_LOOP(t, nn) id[pos[t]] = rank_of_group[gx[t] + head32[t] - 1u];
}

// ------------------------------------------------------------ union-find
__global__ void k_cc_init(unsigned* __restrict__ parent, uint64_t nu) {
  RG_LOOP(i, nu) parent[i] = (unsigned)i;
}

__global__ void k_cc_hook(const unsigned* __restrict__ id, const long long* __restrict__ cnt, uint64_t ne,
                          long long min_weight, unsigned* parent) {
  RG_LOOP(e, ne) {
    if (cnt[e] < min_weight) continue;
    const unsigned a = id[2 * e], b = id[2 * e + 1];
    if (a != b) cc_union(parent, a, b);
  }
}

// Flatten by pointer jumping: out[i] = in[in[i]], `in` only read, `out` a
// separate array.  Starting from parent[] (every node's 1st ancestor), round r
// leaves the 2^r-th ancestor (the root once past it); depths are below the
// node count, so bits_for(nu) rounds leave comp[i] = root of i with no
// convergence flag and no host round trip.  (The rdBG is made of long paths
// numbered in walk order, so the hooked trees are deep: one thread walking
// to its root took 10.9 ms of dependent loads on C3's table.)
__global__ void k_cc_jump(const unsigned* __restrict__ in, uint64_t nu, unsigned* __restrict__ out) {
  RG_LOOP(i, nu) out[i] = in[in[i]];
}

// ------------------------------------------------------------ sweep (pg_cluster_sweep)
// The kernels of the sweep step by whole blocks (SW_TILES), so that every lane of a wave reaches their
// ballots and rg_by_label.
#define SW_TILES(i, n, todo)                                                                          \
  for (uint64_t base_ = blockIdx.x * (uint64_t)RG_BLOCK, i = base_ + threadIdx.x; base_ < (n);        \
       base_ += (uint64_t)gridDim.x * RG_BLOCK, i = base_ + threadIdx.x)                              \
    if (const bool todo = i < (n); true)

// Level i of thr[0 .. nt) ascending holds the edges with thr[i] <= count < thr[i + 1] (the last level has
// no upper bound): band[i] = their number, counted in the block's LDS first; *maxw = the largest count.
__global__ void __launch_bounds__(RG_BLOCK) k_sw_bands(const long long* __restrict__ cnt, uint64_t ne,
                                                       const long long* __restrict__ thr, unsigned nt, ull* band,
                                                       long long* maxw) {
  __shared__ unsigned hist[SW_MAX_LEVELS];
  for (unsigned j = threadIdx.x; j < nt; j += RG_BLOCK) hist[j] = 0;
  __syncthreads();
  long long mx = LLONG_MIN;
  RG_LOOP(e, ne) {
    const long long w = cnt[e];
    mx = w > mx ? w : mx;
    unsigned lo = 0, hi = nt;                  // the levels below lo have thr <= w, the levels from hi on thr > w
    while (lo < hi) {
      const unsigned mid = (lo + hi) >> 1;
      if (thr[mid] <= w) lo = mid + 1; else hi = mid;
    }
    if (lo) atomicAdd(hist + (lo - 1), 1u);
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) { const long long v = __shfl_xor(mx, o); mx = v > mx ? v : mx; }
  if ((threadIdx.x & 63) == 0 && mx != LLONG_MIN) RG_MAX(maxw, mx);
  __syncthreads();
  for (unsigned j = threadIdx.x; j < nt; j += RG_BLOCK)
    if (hist[j]) RG_ADD(band + j, (ull)hist[j]);
}

// k_cc_hook over the edges of one level, lo <= count <= hi, on a parent[] that earlier levels left flat
// (parent[y] <= y: a legal start); *hooks += the unions made, the successful CASes, one add per wave.
// parent[] as in k_cc_hook: agent-scope atomics alone, a failed CAS goes on from the value it returned,
// no loop waits for another thread.
__global__ void __launch_bounds__(RG_BLOCK) k_sw_hook(const unsigned* __restrict__ id, const long long* __restrict__ cnt,
                                                      uint64_t ne, long long lo, long long hi, unsigned* parent,
                                                      ull* hooks) {
  SW_TILES(e, ne, todo) {
    bool won = false;
    if (todo && cnt[e] >= lo && cnt[e] <= hi) won = cc_union(parent, id[2 * e], id[2 * e + 1]);
    const ull m = __ballot(won);
    if (m && (int)(threadIdx.x & 63) == __ffsll(m) - 1) RG_ADD(hooks, (ull)__popcll(m));
  }
}

__global__ void k_sw_init(unsigned* __restrict__ parent, unsigned* __restrict__ size, uint64_t nu) {
  RG_LOOP(i, nu) {
    parent[i] = (unsigned)i;
    size[i] = 1u;
  }
}

// One round of the pointer jumping in place: parent[i] = its 4th ancestor (SW_HOPS pointers followed from
// its parent, the root once reached).  A pointer only ever moves to an ancestor, so whatever mix of this
// round's and earlier values a thread reads, it ends no farther from its root than a round over the values
// of the round's start would leave it: round r leaves the 4^r-th ancestor at least, and sw_rounds(nu)
// rounds flatten every tree, as k_cc_jump's bits_for(nu) doublings do.  *moved is set if a pointer moved.
// prev: the flag of the round before (null: the first round); clear, the trees were already flat
// (parent[p] == p is only ever read of a root, and a root stays one), and this round and every later
// one return at once: below the first levels most rounds do.
#define SW_HOPS 3
static int sw_rounds(uint64_t nu) { return (bits_for(nu) + 1) / 2; }
__global__ void __launch_bounds__(RG_BLOCK) k_sw_jump(unsigned* parent, uint64_t nu, const unsigned* prev,
                                                      unsigned* moved) {
  if (prev && !*prev) return;
  bool any = false;
  SW_TILES(i, nu, todo) {
    if (!todo) continue;
    const unsigned p0 = parent[i];
    unsigned p = p0;
    for (int h = 0; h < SW_HOPS; ++h) {
      const unsigned g = parent[p];
      if (g == p) break;
      p = g;
    }
    if (p != p0) {
      parent[i] = p;
      any = true;
    }
  }
  if (__ballot(any) && (threadIdx.x & 63) == 0) RG_OR(moved, 1u);
}

// The sizes follow the unions: size[] is 1 at every node before the first level and afterwards nonzero
// at the roots alone.  After a level's flatten, a node that still holds a size but is no root any more
// (it was hooked in this level) gives it to its root comp[i] and keeps 0.  A giver is no root, so
// nothing is added to it; a receiver is a root, so it gives nothing: the sums do not depend on the order.
// At a low threshold most givers of a wave share one root: a root shared by RG_AGG_MIN lanes or more
// gets one add for all of them (rg_by_label).  The adds over all levels are the unions, below nu.
__global__ void __launch_bounds__(RG_BLOCK) k_sw_size(const unsigned* __restrict__ comp, uint64_t nu, unsigned* size) {
  SW_TILES(i, nu, todo) {
    const unsigned s = todo ? size[i] : 0u;
    const unsigned r = s ? comp[i] : 0u;
    const bool give = s && r != (unsigned)i;
    const bool own = rg_by_label(give, (ull)r, [&](ull r0, bool mine, ull, bool leader) {
      const ull sum = rg_wave_sum(mine ? (ull)s : 0ull);
      if (leader) RG_ADD(size + r0, (unsigned)sum);
    });
    if (own) RG_ADD(size + r, s);
    if (give) size[i] = 0u;
  }
}
// over the sizes (nonzero at the roots): *largest = the largest, *singles += those equal to 1; reduced in
// the wave and the block first, two atomics per block
__global__ void __launch_bounds__(RG_BLOCK) k_sw_stats(const unsigned* __restrict__ size, uint64_t nu, ull* largest,
                                                       ull* singles) {
  __shared__ ull red[2][RG_BLOCK / 64];
  ull mx = 0, ones = 0;
  RG_LOOP(i, nu) {
    const unsigned s = size[i];
    mx = s > mx ? s : mx;
    ones += s == 1u;
  }
  mx = rg_wave_max(mx);
  ones = rg_wave_sum(ones);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = mx;
    red[1][threadIdx.x >> 6] = ones;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < RG_BLOCK / 64; ++w) {
      mx = red[0][w] > mx ? red[0][w] : mx;
      ones += red[1][w];
    }
    if (mx) RG_MAX(largest, mx);
    if (ones) RG_ADD(singles, ones);
  }
}

// ------------------------------------------------------------ order
// roots and sizes (the run lengths of the sorted comp[]) -> sort keys: size descending, root ascending
__global__ void k_cc_rootkeys(const unsigned* __restrict__ root, const unsigned* __restrict__ size, uint64_t nc,
                              unsigned long long* __restrict__ rkey) {
  RG_LOOP(r, nc) rkey[r] = ((unsigned long long)(0xFFFFFFFFu - size[r]) << 32) | (unsigned long long)root[r];
}
__global__ void k_cc_lines(const unsigned long long* __restrict__ rsorted, uint64_t nc,
                           unsigned* __restrict__ line_of_root) {
  RG_LOOP(r, nc) line_of_root[(unsigned)rsorted[r]] = (unsigned)r;
}
__global__ void k_cc_nodeline(const unsigned* __restrict__ comp, const unsigned* __restrict__ line_of_root, uint64_t nu,
                              unsigned* __restrict__ nl, unsigned* __restrict__ ni) {
  RG_LOOP(i, nu) {
    nl[i] = line_of_root[comp[i]];
    ni[i] = (unsigned)i;
  }
}

// ------------------------------------------------------------ text and labels
// token j of the file: node sm[j] as "<key>_<value>" and one separator (a tab, or the line's end after
// the last token of line sl[j]); the write pass also puts the token into the label list, in file order
struct MclLine {
  const ull *nkey, *nval;
  const unsigned *sm, *sl;
  uint64_t nu;
  long long *lkey, *lval, *lid;
  template <class S>
  __device__ __forceinline__ void operator()(S& s, uint64_t j) const {
    const unsigned m = sm[j];
    const ull key = nkey[m], val = nval[m];
    s.dec(key); s.ch('_'); s.dec(val);
    s.ch((j + 1 == nu || sl[j + 1] != sl[j]) ? '\n' : '\t');
    if constexpr (S::writes) {
      lkey[j] = (long long)key;
      lval[j] = (long long)val;
      lid[j] = (long long)sl[j];
    }
  }
};

CcEdges cc_edges(Ctx& c, const char* what, const uint64_t* h_tuples, const int64_t* h_counts, uint64_t n_edges) {
  CcEdges e;
  if (h_tuples) {
    uint64_t maxv = 0;
    for (uint64_t i = 0; i < 2 * n_edges; ++i) maxv = std::max<uint64_t>(maxv, h_tuples[2 * i + 1]);
    if (maxv > 0xFFFFFFFFull) throw Error(-22, std::string(what) + ": node value above 2^32");
    e.vbits = bits_for(maxv);
    e.up.reserve(40 * (n_edges + 1));
    if (n_edges) {
      PG_HIP(hipMemcpyAsync(e.up.p, h_tuples, 32 * n_edges, hipMemcpyHostToDevice, c.stream));
      PG_HIP(hipMemcpyAsync(e.up.as<unsigned long long>() + 4 * n_edges, h_counts, 8 * n_edges,
                            hipMemcpyHostToDevice, c.stream));
    }
    e.tup = e.up.as<unsigned long long>();
  } else {
    n_edges = c.n_edges;
    e.tup = c.edge_exp.as<unsigned long long>();
  }
  e.cnt = reinterpret_cast<const long long*>(e.tup + 4 * n_edges);
  e.n = n_edges;
  return e;
}

uint64_t cc_node_ids(Ctx& c, const char* what, const CcEdges& e, DevBuf& ids, DevBuf* nodes) {
  const unsigned long long* tup = e.tup;
  const uint64_t nn = 2 * e.n;
  uint64_t nu = 0;
  ids.reserve(4 * nn + 16);
  auto* id = ids.as<unsigned>();
  DevBuf w, flag, cntb, firsts, grp;
  w.reserve((8 + 8 + 8 + 8 + 8 + 4 + 4 + 4 + 4) * nn + 64);
  auto* key = w.as<unsigned long long>();
  auto* skey = key + nn;
  auto* pos = skey + nn;
  auto* pos2 = pos + nn;
  auto* tmpk = pos2 + nn;
  auto* val = reinterpret_cast<unsigned*>(tmpk + nn);
  auto* sval = val + nn;
  auto* head32 = sval + nn;
  auto* gx = head32 + nn;
  CC_LAUNCH(k_nodes, nn, tup, nn, key, val, pos);          // (pg_walk.hip: slot t = words 2t, 2t+1)
  sort_pairs(c, val, sval, pos, pos2, nn, e.vbits);                    // by value
  CC_LAUNCH(k_gather_key, nn, key, pos2, nn, tmpk);
  sort_pairs(c, tmpk, skey, pos2, pos, nn, 64);                        // then stably by key
  flag.reserve(nn + 16);
  CC_LAUNCH(k_cc_heads, nn, skey, pos, val, nn, flag.as<uint8_t>(), head32);
  with_temp(c, [&](void* tmp, size_t& bytes) {
    return rocprim::exclusive_scan(tmp, bytes, head32, gx, 0u, (size_t)nn, rocprim::plus<unsigned>(), c.stream);
  });
  // the groups' first slots, in sorted-group order; then ordered by that slot
  firsts.reserve(16 * nn + 16);
  auto* f0 = firsts.as<unsigned long long>();
  nu = select_flagged(c, pos, flag.as<uint8_t>(), f0, nn, cntb);
  if (nu >= (1ull << 32)) throw Error(-34, std::string(what) + ": 2^32 nodes or more");
  grp.reserve(4 * 3 * nu + 16);
  auto* g0 = grp.as<unsigned>();
  auto* gsorted = g0 + nu;
  auto* rank_of_group = gsorted + nu;
  CC_LAUNCH(k_cc_iota32, nu, g0, nu);
  sort_pairs(c, f0, f0 + nn, g0, gsorted, nu, bits_for(nn));
  unsigned long long *nkey = nullptr, *nval = nullptr;
  if (nodes) {
    nodes->reserve(16 * nu + 16);
    nkey = nodes->as<unsigned long long>();
    nval = nkey + nu;
  }
  CC_LAUNCH(k_cc_rank, nu, f0 + nn, gsorted, nu, tup, rank_of_group, nkey, nval);
  CC_LAUNCH(k_cc_ids, nn, pos, gx, head32, nn, rank_of_group, id);
  c.sync();                                    // (the sort buffers are freed here)
  return nu;
}

void cc_finish(Ctx& c, uint64_t nu, DevBuf& uf, const unsigned long long* nkey, const unsigned long long* nval) {
  c.clu_ready = false;
  c.clu_total = c.n_clusters = c.n_clu_nodes = 0;
  uint64_t nc = 0;
  if (nu) {
    // ---- d. the roots
    auto* parent = uf.as<unsigned>();
    auto* jump_a = parent + nu;
    auto* jump_b = jump_a + nu;
    auto* line_of_root = jump_b + nu;
    auto* nl = line_of_root + nu;
    auto* ni = nl + nu;
    auto* sl = ni + nu;
    auto* sm = sl + nu;
    auto* csorted = sm + nu;
    auto* uroot = csorted + nu;
    auto* usize = uroot + nu;
    const unsigned* comp = parent;
    for (int r = 0, rounds = bits_for(nu); r < rounds; ++r) {
      unsigned* out = (r & 1) ? jump_b : jump_a;
      CC_LAUNCH(k_cc_jump, nu, comp, nu, out);
      comp = out;
    }
    // ---- e. sizes as run lengths of the sorted roots; clusters by (size
    // descending, root ascending); nodes stably by line
    DevBuf rk, cntb;
    rk.reserve(8 * 2 * nu + 16);
    cntb.reserve(16);
    auto* rkey = rk.as<unsigned long long>();
    auto* rsorted = rkey + nu;
    with_temp(c, [&](void* tmp, size_t& bytes) {
      return rocprim::radix_sort_keys(tmp, bytes, comp, csorted, (size_t)nu, 0, bits_for(nu), c.stream);
    });
    with_temp(c, [&](void* tmp, size_t& bytes) {
      return rocprim::run_length_encode(tmp, bytes, csorted, (size_t)nu, uroot, usize, cntb.as<unsigned long long>(),
                                        c.stream);
    });
    {
      unsigned long long h = 0;
      PG_HIP(hipMemcpyAsync(&h, cntb.p, 8, hipMemcpyDeviceToHost, c.stream));
      c.sync();
      nc = h;
    }
    CC_LAUNCH(k_cc_rootkeys, nc, uroot, usize, nc, rkey);
    with_temp(c, [&](void* tmp, size_t& bytes) {
      return rocprim::radix_sort_keys(tmp, bytes, rkey, rsorted, (size_t)nc, 0, 64, c.stream);
    });
    CC_LAUNCH(k_cc_lines, nc, rsorted, nc, line_of_root);
    CC_LAUNCH(k_cc_nodeline, nu, comp, line_of_root, nu, nl, ni);
    sort_pairs(c, nl, sl, ni, sm, nu, bits_for(nc));
    // ---- f, g. the `.mcl` text (kept on the device) and the label list in file order
    c.lab_list.reserve(24 * (nu + 1));
    long long* L = c.lab_list.as<long long>();
    const MclLine line{nkey, nval, sm, sl, nu, L, L + nu, L + 2 * nu};
    // The root keys are done with (k_cc_lines, queued above, read them last), so their storage takes the
    // line offsets: rk holds 16 nu + 16 bytes, the offsets need 8 (nu + 1), and text_measure's reserve
    // therefore allocates nothing.
    DevBuf& off = rk;
    c.clu_total = text_measure(c, line, nu, off);
    c.clu_text.reserve(c.clu_total + 16);
    text_write(c, line, nu, off, c.clu_text.as<char>());
    lab_build(c, L, L + nu, L + 2 * nu, nu);
    c.n_labels = nu;
  } else {
    c.lab_list.reserve(24);
    lab_build(c, nullptr, nullptr, nullptr, 0);
    c.n_labels = 0;
  }
  c.sync();
  c.n_clusters = nc;
  c.n_clu_nodes = nu;
  c.clu_ready = true;
}

void cluster_cc(Ctx& c, const uint64_t* h_tuples, const int64_t* h_counts, uint64_t n_edges, int64_t min_weight) {
  const CcEdges e = cc_edges(c, "pg_cluster_cc", h_tuples, h_counts, n_edges);
  n_edges = e.n;
  c.clu_ready = false;
  c.clu_total = c.n_clusters = c.n_clu_nodes = 0;
  markov_drop(c);
  DevBuf ids, nodes, uf;                       // uint32 [nn] ids; uint64 [nu] keys, [nu] values; the union-find
  uint64_t nu = 0;
  if (n_edges) {
    // ---- a. node ids
    nu = cc_node_ids(c, "pg_cluster_cc", e, ids, &nodes);
    // ---- b, c. union-find over the surviving edges
    uf.reserve(4 * CC_UF_WORDS * nu + 16);
    CC_LAUNCH(k_cc_init, nu, uf.as<unsigned>(), nu);
    CC_LAUNCH(k_cc_hook, n_edges, ids.as<unsigned>(), e.cnt, n_edges, (long long)min_weight, uf.as<unsigned>());
  }
  cc_finish(c, nu, uf, nodes.as<unsigned long long>(), nodes.as<unsigned long long>() + nu);
}

// The cluster curve over thr[0 .. nt) ascending: one union-find that survives from the highest threshold
// down.  The components at thr[i] are those at thr[i + 1] plus the unions of level i's edges, and the
// larger root always goes under the smaller, so after every level a component's root is still its
// smallest node id and the flattened array (parent[y] <= y) is the next level's parent[].  Per level:
// the hook, the pointer jumping of cluster_cc's step d (in place: k_sw_jump), then the sizes, which
// follow the unions (k_sw_size); the figures stay in device arrays of nt entries and come back in one
// copy.  A query: nothing of the context's results is read or written.
void cluster_sweep(Ctx& c, const uint64_t* h_tuples, const int64_t* h_counts, uint64_t n_edges, const int64_t* thr,
                   uint64_t nt, uint64_t* n_nodes, int64_t* max_weight, uint64_t* edges, uint64_t* clusters,
                   uint64_t* largest, uint64_t* singletons) {
  const CcEdges e = cc_edges(c, "pg_cluster_sweep", h_tuples, h_counts, n_edges);
  n_edges = e.n;
  // [nt] thresholds, then band, hooks, largest, singles [nt] each, then the largest count
  DevBuf st;
  st.reserve(8 * (5 * nt + 1));
  auto* d_thr = st.as<long long>();
  auto* d_band = st.as<ull>() + nt;
  auto* d_hooks = d_band + nt;
  auto* d_largest = d_hooks + nt;
  auto* d_singles = d_largest + nt;
  auto* d_maxw = reinterpret_cast<long long*>(d_singles + nt);
  std::vector<ull> h(4 * nt + 1, 0);
  h[4 * nt] = (ull)LLONG_MIN;
  if (nt) PG_HIP(hipMemcpyAsync(d_thr, thr, 8 * nt, hipMemcpyHostToDevice, c.stream));
  PG_HIP(hipMemcpyAsync(d_band, h.data(), 8 * h.size(), hipMemcpyHostToDevice, c.stream));
  uint64_t nu = 0;
  if (n_edges) {
    RG_LAUNCH(k_sw_bands, grid_for(n_edges, RG_BLOCK, 1024), e.cnt, n_edges, d_thr, (unsigned)nt, d_band, d_maxw);
    DevBuf ids;                                // uint32 [2 n_edges]
    nu = cc_node_ids(c, "pg_cluster_sweep", e, ids, nullptr);       // ---- a (its scratch is freed on return)
    if (nt) {
      const int rounds = sw_rounds(nu);
      DevBuf uf, fl;                           // uint32 [nu] parent[], [nu] sizes; [nt][rounds] the jumps' flags
      uf.reserve(4 * 2 * nu + 16);
      fl.reserve(4 * nt * rounds);
      unsigned* parent = uf.as<unsigned>();
      unsigned* size = parent + nu;
      PG_HIP(hipMemsetAsync(fl.p, 0, 4 * nt * rounds, c.stream));
      CC_LAUNCH(k_sw_init, nu, parent, size, nu);
      const unsigned few = grid_for(nu, RG_BLOCK, 1024);            // (a round that returns at once costs its blocks)
      // the levels' edge counts (the stream is idle since step a: one early read).  A level without edges
      // changes nothing and queues nothing: its row is the row above it.
      PG_HIP(hipMemcpyAsync(h.data(), d_band, 8 * nt, hipMemcpyDeviceToHost, c.stream));
      c.sync();
      for (uint64_t i = nt; i-- > 0;) {        // ---- b. the levels, from the highest threshold down
        if (!h[i]) continue;
        const long long hi = i + 1 < nt ? (long long)thr[i + 1] - 1 : LLONG_MAX;
        CC_LAUNCH(k_sw_hook, n_edges, ids.as<unsigned>(), e.cnt, n_edges, (long long)thr[i], hi, parent,
                  d_hooks + i);                                     // ---- c
        unsigned* moved = fl.as<unsigned>() + i * rounds;
        for (int r = 0; r < rounds; ++r)                            // ---- d
          RG_LAUNCH(k_sw_jump, few, parent, nu, r ? moved + r - 1 : nullptr, moved + r);
        CC_LAUNCH(k_sw_size, nu, parent, nu, size);                 // ---- e
        RG_LAUNCH(k_sw_stats, few, size, nu, d_largest + i, d_singles + i);
      }
    }
  }
  PG_HIP(hipMemcpyAsync(h.data(), d_band, 8 * h.size(), hipMemcpyDeviceToHost, c.stream));   // ---- f
  c.sync();
  if (n_nodes) *n_nodes = nu;
  if (max_weight) *max_weight = n_edges ? (int64_t)h[4 * nt] : 0;
  ull kept = 0, hooked = 0, big = nu ? 1 : 0, single = nu;      // (above every edge: each node alone)
  for (uint64_t i = nt; i-- > 0;) {
    kept += h[i];
    hooked += h[nt + i];
    if (h[i]) {                                                   // (a level without edges ran no size pass)
      big = h[2 * nt + i];
      single = h[3 * nt + i];
    }
    if (edges) edges[i] = kept;
    if (clusters) clusters[i] = nu - hooked;
    if (largest) largest[i] = big;
    if (singletons) singletons[i] = single;
  }
}

// the `.mcl` text of the last cluster_cc or cluster_markov: its size (out null, fd < 0), copied
// into out, or written to descriptor fd
uint64_t format_clusters(Ctx& c, char* out, uint64_t cap, int fd) {
  if (!c.clu_ready) throw Error(-22, "pg_clusters_format: no clustering (call pg_cluster_cc or pg_cluster_markov first)");
  return text_out(c, c.clu_text.p, c.clu_total, out, cap, fd, "pg_clusters_format", "pg_clusters_format_fd");
}

}  // namespace pg
