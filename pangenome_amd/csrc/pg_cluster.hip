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
#include <algorithm>
#include <cstring>

#include "pg_internal.h"
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

__device__ __forceinline__ unsigned cc_load(const unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// root of x, with path halving; parent[y] < y for every non-root y, so the walk ends
__device__ __forceinline__ unsigned cc_find(unsigned* parent, unsigned x) {
  for (;;) {
    const unsigned p = cc_load(parent + x);
    if (p == x) return x;
    const unsigned g = cc_load(parent + p);
    if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
  }
}

__global__ void k_cc_hook(const unsigned* __restrict__ id, const long long* __restrict__ cnt, uint64_t ne,
                          long long min_weight, unsigned* parent) {
  RG_LOOP(e, ne) {
    if (cnt[e] < min_weight) continue;
    unsigned a = id[2 * e], b = id[2 * e + 1];
    if (a == b) continue;
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    while (a != b) {
      if (a < b) { const unsigned t = a; a = b; b = t; }        // the larger root goes under the smaller
      unsigned expect = a;
      if (__hip_atomic_compare_exchange_strong(parent + a, &expect, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT))
        break;
      a = cc_find(parent, expect);                                // a got a parent meanwhile: go on from it
      b = cc_find(parent, b);
    }
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

// one thread per item of n, up to 8192 blocks
#define CC_LAUNCH(kern, n, ...) RG_LAUNCH(kern, grid_for((n), RG_BLOCK, 8192), __VA_ARGS__)

void cluster_cc(Ctx& c, const uint64_t* h_tuples, const int64_t* h_counts, uint64_t n_edges, int64_t min_weight) {
  DevBuf up;
  const unsigned long long* tup;
  const long long* cnt;
  int vbits = 32;                              // (the edge pass holds values as 32-bit words)
  if (h_tuples) {
    uint64_t maxv = 0;
    for (uint64_t i = 0; i < 2 * n_edges; ++i) maxv = std::max<uint64_t>(maxv, h_tuples[2 * i + 1]);
    if (maxv > 0xFFFFFFFFull) throw Error(-22, "pg_cluster_cc: node value above 2^32");
    vbits = bits_for(maxv);
    up.reserve(40 * (n_edges + 1));
    if (n_edges) {
      PG_HIP(hipMemcpyAsync(up.p, h_tuples, 32 * n_edges, hipMemcpyHostToDevice, c.stream));
      PG_HIP(hipMemcpyAsync(up.as<unsigned long long>() + 4 * n_edges, h_counts, 8 * n_edges, hipMemcpyHostToDevice,
                            c.stream));
    }
    tup = up.as<unsigned long long>();
    cnt = reinterpret_cast<const long long*>(tup + 4 * n_edges);
  } else {
    n_edges = c.n_edges;
    tup = c.edge_exp.as<unsigned long long>();
    cnt = reinterpret_cast<const long long*>(tup + 4 * n_edges);
  }
  c.clu_ready = false;
  c.clu_total = c.n_clusters = c.n_clu_nodes = 0;
  const uint64_t nn = 2 * n_edges;
  uint64_t nu = 0, nc = 0;
  if (nn) {
    // ---- a. node ids: slots sorted by value, then stably by key, positions carried
    DevBuf ids, nodes;                         // uint32 [nn] ids; uint64 [nu] keys, [nu] values
    ids.reserve(4 * nn + 16);
    auto* id = ids.as<unsigned>();
    unsigned long long *nkey, *nval;
    {
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
      sort_pairs(c, val, sval, pos, pos2, nn, vbits);                      // by value
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
      if (nu >= (1ull << 32)) throw Error(-34, "pg_cluster_cc: 2^32 nodes or more");
      grp.reserve(4 * 3 * nu + 16);
      auto* g0 = grp.as<unsigned>();
      auto* gsorted = g0 + nu;
      auto* rank_of_group = gsorted + nu;
      CC_LAUNCH(k_cc_iota32, nu, g0, nu);
      sort_pairs(c, f0, f0 + nn, g0, gsorted, nu, bits_for(nn));
      nodes.reserve(16 * nu + 16);
      nkey = nodes.as<unsigned long long>();
      nval = nkey + nu;
      CC_LAUNCH(k_cc_rank, nu, f0 + nn, gsorted, nu, tup, rank_of_group, nkey, nval);
      CC_LAUNCH(k_cc_ids, nn, pos, gx, head32, nn, rank_of_group, id);
      c.sync();                                // (the sort buffers are freed here)
    }
    // ---- b-d. union-find over the surviving edges, then the roots and sizes
    DevBuf uf;                                 // uint32 [nu] x 11
    uf.reserve(4 * 11 * nu + 16);
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
    CC_LAUNCH(k_cc_init, nu, parent, nu);
    CC_LAUNCH(k_cc_hook, n_edges, id, cnt, n_edges, (long long)min_weight, parent);
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

// the `.mcl` text of the last cluster_cc: its size (out null, fd < 0), copied
// into out, or written to descriptor fd
uint64_t format_clusters(Ctx& c, char* out, uint64_t cap, int fd) {
  if (!c.clu_ready) throw Error(-22, "pg_clusters_format: no clustering (call pg_cluster_cc first)");
  return text_out(c, c.clu_text.p, c.clu_total, out, cap, fd, "pg_clusters_format", "pg_clusters_format_fd");
}

}  // namespace pg
