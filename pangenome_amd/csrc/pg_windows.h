// pg_windows.h — the window enumerator the passes over the records share
// (pg_walk.hip: edges and rows; pg_colors.hip: the k-mer colours): the windows
// of one record as pg_build_dbg inserts them, the runs of WW windows a thread
// takes, and the host's plan of the runs of the walked records.
#pragma once
#include <vector>

#include "pg_internal.h"

namespace pg {

constexpr int WW = 16;        // windows per thread run
constexpr int WBLOCK = 256;

// --------------------------------------------------------------- windows
// One window of each strand at forward position q of record (rs, n):
// forward window q and reverse-strand window p' = n-k-q, with their keys,
// the reverse complement of each key, and the lastc of pred/succ.
struct Win {
  uint64_t xf, xr;        // forward-window key, reverse-strand-window key
  uint64_t xf_rc, xr_rc;  // reverse complements (for the canonical table lookup)
  uint32_t fp, fs, rp, rs;
};

// Explicit strand enumeration for records with n <= k+1 (rare).
__device__ inline void short_window(const uint8_t* cls, long long rs, long long n, int k, uint64_t shift,
                                    int strand, long long j, uint64_t& x, uint32_t& pred, uint32_t& succ) {
  auto S = [&](long long i) -> uint32_t {
    return strand == 0 ? (uint32_t)cls[rs + i] : comp_class(cls[rs + n - 1 - i]);
  };
  if (n < k) { x = SENTINEL; pred = LAM_HASH; succ = LAM_DOLLAR; return; }
  uint64_t K0 = 0, pw = 1;
  for (int t = 0; t < k; ++t) { K0 += (uint64_t)digit_fw(S(t)) * pw; pw *= 5; }
  if (n == k) { x = K0; pred = LAM_HASH; succ = LAM_DOLLAR; return; }
  if (j == 0) { x = K0; pred = LAM_HASH; succ = lam_fw(S(k)); return; }
  x = K0 / 5 + (uint64_t)digit_fw(S(1)) * shift;     // numba's unbound loop variable == 0
  pred = lam_fw(S(1));
  succ = LAM_DOLLAR;
}

// Iterate windows q in [q0, q1) of one record and call f(q, Win).
template <class F>
__device__ __forceinline__ void for_windows(const uint8_t* __restrict__ cls, long long rs, long long n, int k,
                                            uint64_t shift, long long q0, long long q1, F&& f) {
  if (n <= k + 1) {
    for (long long q = q0; q < q1; ++q) {
      Win w;
      const long long nw = n < k ? 1 : n - k + 1;
      short_window(cls, rs, n, k, shift, 0, q, w.xf, w.fp, w.fs);
      short_window(cls, rs, n, k, shift, 1, nw - 1 - q, w.xr, w.rp, w.rs);
      w.xf_rc = w.xf == SENTINEL ? SENTINEL : rc_key(w.xf, k);
      w.xr_rc = w.xr == SENTINEL ? SENTINEL : rc_key(w.xr, k);
      f(q, w);
    }
    return;
  }
  const long long last = n - k;
  uint64_t K = 0, Kr = 0;
  for (long long q = q0; q < q1; ++q) {
    const uint64_t p = (uint64_t)(rs + q);
    if (q == q0) {
      uint64_t pw = 1;
      for (int j = 0; j < k; ++j) {
        const uint32_t cj = cls[p + j];
        K += (uint64_t)digit_fw(cj) * pw;
        Kr = Kr * 5 + digit_rc(cj);
        pw *= 5;
      }
    } else {
      const uint32_t dout = cls[p - 1], din = cls[p + k - 1];
      K = (K - digit_fw(dout)) * INV5 + (uint64_t)digit_fw(din) * shift;
      Kr = (Kr - (uint64_t)digit_rc(dout) * shift) * 5 + digit_rc(din);
    }
    Win w;
    w.xf = K; w.xf_rc = Kr; w.xr = Kr; w.xr_rc = K;
    w.fp = q == 0 ? LAM_HASH : lam_fw(cls[p - (q == last ? 2 : 1)]);
    w.fs = q == last ? LAM_DOLLAR : lam_fw(cls[p + k]);
    w.rp = q == last ? LAM_HASH : lam_rc(cls[p + k + (q == 0 ? 1 : 0)]);
    w.rs = q == 0 ? LAM_DOLLAR : lam_rc(cls[p - 1]);
    f(q, w);
  }
}

// ------------------------------------------------------------------ runs
// The walked records and their runs of WW windows: run u belongs to the last
// walked record wr with run_off[wr] <= u.
struct WalkRuns {
  const uint8_t* cls;
  const long long* rec_start;
  const long long* rec_len;
  const unsigned long long* run_off;   // per walked record: first run index (size nrec+1)
  const int* run_rec;                  // walked record -> record index
  uint64_t nrec;                       // walked records
  int k; uint64_t shift;
};

__device__ __forceinline__ void run_locate(const WalkRuns& a, uint64_t u, uint64_t& wr, int& r, long long& rs,
                                           long long& n, long long& q0, long long& q1) {
  uint64_t lo = 0, hi = a.nrec;              // last wr with run_off[wr] <= u
  while (lo < hi) {
    uint64_t mid = (lo + hi) >> 1;
    if (a.run_off[mid] <= u) lo = mid + 1; else hi = mid;
  }
  wr = lo - 1;
  r = a.run_rec[wr];
  rs = a.rec_start[r];
  n = a.rec_len[r];
  const long long nw = n < a.k ? 1 : n - a.k + 1;
  q0 = (long long)(u - a.run_off[wr]) * WW;
  q1 = q0 + WW < nw ? q0 + WW : nw;
}

// ------------------------------------------------------------------ host
struct WalkPlan {
  std::vector<int> recs;                   // walked records, in order
  std::vector<unsigned long long> run_off; // per walked record
  uint64_t nruns = 0;
  DevBuf d_recs, d_run_off;
};

// the runs of the records with bit 0 of h_rec_flag set (NULL: all), uploaded on c.stream
inline void plan_walk(Ctx& c, const uint8_t* h_rec_flag, WalkPlan& P) {
  const uint64_t R = c.n_records;
  P.recs.clear(); P.run_off.clear();
  uint64_t runs = 0;
  for (uint64_t r = 0; r < R; ++r) {
    if (h_rec_flag && !(h_rec_flag[r] & 1)) continue;
    const int64_t n = c.h_rec_len[r];
    const int64_t nw = n < c.k ? 1 : n - c.k + 1;
    P.recs.push_back((int)r);
    P.run_off.push_back(runs);
    runs += (uint64_t)((nw + WW - 1) / WW);
  }
  P.run_off.push_back(runs);
  P.nruns = runs;
  P.d_recs.reserve(4 * (P.recs.size() + 1));
  P.d_run_off.reserve(8 * P.run_off.size());
  if (!P.recs.empty())
    PG_HIP(hipMemcpyAsync(P.d_recs.p, P.recs.data(), 4 * P.recs.size(), hipMemcpyHostToDevice, c.stream));
  PG_HIP(hipMemcpyAsync(P.d_run_off.p, P.run_off.data(), 8 * P.run_off.size(), hipMemcpyHostToDevice, c.stream));
}

// the record and run fields of a pass's arguments (the class bytes are filled in first)
inline void fill_runs(Ctx& c, WalkPlan& P, WalkRuns& a) {
  ensure_cls(c);                              // (the walks read class bytes)
  a.cls = c.cls.as<uint8_t>();
  a.rec_start = c.rec_start.as<long long>();
  a.rec_len = c.rec_len.as<long long>();
  a.run_off = P.d_run_off.as<unsigned long long>();
  a.run_rec = P.d_recs.as<int>();
  a.nrec = P.recs.size();
  a.k = c.k;
  a.shift = pow5(c.k - 1);
}

}  // namespace pg
