// pg_text.h — how every text of the library is made: a line is written once,
// as a functor over a sink, and the same functor first counts its bytes
// (TextCount) and then writes them (TextWrite), so the two cannot disagree.
//
// A line functor is trivially copyable, holds the table's column pointers and
// has one   template <class S> void operator()(S& s, uint64_t i) const
// that emits line i through the sink's members.  text_measure runs it over n
// lines with the counting sink and scans the lengths into offsets; text_write
// runs it again with the writing sink at out + off[i].  Host code calls the
// functor in a loop (pg_format_xyz, pg_format_rows).  The `.xyz` and the rows
// line, which the device and the host both write, are defined here.
#pragma once
#include "pg_prim.h"

namespace pg {

// decimal digits of v
__host__ __device__ __forceinline__ uint32_t ndig(ull v) {
  uint32_t d = 1;
  while (v >= 10ull) { v /= 10ull; ++d; }
  return d;
}
__host__ __device__ __forceinline__ char* put_dec(char* o, ull v) {
  const uint32_t d = ndig(v);
  for (uint32_t i = d; i-- > 0;) { o[i] = (char)('0' + v % 10ull); v /= 10ull; }
  return o + d;
}

// The two sinks.  gap(len) leaves len bytes for someone else to fill: the
// writing sink returns where they start in the text, the counting one 0.
// bytes() of the counting sink does not read its source.
struct TextCount {
  static constexpr bool writes = false;
  ull n = 0;
  __host__ __device__ __forceinline__ void dec(ull v) { n += ndig(v); }
  __host__ __device__ __forceinline__ void sdec(long long v) { n += v < 0 ? 1 + ndig(0ull - (ull)v) : ndig((ull)v); }
  __host__ __device__ __forceinline__ void ch(char) { ++n; }
  template <size_t N>
  __host__ __device__ __forceinline__ void lit(const char (&)[N]) { n += N - 1; }
  __host__ __device__ __forceinline__ void bytes(const char*, ull len) { n += len; }
  __host__ __device__ __forceinline__ ull gap(ull len) { n += len; return 0; }
};
struct TextWrite {
  static constexpr bool writes = true;
  char* text;                      // the text's first byte (gap's offsets count from it)
  char* o;                         // the next byte to write
  __host__ __device__ __forceinline__ void dec(ull v) { o = put_dec(o, v); }
  __host__ __device__ __forceinline__ void sdec(long long v) {
    if (v < 0) { *o++ = '-'; v = (long long)(0ull - (ull)v); }
    o = put_dec(o, (ull)v);
  }
  __host__ __device__ __forceinline__ void ch(char c) { *o++ = c; }
  template <size_t N>
  __host__ __device__ __forceinline__ void lit(const char (&s)[N]) {
#pragma unroll
    for (size_t i = 0; i + 1 < N; ++i) o[i] = s[i];
    o += N - 1;
  }
  __host__ __device__ __forceinline__ void bytes(const char* __restrict__ p, ull len) {
    for (ull b = 0; b < len; ++b) o[b] = p[b];
    o += len;
  }
  __host__ __device__ __forceinline__ ull gap(ull len) {
    const ull at = (ull)(o - text);
    o += len;
    return at;
  }
};

template <class Line>
__global__ void k_text_len(Line line, uint64_t n, ull* __restrict__ len) {
  RG_LOOP(i, n) {
    TextCount s;
    line(s, i);
    len[i] = s.n;
  }
}
template <class Line>
__global__ void k_text_write(Line line, uint64_t n, const ull* __restrict__ off, char* __restrict__ out) {
  RG_LOOP(i, n) {
    TextWrite s{out, out + off[i]};
    line(s, i);
  }
}
// The bytes of n lines; off[0 .. n]: where each starts (off[n]: their sum).  The lengths are written
// into off and scanned in place.
template <class Line>
static uint64_t text_measure(Ctx& c, const Line& line, uint64_t n, DevBuf& off) {
  if (!n) return 0;
  off.reserve(8 * (n + 1));
  RG_LAUNCH(k_text_len<Line>, grid_for(n, RG_BLOCK, 8192), line, n, off.as<ull>());
  return excl_scan_total(c, off.as<ull>(), off.as<ull>(), n);
}
// the n lines written at out + off[i], on c.stream
template <class Line>
static void text_write(Ctx& c, const Line& line, uint64_t n, const DevBuf& off, char* out) {
  if (n) RG_LAUNCH(k_text_write<Line>, grid_for(n, RG_BLOCK, 8192), line, n, off.as<ull>(), out);
}

// `.xyz` line "%d_%d\t%d_%d\t%d\n" (:1901), the keys printed as unsigned
struct XyzLine {
  const ull* tup;                  // [n][4]
  const long long* cnt;
  template <class S>
  __host__ __device__ __forceinline__ void operator()(S& s, uint64_t i) const {
    const ull* t = tup + 4 * i;
    s.dec(t[0]); s.ch('_'); s.dec(t[1]); s.ch('\t');
    s.dec(t[2]); s.ch('_'); s.dec(t[3]); s.ch('\t');
    s.sdec(cnt[i]); s.ch('\n');
  }
};
// region row "%s\t%d\t%d\t%s\t%d\n" (:1947-1949); the qid of record r is
// names[name_off[r] .. name_off[r + 1])
struct RowLine {
  const long long* rows;           // [n][5]
  const char* names;
  const long long* name_off;
  template <class S>
  __host__ __device__ __forceinline__ void operator()(S& s, uint64_t i) const {
    const long long* w = rows + 5 * i;
    s.bytes(names + name_off[w[0]], (ull)(name_off[w[0] + 1] - name_off[w[0]]));
    s.ch('\t'); s.sdec(w[1]); s.ch('\t'); s.sdec(w[2]); s.ch('\t');
    s.ch(w[3] == 1 ? '+' : '-'); s.ch('\t'); s.sdec(w[4]); s.ch('\n');
  }
};

}  // namespace pg
