// pg_abi.hip — extern "C" entry points of include/pangenome.h.
#include <chrono>
#include <cstring>
#include <string>

#include "../../include/pangenome.h"
#include "pg_internal.h"
#include "pg_text.h"

struct pg_ctx {
  pg::Ctx c;
};

static thread_local std::string g_err;

template <class F>
static int guard(F&& f) {
  try {
    f();
    return PG_OK;
  } catch (const pg::Error& e) {
    g_err = e.what();
    return e.code;
  } catch (const std::bad_alloc&) {
    g_err = "out of host memory";
    return PG_ENOMEM;
  } catch (const std::exception& e) {
    g_err = e.what();
    return PG_EDEVICE;
  }
}

static void fill_stats(const pg::Ctx& c, pg_stats* s) {
  if (!s) return;
  s->n_bytes = c.n_bytes;
  s->n_records = c.n_records;
  s->n_bases = c.n_bases;
  s->n_windows = c.windows_total;
  s->n_dbg = c.n_dbg;
  s->n_rdbg = c.n_rdbg;
  s->n_slots = c.n_canon;
  s->table_capacity = c.cap;
  s->ms_parse = c.ms_parse;
  s->ms_clear = c.ms_clear;
  s->ms_insert = c.ms_insert;
  s->ms_scan = c.ms_scan;
  s->n_records_a = c.n_records_a;
  s->ms_split = c.ms_split;
  s->ms_range = c.ms_range;
  s->sentinel = c.sentinel;
  s->build_flags = (c.early_split_used ? 1u : 0u) | ((uint64_t)std::min(255, std::max(0, c.bc_attempts - 1)) << 8) |
                   ((uint64_t)std::min(255, std::max(0, c.split_passes)) << 16);
  s->n_work_items = c.work_items;
}

extern "C" {

const char* pg_last_error(void) { return g_err.c_str(); }

int pg_create(pg_ctx** out, int device, int k) {
  return guard([&] {
    if (!out) throw pg::Error(PG_EINVAL, "pg_create: out is NULL");
    int n = 0;
    PG_HIP(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) throw pg::Error(PG_EINVAL, "pg_create: no HIP device " + std::to_string(device));
    PG_HIP(hipSetDevice(device));
    auto* x = new pg_ctx();
    x->c.device = device;
    x->c.k = k < 1 ? 1 : (k > 27 ? 27 : k);
    PG_HIP(hipStreamCreateWithFlags(&x->c.stream, hipStreamNonBlocking));
    PG_HIP(hipStreamCreateWithFlags(&x->c.stream2, hipStreamNonBlocking));
    PG_HIP(hipStreamCreateWithFlags(&x->c.stream3, hipStreamNonBlocking));
    {
      int lo = 0, hi = 0;
      PG_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
      PG_HIP(hipStreamCreateWithPriority(&x->c.stream_hi, hipStreamNonBlocking, hi));
    }
    for (auto& e : x->c.ev) PG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto& e : x->c.cev) PG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    PG_HIP(hipEventCreateWithFlags(&x->c.rec_ev, hipEventDisableTiming));
    PG_HIP(hipEventCreateWithFlags(&x->c.ext_ev, hipEventDisableTiming));
    PG_HIP(hipDeviceGetAttribute(&x->c.n_cu, hipDeviceAttributeMultiprocessorCount, device));
    *out = x;
  });
}

void pg_destroy(pg_ctx* x) {
  if (!x) return;
  pg::Ctx& c = x->c;
  (void)hipSetDevice(c.device);
  (void)hipStreamSynchronize(c.stream);
  pg::DevBuf* bufs[] = {&c.fasta_own, &c.span_sum, &c.span_start, &c.n_sel, &c.rec_start, &c.rec_len,
                        &c.rec_hdr, &c.rec_ptr, &c.rec_flag, &c.cls, &c.p2, &c.e16, &c.scratch, &c.table, &c.ovf, &c.flags,
                        &c.recA_key, &c.recA_mw, &c.ctrA, &c.recS_key[0], &c.recS_key[1], &c.recS_mw[0],
                        &c.recS_mw[1], &c.ctrS, &c.snapA, &c.rseg, &c.k5_ctr, &c.tile_sched, &c.tile_desc, &c.tile_geo, &c.k3_queue,
                        &c.k3_hint, &c.part_cnt, &c.tile_cnt, &c.tile_off, &c.occ, &c.edge_tab, &c.pair_tab,
                        &c.edge_out, &c.edge_exp, &c.lab_tab, &c.lab_list, &c.rows_buf, &c.xyz_off,
                        &c.text_buf, &c.clu_text, &c.mk_mat, &c.fr_tab, &c.fr_spec, &c.fr_grp, &c.fr_text,
                        &c.cmp_shared, &c.cmp_curve, &c.kc_keys, &c.kc_bits, &c.kc_stat, &c.kc_shared, &c.kc_curve, &c.nj_dist, &c.rg_nodes, &c.rg_links, &c.rg_paths, &c.rg_steps, &c.rg_text,
                        &c.rs_tab, &c.rs_blob, &c.preload,
                        &c.dump_cnt};
  for (auto* b : bufs) b->release();
  pg::pool_destroy(c);
  c.stage_pin.release();
  c.rec_pack.release();
  c.h_pin.release();
  c.h_out.release();
  c.tile_pin.release();
  for (auto& b : c.dump_pin) b.release();
  c.t0.destroy();
  c.t1.destroy();
  c.t6.destroy();
  c.t_rs.destroy();
  c.t_nj.destroy();
  for (auto& t : c.t_bt) t.destroy();
  for (auto& t : c.t_kc) t.destroy();
  for (auto& e : c.ev)
    if (e) (void)hipEventDestroy(e);
  for (auto e : c.cev)
    if (e) (void)hipEventDestroy(e);
  if (c.rec_ev) (void)hipEventDestroy(c.rec_ev);
  if (c.ext_ev) (void)hipEventDestroy(c.ext_ev);
  if (c.stream_hi) (void)hipStreamDestroy(c.stream_hi);
  (void)hipStreamDestroy(c.stream3);
  (void)hipStreamDestroy(c.stream2);
  (void)hipStreamDestroy(c.stream);
  delete x;
}

int pg_get_k(const pg_ctx* x) { return x ? x->c.k : -1; }

int pg_stream_wait(pg_ctx* x, void* stream) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_stream_wait: ctx is NULL");
    pg::Ctx& c = x->c;
    PG_HIP(hipSetDevice(c.device));
    PG_HIP(hipEventRecord(c.ext_ev, reinterpret_cast<hipStream_t>(stream)));
    for (hipStream_t s : {c.stream, c.stream2, c.stream3, c.stream_hi})
      if (s) PG_HIP(hipStreamWaitEvent(s, c.ext_ev, 0));
  });
}

int pg_set_fasta(pg_ctx* x, const uint8_t* host, uint64_t n) {
  return guard([&] {
    if (!x || (!host && n)) throw pg::Error(PG_EINVAL, "pg_set_fasta: bad arguments");
    pg::Ctx& c = x->c;
    PG_HIP(hipSetDevice(c.device));
    c.fasta_own.reserve(n + 64);
    {                                          // pageable input through the pinned staging ring
      pg::Upload up(c, c.fasta_own.as<uint8_t>(), host, n, c.h2d_chunk);
      for (uint64_t i = 0; i < up.chunks(); ++i) {
        up.wait_queued(i);
        PG_HIP(hipStreamWaitEvent(c.stream, c.cev[i & 15], 0));
        up.consumed(i);
      }
      up.finish();
    }
    c.sync();
    c.d_fasta = c.fasta_own.as<uint8_t>();
    c.n_bytes = n;
    c.parsed = c.built = c.reduced = false;
  });
}

int pg_set_fasta_device(pg_ctx* x, const uint8_t* dev, uint64_t n) {
  return guard([&] {
    if (!x || (!dev && n)) throw pg::Error(PG_EINVAL, "pg_set_fasta_device: bad arguments");
    pg::Ctx& c = x->c;
    PG_HIP(hipSetDevice(c.device));
    if (reinterpret_cast<uintptr_t>(dev) % 16 != 0) {
      c.fasta_own.reserve(n + 64);
      PG_HIP(hipMemcpyAsync(c.fasta_own.p, dev, n, hipMemcpyDeviceToDevice, c.stream));
      c.sync();
      c.d_fasta = c.fasta_own.as<uint8_t>();
    } else {
      c.d_fasta = dev;
    }
    c.n_bytes = n;
    c.parsed = c.built = c.reduced = false;
  });
}

int pg_parse_host(pg_ctx* x, const uint8_t* host, uint64_t n, uint64_t* n_records, uint64_t* n_bases) {
  return guard([&] {
    if (!x || (!host && n)) throw pg::Error(PG_EINVAL, "pg_parse_host: bad arguments");
    pg::Ctx& c = x->c;
    PG_HIP(hipSetDevice(c.device));
    auto t0 = std::chrono::steady_clock::now();
    c.fasta_own.reserve(n + 64);
    c.d_fasta = c.fasta_own.as<uint8_t>();
    c.n_bytes = n;
    c.parsed = c.built = c.reduced = false;
    pg::parse_fasta(c, host);
    c.sync();                                  // (the emission may still run when parse_fasta returns)
    c.ms_parse = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (n_records) *n_records = c.n_records;
    if (n_bases) *n_bases = c.n_bases;
  });
}

int pg_parse(pg_ctx* x, uint64_t* n_records, uint64_t* n_bases) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_parse: ctx is NULL");
    pg::Ctx& c = x->c;
    PG_HIP(hipSetDevice(c.device));
    if (!c.d_fasta && c.n_bytes) throw pg::Error(PG_EINVAL, "pg_parse: no FASTA set");
    auto t0 = std::chrono::steady_clock::now();
    pg::parse_fasta(c);
    c.sync();                                  // (the emission may still run when parse_fasta returns)
    c.ms_parse = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c.built = c.reduced = false;
    if (n_records) *n_records = c.n_records;
    if (n_bases) *n_bases = c.n_bases;
  });
}

int pg_records(const pg_ctx* x, int64_t* seq_len, int64_t* hdr_start, int64_t* hdr_len, int64_t* ptr) {
  return guard([&] {
    if (!x || !x->c.parsed) throw pg::Error(PG_EINVAL, "pg_records: not parsed");
    const pg::Ctx& c = x->c;
    const size_t R = c.n_records;
    if (seq_len && R) std::memcpy(seq_len, c.h_rec_len.data(), 8 * R);
    if (hdr_start && R) std::memcpy(hdr_start, c.h_rec_hdr_start.data(), 8 * R);
    if (hdr_len && R) std::memcpy(hdr_len, c.h_rec_hdr_len.data(), 8 * R);
    if (ptr && R) std::memcpy(ptr, c.h_rec_ptr.data(), 8 * R);
  });
}

int pg_build_dbg(pg_ctx* x, const uint8_t* rec_flags, int extra_empty, int rc0, pg_stats* stats) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_build_dbg: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::build_dbg(x->c, rec_flags, extra_empty, rc0 != 0);
    fill_stats(x->c, stats);
  });
}

int pg_build_rdbg(pg_ctx* x, uint64_t* n_rdbg, pg_stats* stats) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_build_rdbg: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::build_rdbg(x->c);
    if (n_rdbg) *n_rdbg = x->c.n_rdbg;
    fill_stats(x->c, stats);
  });
}

int pg_build(pg_ctx* x, const uint8_t* rec_flags, int extra_empty, int rc0, uint64_t* n_rdbg, pg_stats* stats) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_build: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::build_dbg(x->c, rec_flags, extra_empty, rc0 != 0);
    pg::build_rdbg(x->c);                      // (the degree scan ran inside the build)
    if (n_rdbg) *n_rdbg = x->c.n_rdbg;
    fill_stats(x->c, stats);
  });
}

int pg_build_device(pg_ctx* x, const uint8_t* dev, uint64_t n, int rc0, uint64_t* n_rdbg, pg_stats* stats) {
  return guard([&] {
    if (!x || (!dev && n)) throw pg::Error(PG_EINVAL, "pg_build_device: bad arguments");
    pg::Ctx& c = x->c;
    PG_HIP(hipSetDevice(c.device));
    if (reinterpret_cast<uintptr_t>(dev) % 16 != 0) {
      c.fasta_own.reserve(n + 64);
      PG_HIP(hipMemcpyAsync(c.fasta_own.p, dev, n, hipMemcpyDeviceToDevice, c.stream));
      c.d_fasta = c.fasta_own.as<uint8_t>();
    } else {
      c.d_fasta = dev;
    }
    c.n_bytes = n;
    c.parsed = c.built = c.reduced = false;
    pg::parse_fasta(c);
    pg::build_dbg(c, nullptr, 0, rc0 != 0);
    pg::build_rdbg(c);
    // K1 on the stream (HIP events; the emission overlaps the host); an empty
    // input returns from parse_fasta before its events are recorded
    c.ms_parse = n ? c.t0.ms() : 0.0;
    if (n_rdbg) *n_rdbg = c.n_rdbg;
    fill_stats(c, stats);
  });
}

int pg_build_host(pg_ctx* x, const uint8_t* host, uint64_t n, int rc0, uint64_t* n_rdbg, pg_stats* stats) {
  return guard([&] {
    if (!x || (!host && n)) throw pg::Error(PG_EINVAL, "pg_build_host: bad arguments");
    pg::Ctx& c = x->c;
    PG_HIP(hipSetDevice(c.device));
    auto t0 = std::chrono::steady_clock::now();
    c.fasta_own.reserve(n + 64);
    c.d_fasta = c.fasta_own.as<uint8_t>();
    c.n_bytes = n;
    c.parsed = c.built = c.reduced = false;
    pg::build_host(c, host, n, rc0 != 0);
    c.ms_parse = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (n_rdbg) *n_rdbg = c.n_rdbg;
    fill_stats(c, stats);
  });
}

int pg_tune(pg_ctx* x, int what, int64_t value) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_tune: ctx is NULL");
    switch (what) {
      case PG_TUNE_K3_CHUNKS:
        if (value < 0 || value > 6) throw pg::Error(PG_EINVAL, "pg_tune: K3 chunks must be in [0, 6]");
        x->c.k3_chunks = (int)value;
        break;
      case PG_TUNE_K3_COVER:
#ifdef PG_COVER_LEGACY
        if (value < 0 || value > 2) throw pg::Error(PG_EINVAL, "pg_tune: K3 cover form must be 0, 1 or 2");
#else
        if (value != 0)
          throw pg::Error(PG_EINVAL, "pg_tune: K3 cover form must be 0 (the class-byte forms 1 and 2 are built only "
                                     "with PG_COVER_LEGACY)");
#endif
        x->c.k3_cover = (int)value;
        break;
      case PG_TUNE_K3_WBLK:
        if (value < 0 || value > 255) throw pg::Error(PG_EINVAL, "pg_tune: K3 work blocks must be in [0, 255]");
        x->c.k3_wblk = (int)value;
        break;
      case PG_TUNE_TIMERS:
        if (value < 0 || value > 7) throw pg::Error(PG_EINVAL, "pg_tune: timers must be in [0, 7]");
        x->c.t0.off = !(value & 1);
        x->c.t1.off = !(value & 2);
        x->c.t6.off = !(value & 4);
        break;
      case PG_TUNE_K3_ANCHORS:
        if (value != 0 && (value < 3 || value > 6) && value != 8)
          throw pg::Error(PG_EINVAL, "pg_tune: K3 anchors must be 3, 4, 5, 6 or 8 (0 = the default)");
        x->c.k3_anchors = (int)value;
        break;
      case PG_TUNE_K1:
        if (value < 0 || value > 7) throw pg::Error(PG_EINVAL, "pg_tune: K1 form must be in [0, 7]");
        x->c.k1_form = (int)value;
        break;
      case PG_TUNE_K3_EMIT:
        if (value < 0 || value > 1) throw pg::Error(PG_EINVAL, "pg_tune: K3 emit form must be 0 or 1");
        x->c.k3_emit = (int)value;
        break;
      case PG_TUNE_K3_TAIL:
        if (value < 0 || value > 64) throw pg::Error(PG_EINVAL, "pg_tune: K3 tail must be in [0, 64]");
        x->c.k3_tail = (int)value;
        break;
      case PG_TUNE_K3_HEAD:
        if (value < 0 || value > 64) throw pg::Error(PG_EINVAL, "pg_tune: K3 head must be in [0, 64]");
        x->c.k3_head = (int)value;
        break;
      case PG_TUNE_H2D_TAIL:
        if (value < 0) throw pg::Error(PG_EINVAL, "pg_tune: H2D tail must be >= 0");
        x->c.h2d_tail = (uint64_t)value;
        break;
      case PG_TUNE_EARLY_SPLIT:
        if (value < 0 || value > 1) throw pg::Error(PG_EINVAL, "pg_tune: early split must be 0 or 1");
        x->c.early_split = (int)value;
        break;
      case PG_TUNE_BUCKET_SHIFT:
        if (value < 0 || value > 8) throw pg::Error(PG_EINVAL, "pg_tune: bucket shift must be in [0, 8]");
        x->c.bb_shift = (int)value;
        break;
      case PG_TUNE_REGION_CAP:
        if (value < 0) throw pg::Error(PG_EINVAL, "pg_tune: region size must be >= 0");
        x->c.region_cap_force = (uint64_t)value;
        break;
      case PG_TUNE_H2D_CHUNK:
        if (value < 0) throw pg::Error(PG_EINVAL, "pg_tune: H2D chunk must be >= 0");
        x->c.h2d_chunk = value ? (uint64_t)value : (64ull << 20);
        break;
      case PG_TUNE_HOST_THREADS:
        if (value < 0 || value > 64) throw pg::Error(PG_EINVAL, "pg_tune: host threads must be in [0, 64]");
        x->c.host_threads = (int)value;
        break;
      case PG_TUNE_STAGE_PIECE:
        if (value < 0 || (value && value < 4096)) throw pg::Error(PG_EINVAL, "pg_tune: staging piece must be 0 or >= 4096");
        x->c.stage_piece = value ? (uint64_t)value : (32ull << 20);
        break;
      case PG_TUNE_HOST_REGISTER:
        if (value < 0 || value > 1) throw pg::Error(PG_EINVAL, "pg_tune: host register must be 0 or 1");
        x->c.host_register = (int)value;
        break;
      case PG_TUNE_DEVICE_CAP:
        if (value < 0) throw pg::Error(PG_EINVAL, "pg_tune: device cap must be >= 0");
        pg::DevBytes::cap().store((uint64_t)value);
        pg::DevBytes::peak().store(pg::DevBytes::cur().load());
        break;
      case PG_TUNE_POISON:
        if (value < -1 || value > 255) throw pg::Error(PG_EINVAL, "pg_tune: poison byte must be in [-1, 255]");
        pg::DevBytes::poison().store((int)value);
        break;
      case PG_TUNE_FREQ_FORM:
        if (value < 0 || value > 1) throw pg::Error(PG_EINVAL, "pg_tune: frequency pass form must be 0 or 1");
        x->c.freq_form = (int)value;
        break;
      case PG_TUNE_CMP_CHUNK:
        if (value < 0 || value > (1 << 25)) throw pg::Error(PG_EINVAL, "pg_tune: comparison chunk must be in [0, 2^25]");
        x->c.cmp_chunk = (uint64_t)value;
        break;
      case PG_TUNE_CMP_FORM:
        if (value < 0 || value > 1) throw pg::Error(PG_EINVAL, "pg_tune: curve pass form must be 0 or 1");
        x->c.cmp_form = (int)value;
        break;
      case PG_TUNE_RDBG_KEYS:
        if (value < 0 || value > 1) throw pg::Error(PG_EINVAL, "pg_tune: rdBG keys form must be 0 or 1");
        x->c.rdbg_keys = (int)value;
        break;
      case PG_TUNE_BUBBLE_HASH_BITS:
        if (value < 0 || value > 32) throw pg::Error(PG_EINVAL, "pg_tune: bubble hash bits must be in [0, 32]");
        x->c.bb_hash_bits = (int)value;
        break;
      case PG_TUNE_ALIGN_CELLS:
        if (value < 0 || value > (1ll << 30))
          throw pg::Error(PG_EINVAL, "pg_tune: alignment cells cap must be in [0, 2^30]");
        x->c.al_cells_cap = (uint64_t)value;
        break;
      case PG_TUNE_ALIGN_SCRATCH:
        if (value < 0) throw pg::Error(PG_EINVAL, "pg_tune: alignment scratch bytes must be >= 0");
        x->c.al_scratch = (uint64_t)value;
        break;
      case PG_TUNE_ALIGN_HASH_BITS:
        if (value < 0 || value > 64) throw pg::Error(PG_EINVAL, "pg_tune: alignment hash bits must be in [0, 64]");
        x->c.al_hash_bits = (int)value;
        break;
      case PG_TUNE_ALIGN_BAND:
        if (value < 0 || value > 1) throw pg::Error(PG_EINVAL, "pg_tune: alignment band must be 0 or 1");
        x->c.al_band = (int)value;
        break;
      case PG_TUNE_ALIGN_BAND_CELLS:
        if (value < 0 || value > (1ll << 34))
          throw pg::Error(PG_EINVAL, "pg_tune: alignment band cells cap must be in [0, 2^34]");
        x->c.al_band_cap = (uint64_t)value;
        break;
      case PG_TUNE_ALIGN_BAND_T0:
        if (value < 0 || value > (1ll << 20))
          throw pg::Error(PG_EINVAL, "pg_tune: alignment band first threshold must be in [0, 2^20]");
        x->c.al_band_t0 = (uint64_t)value;
        break;
      case PG_TUNE_STAGE_SLOTS:
        if (value < 0 || value == 1 || value > 8) throw pg::Error(PG_EINVAL, "pg_tune: staging slots must be 0 or 2..8");
        x->c.stage_slots = value ? (uint64_t)value : 4;
        break;
      case PG_TUNE_NJ_BLOCKS:
        if (value < 0 || value > 4096) throw pg::Error(PG_EINVAL, "pg_tune: arg-min blocks must be in [0, 4096]");
        x->c.nj_blocks = (int)value;
        break;
      case PG_TUNE_BOOT_SCRATCH:
        if (value < 0) throw pg::Error(PG_EINVAL, "pg_tune: bootstrap scratch bytes must be >= 0");
        x->c.bt_scratch = (uint64_t)value;
        break;
      case PG_TUNE_BOOT_FORM:
        if (value < 0 || value > 3) throw pg::Error(PG_EINVAL, "pg_tune: bootstrap form must be 0, 1, 2 or 3");
        x->c.bt_form_tune = (int)value;
        break;
      default:
        throw pg::Error(PG_EINVAL, "pg_tune: unknown parameter " + std::to_string(what));
    }
  });
}

uint64_t pg_device_bytes(int peak) {
  return peak ? pg::DevBytes::peak().load() : pg::DevBytes::cur().load();
}

int pg_get_stats(const pg_ctx* x, pg_stats* stats) {
  return guard([&] {
    if (!x || !stats) throw pg::Error(PG_EINVAL, "pg_get_stats: bad arguments");
    fill_stats(x->c, stats);
  });
}

int pg_dbg_export(pg_ctx* x, uint64_t* keys, uint16_t* masks, uint64_t cap, uint64_t* n) {
  return guard([&] {
    if (!x || !n) throw pg::Error(PG_EINVAL, "pg_dbg_export: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    const uint64_t total = pg::export_dbg(x->c, nullptr, nullptr, 0);
    *n = total;
    if (keys) {
      if (cap < total || !masks) throw pg::Error(PG_ERANGE, "pg_dbg_export: buffer too small");
      pg::export_dbg(x->c, keys, masks, cap);
    }
  });
}

int pg_rdbg_export(pg_ctx* x, uint64_t* keys, uint64_t cap, uint64_t* n) {
  return guard([&] {
    if (!x || !n) throw pg::Error(PG_EINVAL, "pg_rdbg_export: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n = pg::export_rdbg(x->c, nullptr, 0);
    if (keys) {
      if (cap < *n) throw pg::Error(PG_ERANGE, "pg_rdbg_export: buffer too small");
      pg::export_rdbg(x->c, keys, cap);
    }
  });
}

int pg_dbg_dump(pg_ctx* x, uint64_t* capacity, uint64_t* keys, uint16_t* values, uint8_t* counts, uint64_t* size) {
  return guard([&] {
    if (!x || !capacity || !size) throw pg::Error(PG_EINVAL, "pg_dbg_dump: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *size = pg::dbg_dump(x->c, *capacity, keys, values, counts);
  });
}

int pg_dbg_dump_fd(pg_ctx* x, uint64_t* capacity, int fd, const uint64_t* offsets, uint32_t* crcs, uint64_t* size) {
  return guard([&] {
    if (!x || !capacity || !size) throw pg::Error(PG_EINVAL, "pg_dbg_dump_fd: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *size = pg::dbg_dump_fd(x->c, *capacity, fd, offsets, crcs);
  });
}

int pg_dbg_load(pg_ctx* x, const uint64_t* keys, const uint16_t* masks, const uint8_t* counts, uint64_t n) {
  return guard([&] {
    if (!x || (n && !keys)) throw pg::Error(PG_EINVAL, "pg_dbg_load: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    pg::dbg_load(x->c, keys, masks, counts, n);
  });
}

uint64_t pg_oakht_capacity(uint64_t size) {
  try {
    return pg::oakht_capacity(size);
  } catch (...) {
    return 0;
  }
}

int pg_dbg_partition(pg_ctx* x, int nparts, void* d_out, uint64_t out_cap, uint64_t* counts) {
  return guard([&] {
    if (!x || !counts) throw pg::Error(PG_EINVAL, "pg_dbg_partition: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    // the scatter reuses the counts of a count pass over the same table
    const bool counted = x->c.part_gen == x->c.build_gen && x->c.part_nparts == nparts;
    const uint64_t total = d_out && counted ? x->c.part_total : pg::partition_dbg(x->c, nparts, nullptr, 0, counts);
    if (d_out) {
      if (out_cap < total) throw pg::Error(PG_ERANGE, "pg_dbg_partition: output too small");
      pg::partition_dbg(x->c, nparts, d_out, out_cap, counts);
    }
  });
}

int pg_dbg_merge(pg_ctx* x, const void* d_records, uint64_t n, uint64_t cap_hint, int sentinel) {
  return guard([&] {
    if (!x || (!d_records && n)) throw pg::Error(PG_EINVAL, "pg_dbg_merge: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    x->c.merge_sum = x->c.merge_rows = 0;
    pg::merge_dbg(x->c, d_records, n, cap_hint, sentinel);
  });
}

int pg_dbg_partition_sums(pg_ctx* x, int nparts, uint64_t* sums) {
  return guard([&] {
    if (!x || !sums || nparts < 1 || nparts > 64) throw pg::Error(PG_EINVAL, "pg_dbg_partition_sums: bad arguments");
    if (x->c.part_nparts != nparts) throw pg::Error(PG_EINVAL, "pg_dbg_partition_sums: no scatter into that many parts");
    for (int i = 0; i < nparts; ++i) sums[i] = x->c.part_sums[i];
  });
}

int pg_rows_checksum(pg_ctx* x, const void* d_rows, const uint64_t* seg_off, uint64_t nseg, uint64_t* sums) {
  return guard([&] {
    if (!x || !seg_off || (nseg && !sums) || (!d_rows && nseg && seg_off[nseg] > seg_off[0]))
      throw pg::Error(PG_EINVAL, "pg_rows_checksum: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    pg::rows_checksum(x->c, d_rows, seg_off, nseg, sums);
  });
}

int pg_route_rows_checksum(pg_ctx* x, const void* d_rows, const uint64_t* seg_off, uint64_t nseg, uint64_t* sums) {
  return guard([&] {
    if (!x || !seg_off || (nseg && !sums) || (!d_rows && nseg && seg_off[nseg] > seg_off[0]))
      throw pg::Error(PG_EINVAL, "pg_route_rows_checksum: bad arguments");
    if (reinterpret_cast<uintptr_t>(d_rows) & 3u) throw pg::Error(PG_EINVAL, "pg_route_rows_checksum: rows not 4-byte aligned");
    PG_HIP(hipSetDevice(x->c.device));
    pg::rows_checksum(x->c, d_rows, seg_off, nseg, sums, true);
  });
}

static int route_lg(int nparts, const char* what) {
  if (nparts < 1 || nparts > 64 || (nparts & (nparts - 1)))
    throw pg::Error(PG_EINVAL, std::string(what) + ": nparts must be a power of two in [1, 64]");
  return __builtin_ctz((unsigned)nparts);
}
// At most one owner per coarse bin: 2^min(6, kb) of them (8 at k = 1, 32 at
// k = 2).  From k, not from Ctx.cbits, which only a build sets: on a fresh
// context that is still 0, and more owners would rotate h by more than its kb
// bits (TableView::rotk).
static void route_bins(const pg_ctx* x, int lg, const char* what) {
  if (lg > std::min(6, pg::key_bits(x->c.k))) throw pg::Error(PG_EINVAL, std::string(what) + ": more owners than coarse bins");
}

int pg_route_stage_a(pg_ctx* x, const uint8_t* rec_flags, int extra_empty, int rc0, int nparts, uint64_t* counts,
                     int* sentinel) {
  return guard([&] {
    if (!x || !counts) throw pg::Error(PG_EINVAL, "pg_route_stage_a: bad arguments");
    const int lg = route_lg(nparts, "pg_route_stage_a");
    route_bins(x, lg, "pg_route_stage_a");                   // before the build: nothing runs for a refused count
    PG_HIP(hipSetDevice(x->c.device));
    x->c.route_req = true;
    try {
      pg::build_dbg(x->c, rec_flags, extra_empty, rc0 != 0);
    } catch (...) {
      x->c.route_req = false;
      throw;
    }
    if (!x->c.route_ready) throw pg::Error(PG_EINVAL, "pg_route_stage_a: the build did not hold its records");
    pg::route_counts(x->c, lg, counts);
    if (sentinel) *sentinel = x->c.route_sentinel ? 1 : 0;
  });
}

int pg_route_scatter(pg_ctx* x, int nparts, void* d_out, uint64_t out_cap, uint64_t* sums) {
  return guard([&] {
    if (!x || !sums || (!d_out && out_cap)) throw pg::Error(PG_EINVAL, "pg_route_scatter: bad arguments");
    const int lg = route_lg(nparts, "pg_route_scatter");
    route_bins(x, lg, "pg_route_scatter");
    PG_HIP(hipSetDevice(x->c.device));
    pg::route_scatter(x->c, lg, d_out, out_cap, sums);
  });
}

int pg_route_finish(pg_ctx* x, uint64_t* n_rdbg, pg_stats* stats) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_route_finish: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::route_finish(x->c);
    if (n_rdbg) *n_rdbg = x->c.n_rdbg;
    fill_stats(x->c, stats);
  });
}

int pg_route_merge(pg_ctx* x, const void* d_rows, uint64_t n, int nparts, int sentinel, uint64_t* n_rdbg,
                   pg_stats* stats) {
  return guard([&] {
    if (!x || (!d_rows && n)) throw pg::Error(PG_EINVAL, "pg_route_merge: bad arguments");
    const int lg = route_lg(nparts, "pg_route_merge");
    route_bins(x, lg, "pg_route_merge");
    PG_HIP(hipSetDevice(x->c.device));
    x->c.merge_sum = x->c.merge_rows = 0;
    pg::merge_dbg(x->c, d_rows, n, 0, sentinel, lg);
    if (n_rdbg) *n_rdbg = x->c.n_rdbg;
    fill_stats(x->c, stats);
  });
}

int pg_route_merge_segs(pg_ctx* x, const void* const* d_segs, const uint64_t* n, int nseg, int nparts, int sentinel,
                       uint64_t* n_rdbg, pg_stats* stats) {
  return guard([&] {
    if (!x || nseg < 0 || (nseg && (!d_segs || !n))) throw pg::Error(PG_EINVAL, "pg_route_merge_segs: bad arguments");
    for (int s = 0; s < nseg; ++s)
      if (n[s] && !d_segs[s]) throw pg::Error(PG_EINVAL, "pg_route_merge_segs: a non-empty segment has no rows");
    const int lg = route_lg(nparts, "pg_route_merge_segs");
    route_bins(x, lg, "pg_route_merge_segs");
    PG_HIP(hipSetDevice(x->c.device));
    x->c.merge_sum = x->c.merge_rows = 0;
    pg::merge_dbg_segs(x->c, d_segs, n, nseg, sentinel, lg);
    if (n_rdbg) *n_rdbg = x->c.n_rdbg;
    fill_stats(x->c, stats);
  });
}

int pg_dbg_merge_check(const pg_ctx* x, uint64_t* rows, uint64_t* sum) {
  return guard([&] {
    if (!x || !rows || !sum) throw pg::Error(PG_EINVAL, "pg_dbg_merge_check: bad arguments");
    *rows = x->c.merge_rows;
    *sum = x->c.merge_sum;
  });
}

int pg_edges(pg_ctx* x, const uint8_t* rec_flags, int rc1, uint64_t* n_edges) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_edges: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    const uint64_t n = pg::walk_edges(x->c, rec_flags, rc1 != 0);
    if (n_edges) *n_edges = n;
  });
}

int pg_edges_export(pg_ctx* x, uint64_t* tuples, int64_t* counts, int64_t* first_walk, uint64_t cap) {
  return guard([&] {
    if (!x || !tuples || !counts || !first_walk) throw pg::Error(PG_EINVAL, "pg_edges_export: bad arguments");
    if (cap < x->c.n_edges) throw pg::Error(PG_ERANGE, "pg_edges_export: buffer too small");
    PG_HIP(hipSetDevice(x->c.device));
    pg::export_edges(x->c, tuples, counts, first_walk, cap);
  });
}

int pg_set_labels(pg_ctx* x, const int64_t* key, const int64_t* value, const int64_t* label, uint64_t n) {
  return guard([&] {
    if (!x || (n && (!key || !value || !label))) throw pg::Error(PG_EINVAL, "pg_set_labels: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    pg::set_labels(x->c, key, value, label, n);
  });
}

int pg_rows(pg_ctx* x, const uint8_t* rec_flags, int rc1, uint64_t* n_rows) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_rows: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    const uint64_t n = pg::walk_rows(x->c, rec_flags, rc1 != 0);
    if (n_rows) *n_rows = n;
  });
}

int pg_rows_export(pg_ctx* x, int64_t* rows5, uint64_t cap) {
  return guard([&] {
    if (!x || !rows5) throw pg::Error(PG_EINVAL, "pg_rows_export: bad arguments");
    if (cap < x->c.n_rows) throw pg::Error(PG_ERANGE, "pg_rows_export: buffer too small");
    PG_HIP(hipSetDevice(x->c.device));
    pg::export_rows(x->c, rows5, cap);
  });
}

int pg_edges_format(pg_ctx* x, char* out, uint64_t cap, uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes) throw pg::Error(PG_EINVAL, "pg_edges_format: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_edges(x->c, out, cap);
  });
}

int pg_edges_format_fd(pg_ctx* x, int fd, uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes || fd < 0) throw pg::Error(PG_EINVAL, "pg_edges_format_fd: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_edges(x->c, nullptr, 0, fd);
  });
}

int pg_labels_from_edges(pg_ctx* x, const uint64_t* tuples, uint64_t n_edges, const int64_t* mcl_key,
                         const int64_t* mcl_value, const int64_t* mcl_label, uint64_t n_mcl, int64_t next_label,
                         uint64_t* n_labels) {
  return guard([&] {
    if (!x || (n_mcl && (!mcl_key || !mcl_value || !mcl_label)) || (tuples == nullptr && n_edges))
      throw pg::Error(PG_EINVAL, "pg_labels_from_edges: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    const uint64_t n = pg::labels_from_edges(x->c, tuples, n_edges, mcl_key, mcl_value, mcl_label, n_mcl, next_label);
    if (n_labels) *n_labels = n;
  });
}

int pg_labels_export(pg_ctx* x, int64_t* key, int64_t* value, int64_t* label, uint64_t cap) {
  return guard([&] {
    if (!x || !key || !value || !label) throw pg::Error(PG_EINVAL, "pg_labels_export: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    pg::export_labels(x->c, key, value, label, cap);
  });
}

int pg_cluster_cc(pg_ctx* x, const uint64_t* tuples, const int64_t* counts, uint64_t n_edges, int64_t min_weight,
                  uint64_t* n_clusters, uint64_t* n_nodes) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_cluster_cc: ctx is NULL");
    if (min_weight < 1) throw pg::Error(PG_EINVAL, "pg_cluster_cc: min_weight below 1");
    if (tuples && !counts) throw pg::Error(PG_EINVAL, "pg_cluster_cc: tuples without counts");
    if (!tuples && counts) throw pg::Error(PG_EINVAL, "pg_cluster_cc: counts without tuples");
    PG_HIP(hipSetDevice(x->c.device));
    pg::cluster_cc(x->c, tuples, counts, n_edges, min_weight);
    if (n_clusters) *n_clusters = x->c.n_clusters;
    if (n_nodes) *n_nodes = x->c.n_clu_nodes;
  });
}

int pg_cluster_markov(pg_ctx* x, const uint64_t* tuples, const int64_t* counts, uint64_t n_edges, int64_t min_weight,
                      uint32_t inflation2, uint32_t select, uint32_t max_iter, uint64_t* n_clusters, uint64_t* n_nodes,
                      uint32_t* n_iter, uint64_t* chaos) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_cluster_markov: ctx is NULL");
    if (min_weight < 1) throw pg::Error(PG_EINVAL, "pg_cluster_markov: min_weight below 1");
    if (tuples && !counts) throw pg::Error(PG_EINVAL, "pg_cluster_markov: tuples without counts");
    if (!tuples && counts) throw pg::Error(PG_EINVAL, "pg_cluster_markov: counts without tuples");
    if (inflation2 < 3 || inflation2 > 40) throw pg::Error(PG_EINVAL, "pg_cluster_markov: inflation2 outside [3, 40]");
    if (select < 1 || select > 64) throw pg::Error(PG_EINVAL, "pg_cluster_markov: select outside [1, 64]");
    if (max_iter > 10000) throw pg::Error(PG_EINVAL, "pg_cluster_markov: max_iter above 10000");
    PG_HIP(hipSetDevice(x->c.device));
    pg::cluster_markov(x->c, tuples, counts, n_edges, min_weight, inflation2, select, max_iter, n_iter, chaos);
    if (n_clusters) *n_clusters = x->c.n_clusters;
    if (n_nodes) *n_nodes = x->c.n_clu_nodes;
  });
}

int pg_cluster_markov_matrix(pg_ctx* x, uint32_t* col_len, uint32_t* rows, uint32_t* vals, uint64_t cap_nodes,
                             uint32_t* select) {
  return guard([&] {
    if (!x || !col_len || !rows || !vals) throw pg::Error(PG_EINVAL, "pg_cluster_markov_matrix: bad arguments");
    if (!x->c.mk_ready) throw pg::Error(PG_EINVAL, "pg_cluster_markov_matrix: no matrix (call pg_cluster_markov first)");
    if (cap_nodes < x->c.mk_nodes) throw pg::Error(PG_ERANGE, "pg_cluster_markov_matrix: buffers too small");
    PG_HIP(hipSetDevice(x->c.device));
    pg::markov_matrix(x->c, col_len, rows, vals);
    if (select) *select = x->c.mk_select;
  });
}

int pg_cluster_markov_stats(pg_ctx* x, uint64_t* n_nodes, uint32_t* select, uint64_t* cols_wave, uint64_t* cols_mid,
                            uint64_t* cols_block) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_cluster_markov_stats: ctx is NULL");
    if (!x->c.mk_ready) throw pg::Error(PG_EINVAL, "pg_cluster_markov_stats: no matrix (call pg_cluster_markov first)");
    if (n_nodes) *n_nodes = x->c.mk_nodes;
    if (select) *select = x->c.mk_select;
    if (cols_wave) *cols_wave = x->c.mk_cols_wave;
    if (cols_mid) *cols_mid = x->c.mk_cols_mid;
    if (cols_block) *cols_block = x->c.mk_cols_block;
  });
}

int pg_cluster_sweep(pg_ctx* x, const uint64_t* tuples, const int64_t* counts, uint64_t n_edges,
                     const int64_t* thresholds, uint64_t n_thr, uint64_t* n_nodes, int64_t* max_weight,
                     uint64_t* edges, uint64_t* clusters, uint64_t* largest, uint64_t* singletons) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_cluster_sweep: ctx is NULL");
    if (tuples && !counts) throw pg::Error(PG_EINVAL, "pg_cluster_sweep: tuples without counts");
    if (!tuples && !x->c.edges_ready) throw pg::Error(PG_EINVAL, "pg_cluster_sweep: no edges (call pg_edges first)");
    if (n_thr > SW_MAX_LEVELS) throw pg::Error(PG_EINVAL, "pg_cluster_sweep: more than 4096 thresholds");
    if (n_thr && !thresholds) throw pg::Error(PG_EINVAL, "pg_cluster_sweep: thresholds is NULL");
    for (uint64_t i = 0; i < n_thr; ++i)
      if (thresholds[i] < 1 || (i && thresholds[i] <= thresholds[i - 1]))
        throw pg::Error(PG_EINVAL, "pg_cluster_sweep: thresholds must be at least 1 and strictly ascending");
    PG_HIP(hipSetDevice(x->c.device));
    pg::cluster_sweep(x->c, tuples, counts, n_edges, thresholds, n_thr, n_nodes, max_weight, edges, clusters, largest,
                      singletons);
  });
}

int pg_clusters_format(pg_ctx* x, char* out, uint64_t cap, uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes) throw pg::Error(PG_EINVAL, "pg_clusters_format: bad arguments");
    if (!x->c.clu_ready) throw pg::Error(PG_EINVAL, "pg_clusters_format: no clustering (call pg_cluster_cc or pg_cluster_markov first)");
    if (out && cap < x->c.clu_total) throw pg::Error(PG_ERANGE, "pg_clusters_format: buffer too small");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_clusters(x->c, out, cap);
  });
}

int pg_clusters_format_fd(pg_ctx* x, int fd, uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes || fd < 0) throw pg::Error(PG_EINVAL, "pg_clusters_format_fd: bad arguments");
    if (!x->c.clu_ready) throw pg::Error(PG_EINVAL, "pg_clusters_format_fd: no clustering (call pg_cluster_cc or pg_cluster_markov first)");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_clusters(x->c, nullptr, 0, fd);
  });
}

int pg_freq(pg_ctx* x, const int64_t* rows5, uint64_t n_rows, const int32_t* rec_group, uint64_t n_records,
            uint32_t n_groups, uint64_t* n_labels, uint64_t* n_used, uint64_t* n_skipped) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_freq: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::freq(x->c, rows5, n_rows, rec_group, n_records, n_groups, n_labels, n_used, n_skipped);
  });
}

int pg_freq_export(pg_ctx* x, int64_t* label, uint32_t* n_genomes, uint64_t* n_rows, uint64_t* n_plus,
                   uint64_t* total_bp, uint64_t* min_len, uint64_t* max_len, uint64_t* bits, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_freq_export: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::freq_export(x->c, label, n_genomes, n_rows, n_plus, total_bp, min_len, max_len, bits, cap);
  });
}

int pg_freq_spectrum(pg_ctx* x, uint64_t* labels_by_g, uint64_t* bp_by_g, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_freq_spectrum: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::freq_spectrum(x->c, labels_by_g, bp_by_g, cap);
  });
}

int pg_freq_groups(pg_ctx* x, uint64_t* rows, uint64_t* bp_total, uint64_t* bp_core, uint64_t* bp_shell,
                   uint64_t* bp_unique, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_freq_groups: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::freq_groups(x->c, rows, bp_total, bp_core, bp_shell, bp_unique, cap);
  });
}

int pg_freq_format(pg_ctx* x, char* out, uint64_t cap, uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes) throw pg::Error(PG_EINVAL, "pg_freq_format: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_freq(x->c, out, cap);
  });
}

int pg_freq_format_fd(pg_ctx* x, int fd, uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes || fd < 0) throw pg::Error(PG_EINVAL, "pg_freq_format_fd: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_freq(x->c, nullptr, 0, fd);
  });
}

int pg_freq_compare(pg_ctx* x, const uint64_t* bits, uint64_t n_labels, uint32_t n_groups, const int32_t* orders,
                    uint32_t n_orders) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_freq_compare: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::freq_compare(x->c, bits, n_labels, n_groups, orders, n_orders);
  });
}

int pg_freq_shared(pg_ctx* x, uint64_t* shared, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_freq_shared: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::freq_shared(x->c, shared, cap);
  });
}

int pg_freq_curve(pg_ctx* x, uint64_t* pan, uint64_t* core, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_freq_curve: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::freq_curve(x->c, pan, core, cap);
  });
}

int pg_kmer_colors(pg_ctx* x, const int32_t* rec_group, const uint8_t* rec_flags, uint64_t n_records, uint32_t n_groups,
                   int rc0, uint64_t* n_keys, uint64_t* n_windows, uint64_t* n_missing, uint64_t* n_uncoloured) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_kmer_colors: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::kmer_colors(x->c, rec_group, rec_flags, n_records, n_groups, rc0, n_keys, n_windows, n_missing, n_uncoloured);
  });
}

int pg_kmer_colors_export(pg_ctx* x, uint64_t* keys, uint64_t* bits, uint64_t cap, uint64_t* n) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_kmer_colors_export: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::kmer_colors_export(x->c, keys, bits, cap, n);
  });
}

int pg_kmer_colors_spectrum(pg_ctx* x, uint64_t* kmers_by_g, uint64_t* g_kmers, uint64_t* g_core, uint64_t* g_shell,
                            uint64_t* g_unique) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_kmer_colors_spectrum: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::kmer_colors_spectrum(x->c, kmers_by_g, g_kmers, g_core, g_shell, g_unique);
  });
}

int pg_kmer_compare(pg_ctx* x, const int32_t* orders, uint32_t n_orders) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_kmer_compare: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::kmer_compare(x->c, orders, n_orders);
  });
}

int pg_kmer_compare_export(pg_ctx* x, uint64_t* shared, uint64_t shared_cap, uint64_t* pan, uint64_t* core,
                           uint64_t curve_cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_kmer_compare_export: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::kmer_compare_export(x->c, shared, shared_cap, pan, core, curve_cap);
  });
}

int pg_kmer_colors_time(pg_ctx* x, double* ms_index, double* ms_colour, double* ms_compare, uint64_t* n_windows) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_kmer_colors_time: ctx is NULL");
    pg::kmer_colors_time(x->c, ms_index, ms_colour, ms_compare, n_windows);
  });
}

int pg_kmer_colors_drop(pg_ctx* x) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_kmer_colors_drop: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::kmer_colors_drop(x->c);
  });
}

int pg_tree_nj(pg_ctx* x, const uint64_t* dist, uint32_t n, uint64_t* n_joins) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_tree_nj: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::tree_nj(x->c, dist, n, n_joins);
  });
}

int pg_tree_dist(pg_ctx* x, uint64_t* dist, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_tree_dist: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::tree_dist(x->c, dist, cap);
  });
}

int pg_tree_joins(pg_ctx* x, uint32_t* left, uint32_t* right, uint64_t* left_len, uint64_t* right_len, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_tree_joins: ctx is NULL");
    pg::tree_joins(x->c, left, right, left_len, right_len, cap);
  });
}

int pg_tree_root(pg_ctx* x, uint32_t* n_children, uint32_t child[3], uint64_t len[3]) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_tree_root: ctx is NULL");
    pg::tree_root(x->c, n_children, child, len);
  });
}

int pg_tree_time(pg_ctx* x, double* ms, uint64_t* cells) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_tree_time: ctx is NULL");
    pg::tree_time(x->c, ms, cells);
  });
}

int pg_tree_bootstrap(pg_ctx* x, const uint64_t* bits, uint64_t n_labels, uint32_t n_groups, uint32_t n_reps,
                      uint64_t seed, uint64_t* rep_dist, uint64_t rep_dist_cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_tree_bootstrap: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::tree_bootstrap(x->c, bits, n_labels, n_groups, n_reps, seed, rep_dist, rep_dist_cap);
  });
}

int pg_tree_support(pg_ctx* x, uint32_t* support, uint64_t cap, uint32_t* n_reps) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_tree_support: ctx is NULL");
    pg::tree_support(x->c, support, cap, n_reps);
  });
}

int pg_tree_bootstrap_joins(pg_ctx* x, uint32_t* left, uint32_t* right, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_tree_bootstrap_joins: ctx is NULL");
    pg::tree_bootstrap_joins(x->c, left, right, cap);
  });
}

int pg_tree_bootstrap_time(pg_ctx* x, double* ms_dist, double* ms_nj, double* ms_support, uint64_t* cells) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_tree_bootstrap_time: ctx is NULL");
    pg::tree_bootstrap_time(x->c, ms_dist, ms_nj, ms_support, cells);
  });
}

int pg_tree_bootstrap_form(pg_ctx* x, uint32_t* form, uint32_t* n_batches) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_tree_bootstrap_form: ctx is NULL");
    pg::tree_bootstrap_form(x->c, form, n_batches);
  });
}

int pg_region_graph(pg_ctx* x, const int64_t* rows5, uint64_t n_rows, const int32_t* rec_group, uint64_t n_records,
                    uint32_t n_groups, uint64_t* n_nodes, uint64_t* n_links, uint64_t* n_paths,
                    uint64_t* n_skipped) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_graph: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_graph(x->c, rows5, n_rows, rec_group, n_records, n_groups, n_nodes, n_links, n_paths, n_skipped);
  });
}

int pg_region_nodes(pg_ctx* x, int64_t* label, uint64_t* n_rows, uint64_t* max_len, uint32_t* n_out, uint32_t* n_in,
                    uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_nodes: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_nodes(x->c, label, n_rows, max_len, n_out, n_in, cap);
  });
}

int pg_region_links(pg_ctx* x, int64_t* from, int64_t* to, uint64_t* count, uint32_t* n_genomes, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_links: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_links(x->c, from, to, count, n_genomes, cap);
  });
}

int pg_region_paths(pg_ctx* x, int64_t* record, int64_t* strand, int64_t* lo, int64_t* hi, uint64_t* n_steps,
                    uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_paths: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_paths(x->c, record, strand, lo, hi, n_steps, cap);
  });
}

int pg_region_links_format(pg_ctx* x, char* out, uint64_t cap, uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes) throw pg::Error(PG_EINVAL, "pg_region_links_format: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_region_links(x->c, out, cap);
  });
}

int pg_region_links_format_fd(pg_ctx* x, int fd, uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes || fd < 0) throw pg::Error(PG_EINVAL, "pg_region_links_format_fd: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_region_links(x->c, nullptr, 0, fd);
  });
}

int pg_region_gfa(pg_ctx* x, const char* names, const int64_t* name_off, uint64_t n_names, char* out, uint64_t cap,
                  uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes) throw pg::Error(PG_EINVAL, "pg_region_gfa: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_region_gfa(x->c, names, name_off, n_names, out, cap);
  });
}

int pg_region_gfa_fd(pg_ctx* x, const char* names, const int64_t* name_off, uint64_t n_names, int fd,
                     uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes || fd < 0) throw pg::Error(PG_EINVAL, "pg_region_gfa_fd: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_region_gfa(x->c, names, name_off, n_names, nullptr, 0, fd);
  });
}

int pg_region_seqs(pg_ctx* x, const int64_t* rows5, uint64_t n_rows, const int32_t* rec_group, uint64_t n_records,
                   uint32_t n_groups, uint64_t* n_regions, uint64_t* n_bases, uint64_t* n_skipped) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_seqs: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_seqs(x->c, rows5, n_rows, rec_group, n_records, n_groups, n_regions, n_bases, n_skipped);
  });
}

int pg_region_seqs_table(pg_ctx* x, int64_t* label, int64_t* row, int64_t* record, int64_t* start, int64_t* end,
                         int64_t* strand, uint64_t* len, uint64_t* gc, uint64_t* amb, uint64_t* offset,
                         uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_seqs_table: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_seqs_table(x->c, label, row, record, start, end, strand, len, gc, amb, offset, cap);
  });
}

int pg_region_seqs_bases(pg_ctx* x, uint8_t* out, uint64_t cap, uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes) throw pg::Error(PG_EINVAL, "pg_region_seqs_bases: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::region_seqs_bases(x->c, out, cap);
  });
}

int pg_region_seqs_time(pg_ctx* x, double* ms_decode, uint64_t* n_chunks) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_seqs_time: ctx is NULL");
    if (!x->c.rs_ready) throw pg::Error(PG_EINVAL, "pg_region_seqs_time: no region sequences (call pg_region_seqs first)");
    if (ms_decode) *ms_decode = x->c.ms_rs_decode;
    if (n_chunks) *n_chunks = x->c.rs_chunks;
  });
}

int pg_region_fasta(pg_ctx* x, const char* names, const int64_t* name_off, uint64_t n_names, char* out, uint64_t cap,
                    uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes) throw pg::Error(PG_EINVAL, "pg_region_fasta: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_region_fasta(x->c, names, name_off, n_names, out, cap);
  });
}

int pg_region_fasta_fd(pg_ctx* x, const char* names, const int64_t* name_off, uint64_t n_names, int fd,
                       uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes || fd < 0) throw pg::Error(PG_EINVAL, "pg_region_fasta_fd: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_region_fasta(x->c, names, name_off, n_names, nullptr, 0, fd);
  });
}

int pg_region_gfa_seq(pg_ctx* x, const char* names, const int64_t* name_off, uint64_t n_names, char* out,
                      uint64_t cap, uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes) throw pg::Error(PG_EINVAL, "pg_region_gfa_seq: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_region_gfa(x->c, names, name_off, n_names, out, cap, -1, true);
  });
}

int pg_region_gfa_seq_fd(pg_ctx* x, const char* names, const int64_t* name_off, uint64_t n_names, int fd,
                         uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes || fd < 0) throw pg::Error(PG_EINVAL, "pg_region_gfa_seq_fd: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_region_gfa(x->c, names, name_off, n_names, nullptr, 0, fd, true);
  });
}

int pg_region_sites(pg_ctx* x, const int64_t* rows5, uint64_t n_rows, const int32_t* rec_group, uint64_t n_records,
                    uint32_t n_groups, uint64_t* n_sites, uint64_t* n_alleles, uint64_t* n_records_emitted,
                    uint64_t* n_skipped) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_sites: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_sites(x->c, rows5, n_rows, rec_group, n_records, n_groups, n_sites, n_alleles, n_records_emitted,
                     n_skipped);
  });
}

int pg_region_sites_table(pg_ctx* x, int64_t* from, int64_t* to, uint32_t* n_alleles, uint64_t* first,
                          uint64_t* count, uint32_t* n_genomes, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_sites_table: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_sites_table(x->c, from, to, n_alleles, first, count, n_genomes, cap);
  });
}

int pg_region_sites_alleles(pg_ctx* x, uint64_t* site, int64_t* via, uint64_t* count, uint32_t* n_genomes,
                            uint64_t* min_len, uint64_t* max_len, uint64_t* bits, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_sites_alleles: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_sites_alleles(x->c, site, via, count, n_genomes, min_len, max_len, bits, cap);
  });
}

int pg_region_sites_groups(pg_ctx* x, uint64_t* sites, uint64_t* alleles, uint64_t* private_alleles, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_sites_groups: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_sites_groups(x->c, sites, alleles, private_alleles, cap);
  });
}

int pg_region_sites_format(pg_ctx* x, char* out, uint64_t cap, uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes) throw pg::Error(PG_EINVAL, "pg_region_sites_format: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_region_sites(x->c, out, cap);
  });
}

int pg_region_sites_format_fd(pg_ctx* x, int fd, uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes || fd < 0) throw pg::Error(PG_EINVAL, "pg_region_sites_format_fd: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_region_sites(x->c, nullptr, 0, fd);
  });
}

int pg_region_bubbles(pg_ctx* x, const int64_t* rows5, uint64_t n_rows, const int32_t* rec_group, uint64_t n_records,
                      uint32_t n_groups, uint32_t min_genomes, uint64_t* n_anchors, uint64_t* n_segments,
                      uint64_t* n_sites, uint64_t* n_alleles, uint64_t* n_skipped) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_bubbles: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_bubbles(x->c, rows5, n_rows, rec_group, n_records, n_groups, min_genomes, n_anchors, n_segments,
                       n_sites, n_alleles, n_skipped);
  });
}

int pg_region_bubbles_table(pg_ctx* x, int64_t* from, int64_t* to, uint32_t* n_alleles, uint64_t* first,
                            uint64_t* count, uint32_t* n_genomes, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_bubbles_table: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_bubbles_table(x->c, from, to, n_alleles, first, count, n_genomes, cap);
  });
}

int pg_region_bubbles_alleles(pg_ctx* x, uint64_t* site, uint64_t* regions, uint64_t* first_row, uint64_t* count,
                              uint32_t* n_genomes, uint64_t* min_bp, uint64_t* max_bp, uint64_t* inner_off,
                              uint64_t* bits, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_bubbles_alleles: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_bubbles_alleles(x->c, site, regions, first_row, count, n_genomes, min_bp, max_bp, inner_off, bits, cap);
  });
}

int pg_region_bubbles_inner(pg_ctx* x, int64_t* inner, uint64_t cap, uint64_t* n_inner) {
  return guard([&] {
    if (!x || !n_inner) throw pg::Error(PG_EINVAL, "pg_region_bubbles_inner: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_inner = pg::region_bubbles_inner(x->c, inner, cap);
  });
}

int pg_region_bubbles_groups(pg_ctx* x, uint64_t* sites, uint64_t* alleles, uint64_t* private_alleles, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_bubbles_groups: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_bubbles_groups(x->c, sites, alleles, private_alleles, cap);
  });
}

int pg_region_bubbles_anchors(pg_ctx* x, int64_t* label, uint32_t* n_genomes, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_bubbles_anchors: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_bubbles_anchors(x->c, label, n_genomes, cap);
  });
}

int pg_region_bubbles_format(pg_ctx* x, char* out, uint64_t cap, uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes) throw pg::Error(PG_EINVAL, "pg_region_bubbles_format: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_region_bubbles(x->c, out, cap);
  });
}

int pg_region_bubbles_format_fd(pg_ctx* x, int fd, uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes || fd < 0) throw pg::Error(PG_EINVAL, "pg_region_bubbles_format_fd: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_region_bubbles(x->c, nullptr, 0, fd);
  });
}

int pg_region_variants(pg_ctx* x, const int64_t* rows5, uint64_t n_rows, const int32_t* rec_group, uint64_t n_records,
                       uint32_t n_groups, uint32_t ref_group, uint64_t* n_alleles, uint64_t* n_bases,
                       uint64_t* n_placed, uint64_t* n_unplaced) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_variants: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_variants(x->c, rows5, n_rows, rec_group, n_records, n_groups, ref_group, n_alleles, n_bases, n_placed,
                        n_unplaced);
  });
}

int pg_region_variants_alleles(pg_ctx* x, int64_t* record, int64_t* lo, int64_t* hi, int64_t* strand, uint64_t* len,
                               uint64_t* gc, uint64_t* amb, uint64_t* offset, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_variants_alleles: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_variants_alleles(x->c, record, lo, hi, strand, len, gc, amb, offset, cap);
  });
}

int pg_region_variants_bases(pg_ctx* x, uint8_t* out, uint64_t cap, uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes) throw pg::Error(PG_EINVAL, "pg_region_variants_bases: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::region_variants_bases(x->c, out, cap);
  });
}

int pg_region_variants_placed(pg_ctx* x, uint64_t* site, int64_t* record, int64_t* pos0, uint64_t* ref_row,
                              uint32_t* ref_allele, uint64_t* ref_len, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_variants_placed: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_variants_placed(x->c, site, record, pos0, ref_row, ref_allele, ref_len, cap);
  });
}

int pg_region_variants_time(pg_ctx* x, double* ms_decode, uint64_t* n_chunks) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_variants_time: ctx is NULL");
    if (!x->c.vr_ready) throw pg::Error(PG_EINVAL, std::string("pg_region_variants_time: ") + NEED_VARIANTS);
    if (ms_decode) *ms_decode = x->c.ms_vr_decode;
    if (n_chunks) *n_chunks = x->c.vr_chunks;
  });
}

int pg_region_alleles_fasta(pg_ctx* x, const char* names, const int64_t* name_off, uint64_t n_names, char* out,
                            uint64_t cap, uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes) throw pg::Error(PG_EINVAL, "pg_region_alleles_fasta: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_region_alleles_fasta(x->c, names, name_off, n_names, out, cap);
  });
}

int pg_region_alleles_fasta_fd(pg_ctx* x, const char* names, const int64_t* name_off, uint64_t n_names, int fd,
                               uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes || fd < 0) throw pg::Error(PG_EINVAL, "pg_region_alleles_fasta_fd: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_region_alleles_fasta(x->c, names, name_off, n_names, nullptr, 0, fd);
  });
}

int pg_region_vcf(pg_ctx* x, const char* names, const int64_t* name_off, uint64_t n_names, char* out, uint64_t cap,
                  uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes) throw pg::Error(PG_EINVAL, "pg_region_vcf: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_region_vcf(x->c, names, name_off, n_names, out, cap);
  });
}

int pg_region_vcf_fd(pg_ctx* x, const char* names, const int64_t* name_off, uint64_t n_names, int fd,
                     uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes || fd < 0) throw pg::Error(PG_EINVAL, "pg_region_vcf_fd: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_region_vcf(x->c, names, name_off, n_names, nullptr, 0, fd);
  });
}

int pg_region_align(pg_ctx* x, uint64_t* n_pairs, uint64_t* n_aligned, uint64_t* n_ops, uint64_t* n_prims,
                    uint64_t* n_lines) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_align: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_align(x->c, n_pairs, n_aligned, n_ops, n_prims, n_lines);
  });
}

int pg_region_align_pairs(pg_ctx* x, uint64_t* site, uint64_t* allele, uint64_t* placed, uint64_t* t_len,
                          uint64_t* q_len, uint64_t* prefix, uint64_t* suffix, uint64_t* status, uint64_t* distance,
                          uint64_t* n_eq, uint64_t* n_sub, uint64_t* n_ins, uint64_t* n_del, uint64_t* op_off,
                          uint64_t* n_ops, uint64_t* prim_off, uint64_t* n_prims, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_align_pairs: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    uint64_t* const cols[17] = {site, allele, placed, t_len, q_len, prefix, suffix, status, distance,
                                n_eq, n_sub,  n_ins,  n_del, op_off, n_ops, prim_off, n_prims};
    pg::region_align_pairs(x->c, cols, cap);
  });
}

int pg_region_align_ops(pg_ctx* x, uint8_t* op, uint64_t* len, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_align_ops: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_align_ops(x->c, op, len, cap);
  });
}

int pg_region_align_prims(pg_ctx* x, uint64_t* pair, uint8_t* type, uint64_t* tpos, uint64_t* qpos, uint64_t* tlen,
                          uint64_t* qlen, uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_align_prims: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_align_prims(x->c, pair, type, tpos, qpos, tlen, qlen, cap);
  });
}

int pg_region_align_lines(pg_ctx* x, uint64_t* site, int64_t* pos, uint8_t* type, uint64_t* tpos, uint64_t* tlen,
                          uint64_t* qlen, uint64_t* first_prim, uint64_t* ac, uint32_t* n_genomes, uint64_t* bits,
                          uint64_t cap) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_align_lines: ctx is NULL");
    PG_HIP(hipSetDevice(x->c.device));
    pg::region_align_lines(x->c, site, pos, type, tpos, tlen, qlen, first_prim, ac, n_genomes, bits, cap);
  });
}

int pg_region_align_time(pg_ctx* x, double* ms_fill, uint64_t* cells) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_align_time: ctx is NULL");
    if (!x->c.al_ready) throw pg::Error(PG_EINVAL, std::string("pg_region_align_time: ") + NEED_ALIGN);
    if (ms_fill) *ms_fill = x->c.ms_al_fill;
    if (cells) *cells = x->c.al_cells;
  });
}

int pg_region_align_band(pg_ctx* x, uint64_t* n_over, uint64_t* n_banded, uint64_t* n_attempts, uint64_t* band_cells,
                         double* ms_band) {
  return guard([&] {
    if (!x) throw pg::Error(PG_EINVAL, "pg_region_align_band: ctx is NULL");
    if (!x->c.al_ready) throw pg::Error(PG_EINVAL, std::string("pg_region_align_band: ") + NEED_ALIGN);
    if (n_over) *n_over = x->c.al_nover;
    if (n_banded) *n_banded = x->c.al_nbanded;
    if (n_attempts) *n_attempts = x->c.al_nattempts;
    if (band_cells) *band_cells = x->c.al_bandcells;
    if (ms_band) *ms_band = x->c.ms_al_band;
  });
}

int pg_region_align_format(pg_ctx* x, char* out, uint64_t cap, uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes) throw pg::Error(PG_EINVAL, "pg_region_align_format: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_region_align(x->c, out, cap);
  });
}

int pg_region_align_format_fd(pg_ctx* x, int fd, uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes || fd < 0) throw pg::Error(PG_EINVAL, "pg_region_align_format_fd: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_region_align(x->c, nullptr, 0, fd);
  });
}

int pg_region_primitives_vcf(pg_ctx* x, const char* names, const int64_t* name_off, uint64_t n_names, char* out,
                             uint64_t cap, uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes) throw pg::Error(PG_EINVAL, "pg_region_primitives_vcf: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_region_primitives_vcf(x->c, names, name_off, n_names, out, cap);
  });
}

int pg_region_primitives_vcf_fd(pg_ctx* x, const char* names, const int64_t* name_off, uint64_t n_names, int fd,
                                uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes || fd < 0) throw pg::Error(PG_EINVAL, "pg_region_primitives_vcf_fd: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    *n_bytes = pg::format_region_primitives_vcf(x->c, names, name_off, n_names, nullptr, 0, fd);
  });
}

int pg_rows_format(pg_ctx* x, const char* names, const int64_t* name_off, uint64_t n_names, char* out, uint64_t cap,
                   uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes || !name_off) throw pg::Error(PG_EINVAL, "pg_rows_format: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    if (n_names < x->c.n_records) throw pg::Error(PG_EINVAL, "pg_rows_format: fewer names than records");
    *n_bytes = pg::format_rows_text(x->c, names, name_off, n_names, out, cap);
  });
}

int pg_rows_format_fd(pg_ctx* x, const char* names, const int64_t* name_off, uint64_t n_names, int fd,
                      uint64_t* n_bytes) {
  return guard([&] {
    if (!x || !n_bytes || !name_off || fd < 0) throw pg::Error(PG_EINVAL, "pg_rows_format_fd: bad arguments");
    PG_HIP(hipSetDevice(x->c.device));
    if (n_names < x->c.n_records) throw pg::Error(PG_EINVAL, "pg_rows_format_fd: fewer names than records");
    *n_bytes = pg::format_rows_text(x->c, names, name_off, n_names, nullptr, 0, fd);
  });
}

// ---- text of the side file and the region rows (host only, no device work)
uint64_t pg_format_xyz(const uint64_t* t, const int64_t* counts, uint64_t n, char* out, uint64_t cap) {
  if (!out) return n * 106;                               // upper bound: 4 x 20 digits + count + 5 separators
  if (cap < n * 106) return 0;
  const pg::XyzLine line{reinterpret_cast<const pg::ull*>(t), reinterpret_cast<const long long*>(counts)};
  pg::TextWrite s{out, out};
  for (uint64_t i = 0; i < n; ++i) line(s, i);
  return (uint64_t)(s.o - out);
}

uint64_t pg_format_rows(const int64_t* rows5, uint64_t n, const char* names, const int64_t* name_off, char* out,
                        uint64_t cap) {
  uint64_t need = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const int64_t r = rows5[5 * i];
    need += (uint64_t)(name_off[r + 1] - name_off[r]) + 3 * 21 + 6;
  }
  if (!out) return need;
  if (cap < need) return 0;
  const pg::RowLine line{reinterpret_cast<const long long*>(rows5), names,
                         reinterpret_cast<const long long*>(name_off)};
  pg::TextWrite s{out, out};
  for (uint64_t i = 0; i < n; ++i) line(s, i);
  return (uint64_t)(s.o - out);
}

}  // extern "C"
