"""ctypes binding of include/pangenome.h (libpangenome_hip.so).

There is no CPU fallback: if the in-tree HIP library is missing or no HIP
device is usable, every call raises.  Build it with ``python -c "import
__graft_entry__ as g; g.build()"`` (or ``make -C pangenome_amd/csrc``).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, os.environ.get("PG_LIB_NAME", "libpangenome_hip.so"))   # diag builds only

PG_OK = 0
PG_TUNE_K3_CHUNKS = 1
PG_TUNE_BUCKET_SHIFT = 2
PG_TUNE_REGION_CAP = 3
PG_TUNE_H2D_CHUNK = 4
PG_TUNE_HOST_THREADS = 5
PG_TUNE_STAGE_PIECE = 6
PG_TUNE_STAGE_SLOTS = 7
PG_TUNE_HOST_REGISTER = 8
PG_TUNE_DEVICE_CAP = 9          # process-wide: caps (and restarts the peak of) every context's buffers
PG_TUNE_K3_COVER = 10
PG_TUNE_K3_WBLK = 11
PG_TUNE_K3_EMIT = 12
PG_TUNE_K3_TAIL = 13
PG_TUNE_EARLY_SPLIT = 14
PG_TUNE_K3_HEAD = 15
PG_TUNE_H2D_TAIL = 16
PG_TUNE_POISON = 17             # process-wide debug: new device buffers filled with this byte
PG_TUNE_K1 = 18                 # K1 form bits (bit 0 whole-span pass, bit 1 deeper emission prefetch, bit 2 record table ahead of the emission)
PG_TUNE_TIMERS = 19             # bits: HIP timing events of K1 / stage A / stages B-C (default 7)
PG_TUNE_K3_ANCHORS = 20         # packed coverage pass anchors per tile and reference (3-6, 8; 0 = 4)
PG_TUNE_FREQ_FORM = 21          # pg_freq's accumulate pass: 0 aggregated in the wave, 1 every lane its own atomics
PG_TUNE_CMP_CHUNK = 22          # pg_freq_compare's shared pass: label-axis words per block (0 = by size)
PG_TUNE_CMP_FORM = 23           # pg_freq_compare's curve pass: 0 LDS counters up to 2048 genomes, 1 global atomics
PG_TUNE_RDBG_KEYS = 24          # 0 the range pass counts rdBG members, keys swept from the table on export; 1 keys written by the build
PG_TUNE_BUBBLE_HASH_BITS = 25   # 0 the full hash of an inner path; 1..32 its low bits only (tests of the comparison)
PG_TUNE_ALIGN_CELLS = 26        # pg_region_align: a pair with more cells than this is not aligned (0 = 2^24)
PG_TUNE_ALIGN_SCRATCH = 27      # pg_region_align: bytes of direction bits per batch of pairs (0 = 256 MiB)
PG_TUNE_ALIGN_HASH_BITS = 28    # 0 the full hash of a primitive's letters; 1..64 its low bits only (tests of the comparison)
PG_TUNE_ALIGN_BAND = 29         # pg_region_align: 1 = the pairs above the cells cap are aligned in a band of diagonals
PG_TUNE_ALIGN_BAND_CELLS = 30   # the band form: a pair is given up before a band of more cells than this (0 = 2^26)
PG_TUNE_ALIGN_BAND_T0 = 31      # the band form: the first threshold, doubled until it holds the distance (0 = 64)
PG_TUNE_NJ_BLOCKS = 32          # pg_tree_nj: blocks of the arg-min pass (0 = by size); the result is the same at any value
PG_TUNE_BOOT_SCRATCH = 33       # pg_tree_bootstrap: device bytes of a batch of replicates (0 = 256 MiB); the result is the same
PG_TUNE_BOOT_FORM = 34          # pg_tree_bootstrap's NJ: 0 by size and replicates, 1 LDS (n <= 128), 2 global scratch (n <= 1024), 3 per-join launches


class PgStats(C.Structure):
    _fields_ = [
        ("n_bytes", C.c_uint64), ("n_records", C.c_uint64), ("n_bases", C.c_uint64),
        ("n_windows", C.c_uint64), ("n_dbg", C.c_uint64), ("n_rdbg", C.c_uint64),
        ("n_slots", C.c_uint64), ("table_capacity", C.c_uint64),
        ("ms_parse", C.c_double), ("ms_clear", C.c_double), ("ms_insert", C.c_double),
        ("ms_scan", C.c_double), ("sentinel", C.c_uint64),
        ("n_records_a", C.c_uint64), ("ms_split", C.c_double), ("ms_range", C.c_double),
        ("build_flags", C.c_uint64), ("n_work_items", C.c_uint64),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


# every symbol include/pangenome.h declares, with (restype, argtypes)
_P, _U8P, _U64P = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
_I64P, _U16P = C.POINTER(C.c_int64), C.POINTER(C.c_uint16)
_SP = C.POINTER(PgStats)
SIGNATURES = {
    "pg_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "pg_destroy": (None, [_P]),
    "pg_last_error": (C.c_char_p, []),
    "pg_get_k": (C.c_int, [_P]),
    "pg_stream_wait": (C.c_int, [_P, _P]),
    "pg_set_fasta": (C.c_int, [_P, _P, C.c_uint64]),
    "pg_set_fasta_device": (C.c_int, [_P, _P, C.c_uint64]),
    "pg_parse": (C.c_int, [_P, _U64P, _U64P]),
    "pg_parse_host": (C.c_int, [_P, _P, C.c_uint64, _U64P, _U64P]),
    "pg_records": (C.c_int, [_P, _P, _P, _P, _P]),
    "pg_build_dbg": (C.c_int, [_P, _P, C.c_int, C.c_int, _SP]),
    "pg_build_rdbg": (C.c_int, [_P, _U64P, _SP]),
    "pg_build": (C.c_int, [_P, _P, C.c_int, C.c_int, _U64P, _SP]),
    "pg_build_host": (C.c_int, [_P, _P, C.c_uint64, C.c_int, _U64P, _SP]),
    "pg_build_device": (C.c_int, [_P, _P, C.c_uint64, C.c_int, _U64P, _SP]),
    "pg_dbg_export": (C.c_int, [_P, _P, _P, C.c_uint64, _U64P]),
    "pg_rdbg_export": (C.c_int, [_P, _P, C.c_uint64, _U64P]),
    "pg_dbg_partition": (C.c_int, [_P, C.c_int, _P, C.c_uint64, _P]),
    "pg_dbg_merge": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, C.c_int]),
    "pg_dbg_partition_sums": (C.c_int, [_P, C.c_int, _P]),
    "pg_rows_checksum": (C.c_int, [_P, _P, _P, C.c_uint64, _P]),
    "pg_dbg_merge_check": (C.c_int, [_P, _U64P, _U64P]),
    "pg_route_stage_a": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.POINTER(C.c_int)]),
    "pg_route_scatter": (C.c_int, [_P, C.c_int, _P, C.c_uint64, _P]),
    "pg_route_rows_checksum": (C.c_int, [_P, _P, _P, C.c_uint64, _P]),
    "pg_route_finish": (C.c_int, [_P, _U64P, _SP]),
    "pg_route_merge": (C.c_int, [_P, _P, C.c_uint64, C.c_int, C.c_int, _U64P, _SP]),
    "pg_route_merge_segs": (C.c_int, [_P, C.POINTER(C.c_void_p), _P, C.c_int, C.c_int, C.c_int, _U64P, _SP]),
    "pg_edges": (C.c_int, [_P, _P, C.c_int, _U64P]),
    "pg_edges_export": (C.c_int, [_P, _P, _P, _P, C.c_uint64]),
    "pg_set_labels": (C.c_int, [_P, _P, _P, _P, C.c_uint64]),
    "pg_rows": (C.c_int, [_P, _P, C.c_int, _U64P]),
    "pg_rows_export": (C.c_int, [_P, _P, C.c_uint64]),
    "pg_edges_format": (C.c_int, [_P, _P, C.c_uint64, _U64P]),
    "pg_edges_format_fd": (C.c_int, [_P, C.c_int, _U64P]),
    "pg_labels_from_edges": (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P, C.c_uint64, C.c_int64, _U64P]),
    "pg_labels_export": (C.c_int, [_P, _P, _P, _P, C.c_uint64]),
    "pg_cluster_cc": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_int64, _U64P, _U64P]),
    "pg_cluster_markov": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_int64, C.c_uint32, C.c_uint32, C.c_uint32, _U64P, _U64P,
                                    C.POINTER(C.c_uint32), _U64P]),
    "pg_cluster_markov_matrix": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.POINTER(C.c_uint32)]),
    "pg_cluster_markov_stats": (C.c_int, [_P, _U64P, C.POINTER(C.c_uint32), _U64P, _U64P, _U64P]),
    "pg_cluster_sweep": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.c_uint64, _U64P, _I64P, _P, _P, _P, _P]),
    "pg_clusters_format": (C.c_int, [_P, _P, C.c_uint64, _U64P]),
    "pg_clusters_format_fd": (C.c_int, [_P, C.c_int, _U64P]),
    "pg_freq": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, C.c_uint32, _U64P, _U64P, _U64P]),
    "pg_freq_export": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_uint64]),
    "pg_freq_spectrum": (C.c_int, [_P, _P, _P, C.c_uint64]),
    "pg_freq_groups": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint64]),
    "pg_freq_format": (C.c_int, [_P, _P, C.c_uint64, _U64P]),
    "pg_freq_format_fd": (C.c_int, [_P, C.c_int, _U64P]),
    "pg_freq_compare": (C.c_int, [_P, _P, C.c_uint64, C.c_uint32, _P, C.c_uint32]),
    "pg_freq_shared": (C.c_int, [_P, _P, C.c_uint64]),
    "pg_freq_curve": (C.c_int, [_P, _P, _P, C.c_uint64]),
    "pg_kmer_colors": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint32, C.c_int, _U64P, _U64P, _U64P, _U64P]),
    "pg_kmer_colors_export": (C.c_int, [_P, _P, _P, C.c_uint64, _U64P]),
    "pg_kmer_colors_spectrum": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "pg_kmer_compare": (C.c_int, [_P, _P, C.c_uint32]),
    "pg_kmer_compare_export": (C.c_int, [_P, _P, C.c_uint64, _P, _P, C.c_uint64]),
    "pg_kmer_colors_time": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), _U64P]),
    "pg_kmer_colors_drop": (C.c_int, [_P]),
    "pg_tree_nj": (C.c_int, [_P, _P, C.c_uint32, _U64P]),
    "pg_tree_dist": (C.c_int, [_P, _P, C.c_uint64]),
    "pg_tree_joins": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint64]),
    "pg_tree_root": (C.c_int, [_P, C.POINTER(C.c_uint32), _P, _P]),
    "pg_tree_time": (C.c_int, [_P, C.POINTER(C.c_double), _U64P]),
    "pg_tree_bootstrap": (C.c_int, [_P, _P, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, _P, C.c_uint64]),
    "pg_tree_support": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(C.c_uint32)]),
    "pg_tree_bootstrap_joins": (C.c_int, [_P, _P, _P, C.c_uint64]),
    "pg_tree_bootstrap_time": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), _U64P]),
    "pg_tree_bootstrap_form": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "pg_region_graph": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, C.c_uint32, _U64P, _U64P, _U64P, _U64P]),
    "pg_region_nodes": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint64]),
    "pg_region_links": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint64]),
    "pg_region_paths": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint64]),
    "pg_region_links_format": (C.c_int, [_P, _P, C.c_uint64, _U64P]),
    "pg_region_links_format_fd": (C.c_int, [_P, C.c_int, _U64P]),
    "pg_region_gfa": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.c_uint64, _U64P]),
    "pg_region_gfa_fd": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_int, _U64P]),
    "pg_region_seqs": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, C.c_uint32, _U64P, _U64P, _U64P]),
    "pg_region_seqs_table": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_uint64]),
    "pg_region_seqs_bases": (C.c_int, [_P, _P, C.c_uint64, _U64P]),
    "pg_region_seqs_time": (C.c_int, [_P, C.POINTER(C.c_double), _U64P]),
    "pg_region_fasta": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.c_uint64, _U64P]),
    "pg_region_fasta_fd": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_int, _U64P]),
    "pg_region_gfa_seq": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.c_uint64, _U64P]),
    "pg_region_gfa_seq_fd": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_int, _U64P]),
    "pg_region_sites": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, C.c_uint32, _U64P, _U64P, _U64P, _U64P]),
    "pg_region_sites_table": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_uint64]),
    "pg_region_sites_alleles": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_uint64]),
    "pg_region_sites_groups": (C.c_int, [_P, _P, _P, _P, C.c_uint64]),
    "pg_region_sites_format": (C.c_int, [_P, _P, C.c_uint64, _U64P]),
    "pg_region_sites_format_fd": (C.c_int, [_P, C.c_int, _U64P]),
    "pg_region_bubbles": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, C.c_uint32, C.c_uint32, _U64P, _U64P, _U64P,
                                    _U64P, _U64P]),
    "pg_region_bubbles_table": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_uint64]),
    "pg_region_bubbles_alleles": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_uint64]),
    "pg_region_bubbles_inner": (C.c_int, [_P, _P, C.c_uint64, _U64P]),
    "pg_region_bubbles_groups": (C.c_int, [_P, _P, _P, _P, C.c_uint64]),
    "pg_region_bubbles_anchors": (C.c_int, [_P, _P, _P, C.c_uint64]),
    "pg_region_bubbles_format": (C.c_int, [_P, _P, C.c_uint64, _U64P]),
    "pg_region_bubbles_format_fd": (C.c_int, [_P, C.c_int, _U64P]),
    "pg_region_variants": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, C.c_uint32, C.c_uint32, _U64P, _U64P, _U64P,
                                     _U64P]),
    "pg_region_variants_alleles": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_uint64]),
    "pg_region_variants_bases": (C.c_int, [_P, _P, C.c_uint64, _U64P]),
    "pg_region_variants_placed": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_uint64]),
    "pg_region_variants_time": (C.c_int, [_P, C.POINTER(C.c_double), _U64P]),
    "pg_region_alleles_fasta": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.c_uint64, _U64P]),
    "pg_region_alleles_fasta_fd": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_int, _U64P]),
    "pg_region_vcf": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.c_uint64, _U64P]),
    "pg_region_vcf_fd": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_int, _U64P]),
    "pg_region_align": (C.c_int, [_P, _U64P, _U64P, _U64P, _U64P, _U64P]),
    "pg_region_align_pairs": (C.c_int, [_P] + [_P] * 17 + [C.c_uint64]),
    "pg_region_align_ops": (C.c_int, [_P, _P, _P, C.c_uint64]),
    "pg_region_align_prims": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_uint64]),
    "pg_region_align_lines": (C.c_int, [_P] + [_P] * 10 + [C.c_uint64]),
    "pg_region_align_time": (C.c_int, [_P, C.POINTER(C.c_double), _U64P]),
    "pg_region_align_band": (C.c_int, [_P, _U64P, _U64P, _U64P, _U64P, C.POINTER(C.c_double)]),
    "pg_region_align_format": (C.c_int, [_P, _P, C.c_uint64, _U64P]),
    "pg_region_align_format_fd": (C.c_int, [_P, C.c_int, _U64P]),
    "pg_region_primitives_vcf": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.c_uint64, _U64P]),
    "pg_region_primitives_vcf_fd": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_int, _U64P]),
    "pg_rows_format": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.c_uint64, _U64P]),
    "pg_rows_format_fd": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_int, _U64P]),
    "pg_get_stats": (C.c_int, [_P, _SP]),
    "pg_tune": (C.c_int, [_P, C.c_int, C.c_int64]),
    "pg_dbg_dump": (C.c_int, [_P, _U64P, _P, _P, _P, _U64P]),
    "pg_dbg_dump_fd": (C.c_int, [_P, _U64P, C.c_int, _P, _P, _U64P]),
    "pg_dbg_load": (C.c_int, [_P, _P, _P, _P, C.c_uint64]),
    "pg_oakht_capacity": (C.c_uint64, [C.c_uint64]),
    "pg_device_bytes": (C.c_uint64, [C.c_int]),
    "pg_format_xyz": (C.c_uint64, [_P, _P, C.c_uint64, _P, C.c_uint64]),
    "pg_format_rows": (C.c_uint64, [_P, C.c_uint64, _P, _P, _P, C.c_uint64]),
}

_lib = None


class PangenomeError(RuntimeError):
    pass


def load():
    """Load the in-tree HIP library (raises if it is not built)."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise ImportError(
                "libpangenome_hip.so is not built (%s); run __graft_entry__.build() "
                "or `make -C pangenome_amd/csrc` — there is no CPU fallback" % LIB_PATH)
        # One HIP runtime per process: torch ships its own libamdhip64.so.7
        # (same SONAME as /opt/rocm's).  Whichever loads first serves both, and
        # torch's build refuses the system one, so let torch load it first;
        # device buffers from torch (bench, multi-GPU exchange) then share it.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc: int, what: str):
    if rc != PG_OK:
        msg = load().pg_last_error()
        raise PangenomeError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))


def ptr(a: np.ndarray | None):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _names_blob(names: list):
    """Record names as pg_rows_format takes them: one byte blob and R + 1
    offsets."""
    blob = b"".join(names)
    off = np.zeros(len(names) + 1, np.int64)
    if names:
        off[1:] = np.cumsum([len(x) for x in names])
    return (np.frombuffer(blob, np.uint8) if blob else np.zeros(1, np.uint8)), off


def _names_args(names: list):
    """The leading arguments of a text call that takes record names."""
    return (*_names_blob(names), len(names))


def _row_args(rec_group, rows):
    """(rows5, n_rows, rec_group, n_records) as a row pass takes them
    (pg_freq, pg_region_graph, pg_region_seqs); rows None: the device rows."""
    grp = np.ascontiguousarray(rec_group, dtype=np.int32).reshape(-1)
    n_records = grp.shape[0]
    if not n_records:
        grp = np.full(1, -1, np.int32)               # (never NULL: an empty array's pointer may be)
    r5, n_rows = None, 0
    if rows is not None:
        r5 = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 5)
        n_rows = r5.shape[0]
        if not n_rows:
            r5 = np.zeros((1, 5), np.int64)          # (NULL would mean the device rows)
    return r5, n_rows, grp, n_records


def _text(h, fn, what, *lead) -> bytes:
    """The bytes of a size-then-fill call fn(h, *lead, out, cap, &n); an
    array in lead goes as its pointer."""
    lead = [ptr(a) if isinstance(a, np.ndarray) else a for a in lead]
    n = C.c_uint64()
    check(fn(h, *lead, None, 0, C.byref(n)), what)
    buf = np.empty(max(n.value, 1), np.uint8)
    check(fn(h, *lead, ptr(buf), buf.shape[0], C.byref(n)), what)
    return buf[:n.value].tobytes()


def _write(h, fn, what, fd, *lead) -> int:
    """fn(h, *lead, fd, &n): the text written to descriptor fd; its bytes."""
    lead = [ptr(a) if isinstance(a, np.ndarray) else a for a in lead]
    n = C.c_uint64()
    check(fn(h, *lead, int(fd), C.byref(n)), what)
    return n.value


class Context:
    """One pg_ctx: one HIP device, one stream, all device buffers."""

    def __init__(self, k: int, device: int = 0):
        self.lib = load()
        h = C.c_void_p()
        check(self.lib.pg_create(C.byref(h), device, k), "pg_create")
        self.h = h
        self.k = self.lib.pg_get_k(h)
        self.n_records = 0
        self.n_bases = 0
        self._keepalive = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.pg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -------------------------------------------------------------- input
    def set_fasta(self, data):
        """Host bytes (bytes / bytearray / np.uint8 array / mmap)."""
        arr = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        check(self.lib.pg_set_fasta(self.h, ptr(arr), arr.shape[0]), "pg_set_fasta")

    def set_fasta_host_ptr(self, host_ptr: int, nbytes: int):
        """Host bytes at a raw address (e.g. a pinned torch tensor's data_ptr():
        the H2D copy is then plain DMA)."""
        check(self.lib.pg_set_fasta(self.h, C.c_void_p(host_ptr), nbytes), "pg_set_fasta")

    def set_fasta_device(self, dev_ptr: int, nbytes: int, keepalive=None):
        self._keepalive = keepalive
        check(self.lib.pg_set_fasta_device(self.h, C.c_void_p(dev_ptr), nbytes), "pg_set_fasta_device")

    def parse(self):
        nr, nb = C.c_uint64(), C.c_uint64()
        check(self.lib.pg_parse(self.h, C.byref(nr), C.byref(nb)), "pg_parse")
        self.n_records, self.n_bases = nr.value, nb.value
        return self.n_records, self.n_bases

    def parse_host(self, data):
        """set_fasta + parse of host bytes in one call: chunked H2D pipelined
        with K1 (pg_parse_host)."""
        arr = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        return self.parse_host_ptr(arr.ctypes.data if arr.shape[0] else None, arr.shape[0])

    def parse_host_ptr(self, host_ptr, nbytes: int):
        """parse_host from a raw address (e.g. a pinned torch tensor's data_ptr())."""
        nr, nb = C.c_uint64(), C.c_uint64()
        check(self.lib.pg_parse_host(self.h, C.c_void_p(host_ptr), nbytes, C.byref(nr), C.byref(nb)),
              "pg_parse_host")
        self.n_records, self.n_bases = nr.value, nb.value
        return self.n_records, self.n_bases

    def records(self):
        R = self.n_records
        out = [np.empty(R, np.int64) for _ in range(4)]
        check(self.lib.pg_records(self.h, *[ptr(a) for a in out]), "pg_records")
        return dict(seq_len=out[0], hdr_start=out[1], hdr_len=out[2], ptr=out[3])

    # ---------------------------------------------------------------- dBG
    def build_dbg(self, rec_flags=None, extra_empty: int = 0, rc0: bool = True) -> PgStats:
        st = PgStats()
        f = None if rec_flags is None else np.ascontiguousarray(rec_flags, dtype=np.uint8)
        check(self.lib.pg_build_dbg(self.h, ptr(f), int(extra_empty), int(bool(rc0)), C.byref(st)),
              "pg_build_dbg")
        return st

    def build_rdbg(self) -> PgStats:
        st = PgStats()
        n = C.c_uint64()
        check(self.lib.pg_build_rdbg(self.h, C.byref(n), C.byref(st)), "pg_build_rdbg")
        return st

    def build(self, rec_flags=None, extra_empty: int = 0, rc0: bool = True) -> PgStats:
        """build_dbg + build_rdbg in one call (pg_build: K5 runs right behind K3)."""
        st = PgStats()
        n = C.c_uint64()
        f = None if rec_flags is None else np.ascontiguousarray(rec_flags, dtype=np.uint8)
        check(self.lib.pg_build(self.h, ptr(f), int(extra_empty), int(bool(rc0)), C.byref(n), C.byref(st)),
              "pg_build")
        return st

    def build_host(self, data, rc0: bool = True) -> PgStats:
        """parse + build of every record from host bytes with stage A streamed
        under the chunked upload (pg_build_host); the record table is
        available afterwards (records())."""
        arr = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        return self.build_host_ptr(arr.ctypes.data if arr.shape[0] else None, arr.shape[0], rc0)

    def build_host_ptr(self, host_ptr, nbytes: int, rc0: bool = True) -> PgStats:
        st = PgStats()
        n = C.c_uint64()
        check(self.lib.pg_build_host(self.h, C.c_void_p(host_ptr), nbytes, int(bool(rc0)), C.byref(n), C.byref(st)),
              "pg_build_host")
        self.n_records, self.n_bases = st.n_records, st.n_bases
        return st

    def build_device(self, dev_ptr: int, nbytes: int, rc0: bool = True, keepalive=None) -> PgStats:
        """set_fasta_device + parse + build of every record in one call
        (pg_build_device) for a FASTA already in HBM."""
        st = PgStats()
        n = C.c_uint64()
        self._keepalive = keepalive
        check(self.lib.pg_build_device(self.h, C.c_void_p(dev_ptr), nbytes, int(bool(rc0)), C.byref(n),
                                       C.byref(st)), "pg_build_device")
        self.n_records, self.n_bases = st.n_records, st.n_bases
        return st

    def stream_wait(self, stream_handle: int):
        """This context's streams wait (on the device) for the work queued so
        far on the HIP stream `stream_handle` (e.g. torch's current stream's
        .cuda_stream): pg_stream_wait."""
        check(self.lib.pg_stream_wait(self.h, C.c_void_p(stream_handle) if stream_handle else None),
              "pg_stream_wait")

    def tune(self, what: int, value: int):
        check(self.lib.pg_tune(self.h, int(what), int(value)), "pg_tune")

    def stats(self) -> PgStats:
        st = PgStats()
        check(self.lib.pg_get_stats(self.h, C.byref(st)), "pg_get_stats")
        return st

    def dbg(self):
        n = C.c_uint64()
        check(self.lib.pg_dbg_export(self.h, None, None, 0, C.byref(n)), "pg_dbg_export")
        keys = np.empty(n.value, np.uint64)
        masks = np.empty(n.value, np.uint16)
        check(self.lib.pg_dbg_export(self.h, ptr(keys), ptr(masks), n.value, C.byref(n)), "pg_dbg_export")
        return keys, masks                        # (sorted by key on the device)

    def rdbg(self):
        n = C.c_uint64()
        check(self.lib.pg_rdbg_export(self.h, None, 0, C.byref(n)), "pg_rdbg_export")
        keys = np.empty(n.value, np.uint64)
        check(self.lib.pg_rdbg_export(self.h, ptr(keys), n.value, C.byref(n)), "pg_rdbg_export")
        return keys                               # (sorted on the device)

    # ----------------------------------------------------- npz persistence
    def dbg_dump(self, capacity: int = 0):
        """The last build's dBG as oakht slot arrays (dump(), :243-261):
        (capacity, size, keys, values, counts)."""
        cap, size = C.c_uint64(capacity), C.c_uint64()
        check(self.lib.pg_dbg_dump(self.h, C.byref(cap), None, None, None, C.byref(size)), "pg_dbg_dump")
        keys = np.empty(cap.value, np.uint64)
        values = np.empty(cap.value, np.uint16)
        counts = np.empty(cap.value, np.uint8)
        check(self.lib.pg_dbg_dump(self.h, C.byref(cap), ptr(keys), ptr(values), ptr(counts), C.byref(size)),
              "pg_dbg_dump")
        return cap.value, size.value, keys, values, counts

    def dbg_dump_size(self, capacity: int = 0):
        """(capacity, size) of dbg_dump without placing or copying anything."""
        cap, size = C.c_uint64(capacity), C.c_uint64()
        check(self.lib.pg_dbg_dump_fd(self.h, C.byref(cap), -1, None, None, C.byref(size)), "pg_dbg_dump_fd")
        return cap.value, size.value

    def dbg_dump_fd(self, fd: int, offsets, capacity: int):
        """The slot arrays of dbg_dump(capacity) written into the open file
        `fd` at offsets[0..2] (keys, values, counts); their CRC-32s."""
        cap, size = C.c_uint64(capacity), C.c_uint64()
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        crc = np.zeros(3, np.uint32)
        check(self.lib.pg_dbg_dump_fd(self.h, C.byref(cap), int(fd), ptr(off), ptr(crc), C.byref(size)),
              "pg_dbg_dump_fd")
        return [int(x) for x in crc]

    def dbg_load(self, keys, masks=None, counts=None):
        """Stage oriented (key, mask, count) slots for the following builds."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        m = None if masks is None else np.ascontiguousarray(masks, dtype=np.uint16)
        c = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint8)
        check(self.lib.pg_dbg_load(self.h, ptr(keys), ptr(m), ptr(c), keys.shape[0]), "pg_dbg_load")

    # ------------------------------------------------------ multi-GPU hooks
    def partition(self, nparts: int, d_out: int | None = None, out_cap: int = 0):
        counts = np.zeros(nparts, np.uint64)
        check(self.lib.pg_dbg_partition(self.h, nparts, None if d_out is None else C.c_void_p(d_out),
                                        out_cap, ptr(counts)), "pg_dbg_partition")
        return counts

    def merge(self, d_records: int, n: int, capacity_hint: int = 0, sentinel: bool = False):
        check(self.lib.pg_dbg_merge(self.h, C.c_void_p(d_records) if n else None, n, capacity_hint,
                                    int(bool(sentinel))), "pg_dbg_merge")

    def partition_sums(self, nparts: int):
        """row_check sums of the last partition scatter's runs (uint64[nparts])."""
        sums = np.zeros(nparts, np.uint64)
        check(self.lib.pg_dbg_partition_sums(self.h, nparts, ptr(sums)), "pg_dbg_partition_sums")
        return sums

    def rows_checksum(self, d_rows: int, seg_off):
        """row_check sums of segments [seg_off[s], seg_off[s+1]) of the 16-byte
        records at device address d_rows (uint64[len(seg_off) - 1])."""
        off = np.ascontiguousarray(seg_off, dtype=np.uint64)
        sums = np.zeros(max(off.shape[0] - 1, 1), np.uint64)
        check(self.lib.pg_rows_checksum(self.h, C.c_void_p(d_rows) if d_rows else None, ptr(off),
                                        max(off.shape[0] - 1, 0), ptr(sums)), "pg_rows_checksum")
        return sums[:max(off.shape[0] - 1, 0)]

    def route_rows_checksum(self, d_rows: int, seg_off):
        """rows_checksum over 12-byte routed rows (pg_route_scatter's layout)."""
        off = np.ascontiguousarray(seg_off, dtype=np.uint64)
        sums = np.zeros(max(off.shape[0] - 1, 1), np.uint64)
        check(self.lib.pg_route_rows_checksum(self.h, C.c_void_p(d_rows) if d_rows else None, ptr(off),
                                              max(off.shape[0] - 1, 0), ptr(sums)), "pg_route_rows_checksum")
        return sums[:max(off.shape[0] - 1, 0)]

    def merge_check(self):
        """(non-empty records, row_check sum) the last merge read."""
        rows, s = C.c_uint64(), C.c_uint64()
        check(self.lib.pg_dbg_merge_check(self.h, C.byref(rows), C.byref(s)), "pg_dbg_merge_check")
        return rows.value, s.value

    # ---------------------------------------------------- routed exchange
    def route_stage_a(self, rec_flags=None, extra_empty: int = 0, rc0: bool = True, nparts: int = 1):
        """Stage A of the build, held for its owners: (records per owner as
        uint64[nparts], whether the n<k sentinel was seen)."""
        counts = np.zeros(nparts, np.uint64)
        sent = C.c_int(0)
        f = None if rec_flags is None else np.ascontiguousarray(rec_flags, dtype=np.uint8)
        check(self.lib.pg_route_stage_a(self.h, ptr(f), int(extra_empty), int(bool(rc0)), int(nparts), ptr(counts),
                                        C.byref(sent)), "pg_route_stage_a")
        return counts, bool(sent.value)

    def route_scatter(self, nparts: int, d_out: int, out_cap: int):
        """The held records as 12-byte rows grouped by owner at d_out; their
        integrity sums per owner (uint64[nparts])."""
        sums = np.zeros(nparts, np.uint64)
        check(self.lib.pg_route_scatter(self.h, int(nparts), C.c_void_p(d_out) if d_out else None, int(out_cap),
                                        ptr(sums)), "pg_route_scatter")
        return sums

    def route_finish(self) -> PgStats:
        st = PgStats()
        n = C.c_uint64()
        check(self.lib.pg_route_finish(self.h, C.byref(n), C.byref(st)), "pg_route_finish")
        return st

    def route_merge(self, d_rows: int, n: int, nparts: int, sentinel: bool = False) -> PgStats:
        st = PgStats()
        nr = C.c_uint64()
        check(self.lib.pg_route_merge(self.h, C.c_void_p(d_rows) if n else None, int(n), int(nparts),
                                      int(bool(sentinel)), C.byref(nr), C.byref(st)), "pg_route_merge")
        return st

    def route_merge_segs(self, segs, nparts: int, sentinel: bool = False) -> PgStats:
        """route_merge over several runs of rows [(device pointer, rows), ...]
        merged as one owner table (pg_route_merge_segs)."""
        st = PgStats()
        nr = C.c_uint64()
        m = len(segs)
        ptrs = (C.c_void_p * max(m, 1))(*[C.c_void_p(p) if n else None for p, n in segs])
        ns = np.ascontiguousarray([int(n) for _, n in segs] or [0], dtype=np.uint64)
        check(self.lib.pg_route_merge_segs(self.h, ptrs, ptr(ns), m, int(nparts), int(bool(sentinel)), C.byref(nr),
                                           C.byref(st)), "pg_route_merge_segs")
        return st

    # -------------------------------------------------------------- walks
    def edges_count(self, rec_flags=None, rc1: bool = False) -> int:
        """pg_edges only: the edges stay on the device (edges_text /
        labels_from_edges / edges_export)."""
        n = C.c_uint64()
        f = None if rec_flags is None else np.ascontiguousarray(rec_flags, dtype=np.uint8)
        check(self.lib.pg_edges(self.h, ptr(f), int(bool(rc1)), C.byref(n)), "pg_edges")
        self.n_edges = n.value
        return n.value

    def edges_export(self):
        m = getattr(self, "n_edges", 0)
        t = np.empty((m, 4), np.uint64)
        cnt = np.empty(m, np.int64)
        walk = np.empty(m, np.int64)
        if m:
            check(self.lib.pg_edges_export(self.h, ptr(t), ptr(cnt), ptr(walk), m), "pg_edges_export")
        return t, cnt, walk

    def edges(self, rec_flags=None, rc1: bool = False):
        n = C.c_uint64()
        f = None if rec_flags is None else np.ascontiguousarray(rec_flags, dtype=np.uint8)
        check(self.lib.pg_edges(self.h, ptr(f), int(bool(rc1)), C.byref(n)), "pg_edges")
        m = n.value
        t = np.empty((m, 4), np.uint64)
        cnt = np.empty(m, np.int64)
        walk = np.empty(m, np.int64)
        if m:
            check(self.lib.pg_edges_export(self.h, ptr(t), ptr(cnt), ptr(walk), m), "pg_edges_export")
        return t, cnt, walk

    def edges_text(self) -> bytes:
        """The `.xyz` text of the last edges() pass (first-occurrence order),
        formatted on the device (pg_edges_format)."""
        return _text(self.h, self.lib.pg_edges_format, "pg_edges_format")

    def edges_write(self, fd: int) -> int:
        """edges_text() written straight to descriptor fd at its position
        (pg_edges_format_fd: pinned pieces, parallel pwrite into a regular
        file); flush any buffered writer on fd first.  Returns the bytes."""
        return _write(self.h, self.lib.pg_edges_format_fd, "pg_edges_format_fd", fd)

    def labels_from_edges(self, tuples=None, mcl_keys=None, mcl_vals=None, mcl_ids=None, next_label: int = 0):
        """seq2graph's label table on the device (pg_labels_from_edges): the
        .mcl entries, then the .xyz nodes in first-appearance order.  tuples
        None: the last edges() pass."""
        n = C.c_uint64()
        t = None if tuples is None else np.ascontiguousarray(tuples, dtype=np.uint64).reshape(-1, 4)
        mk = np.ascontiguousarray(mcl_keys if mcl_keys is not None else np.zeros(0), dtype=np.int64)
        mv = np.ascontiguousarray(mcl_vals if mcl_vals is not None else np.zeros(0), dtype=np.int64)
        mi = np.ascontiguousarray(mcl_ids if mcl_ids is not None else np.zeros(0), dtype=np.int64)
        check(self.lib.pg_labels_from_edges(self.h, ptr(t), 0 if t is None else t.shape[0], ptr(mk), ptr(mv),
                                            ptr(mi), mk.shape[0], int(next_label), C.byref(n)),
              "pg_labels_from_edges")
        self.n_labels = n.value
        self.label_gen = getattr(self, "label_gen", 0) + 1
        return n.value

    def cluster_cc(self, tuples=None, counts=None, min_weight: int = 1):
        """The built-in clusterer (pg_cluster_cc): edges with count <
        min_weight dropped, the connected components of the rest as clusters
        (size descending, then first appearance).  tuples None: the last
        edges() pass on the device.  Replaces the label table with (key,
        value) -> `.mcl` line index; returns (n_clusters, n_nodes)."""
        nc, nu = C.c_uint64(), C.c_uint64()
        t = None if tuples is None else np.ascontiguousarray(tuples, dtype=np.uint64).reshape(-1, 4)
        cn = None if counts is None else np.ascontiguousarray(counts, dtype=np.int64)
        if t is not None and cn is not None and cn.shape[0] != t.shape[0]:
            raise ValueError("cluster_cc: %d tuples, %d counts" % (t.shape[0], cn.shape[0]))
        check(self.lib.pg_cluster_cc(self.h, ptr(t), ptr(cn), 0 if t is None else t.shape[0], int(min_weight),
                                     C.byref(nc), C.byref(nu)), "pg_cluster_cc")
        self.n_labels = nu.value
        self.label_gen = getattr(self, "label_gen", 0) + 1
        return nc.value, nu.value

    def cluster_markov(self, tuples=None, counts=None, min_weight: int = 1, inflation2: int = 3, select: int = 64,
                       max_iter: int = 200):
        """Markov clustering (pg_cluster_markov; host.cluster_markov is its
        specification): inflation inflation2 / 2, columns pruned to `select`
        entries, at most max_iter iterations.  tuples None: the last edges()
        pass on the device.  The result takes cluster_cc's place (clusters_text,
        labels); returns (n_clusters, n_nodes, n_iter, chaos)."""
        nc, nu, ni, ch = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint64()
        t = None if tuples is None else np.ascontiguousarray(tuples, dtype=np.uint64).reshape(-1, 4)
        cn = None if counts is None else np.ascontiguousarray(counts, dtype=np.int64)
        if t is not None and cn is not None and cn.shape[0] != t.shape[0]:
            raise ValueError("cluster_markov: %d tuples, %d counts" % (t.shape[0], cn.shape[0]))
        for name, v in (("inflation2", inflation2), ("select", select), ("max_iter", max_iter)):
            if not 0 <= int(v) < 2 ** 32:
                raise ValueError("cluster_markov: %s = %d" % (name, int(v)))
        check(self.lib.pg_cluster_markov(self.h, ptr(t), ptr(cn), 0 if t is None else t.shape[0], int(min_weight),
                                         int(inflation2), int(select), int(max_iter), C.byref(nc), C.byref(nu),
                                         C.byref(ni), C.byref(ch)), "pg_cluster_markov")
        self.n_labels = nu.value
        self.label_gen = getattr(self, "label_gen", 0) + 1
        self.mk_shape = (nu.value, int(select))
        return nc.value, nu.value, ni.value, ch.value

    def cluster_markov_matrix(self):
        """The last cluster_markov's final matrix (pg_cluster_markov_matrix):
        col_len uint32 [U], rows and vals uint32 [U, select], each column's
        entries by row ascending, zero behind them."""
        U, S = getattr(self, "mk_shape", (0, 1))
        col_len, rows, vals = np.zeros(max(U, 1), np.uint32), np.zeros((max(U, 1), S), np.uint32), np.zeros((max(U, 1), S), np.uint32)
        sel = C.c_uint32()
        check(self.lib.pg_cluster_markov_matrix(self.h, ptr(col_len), ptr(rows), ptr(vals), U, C.byref(sel)),
              "pg_cluster_markov_matrix")
        return col_len[:U], rows[:U], vals[:U]

    def cluster_markov_stats(self):
        """(n_nodes, select, cols_wave, cols_mid, cols_block) of the last
        cluster_markov: the columns its iterations ran in each size class
        (pg_cluster_markov_stats)."""
        nu, sel, cw, cm, cb = C.c_uint64(), C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(self.lib.pg_cluster_markov_stats(self.h, C.byref(nu), C.byref(sel), C.byref(cw), C.byref(cm),
                                               C.byref(cb)), "pg_cluster_markov_stats")
        return nu.value, sel.value, cw.value, cm.value, cb.value

    def _sweep(self, thresholds, tuples, counts):
        """pg_cluster_sweep: (n_nodes, max_weight) and the four arrays."""
        thr = np.ascontiguousarray(thresholds, dtype=np.int64).reshape(-1)
        t = None if tuples is None else np.ascontiguousarray(tuples, dtype=np.uint64).reshape(-1, 4)
        cn = None if counts is None else np.ascontiguousarray(counts, dtype=np.int64)
        if t is not None and cn is not None and cn.shape[0] != t.shape[0]:
            raise ValueError("cluster_sweep: %d tuples, %d counts" % (t.shape[0], cn.shape[0]))
        n = 0 if t is None else t.shape[0]
        if t is not None and not n:                      # (never NULL: an empty array's pointer may be,
            t = np.zeros((1, 4), np.uint64)              # and NULL tuples would mean the device edges)
            cn = None if cn is None else np.zeros(1, np.int64)
        nu, mw = C.c_uint64(), C.c_int64()
        out = [np.zeros(thr.shape[0], np.uint64) for _ in range(4)]
        check(self.lib.pg_cluster_sweep(self.h, ptr(t), ptr(cn), n,
                                        ptr(thr) if thr.shape[0] else None, thr.shape[0], C.byref(nu), C.byref(mw),
                                        *[ptr(a) for a in out]), "pg_cluster_sweep")
        return nu.value, mw.value, thr, out

    def cluster_sweep(self, thresholds, tuples=None, counts=None):
        """The cluster curve (pg_cluster_sweep): for every threshold of the
        strictly ascending list, what cluster_cc(min_weight=threshold) would
        form, from one union-find kept from the highest threshold down.
        tuples None: the last edges() pass on the device.  A query: the label
        table and the last cluster_cc's text stay.  Returns a dict of arrays:
        w, edges (count >= w), clusters, largest, singletons."""
        _, _, thr, (edges, clusters, largest, singles) = self._sweep(thresholds, tuples, counts)
        return {"w": thr, "edges": edges, "clusters": clusters, "largest": largest, "singletons": singles}

    def cluster_weights(self, tuples=None, counts=None):
        """(n_nodes, max_weight) of the edges, max_weight the largest count
        (0 with no edges): pg_cluster_sweep's query form."""
        return self._sweep(np.zeros(0, np.int64), tuples, counts)[:2]

    def clusters_text(self) -> bytes:
        """The `.mcl` text of the last cluster_cc (pg_clusters_format)."""
        return _text(self.h, self.lib.pg_clusters_format, "pg_clusters_format")

    def clusters_write(self, fd: int) -> int:
        """clusters_text() written straight to descriptor fd at its position
        (pg_clusters_format_fd); flush any buffered writer on fd first."""
        return _write(self.h, self.lib.pg_clusters_format_fd, "pg_clusters_format_fd", fd)

    def labels(self, gen=None):
        """(keys, vals, ids) of the device label table, in insertion order.
        `gen`: the label_gen a caller's view was made at; a later label pass
        (set_labels / labels_from_edges / cluster_cc) on this context replaced that table,
        and reading it then raises instead of returning the newer labels."""
        if gen is not None and gen != getattr(self, "label_gen", 0):
            raise RuntimeError("label table: replaced by a later label pass on this context (generation %d, now %d)"
                               % (gen, getattr(self, "label_gen", 0)))
        n = getattr(self, "n_labels", 0)
        out = [np.empty(n, np.int64) for _ in range(3)]
        if n:
            check(self.lib.pg_labels_export(self.h, *[ptr(a) for a in out], n), "pg_labels_export")
        return tuple(out)

    def set_labels(self, keys, vals, ids):
        keys = np.ascontiguousarray(keys, np.int64)
        vals = np.ascontiguousarray(vals, np.int64)
        ids = np.ascontiguousarray(ids, np.int64)
        check(self.lib.pg_set_labels(self.h, ptr(keys), ptr(vals), ptr(ids), keys.shape[0]), "pg_set_labels")
        self.n_labels = keys.shape[0]
        self.label_gen = getattr(self, "label_gen", 0) + 1

    def rows_count(self, rec_flags=None, rc1: bool = False) -> int:
        """pg_rows only: the rows stay on the device (rows_text / rows())."""
        n = C.c_uint64()
        f = None if rec_flags is None else np.ascontiguousarray(rec_flags, dtype=np.uint8)
        check(self.lib.pg_rows(self.h, ptr(f), int(bool(rc1)), C.byref(n)), "pg_rows")
        return n.value

    def rows_text(self, names: list) -> bytes:
        """The region rows' text of the last pg_rows, formatted on the device
        (pg_rows_format); names[r] = record r's qid."""
        return _text(self.h, self.lib.pg_rows_format, "pg_rows_format", *_names_args(names))

    def rows_write(self, names: list, fd: int) -> int:
        """rows_text(names) written straight to descriptor fd at its position
        (pg_rows_format_fd); flush any buffered writer on fd first."""
        return _write(self.h, self.lib.pg_rows_format_fd, "pg_rows_format_fd", fd, *_names_args(names))

    def rows(self, rec_flags=None, rc1: bool = False):
        n = C.c_uint64()
        f = None if rec_flags is None else np.ascontiguousarray(rec_flags, dtype=np.uint8)
        check(self.lib.pg_rows(self.h, ptr(f), int(bool(rc1)), C.byref(n)), "pg_rows")
        out = np.empty((n.value, 5), np.int64)
        if n.value:
            check(self.lib.pg_rows_export(self.h, ptr(out), n.value), "pg_rows_export")
        return out

    # ---------------------------------------------------- frequency table
    def freq(self, rec_group, n_groups: int, rows=None):
        """The frequency table (pg_freq) of the last row pass where it lies on
        the device (rows None) or of host rows [n, 5]; rec_group[r] = record
        r's genome in [0, n_groups) or -1.  Returns (n_labels, n_used,
        n_skipped); the table stays on the device (freq_table /
        freq_spectrum / freq_groups / freq_text / freq_write)."""
        r5, n_rows, grp, n_records = _row_args(rec_group, rows)
        nl, nu, ns = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(self.lib.pg_freq(self.h, ptr(r5), n_rows, ptr(grp), n_records, int(n_groups),
                               C.byref(nl), C.byref(nu), C.byref(ns)), "pg_freq")
        self.n_freq, self.freq_groups_n = nl.value, int(n_groups)
        return nl.value, nu.value, ns.value

    def freq_table(self) -> dict:
        """The table of the last freq(): labels, n_genomes, rows, plus, bp,
        min_len, max_len and the presence bits [n, W] (pg_freq_export)."""
        n, G = getattr(self, "n_freq", 0), getattr(self, "freq_groups_n", 0)
        W = (G + 63) // 64
        t = {"labels": np.empty(n, np.int64), "n_genomes": np.empty(n, np.uint32)}
        for k in ("rows", "plus", "bp", "min_len", "max_len"):
            t[k] = np.empty(n, np.uint64)
        t["bits"] = np.empty((n, W), np.uint64)
        check(self.lib.pg_freq_export(self.h, *[ptr(t[k]) for k in ("labels", "n_genomes", "rows", "plus", "bp",
                                                                     "min_len", "max_len", "bits")], n),
              "pg_freq_export")
        return t

    def freq_spectrum(self):
        """(labels_by_g, bp_by_g), uint64 [n_groups + 1] (pg_freq_spectrum)."""
        nb = getattr(self, "freq_groups_n", 0) + 1
        a, b = np.empty(nb, np.uint64), np.empty(nb, np.uint64)
        check(self.lib.pg_freq_spectrum(self.h, ptr(a), ptr(b), nb), "pg_freq_spectrum")
        return a, b

    def freq_groups(self) -> dict:
        """Per genome: g_rows, g_bp, g_core, g_shell, g_unique (pg_freq_groups)."""
        G = getattr(self, "freq_groups_n", 0)
        names = ("g_rows", "g_bp", "g_core", "g_shell", "g_unique")
        t = {k: np.empty(G, np.uint64) for k in names}
        check(self.lib.pg_freq_groups(self.h, *[ptr(t[k]) for k in names], G), "pg_freq_groups")
        return t

    def freq_text(self) -> bytes:
        """The table's text, formatted on the device (pg_freq_format)."""
        return _text(self.h, self.lib.pg_freq_format, "pg_freq_format")

    def freq_write(self, fd: int) -> int:
        """freq_text() written straight to descriptor fd at its position
        (pg_freq_format_fd); flush any buffered writer on fd first."""
        return _write(self.h, self.lib.pg_freq_format_fd, "pg_freq_format_fd", fd)

    # ---------------------------------------------------- genome comparison
    def freq_compare(self, orders, bits=None, n_groups=None):
        """The shared-label matrix and the pan / core curves (pg_freq_compare)
        of the last freq()'s table where it lies on the device (bits None;
        n_groups defaults to that table's) or of host presence bits [n, W]
        over n_groups genomes.  orders: int32 [P, n_groups], every row a
        permutation (None: no order).  The results stay on the device
        (freq_shared / freq_curves)."""
        G = int(getattr(self, "freq_groups_n", 0) if n_groups is None else n_groups)
        o = np.zeros((0, G), np.int32) if orders is None else np.ascontiguousarray(orders, dtype=np.int32)
        o = o.reshape(-1, G) if G else o.reshape(o.shape[0], 0)
        P = o.shape[0]
        b, n = None, 0
        if bits is not None:
            b = np.ascontiguousarray(bits, dtype=np.uint64)
            n = b.shape[0]
            b = b.reshape(n, (G + 63) // 64)
            if not b.size:
                b = np.zeros(1, np.uint64)           # (NULL would mean the device table)
        if P and not o.size:
            o = np.zeros(1, np.int32)                # (no genomes: P empty rows, but not NULL)
        check(self.lib.pg_freq_compare(self.h, ptr(b), n, G, ptr(o) if P else None, P), "pg_freq_compare")
        self.cmp_groups_n, self.cmp_orders_n = G, P

    def freq_shared(self) -> np.ndarray:
        """shared[g][h], uint64 [G, G]: the labels in both g and h (pg_freq_shared)."""
        G = getattr(self, "cmp_groups_n", 0)
        s = np.empty((G, G), np.uint64)
        check(self.lib.pg_freq_shared(self.h, ptr(s), G * G), "pg_freq_shared")
        return s

    def freq_curves(self):
        """(pan, core), uint64 [P, G]: the labels in at least one / in every
        one of the first n genomes of each order (pg_freq_curve)."""
        G, P = getattr(self, "cmp_groups_n", 0), getattr(self, "cmp_orders_n", 0)
        pan, core = np.empty((P, G), np.uint64), np.empty((P, G), np.uint64)
        check(self.lib.pg_freq_curve(self.h, ptr(pan), ptr(core), P * G), "pg_freq_curve")
        return pan, core

    # ---------------------------------------------------- k-mer colours
    def kmer_colors(self, rec_group, n_groups: int, rec_flags=None, rc0: bool = True):
        """The k-mer colours (pg_kmer_colors) of the dBG table in the context:
        rec_group[r] = record r's genome in [0, n_groups) or -1; rec_flags as
        build_dbg takes them (None: all); rc0 as the table was built.  Returns
        (n_keys, n_windows, n_missing, n_uncoloured); the colours stay on the
        device (kmer_colors_export / kmer_colors_spectrum / kmer_compare)
        until kmer_colors_drop or a call that replaces the table."""
        grp = np.ascontiguousarray(rec_group, dtype=np.int32).reshape(-1)
        R = grp.shape[0]
        if not R:
            grp = np.full(1, -1, np.int32)               # (never NULL: an empty array's pointer may be)
        f = None if rec_flags is None else np.ascontiguousarray(rec_flags, dtype=np.uint8)
        if f is not None and not f.size:
            f = None
        out = [C.c_uint64() for _ in range(4)]
        check(self.lib.pg_kmer_colors(self.h, ptr(grp), ptr(f), R, int(n_groups), int(bool(rc0)),
                                      *[C.byref(x) for x in out]), "pg_kmer_colors")
        self.kc_groups_n = int(n_groups)
        return tuple(x.value for x in out)

    def kmer_colors_export(self, keys: bool = True, bits: bool = True):
        """(keys uint64 [n] ascending, bits uint64 [n, W]) of the last
        kmer_colors() (pg_kmer_colors_export); a part not asked for is None."""
        n = C.c_uint64()
        check(self.lib.pg_kmer_colors_export(self.h, None, None, 0, C.byref(n)), "pg_kmer_colors_export")
        W = (getattr(self, "kc_groups_n", 0) + 63) // 64
        k = np.empty(n.value, np.uint64) if keys else None
        b = np.empty((n.value, W), np.uint64) if bits else None
        check(self.lib.pg_kmer_colors_export(self.h, ptr(k), ptr(b), n.value, C.byref(n)), "pg_kmer_colors_export")
        return k, b

    def kmer_colors_spectrum(self) -> dict:
        """kmers_by_g [G + 1] and per genome g_kmers, g_core, g_shell,
        g_unique [G] of the last kmer_colors() (pg_kmer_colors_spectrum)."""
        G = getattr(self, "kc_groups_n", 0)
        t = {"kmers_by_g": np.zeros(G + 1, np.uint64)}
        for k in ("g_kmers", "g_core", "g_shell", "g_unique"):
            t[k] = np.zeros(max(G, 1), np.uint64)
        check(self.lib.pg_kmer_colors_spectrum(self.h, *[ptr(a) for a in t.values()]), "pg_kmer_colors_spectrum")
        for k in ("g_kmers", "g_core", "g_shell", "g_unique"):
            t[k] = t[k][:G]
        return t

    def kmer_compare(self, orders):
        """The colours compared where they lie (pg_kmer_compare): orders int32
        [P, G], every row a permutation (None: no order).  Returns (shared
        [G, G], pan [P, G], core [P, G]) (pg_kmer_compare_export)."""
        G = getattr(self, "kc_groups_n", 0)
        o = np.zeros((0, G), np.int32) if orders is None else np.ascontiguousarray(orders, dtype=np.int32)
        o = o.reshape(-1, G) if G else o.reshape(o.shape[0], 0)
        P = o.shape[0]
        if P and not o.size:
            o = np.zeros(1, np.int32)                # (no genomes: P empty rows, but not NULL)
        check(self.lib.pg_kmer_compare(self.h, ptr(o) if P else None, P), "pg_kmer_compare")
        self.kc_orders_n = P
        return self.kmer_compare_export()

    def kmer_compare_export(self):
        """(shared, pan, core) of the last kmer_compare() (pg_kmer_compare_export)."""
        G, P = getattr(self, "kc_groups_n", 0), getattr(self, "kc_orders_n", 0)
        s = np.zeros((G, G), np.uint64)
        pan, core = np.zeros((P, G), np.uint64), np.zeros((P, G), np.uint64)
        check(self.lib.pg_kmer_compare_export(self.h, ptr(s), G * G, ptr(pan), ptr(core), P * G),
              "pg_kmer_compare_export")
        return s, pan, core

    def kmer_colors_time(self):
        """(ms_index, ms_colour, ms_compare, n_windows) of the last kmer_colors()
        (pg_kmer_colors_time)."""
        a, b, d, n = C.c_double(), C.c_double(), C.c_double(), C.c_uint64()
        check(self.lib.pg_kmer_colors_time(self.h, C.byref(a), C.byref(b), C.byref(d), C.byref(n)),
              "pg_kmer_colors_time")
        return a.value, b.value, d.value, n.value

    def kmer_colors_drop(self):
        """Release the colours and their comparison (pg_kmer_colors_drop)."""
        check(self.lib.pg_kmer_colors_drop(self.h), "pg_kmer_colors_drop")

    # ---------------------------------------------------- genome tree
    def tree_nj(self, dist=None, n=None) -> int:
        """The neighbour-joining tree (pg_tree_nj) of a host distance matrix
        uint64 [n, n] (symmetric, zero diagonal, entries <= 2^31), or, dist
        None, of the distances the device forms from the last freq_compare()'s
        shared matrix (n defaults to its genomes).  Returns the number of
        joins; the tree stays in the context (tree_dist / tree_joins /
        tree_root)."""
        if dist is None:
            d, n = None, int(getattr(self, "cmp_groups_n", 0) if n is None else n)
        else:
            d = np.ascontiguousarray(dist, dtype=np.uint64)
            n = int(d.shape[0] if n is None else n)
            if d.size < n * n or not d.size:
                d = np.concatenate([d.reshape(-1), np.zeros(1, np.uint64)])   # (never NULL; too large an n is refused unread)
        nj = C.c_uint64()
        check(self.lib.pg_tree_nj(self.h, ptr(d), n, C.byref(nj)), "pg_tree_nj")
        self.tree_n = n
        return nj.value

    def tree_dist(self) -> np.ndarray:
        """The distances the tree was built from, uint64 [n, n] (pg_tree_dist)."""
        n = getattr(self, "tree_n", 0)
        d = np.empty((n, n), np.uint64)
        check(self.lib.pg_tree_dist(self.h, ptr(d), n * n), "pg_tree_dist")
        return d

    def tree_joins(self) -> dict:
        """The joins in order: left, right (uint32 node ids; leaves 0 .. n - 1,
        join t makes node n + t), left_len, right_len (uint64, 16 fractional
        bits) (pg_tree_joins)."""
        J = max(getattr(self, "tree_n", 0) - 3, 0)
        t = {"left": np.empty(J, np.uint32), "right": np.empty(J, np.uint32),
             "left_len": np.empty(J, np.uint64), "right_len": np.empty(J, np.uint64)}
        check(self.lib.pg_tree_joins(self.h, *[ptr(a) for a in t.values()], J), "pg_tree_joins")
        return t

    def tree_root(self):
        """(child, len): the root's children (uint32, at most 3) and their
        lengths (uint64, 16 fractional bits) (pg_tree_root)."""
        nc, child, ln = C.c_uint32(), np.zeros(3, np.uint32), np.zeros(3, np.uint64)
        check(self.lib.pg_tree_root(self.h, C.byref(nc), ptr(child), ptr(ln)), "pg_tree_root")
        return child[:nc.value].copy(), ln[:nc.value].copy()

    def tree_time(self):
        """(ms, cells): the joins' time in the last tree_nj() and the sum of
        m^2 over them (pg_tree_time)."""
        ms, n = C.c_double(), C.c_uint64()
        check(self.lib.pg_tree_time(self.h, C.byref(ms), C.byref(n)), "pg_tree_time")
        return ms.value, n.value

    # ---------------------------------------------------- tree support
    def tree_bootstrap(self, n_reps: int, seed: int, bits=None, n_groups=None, rep_dist: bool = False):
        """Bootstrap support (pg_tree_bootstrap) for the joins of the last
        tree_nj() over the last freq()'s table where it lies on the device
        (bits None; n_groups defaults to the tree's leaves) or over host
        presence bits [L, W].  The support and the replicate joins stay in the
        context (tree_support / tree_bootstrap_joins).  rep_dist: return the
        replicate matrices, uint64 [n_reps, n, n] (for tests)."""
        G = int(getattr(self, "tree_n", 0) if n_groups is None else n_groups)
        b, L = None, 0
        if bits is not None:
            b = np.ascontiguousarray(bits, dtype=np.uint64)
            L = b.shape[0]
            b = b.reshape(L, (G + 63) // 64)
            if not b.size:
                b = np.zeros(1, np.uint64)           # (NULL would mean the device table)
        rd = np.zeros((int(n_reps), G, G), np.uint64) if rep_dist else None
        check(self.lib.pg_tree_bootstrap(self.h, ptr(b), L, G, int(n_reps), int(seed) & (2 ** 64 - 1),
                                         ptr(rd) if rd is not None and rd.size else None, 0 if rd is None else rd.size),
              "pg_tree_bootstrap")
        self.boot_reps_n, self.boot_joins_n = int(n_reps), max(G - 3, 0)
        return rd

    def tree_support(self):
        """(support uint32 [J], replicates): the replicates whose tree has
        each join's split (pg_tree_support)."""
        J = getattr(self, "boot_joins_n", 0)
        s, r = np.zeros(J, np.uint32), C.c_uint32()
        check(self.lib.pg_tree_support(self.h, ptr(s) if J else None, J, C.byref(r)), "pg_tree_support")
        return s, r.value

    def tree_bootstrap_joins(self):
        """(left, right), uint32 [R, J]: every replicate tree's joins
        (pg_tree_bootstrap_joins)."""
        R, J = getattr(self, "boot_reps_n", 0), getattr(self, "boot_joins_n", 0)
        a, b = np.zeros((R, J), np.uint32), np.zeros((R, J), np.uint32)
        check(self.lib.pg_tree_bootstrap_joins(self.h, ptr(a) if a.size else None, ptr(b) if b.size else None, R * J),
              "pg_tree_bootstrap_joins")
        return a, b

    def tree_bootstrap_time(self):
        """(ms_dist, ms_nj, ms_support, cells) of the last tree_bootstrap()
        (pg_tree_bootstrap_time)."""
        a, b, d, n = C.c_double(), C.c_double(), C.c_double(), C.c_uint64()
        check(self.lib.pg_tree_bootstrap_time(self.h, C.byref(a), C.byref(b), C.byref(d), C.byref(n)),
              "pg_tree_bootstrap_time")
        return a.value, b.value, d.value, n.value

    def tree_bootstrap_form(self):
        """(form, batches): which form of the neighbour joining the last
        tree_bootstrap() ran (1 LDS, 2 global scratch, 3 per-join launches, 0
        no join) and in how many batches (pg_tree_bootstrap_form)."""
        f, n = C.c_uint32(), C.c_uint32()
        check(self.lib.pg_tree_bootstrap_form(self.h, C.byref(f), C.byref(n)), "pg_tree_bootstrap_form")
        return f.value, n.value

    # ---------------------------------------------------- region graph
    def region_graph(self, rec_group, n_groups: int, rows=None):
        """The region graph (pg_region_graph) of the last row pass where it
        lies on the device (rows None) or of host rows [n, 5]; rec_group as
        freq() takes it.  Returns (n_nodes, n_links, n_paths, n_skipped); the
        graph stays on the device (region_nodes / region_links / region_paths
        / region_links_text / region_gfa_text and their _write forms)."""
        r5, n_rows, grp, n_records = _row_args(rec_group, rows)
        nn, nl, npth, ns = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(self.lib.pg_region_graph(self.h, ptr(r5), n_rows, ptr(grp), n_records, int(n_groups),
                                       C.byref(nn), C.byref(nl), C.byref(npth), C.byref(ns)), "pg_region_graph")
        self.n_region = (nn.value, nl.value, npth.value)
        return nn.value, nl.value, npth.value, ns.value

    def region_nodes(self) -> dict:
        """The nodes of the last region_graph(), labels ascending: labels,
        rows, max_len, n_out, n_in (pg_region_nodes)."""
        n = getattr(self, "n_region", (0, 0, 0))[0]
        t = {"labels": np.empty(n, np.int64), "rows": np.empty(n, np.uint64), "max_len": np.empty(n, np.uint64),
             "n_out": np.empty(n, np.uint32), "n_in": np.empty(n, np.uint32)}
        check(self.lib.pg_region_nodes(self.h, *[ptr(t[k]) for k in ("labels", "rows", "max_len", "n_out", "n_in")],
                                       n), "pg_region_nodes")
        return t

    def region_links(self) -> dict:
        """The links by (from, to) ascending: link_from, link_to, link_count,
        link_genomes (pg_region_links)."""
        n = getattr(self, "n_region", (0, 0, 0))[1]
        t = {"link_from": np.empty(n, np.int64), "link_to": np.empty(n, np.int64),
             "link_count": np.empty(n, np.uint64), "link_genomes": np.empty(n, np.uint32)}
        check(self.lib.pg_region_links(self.h, *[ptr(t[k]) for k in ("link_from", "link_to", "link_count",
                                                                      "link_genomes")], n), "pg_region_links")
        return t

    def region_paths(self) -> dict:
        """The paths in list order: path_record, path_strand, path_lo,
        path_hi, path_steps (pg_region_paths)."""
        n = getattr(self, "n_region", (0, 0, 0))[2]
        t = {k: np.empty(n, np.int64) for k in ("path_record", "path_strand", "path_lo", "path_hi")}
        t["path_steps"] = np.empty(n, np.uint64)
        check(self.lib.pg_region_paths(self.h, *[ptr(t[k]) for k in ("path_record", "path_strand", "path_lo",
                                                                      "path_hi", "path_steps")], n), "pg_region_paths")
        return t

    def region_links_text(self) -> bytes:
        """The links table's text, formatted on the device (pg_region_links_format)."""
        return _text(self.h, self.lib.pg_region_links_format, "pg_region_links_format")

    def region_links_write(self, fd: int) -> int:
        """region_links_text() written straight to descriptor fd at its
        position (pg_region_links_format_fd); flush any buffered writer on fd first."""
        return _write(self.h, self.lib.pg_region_links_format_fd, "pg_region_links_format_fd", fd)

    def region_gfa_text(self, names: list) -> bytes:
        """The graph as GFA 1, formatted on the device (pg_region_gfa);
        names[r] = record r's name in the path lines."""
        return _text(self.h, self.lib.pg_region_gfa, "pg_region_gfa", *_names_args(names))

    def region_gfa_write(self, names: list, fd: int) -> int:
        """region_gfa_text(names) written straight to descriptor fd at its
        position (pg_region_gfa_fd); flush any buffered writer on fd first."""
        return _write(self.h, self.lib.pg_region_gfa_fd, "pg_region_gfa_fd", fd, *_names_args(names))

    # ---------------------------------------------------- region sequences
    def region_seqs(self, rec_group, n_groups: int, rows=None):
        """One representative sequence per label (pg_region_seqs) of the last
        row pass where it lies on the device (rows None) or of host rows
        [n, 5], decoded from the context's parse; rec_group as region_graph()
        takes it.  Returns (n_regions, n_bases, n_skipped); the result stays
        on the device (region_seqs_table / region_seqs_bases /
        region_fasta_text / region_gfa_seq_text and their _write forms)."""
        r5, n_rows, grp, n_records = _row_args(rec_group, rows)
        nr, nb, ns = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(self.lib.pg_region_seqs(self.h, ptr(r5), n_rows, ptr(grp), n_records, int(n_groups),
                                      C.byref(nr), C.byref(nb), C.byref(ns)), "pg_region_seqs")
        self.n_region_seqs = nr.value
        return nr.value, nb.value, ns.value

    def region_seqs_table(self) -> dict:
        """The table of the last region_seqs(), labels ascending: label, row,
        record, start, end, strand (int64), len, gc, amb, offset (uint64)
        (pg_region_seqs_table)."""
        n = getattr(self, "n_region_seqs", 0)
        t = {k: np.empty(n, np.int64) for k in ("label", "row", "record", "start", "end", "strand")}
        t.update({k: np.empty(n, np.uint64) for k in ("len", "gc", "amb", "offset")})
        check(self.lib.pg_region_seqs_table(self.h, *[ptr(a) for a in t.values()], n), "pg_region_seqs_table")
        return t

    def region_seqs_bases(self) -> bytes:
        """The sequences one after another in table order, no separators
        (pg_region_seqs_bases)."""
        return _text(self.h, self.lib.pg_region_seqs_bases, "pg_region_seqs_bases")

    def region_seqs_time(self):
        """(ms, chunks): the decoder kernel's time in the last region_seqs()
        and the 16-letter chunks it wrote (pg_region_seqs_time)."""
        ms, n = C.c_double(), C.c_uint64()
        check(self.lib.pg_region_seqs_time(self.h, C.byref(ms), C.byref(n)), "pg_region_seqs_time")
        return ms.value, n.value

    def region_fasta_text(self, names: list) -> bytes:
        """The sequences as FASTA, formatted on the device (pg_region_fasta);
        names[r] = record r's name in the header lines."""
        return _text(self.h, self.lib.pg_region_fasta, "pg_region_fasta", *_names_args(names))

    def region_fasta_write(self, names: list, fd: int) -> int:
        """region_fasta_text(names) written straight to descriptor fd at its
        position (pg_region_fasta_fd); flush any buffered writer on fd first."""
        return _write(self.h, self.lib.pg_region_fasta_fd, "pg_region_fasta_fd", fd, *_names_args(names))

    def region_gfa_seq_text(self, names: list) -> bytes:
        """region_gfa_text(names) with every S line carrying its sequence
        (pg_region_gfa_seq): needs region_graph() and region_seqs() of the
        same rows and groups."""
        return _text(self.h, self.lib.pg_region_gfa_seq, "pg_region_gfa_seq", *_names_args(names))

    def region_gfa_seq_write(self, names: list, fd: int) -> int:
        """region_gfa_seq_text(names) written straight to descriptor fd at its
        position (pg_region_gfa_seq_fd); flush any buffered writer on fd first."""
        return _write(self.h, self.lib.pg_region_gfa_seq_fd, "pg_region_gfa_seq_fd", fd, *_names_args(names))

    # ---------------------------------------------------- variable sites
    def region_sites(self, rec_group, n_groups: int, rows=None):
        """The variable sites (pg_region_sites) of the last row pass where it
        lies on the device (rows None) or of host rows [n, 5]; rec_group as
        region_graph() takes it.  Returns (n_sites, n_alleles, n_records,
        n_skipped); the result stays on the device (region_sites_table /
        region_sites_alleles / region_sites_groups / region_sites_text and
        region_sites_write)."""
        r5, n_rows, grp, n_records = _row_args(rec_group, rows)
        ns, na, nr, nk = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(self.lib.pg_region_sites(self.h, ptr(r5), n_rows, ptr(grp), n_records, int(n_groups),
                                       C.byref(ns), C.byref(na), C.byref(nr), C.byref(nk)), "pg_region_sites")
        self.n_sites = (ns.value, na.value, int(n_groups))
        return ns.value, na.value, nr.value, nk.value

    def region_sites_table(self) -> dict:
        """The sites of the last region_sites() by (from, to) ascending:
        site_from, site_to, site_alleles, site_first, site_count,
        site_genomes (pg_region_sites_table)."""
        n = getattr(self, "n_sites", (0, 0, 0))[0]
        t = {"site_from": np.empty(n, np.int64), "site_to": np.empty(n, np.int64),
             "site_alleles": np.empty(n, np.uint32), "site_first": np.empty(n, np.uint64),
             "site_count": np.empty(n, np.uint64), "site_genomes": np.empty(n, np.uint32)}
        check(self.lib.pg_region_sites_table(self.h, *[ptr(a) for a in t.values()], n), "pg_region_sites_table")
        return t

    def region_sites_alleles(self) -> dict:
        """The alleles by (from, to, via) ascending: allele_site, allele_via
        (-1: the direct join), allele_count, allele_genomes, allele_min,
        allele_max and bits, uint64 [n, W] (pg_region_sites_alleles)."""
        _, n, G = getattr(self, "n_sites", (0, 0, 0))
        t = {"allele_site": np.empty(n, np.uint64), "allele_via": np.empty(n, np.int64),
             "allele_count": np.empty(n, np.uint64), "allele_genomes": np.empty(n, np.uint32),
             "allele_min": np.empty(n, np.uint64), "allele_max": np.empty(n, np.uint64),
             "bits": np.empty((n, (G + 63) // 64), np.uint64)}
        check(self.lib.pg_region_sites_alleles(self.h, *[ptr(a) for a in t.values()], n), "pg_region_sites_alleles")
        return t

    def region_sites_groups(self) -> dict:
        """Per genome: genome_sites, genome_alleles, genome_private
        (pg_region_sites_groups)."""
        G = getattr(self, "n_sites", (0, 0, 0))[2]
        t = {k: np.empty(G, np.uint64) for k in ("genome_sites", "genome_alleles", "genome_private")}
        check(self.lib.pg_region_sites_groups(self.h, *[ptr(a) for a in t.values()], G), "pg_region_sites_groups")
        return t

    def region_sites_text(self) -> bytes:
        """The alleles table's text, formatted on the device (pg_region_sites_format)."""
        return _text(self.h, self.lib.pg_region_sites_format, "pg_region_sites_format")

    def region_sites_write(self, fd: int) -> int:
        """region_sites_text() written straight to descriptor fd at its
        position (pg_region_sites_format_fd); flush any buffered writer on fd first."""
        return _write(self.h, self.lib.pg_region_sites_format_fd, "pg_region_sites_format_fd", fd)

    # ---------------------------------------------------- variable sites between anchors
    def region_bubbles(self, rec_group, n_groups: int, min_genomes: int, rows=None):
        """The variable sites between anchor regions (pg_region_bubbles) of
        the last row pass where it lies on the device (rows None) or of host
        rows [n, 5]; rec_group as region_graph() takes it; an anchor is a
        label carried by min_genomes genomes or more.  Returns (n_anchors,
        n_segments, n_sites, n_alleles, n_skipped); the result stays on the
        device (region_bubbles_table / _alleles / _inner / _groups /
        _anchors / _text and region_bubbles_write)."""
        r5, n_rows, grp, n_records = _row_args(rec_group, rows)
        if not 0 <= int(min_genomes) < 2 ** 32:
            raise ValueError("min_genomes = %d does not fit the call's unsigned 32 bits" % int(min_genomes))
        out = [C.c_uint64() for _ in range(5)]
        check(self.lib.pg_region_bubbles(self.h, ptr(r5), n_rows, ptr(grp), n_records, int(n_groups), int(min_genomes),
                                         *[C.byref(x) for x in out]), "pg_region_bubbles")
        self.n_bubbles = (out[2].value, out[3].value, int(n_groups), out[0].value)
        return tuple(x.value for x in out)

    def region_bubbles_table(self) -> dict:
        """The sites of the last region_bubbles() by (from, to) ascending:
        site_from, site_to, site_alleles, site_first, site_count,
        site_genomes (pg_region_bubbles_table)."""
        n = getattr(self, "n_bubbles", (0, 0, 0, 0))[0]
        t = {"site_from": np.empty(n, np.int64), "site_to": np.empty(n, np.int64),
             "site_alleles": np.empty(n, np.uint32), "site_first": np.empty(n, np.uint64),
             "site_count": np.empty(n, np.uint64), "site_genomes": np.empty(n, np.uint32)}
        check(self.lib.pg_region_bubbles_table(self.h, *[ptr(a) for a in t.values()], n), "pg_region_bubbles_table")
        return t

    def region_bubbles_alleles(self) -> dict:
        """The alleles by site and, inside a site, by first row: allele_site,
        allele_regions, allele_first_row, allele_count, allele_genomes,
        allele_min_bp, allele_max_bp, allele_inner_off and bits, uint64
        [n, W] (pg_region_bubbles_alleles)."""
        _, n, G, _ = getattr(self, "n_bubbles", (0, 0, 0, 0))
        t = {"allele_site": np.empty(n, np.uint64), "allele_regions": np.empty(n, np.uint64),
             "allele_first_row": np.empty(n, np.uint64), "allele_count": np.empty(n, np.uint64),
             "allele_genomes": np.empty(n, np.uint32), "allele_min_bp": np.empty(n, np.uint64),
             "allele_max_bp": np.empty(n, np.uint64), "allele_inner_off": np.empty(n, np.uint64),
             "bits": np.empty((n, (G + 63) // 64), np.uint64)}
        check(self.lib.pg_region_bubbles_alleles(self.h, *[ptr(a) for a in t.values()], n),
              "pg_region_bubbles_alleles")
        return t

    def region_bubbles_inner(self) -> np.ndarray:
        """The alleles' inner paths one after another in table order, int64
        (pg_region_bubbles_inner); allele i's is inner[allele_inner_off[i]:][:allele_regions[i]]."""
        n = C.c_uint64()
        check(self.lib.pg_region_bubbles_inner(self.h, None, 0, C.byref(n)), "pg_region_bubbles_inner")
        out = np.empty(n.value, np.int64)
        if n.value:
            check(self.lib.pg_region_bubbles_inner(self.h, ptr(out), n.value, C.byref(n)), "pg_region_bubbles_inner")
        return out

    def region_bubbles_groups(self) -> dict:
        """Per genome: genome_sites, genome_alleles, genome_private
        (pg_region_bubbles_groups)."""
        G = getattr(self, "n_bubbles", (0, 0, 0, 0))[2]
        t = {k: np.empty(G, np.uint64) for k in ("genome_sites", "genome_alleles", "genome_private")}
        check(self.lib.pg_region_bubbles_groups(self.h, *[ptr(a) for a in t.values()], G), "pg_region_bubbles_groups")
        return t

    def region_bubbles_anchors(self) -> dict:
        """The anchors, labels ascending: anchors, anchor_genomes
        (pg_region_bubbles_anchors)."""
        n = getattr(self, "n_bubbles", (0, 0, 0, 0))[3]
        t = {"anchors": np.empty(n, np.int64), "anchor_genomes": np.empty(n, np.uint32)}
        check(self.lib.pg_region_bubbles_anchors(self.h, ptr(t["anchors"]), ptr(t["anchor_genomes"]), n),
              "pg_region_bubbles_anchors")
        return t

    def region_bubbles_text(self) -> bytes:
        """The alleles table's text, formatted on the device (pg_region_bubbles_format)."""
        return _text(self.h, self.lib.pg_region_bubbles_format, "pg_region_bubbles_format")

    def region_bubbles_write(self, fd: int) -> int:
        """region_bubbles_text() written straight to descriptor fd at its
        position (pg_region_bubbles_format_fd); flush any buffered writer on fd first."""
        return _write(self.h, self.lib.pg_region_bubbles_format_fd, "pg_region_bubbles_format_fd", fd)

    # ---------------------------------------------------- the bubbles' alleles as sequences, the VCF
    NO_REF = 2 ** 32 - 1

    def region_variants(self, rec_group, n_groups: int, ref_group=None, rows=None):
        """The bases of every allele of the last region_bubbles() and the
        sites placed on the walks of genome ref_group (None: PG_NO_REF, no
        site is placed) (pg_region_variants); rows and rec_group must be the
        ones region_bubbles() took.  Returns (n_alleles, n_bases, n_placed,
        n_unplaced); the result stays on the device (region_variants_alleles
        / _bases / _placed, region_alleles_fasta_text, region_vcf_text and
        their _write forms) until the next region_bubbles()."""
        r5, n_rows, grp, n_records = _row_args(rec_group, rows)
        ref = self.NO_REF if ref_group is None else int(ref_group)
        if not 0 <= ref < 2 ** 32:
            raise ValueError("ref_group = %d does not fit the call's unsigned 32 bits" % ref)
        out = [C.c_uint64() for _ in range(4)]
        check(self.lib.pg_region_variants(self.h, ptr(r5), n_rows, ptr(grp), n_records, int(n_groups), ref,
                                          *[C.byref(x) for x in out]), "pg_region_variants")
        self.n_variants = (out[0].value, out[2].value)
        return tuple(x.value for x in out)

    def region_variants_alleles(self) -> dict:
        """The allele table in the bubbles alleles' order: record, lo, hi,
        strand (int64), len, gc, amb, offset (uint64) (pg_region_variants_alleles)."""
        n = getattr(self, "n_variants", (0, 0))[0]
        t = {k: np.empty(n, np.int64) for k in ("record", "lo", "hi", "strand")}
        t.update({k: np.empty(n, np.uint64) for k in ("len", "gc", "amb", "offset")})
        check(self.lib.pg_region_variants_alleles(self.h, *[ptr(a) for a in t.values()], n),
              "pg_region_variants_alleles")
        return t

    def region_variants_bases(self) -> bytes:
        """The alleles' sequences one after another in table order, no
        separators (pg_region_variants_bases)."""
        return _text(self.h, self.lib.pg_region_variants_bases, "pg_region_variants_bases")

    def region_variants_placed(self) -> dict:
        """The placed sites by (record, pos0, site) ascending: site, record,
        pos0, ref_row, ref_allele, ref_len (pg_region_variants_placed)."""
        n = getattr(self, "n_variants", (0, 0))[1]
        t = {"site": np.empty(n, np.uint64), "record": np.empty(n, np.int64), "pos0": np.empty(n, np.int64),
             "ref_row": np.empty(n, np.uint64), "ref_allele": np.empty(n, np.uint32),
             "ref_len": np.empty(n, np.uint64)}
        check(self.lib.pg_region_variants_placed(self.h, *[ptr(a) for a in t.values()], n),
              "pg_region_variants_placed")
        return t

    def region_variants_time(self):
        """(ms, chunks): the decoder kernel's time in the last
        region_variants() and the 16-letter chunks it wrote (pg_region_variants_time)."""
        ms, n = C.c_double(), C.c_uint64()
        check(self.lib.pg_region_variants_time(self.h, C.byref(ms), C.byref(n)), "pg_region_variants_time")
        return ms.value, n.value

    def region_alleles_fasta_text(self, names: list) -> bytes:
        """The alleles as FASTA, formatted on the device
        (pg_region_alleles_fasta); names[r] = record r's name."""
        return _text(self.h, self.lib.pg_region_alleles_fasta, "pg_region_alleles_fasta", *_names_args(names))

    def region_alleles_fasta_write(self, names: list, fd: int) -> int:
        """region_alleles_fasta_text(names) written straight to descriptor fd
        at its position (pg_region_alleles_fasta_fd); flush any buffered writer on fd first."""
        return _write(self.h, self.lib.pg_region_alleles_fasta_fd, "pg_region_alleles_fasta_fd", fd,
                      *_names_args(names))

    def region_vcf_text(self, names: list) -> bytes:
        """The VCF body, one line per placed site, formatted on the device
        (pg_region_vcf); names[r] = record r's name, the CHROM column."""
        return _text(self.h, self.lib.pg_region_vcf, "pg_region_vcf", *_names_args(names))

    def region_vcf_write(self, names: list, fd: int) -> int:
        """region_vcf_text(names) written straight to descriptor fd at its
        position (pg_region_vcf_fd); flush any buffered writer on fd first."""
        return _write(self.h, self.lib.pg_region_vcf_fd, "pg_region_vcf_fd", fd, *_names_args(names))

    ALIGN_PAIR_COLS = ("site", "allele", "placed", "t_len", "q_len", "prefix", "suffix", "status", "distance", "n_eq",
                       "n_sub", "n_ins", "n_del", "op_off", "n_ops", "prim_off", "n_prims")

    def region_align(self):
        """Every allele of the last region_variants() aligned against its
        site's reference - a placed site's REF, else the site's allele 0
        (pg_region_align).  Returns (n_pairs, n_aligned, n_ops, n_prims,
        n_lines); the result stays on the device (region_align_pairs / _ops /
        _prims / _lines, region_align_text, region_primitives_vcf_text and
        their _write forms) until the next region_variants() or
        region_bubbles()."""
        out = [C.c_uint64() for _ in range(5)]
        check(self.lib.pg_region_align(self.h, *[C.byref(x) for x in out]), "pg_region_align")
        self.n_align = tuple(x.value for x in out)
        return self.n_align

    def region_align_pairs(self) -> dict:
        """The pair table, every column uint64: ALIGN_PAIR_COLS (pg_region_align_pairs)."""
        n = getattr(self, "n_align", (0,) * 5)[0]
        t = {k: np.empty(n, np.uint64) for k in self.ALIGN_PAIR_COLS}
        check(self.lib.pg_region_align_pairs(self.h, *[ptr(a) for a in t.values()], n), "pg_region_align_pairs")
        return t

    def region_align_ops(self) -> dict:
        """The runs of every pair one after another: op (uint8, one of
        b"=XDI") and len (uint64) (pg_region_align_ops)."""
        n = getattr(self, "n_align", (0,) * 5)[2]
        t = {"op": np.empty(n, np.uint8), "len": np.empty(n, np.uint64)}
        check(self.lib.pg_region_align_ops(self.h, ptr(t["op"]), ptr(t["len"]), n), "pg_region_align_ops")
        return t

    def region_align_prims(self) -> dict:
        """The primitives: pair, type (uint8: 0 SNV, 1 DEL, 2 INS, 3 REPL),
        tpos, qpos, tlen, qlen (pg_region_align_prims)."""
        n = getattr(self, "n_align", (0,) * 5)[3]
        t = {k: np.empty(n, np.uint8 if k == "type" else np.uint64)
             for k in ("pair", "type", "tpos", "qpos", "tlen", "qlen")}
        check(self.lib.pg_region_align_prims(self.h, *[ptr(a) for a in t.values()], n), "pg_region_align_prims")
        return t

    def region_align_lines(self, n_groups: int) -> dict:
        """The merged lines of the placed sites in the VCF's order: site, pos
        (int64), type (uint8), tpos, tlen, qlen, first_prim, ac, n_genomes
        (uint32) and bits, uint64 [lines, ceil(n_groups / 64)] (pg_region_align_lines)."""
        n = getattr(self, "n_align", (0,) * 5)[4]
        t = {k: np.empty(n, np.uint64) for k in ("site", "pos", "type", "tpos", "tlen", "qlen", "first_prim", "ac")}
        t["pos"], t["type"] = np.empty(n, np.int64), np.empty(n, np.uint8)
        t["n_genomes"] = np.empty(n, np.uint32)
        t["bits"] = np.empty((n, (int(n_groups) + 63) // 64), np.uint64)
        check(self.lib.pg_region_align_lines(self.h, *[ptr(a) for a in t.values()], n), "pg_region_align_lines")
        return t

    def region_align_time(self):
        """(ms, cells): the fill kernels' time in the last region_align() and
        the cells they computed (pg_region_align_time)."""
        ms, n = C.c_double(), C.c_uint64()
        check(self.lib.pg_region_align_time(self.h, C.byref(ms), C.byref(n)), "pg_region_align_time")
        return ms.value, n.value

    def region_align_band(self):
        """(n_over, n_banded, n_attempts, band_cells, ms): the band form's part
        of the last region_align() - the pairs above the cells cap, those of
        them that came out aligned, the attempts, their band cells and the band
        fills' time; zeros with PG_TUNE_ALIGN_BAND 0 (pg_region_align_band)."""
        out, ms = [C.c_uint64() for _ in range(4)], C.c_double()
        check(self.lib.pg_region_align_band(self.h, *[C.byref(x) for x in out], C.byref(ms)), "pg_region_align_band")
        return tuple(x.value for x in out) + (ms.value,)

    def region_align_text(self) -> bytes:
        """The pair table's text, formatted on the device (pg_region_align_format)."""
        return _text(self.h, self.lib.pg_region_align_format, "pg_region_align_format")

    def region_align_write(self, fd: int) -> int:
        """region_align_text() written straight to descriptor fd at its
        position (pg_region_align_format_fd); flush any buffered writer on fd first."""
        return _write(self.h, self.lib.pg_region_align_format_fd, "pg_region_align_format_fd", fd)

    def region_primitives_vcf_text(self, names: list) -> bytes:
        """The primitives' VCF body, one line per merged primitive, formatted
        on the device (pg_region_primitives_vcf); names[r] = record r's name."""
        return _text(self.h, self.lib.pg_region_primitives_vcf, "pg_region_primitives_vcf", *_names_args(names))

    def region_primitives_vcf_write(self, names: list, fd: int) -> int:
        """region_primitives_vcf_text(names) written straight to descriptor fd
        at its position (pg_region_primitives_vcf_fd); flush any buffered writer on fd first."""
        return _write(self.h, self.lib.pg_region_primitives_vcf_fd, "pg_region_primitives_vcf_fd", fd,
                      *_names_args(names))

    def rows_export(self, n: int):
        """The [n, 5] rows of the last rows_count() (pg_rows_export)."""
        out = np.empty((int(n), 5), np.int64)
        if n:
            check(self.lib.pg_rows_export(self.h, ptr(out), int(n)), "pg_rows_export")
        return out


# ------------------------------------------------------------------ text output
def format_xyz(tuples: np.ndarray, counts: np.ndarray) -> bytes:
    """The `.xyz` side file's text (kmer_numba.py:1901), formatted natively."""
    lib = load()
    t = np.ascontiguousarray(tuples, dtype=np.uint64)
    c = np.ascontiguousarray(counts, dtype=np.int64)
    n = c.shape[0]
    cap = lib.pg_format_xyz(None, None, n, None, 0)
    buf = np.empty(max(cap, 1), np.uint8)
    m = lib.pg_format_xyz(ptr(t), ptr(c), n, ptr(buf), cap)
    if n and not m:
        raise PangenomeError("pg_format_xyz: buffer too small")
    return buf[:m].tobytes()


def format_rows(rows: np.ndarray, names: list) -> bytes:
    """The region rows (:1947-1949) for records named names[r], natively."""
    lib = load()
    r5 = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 5)
    blob = b"".join(names)
    off = np.zeros(len(names) + 1, np.int64)
    if names:
        off[1:] = np.cumsum([len(x) for x in names])
    nb = np.frombuffer(blob, np.uint8) if blob else np.zeros(1, np.uint8)
    n = r5.shape[0]
    cap = lib.pg_format_rows(ptr(r5), n, ptr(nb), ptr(off), None, 0)
    buf = np.empty(max(cap, 1), np.uint8)
    m = lib.pg_format_rows(ptr(r5), n, ptr(nb), ptr(off), ptr(buf), cap)
    if n and not m:
        raise PangenomeError("pg_format_rows: buffer too small")
    return buf[:m].tobytes()
