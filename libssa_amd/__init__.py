"""libssa_amd -- MI355X-native optimal-alignment database search.

Python mirror of the C ABI in ``include/libssa.h`` / ``include/libssa_amd.h``
(the reference's public API, ``src/libssa.h:122-263``), loaded with ctypes
from the in-tree ``libssa_amd/lib/libssa_amd.so``.  Function names, argument
meaning and error behaviour are the reference's: configuration errors end the
process with status 1 (``fatal``), query-file errors return ``None``.

The library itself holds no Python: the scoring runs in the gfx950 kernels
of ``csrc/kernels.hip``; there is no CPU fallback, and loading fails loudly
when the shared library has not been built (``python -m libssa_amd.build``).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_int, c_int8, c_long, c_size_t, c_uint8, \
    c_uint32, c_uint64, c_int64, c_int32, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(HERE, "lib")
# SSA_AMD_LIB: an alternative build of the library (A/B measurements only)
LIB_PATH = os.environ.get("SSA_AMD_LIB") or os.path.join(LIB_DIR, "libssa_amd.so")
DB_LIB_PATH = os.path.join(LIB_DIR, "libssa_fasta_db.so")

# ---- constants (libssa.h) ---------------------------------------------------
BLOSUM45, BLOSUM50, BLOSUM62, BLOSUM80, BLOSUM90 = "blosum45", "blosum50", "blosum62", "blosum80", "blosum90"
PAM30, PAM70, PAM250 = "pam30", "pam70", "pam250"
NUCLEOTIDE, AMINOACID, TRANS_QUERY, TRANS_DB, TRANS_BOTH = 0, 1, 2, 3, 4
FORWARD_STRAND, COMPLEMENTARY_STRAND, BOTH_STRANDS = 1, 2, 3
BIT_WIDTH_8, BIT_WIDTH_16, BIT_WIDTH_64 = 8, 16, 64
OUTPUT_SILENT, OUTPUT_ERROR, OUTPUT_WARNING, OUTPUT_INFO = 0, 1, 2, 3
COMPUTE_SCORE, COMPUTE_ALIGNMENT = 0, 1
READ_FROM_FILE, READ_FROM_STRING, MATRIX_BUILDIN = 0, 1, 2
COMPUTE_ON_SSE2, COMPUTE_ON_SSE41, COMPUTE_ON_AVX2 = 0, 1, 2
SW, NW = 0, 1
TOPK, LOG = 0, 1


class db_seq_t(Structure):
    _fields_ = [("seq", c_void_p), ("len", c_size_t), ("ID", c_size_t), ("strand", c_int), ("frame", c_int)]


class q_seq_t(Structure):
    _fields_ = [("seq", c_void_p), ("len", c_size_t), ("strand", c_int), ("frame", c_int)]


class alignment_t(Structure):
    _fields_ = [("db_seq", db_seq_t), ("query", q_seq_t), ("alignment", c_char_p), ("alignment_len", c_size_t),
                ("score", c_long), ("align_q_start", c_size_t), ("align_q_end", c_size_t),
                ("align_d_start", c_size_t), ("align_d_end", c_size_t)]


class alignment_list_t(Structure):
    _fields_ = [("alignments", POINTER(POINTER(alignment_t))), ("len", c_size_t)]


class ssa_hit_t(Structure):
    _fields_ = [("score", c_int64), ("db_id", c_uint64), ("query_id", c_uint8), ("db_strand", c_uint8),
                ("db_frame", c_uint8), ("pad", c_uint8 * 5)]


class ssa_amd_stats_t(Structure):
    _fields_ = [("search_ms", c_double), ("kernel_ms", c_double), ("wide_ms", c_double), ("d2h_ms", c_double),
                ("replay_ms", c_double), ("pack_ms", c_double), ("cells", c_uint64), ("entries", c_uint64),
                ("overflow_8", c_uint64), ("overflow_16", c_uint64), ("wide_count", c_uint64),
                ("kernel_launches", c_uint32), ("device", c_int32), ("kernel_bytes", c_uint64),
                ("kernel", ctypes.c_char * 32), ("prep_ms", c_double), ("upload_ms", c_double),
                ("sync_wait_ms", c_double), ("strip_rows", c_uint32), ("counters", c_uint32),
                ("long_entries", c_uint32), ("long_kernel", ctypes.c_char * 24), ("part_retries", c_uint32),
                ("total_searches", c_uint64), ("total_kernel_ms", c_double), ("total_search_ms", c_double),
                ("filter_candidates", c_uint64), ("gather_ms", c_double), ("gather_rounds", c_uint32),
                ("rare_merged", c_uint32), ("rare_rescored", c_uint32), ("slots", c_uint32),
                ("slot_device", ctypes.c_int32 * 16), ("slot_kernel_ms", c_double * 16),
                ("slot_search_ms", c_double * 16), ("part_units", c_uint32), ("pruned_units", c_uint32),
                ("inplace_units", c_uint32), ("pruned_first", c_uint32)]


class ssa_amd_pairs_stats_t(Structure):
    _fields_ = [("pairs", c_uint64), ("cells", c_uint64), ("swept_cells", c_uint64), ("host_pairs", c_uint64),
                ("groups", c_uint32), ("chunks", c_uint32), ("launches", c_uint32), ("strip_rows", c_uint32),
                ("total_ms", c_double), ("pack_ms", c_double), ("kernel_ms", c_double), ("host_ms", c_double),
                ("device", c_int32), ("kernel", ctypes.c_char * 32), ("gather_ms", c_double),
                ("pool_bytes", c_uint64)]


class ssa_amd_pair_alignment_t(Structure):
    _fields_ = [("score", c_int64), ("region", c_uint64 * 4), ("cigar_off", c_uint64), ("cigar_len", c_uint32),
                ("flags", c_uint32)]


class ssa_amd_pair_summary_t(Structure):
    _fields_ = [("score", c_int64), ("region", c_uint64 * 4), ("columns", c_uint32), ("matched", c_uint32),
                ("identical", c_uint32), ("flags", c_uint32)]


class ssa_amd_align_pairs_stats_t(Structure):
    _fields_ = [("pairs", c_uint64), ("cells", c_uint64), ("host_pairs", c_uint64), ("zero_pairs", c_uint64),
                ("device_fallbacks", c_uint64), ("dir_bytes", c_uint64), ("groups", c_uint32), ("chunks", c_uint32),
                ("launches", c_uint32), ("reserved", c_uint32), ("total_ms", c_double), ("pack_ms", c_double),
                ("host_ms", c_double), ("text_ms", c_double), ("fwd_ms", c_double), ("rev_ms", c_double),
                ("dir_ms", c_double), ("walk_ms", c_double), ("kernel_ms", c_double), ("device", c_int32),
                ("kernels", ctypes.c_char * 96)]


assert ctypes.sizeof(db_seq_t) == 32 and ctypes.sizeof(q_seq_t) == 24
assert ctypes.sizeof(alignment_t) == 112 and ctypes.sizeof(alignment_list_t) == 16
assert ctypes.sizeof(ssa_hit_t) == 24 and ctypes.sizeof(ssa_amd_pair_alignment_t) == 56
assert ctypes.sizeof(ssa_amd_pair_summary_t) == 56


class ssa_amd_hits_stats_t(Structure):
    _fields_ = [("hits", c_uint64), ("gathered", c_uint64), ("fetched", c_uint64), ("upload_bytes", c_uint64),
                ("gather_ms", c_double)]

# every symbol include/*.h declares (checked by tests/test_abi.py)
EXPORTS = {
    "libssa_amd.so": ["set_output_mode", "set_simd_compute_mode", "set_chunk_size", "set_thread_count",
                      "init_score_matrix", "init_constant_scores", "init_gap_penalties", "init_symbol_translation",
                      "init_db", "init_sequence_fasta", "free_sequence", "sw_align", "nw_align", "free_alignment",
                      "ssa_exit", "ssa_amd_device_count", "ssa_amd_set_device", "ssa_amd_set_id_offset",
                      "ssa_amd_prepare_db", "ssa_amd_get_stats", "ssa_amd_set_option", "ssa_amd_search",
                      "ssa_amd_replay", "ssa_amd_query_views", "ssa_amd_translate", "ssa_amd_align_pair",
                      "ssa_amd_save_db", "ssa_amd_load_db", "ssa_amd_set_devices", "ssa_amd_search_batch",
                      "ssa_amd_dist_unique_id", "ssa_amd_dist_unique_id_bytes", "ssa_amd_dist_init",
                      "ssa_amd_dist_finalize", "ssa_amd_gather_logs", "ssa_amd_merge_logs", "ssa_amd_get_timeline",
                      "ssa_amd_dist_available", "ssa_amd_dist_init_fake", "ssa_amd_dist_ranks", "ssa_amd_shard_bounds",
                      "ssa_amd_get_devices", "ssa_amd_score_pairs", "ssa_amd_get_pairs_stats",
                      "ssa_amd_map_residues", "ssa_amd_align_pairs", "ssa_amd_get_align_pairs_stats",
                      "ssa_amd_score_pairs_ends", "ssa_amd_align_pairs_ends",
                      "ssa_amd_score_pairs_banded", "ssa_amd_align_pairs_banded",
                      "ssa_amd_score_pairs_local", "ssa_amd_align_pairs_local", "ssa_amd_score_pairs_indexed",
                      "ssa_amd_prune_start_order", "ssa_amd_get_pruned_whole", "ssa_amd_get_promoted_lanes",
                      "ssa_amd_align_hits",
                      "ssa_amd_get_align_hits_stats", "ssa_amd_summarize_pairs_local",
                      "ssa_amd_score_pairs_xdrop", "ssa_amd_align_pairs_xdrop", "ssa_amd_summarize_pairs_xdrop",
                      "ssa_amd_get_xdrop_dropped", "ssa_amd_search_above", "ssa_amd_merge_above",
                      "ssa_amd_summarize_hits", "ssa_amd_get_summarize_hits_stats",
                      "ssa_amd_profile_create", "ssa_amd_profile_from_query", "ssa_amd_profile_rows",
                      "ssa_amd_profile_free", "ssa_amd_profile_score_host", "ssa_amd_search_profile",
                      "ssa_amd_search_profile_above", "ssa_amd_get_upload_bytes"],
    "libssa_fasta_db.so": ["ssa_db_init", "ssa_db_get_sequence_count", "ssa_db_get_sequence", "ssa_db_close"],
}

_lib = None


def load():
    """Loads the in-tree shared library (fails loudly if it is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"libssa_amd native library not built: {LIB_PATH} missing "
                           "(run `python -m libssa_amd.build`)")
    ctypes.CDLL(DB_LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    P = c_void_p
    sig = {
        "set_output_mode": ([c_int], None), "set_simd_compute_mode": ([c_int], None),
        "set_chunk_size": ([c_size_t], None), "set_thread_count": ([c_size_t], None),
        "init_score_matrix": ([c_int, c_char_p], None), "init_constant_scores": ([c_int8, c_int8], None),
        "init_gap_penalties": ([c_int8, c_int8], None), "init_symbol_translation": ([c_int] * 4, None),
        "init_db": ([c_char_p], None), "init_sequence_fasta": ([c_int, c_char_p], P),
        "free_sequence": ([P], None),
        "sw_align": ([P, c_size_t, c_int, c_int], POINTER(alignment_list_t)),
        "nw_align": ([P, c_size_t, c_int, c_int], POINTER(alignment_list_t)),
        "free_alignment": ([POINTER(alignment_list_t)], None), "ssa_exit": ([], None),
        "ssa_amd_device_count": ([], c_int), "ssa_amd_set_device": ([c_int], None),
        "ssa_amd_set_id_offset": ([c_size_t], None), "ssa_amd_prepare_db": ([], c_int),
        "ssa_amd_get_stats": ([POINTER(ssa_amd_stats_t)], None), "ssa_amd_set_option": ([c_char_p, c_long], None),
        "ssa_amd_search": ([P, c_int, c_size_t, c_int, c_int, POINTER(ssa_hit_t), c_size_t], c_size_t),
        "ssa_amd_replay": ([POINTER(ssa_hit_t), c_size_t, c_size_t, POINTER(ssa_hit_t)], c_size_t),
        "ssa_amd_search_above": ([P, c_int, c_int64, c_int, POINTER(ssa_hit_t), c_size_t, POINTER(c_size_t)],
                                 c_size_t),
        "ssa_amd_merge_above": ([POINTER(ssa_hit_t), c_size_t, c_int64, POINTER(ssa_hit_t), c_size_t,
                                 POINTER(c_size_t)], c_size_t),
        "ssa_amd_query_views": ([P, POINTER(q_seq_t), c_size_t], c_size_t),
        "ssa_amd_save_db": ([c_char_p], c_int), "ssa_amd_load_db": ([c_char_p], c_int),
        "ssa_amd_set_devices": ([POINTER(c_int), c_int], c_int),
        "ssa_amd_get_devices": ([POINTER(c_int), c_int], c_int),
        "ssa_amd_search_batch": ([POINTER(c_void_p), c_size_t, c_int, c_size_t, c_int, POINTER(ssa_hit_t),
                                  POINTER(c_size_t)], c_size_t),
        "ssa_amd_align_pair": ([c_int, c_char_p, c_size_t, c_char_p, c_size_t, POINTER(c_size_t), c_char_p, c_size_t],
                               c_size_t),
        "ssa_amd_translate": ([c_int, c_char_p, c_size_t, c_int, c_int, c_char_p, c_size_t], c_size_t),
        "ssa_amd_dist_unique_id": ([c_char_p], c_int), "ssa_amd_dist_unique_id_bytes": ([], c_size_t),
        "ssa_amd_dist_init": ([c_int, c_int, c_char_p], c_int), "ssa_amd_dist_finalize": ([], None),
        "ssa_amd_gather_logs": ([POINTER(ssa_hit_t), c_size_t, c_size_t, POINTER(ssa_hit_t)], c_size_t),
        "ssa_amd_merge_logs": ([POINTER(ssa_hit_t), POINTER(c_size_t), c_size_t, c_size_t, c_size_t,
                                POINTER(ssa_hit_t)], c_size_t),
        "ssa_amd_get_timeline": ([c_void_p, c_size_t], c_size_t),
        "ssa_amd_get_pruned_whole": ([], ctypes.c_uint32),
        "ssa_amd_get_promoted_lanes": ([], ctypes.c_uint32),
        "ssa_amd_prune_start_order": ([c_void_p, c_size_t, c_size_t, ctypes.c_uint, ctypes.c_uint, c_void_p, c_size_t],
                                      c_size_t),
        "ssa_amd_dist_available": ([], c_int), "ssa_amd_dist_init_fake": ([c_int, c_int, c_int], c_int),
        "ssa_amd_dist_ranks": ([], c_int),
        "ssa_amd_score_pairs": ([c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p], c_int),
        "ssa_amd_get_pairs_stats": ([POINTER(ssa_amd_pairs_stats_t)], None),
        "ssa_amd_score_pairs_indexed": ([c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p,
                                         c_void_p, c_size_t, c_void_p], c_int),
        "ssa_amd_align_pairs": ([c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p,
                                 c_size_t], c_int),
        "ssa_amd_get_align_pairs_stats": ([POINTER(ssa_amd_align_pairs_stats_t)], None),
        "ssa_amd_align_hits": ([P, c_int, POINTER(ssa_hit_t), c_size_t], POINTER(alignment_list_t)),
        "ssa_amd_get_align_hits_stats": ([POINTER(ssa_amd_align_pairs_stats_t)], None),
        "ssa_amd_score_pairs_ends": ([c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p], c_int),
        "ssa_amd_align_pairs_ends": ([c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p,
                                      c_size_t], c_int),
        "ssa_amd_score_pairs_banded": ([c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                        c_void_p], c_int),
        "ssa_amd_align_pairs_banded": ([c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                        c_void_p, c_void_p, c_size_t], c_int),
        "ssa_amd_score_pairs_local": ([c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                       c_void_p], c_int),
        "ssa_amd_align_pairs_local": ([c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                       c_void_p, c_void_p, c_size_t], c_int),
        "ssa_amd_summarize_pairs_local": ([c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_size_t, c_void_p], c_int),
        "ssa_amd_score_pairs_xdrop": ([c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_size_t, c_void_p], c_int),
        "ssa_amd_align_pairs_xdrop": ([c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_size_t, c_void_p, c_void_p, c_size_t], c_int),
        "ssa_amd_summarize_pairs_xdrop": ([c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_size_t, c_void_p], c_int),
        "ssa_amd_get_xdrop_dropped": ([], c_uint64),
        "ssa_amd_summarize_hits": ([P, c_int, c_void_p, c_size_t, c_void_p], c_int),
        "ssa_amd_get_summarize_hits_stats": ([POINTER(ssa_amd_hits_stats_t)], None),
        "ssa_amd_map_residues": ([c_char_p, c_size_t, c_char_p, c_size_t], c_size_t),
        "ssa_amd_profile_create": ([c_void_p, c_size_t], P),
        "ssa_amd_profile_from_query": ([P, c_size_t], P),
        "ssa_amd_profile_rows": ([P], c_size_t), "ssa_amd_profile_free": ([P], None),
        "ssa_amd_profile_score_host": ([P, c_int, c_void_p, c_void_p, c_size_t, c_void_p], c_int),
        "ssa_amd_search_profile": ([P, c_int, c_size_t, c_int, POINTER(ssa_hit_t), c_size_t], c_size_t),
        "ssa_amd_search_profile_above": ([P, c_int, c_int64, POINTER(ssa_hit_t), c_size_t, POINTER(c_size_t)],
                                         c_size_t),
        "ssa_amd_get_upload_bytes": ([], c_uint64),
        "ssa_amd_shard_bounds": ([c_void_p, c_size_t, c_size_t, c_size_t, POINTER(c_size_t)], c_int),
    }
    for name, (args, res) in sig.items():
        if os.environ.get("SSA_AMD_LIB") and not hasattr(L, name):
            continue            # an older build under A/B measurement
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    _lib = L
    return L


def _b(s):
    return s.encode() if isinstance(s, str) else s


# ---- thin Pythonic layer (same names as the C API) ---------------------------
def set_output_mode(mode): load().set_output_mode(mode)
def set_simd_compute_mode(mode): load().set_simd_compute_mode(mode)
def set_chunk_size(size): load().set_chunk_size(size)
def set_thread_count(n): load().set_thread_count(n)
def init_score_matrix(mode, matrix): load().init_score_matrix(mode, _b(matrix))
def init_constant_scores(match, mismatch): load().init_constant_scores(match, mismatch)
def init_gap_penalties(gap_open, gap_extend): load().init_gap_penalties(gap_open, gap_extend)
def init_symbol_translation(t, strands, db_gencode, q_gencode):
    load().init_symbol_translation(t, strands, db_gencode, q_gencode)
def init_db(path): load().init_db(_b(path))
def init_sequence_fasta(mode, s): return load().init_sequence_fasta(mode, _b(s))
def free_sequence(q): load().free_sequence(q)
def ssa_exit(): load().ssa_exit()


def _unpack(alist):
    if not alist:
        return []
    a = alist.contents
    out = []
    for i in range(a.len):
        x = a.alignments[i].contents
        out.append({"score": int(x.score), "id": int(x.db_seq.ID), "db_len": int(x.db_seq.len),
                    "db_strand": x.db_seq.strand, "db_frame": x.db_seq.frame,
                    "q_len": int(x.query.len), "q_strand": x.query.strand, "q_frame": x.query.frame,
                    "db_seq": ctypes.string_at(x.db_seq.seq, x.db_seq.len) if x.db_seq.seq else b"",
                    "alignment": x.alignment.decode() if x.alignment else None,
                    "region": (int(x.align_q_start), int(x.align_q_end), int(x.align_d_start), int(x.align_d_end))})
    return out


def sw_align(q, hitcount, bit_width=BIT_WIDTH_16, align_type=COMPUTE_SCORE):
    """Returns the reference's alignment list as a list of dicts (freed)."""
    L = load()
    al = L.sw_align(q, hitcount, bit_width, align_type)
    res = _unpack(al)
    L.free_alignment(al)
    return res


def align_scores(q, hitcount, bit_width=BIT_WIDTH_16, algo=SW):
    """sw_align / nw_align (COMPUTE_SCORE) + free_alignment, exactly the
    public calls the reference's benchmark times (benchmark_util.c:27-48),
    returning only [(score, db_id)] -- reading two fields per hit keeps the
    Python side to a few microseconds (bench.py's timed step)."""
    L = load()
    al = (L.sw_align if algo == SW else L.nw_align)(q, hitcount, bit_width, COMPUTE_SCORE)
    out = []
    if al:
        a = al.contents
        arr = a.alignments
        for i in range(a.len):
            x = arr[i].contents
            out.append((x.score, x.db_seq.ID))
    L.free_alignment(al)
    return out


def align_free(q, hitcount, bit_width=BIT_WIDTH_16, algo=SW):
    """free_alignment(sw_align(...)) / free_alignment(nw_align(...)) with the
    hits unread: the call the reference's benchmark times
    (benchmark/src/benchmark_util.c:27-48)."""
    L = load()
    L.free_alignment((L.sw_align if algo == SW else L.nw_align)(q, hitcount, bit_width, COMPUTE_SCORE))


def nw_align(q, hitcount, bit_width=BIT_WIDTH_16, align_type=COMPUTE_SCORE):
    L = load()
    al = L.nw_align(q, hitcount, bit_width, align_type)
    res = _unpack(al)
    L.free_alignment(al)
    return res


def device_count():
    return load().ssa_amd_device_count()


def set_device(dev): load().ssa_amd_set_device(dev)


def set_devices(devs):
    """ssa_amd_set_devices: search on all of `devs` from this process ([] = single device)."""
    arr = (c_int * max(len(devs), 1))(*devs)
    return load().ssa_amd_set_devices(arr, len(devs))


def get_devices():
    """ssa_amd_get_devices: the device slots the next search uses (after
    SSA_AMD_DEVICES, read at the first init_db unless set_device(s) ran)."""
    arr = (c_int * 16)()
    n = load().ssa_amd_get_devices(arr, 16)
    return [arr[i] for i in range(min(n, 16))]


def set_id_offset(off): load().ssa_amd_set_id_offset(off)
def prepare_db(): return load().ssa_amd_prepare_db()
def set_option(name, value): load().ssa_amd_set_option(_b(name), value)
def save_db(path): return load().ssa_amd_save_db(_b(path))
def load_db(path): return load().ssa_amd_load_db(_b(path))




def stats():
    s = ssa_amd_stats_t()          # (per call: threads of a fake dist group read their own)
    load().ssa_amd_get_stats(ctypes.byref(s))
    d = {f: getattr(s, f) for f, _ in ssa_amd_stats_t._fields_}
    d["pruned_whole"] = int(load().ssa_amd_get_pruned_whole())    # (beside the struct, whose layout is kept)
    # (an older build under A/B measurement has no such call)
    d["promoted_lanes"] = int(load().ssa_amd_get_promoted_lanes()) if hasattr(load(), "ssa_amd_get_promoted_lanes") else 0
    d["kernel"] = d["kernel"].decode()
    d["long_kernel"] = d["long_kernel"].decode()
    n = d["slots"]
    for f in ("slot_device", "slot_kernel_ms", "slot_search_ms"):
        d[f] = list(d[f])[:n]
    return d


def timeline():
    """ssa_amd_get_timeline: the last search's DP wave rows (option
    "timeline") as a uint32 array [rows, 4]: (group or 0x80000000 | lane,
    start, end, place), s_memrealtime ticks (100 MHz)."""
    import numpy as np
    L = load()
    n = L.ssa_amd_get_timeline(None, 0)
    out = np.zeros((n, 4), np.uint32)
    if n:
        L.ssa_amd_get_timeline(out.ctypes.data, n)
    return out


def prune_start_order(ncols, qlen, pct=25, most=0):
    """ssa_amd_prune_start_order: the unit each first-part ticket of a pruned
    search runs, for groups of ncols columns (longest first).  Host only."""
    import numpy as np
    nc = np.ascontiguousarray(ncols, np.uint32)
    L = load()
    n = L.ssa_amd_prune_start_order(nc.ctypes.data, nc.size, qlen, pct, most, None, 0)
    out = np.zeros(n, np.uint32)
    if n:
        L.ssa_amd_prune_start_order(nc.ctypes.data, nc.size, qlen, pct, most, out.ctypes.data, n)
    return out


_hitbuf = [None, 0]     # reused output array (a fresh 64 Ki-entry ctypes array per call costs ~0.2 ms)


def _hits(cap):
    if _hitbuf[1] < cap:
        _hitbuf[0], _hitbuf[1] = (ssa_hit_t * cap)(), cap
    return _hitbuf[0]


def search(q, algo, hitcount, bit_width=BIT_WIDTH_16, mode=TOPK, cap=None):
    """ssa_amd_search: sorted top-k (mode=TOPK) or the shard insertion log
    (mode=LOG) as a list of (score, global_id, query_id, strand, frame)."""
    L = load()
    explicit = cap is not None
    if cap is None:
        cap = max(hitcount, 1) if mode == TOPK else max(4 * hitcount + 4096, 65536)
    while True:
        buf = _hits(cap)
        n = L.ssa_amd_search(q, algo, hitcount, bit_width, mode, buf, cap)
        if n < cap or explicit or mode == TOPK:
            break
        cap *= 4            # a log filled the buffer: search again with room
    return [(buf[i].score, buf[i].db_id, buf[i].query_id, buf[i].db_strand, buf[i].db_frame) for i in range(n)]


def _above_args(min_score, cap):
    if isinstance(min_score, bool) or not isinstance(min_score, int):
        raise TypeError(f"min_score must be an int, not {type(min_score).__name__}")
    if not -2 ** 63 <= min_score < 2 ** 63:
        raise OverflowError(f"min_score {min_score} is no int64")
    if cap is not None and (isinstance(cap, bool) or not isinstance(cap, int)):
        raise TypeError(f"cap must be an int or None, not {type(cap).__name__}")
    if cap is not None and cap < 0:
        raise ValueError(f"cap must be >= 0, not {cap}")


def _hit_tuples(buf, n):
    return [(buf[i].score, buf[i].db_id, buf[i].query_id, buf[i].db_strand, buf[i].db_frame) for i in range(n)]


def search_above(q, algo, min_score, bit_width=BIT_WIDTH_16, cap=None):
    """ssa_amd_search_above: (hits, total) -- every (view, entry) of the open
    DB scoring at least min_score as (score, global_id, query_id, strand,
    frame), best first, and their number.  cap: at most that many hits (the
    first of the full list; 0 counts only); None: count first, then fetch all
    -- two whole searches, so pass a cap where an upper bound is known."""
    _above_args(min_score, cap)
    L = load()
    total = c_size_t(0)
    if cap is None or cap == 0:
        L.ssa_amd_search_above(q, algo, min_score, bit_width, None, 0, ctypes.byref(total))
        if cap == 0 or total.value == 0:
            return [], total.value
        cap = total.value
    buf = _hits(cap)
    n = L.ssa_amd_search_above(q, algo, min_score, bit_width, buf, cap, ctypes.byref(total))
    return _hit_tuples(buf, n), total.value


def profile_create(rows):
    """ssa_amd_profile_create: a profile from an int array [rows, 32], rows[i][c]
    the score of DB residue code c at query position i, every value within
    [-32768, 32767].  Returns the handle, or None when the library refuses it
    (no rows, a value out of range).  Free it with profile_free."""
    import numpy as np
    a = np.asarray(rows)
    if a.ndim != 2 or a.shape[1] != 32 or a.dtype.kind not in "iu":
        raise ValueError("profile_create: an integer array [rows, 32] expected")
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        return None                 # (no int32: out of the profile's range anyway)
    a = np.ascontiguousarray(a, np.int32)
    return load().ssa_amd_profile_create(a.ctypes.data if a.size else None, a.shape[0])


def profile_from_query(q, view=0):
    """ssa_amd_profile_from_query: the profile that view `view` of the sequence
    query q is under the current matrix (None for a bad or empty view)."""
    return load().ssa_amd_profile_from_query(q, view)


def profile_rows(p): return load().ssa_amd_profile_rows(p)
def profile_free(p): load().ssa_amd_profile_free(p)


def profile_score_host(p, algo, codes, off):
    """ssa_amd_profile_score_host: the exact int64 scores of profile p against
    the sequences codes[off[e]:off[e + 1]] (uint8 codes, uint64 offsets), on the
    host.  Raises ValueError when the library refuses the arguments."""
    import numpy as np
    codes = np.ascontiguousarray(codes, np.uint8)
    off = np.ascontiguousarray(off, np.uint64)
    if len(off) < 1:
        raise ValueError("profile_score_host: an offset array of n + 1 entries expected")
    n = len(off) - 1
    out = np.zeros(n, np.int64)
    rc = load().ssa_amd_profile_score_host(p, algo, codes.ctypes.data, off.ctypes.data, n, out.ctypes.data)
    if rc != 0:
        raise ValueError(f"ssa_amd_profile_score_host refused its arguments ({rc})")
    return out


def search_profile(p, algo, hitcount, mode=TOPK, cap=None):
    """ssa_amd_search_profile: search()'s result with profile p in the query's place."""
    L = load()
    explicit = cap is not None
    if cap is None:
        cap = max(hitcount, 1) if mode == TOPK else max(4 * hitcount + 4096, 65536)
    while True:
        buf = _hits(cap)
        n = L.ssa_amd_search_profile(p, algo, hitcount, mode, buf, cap)
        if n < cap or explicit or mode == TOPK:
            break
        cap *= 4            # a log filled the buffer: search again with room
    return _hit_tuples(buf, n)


def search_profile_above(p, algo, min_score, cap=None):
    """ssa_amd_search_profile_above: search_above()'s (hits, total) with profile p
    in the query's place."""
    _above_args(min_score, cap)
    L = load()
    total = c_size_t(0)
    if cap is None or cap == 0:
        L.ssa_amd_search_profile_above(p, algo, min_score, None, 0, ctypes.byref(total))
        if cap == 0 or total.value == 0:
            return [], total.value
        cap = total.value
    buf = _hits(cap)
    n = L.ssa_amd_search_profile_above(p, algo, min_score, buf, cap, ctypes.byref(total))
    return _hit_tuples(buf, n), total.value


def upload_bytes():
    """ssa_amd_get_upload_bytes: bytes the last search staged for its per-search upload."""
    return int(load().ssa_amd_get_upload_bytes())


def merge_above(hits, min_score, cap=None):
    """ssa_amd_merge_above: (hits, total) -- the hits of a (concatenated)
    list of hit tuples at or above min_score in search_above's order, cut to
    cap (None: all), and their number before the cut.  Host only."""
    _above_args(min_score, cap)
    L = load()
    n = len(hits)
    arr = _hit_array(hits)
    total = c_size_t(0)
    if cap is None:
        cap = n
    out = (ssa_hit_t * max(cap, 1))()
    c = L.ssa_amd_merge_above(arr, n, min_score, out, cap, ctypes.byref(total))
    return _hit_tuples(out, c), total.value


def replay(log, hitcount):
    """ssa_amd_replay over a (concatenated) insertion log."""
    L = load()
    n = len(log)
    arr = (ssa_hit_t * max(n, 1))()
    for i, h in enumerate(log):
        arr[i].score, arr[i].db_id = int(h[0]), int(h[1])
        if len(h) > 2:
            arr[i].query_id, arr[i].db_strand, arr[i].db_frame = int(h[2]), int(h[3]), int(h[4])
    out = (ssa_hit_t * max(hitcount, 1))()
    c = L.ssa_amd_replay(arr, n, hitcount, out)
    return [(out[i].score, out[i].db_id) for i in range(c)]


def query_views(q):
    """ssa_amd_query_views: [(codes: bytes, strand, frame)] of the search's query buffers."""
    L = load()
    buf = (q_seq_t * 8)()
    n = L.ssa_amd_query_views(q, buf, 8)
    return [(ctypes.string_at(buf[i].seq, buf[i].len), buf[i].strand, buf[i].frame) for i in range(min(n, 8))]


def translate(db_side, nt_codes, strand, frame):
    """ssa_amd_translate on mapped nucleotide codes; returns amino-acid codes (bytes)."""
    L = load()
    src = bytes(nt_codes)
    out = ctypes.create_string_buffer(len(src) // 3 + 1)
    n = L.ssa_amd_translate(db_side, src, len(src), strand, frame, out, len(out))
    return out.raw[:n]


def align_pair(algo, query_codes, db_codes):
    """ssa_amd_align_pair: ((q_begin, q_end, d_begin, d_end), cigar) of one pair."""
    L = load()
    q, d = bytes(query_codes), bytes(db_codes)
    reg = (c_size_t * 4)()
    n = L.ssa_amd_align_pair(algo, q, len(q), d, len(d), reg, None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    L.ssa_amd_align_pair(algo, q, len(q), d, len(d), reg, buf, n + 1)
    return tuple(reg), buf.value.decode()


def _concat_codes(seqs):
    import numpy as np
    off = np.zeros(len(seqs) + 1, np.uint64)
    if seqs:
        np.cumsum([len(s) for s in seqs], out=off[1:])
    parts = [np.frombuffer(s, np.uint8) if isinstance(s, (bytes, bytearray)) else np.asarray(s, np.uint8)
             for s in seqs]
    codes = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    if codes.size == 0:
        codes = np.zeros(1, np.uint8)
    return np.ascontiguousarray(codes), off


def score_pairs(algo, queries, targets):
    """ssa_amd_score_pairs: the exact score of queries[i] against targets[i]
    (two equal-length lists of uint8 residue-code arrays) as an int64 array --
    what sw_align / nw_align report for query i against the one-entry DB
    targets[i].  Raises ValueError when the library refuses the arguments."""
    import numpy as np
    if len(queries) != len(targets):
        raise ValueError("score_pairs: queries and targets differ in length")
    q, qo = _concat_codes(queries)
    d, do = _concat_codes(targets)
    return score_pairs_flat(algo, q, qo, d, do)


def score_pairs_flat(algo, q_codes, q_off, d_codes, d_off):
    """ssa_amd_score_pairs on the C layout itself: contiguous uint8 code
    arrays and uint64 offset arrays of npairs + 1 entries each (no per-call
    concatenation: what a caller with many pairs keeps around)."""
    return _score_flat("ssa_amd_score_pairs", "score_pairs_flat", algo, q_codes, q_off, d_codes, d_off)


def score_pairs_indexed(algo, queries, targets, q_idx, d_idx):
    """ssa_amd_score_pairs_indexed: the exact score of queries[q_idx[p]]
    against targets[d_idx[p]] for every p, as an int64 array -- what
    score_pairs gives for the expanded lists.  queries and targets are lists
    of uint8 residue-code arrays (the same list object for a set against
    itself: it is then uploaded once), q_idx and d_idx equal-length integer
    arrays.  Raises ValueError when the library refuses the arguments."""
    q, qo = _concat_codes(queries)
    d, do = (q, qo) if targets is queries else _concat_codes(targets)
    return score_pairs_indexed_flat(algo, q, qo, d, do, q_idx, d_idx)


def score_pairs_indexed_flat(algo, q_codes, q_off, d_codes, d_off, q_idx, d_idx):
    """ssa_amd_score_pairs_indexed on the C layout itself: contiguous uint8
    pools, uint64 offset arrays of nq + 1 and nd + 1 entries, and two index
    arrays of npairs entries (any integer type; values outside uint32 are
    refused here)."""
    import numpy as np
    name = "score_pairs_indexed_flat"
    for a, t in ((q_codes, np.uint8), (d_codes, np.uint8), (q_off, np.uint64), (d_off, np.uint64)):
        if a.dtype != t or not a.flags.c_contiguous:
            raise ValueError(f"{name}: contiguous uint8 codes and uint64 offsets expected")
    if len(q_off) < 1 or len(d_off) < 1:
        raise ValueError(f"{name}: offset arrays of nq + 1 and nd + 1 entries expected")
    idx = []
    for a in (q_idx, d_idx):
        a = np.asarray(a)
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
            raise ValueError(f"{name}: one-dimensional integer index arrays expected")
        if a.size and (int(a.min()) < 0 or int(a.max()) > 0xffffffff):
            raise ValueError(f"{name}: an index outside uint32")
        idx.append(np.ascontiguousarray(a, np.uint32))
    if len(idx[0]) != len(idx[1]):
        raise ValueError(f"{name}: q_idx and d_idx differ in length")
    n = len(idx[0])
    out = np.zeros(n, np.int64)
    rc = load().ssa_amd_score_pairs_indexed(algo, q_codes.ctypes.data, q_off.ctypes.data, len(q_off) - 1,
                                            d_codes.ctypes.data, d_off.ctypes.data, len(d_off) - 1,
                                            idx[0].ctypes.data, idx[1].ctypes.data, n, out.ctypes.data)
    if rc != 0:
        raise ValueError(f"ssa_amd_score_pairs_indexed refused its arguments ({rc})")
    return out


def _band_arrays(name, band, n):
    """(band_lo, band_hi) as contiguous int64 arrays of n entries; () for a
    call without band arguments; a (None, None) band stays two NULL pointers."""
    import numpy as np
    if band is None:
        return ()
    if band[0] is None and band[1] is None:
        return None, None
    if band[0] is None or band[1] is None:
        raise ValueError(f"{name}: band_lo and band_hi are given together or not at all")
    lo, hi = (np.ascontiguousarray(b, np.int64) for b in band)
    if lo.shape != (n,) or hi.shape != (n,):
        raise ValueError(f"{name}: band_lo and band_hi of npairs entries expected")
    return lo, hi


def _score_flat(symbol, name, mode, q_codes, q_off, d_codes, d_off, band=None, extra=()):
    import numpy as np
    for a, t in ((q_codes, np.uint8), (d_codes, np.uint8), (q_off, np.uint64), (d_off, np.uint64)):
        if a.dtype != t or not a.flags.c_contiguous:
            raise ValueError(f"{name}: contiguous uint8 codes and uint64 offsets expected")
    if len(q_off) != len(d_off) or len(q_off) < 1:
        raise ValueError(f"{name}: offset arrays of npairs + 1 entries expected")
    n = len(q_off) - 1
    out = np.zeros(n, np.int64)
    band = _band_arrays(name, band, n)
    rc = getattr(load(), symbol)(mode, *extra, *(None if b is None else b.ctypes.data for b in band),
                                 q_codes.ctypes.data, q_off.ctypes.data, d_codes.ctypes.data, d_off.ctypes.data, n,
                                 out.ctypes.data)
    if rc != 0:
        raise ValueError(f"{symbol} refused its arguments ({rc})")
    return out


def pairs_stats():
    """ssa_amd_get_pairs_stats: the last score_pairs call as a dict."""
    s = ssa_amd_pairs_stats_t()
    load().ssa_amd_get_pairs_stats(ctypes.byref(s))
    d = {f: getattr(s, f) for f, _ in ssa_amd_pairs_stats_t._fields_}
    d["kernel"] = d["kernel"].decode()
    return d


def align_pairs(algo, queries, targets):
    """ssa_amd_align_pairs: [(score, (q_begin, q_end, d_begin, d_end), cigar)]
    of queries[i] against targets[i] (two equal-length lists of uint8
    residue-code arrays); region and CIGAR are align_pair's, the score is
    score_pairs'.  Raises ValueError when the library refuses the arguments."""
    if len(queries) != len(targets):
        raise ValueError("align_pairs: queries and targets differ in length")
    q, qo = _concat_codes(queries)
    d, do = _concat_codes(targets)
    return _alignment_list(*align_pairs_flat(algo, q, qo, d, do))


ALIGNMENT_DTYPE = [("score", "<i8"), ("region", "<u8", (4,)), ("cigar_off", "<u8"), ("cigar_len", "<u4"),
                   ("flags", "<u4")]


def align_pairs_flat(algo, q_codes, q_off, d_codes, d_off):
    """ssa_amd_align_pairs on the C layout itself (the arrays of
    score_pairs_flat): returns (out, cigars) -- a structured array of
    ssa_amd_pair_alignment_t records (ALIGNMENT_DTYPE) and the uint8 CIGAR
    buffer of sum(qlen + dlen + 1) bytes that out's cigar_off / cigar_len
    index."""
    return _align_flat("ssa_amd_align_pairs", "align_pairs_flat", algo, q_codes, q_off, d_codes, d_off)


def _align_flat(symbol, name, mode, q_codes, q_off, d_codes, d_off, band=None, extra=()):
    import numpy as np
    for a, t in ((q_codes, np.uint8), (d_codes, np.uint8), (q_off, np.uint64), (d_off, np.uint64)):
        if a.dtype != t or not a.flags.c_contiguous:
            raise ValueError(f"{name}: contiguous uint8 codes and uint64 offsets expected")
    if len(q_off) != len(d_off) or len(q_off) < 1:
        raise ValueError(f"{name}: offset arrays of npairs + 1 entries expected")
    n = len(q_off) - 1
    out = np.zeros(n, np.dtype(ALIGNMENT_DTYPE))
    assert out.dtype.itemsize == ctypes.sizeof(ssa_amd_pair_alignment_t)
    cap = 1
    if n and q_off[n] >= q_off[0] and d_off[n] >= d_off[0]:
        cap = int(q_off[n] - q_off[0]) + int(d_off[n] - d_off[0]) + n
    cigars = np.zeros(cap, np.uint8)
    band = _band_arrays(name, band, n)
    rc = getattr(load(), symbol)(mode, *extra, *(None if b is None else b.ctypes.data for b in band),
                                 q_codes.ctypes.data, q_off.ctypes.data, d_codes.ctypes.data, d_off.ctypes.data, n,
                                 out.ctypes.data, cigars.ctypes.data, cap)
    if rc != 0:
        raise ValueError(f"{symbol} refused its arguments ({rc})")
    return out, cigars


def _alignment_list(out, text):
    raw = text.tobytes()
    return [(int(o["score"]), tuple(int(x) for x in o["region"]),
             raw[int(o["cigar_off"]):int(o["cigar_off"]) + int(o["cigar_len"])].decode()) for o in out]


# ends-free (semi-global) alignment: the mask bits of ssa_amd_*_pairs_ends
FREE_Q_BEGIN, FREE_Q_END, FREE_D_BEGIN, FREE_D_END = 1, 2, 4, 8


def score_pairs_ends(ends, queries, targets):
    """ssa_amd_score_pairs_ends: the ends-free score of queries[i] against
    targets[i] under the mask `ends` (FREE_* bits) as an int64 array; lists
    as score_pairs takes them.  Raises ValueError when the library refuses
    the arguments (a mask outside 0..15 among them)."""
    if len(queries) != len(targets):
        raise ValueError("score_pairs_ends: queries and targets differ in length")
    q, qo = _concat_codes(queries)
    d, do = _concat_codes(targets)
    return score_pairs_ends_flat(ends, q, qo, d, do)


def score_pairs_ends_flat(ends, q_codes, q_off, d_codes, d_off):
    """ssa_amd_score_pairs_ends on the C layout itself (score_pairs_flat's arrays)."""
    return _score_flat("ssa_amd_score_pairs_ends", "score_pairs_ends_flat", ends, q_codes, q_off, d_codes, d_off)


def align_pairs_ends(ends, queries, targets):
    """ssa_amd_align_pairs_ends: [(score, (q_begin, q_end, d_begin, d_end),
    cigar)] of queries[i] against targets[i] under the mask `ends`; shapes
    and errors as align_pairs."""
    if len(queries) != len(targets):
        raise ValueError("align_pairs_ends: queries and targets differ in length")
    q, qo = _concat_codes(queries)
    d, do = _concat_codes(targets)
    return _alignment_list(*align_pairs_ends_flat(ends, q, qo, d, do))


def align_pairs_ends_flat(ends, q_codes, q_off, d_codes, d_off):
    """ssa_amd_align_pairs_ends on the C layout itself: (out, cigars) as align_pairs_flat."""
    return _align_flat("ssa_amd_align_pairs_ends", "align_pairs_ends_flat", ends, q_codes, q_off, d_codes, d_off)


def default_band(qlens, dlens, w):
    """The band of half-width w around both corners' diagonals, valid for
    every mask: (lo, hi) int64 arrays with lo = min(0, n - m) - w and
    hi = max(0, n - m) + w for m = qlens[i], n = dlens[i]."""
    import numpy as np
    diff = np.asarray(dlens, np.int64) - np.asarray(qlens, np.int64)
    return np.minimum(0, diff) - int(w), np.maximum(0, diff) + int(w)


def score_pairs_banded(ends, queries, targets, band_lo, band_hi):
    """ssa_amd_score_pairs_banded: the ends-free score of queries[i] against
    targets[i] under the mask `ends`, over the cells whose diagonal k =
    (target position) - (query position) lies in [band_lo[i], band_hi[i]], as
    an int64 array.  Raises ValueError when the library refuses the arguments
    (a band that admits no alignment among them)."""
    if len(queries) != len(targets):
        raise ValueError("score_pairs_banded: queries and targets differ in length")
    q, qo = _concat_codes(queries)
    d, do = _concat_codes(targets)
    return score_pairs_banded_flat(ends, q, qo, d, do, band_lo, band_hi)


def score_pairs_banded_flat(ends, q_codes, q_off, d_codes, d_off, band_lo, band_hi):
    """ssa_amd_score_pairs_banded on the C layout itself (score_pairs_flat's
    arrays, and one int64 band_lo / band_hi entry per pair)."""
    return _score_flat("ssa_amd_score_pairs_banded", "score_pairs_banded_flat", ends, q_codes, q_off, d_codes, d_off,
                       band=(band_lo, band_hi))


def align_pairs_banded(ends, queries, targets, band_lo, band_hi):
    """ssa_amd_align_pairs_banded: [(score, (q_begin, q_end, d_begin, d_end),
    cigar)] of the same alignments; shapes and errors as align_pairs_ends."""
    if len(queries) != len(targets):
        raise ValueError("align_pairs_banded: queries and targets differ in length")
    q, qo = _concat_codes(queries)
    d, do = _concat_codes(targets)
    return _alignment_list(*align_pairs_banded_flat(ends, q, qo, d, do, band_lo, band_hi))


def align_pairs_banded_flat(ends, q_codes, q_off, d_codes, d_off, band_lo, band_hi):
    """ssa_amd_align_pairs_banded on the C layout itself: (out, cigars) as align_pairs_flat."""
    return _align_flat("ssa_amd_align_pairs_banded", "align_pairs_banded_flat", ends, q_codes, q_off, d_codes, d_off,
                       band=(band_lo, band_hi))


# local begin / end: the mode bits of ssa_amd_*_pairs_local beside the FREE_* ones
LOCAL_BEGIN, LOCAL_END, LOCAL = 16, 32, 48


def score_pairs_local(mode, queries, targets, band_lo=None, band_hi=None):
    """ssa_amd_score_pairs_local: the score of queries[i] against targets[i]
    under `mode` (FREE_* and LOCAL_* bits; LOCAL = 48 is Smith-Waterman) inside
    the bands, as an int64 array; band_lo = band_hi = None is unbanded (NULL
    pointers).  Raises ValueError when the library refuses the arguments."""
    if len(queries) != len(targets):
        raise ValueError("score_pairs_local: queries and targets differ in length")
    q, qo = _concat_codes(queries)
    d, do = _concat_codes(targets)
    return score_pairs_local_flat(mode, q, qo, d, do, band_lo, band_hi)


def score_pairs_local_flat(mode, q_codes, q_off, d_codes, d_off, band_lo=None, band_hi=None):
    """ssa_amd_score_pairs_local on the C layout itself (score_pairs_banded_flat's arrays)."""
    return _score_flat("ssa_amd_score_pairs_local", "score_pairs_local_flat", mode, q_codes, q_off, d_codes, d_off,
                       band=(band_lo, band_hi))


def align_pairs_local(mode, queries, targets, band_lo=None, band_hi=None):
    """ssa_amd_align_pairs_local: [(score, (q_begin, q_end, d_begin, d_end),
    cigar)] of the same alignments; a zero score has region zeros and an
    empty CIGAR.  Shapes and errors as align_pairs_banded."""
    if len(queries) != len(targets):
        raise ValueError("align_pairs_local: queries and targets differ in length")
    q, qo = _concat_codes(queries)
    d, do = _concat_codes(targets)
    return _alignment_list(*align_pairs_local_flat(mode, q, qo, d, do, band_lo, band_hi))


def align_pairs_local_flat(mode, q_codes, q_off, d_codes, d_off, band_lo=None, band_hi=None):
    """ssa_amd_align_pairs_local on the C layout itself: (out, cigars) as align_pairs_flat."""
    return _align_flat("ssa_amd_align_pairs_local", "align_pairs_local_flat", mode, q_codes, q_off, d_codes, d_off,
                       band=(band_lo, band_hi))


SUMMARY_DTYPE = [("score", "<i8"), ("region", "<u8", (4,)), ("columns", "<u4"), ("matched", "<u4"),
                 ("identical", "<u4"), ("flags", "<u4")]


def summarize_pairs_local(mode, queries, targets, band_lo=None, band_hi=None):
    """ssa_amd_summarize_pairs_local: [(score, (q_begin, q_end, d_begin,
    d_end), columns, matched, identical, flags)] of align_pairs_local's
    alignments, without their CIGARs; a pair that has none there is all zeros
    behind its score.  Shapes and errors as align_pairs_local."""
    if len(queries) != len(targets):
        raise ValueError("summarize_pairs_local: queries and targets differ in length")
    q, qo = _concat_codes(queries)
    d, do = _concat_codes(targets)
    out = summarize_pairs_local_flat(mode, q, qo, d, do, band_lo, band_hi)
    return [(int(o["score"]), tuple(int(x) for x in o["region"]), int(o["columns"]), int(o["matched"]),
             int(o["identical"]), int(o["flags"])) for o in out]


def summarize_pairs_local_flat(mode, q_codes, q_off, d_codes, d_off, band_lo=None, band_hi=None):
    """ssa_amd_summarize_pairs_local on the C layout itself (score_pairs_banded_flat's
    arrays): a structured array of ssa_amd_pair_summary_t records (SUMMARY_DTYPE)."""
    return _summary_flat("ssa_amd_summarize_pairs_local", "summarize_pairs_local_flat", mode, q_codes, q_off, d_codes,
                         d_off, band_lo, band_hi)


def _summary_flat(symbol, name, mode, q_codes, q_off, d_codes, d_off, band_lo, band_hi, extra=()):
    import numpy as np
    for a, t in ((q_codes, np.uint8), (d_codes, np.uint8), (q_off, np.uint64), (d_off, np.uint64)):
        if a.dtype != t or not a.flags.c_contiguous:
            raise ValueError(f"{name}: contiguous uint8 codes and uint64 offsets expected")
    if len(q_off) != len(d_off) or len(q_off) < 1:
        raise ValueError(f"{name}: offset arrays of npairs + 1 entries expected")
    n = len(q_off) - 1
    out = np.zeros(n, np.dtype(SUMMARY_DTYPE))
    assert out.dtype.itemsize == ctypes.sizeof(ssa_amd_pair_summary_t)
    band = _band_arrays(name, (band_lo, band_hi), n)
    rc = getattr(load(), symbol)(mode, *extra, *(None if b is None else b.ctypes.data for b in band),
                                 q_codes.ctypes.data, q_off.ctypes.data, d_codes.ctypes.data, d_off.ctypes.data, n,
                                 out.ctypes.data)
    if rc != 0:
        raise ValueError(f"{symbol} refused its arguments ({rc})")
    return out


def _xdrop_value(name, xdrop):
    x = int(xdrop)
    if not -(1 << 63) <= x < (1 << 63):
        raise ValueError(f"{name}: xdrop outside int64")
    return x


def score_pairs_xdrop(mode, xdrop, queries, targets, band_lo=None, band_hi=None):
    """ssa_amd_score_pairs_xdrop: score_pairs_local under a mode that
    canonicalises to 42, 43, 46 or 47, with the end candidates cut at the
    first row whose greatest H lies more than `xdrop` (>= 0) below the best
    score so far.  Raises ValueError when the library refuses the arguments."""
    if len(queries) != len(targets):
        raise ValueError("score_pairs_xdrop: queries and targets differ in length")
    q, qo = _concat_codes(queries)
    d, do = _concat_codes(targets)
    return score_pairs_xdrop_flat(mode, xdrop, q, qo, d, do, band_lo, band_hi)


def score_pairs_xdrop_flat(mode, xdrop, q_codes, q_off, d_codes, d_off, band_lo=None, band_hi=None):
    """ssa_amd_score_pairs_xdrop on the C layout itself (score_pairs_banded_flat's arrays)."""
    return _score_flat("ssa_amd_score_pairs_xdrop", "score_pairs_xdrop_flat", mode, q_codes, q_off, d_codes, d_off,
                       band=(band_lo, band_hi), extra=(_xdrop_value("score_pairs_xdrop_flat", xdrop),))


def align_pairs_xdrop(mode, xdrop, queries, targets, band_lo=None, band_hi=None):
    """ssa_amd_align_pairs_xdrop: [(score, (q_begin, q_end, d_begin, d_end),
    cigar)] of the same alignments; shapes and errors as align_pairs_local."""
    if len(queries) != len(targets):
        raise ValueError("align_pairs_xdrop: queries and targets differ in length")
    q, qo = _concat_codes(queries)
    d, do = _concat_codes(targets)
    return _alignment_list(*align_pairs_xdrop_flat(mode, xdrop, q, qo, d, do, band_lo, band_hi))


def align_pairs_xdrop_flat(mode, xdrop, q_codes, q_off, d_codes, d_off, band_lo=None, band_hi=None):
    """ssa_amd_align_pairs_xdrop on the C layout itself: (out, cigars) as align_pairs_flat."""
    return _align_flat("ssa_amd_align_pairs_xdrop", "align_pairs_xdrop_flat", mode, q_codes, q_off, d_codes, d_off,
                       band=(band_lo, band_hi), extra=(_xdrop_value("align_pairs_xdrop_flat", xdrop),))


def summarize_pairs_xdrop(mode, xdrop, queries, targets, band_lo=None, band_hi=None):
    """ssa_amd_summarize_pairs_xdrop: summarize_pairs_local's tuples of
    align_pairs_xdrop's alignments, without their CIGARs."""
    if len(queries) != len(targets):
        raise ValueError("summarize_pairs_xdrop: queries and targets differ in length")
    q, qo = _concat_codes(queries)
    d, do = _concat_codes(targets)
    out = summarize_pairs_xdrop_flat(mode, xdrop, q, qo, d, do, band_lo, band_hi)
    return [(int(o["score"]), tuple(int(x) for x in o["region"]), int(o["columns"]), int(o["matched"]),
             int(o["identical"]), int(o["flags"])) for o in out]


def summarize_pairs_xdrop_flat(mode, xdrop, q_codes, q_off, d_codes, d_off, band_lo=None, band_hi=None):
    """ssa_amd_summarize_pairs_xdrop on the C layout itself: SUMMARY_DTYPE records."""
    return _summary_flat("ssa_amd_summarize_pairs_xdrop", "summarize_pairs_xdrop_flat", mode, q_codes, q_off, d_codes,
                         d_off, band_lo, band_hi, extra=(_xdrop_value("summarize_pairs_xdrop_flat", xdrop),))


def xdrop_dropped():
    """ssa_amd_get_xdrop_dropped: pairs of the last xdrop call that met a drop row."""
    return int(load().ssa_amd_get_xdrop_dropped())


def align_pairs_stats():
    """ssa_amd_get_align_pairs_stats: the last align_pairs call as a dict."""
    s = ssa_amd_align_pairs_stats_t()
    load().ssa_amd_get_align_pairs_stats(ctypes.byref(s))
    d = {f: getattr(s, f) for f, _ in ssa_amd_align_pairs_stats_t._fields_}
    d["kernels"] = d["kernels"].decode()
    return d


def align_hits(q, algo, hits):
    """ssa_amd_align_hits: the alignment list (dicts, as sw_align returns them)
    sw_align / nw_align with COMPUTE_ALIGNMENT would give for these hits of the
    open DB -- tuples (score, db_id[, query_id, db_strand, db_frame]) as search
    and search_batch return them.  None when the library refuses the hits."""
    L = load()
    al = L.ssa_amd_align_hits(q, algo, _hit_array(hits), len(hits))
    if not al:
        return None
    res = _unpack(al)
    L.free_alignment(al)
    return res


def summarize_hits(q, mode, hits):
    """ssa_amd_summarize_hits: summarize_pairs_local's tuples [(score, (q_begin,
    q_end, d_begin, d_end), columns, matched, identical, flags)] for hits of
    the open DB -- tuples (score, db_id[, query_id, db_strand, db_frame]) as
    search and search_above return them; the d side is the entry as the search
    scored it.  None when the library refuses the hits."""
    out = summarize_hits_flat(q, mode, _hit_array(hits), len(hits))
    if out is None:
        return None
    return [(int(o["score"]), tuple(int(x) for x in o["region"]), int(o["columns"]), int(o["matched"]),
             int(o["identical"]), int(o["flags"])) for o in out]


def summarize_hits_flat(q, mode, hit_array, n):
    """ssa_amd_summarize_hits on the C layout itself: the first n ssa_hit_t of a
    ctypes array (as _hits / search write them) -> SUMMARY_DTYPE records, or
    None when the library refuses them."""
    import numpy as np
    out = np.zeros(n, np.dtype(SUMMARY_DTYPE))
    rc = load().ssa_amd_summarize_hits(q, mode, ctypes.addressof(hit_array) if n else None, n,
                                       out.ctypes.data if n else None)
    return out if rc == 0 else None


def summarize_hits_stats():
    """ssa_amd_get_summarize_hits_stats: what only the last summarize_hits call
    has (hits, gathered, fetched, upload_bytes, gather_ms) as a dict; the rest
    of the call is in align_pairs_stats()."""
    s = ssa_amd_hits_stats_t()
    load().ssa_amd_get_summarize_hits_stats(ctypes.byref(s))
    return {f: getattr(s, f) for f, _ in ssa_amd_hits_stats_t._fields_}


def align_hits_stats():
    """ssa_amd_get_align_hits_stats: the last COMPUTE_ALIGNMENT / align_hits
    alignment stage as a dict (align_pairs_stats' fields)."""
    s = ssa_amd_align_pairs_stats_t()
    load().ssa_amd_get_align_hits_stats(ctypes.byref(s))
    d = {f: getattr(s, f) for f, _ in ssa_amd_align_pairs_stats_t._fields_}
    d["kernels"] = d["kernels"].decode()
    return d


def map_residues(seq):
    """ssa_amd_map_residues: ASCII -> DB-side residue codes (uint8 array) of
    the current symbol type; unknown letters map to 0."""
    import numpy as np
    src = _b(seq)
    out = ctypes.create_string_buffer(max(len(src), 1))
    load().ssa_amd_map_residues(src, len(src), out, len(src))
    return np.frombuffer(out.raw[:len(src)], np.uint8).copy()


def search_batch(queries, algo, hitcount, bit_width=BIT_WIDTH_16):
    """ssa_amd_search_batch: per query, the sorted top-k [(score, id), ...]."""
    L = load()
    nq = len(queries)
    qs = (c_void_p * max(nq, 1))(*queries)
    out = (ssa_hit_t * max(nq * hitcount, 1))()
    counts = (c_size_t * max(nq, 1))()
    L.ssa_amd_search_batch(qs, nq, algo, hitcount, bit_width, out, counts)
    return [[(out[i * hitcount + j].score, out[i * hitcount + j].db_id) for j in range(counts[i])] for i in range(nq)]


# ---- multi-process gather over RCCL (libssa_amd.h ssa_amd_dist_*) ------------
def dist_unique_id():
    """Rank 0: the RCCL unique id (bytes) to hand to every rank."""
    L = load()
    buf = ctypes.create_string_buffer(L.ssa_amd_dist_unique_id_bytes())
    if L.ssa_amd_dist_unique_id(buf) != 0:
        raise RuntimeError("ssa_amd_dist_unique_id failed")
    return buf.raw


def dist_available():
    """ssa_amd_dist_available: True when this rank could enter ssa_amd_dist_init."""
    return load().ssa_amd_dist_available() == 0


def dist_init(rank, world, uid):
    if load().ssa_amd_dist_init(rank, world, uid) != 0:
        raise RuntimeError(f"ssa_amd_dist_init({rank}, {world}) failed")


def dist_init_fake(rank, world, group=0):
    """ssa_amd_dist_init_fake: the calling thread becomes rank `rank` of an
    in-process group of `world` threads (test support)."""
    if load().ssa_amd_dist_init_fake(rank, world, group) != 0:
        raise RuntimeError(f"ssa_amd_dist_init_fake({rank}, {world}, {group}) failed")


def dist_ranks():
    """ssa_amd_dist_ranks: ranks of the communicator (ncclCommCount)."""
    return load().ssa_amd_dist_ranks()


def dist_finalize(): load().ssa_amd_dist_finalize()


def shard_bounds(lengths, world, align=1):
    """ssa_amd_shard_bounds: world + 1 record bounds of residue-balanced
    contiguous shards (cuts at multiples of `align`)."""
    import numpy as np
    lens = np.ascontiguousarray(lengths, dtype=np.uint64)
    out = (c_size_t * (world + 1))()
    if load().ssa_amd_shard_bounds(lens.ctypes.data, len(lens), world, align, out) != 0:
        raise ValueError("ssa_amd_shard_bounds: world must be >= 1")
    return [int(x) for x in out]


def _hit_array(log):
    arr = (ssa_hit_t * max(len(log), 1))()
    for i, h in enumerate(log):
        arr[i].score, arr[i].db_id = int(h[0]), int(h[1])
        if len(h) > 2:
            arr[i].query_id, arr[i].db_strand, arr[i].db_frame = int(h[2]), int(h[3]), int(h[4])
    return arr


def gather_logs(log, hitcount):
    """ssa_amd_gather_logs (collective): rank 0 gets the global sorted top-k
    [(score, db_id)], the other ranks []."""
    L = load()
    arr = _hit_array(log)
    out = (ssa_hit_t * max(hitcount, 1))()
    c = L.ssa_amd_gather_logs(arr, len(log), hitcount, out)
    return [(out[i].score, out[i].db_id) for i in range(c)]


def merge_logs(logs, hitcount):
    """ssa_amd_merge_logs: rank 0's merge of per-shard logs (in shard order)."""
    L = load()
    stride = max([len(x) for x in logs] + [1])
    rows = (ssa_hit_t * (stride * max(len(logs), 1)))()
    for r, lg in enumerate(logs):
        for i, h in enumerate(lg):
            rows[r * stride + i].score, rows[r * stride + i].db_id = int(h[0]), int(h[1])
            if len(h) > 2:
                rows[r * stride + i].query_id = int(h[2])
                rows[r * stride + i].db_strand, rows[r * stride + i].db_frame = int(h[3]), int(h[4])
    counts = (c_size_t * max(len(logs), 1))(*[len(x) for x in logs])
    out = (ssa_hit_t * max(hitcount, 1))()
    c = L.ssa_amd_merge_logs(rows, counts, len(logs), stride, hitcount, out)
    return [(out[i].score, out[i].db_id) for i in range(c)]
