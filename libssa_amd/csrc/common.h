// common.h -- internal declarations shared by the libssa_amd host sources.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "libssa.h"
#include "libssa_amd.h"
#include "libssa_extern_db.h"

namespace ssa {

constexpr int kDim = 32;          // score matrix is 32 x 32, M(x,y) = m[(x << 5) + y]
constexpr int kAlgoSW = 0;
constexpr int kAlgoNW = 1;
constexpr size_t kMaxSlots = 16;   // devices one process can search on

// ------------------------------------------------------------------ config
struct Config {
    // bumped by every setter of the scoring or the options (api.cpp): the
    // per-DB plan cache (engine.cpp cached_plan) keys on it
    uint64_t plan_gen = 0;
    int output_mode = OUTPUT_WARNING;     // reference util.c:34
    size_t chunk_size = 1000;             // reference util.h:31 DEFAULT_CHUNK_SIZE
    size_t thread_count = 0;              // 0 = all host cores
    int symtype = AMINOACID;              // reference util_sequence.c:178
    int strands = FORWARD_STRAND;         // util_sequence.c:179
    int q_gencode = 1, d_gencode = 1;
    int8_t gap_open = 0, gap_extend = 0;  // libssa.c:35-36
    int device = -1;                      // -1: current HIP device
    std::vector<int> devices;             // ssa_amd_set_devices: shard the DB over these
    bool device_chosen = false;           // the caller called ssa_amd_set_device(s): SSA_AMD_DEVICES is not read
    bool device_env_read = false;         // SSA_AMD_DEVICES was applied (at the first init_db)
    std::vector<int> env_devices;         // the devices SSA_AMD_DEVICES (or its default, all) lists; the search
                                          // uses the first set_thread_count() of them (api.cpp refresh_env_devices)
    size_t id_offset = 0;                 // global ID of local record 0
    uint64_t db_generation = 0;           // bumped by init_db
    // tuning knobs (ssa_amd_set_option)
    int strip_np = 16;                    // packed rows per strip (2*np query rows)
    int waves_per_block = 4;
    int force_wide = 0;                   // 1: score everything with the int64 kernel
    int sw_kernel = 0;                    // 0: f16-pattern kernel when applicable, 1: int16 kernel
    int no_filter = 0;                    // 1: copy every score back (no device top-k filter)
    int above_filter = 1;                 // ssa_amd_search_above: 1 (default) the device forwards the scores at or
                                          // above the threshold (above.hip); 0: every score back, the host scans
    int pair_np = 0;                      // pair kernel main strip: 2 x pair_np rows; 0 auto (engine.cpp pair_strip_np)
    int long_groups = -1;                 // leading groups scored by long_kernel: -1 auto, 0 never, N forced
    int long_share_pct = 50;              // auto: groups longer than this % of a SIMD's share of all columns
    int long_waves = 0;                   // waves per long entry: 0 auto, 4 (rows over a workgroup) or 1
    int long4_share_pct = 1500;           // auto: 4 waves for groups longer than this % of a SIMD's share
                                          // (400 until round 6: NW's Swiss-Prot form +11 % at 1500, engine.cpp)
    int long16 = 1;                       // SW long entries on packed 16-bit patterns (long16_kernel) when exact
    int upload_kernel = 1;                // 1: the per-search upload block is read from pinned memory by a kernel
                                          // on the search's stream instead of a copy-engine transfer (-14 us
                                          // between searches, profiles/r05/host_gap/kgap_upk*.txt)
    int tier_defer = 1;                   // single-view searches: the int32 re-score tier runs after the result's
                                          // copy, only when the search has overflowed lanes
    int tail_rows4 = 1;                   // pair kernel tail strips at 4-row granularity (default heights)
    int long_prio = 1;                    // long16 waves at raised issue priority (s_setprio 3)
    int long_pad = 1;                     // 1: long-entry workgroups pad their LDS to the pair kernel's (a finished
                                          // one leaves exactly a pair workgroup's hole); 0: their own LDS only
    int filter_onepass = 1;               // kernels.hip filter_onepass (0: three launches)
    int long_latency = 1;                 // engine.cpp long_plan: a tiny DB's groups all go to the long kernels
    int plan_cache = 1;                   // engine.cpp cached_plan (0: plan every search)
    int long_gate = 1;                    // the tables kernel holds the pair kernel until the long-entry
                                          // workgroups have started (TableArgs::gate)
    int long16_rows = 1;                  // long16_kernel may leave up to 8 query rows to its row scan (LongArgs::extra16)
    int pair_parts = 0;                   // pair_kernel: each group's strips in 2 dependent parts (StripArgs::nparts):
                                          // 0 auto (groups of >= 4 strips), 1 whole groups, 2 always
    int batch_fuse = 1;                   // ssa_amd_search_batch: queries of one pair-kernel plan in one launch
    int pair_ticket = 1;                  // pair_kernel workgroups take groups in start order (StripArgs::ticket)
    int rescore32 = 1;                    // overflowed lanes re-scored in int32 (long_kernel list mode) when exact
    long part_wait_us = 2000000;          // bound of a strip part's wait for its group's first part (then the
                                          // search runs again without parts; never a hang, never fatal)
    int timeline = 0;                     // record the DP waves' start/end (ssa_amd_get_timeline)
    int counters = -1;                    // the reference's 8/16-bit overflow counters: -1 auto (output mode
                                          // >= INFO, when m_run prints them), 0 never, 1 always
    int sync_spin = 1;                    // 1: hipDeviceScheduleSpin for this library's devices (set at the first
                                          // pack on a device): the host spins, not yields, while a search runs
                                          // (-15 us between searches, profiles/r05/host_gap/kgap_spin.txt)
    int lean_events = 1;                  // 1 (default): no timing markers around the upload, the tier and the filter
                                          // (stats upload_ms / wide_ms / d2h_ms stay 0; kernel_ms kept;
                                          // C2 +0.5 %, profiles/r05/ab/lean_events)
    int pairs_chunk = 0;                  // ssa_amd_score_pairs: pairs per pack / launch round; 0: by a byte budget
    int pairs_host = 0;                   // 1: every pair of ssa_amd_score_pairs on the exact host path
    int pairs_gather = 1;                 // ssa_amd_score_pairs_indexed: 1 (default) packs on the device from the
                                          // uploaded pools (pairs_gather.hip), 0 packs on the host
    int hits_gather = 1;                  // ssa_amd_summarize_hits: 1 (default) the hits' DB sides are packed on the
                                          // device from the packed DB (hits_gather.hip), 0 fetched through the plugin
                                          // and packed by ssa_amd_summarize_pairs_local
    int pairs_pool_mb = 1024;             // ... and packs on the host when the pools exceed this many MiB
    int pairs_wave = 0;                   // 1: ssa_amd_align_pairs aligns on the wave kernels, one wave per pair
                                          // (align_wave.cpp); 0: one pair per lane (pairs_align.cpp)
    int align_wave = 1;                   // COMPUTE_ALIGNMENT and ssa_amd_align_hits on the wave kernels; 0: host threads
    int align_wave_min = 1;               // ... for hit lists of at least this many hits
    int align_wave_rl = 0;                // the wave kernels' rows per lane: 0 by cost (align_wave.cpp pick_rl),
                                          // else one of align_wave.h's kWaveRL forced
    int topk_prune = 1;                   // SW top-k searches on the pair kernel skip the strip parts of groups
                                          // that can no longer reach the top-k (StripArgs::prune)
    int prune_inplace_pct = 25;           // a pruned search's work unit that cannot be skipped at a part boundary
                                          // runs its remaining parts itself, in the same workgroup, when its best
                                          // lane has reached this share (%) of what the rows so far can give at
                                          // most; 0: never (every later part as a work unit of its own)
    int prune_len = 1;                    // a pruned search skips a whole work unit none of whose entries is long
                                          // enough to reach the threshold (kernels.h kPruneLen; stats pruned_whole)
    int prune_promote = 1;                // a pruned search's part-0 unit that would finish in place scores its
                                          // promising entries exactly at once, one wave per entry, and defers its
                                          // later parts (kernels.h kPruneMask; stats promoted_lanes); 0: in place
    int prune_order = 1;                  // a pruned search starts the units whose entry lengths lie near the
                                          // query's alternately with the longest ones (engine.cpp prune_start_order);
                                          // only with prune_len
    int prune_order_pct = 25;             // ... within this many % of the query length
    int rare_merge = 0;                   // 1: when the query's residue classes leave the pair table too big for
                                          // three workgroups per CU, the rarest classes share one upper-bound
                                          // class and the forwarded entries holding them are re-scored exactly
                                          // (default off: Swiss-Prot form kernel +0.8 %, end to end -4 %,
                                          // profiles/r05/ab/merge_sprot2)
};
Config& cfg();
// whether a search computes the overflow counters (Config::counters)
inline bool counters_on(const Config& C) {
    return C.counters > 0 || (C.counters < 0 && C.output_mode >= OUTPUT_INFO);
}

// SSA_AMD_TRACE=1: per-search host/device timing lines on stderr
bool trace_on();

// --------------------------------------------------------------- messages
// Same channels and prefixes as the reference (util.c:36-89): errors and
// warnings and infos go to stdout gated by the output mode, fatal goes to
// stderr and exits with status 1.
[[noreturn]] void fatal(const char* fmt, ...);
void print_info(const char* fmt, ...);
void print_warning(const char* fmt, ...);
void print_error(const char* fmt, ...);

// --------------------------------------------------------------- alphabets
extern const signed char* map_aa();   // 256-entry ASCII -> code, -1 unknown
extern const signed char* map_nt();
uint8_t nt_complement(uint8_t code);
void revcompl(const uint8_t* in, size_t len, uint8_t* out);
void init_translation(int q_gencode, int d_gencode);
bool gencode_valid(int code);
// translate mapped NT codes, strand 0 = forward, 1 = reverse complement
std::vector<uint8_t> translate(bool db_side, const uint8_t* dna, size_t len, int strand, int frame);

// ----------------------------------------------------------------- matrix
struct Matrix {
    bool ready = false;
    bool constant = false;                // reference never clears this flag
    int64_t m[kDim * kDim];
};
Matrix& matrix();
void matrix_builtin(const char* name);
void matrix_from_string(const char* text);
void matrix_from_file(const char* path);
void matrix_constant(int match, int mismatch);
void matrix_free();

// ------------------------------------------------------------------ query
struct SeqBuf {
    std::vector<uint8_t> seq;   // codes, plus a trailing 0 kept for C callers
    size_t len() const { return seq.empty() ? 0 : seq.size() - 1; }
};
}  // namespace ssa

struct _query {
    ssa::SeqBuf nt[2];
    ssa::SeqBuf aa[6];
    std::string header;
    int symtype;
};

namespace ssa {
struct QueryView {                // one search "query buffer" (searcher.c:42-90)
    const uint8_t* seq;
    size_t len;
    int strand, frame;
    char* cseq;                   // pointer handed out in q_seq_t.seq
    // a profile view (ssa_amd_search_profile): seq == nullptr and `len` position
    // rows of 32 scores, prof[i * 32 + c] = DB residue code c at query row i
    const int32_t* prof = nullptr;
};
std::vector<QueryView> query_views(p_query q);
}  // namespace ssa

// a position-specific scoring matrix (ssa_amd_profile_create)
struct ssa_amd_profile {
    std::vector<int32_t> rows;    // [nrows][32]
    size_t nrows = 0;
};

namespace ssa {
// profile.cpp: ssa_amd_profile_score_host, the profile recurrences' definition
int profile_score_host(const ssa_amd_profile* p, int algo, const uint8_t* d_codes, const uint64_t* d_off, size_t n,
                       int64_t* scores);

// ---------------------------------------------------------------- top-k
struct Hit {
    int64_t score;
    uint64_t id;
    uint8_t qid, strand, frame;
};
// Reference min-heap (minheap.c:50-106) with exact tie behaviour.
class TopK {
public:
    explicit TopK(size_t k) : k_(k) { a_.reserve(k); }
    // returns true when the element entered the heap
    bool add(const Hit& h);
    size_t size() const { return a_.size(); }
    bool full() const { return a_.size() >= k_; }
    int64_t root_score() const { return a_.empty() ? INT64_MIN : a_[0].score; }
    // an element scoring what the root scores now was evicted: which of the
    // elements tied at the k-th score remain then depends on the heap's
    // layout, i.e. on every lower score fed before
    bool tie_evicted() const { return !a_.empty() && evicted_max_ == a_[0].score; }
    std::vector<Hit> sorted() const;
private:
    size_t k_;
    std::vector<Hit> a_;
    int64_t evicted_max_ = INT64_MIN;     // largest score ever evicted (they only grow)
};
void sort_hits(std::vector<Hit>& v);   // score desc, id desc (util.h:12)

// ------------------------------------------------------ COMPUTE_ALIGNMENT
// align.cpp: region {q begin, q end, db begin, db end} and CIGAR of a pair
std::string traceback(int algo, const uint8_t* q, size_t qn, const uint8_t* d, size_t dn, size_t region[4]);
void compute_alignments(p_alignment_list L, int algo);
void compute_alignments_host(p_alignment_list L, int algo);   // ... on host threads, one hit per thread
// align_wave.cpp: the wave aligner (one wave per pair on the device).  Region, CIGAR length, flags (and the
// score when asked for) of every item go to out[i], the NUL-terminated text to items[i].text (qlen + dlen + 1
// bytes); device < 0: ssa_amd_set_device's, else the current one
struct WaveItem {
    const uint8_t* q;
    size_t qlen;
    const uint8_t* d;
    size_t dlen;
    char* text;
};
void align_wave(int algo, const WaveItem* items, size_t n, int device, bool allow_device, bool want_score,
                ssa_amd_pair_alignment_t* out, ssa_amd_align_pairs_stats_t& stats);
void align_hits(p_alignment_list L, int algo);                // compute_alignments' body
const ssa_amd_align_pairs_stats_t& align_hits_stats();

// ------------------------------------------------------------ pair batches
// pairs.cpp: ssa_amd_score_pairs and its statistics
int score_pairs(int algo, const uint8_t* q_codes, const uint64_t* q_off, const uint8_t* d_codes, const uint64_t* d_off,
                size_t npairs, int64_t* scores);
const ssa_amd_pairs_stats_t& pairs_stats();
// pairs.cpp: ssa_amd_score_pairs_indexed (the same statistics)
int score_pairs_indexed(int algo, const uint8_t* q_codes, const uint64_t* q_off, size_t nq, const uint8_t* d_codes,
                        const uint64_t* d_off, size_t nd, const uint32_t* q_idx, const uint32_t* d_idx, size_t npairs,
                        int64_t* scores);
// pairs_align.cpp: ssa_amd_align_pairs and its statistics
int align_pairs(int algo, const uint8_t* q_codes, const uint64_t* q_off, const uint8_t* d_codes, const uint64_t* d_off,
                size_t npairs, ssa_amd_pair_alignment_t* out, char* cigars, size_t cigar_cap);
const ssa_amd_align_pairs_stats_t& align_pairs_stats();
// pairs_ends.cpp: ssa_amd_score_pairs_ends / ssa_amd_align_pairs_ends; they report through the two
// statistics above (set_*: pairs.cpp, pairs_align.cpp)
int score_pairs_ends(int ends, const uint8_t* q_codes, const uint64_t* q_off, const uint8_t* d_codes,
                     const uint64_t* d_off, size_t npairs, int64_t* scores);
int align_pairs_ends(int ends, const uint8_t* q_codes, const uint64_t* q_off, const uint8_t* d_codes,
                     const uint64_t* d_off, size_t npairs, ssa_amd_pair_alignment_t* out, char* cigars,
                     size_t cigar_cap);
// pairs_banded.cpp: ssa_amd_score_pairs_banded / ssa_amd_align_pairs_banded; the same two statistics
int score_pairs_banded(int ends, const int64_t* band_lo, const int64_t* band_hi, const uint8_t* q_codes,
                       const uint64_t* q_off, const uint8_t* d_codes, const uint64_t* d_off, size_t npairs,
                       int64_t* scores);
int align_pairs_banded(int ends, const int64_t* band_lo, const int64_t* band_hi, const uint8_t* q_codes,
                       const uint64_t* q_off, const uint8_t* d_codes, const uint64_t* d_off, size_t npairs,
                       ssa_amd_pair_alignment_t* out, char* cigars, size_t cigar_cap);
// pairs_local.cpp: ssa_amd_score_pairs_local / ssa_amd_align_pairs_local; the same two statistics
int score_pairs_local(int mode, const int64_t* band_lo, const int64_t* band_hi, const uint8_t* q_codes,
                      const uint64_t* q_off, const uint8_t* d_codes, const uint64_t* d_off, size_t npairs,
                      int64_t* scores);
int align_pairs_local(int mode, const int64_t* band_lo, const int64_t* band_hi, const uint8_t* q_codes,
                      const uint64_t* q_off, const uint8_t* d_codes, const uint64_t* d_off, size_t npairs,
                      ssa_amd_pair_alignment_t* out, char* cigars, size_t cigar_cap);
// pairs_summary.cpp: ssa_amd_summarize_pairs_local; it reports through the align statistics
int summarize_pairs_local(int mode, const int64_t* band_lo, const int64_t* band_hi, const uint8_t* q_codes,
                          const uint64_t* q_off, const uint8_t* d_codes, const uint64_t* d_off, size_t npairs,
                          ssa_amd_pair_summary_t* out);
// pairs_xdrop.cpp: ssa_amd_score_pairs_xdrop / ssa_amd_align_pairs_xdrop / ssa_amd_summarize_pairs_xdrop; the
// same statistics, and the pairs of the last such call that met a drop row
int score_pairs_xdrop(int mode, int64_t xdrop, const int64_t* band_lo, const int64_t* band_hi, const uint8_t* q_codes,
                      const uint64_t* q_off, const uint8_t* d_codes, const uint64_t* d_off, size_t npairs,
                      int64_t* scores);
int align_pairs_xdrop(int mode, int64_t xdrop, const int64_t* band_lo, const int64_t* band_hi, const uint8_t* q_codes,
                      const uint64_t* q_off, const uint8_t* d_codes, const uint64_t* d_off, size_t npairs,
                      ssa_amd_pair_alignment_t* out, char* cigars, size_t cigar_cap);
int summarize_pairs_xdrop(int mode, int64_t xdrop, const int64_t* band_lo, const int64_t* band_hi,
                          const uint8_t* q_codes, const uint64_t* q_off, const uint8_t* d_codes, const uint64_t* d_off,
                          size_t npairs, ssa_amd_pair_summary_t* out);
uint64_t xdrop_dropped();
// hits_summary.cpp: ssa_amd_summarize_hits; it reports through the align statistics and its own
int summarize_hits(p_query query, int mode, const ssa_hit_t* hits, size_t n, ssa_amd_pair_summary_t* out);
const ssa_amd_hits_stats_t& summarize_hits_stats();
void set_pairs_stats(const ssa_amd_pairs_stats_t& s);
void set_align_pairs_stats(const ssa_amd_align_pairs_stats_t& s);

}  // namespace ssa
