/*
 * libssa_amd.h -- MI355X-specific extensions to the libssa C ABI.
 *
 * Everything in libssa.h works unchanged; these entry points add what a
 * sharded, multi-GPU deployment needs and what the benchmark measures:
 *
 *   - ssa_amd_search(..., SSA_AMD_LOG) scores the locally opened DB (a shard
 *     whose IDs start at ssa_amd_set_id_offset()) and returns its top-k
 *     INSERTION LOG: the exact subset of (score, id) pairs that the
 *     reference's min-heap (src/util/minheap.c:75-91) would ever accept when
 *     fed this shard in ID order.  Any element the global heap accepts is in
 *     its shard's log, so concatenating the logs in shard order and calling
 *     ssa_amd_replay() reproduces the 64-bit single-thread reference result
 *     bit for bit, including the IDs chosen among equal scores.  Logs are a
 *     few hundred elements, so one gather over RCCL/xGMI is all the
 *     cross-GPU traffic a search needs.
 *   - ssa_amd_get_stats() exposes HIP-event kernel times and counters.
 */
#ifndef LIBSSA_AMD_H_
#define LIBSSA_AMD_H_

#include <stdint.h>
#include <stddef.h>
#include "libssa.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int64_t score;
    uint64_t db_id;      /* global DB ID (local ID + id offset) */
    uint8_t query_id;    /* index into the query's strand/frame buffers */
    uint8_t db_strand;
    uint8_t db_frame;
    uint8_t pad[5];
} ssa_hit_t;             /* 24 bytes, like the reference's elem_t */

typedef struct {
    double search_ms;    /* host wall time of the last search call */
    double kernel_ms;    /* HIP-event time of the int16 strip kernels */
    double wide_ms;      /* HIP-event time of the exact re-score tier (0 under option "lean_events") */
    double d2h_ms;       /* device filter + result copy (HIP events; 0 under "lean_events") */
    double replay_ms;    /* host top-k replay */
    double pack_ms;      /* DB packing + upload (only when the DB changed) */
    uint64_t cells;      /* sum over queries of qlen * sum of entry lengths */
    uint64_t entries;    /* DB entries scored per query */
    uint64_t overflow_8; /* reference-style counters (manager.c:157-160) */
    uint64_t overflow_16;
    uint64_t wide_count; /* entries re-scored exactly by the int64 kernel */
    uint32_t kernel_launches;
    int32_t device;
    uint64_t kernel_bytes;   /* algorithmic HBM bytes of the strip kernels */
    char kernel[32];         /* main scoring kernel of the last search, e.g. "pair_f16_sw" */
    double prep_ms;          /* host work before the first kernel launch (profiles, uploads) */
    double upload_ms;        /* device time of the per-search uploads before the first kernel (0 under
                                option "lean_events") */
    double sync_wait_ms;     /* host time blocked in the final stream synchronisation */
    uint32_t strip_rows;     /* pair kernel: rows of its main strips (2 x "pair_np"); 0: other kernels */
    uint32_t counters;       /* 1: overflow_8/16 were computed (bit width 64, output mode >= OUTPUT_INFO
                                or option "counters" 1); 0: not computed, they read 0 */
    uint32_t long_entries;   /* lanes (64 per group) of the longest groups scored by a long-entry kernel (view 0) */
    char long_kernel[24];    /* that kernel: "long16_rl<R>" (packed 16-bit SW), "long32_w<W>_rl<R>" (int32;
                                "+"-joined when split over two launches), "" none */
    uint32_t part_retries;   /* searches run again without strip parts because a part's wait for its
                                group's first part ran into option "part_wait_us" (results unaffected) */
    /* running totals since the library was loaded (never reset): a caller
     * times N searches by two reads, with no call between the searches */
    uint64_t total_searches;
    double total_kernel_ms;  /* sum of kernel_ms */
    double total_search_ms;  /* sum of search_ms */
    uint64_t filter_candidates;  /* scores of the last search the device top-k filter let through to
                                    the host (every score when it ran without the filter) */
    double gather_ms;        /* host wall time of this rank's last ssa_amd_gather_logs (staging, the
                                collective, rank 0's replay) */
    uint32_t gather_rounds;  /* 1: the slot gather alone; 2: this rank also sent (or rank 0 received)
                                log rows beyond the 512-row slot point to point */
    uint32_t rare_merged;    /* DB residue codes the last search scored through one upper-bound class
                                (option "rare_merge"; 0: none) */
    uint32_t rare_rescored;  /* entries holding one of them that the device filter forwarded and the
                                int32 tier re-scored exactly */
    uint32_t slots;          /* device slots of the last search (1: one device; more: SSA_AMD_DEVICES or
                                ssa_amd_set_devices, one host thread per slot) */
    int32_t slot_device[16];     /* per slot: its HIP device */
    double slot_kernel_ms[16];   /* per slot: HIP-event time of its DP kernels */
    double slot_search_ms[16];   /* per slot: host time of its device search and shard replay */
    uint32_t part_units;     /* pair kernel strip parts: work units of second and later parts in the last
                                search's launch (0: the groups ran whole) */
    uint32_t pruned_units;   /* of those, skipped because no entry of theirs could still reach the top-k
                                (option "topk_prune"; scores and hits unaffected) */
    uint32_t inplace_units;  /* work units of a pruned search that ran their remaining parts themselves, in the
                                same workgroup, instead of leaving them to later units (option
                                "prune_inplace_pct"); the later units of their groups return at once and
                                are not counted as pruned */
    uint32_t pruned_first;   /* of pruned_units, those skipped at the first part boundary */
} ssa_amd_stats_t;

typedef struct {
    uint64_t pairs;        /* pairs of the last ssa_amd_score_pairs call */
    uint64_t cells;        /* sum of qlen * dlen */
    uint64_t swept_cells;  /* cells the waves walked: padding lanes, rows and columns included
                              (cells of device pairs / swept_cells = the packing efficiency) */
    uint64_t host_pairs;   /* pairs scored on the host: the exact int64 path and empty-side pairs */
    uint32_t groups;       /* groups of 64 pairs, one per wave */
    uint32_t chunks;       /* pack / upload / launch / copy rounds (option "pairs_chunk") */
    uint32_t launches;     /* kernel launches */
    uint32_t strip_rows;   /* query rows per strip of pairs_kernel */
    double total_ms;       /* host wall time of the call */
    double pack_ms;        /* host: ordering and lane-interleaved packing */
    double kernel_ms;      /* HIP-event time of the kernel launches */
    double host_ms;        /* host wall time of the exact host path */
    int32_t device;        /* HIP device of the call, -1: none used */
    char kernel[32];       /* "pairs_sw_i32" / "pairs_nw_i32" */
    double gather_ms;      /* ssa_amd_score_pairs_indexed on its gather path: HIP-event time of the
                              pairs_gather_kernel launches (they count in `launches`); else 0 */
    uint64_t pool_bytes;   /* ... and the bytes of sequence pool the call uploaded; else 0 */
} ssa_amd_pairs_stats_t;

/* One pair's result of ssa_amd_align_pairs. */
typedef struct {
    int64_t  score;       /* what ssa_amd_score_pairs reports for the pair */
    uint64_t region[4];   /* q begin, q end, d begin, d end -- exactly ssa_amd_align_pair's */
    uint64_t cigar_off;   /* NUL-terminated CIGAR at cigars + cigar_off */
    uint32_t cigar_len;
    uint32_t flags;       /* bit 0: aligned on the host path */
} ssa_amd_pair_alignment_t;

typedef struct {
    uint64_t pairs;        /* pairs of the last ssa_amd_align_pairs call */
    uint64_t cells;        /* sum of qlen * dlen */
    uint64_t host_pairs;   /* pairs aligned on the host (device_fallbacks included) */
    uint64_t zero_pairs;   /* device SW pairs whose best score is 0: region zeros, empty CIGAR */
    uint64_t device_fallbacks; /* device pairs a pass gave no cell for, handed to the host routine (expected 0) */
    uint64_t dir_bytes;    /* direction bits written on the device, all chunks */
    uint32_t groups;       /* groups of 64 pairs, one per wave */
    uint32_t chunks;       /* pack / upload / launch / copy rounds */
    uint32_t launches;     /* kernel launches */
    uint32_t reserved;
    double total_ms;       /* host wall time of the call */
    double pack_ms;        /* host: ordering and packing, the work between two passes included */
    double host_ms;        /* host wall time of the host path */
    double text_ms;        /* host: runs -> CIGAR text */
    double fwd_ms;         /* HIP-event time per pass: SW forward (the end cell) */
    double rev_ms;         /*   SW reverse (the begin cell) */
    double dir_ms;         /*   directions */
    double walk_ms;        /*   the walk */
    double kernel_ms;      /* fwd_ms + rev_ms + dir_ms + walk_ms */
    int32_t device;        /* HIP device of the call, -1: none used */
    char kernels[96];      /* the kernels of the call, comma-separated */
} ssa_amd_align_pairs_stats_t;

#define SSA_AMD_SW 0
#define SSA_AMD_NW 1
#define SSA_AMD_TOPK 0      /* sorted top-k, as sw_align/nw_align */
#define SSA_AMD_LOG 1       /* insertion log in replay order */

/* Devices.  An unchanged libssa caller searches on every visible GPU, as
 * the reference uses every core by default (src/util/thread_pool.c:42,
 * get_nprocs()): at the first init_db, unless ssa_amd_set_device(s) was
 * called before, the library reads the environment variable
 *   SSA_AMD_DEVICES = all (also: unset or empty) | current | 0,2,...
 * -- every visible device, the current HIP device only, or this list
 * (repeats allowed: several slots on one device).  Several devices work as
 * ssa_amd_set_devices below.  set_thread_count(n) (libssa.h: the reference's
 * number of search workers) caps that list at its first n devices (0: all),
 * so the reference's thread sweeps become device sweeps.  An explicit
 * ssa_amd_set_device(s) always wins (one rank per GPU:
 * ssa_amd_set_device(local_rank)) and no thread count changes it. */
int ssa_amd_device_count( void );
void ssa_amd_set_device( int device );
void ssa_amd_set_id_offset( size_t offset );
/* Search on several devices from this one process (one persistent host
 * thread per device slot inside sw_align / nw_align -- the caller's thread
 * drives slot 0 -- the DB split into contiguous record ranges at chunk_size
 * boundaries, balanced by residues, the slots' insertion logs merged in
 * slot order; results identical to a single device).  n = 0 returns to
 * single-device mode (ssa_amd_set_device).  Returns 0, or 1 for an invalid
 * device list. */
int ssa_amd_set_devices( const int * devices, int n );
/* The device slots the next search uses (after SSA_AMD_DEVICES, which is
 * read here if init_db has not read it yet): writes up to cap device ids to
 * out (may be NULL) and returns the slot count. */
int ssa_amd_get_devices( int * out, int cap );
int ssa_amd_prepare_db( void );            /* pack + upload the DB now; returns 0 on success */
void ssa_amd_get_stats( ssa_amd_stats_t * out );
/* One more figure of the last search, beside ssa_amd_stats_t (whose layout is
 * kept as it is): the work units of a pruned search skipped before their first
 * part because no entry of theirs is long enough to reach the top-k threshold
 * (option "prune_len"); their later units return at once and are not counted in
 * pruned_units.  A batch reports the sum. */
uint32_t ssa_amd_get_pruned_whole( void );
/* ... and the entries of a pruned search that were scored exactly, one wave
 * each, at the first part boundary instead of in place (option
 * "prune_promote").  A batch reports the sum. */
uint32_t ssa_amd_get_promoted_lanes( void );
/* Tuning knobs (results never change, only which kernel computes them):
 *   "strip_np" 8|16|32   int16 strip kernels: packed rows per strip
 *   "pair_np" 0|16|24|32|36|40  pair kernel main strip of 2 x pair_np rows; 0 (default):
 *                        SW 24, NW the tallest of 40/32/24 whose pair table lets
 *                        two workgroups share a CU (36 is SW only)
 *   "sw_kernel" 0|1      1: int16 strip kernel instead of the pair kernel
 *   "force_wide" 0|1     1: every entry through the int64 kernel
 *   "no_filter" 0|1      1: copy every score back (no device top-k filter)
 *   "above_filter" 1|0   ssa_amd_search_above: 1 (default) the device forwards only the scores at or
 *                        above the threshold; 0: every score is copied back and the host scans them
 *                        (the same list; also what "no_filter" 1 or a query view without rows gets)
 *   "long_groups" -1|0|N leading groups scored one entry per wave: auto, never, N
 *   "long_share_pct" P   auto threshold: P % of one SIMD's share of all columns
 *   "long_waves" 0|4|1   waves scoring one long entry (its query rows split over
 *                        them): auto (4 for groups beyond "long4_share_pct", 1
 *                        for the rest), always 4, always 1
 *   "long4_share_pct" P  auto: 4 waves per entry for groups longer than P % of
 *                        one SIMD's share of all columns (default 1500: where one
 *                        wave's latency would outlast the pair kernel)
 *   "long16" 1|0         SW long entries on packed 16-bit patterns, one wave
 *                        per entry, whenever min(m, n) x max score fits (default);
 *                        0: the int32 kernel ("long_waves" applies to it)
 *   "filter_prefix_regs" 1|0  the top-k filter's block scan with its states in registers and
 *                        merges at the list width k needs, for DBs of <= 256 filter blocks
 *                        (default), or always the general scan
 *   "upload_kernel" 1|0  1 (default): the per-search upload block (matrix, boundary, query) is read
 *                        from pinned host memory by a kernel on the search's stream; 0: a
 *                        copy-engine transfer (hipMemcpyAsync)
 *   "tier_defer" 1|0     single-view searches: the exact re-score tier runs only when the device
 *                        filter's header reports overflowed lanes, after the result's copy
 *                        (default 1); 0: always, between the DP kernels and the filter
 *   "tail_rows4" 1|0     the pair kernel's last strip at 4-row granularity (default; SW 48-row and
 *                        NW 64/80-row strips, after a main strip), or 8-row (0)
 *   "long_prio" 1|0      long16 waves at raised issue priority over the pair waves (default 1)
 *   "long_pad" 1|0       long-entry workgroups pad their LDS to the pair kernel's, so a finished one
 *                        leaves a pair workgroup's hole (default 1; 0 measured -6 % on the Swiss-Prot form)
 *   "filter_onepass" 1|0 the device top-k filter as one launch (a decoupled look-back over its
 *                        blocks; default 1) or as three (block maxima, prefix, select)
 *   "long_latency" 1|0   a DB of at most 256 groups (16 384 entries), a query of two strips or more:
 *                        every group goes to the long-entry kernels when their throughput estimate
 *                        beats the pair wave's latency (default 1; one 513-residue entry, q = 390:
 *                        SW 1.48 -> 0.14 ms); 0: the length rules alone
 *   "plan_cache" 1|0     a search with the query and settings of one of the last four reuses
 *                        their plan (residue classes, bounds, strips; default 1); 0: plan each search
 *   "long_gate" 1|0|P    the pair kernel starts after the long-entry workgroups have (default 1;
 *                        0: no wait, the long-entry streams' priority alone orders them; 2..99:
 *                        after the first P % of them)
 *   "long16_rows" 1|0|2  queries beyond 1 024 rows: long16 passes planned by issue cost, up to 8
 *                        last rows scored by a row scan (default 1); 0: RL 16 passes; 2: the
 *                        cost model at every query length (q = 513: RL 8 + 1 scanned row)
 *   "timeline" 0|1       1: record every DP wave's start/end (ssa_amd_get_timeline)
 *   "pair_ticket" 1|0    pair-kernel workgroups take the next groups in start order
 *                        (an atomic ticket; default) or in blockIdx order
 *   "pair_parts" 0|1|2|3 pair-kernel groups run as 2 (or 3) dependent work units of
 *                        consecutive strips (all groups' first parts, then all second
 *                        parts, ...), so the launch ends on small units: 0 (default) 2
 *                        for groups of at least 4 strips, 1 never, 2 always, 3 three
 *   "rescore32" 1|0      entries the DP kernels cannot score exactly (overflow) are re-scored
 *                        by the int32 long-entry kernel, one wave per entry, whenever int32 is
 *                        exact for the DB (default); 0: always the int64 kernel
 *   "part_wait_us" N     bound of a strip part's wait for its group's first part (default
 *                        2000000); a timed-out wait makes the search run again without parts
 *                        (stats part_retries), results unchanged
 *   "topk_prune" 1|0     1 (default): a single-query SW top-k search (sw_align, ssa_amd_search TOPK; width
 *                        16 or 64, k <= 64, one device) whose groups run as strip parts skips the
 *                        later parts of every work unit whose entries provably stay below the k-th
 *                        best score (stats part_units / pruned_units); hits are identical; 0: never
 *   "prune_inplace_pct" N  a pruned search's work unit that cannot be skipped at a part boundary runs
 *                        its remaining parts itself, at once, when its best entry so far has reached
 *                        N % (default 25) of the most the query rows so far can score; 0: never.
 *                        Changes the schedule only, never a score (stats inplace_units)
 *   "prune_promote" 1|0  1 (default): a work unit that would run its remaining parts itself scores its
 *                        promising entries (up to 8 per 64, queries of up to 512 rows) exactly at once
 *                        instead, one wave per entry, so the k-th best score is known early, and leaves
 *                        its later parts to the ordinary skip (ssa_amd_get_promoted_lanes); 0: in place.
 *                        Changes the schedule only, never a score
 *   "prune_len" 1|0      1 (default): a pruned search skips a whole work unit, before its first row, when
 *                        none of its entries is long enough to reach the current k-th best score
 *                        (ssa_amd_get_pruned_whole); hits are identical
 *   "prune_order" 1|0    1 (default): a pruned search starts the work units whose entry lengths lie
 *                        within "prune_order_pct" % (default 25) of the query's length alternately
 *                        with the longest ones, instead of longest first (only with "prune_len" on).  The schedule only
 *   "rare_merge" 0|1     1 (default 0): when a query's residue classes leave the pair table too big
 *                        for three workgroups per CU, the rarest classes share one class scoring
 *                        the maximum of their rows, and the entries holding them that the device
 *                        filter forwards are re-scored exactly (stats rare_merged / rare_rescored)
 *   "sync_spin" 1|0      1 (default): the host thread spins while a search runs (hipDeviceScheduleSpin,
 *                        set at the library's first pack on a device; 15 us less between two
 *                        searches); 0: HIP's own scheduling (yields the core).  The flag is
 *                        PROCESS-WIDE for that device: every HIP user of the process (e.g. torch)
 *                        then spins in its own synchronisations too, and a search keeps one host
 *                        core busy for its whole duration.  It only takes effect when the library
 *                        is the first to use the device in the process (a context made before keeps
 *                        its flags); set 0 before the first init_db to leave the flags alone
 *   "lean_events" 1|0    1 (default): no timing markers around the upload, the re-score tier
 *                        and the filter (stats upload_ms, wide_ms, d2h_ms read 0; kernel_ms
 *                        kept; C2 +0.5 %, profiles/r05/ab/lean_events); 0: all markers
 *   "counters" -1|0|1    the reference's 8/16-bit overflow counters (stats overflow_8/16,
 *                        m_run's INFO line): -1 (default) only at output mode
 *                        OUTPUT_INFO, where the reference prints them; 0 never; 1 always
 * Unknown names print a warning. */
void ssa_amd_set_option( const char * name, long value );

/* The last search's wave timeline (option "timeline"; of the last query view
 * for multi-view searches): rows of 4 uint32 --
 *   pair_kernel: (group, start, end, place); long_kernel: (0x80000000 | lane
 *   of its entry, start, end, place)
 * start/end in s_memrealtime ticks (100 MHz, low 32 bits), place = XCC << 16 |
 * HW_ID[15:0].  Rows never written stay zero.  Copies at most cap rows to out
 * (may be NULL) and returns the row count.  A profiling aid (tools/timeline.py),
 * not part of the reference's interface. */
size_t ssa_amd_get_timeline( uint32_t * out, size_t cap );

/* The order in which a pruned search (option "topk_prune") starts its first
 * work units (option "prune_order"), as the library plans it: ncols[ngroups]
 * are the column counts of the launch's 64-entry groups, longest first, a unit
 * is four consecutive groups, qlen the query's length and pct the window
 * (option "prune_order_pct"), of which at most `most` units, the nearest to qlen,
 * are moved ahead (0: all; a search passes half of what the device holds at
 * once).  Writes at most cap unit indices to out (may be
 * NULL) and returns the unit count.  Host code only: no device, no DB.  A
 * testing aid, not part of the reference's interface. */
size_t ssa_amd_prune_start_order( const uint32_t * ncols, size_t ngroups, size_t qlen, unsigned pct,
                                  unsigned most, uint32_t * out, size_t cap );

/* Scores the open DB against the query.  mode: SSA_AMD_TOPK or SSA_AMD_LOG.
 * Returns the number of hits written (at most cap; the log never exceeds
 * the number of DB entries). */
size_t ssa_amd_search( p_query query, int algo, size_t hitcount, int bit_width, int mode,
                       ssa_hit_t * out, size_t cap );

/* Several queries against the open DB in one call.
 * Query i's sorted top-k goes to out[i * hitcount ...], its length to
 * counts[i]; returns the total.  Each query is exactly sw_align/nw_align's
 * result.  The DB is packed once and stays in HBM; per query the library
 * adds ~0.1 ms of fixed work (profile upload, filter, replay) to the DP,
 * which is VALU-bound, so there is no DB streaming for a batch to amortise
 * (DESIGN.md §7). */
size_t ssa_amd_search_batch( const p_query * queries, size_t nq, int algo, size_t hitcount, int bit_width,
                             ssa_hit_t * out, size_t * counts );

/* Every (query view, DB entry) of the open DB whose exact score is >= min_score
 * -- where the calls above return the k best.  algo: SSA_AMD_SW or SSA_AMD_NW;
 * bit_width as in ssa_amd_search (scores are exact at every width, the width
 * only decides the overflow counters).  Each hit's score is what sw_align /
 * nw_align report for that (view, entry), db_id is global
 * (ssa_amd_set_id_offset), query_id / db_strand / db_frame as ssa_amd_search
 * fills them.  *total (may be NULL) receives the number of qualifying hits;
 * the return value is the number written, min(total, cap): the FIRST cap hits
 * of the full list in the order
 *   score descending, then db_id descending (sw_align's order: the list
 *   continues a top-k list), then query_id, db_strand, db_frame ascending.
 * out == NULL or cap == 0 counts only.  min_score is any int64 (NW thresholds
 * may be negative); SW with min_score <= 0 returns every entry, a threshold
 * above every score returns 0.  A NULL query and configuration errors behave
 * as in ssa_amd_search.  The call never prunes and never merges rare codes
 * (stats pruned_units, inplace_units, pruned_first, rare_merged and
 * ssa_amd_get_pruned_whole() read 0; part_units may not): every score it
 * compares is exact.  ssa_amd_get_stats reports it as a search;
 * filter_candidates is the number of (position, score) pairs that crossed PCIe
 * (option "above_filter").  With several device slots (ssa_amd_set_devices,
 * SSA_AMD_DEVICES) each searches its shard and the lists are merged: the
 * result is that of one device. */
size_t ssa_amd_search_above( p_query query, int algo, int64_t min_score, int bit_width,
                             ssa_hit_t * out, size_t cap, size_t * total );

/* Host only: the threshold, order and cut of ssa_amd_search_above applied to
 * any n hits -- the concatenated lists of a sharded caller's ranks, each
 * searched with its own ssa_amd_set_id_offset (the counterpart of
 * ssa_amd_replay for threshold lists).  No device and no DB are involved.
 * Returns the number written, min(*total, cap); out == NULL or cap == 0
 * counts only. */
size_t ssa_amd_merge_above( const ssa_hit_t * hits, size_t n, int64_t min_score,
                            ssa_hit_t * out, size_t cap, size_t * total );

/* Profile search: a position-specific scoring matrix (PSSM) in the query's
 * place.  A profile has one row of 32 residue scores per query
 * position, where a sequence query has one residue.
 *
 * Recurrence and conventions: exactly sw_align's / nw_align's (the reference's
 * full_sw / full_nw, affine gaps, the current init_gap_penalties), with the
 * substitution score M[d_j][q_i] replaced by scores[i * 32 + d_j].  The
 * empty-DB-entry conventions are unchanged (SW 0; such records are no entries
 * of a search).  The matrix set by init_score_matrix / init_constant_scores is
 * NOT read and need not be initialised.  There is no bit width: scores are
 * exact, as at every width of the sequence calls, and the reference's 8/16-bit
 * overflow counters are not computed (stats counters, overflow_8 and
 * overflow_16 read 0).
 *
 * Not done for a profile view (each may be lifted later): top-k pruning and
 * promotion, the rare-code merge, fused batches and the overflow-counter
 * kernels -- stats pruned_units, inplace_units, pruned_first, rare_merged,
 * ssa_amd_get_pruned_whole() and ssa_amd_get_promoted_lanes() read 0.
 * Alignments (CIGARs, ssa_amd_align_hits, ssa_amd_summarize_hits) are not
 * offered for profile hits. */
typedef struct ssa_amd_profile * p_ssa_profile;

/* rows >= 1 position rows of 32 scores: scores[i * 32 + c] is the score of DB residue code c
 * (a DB-side mapped code of the symbol type in force, what ssa_amd_map_residues writes; 0..31)
 * at query position i.  Every value must lie in [-32768, 32767].  The scores are copied.
 * NULL for scores == NULL, rows == 0, or a value out of range. */
p_ssa_profile ssa_amd_profile_create( const int32_t * scores, size_t rows );
/* The profile a sequence query IS under the current matrix: row i = M[c][q_i] for view `view`
 * of `query` (ssa_amd_query_views' order).  NULL for a NULL query, a bad view, an empty view,
 * or a matrix value outside [-32768, 32767]. */
p_ssa_profile ssa_amd_profile_from_query( p_query query, size_t view );
size_t ssa_amd_profile_rows( p_ssa_profile p );     /* 0 for NULL */
void   ssa_amd_profile_free( p_ssa_profile p );     /* NULL is allowed */

/* Host only, no device, no DB: the definition.  scores[e] of profile p against the n sequences
 * d_codes[d_off[e] .. d_off[e+1]), int64, algo SSA_AMD_SW / SSA_AMD_NW, current gap penalties,
 * on set_thread_count threads.  An empty sequence scores 0 (SW) or the boundary value
 * gap_open + rows * gap_extend (NW).
 * Non-zero (nothing written) for NULL arguments with n > 0, decreasing offsets, a code >= 32
 * or an unknown algo. */
int ssa_amd_profile_score_host( p_ssa_profile p, int algo, const uint8_t * d_codes,
                                const uint64_t * d_off, size_t n, int64_t * scores );

/* ssa_amd_search / ssa_amd_search_above with a profile in the query's place.  A profile is one
 * query view: every hit's query_id is 0; db_id, db_strand and db_frame are filled as
 * ssa_amd_search fills them, for every entry the open DB has (AMINOACID, NUCLEOTIDE with one or
 * both strands, TRANS_DB).  A symbol type that translates the query (TRANS_QUERY, TRANS_BOTH)
 * has no meaning for a profile: the call prints a warning and returns 0 with nothing launched,
 * and so does a NULL profile.  Orders and modes are the sequence calls': SSA_AMD_TOPK's order and
 * tie IDs are the reference heap replay, SSA_AMD_LOG is the insertion log (ssa_amd_replay,
 * ssa_amd_merge_logs and ssa_amd_gather_logs work on it unchanged), the threshold order is
 * ssa_amd_search_above's (ssa_amd_merge_above works on its lists), and several device slots
 * give the single-device result.  ssa_amd_get_stats reports the call as a search. */
size_t ssa_amd_search_profile( p_ssa_profile p, int algo, size_t hitcount, int mode,
                               ssa_hit_t * out, size_t cap );
size_t ssa_amd_search_profile_above( p_ssa_profile p, int algo, int64_t min_score,
                                     ssa_hit_t * out, size_t cap, size_t * total );
/* Bytes the last search staged for its per-search upload on the first device slot (the scoring
 * block -- the 8 KB matrix, or a profile's position scores -- the query codes, and the strip
 * kernels' table when those run); beside ssa_amd_stats_t, whose layout is kept. */
uint64_t ssa_amd_get_upload_bytes( void );

/* Replays an insertion log (concatenated shard logs, in shard order) and
 * writes the sorted top-k (score desc, id desc).  Returns the count. */
size_t ssa_amd_replay( const ssa_hit_t * log, size_t n, size_t hitcount, ssa_hit_t * out );

/* Multi-process search over RCCL (one process per GPU).  The
 * reference merges its worker threads' heaps in one process
 * (src/algo/manager.c:141-145); a sharded deployment merges the shards'
 * insertion logs instead:
 *   rank 0:        ssa_amd_dist_unique_id(id)   (id: ssa_amd_dist_unique_id_bytes()
 *                  bytes, handed to the other ranks out of band -- MPI, a TCP
 *                  store, a shared file)
 *   every rank:    ssa_amd_set_device(local GPU); ssa_amd_dist_init(rank, world, id)
 *   every search:  n = ssa_amd_search(q, algo, k, width, SSA_AMD_LOG, log, cap);
 *                  c = ssa_amd_gather_logs(log, n, k, out)   (collective)
 * ssa_amd_gather_logs gathers every rank's log over RCCL (one ncclGather of
 * fixed 512-row slots to rank 0; a log longer than its slot sends the rest of
 * its rows to rank 0 point to point, ncclSend / ncclRecv between those two
 * ranks only) and on rank 0 writes the global sorted top-k to out and returns
 * its length -- bit-identical to one process searching the whole DB; other
 * ranks return 0.  ssa_amd_dist_init returns 0 on success.
 * ssa_amd_merge_logs is rank 0's merge alone: nlogs logs at rows + r * stride
 * (counts[r] rows each), replayed in order through the reference heap. */
int ssa_amd_dist_unique_id( void * id );
size_t ssa_amd_dist_unique_id_bytes( void );
/* Local readiness, no communication: 0 when RCCL resolves and this rank's
 * device can be selected, i.e. everything ssa_amd_dist_init checks before it
 * enters the collective ncclCommInitRank.  Agree on it across ranks (e.g. a
 * MIN all-reduce) before calling ssa_amd_dist_init, so that no rank waits in
 * the init for a peer that gave up. */
int ssa_amd_dist_available( void );
int ssa_amd_dist_init( int rank, int world, const void * id );
/* Test support: the calling THREAD becomes rank `rank` of an in-process
 * group of `world` threads (keyed by `group`), whose collectives exchange
 * through host memory instead of RCCL -- the same slot layout, count rows and
 * point-to-point remainder as over RCCL.  Released by ssa_amd_dist_finalize on
 * that thread.  Returns 0 on success. */
int ssa_amd_dist_init_fake( int rank, int world, int group );
/* Ranks of the current communicator (ncclCommCount), 0 before init. */
int ssa_amd_dist_ranks( void );
void ssa_amd_dist_finalize( void );
size_t ssa_amd_gather_logs( const ssa_hit_t * log, size_t n, size_t hitcount, ssa_hit_t * out );
size_t ssa_amd_merge_logs( const ssa_hit_t * rows, const size_t * counts, size_t nlogs, size_t stride,
                           size_t hitcount, ssa_hit_t * out );
/* Residue-balanced contiguous shards: cuts records
 * [0, n) with the given lengths into `world` ID ranges
 * [bounds[r], bounds[r + 1]) (bounds has world + 1 entries, bounds[0] = 0,
 * bounds[world] = n) whose residue sums are as equal as cuts at multiples of
 * `align` allow (align = chunk_size keeps a multi-view search's chunk-
 * interleaved insertion order the concatenation of the shards' orders;
 * 0 or 1 = any record).  The multi-process analogue of ssa_amd_set_devices'
 * split.  Returns 0, or 1 for world < 1. */
int ssa_amd_shard_bounds( const uint64_t * lengths, size_t n, size_t world, size_t align, size_t * bounds );

/* Persistent packed DB: ssa_amd_save_db writes the device
 * layout of the open DB (packing it first if needed); ssa_amd_load_db,
 * called after init_db on the same DB file and with the same
 * init_symbol_translation settings, uploads that layout instead of
 * re-reading, mapping and packing every record.  The file records symbol
 * type, strands, DB genetic code and record count and is refused when they
 * differ.  Both return 0 on success. */
int ssa_amd_save_db( const char * path );
int ssa_amd_load_db( const char * path );

/* COMPUTE_ALIGNMENT traceback of one (query, DB sequence) pair of mapped
 * codes with the current matrix and gap penalties (reference align.c +
 * cigar.c, the same routine sw_align/nw_align use for their hits).  Writes
 * region = {query begin, query end, db begin, db end} and the NUL-terminated
 * CIGAR (truncated to cap - 1 characters); returns the CIGAR length. */
size_t ssa_amd_align_pair( int algo, const char * query, size_t qlen, const char * db, size_t dlen,
                           size_t region[4], char * cigar, size_t cap );

/* Exact optimal scores of npairs independent pairs with the current matrix and
 * gap penalties (init_score_matrix / init_constant_scores / init_gap_penalties).
 * Sequences are mapped residue codes (< 32), as ssa_amd_align_pair takes them:
 * pair i is q_codes[q_off[i] .. q_off[i+1]) against d_codes[d_off[i] .. d_off[i+1]).
 * scores[i] is what sw_align / nw_align report for that pair (query = q side,
 * DB sequence = d side: the search scores M[d][q]).  Returns 0, or non-zero
 * (nothing written, nothing launched) for a NULL argument with npairs > 0,
 * decreasing offsets, a code >= 32 or an unknown algo.
 * An empty side is defined: SW scores 0; NW scores 0 when both sides are empty
 * and gap_open + L * gap_extend against a side of length L.
 * The batch is ordered by shape, packed 64 pairs to a wave and scored in int32
 * by pairs_kernel on the current device (ssa_amd_set_device; one device, never
 * the SSA_AMD_DEVICES slots); pairs int32 cannot score exactly -- a matrix
 * entry outside int8, a positive gap penalty, a score bound near 2^29 -- and
 * every pair when no HIP device is visible go through the int64 recurrences
 * on the host, in parallel (set_thread_count).  An open DB, its device copy
 * and ssa_amd_get_stats are left alone.  Options:
 *   "pairs_chunk" N      pairs per pack / launch round (multiples of 64); 0 (default): as many as
 *                        fit 256 MiB of device memory
 *   "pairs_host" 0|1     1: every pair on the host path (default 0)
 * Tracebacks: ssa_amd_align_pairs for a batch, ssa_amd_align_pair for one pair. */
int ssa_amd_score_pairs( int algo, const uint8_t * q_codes, const uint64_t * q_off,
                         const uint8_t * d_codes, const uint64_t * d_off,
                         size_t npairs, int64_t * scores );
void ssa_amd_get_pairs_stats( ssa_amd_pairs_stats_t * out );
/* ssa_amd_score_pairs for a list of index pairs over two sequence SETS: the
 * caller keeps each sequence once, however many pairs it appears in.
 * q_off has nq + 1 entries and d_off nd + 1; sequence a of the q set is
 * q_codes[q_off[a] .. q_off[a+1]), likewise for d.  Pair p is q sequence
 * q_idx[p] against d sequence d_idx[p], and scores[p] is exactly what
 * ssa_amd_score_pairs writes for that pair in the expanded list (SW and NW,
 * M[d][q], the empty-side values, the host path for what int32 cannot score).
 * Duplicate pairs, unreferenced sequences and one set against itself
 * (q_codes == d_codes) are fine.
 * Returns 0, or non-zero (nothing written, nothing launched) for an unknown
 * algo, a NULL argument with npairs > 0, decreasing offsets anywhere in
 * either set, a code >= 32 anywhere in either pool q_codes[q_off[0] ..
 * q_off[nq]) / d_codes[d_off[0] .. d_off[nd]) -- the WHOLE pool is checked,
 * sequences no pair references included, because the whole pool is uploaded
 * -- or an index q_idx[p] >= nq / d_idx[p] >= nd.  npairs == 0 returns 0.
 * By default nothing is expanded or interleaved on the host: both pools go to
 * the device once per call (once in all when q_codes == d_codes, q_off ==
 * d_off and nq == nd), each pair costs a 24-byte descriptor, and
 * pairs_gather_kernel writes pairs_kernel's lane-interleaved input on the
 * device in front of it.  Device choice, stream, "pairs_chunk", "pairs_host"
 * and ssa_amd_get_pairs_stats are ssa_amd_score_pairs'; on the gather path
 * `launches` counts both kernels (2 per chunk), pack_ms is the ordering and
 * the descriptor fill, gather_ms and pool_bytes are set.  Options:
 *   "pairs_gather" 1|0   1 (default): as above; 0: the pairs are packed on the host, as
 *                        ssa_amd_score_pairs packs them (same scores; gather_ms = pool_bytes = 0)
 *   "pairs_pool_mb" N    (default 1024) uploaded pools above N MiB: pack on the host, as under
 *                        "pairs_gather" 0 */
int ssa_amd_score_pairs_indexed( int algo,
                                 const uint8_t * q_codes, const uint64_t * q_off, size_t nq,
                                 const uint8_t * d_codes, const uint64_t * d_off, size_t nd,
                                 const uint32_t * q_idx, const uint32_t * d_idx, size_t npairs,
                                 int64_t * scores );
/* Region and CIGAR of npairs independent pairs in one call: for every pair
 * (region, CIGAR) is exactly what ssa_amd_align_pair returns for it under the
 * current matrix and gap penalties -- a zero-score SW pair gives (0, 0, 0, 0)
 * and an empty CIGAR, an empty side whatever that routine yields -- and score
 * is what ssa_amd_score_pairs reports.  Arguments and their checks are
 * ssa_amd_score_pairs'; non-zero (nothing written, nothing launched) also for
 * a cigar_cap below the bound.
 * The CIGAR buffer: a CIGAR's text is never longer than its operation count,
 * which is at most qlen + dlen, so cigar_cap must be at least the sum over all
 * pairs of (qlen_i + dlen_i + 1).  Pair i's text starts at cigars +
 * out[i].cigar_off, is out[i].cigar_len characters long and NUL-terminated;
 * texts do not overlap.
 * A pair is aligned on the device under ssa_amd_score_pairs' conditions and
 * three more: for SW a symmetric matrix (the reference's region passes score
 * M[query][db], its direction pass M[db][query]); both lengths below 65 535
 * (cell positions travel as 16 + 16 bits); direction bits (2 per cell) of at
 * most 512 MiB for the pair alone.  Everything else, and every pair when no
 * HIP device is visible, goes through ssa_amd_align_pair's routine on the
 * host, in parallel (set_thread_count); flags bit 0 marks those.  On the
 * device a chunk of groups runs four kernels -- SW forward (the end cell), SW
 * reverse (the begin cell), directions, walk; NW the last two -- with the
 * direction bits kept in device memory: a chunk holds at most 1 GiB, of which
 * they are the largest part (ssa_amd_align_pairs_stats_t::dir_bytes).
 * Options "pairs_chunk" and "pairs_host" apply as for ssa_amd_score_pairs, and
 *   "pairs_wave" 0|1     1 (default 0): the pairs that qualify (the conditions above; the direction
 *                        bits counted in the wave kernels' layout) are aligned one WAVE per pair by
 *                        the kernels of ssa_amd_align_hits below instead of one pair per lane: the
 *                        same results; a call's device time is then its longest pair's alone, which
 *                        suits a few long pairs and wastes the chip on many short ones.  The
 *                        statistics read kernels "wave_fwd,wave_rev,wave_dir,wave_walk" (NW:
 *                        "wave_dir,wave_walk"), groups = device pairs, launches = chunks x 4
 *                        (NW: x 2); "pairs_chunk" does not apply (a chunk is 1 GiB of device memory) */
int ssa_amd_align_pairs( int algo, const uint8_t * q_codes, const uint64_t * q_off,
                         const uint8_t * d_codes, const uint64_t * d_off, size_t npairs,
                         ssa_amd_pair_alignment_t * out, char * cigars, size_t cigar_cap );
void ssa_amd_get_align_pairs_stats( ssa_amd_align_pairs_stats_t * out );
/* The alignment list sw_align / nw_align with COMPUTE_ALIGNMENT would return
 * for exactly these n hits of the open DB (hits as ssa_amd_search and
 * ssa_amd_search_batch write them: global DB ID, query view, DB strand and
 * frame; algo SSA_AMD_SW or SSA_AMD_NW), field by field -- the DB sequence
 * re-fetched as mapped codes, the query borrowed from `query`, the reference's
 * swap of db_seq.strand and db_seq.frame, score = hits[i].score, region and
 * CIGAR.  Free it with free_alignment.  Returns NULL, with nothing launched,
 * for a NULL query, an unknown algo, NULL hits with n > 0, a db_id outside the
 * open DB's ID range, a query_id that is not one of the query's views or a
 * strand / frame no entry has.
 * Both this call and sw_align / nw_align with COMPUTE_ALIGNMENT align their
 * hits on the device of the search's first slot, one wave per hit
 * (align_wave.hip: the hit's query rows spread over the lanes, its columns
 * swept through them; SW forward, SW reverse, directions, walk -- NW the last
 * two -- enqueued back to back, one upload, one copy back), under
 * ssa_amd_align_pairs' conditions per hit; every other hit, and every hit when
 * no gfx950 device is visible, goes through ssa_amd_align_pair's routine on the
 * host threads (set_thread_count).  The results are identical either way.
 * ssa_amd_get_align_hits_stats reports the last such alignment stage in
 * ssa_amd_align_pairs' struct: pairs = hits, total_ms = the whole stage, groups
 * = hits aligned on the device, device = -1 when nothing was launched;
 * ssa_amd_get_stats is untouched.  Options:
 *   "align_wave" 1|0     1 (default): as above; 0: every hit on the host threads, one hit per thread
 *   "align_wave_min" N   hit lists shorter than N stay on the host (default 1)
 *   "align_wave_rl" N    query rows per lane of the wave kernels: 0 (default) chosen per call for the
 *                        fewest row steps, or one of 1 .. 10, 12, 16 (a testing aid; also under "pairs_wave") */
p_alignment_list ssa_amd_align_hits( p_query query, int algo, const ssa_hit_t * hits, size_t n );
void ssa_amd_get_align_hits_stats( ssa_amd_align_pairs_stats_t * out );
/* ASCII -> DB-side residue codes of the current symbol type (us_map_sequence:
 * unknown -> 0); writes min(len, cap) codes, returns len. */
size_t ssa_amd_map_residues( const char * ascii, size_t len, char * out, size_t cap );

/* The query buffers a search scores for the current symbol type and strands
 * (reference searcher.c:42-90): one q_seq_t per strand/frame view, codes as
 * handed out in alignment_t.query.seq.  Writes up to cap views; returns the
 * number of views. */
size_t ssa_amd_query_views( p_query query, q_seq_t * out, size_t cap );

/* Translates mapped nucleotide codes (map_ncbi_nt16 values) with the query
 * (db_side = 0) or DB (db_side = 1) genetic code chosen by
 * init_symbol_translation, strand 0 (forward) or 1 (reverse complement),
 * frame 0..2 -- reference util_sequence.c:332-382.  Writes min(result, cap)
 * amino-acid codes; returns the protein length (len - frame) / 3, 0 when
 * len < frame. */
size_t ssa_amd_translate( int db_side, const char * nt_codes, size_t len, int strand, int frame,
                          char * out, size_t cap );

/* Ends-free (semi-global) alignment of a batch of pairs: NW's recurrence
 * (rows = q side, columns = d side, scores M[d][q], a gap of length L costs
 * gap_open + L * gap_extend) in which each of the four sequence ends may be
 * free.  `ends` is a mask of: */
#define SSA_AMD_FREE_Q_BEGIN 1   /* the alignment may start anywhere in q: H(i, -1) = 0 */
#define SSA_AMD_FREE_Q_END   2   /* ... and end anywhere in q: candidates (i, dlen - 1) for every i */
#define SSA_AMD_FREE_D_BEGIN 4   /* the alignment may start anywhere in d: H(-1, j) = 0 */
#define SSA_AMD_FREE_D_END   8   /* ... and end anywhere in d: candidates (qlen - 1, j) for every j */
/* Mask 0 is NW's score; 15 is the overlap alignment; FREE_Q_BEGIN | FREE_Q_END
 * places d (a read) globally inside q (a window), FREE_D_BEGIN | FREE_D_END the
 * other way round.  The end cell is the candidate with the greatest H -- the
 * corner (qlen - 1, dlen - 1) is always one -- and among equal candidates the
 * one with the greatest (d_end, q_end) in lexicographic order; the score is
 * its H.  An empty side: 0 when both sides are empty or the other side has a
 * free begin or end, else gap_open + L * gap_extend over the other side's
 * length L.
 * ssa_amd_score_pairs_ends: arguments, their checks, return codes, options
 * ("pairs_chunk", "pairs_host"), device choice and host path are
 * ssa_amd_score_pairs'; an `ends` outside 0..15 also returns non-zero (nothing
 * written, nothing launched).  The call reports through
 * ssa_amd_get_pairs_stats with kernel "pairs_ends_i32". */
int ssa_amd_score_pairs_ends( int ends, const uint8_t * q_codes, const uint64_t * q_off,
                              const uint8_t * d_codes, const uint64_t * d_off,
                              size_t npairs, int64_t * scores );
/* Region and CIGAR of the same alignments; arguments, checks, the CIGAR
 * buffer and its bound are ssa_amd_align_pairs'.  score is what
 * ssa_amd_score_pairs_ends reports; region = {q begin, q end, d begin, d end},
 * inclusive, ends at the end cell above.  Direction bits are derived as
 * ssa_amd_align_pair derives them for NW, under the ends-free boundaries; the
 * walk goes from the end cell until it leaves the matrix, left first ('I', a
 * target residue), then up ('D', a query residue), else diagonal ('M'), and --
 * unlike ssa_amd_align_pair's -- reads a cell's gap-extension bits only when
 * it entered the cell through that gap, so that the text re-scores exactly.
 * Unlike NW's, the CIGAR also accounts for the whole region: where
 * the walk leaves through column -1 at row i, a free q begin starts the
 * region at q begin = i + 1, else q begin = 0 and a run of i + 1 D leads the
 * text; the same through row -1 with the d begin and I.  So M adds M[d][q],
 * a run of L adds gap_open + L * gap_extend, and the text re-scored from
 * (q begin, d begin) gives the score and ends at (q end + 1, d end + 1).  An
 * empty side gives region zeros and an empty CIGAR.
 * A pair is aligned on the device under ssa_amd_align_pairs' NW conditions
 * (an int8 matrix, penalties <= 0, the score bound, both lengths below
 * 65 535, direction bits -- four per cell here -- of at most 512 MiB for the
 * pair; no symmetry needed): one sweep writes direction bits, score and end
 * cell, the walk follows on the device; a chunk holds at most 2 GiB.
 * Everything else goes through the int64 host routine; flags bit 0 marks
 * those.  The call reports through
 * ssa_amd_get_align_pairs_stats: kernels "pairs_ends_dir,pairs_ends_walk"
 * (empty when nothing was launched), fwd_ms = rev_ms = 0, zero_pairs = 0. */
int ssa_amd_align_pairs_ends( int ends, const uint8_t * q_codes, const uint64_t * q_off,
                              const uint8_t * d_codes, const uint64_t * d_off, size_t npairs,
                              ssa_amd_pair_alignment_t * out, char * cigars, size_t cigar_cap );

/* Banded ends-free alignment of a batch of pairs: the recurrence above,
 * restricted pair by pair to a band of diagonals.  With i the q (row) index
 * and j the d (column) index, pair p's band is the set of diagonals k = j - i
 * with band_lo[p] <= k <= band_hi[p].  A cell (i, j), -1 <= i < qlen and
 * -1 <= j < dlen, EXISTS iff its diagonal is in the band; a boundary cell
 * (row -1 or column -1) whose begin is not free must also have diagonal 0 in
 * the band, because its value gap_open + L * gap_extend is a gap that starts
 * at (-1, -1).  H, E and F of a cell that does not exist are minus infinity.
 * Everything else -- boundaries, candidates, the rule among equal candidates --
 * is the ends-free definition over existing cells.  A band with lo <= -qlen
 * and hi >= dlen gives exactly ssa_amd_score_pairs_ends' score and
 * ssa_amd_align_pairs_ends' region and CIGAR text, for every mask.
 * A band is VALID iff lo <= hi, [lo, hi] meets the diagonals an alignment may
 * start on, [FREE_Q_BEGIN ? -qlen : 0, FREE_D_BEGIN ? dlen : 0], and meets those
 * it may end on, [FREE_D_END ? -(qlen - 1) : dlen - qlen,
 * FREE_Q_END ? dlen - 1 : dlen - qlen]: exactly then the best banded score is
 * finite.  A pair of two non-empty sides with an invalid band makes the call
 * return non-zero (nothing written, nothing launched), so no result ever
 * means "no alignment".  A pair with an empty side ignores its band and gets
 * the ends-free closed form.  Band values beyond [-qlen, dlen] are legal and
 * equivalent to the clamped ones (lo = min(0, dlen - qlen) - w, hi = max(0,
 * dlen - qlen) + w is the band of half-width w around both corners'
 * diagonals, valid for every mask).
 * ssa_amd_score_pairs_banded: `ends` is the mask, 0..15; the other arguments,
 * their checks, return codes, options ("pairs_chunk", "pairs_host") and
 * device choice are ssa_amd_score_pairs_ends'; band_lo / band_hi NULL with
 * npairs > 0 also returns non-zero.  The call reports through
 * ssa_amd_get_pairs_stats with kernel "pairs_banded_i32"; swept_cells counts
 * the cells of the column blocks the waves swept, which follow the bands. */
int ssa_amd_score_pairs_banded( int ends, const int64_t * band_lo, const int64_t * band_hi,
                                const uint8_t * q_codes, const uint64_t * q_off,
                                const uint8_t * d_codes, const uint64_t * d_off,
                                size_t npairs, int64_t * scores );
/* Region and CIGAR of the same alignments, by ssa_amd_align_pairs_ends' walk
 * and contract: the text re-scored from (q begin, d begin) gives the score and
 * ends at (q end + 1, d end + 1); in addition every cell it visits lies in the
 * band.  The CIGAR buffer and its bound are ssa_amd_align_pairs'.
 * A pair is aligned on the device under ssa_amd_align_pairs_ends' conditions,
 * with the direction bits counted for the band alone: both lengths below
 * 65 535 and banded bits of at most 512 MiB for the pair, so long pairs with
 * narrow bands are device pairs.  Direction bits are kept only for the swept
 * column blocks (ssa_amd_align_pairs_stats_t::dir_bytes); a walk that ever
 * stood outside them would hand its pair to the host routine
 * (device_fallbacks, expected 0).  Everything else goes through the int64 host
 * routine, which keeps its matrices for the band only; flags bit 0 marks
 * those.  The call reports through ssa_amd_get_align_pairs_stats: kernels
 * "pairs_banded_dir,pairs_banded_walk" (empty when nothing was launched),
 * fwd_ms = rev_ms = 0, zero_pairs = 0. */
int ssa_amd_align_pairs_banded( int ends, const int64_t * band_lo, const int64_t * band_hi,
                                const uint8_t * q_codes, const uint64_t * q_off,
                                const uint8_t * d_codes, const uint64_t * d_off, size_t npairs,
                                ssa_amd_pair_alignment_t * out, char * cigars, size_t cigar_cap );

/* Local begin / end modes of the banded calls: Smith-Waterman inside a band,
 * and extension alignment.  `mode` is a mask of the four SSA_AMD_FREE_* bits
 * and of: */
#define SSA_AMD_LOCAL_BEGIN 16  /* the alignment may begin at any cell */
#define SSA_AMD_LOCAL_END   32  /* ... and end at any cell */
/* Modes 0..63 are legal.  The CANONICAL mode adds FREE_Q_BEGIN | FREE_D_BEGIN
 * when LOCAL_BEGIN is set and FREE_Q_END | FREE_D_END when LOCAL_END is set;
 * every mode behaves exactly as its canonical one.  The 25 canonical modes:
 * 0..15; 21, 23, 29, 31 (local begin; end = corner / q free / d free / both
 * free); 42, 43, 46, 47 (local end; begin = fixed / q free / d free / both
 * free); 63.  Mode 63 is Smith-Waterman, 42 extends to the right from a fixed
 * begin, 21 to the left towards a fixed end.
 * Everything not said here is the banded definition above: rows = q, columns =
 * d, scores M[d][q], gaps gap_open + L * gap_extend, a cell exists iff its
 * diagonal k = j - i is in [lo, hi], minus infinity outside the band, a
 * boundary cell whose begin is not free needs diagonal 0 in the band.
 * LOCAL_BEGIN: every existing boundary cell is 0; every existing real cell has
 * H(i, j) = max(0, D, E, F) with D = H(i-1, j-1) + M[d_j][q_i], and STOP(i, j)
 * holds iff max(D, E, F) <= 0 (the floor wins ties: the shortest alignment);
 * E and F are computed from the floored H; a cell outside the band is minus
 * infinity, not 0.
 * LOCAL_END: the end candidates are all existing real cells with a finite H;
 * the score is max(0, greatest candidate H); if that is 0 the result is the
 * empty alignment, else the end cell is the candidate with the greatest H and
 * among equal ones the SMALLEST (d_end, q_end) in lexicographic order (the
 * cell the reference's forward SW pass picks).  Without LOCAL_END candidates
 * and the greatest-(d_end, q_end) rule are the ends-free calls'.
 * The walk is ssa_amd_align_pairs_ends' with one addition: at a cell it stands
 * on through its H -- the end cell, a cell reached by M, or one reached by a
 * gap whose extension bit is not set -- it first tests STOP and, if set, stops
 * there; that cell is not part of the alignment (q begin = i + 1, d begin =
 * j + 1).  Leaving through row -1 or column -1 works as before under the
 * canonical mode.  The score is the end cell's H; the region is inclusive; the
 * CIGAR re-scored from (q begin, d begin) gives exactly the score and ends at
 * (q end + 1, d end + 1); every visited cell lies in the band.  With a local
 * bit set, score 0 <=> empty CIGAR <=> region (0, 0, 0, 0), counted in
 * zero_pairs.
 * A band is VALID iff lo <= hi and [lo, hi] meets the start diagonals
 * [FREE_Q_BEGIN ? -qlen : 0, FREE_D_BEGIN ? dlen : 0] and the end diagonals of
 * the canonical mode (under LOCAL_END every real cell's diagonal,
 * [-(qlen - 1), dlen - 1]); a band that holds no real cell of the pair is
 * refused, under mode 63 too.  An invalid band of a pair with two non-empty
 * sides makes the call return non-zero before anything runs.  An empty side
 * ignores its band: score 0 with either local bit, region zeros, empty CIGAR.
 * Band values are clamped as above.  band_lo == band_hi == NULL means
 * unbanded (lo = -qlen - 1, hi = dlen + 1 for every pair); exactly one of them
 * NULL is refused, as is a mode outside 0..63.
 * Arguments, checks, return codes, the CIGAR buffer bound, options
 * ("pairs_chunk", "pairs_host"), device choice and statistics getters are the
 * banded calls'.  A canonical mode below 16 is handed to
 * ssa_amd_*_pairs_banded (with bands) or ssa_amd_*_pairs_ends (NULL bands)
 * unchanged: results and statistics are those calls'.  With a local bit the
 * score call reports kernel "pairs_local_i32"; the align call reports kernels
 * "pairs_local_end,pairs_local_dir,pairs_local_walk" under LOCAL_END (fwd_ms =
 * the end-cell pass) and "pairs_local_dir,pairs_local_walk" under LOCAL_BEGIN
 * alone (fwd_ms = 0); rev_ms = 0, kernel_ms is the sum, dir_bytes counts the
 * direction bits and the STOP bits.  Device conditions are the banded calls'
 * (no symmetric matrix needed; the 512 MiB of a pair include its STOP bits). */
int ssa_amd_score_pairs_local( int mode, const int64_t * band_lo, const int64_t * band_hi,
                               const uint8_t * q_codes, const uint64_t * q_off,
                               const uint8_t * d_codes, const uint64_t * d_off,
                               size_t npairs, int64_t * scores );
int ssa_amd_align_pairs_local( int mode, const int64_t * band_lo, const int64_t * band_hi,
                               const uint8_t * q_codes, const uint64_t * q_off,
                               const uint8_t * d_codes, const uint64_t * d_off, size_t npairs,
                               ssa_amd_pair_alignment_t * out, char * cigars, size_t cigar_cap );

/* What a batch caller thresholds on -- identity, aligned columns and the region
 * for coverage -- without the traceback: one pair's result of
 * ssa_amd_summarize_pairs_local. */
typedef struct {
    int64_t  score;       /* ssa_amd_score_pairs_local's */
    uint64_t region[4];   /* q begin, q end, d begin, d end -- ssa_amd_align_pairs_local's */
    uint32_t columns;     /* operations of that call's CIGAR: M + I + D */
    uint32_t matched;     /* its M columns */
    uint32_t identical;   /* M columns whose q code equals the d code (mapped codes compared) */
    uint32_t flags;       /* bit 0: summarized on the host path */
} ssa_amd_pair_summary_t;   /* 56 bytes */

/* Pair i's score and region are exactly what ssa_amd_align_pairs_local returns
 * with the same mode, bands, sequences, matrix and penalties; columns and
 * matched count that call's CIGAR, and identical counts the M columns in which
 * the two residue codes are equal when the text is walked from (q begin, d
 * begin).  All 64 modes are accepted, through their 25 canonical ones; NULL
 * bands mean unbanded; modes below 16 are the ends-free and banded
 * definitions.  Where that call has no CIGAR -- an empty side, a zero score
 * under a local bit -- every counter and the region are 0.  A leading D or I
 * run of a begin that is not free counts in columns, as it does in the text;
 * columns = (q end - q begin + 1) + (d end - d begin + 1) - matched always.
 * Arguments, checks, band validity, return codes and "nothing written, nothing
 * launched" are ssa_amd_score_pairs_local's, and out == NULL with npairs > 0
 * returns non-zero; there is no CIGAR buffer.  Options "pairs_chunk" and
 * "pairs_host" apply.
 * Nothing of the traceback is kept: a chunk (256 MiB of residues and row
 * buffers) runs the score pass, which leaves the end cell, and one sweep that
 * carries, beside every H, E and F, the counters and the begin of the path the
 * walk would take from it, selected by the comparisons that define the
 * direction bits; the words at the end cell are the result, ties included.  No
 * direction bits, walk, runs or text exist on the device path.
 * Device conditions: ssa_amd_score_pairs_local's (a device visible, the matrix
 * in int8, gap penalties <= 0, (qlen + dlen) inside the 2^29 score bound, two
 * non-empty sides) and both lengths below 65 535, because positions travel as
 * 16 + 16 bits.  No direction-bit budget applies: a 60 000 x 60 000 unbanded
 * pair is a device pair.  Every other pair takes the host path -- the host
 * align routine of the canonical mode, its text counted in place, quadratic
 * memory in the band -- and has bit 0 of flags set.
 * Statistics through ssa_amd_get_align_pairs_stats: pairs, cells, host_pairs,
 * zero_pairs, groups, chunks; launches = 2 * chunks; kernels =
 * "pairs_summary_end,pairs_summary_sweep" (empty when nothing was launched);
 * fwd_ms = the end-cell pass, dir_ms = the summary sweep, rev_ms = walk_ms =
 * text_ms = 0, kernel_ms their sum; dir_bytes = 0; device_fallbacks = 0. */
int ssa_amd_summarize_pairs_local( int mode, const int64_t * band_lo, const int64_t * band_hi,
                                   const uint8_t * q_codes, const uint64_t * q_off,
                                   const uint8_t * d_codes, const uint64_t * d_off,
                                   size_t npairs, ssa_amd_pair_summary_t * out );

/* X-drop extension: the local calls of a mode with LOCAL_END and without
 * LOCAL_BEGIN, whose alignment stops once a whole row has fallen more than
 * `xdrop` below the best score seen (the rule of BLAST's gapped extension and
 * of ksw2's Z-drop, without the latter's diagonal term).  xdrop is >= 0; `mode`
 * must canonicalise to 42, 43, 46 or 47.  Everything not said here is
 * ssa_amd_*_pairs_local's and stays as it is: bands, boundary cells, the
 * recurrence, "a cell exists", minus infinity, the walk, the CIGAR contract,
 * empty sides, band validity and NULL bands.  No cell is pruned -- every H, E,
 * F and direction bit is the local call's -- only the set of end candidates is
 * cut, row by row.  For row i (0 <= i < qlen) let C_i be the existing real
 * cells (i, j) with a finite H, m_i the greatest H in C_i and c_i the smallest
 * column that attains m_i.  Walk the rows in ascending order, starting with
 * best = 0 and no end cell:
 *   - C_i empty (no cell of the row in the band or in the matrix, or none
 *     reachable): the row is passed over;
 *   - else best - m_i > xdrop: stop.  Row i is the DROP ROW; rows >= i hold no
 *     candidate;
 *   - else m_i > best: the end cell becomes (i, c_i) and best = m_i; the same
 *     if m_i == best, an end cell exists and c_i is smaller than its column.
 * The score is best; 0 means the empty alignment (region zeros, empty CIGAR,
 * counted in zero_pairs).  Equivalently the result is the local call's with
 * its candidates restricted to the rows before the drop row; ties keep the
 * local rule, the smallest (d_end, q_end).  An xdrop at or above 2^30 never
 * stops a device pair (the host clamps it; device scores lie inside 2^29), so
 * the result is then exactly the local call's.  Not part of this: ksw2's
 * diagonal term, per-pair drops, LOCAL_BEGIN modes (a left extension is the
 * right extension of the reversed sequences), pruning of columns.
 * Arguments, checks, return codes, "nothing written, nothing launched",
 * options ("pairs_chunk", "pairs_host"), device conditions, host routing and
 * the statistics getters are the corresponding local calls'; a negative xdrop
 * and a mode whose canonical form is not 42, 43, 46 or 47 also return
 * non-zero.  The host path is the local calls' int64 routine with the row rule
 * (its loop stops at the drop row; flags bit 0).  On the device a chunk first
 * runs the end pass, the local score pass with the candidates tracked per row;
 * a wave leaves its strip loop once every lane has met its drop row or run out
 * of rows.
 * ssa_amd_score_pairs_xdrop reports kernel "pairs_xdrop_i32"; swept_cells
 * counts only the column blocks of the strips the waves entered.
 * ssa_amd_align_pairs_xdrop reports kernels
 * "pairs_xdrop_end,pairs_local_dir,pairs_local_walk", fwd_ms = the end pass:
 * after it every group is cut to the strip of its furthest end row (a group
 * without an end cell to nothing), and the local direction pass and walk run
 * on what is left; dir_bytes counts the direction bits that were swept.  The
 * 512 MiB condition of a pair is the local align call's, planned for the whole
 * band.  ssa_amd_summarize_pairs_xdrop reports kernels
 * "pairs_xdrop_end,pairs_summary_sweep", with the same cut.
 * ssa_amd_get_xdrop_dropped: the pairs of the last xdrop call that met a drop
 * row, device and host pairs alike. */
int ssa_amd_score_pairs_xdrop( int mode, int64_t xdrop, const int64_t * band_lo, const int64_t * band_hi,
                               const uint8_t * q_codes, const uint64_t * q_off,
                               const uint8_t * d_codes, const uint64_t * d_off,
                               size_t npairs, int64_t * scores );
int ssa_amd_align_pairs_xdrop( int mode, int64_t xdrop, const int64_t * band_lo, const int64_t * band_hi,
                               const uint8_t * q_codes, const uint64_t * q_off,
                               const uint8_t * d_codes, const uint64_t * d_off, size_t npairs,
                               ssa_amd_pair_alignment_t * out, char * cigars, size_t cigar_cap );
int ssa_amd_summarize_pairs_xdrop( int mode, int64_t xdrop, const int64_t * band_lo, const int64_t * band_hi,
                                   const uint8_t * q_codes, const uint64_t * q_off,
                                   const uint8_t * d_codes, const uint64_t * d_off,
                                   size_t npairs, ssa_amd_pair_summary_t * out );
uint64_t ssa_amd_get_xdrop_dropped( void );

/* ssa_amd_summarize_pairs_local for search hits: out[i] is,
 * field for field, what ssa_amd_summarize_pairs_local( mode, NULL, NULL, ... )
 * returns under the current matrix and penalties for the pair
 *   q side: the query view hits[i].query_id of `query` (ssa_amd_query_views' codes),
 *   d side: the DB entry (db_id - ID offset, db_strand, db_frame) AS THE SEARCH
 *           SCORED IT: the codes the packed DB holds for that entry.
 * For NUCLEOTIDE with the complementary strand the d side of a strand-1 hit is
 * the record's reverse complement.  This differs from ssa_amd_align_hits, which
 * keeps the reference aligner's behaviour and aligns the record's FORWARD copy
 * for such a hit (aligner.c:76 never flips it), so that call's text does not
 * belong to the score the search reported; this call's summary does.
 * hits are as ssa_amd_search, ssa_amd_search_batch and ssa_amd_search_above
 * write them; hits[i].score is not read: out[i].score is the DP's own score, so
 * under mode 63 it equals what sw_align reported for the hit and under mode 0
 * what nw_align reported.  All 64 modes are accepted, through their canonical
 * ones; the call is unbanded.  flags bit 0: summarized on the int64 host path.
 * Returns non-zero, with nothing written and nothing launched, for a NULL
 * query, a mode outside 0..63, NULL hits or out with n > 0, a db_id outside the
 * open DB's ID range, a query_id that is not one of the query's views,
 * db_strand > 1 or db_frame > 2, or a (record, strand, frame) no entry exists
 * for (an empty record has no entry).  n == 0 returns 0; duplicates are fine.
 * Routing.  A hit is GATHERED when option "hits_gather" is 1, a gfx950 device
 * is visible, the search runs on one device slot (the pair calls' device), the
 * packed DB is current there (it is packed when it is not) and the pair meets
 * ssa_amd_summarize_pairs_local's device conditions.  Only a 16-byte
 * descriptor per hit, the tables of a chunk and the query views are uploaded:
 * hits_gather_kernel writes the summary kernels' lane-interleaved input from
 * the device copy of the DB, translating its compact codes back to residue
 * codes, directly in front of the unchanged summary kernels on the same stream.
 * Every other hit is FETCHED: its entry codes are produced on the host as the
 * packer produces them and the pair goes through ssa_amd_summarize_pairs_local
 * itself (its device path, or its int64 host path under "pairs_host" 1 or
 * without a device).  With several device slots (ssa_amd_set_devices,
 * SSA_AMD_DEVICES) every hit is fetched: each slot holds a shard only.
 * The results are identical either way.
 * Statistics: ssa_amd_get_align_pairs_stats reports the call as the summary
 * call does; when hits were gathered, kernels =
 * "hits_gather,pairs_summary_end,pairs_summary_sweep" and launches = 3 x chunks
 * of the gather path (+ 2 x chunks of the fetched rest).  ssa_amd_get_stats
 * (the last search) is left alone.  Options:
 *   "hits_gather" 1|0    1 (default): as above; 0: every hit is fetched
 *   "pairs_chunk", "pairs_host" as for ssa_amd_summarize_pairs_local */
typedef struct {
    uint64_t hits;          /* hits of the last ssa_amd_summarize_hits call */
    uint64_t gathered;      /* ... whose sequences the device packer took from the device copy of the DB */
    uint64_t fetched;       /* ... fetched through the DB plugin on the host (hits = gathered + fetched) */
    uint64_t upload_bytes;  /* bytes of descriptors, tables and query views uploaded on the gather path */
    double   gather_ms;     /* HIP-event time of the hits_gather_kernel launches */
} ssa_amd_hits_stats_t;
int ssa_amd_summarize_hits( p_query query, int mode, const ssa_hit_t * hits, size_t n,
                            ssa_amd_pair_summary_t * out );
void ssa_amd_get_summarize_hits_stats( ssa_amd_hits_stats_t * out );

#ifdef __cplusplus
}
#endif

#endif /* LIBSSA_AMD_H_ */
