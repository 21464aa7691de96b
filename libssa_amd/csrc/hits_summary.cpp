// hits_summary.cpp -- ssa_amd_summarize_hits: ssa_amd_summarize_pairs_local for
// search hits.  A hit names a query view and a DB entry; the
// entry's residues already lie on the device, in the packed DB the search
// kernels read.  The GATHER path uploads a 16-byte descriptor per hit, the
// chunk's tables and the query views; hits_gather_kernel (hits_gather.hip)
// writes the summary kernels' lane-interleaved input from them, and the
// summary call's two launches follow on the same stream.  Ordering, grouping,
// strips, the byte budget and the chunk loop are that call's
// (pairs_banded_host.h: BandDescBatch::order, banded_pack_chunk_tables).
// Whatever the gather path does not take is FETCHED: the entry's codes are
// staged on the host as the packer stages them (engine.cpp
// staged_entry_codes) and the pair goes through summarize_pairs_local itself.
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "pairs_banded_host.h"
#include "pairs_gather.h"   // kGatherPoolPad
#include "pairs_local.h"

namespace ssa {

namespace {

ssa_amd_hits_stats_t g_hits_stats{};

static_assert(sizeof(GroupDesc) == sizeof(uint2) && offsetof(GroupDesc, blk) == 0,
              "hits_gather_kernel reads a DB group as (blk, ncols)");

// the per-call table and view pool, and what the gather kernel fills (lens, qres, tres); kept between calls
struct HitsDevice {
    int device = -1;
    PairsBuf call, res;
} g_dev;

// The entry (record, strand, frame) of D's pack, or SIZE_MAX: EntryMeta::id ascends, a record's entries adjoin.
size_t find_entry(const EntryMeta& M, uint64_t local, uint8_t strand, uint8_t frame) {
    size_t e = (size_t)(std::lower_bound(M.id.begin(), M.id.end(), local) - M.id.begin());
    for (; e < M.size() && M.id[e] == local; e++)
        if (M.strand[e] == strand && M.frame[e] == frame) return e;
    return SIZE_MAX;
}

}  // namespace

const ssa_amd_hits_stats_t& summarize_hits_stats() { return g_hits_stats; }

int summarize_hits(p_query query, int mode, const ssa_hit_t* hits, size_t n, ssa_amd_pair_summary_t* out) {
    const double t0 = now_ms();
    if (!query || mode < 0 || mode > 63 || (n && (!hits || !out))) return 1;
    const Config& C = cfg();
    const std::vector<QueryView> views = query_views(query);
    const uint64_t first = C.id_offset, count = ssa_db_get_sequence_count();
    for (size_t i = 0; i < n; i++) {
        const ssa_hit_t& h = hits[i];
        if (h.db_id < first || h.db_id - first >= count || h.query_id >= views.size() || h.db_strand > 1 ||
            h.db_frame > 2)
            return 1;
    }
    ssa_amd_hits_stats_t HS{};
    if (n == 0) {
        ssa_amd_align_pairs_stats_t S{};
        S.device = -1;
        set_align_pairs_stats(S);
        g_hits_stats = HS;
        return 0;
    }
    if (!matrix().ready) fatal("Scoring matrix not initialized");
    const int cmode = local_canonical(mode);
    const bool local = cmode >= 16;
    EndsRouting T;
    ends_route(T, n);

    // ---- route: the gather path needs the whole packed DB on the pair calls' device
    DeviceDB* D = nullptr;
    if (C.hits_gather && T.device && views.size() <= kHitsMaxViews) {
        const std::vector<SlotPlan> plan = device_plan();
        if (plan.size() == 1 && plan[0].device == T.dev_id) {
            ensure_device_db();
            D = &device_db(0);
            if (D->device != T.dev_id || D->meta.size() == 0) D = nullptr;
        }
    }
    std::vector<HitDesc> desc;           // the gathered hits
    std::vector<uint32_t> gat, fet;      // ... and the fetched ones, by input index
    std::vector<std::vector<uint8_t>> fcodes;
    uint64_t gcells = 0;
    if (D) {
        const EntryMeta& M = D->meta;
        const std::vector<uint32_t>& lane_of = entry_lanes(*D);
        for (size_t i = 0; i < n; i++) {
            const ssa_hit_t& h = hits[i];
            const size_t e = find_entry(M, h.db_id - first, h.db_strand, h.db_frame);
            if (e == SIZE_MAX) return 1;
            const uint64_t ql = views[h.query_id].len, dl = M.len[e];
            // the summary call's device conditions; positions travel as 16 + 16 bits
            if (ql && dl && (int64_t)(ql + dl) <= T.residue_limit && ql < kAlignMaxLen && dl < kAlignMaxLen &&
                lane_of[e] != 0xffffffffu) {
                desc.push_back(HitDesc{lane_of[e], (uint32_t)dl, h.query_id, (uint32_t)ql});
                gat.push_back((uint32_t)i);
                gcells += ql * dl;
            } else {
                fet.push_back((uint32_t)i);
            }
        }
    } else {
        fet.resize(n);
        for (size_t i = 0; i < n; i++) fet[i] = (uint32_t)i;
    }

    // ---- the fetch path, first: it may still refuse a hit, and then nothing has been launched or written
    ssa_amd_align_pairs_stats_t S{};
    S.device = -1;
    std::vector<ssa_amd_pair_summary_t> fout(fet.size());
    if (!fet.empty()) {
        fcodes.resize(fet.size());
        std::atomic<uint32_t> missing{0};
        parallel_ranges(fet.size(), 256, [&](size_t b, size_t e) {
            for (size_t k = b; k < e; k++) {
                const ssa_hit_t& h = hits[fet[k]];
                if (!staged_entry_codes(h.db_id - first, h.db_strand, h.db_frame, fcodes[k])) missing++;
            }
        });
        if (missing.load()) return 1;
        std::vector<uint64_t> qoff(fet.size() + 1, 0), doff(fet.size() + 1, 0);
        for (size_t k = 0; k < fet.size(); k++) {
            qoff[k + 1] = qoff[k] + views[hits[fet[k]].query_id].len;
            doff[k + 1] = doff[k] + fcodes[k].size();
        }
        std::vector<uint8_t> qc(qoff.back() + 1), dc(doff.back() + 1);
        parallel_ranges(fet.size(), 1024, [&](size_t b, size_t e) {
            for (size_t k = b; k < e; k++) {
                const QueryView& v = views[hits[fet[k]].query_id];
                if (v.len) memcpy(qc.data() + qoff[k], v.seq, v.len);
                if (!fcodes[k].empty()) memcpy(dc.data() + doff[k], fcodes[k].data(), fcodes[k].size());
            }
        });
        fcodes = {};
        if (summarize_pairs_local(mode, nullptr, nullptr, qc.data(), qoff.data(), dc.data(), doff.data(), fet.size(),
                                  fout.data()) != 0)
            return 1;
        S = align_pairs_stats();
    }
    for (size_t k = 0; k < fet.size(); k++) out[fet[k]] = fout[k];
    HS.hits = n;
    HS.fetched = fet.size();
    HS.gathered = gat.size();

    // ---- the gather path
    if (!gat.empty()) {
        const size_t ng = gat.size();
        std::vector<int64_t> lo(ng), hi(ng);
        for (size_t k = 0; k < ng; k++) {
            lo[k] = -(int64_t)desc[k].qlen - 1;      // NULL bands: the full range of every pair
            hi[k] = (int64_t)desc[k].dlen + 1;
        }
        BandedDevice& P = banded_device();
        banded_prepare_device(T.dev_id);
        HitsDevice& H = g_dev;
        if (H.device != T.dev_id) {
            H.call.release();
            H.res.release();
            H.device = T.dev_id;
        }
        S.pairs += ng;
        S.cells += gcells;
        S.device = T.dev_id;
        snprintf(S.kernels, sizeof S.kernels, "hits_gather,pairs_summary_end,pairs_summary_sweep");
        const double tp0 = now_ms();
        // ---- once per call: the code table and the views, with readable bytes behind them
        const size_t o_pool = pairs_align_up(sizeof(HitsTable));
        size_t pool = 0;
        for (const QueryView& v : views) pool += v.len;
        const size_t call_bytes = o_pool + pool + kGatherPoolPad;
        H.call.need(call_bytes, true, "hits_summary views");
        memset(H.call.h, 0, call_bytes);
        HitsTable* tab = (HitsTable*)H.call.h;
        for (uint32_t c = 0; c < kHitsCodes; c++) tab->code_of[c] = c < D->alpha ? D->code_of[c] : (uint8_t)kPairsPad;
        pool = 0;
        for (size_t v = 0; v < views.size(); v++) {
            tab->view_start[v] = (uint32_t)pool;
            if (views[v].len) memcpy(H.call.h + o_pool + pool, views[v].seq, views[v].len);
            pool += views[v].len;
        }
        check(hipMemcpyAsync(H.call.d, H.call.h, call_bytes, hipMemcpyHostToDevice, T.stream), "hits_summary upload");
        HS.upload_bytes += call_bytes;

        BandDescBatch B{desc.data(), lo.data(), hi.data(), {}, {}, {}, {}, {}};
        B.idx.resize(ng);
        for (size_t k = 0; k < ng; k++) B.idx[k] = (uint32_t)k;
        B.order(false);
        S.groups += (uint32_t)B.groups.size();
        S.pack_ms += now_ms() - tp0;
        uint64_t zeros = 0;
        for (size_t g0 = 0; g0 < B.groups.size();) {
            const double tc0 = now_ms();
            BandChunk K = banded_pack_chunk_tables(B, g0, cmode & 15, T);
            // what the gather kernel writes whole: lens, qres, tres of the chunk
            const size_t o_q = pairs_align_up(K.nl * sizeof(uint2));
            const size_t o_t = o_q + (size_t)K.qrow * 256;
            H.res.need(o_t + (size_t)K.trow * 256, false, "hits_summary residues");
            K.A.lens = (const uint2*)H.res.d;
            K.A.qres = (const uint32_t*)(H.res.d + o_q);
            K.A.tres = (const uint32_t*)(H.res.d + o_t);
            const uint2* h_sum = nullptr;
            const SummaryArgs A = summary_chunk_args(B.groups, K, T.dev_id, &h_sum);
            HitsGatherArgs GA;
            GA.desc = K.desc;
            GA.groups = K.A.groups;
            GA.table = (const HitsTable*)H.call.d;
            GA.qpool = H.call.d + o_pool;
            // The packed DB is only read.  d_res is immutable between packs (ensure_device_db above was the
            // last one) and every search has synchronised before it returned, so nothing orders this stream
            // against the search streams; d_res_cls, which a search rewrites per query, is not touched.
            GA.dres = D->d_res;
            GA.dgroups = (const uint2*)D->d_groups;
            GA.qres = (uint32_t*)(H.res.d + o_q);
            GA.tres = (uint32_t*)(H.res.d + o_t);
            GA.lens = (uint2*)H.res.d;
            GA.ngroups = (uint32_t)K.ng;
            HS.upload_bytes += K.up_bytes;
            S.pack_ms += now_ms() - tc0;
            // ---- the packer, the end cells, the sweep: launch order is the dependency
            check(hipEventRecord(P.ev[0], T.stream), "hipEventRecord");
            check(launch_hits_gather(GA, T.stream), "hits_gather");
            check(hipEventRecord(P.ev[1], T.stream), "hipEventRecord");
            if (local) {
                LocalArgs LA;
                LA.b = K.A;
                LA.stop = nullptr;
                check(launch_pairs_local(0, cmode, LA, T.stream), "pairs_summary_end");
            } else {
                check(launch_pairs_banded(0, K.A, T.stream), "pairs_summary_end");
            }
            check(hipEventRecord(P.ev[2], T.stream), "hipEventRecord");
            check(launch_pairs_summary(cmode & kLocalBegin, local, A, T.stream), "pairs_summary_sweep");
            check(hipEventRecord(P.ev[3], T.stream), "hipEventRecord");
            check(hipMemcpyAsync(P.out.h, P.out.d, K.nl * sizeof(int2), hipMemcpyDeviceToHost, T.stream),
                  "hits_summary end cells copy");
            check(hipMemcpyAsync((void*)h_sum, A.sum, K.nl * sizeof(uint2), hipMemcpyDeviceToHost, T.stream),
                  "hits_summary words copy");
            check(hipStreamSynchronize(T.stream), "hits_summary synchronize");
            HS.gather_ms += banded_elapsed(0);
            S.fwd_ms += banded_elapsed(1);
            S.dir_ms += banded_elapsed(2);
            S.launches += 3;

            const int2* h_out = (const int2*)P.out.h;
            for (size_t p = K.p0; p < K.p1; p++)
                zeros += summary_record(local, h_out[p - K.p0], h_sum[p - K.p0], out[gat[B.idx[p]]]);
            S.chunks++;
            g0 = K.g1;
        }
        S.zero_pairs += zeros;
    }
    S.kernel_ms = S.fwd_ms + S.dir_ms;
    S.total_ms = now_ms() - t0;
    set_align_pairs_stats(S);
    g_hits_stats = HS;
    return 0;
}

}  // namespace ssa
