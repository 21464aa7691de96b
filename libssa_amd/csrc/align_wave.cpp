// align_wave.cpp -- the wave aligner's host side: region and
// CIGAR of a list of (query, target) pairs, one wave per pair on the device
// (align_wave.hip), for three callers:
//   * compute_alignments (align.cpp): sw_align / nw_align with COMPUTE_ALIGNMENT
//     and ssa_amd_align_hits, on the device of the search's first slot
//     (options "align_wave", "align_wave_min"; ssa_amd_get_align_hits_stats)
//   * ssa_amd_align_pairs under option "pairs_wave" 1 (pairs_align.cpp)
// A chunk's passes are enqueued back to back on one stream -- SW: wave_fwd,
// wave_rev, wave_dir, wave_walk; NW the last two -- between one upload (matrix,
// descriptors, codes) and one copy back (records, runs); the host waits once.
// What the device cannot do exactly goes through traceback() (align.cpp) on
// the host, in parallel.  The aligner owns its stream and its buffers (which
// only grow); an open DB, its device copy and ssa_amd_get_stats are left alone.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "align_wave.h"
#include "pairs_host.h"

namespace ssa {

namespace {

// Device bytes of one chunk; a pair's own direction bits may take half of it.
constexpr size_t kChunkBudget = (size_t)1 << 30;

struct WaveDevice {
    int device = -1;
    bool probed = false, usable = false;
    hipStream_t stream = nullptr;
    hipEvent_t ev[5] = {};
    PairsBuf up, down, scr, fin, dir;
} g_dev;
std::mutex g_mu;                     // one call at a time owns the buffers

ssa_amd_align_pairs_stats_t g_hits_stats = [] {
    ssa_amd_align_pairs_stats_t s{};
    s.device = -1;
    return s;
}();

// Makes `dev` (< 0: ssa_amd_set_device's, else the current HIP device) current
// and the aligner's; false when no HIP device is visible or it is not a gfx950.
bool use_device(int dev) {
    WaveDevice& P = g_dev;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        return false;
    }
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if (dev < 0) dev = cfg().device >= 0 ? cfg().device : cur;
    if (dev >= count) return false;
    if (dev != cur) check(hipSetDevice(dev), "hipSetDevice");
    if (P.probed && P.device == dev) return P.usable;
    if (P.probed && P.usable) {
        // another device than the last call's: its buffers go, on their own device
        check(hipSetDevice(P.device), "hipSetDevice");
        for (PairsBuf* b : {&P.up, &P.down, &P.scr, &P.fin, &P.dir}) b->release();
        (void)hipStreamDestroy(P.stream);
        for (auto& e : P.ev) (void)hipEventDestroy(e);
        P.stream = nullptr;
        check(hipSetDevice(dev), "hipSetDevice");
    }
    P.probed = true;
    P.device = dev;
    P.usable = false;
    hipDeviceProp_t prop;
    check(hipGetDeviceProperties(&prop, dev), "hipGetDeviceProperties");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return false;   // the code object holds gfx950 kernels only
    check(hipStreamCreateWithFlags(&P.stream, hipStreamNonBlocking), "hipStreamCreate");
    for (auto& e : P.ev) check(hipEventCreate(&e), "hipEventCreate");
    P.usable = true;
    return true;
}

// Rows per lane of a call, as engine.cpp long_plan chooses them: the fewest row
// steps, ceil(qlen / 64 RL) passes of RL + kStepRows (the lane's rows and the
// step's fixed work in rows' worth, measured: DESIGN.md §9.6) over the pair's
// columns and the wavefront's 63 steps of skew; ties: the larger RL, fewer passes.
constexpr uint64_t kStepRows = 12;

bool wave_rl_ok(int rl) {
    for (const int x : kWaveRL)
        if (x == rl) return true;
    return false;
}

uint32_t pick_rl(const WaveItem* items, const std::vector<uint32_t>& idx) {
    if (wave_rl_ok(cfg().align_wave_rl)) return (uint32_t)cfg().align_wave_rl;
    uint32_t best = 1;
    uint64_t best_cost = UINT64_MAX;
    for (const int x : kWaveRL) {
        const uint64_t rl = (uint64_t)x;
        uint64_t cost = 0;
        for (const uint32_t i : idx)
            cost += (items[i].qlen + 64 * rl - 1) / (64 * rl) * (rl + kStepRows) * (items[i].dlen + 63);
        if (cost <= best_cost) {
            best_cost = cost;
            best = (uint32_t)rl;
        }
    }
    return best;
}

}  // namespace

const ssa_amd_align_pairs_stats_t& align_hits_stats() { return g_hits_stats; }

void align_wave(int algo, const WaveItem* items, size_t n, int device, bool allow_device, bool want_score,
                ssa_amd_pair_alignment_t* out, ssa_amd_align_pairs_stats_t& S) {
    const double t0 = now_ms();
    const bool nw = algo == kAlgoNW;
    static const char* const kNames[2] = {"wave_fwd,wave_rev,wave_dir,wave_walk", "wave_dir,wave_walk"};
    S = ssa_amd_align_pairs_stats_t{};
    S.pairs = n;
    S.device = -1;
    if (n == 0) return;
    if (!matrix().ready) fatal("Scoring matrix not initialized");
    std::lock_guard<std::mutex> lock(g_mu);

    const Config& C = cfg();
    const int64_t* M = matrix().m;
    const int64_t Q = C.gap_open, Ge = C.gap_extend;
    // the device's conditions are ssa_amd_align_pairs' (pairs_align.cpp)
    int64_t max_abs = 0;
    bool int8_matrix = true, symmetric = true;
    for (int i = 0; i < kDim * kDim; i++) {
        if (M[i] < -128 || M[i] > 127) int8_matrix = false;
        if (M[i] != M[((i & 31) << 5) + (i >> 5)]) symmetric = false;
        max_abs = std::max<int64_t>(max_abs, std::llabs(M[i]));
    }
    bool dev_ok = allow_device && int8_matrix && Q <= 0 && Ge <= 0 && (nw || symmetric) && n <= UINT32_MAX;
    if (dev_ok) dev_ok = use_device(device);
    const int64_t per_residue = max_abs + std::llabs(Ge);
    const int64_t residue_limit = per_residue ? (((int64_t)1 << 29) - 2 * std::llabs(Q)) / per_residue : INT64_MAX;

    std::vector<uint32_t> dev_idx;   // the pairs the device aligns, by input index
    std::vector<size_t> todo;        // the pairs of the host path
    for (size_t i = 0; i < n; i++) {
        const uint64_t ql = items[i].qlen, dl = items[i].dlen;
        S.cells += ql * dl;
        bool codes_ok = dev_ok && ql && dl && (int64_t)(ql + dl) <= residue_limit && ql < kWaveMaxLen && dl < kWaveMaxLen;
        if (codes_ok) dev_idx.push_back((uint32_t)i);
        else todo.push_back(i);
    }
    const uint32_t rl = dev_idx.empty() ? 1 : pick_rl(items, dev_idx);
    {
        // the pair's own direction bits, in this call's layout, fit half a chunk
        std::vector<uint32_t> keep;
        for (const uint32_t i : dev_idx) {
            if (wave_dir_bytes(rl, items[i].qlen, items[i].dlen) <= kChunkBudget / 2) keep.push_back(i);
            else todo.push_back(i);
        }
        dev_idx.swap(keep);
    }
    auto run_host = [&](const std::vector<size_t>& list) {
        if (list.empty()) return;
        const double th0 = now_ms();
        parallel_ranges(list.size(), list.size() <= 256 ? 1 : 4, [&](size_t b, size_t e) {
            std::vector<int64_t> he;
            for (size_t k = b; k < e; k++) {
                const WaveItem& it = items[list[k]];
                ssa_amd_pair_alignment_t& o = out[list[k]];
                o.score = 0;
                if (want_score) {
                    if (he.size() < 2 * it.qlen) he.resize(2 * it.qlen);
                    o.score = nw ? host_nw(it.d, it.dlen, it.q, it.qlen, M, Q, Ge, he.data())
                                 : host_sw(it.d, it.dlen, it.q, it.qlen, M, Q, Ge, he.data());
                }
                size_t rg[4];
                const std::string c = traceback(algo, it.q, it.qlen, it.d, it.dlen, rg);
                for (int r = 0; r < 4; r++) o.region[r] = rg[r];
                memcpy(it.text, c.c_str(), c.size() + 1);     // (at most qlen + dlen operations: the slot holds it)
                o.cigar_len = (uint32_t)c.size();
                o.flags = 1;
            }
        });
        S.host_pairs += list.size();
        S.host_ms += now_ms() - th0;
    };
    run_host(todo);
    todo.clear();                    // from here on: device pairs a pass gave no cell for (expected none)

    if (!dev_idx.empty()) {
        WaveDevice& P = g_dev;
        S.device = P.device;
        S.groups = (uint32_t)dev_idx.size();
        snprintf(S.kernels, sizeof S.kernels, "%s", kNames[nw ? 1 : 0]);
        // longest first: the launch ends on short pairs
        const double tp0 = now_ms();
        std::stable_sort(dev_idx.begin(), dev_idx.end(), [&](uint32_t x, uint32_t y) {
            return (uint64_t)items[x].qlen * items[x].dlen > (uint64_t)items[y].qlen * items[y].dlen;
        });
        int8_t mt[32 * 32];
        for (int q = 0; q < kDim; q++)
            for (int d = 0; d < kDim; d++) mt[q * 32 + d] = (int8_t)M[(d << 5) + q];
        S.pack_ms += now_ms() - tp0;

        const size_t npd = dev_idx.size();
        for (size_t p0 = 0; p0 < npd;) {
            // ---- the chunk: pairs [p0, p1) within the byte budget (at least one)
            const double tc0 = now_ms();
            size_t p1 = p0, bytes = 0;
            uint64_t ncodes = 0, nscr = 0, nfin = 0, nruns = 0, ndir = 0;
            std::vector<WavePair> desc;
            while (p1 < npd) {
                const WaveItem& it = items[dev_idx[p1]];
                const uint64_t ql = it.qlen, dl = it.dlen;
                const uint64_t dirb = pairs_align_up(wave_dir_bytes(rl, ql, dl));
                const size_t pb = (size_t)(ql + dl + 3) + sizeof(WavePair) + sizeof(WaveRec) + dirb + 16 * dl +
                                  (nw ? 0 : 8 * ql) + 4 * (ql + dl);
                if (p1 > p0 && bytes + pb > kChunkBudget) break;
                WavePair D{};
                D.q_off = (uint32_t)ncodes;
                D.d_off = (uint32_t)(ncodes + ql);
                D.qlen = (uint32_t)ql;
                D.dlen = (uint32_t)dl;
                D.dir_off = ndir;
                D.scr_off = (uint32_t)nscr;
                D.fin_off = (uint32_t)nfin;
                D.runs_off = (uint32_t)nruns;
                desc.push_back(D);
                ncodes += (ql + dl + 3) & ~(uint64_t)3;
                nscr += 2 * dl;
                nfin += nw ? 0 : ql;
                nruns += ql + dl;
                ndir += dirb;
                bytes += pb;
                p1++;
            }
            const size_t np = p1 - p0;
            const size_t o_desc = pairs_align_up(sizeof mt);
            const size_t o_codes = o_desc + pairs_align_up(np * sizeof(WavePair));
            const size_t up_bytes = o_codes + (size_t)ncodes;
            const size_t o_runs = pairs_align_up(np * sizeof(WaveRec));
            const size_t down_bytes = o_runs + (size_t)nruns * sizeof(uint32_t);
            P.up.need(up_bytes, true, "align_wave upload");
            P.down.need(down_bytes, true, "align_wave results");
            P.scr.need(std::max<size_t>(nscr, 1) * sizeof(int64_t), false, "align_wave scratch rows");
            P.fin.need(std::max<size_t>(nfin, 1) * sizeof(int2), false, "align_wave fin rows");
            P.dir.need(std::max<size_t>(ndir, 1), false, "align_wave direction bits");
            S.dir_bytes += ndir;

            memcpy(P.up.h, mt, sizeof mt);
            memcpy(P.up.h + o_desc, desc.data(), np * sizeof(WavePair));
            parallel_ranges(np, 64, [&](size_t b, size_t e) {
                for (size_t k = b; k < e; k++) {
                    const WaveItem& it = items[dev_idx[p0 + k]];
                    memcpy(P.up.h + o_codes + desc[k].q_off, it.q, it.qlen);
                    memcpy(P.up.h + o_codes + desc[k].d_off, it.d, it.dlen);
                }
            });
            S.pack_ms += now_ms() - tc0;

            hipStream_t st = P.stream;
            check(hipMemcpyAsync(P.up.d, P.up.h, up_bytes, hipMemcpyHostToDevice, st), "align_wave upload");
            WaveArgs A{};
            A.mt = (const int8_t*)P.up.d;
            A.pairs = (const WavePair*)(P.up.d + o_desc);
            A.codes = P.up.d + o_codes;
            A.rec = (WaveRec*)P.down.d;
            A.runs = (uint32_t*)(P.down.d + o_runs);
            A.scr = (int64_t*)P.scr.d;
            A.fin = (int2*)P.fin.d;
            A.dir = P.dir.d;
            A.gap_open = (int32_t)Q;
            A.gap_extend = (int32_t)Ge;
            A.npairs = (uint32_t)np;
            A.rl = rl;
            check(hipEventRecord(P.ev[0], st), "hipEventRecord");
            if (!nw) {
                check(launch_align_wave(0, false, A, st), "wave_fwd");
                check(hipEventRecord(P.ev[1], st), "hipEventRecord");
                check(launch_align_wave(1, false, A, st), "wave_rev");
            }
            check(hipEventRecord(P.ev[2], st), "hipEventRecord");
            check(launch_align_wave(2, nw, A, st), "wave_dir");
            check(hipEventRecord(P.ev[3], st), "hipEventRecord");
            check(launch_align_wave(3, nw, A, st), "wave_walk");
            check(hipEventRecord(P.ev[4], st), "hipEventRecord");
            check(hipMemcpyAsync(P.down.h, P.down.d, down_bytes, hipMemcpyDeviceToHost, st), "align_wave results copy");
            check(hipStreamSynchronize(st), "align_wave synchronize");
            auto elapsed = [&](int e0, int e1) {
                float ms = 0;
                check(hipEventElapsedTime(&ms, P.ev[e0], P.ev[e1]), "hipEventElapsedTime");
                return (double)ms;
            };
            if (!nw) {
                S.fwd_ms += elapsed(0, 1);
                S.rev_ms += elapsed(1, 2);
            }
            S.dir_ms += elapsed(2, 3);
            S.walk_ms += elapsed(3, 4);
            S.launches += nw ? 2 : 4;

            // ---- text
            const double tt0 = now_ms();
            const WaveRec* recs = (const WaveRec*)P.down.h;
            const uint32_t* h_runs = (const uint32_t*)(P.down.h + o_runs);
            std::atomic<uint64_t> zeros{0};
            std::vector<uint8_t> failed(np, 0);
            parallel_ranges(np, 64, [&](size_t b, size_t e) {
                uint64_t z = 0;
                for (size_t k = b; k < e; k++) {
                    const uint32_t i = dev_idx[p0 + k];
                    const WaveRec& R = recs[k];
                    ssa_amd_pair_alignment_t& o = out[i];
                    char* text = items[i].text;
                    const uint32_t cap = desc[k].qlen + desc[k].dlen;
                    if (R.state == kWaveZero && !nw) {
                        // a zero pair: traceback()'s (0, 0, 0, 0) and an empty CIGAR
                        o.score = 0;
                        for (auto& r : o.region) r = 0;
                        o.cigar_len = 0;
                        o.flags = 0;
                        text[0] = 0;
                        z++;
                        continue;
                    }
                    if (R.state != kWaveOk || R.a_end >= desc[k].qlen || R.b_end >= desc[k].dlen ||
                        R.a_begin > R.a_end || R.b_begin > R.b_end || R.nruns > cap) {
                        failed[k] = 1;       // the host routine decides (it reports the reference's internal error)
                        continue;
                    }
                    o.score = R.score;
                    o.region[0] = R.a_begin;
                    o.region[1] = R.a_end;
                    o.region[2] = R.b_begin;
                    o.region[3] = R.b_end;
                    o.cigar_len = format_runs(h_runs + desc[k].runs_off, R.nruns, text);
                    o.flags = 0;
                }
                zeros.fetch_add(z);
            });
            for (size_t k = 0; k < np; k++)
                if (failed[k]) todo.push_back(dev_idx[p0 + k]);
            S.zero_pairs += zeros.load();
            S.text_ms += now_ms() - tt0;
            S.chunks++;
            p0 = p1;
        }
        if (!todo.empty()) {
            S.device_fallbacks = todo.size();
            run_host(todo);
        }
    }
    S.kernel_ms = S.fwd_ms + S.rev_ms + S.dir_ms + S.walk_ms;
    S.total_ms = now_ms() - t0;
}

// compute_alignments' body (align.cpp): region and CIGAR of every alignment of
// the list, on the wave kernels unless option "align_wave" 0 or a list shorter
// than "align_wave_min" keeps the call on the host threads.
void align_hits(p_alignment_list L, int algo) {
    const double t0 = now_ms();
    const size_t n = L->len;
    const Config& C = cfg();
    ssa_amd_align_pairs_stats_t S{};
    S.pairs = n;
    S.device = -1;
    if (n == 0) {
        g_hits_stats = S;
        return;
    }
    if (!C.align_wave || n < (size_t)std::max(C.align_wave_min, 0)) {
        compute_alignments_host(L, algo);
        for (size_t i = 0; i < n; i++) S.cells += (uint64_t)L->alignments[i]->query.len * L->alignments[i]->db_seq.len;
        S.host_pairs = n;
        S.host_ms = S.total_ms = now_ms() - t0;
        g_hits_stats = S;
        return;
    }
    std::vector<WaveItem> items(n);
    std::vector<size_t> toff(n + 1, 0);
    for (size_t i = 0; i < n; i++) {
        const p_alignment a = L->alignments[i];
        toff[i + 1] = toff[i] + a->query.len + a->db_seq.len + 1;
    }
    std::vector<char> text(toff[n]);
    for (size_t i = 0; i < n; i++) {
        const p_alignment a = L->alignments[i];
        items[i] = WaveItem{(const uint8_t*)a->query.seq, a->query.len, (const uint8_t*)a->db_seq.seq, a->db_seq.len,
                            text.data() + toff[i]};
    }
    std::vector<ssa_amd_pair_alignment_t> out(n);
    const int dev = device_db(0).device;      // the search's first slot
    align_wave(algo, items.data(), n, dev, true, false, out.data(), S);
    for (size_t i = 0; i < n; i++) {
        p_alignment a = L->alignments[i];
        a->align_q_start = out[i].region[0];
        a->align_q_end = out[i].region[1];
        a->align_d_start = out[i].region[2];
        a->align_d_end = out[i].region[3];
        a->alignment = (char*)malloc((size_t)out[i].cigar_len + 1);
        memcpy(a->alignment, items[i].text, (size_t)out[i].cigar_len + 1);
        a->alignment_len = out[i].cigar_len;
    }
    S.total_ms = now_ms() - t0;
    g_hits_stats = S;
}

}  // namespace ssa
