// pairs_align.cpp -- ssa_amd_align_pairs: region and CIGAR of a batch of
// independent (query, target) pairs in one call.  The batch
// is ordered and packed as ssa_amd_score_pairs packs it (pairs.cpp) and goes
// through four kernels per chunk (pairs_align.hip): SW forward (the end
// cell), SW reverse (the begin cell), directions, walk.  Between the passes
// the host reads the ends / begins back and packs what the next pass needs.
// What the device cannot do exactly goes through traceback() (align.cpp), the
// routine ssa_amd_align_pair runs, in parallel on the host.  The call shares
// ssa_amd_score_pairs' stream and owns its buffers; an open DB, its device
// copy and ssa_amd_get_stats are not touched.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pairs_host.h"

namespace ssa {

namespace {

ssa_amd_align_pairs_stats_t g_stats;

// Device bytes of one chunk.  The direction bits dominate: a group costs
// nstrips * ncb * 512 B of them (64 pairs of 390 x 513: 3.2 MB), against
// 256 MiB for a whole chunk of ssa_amd_score_pairs; each chunk costs two host
// round trips, so the budget is larger here.
constexpr size_t kChunkBudget = (size_t)1 << 30;

using Buf = PairsBuf;
inline size_t align_up(size_t x) { return pairs_align_up(x); }

struct AlignDevice {
    int device = -1;
    hipEvent_t ev[7] = {};
    bool events = false;
    Buf up, up2, bnd, fin, dir, runs, out;
} g_dev;

// One pair on the host: ssa_amd_align_pair's routine and the exact int64 score.
void host_align(bool nw, const uint8_t* q, size_t ql, const uint8_t* d, size_t dl, std::vector<int64_t>& he,
                ssa_amd_pair_alignment_t& o, char* text) {
    const int64_t* M = matrix().m;
    const int64_t Q = cfg().gap_open, Ge = cfg().gap_extend;
    if (he.size() < 2 * ql) he.resize(2 * ql);
    o.score = nw ? host_nw(d, dl, q, ql, M, Q, Ge, he.data()) : host_sw(d, dl, q, ql, M, Q, Ge, he.data());
    size_t rg[4];
    const std::string c = traceback(nw ? kAlgoNW : kAlgoSW, q, ql, d, dl, rg);
    for (int k = 0; k < 4; k++) o.region[k] = rg[k];
    memcpy(text, c.c_str(), c.size() + 1);     // (at most ql + dl operations: the slot holds it)
    o.cigar_len = (uint32_t)c.size();
    o.flags = 1;
}

}  // namespace

const ssa_amd_align_pairs_stats_t& align_pairs_stats() { return g_stats; }
void set_align_pairs_stats(const ssa_amd_align_pairs_stats_t& s) { g_stats = s; }

int align_pairs(int algo, const uint8_t* qc, const uint64_t* qoff, const uint8_t* dc, const uint64_t* doff, size_t n,
                ssa_amd_pair_alignment_t* out, char* cigars, size_t cigar_cap) {
    const double t0 = now_ms();
    if (algo != SSA_AMD_SW && algo != SSA_AMD_NW) return 1;
    const bool nw = algo == SSA_AMD_NW;
    static const char* const kNames[2] = {"pairs_align_fwd,pairs_align_rev,pairs_align_dir_sw,pairs_align_walk",
                                          "pairs_align_dir_nw,pairs_align_walk"};
    if (n == 0) {
        g_stats = ssa_amd_align_pairs_stats_t{};
        g_stats.device = -1;
        return 0;
    }
    if (!qc || !qoff || !dc || !doff || !out || !cigars) return 1;
    if (!matrix().ready) fatal("Scoring matrix not initialized");
    for (size_t i = 0; i < n; i++)
        if (qoff[i + 1] < qoff[i] || doff[i + 1] < doff[i]) return 1;
    // every residue is a code < 32 (the matrix is 32 x 32)
    {
        std::atomic<uint32_t> seen{0};
        auto scan = [&](const uint8_t* p, size_t len) {
            parallel_ranges(len, 1 << 20, [&](size_t b, size_t e) {
                uint8_t acc = 0;
                for (size_t i = b; i < e; i++) acc |= p[i];
                seen.fetch_or(acc);
            });
        };
        scan(qc + qoff[0], qoff[n] - qoff[0]);
        scan(dc + doff[0], doff[n] - doff[0]);
        if (seen.load() >= (uint32_t)kDim) return 1;
    }
    // every pair's CIGAR slot: qlen + dlen + 1 bytes, in input order
    std::vector<uint64_t> coff(n + 1);
    coff[0] = 0;
    for (size_t i = 0; i < n; i++) coff[i + 1] = coff[i] + (qoff[i + 1] - qoff[i]) + (doff[i + 1] - doff[i]) + 1;
    if (cigar_cap < coff[n]) return 1;

    if (cfg().pairs_wave) {
        // option "pairs_wave": one wave per pair (align_wave.cpp) instead of one pair per lane
        std::vector<WaveItem> items(n);
        for (size_t i = 0; i < n; i++) {
            items[i] = WaveItem{qc + qoff[i], (size_t)(qoff[i + 1] - qoff[i]), dc + doff[i],
                                (size_t)(doff[i + 1] - doff[i]), cigars + coff[i]};
            out[i].cigar_off = coff[i];
        }
        align_wave(nw ? kAlgoNW : kAlgoSW, items.data(), n, -1, !cfg().pairs_host, true, out, g_stats);
        g_stats.total_ms = now_ms() - t0;
        return 0;
    }

    const Config& C = cfg();
    const int64_t* M = matrix().m;
    const int64_t Q = C.gap_open, Ge = C.gap_extend;
    // the device's conditions are ssa_amd_score_pairs' (pairs.cpp); SW also needs M[a][b] == M[b][a]: the
    // reference's region passes score M[query][db], the kernels M[db][query]
    int64_t max_abs = 0;
    bool int8_matrix = true, symmetric = true;
    for (int i = 0; i < kDim * kDim; i++) {
        if (M[i] < -128 || M[i] > 127) int8_matrix = false;
        if (M[i] != M[((i & 31) << 5) + (i >> 5)]) symmetric = false;
        max_abs = std::max<int64_t>(max_abs, std::llabs(M[i]));
    }
    bool device = !C.pairs_host && int8_matrix && Q <= 0 && Ge <= 0 && (nw || symmetric) && n <= UINT32_MAX;
    int dev_id = -1;
    hipStream_t stream = nullptr;
    if (device) device = pairs_use_device(&dev_id, &stream);
    const int64_t per_residue = max_abs + std::llabs(Ge);
    const int64_t residue_limit = per_residue ? (((int64_t)1 << 29) - 2 * std::llabs(Q)) / per_residue : INT64_MAX;

    ssa_amd_align_pairs_stats_t S{};
    S.pairs = n;
    S.device = device ? dev_id : -1;
    snprintf(S.kernels, sizeof S.kernels, "%s", kNames[nw ? 1 : 0]);

    auto qlen = [&](size_t i) { return (uint32_t)(qoff[i + 1] - qoff[i]); };
    auto dlen = [&](size_t i) { return (uint32_t)(doff[i + 1] - doff[i]); };
    auto strips = [&](size_t i) { return (qlen(i) + kPairsRows - 1) / kPairsRows; };

    std::vector<uint32_t> dev_idx;   // the pairs the device aligns, by input index
    std::vector<size_t> todo;        // the pairs of the host path
    {
        uint64_t cells = 0;
        for (size_t i = 0; i < n; i++) {
            const uint64_t ql = qoff[i + 1] - qoff[i], dl = doff[i + 1] - doff[i];
            cells += ql * dl;
            // (b) positions travel as col << 16 | row; (c) the pair's direction bits alone fit a chunk
            if (device && ql && dl && (int64_t)(ql + dl) <= residue_limit && ql < kAlignMaxLen && dl < kAlignMaxLen &&
                ((ql + 7) / 8) * ((dl + 3) / 4) * 512 <= kChunkBudget / 2)
                dev_idx.push_back((uint32_t)i);
            else
                todo.push_back(i);
        }
        S.cells = cells;
    }
    auto run_host = [&](const std::vector<size_t>& list) {
        const double th0 = now_ms();
        parallel_ranges(list.size(), 4, [&](size_t b, size_t e) {
            std::vector<int64_t> he;
            for (size_t k = b; k < e; k++) {
                const size_t i = list[k];
                out[i].cigar_off = coff[i];
                host_align(nw, qc + qoff[i], qlen(i), dc + doff[i], dlen(i), he, out[i], cigars + coff[i]);
            }
        });
        S.host_pairs += list.size();
        S.host_ms += now_ms() - th0;
    };
    run_host(todo);
    todo.clear();                    // from here on: device pairs a pass gave no cell for (expected none)

    if (!dev_idx.empty()) {
        AlignDevice& P = g_dev;
        if (P.device != dev_id) {
            for (Buf* b : {&P.up, &P.up2, &P.bnd, &P.fin, &P.dir, &P.runs, &P.out}) b->release();
            P.device = dev_id;
        }
        if (!P.events) {
            for (auto& e : P.ev) check(hipEventCreate(&e), "hipEventCreate");
            P.events = true;
        }
        // a wave sweeps (most strips) x (most columns) of its 64 pairs: order by both, longest first
        const double tp0 = now_ms();
        {
            struct Key {
                uint64_t shape;   // strips << 32 | dlen
                uint32_t pair;
            };
            std::vector<Key> keys(dev_idx.size());
            for (size_t p = 0; p < keys.size(); p++)
                keys[p] = Key{(uint64_t)strips(dev_idx[p]) << 32 | dlen(dev_idx[p]), dev_idx[p]};
            std::sort(keys.begin(), keys.end(), [](const Key& x, const Key& y) {
                return x.shape != y.shape ? x.shape > y.shape : x.pair < y.pair;
            });
            for (size_t p = 0; p < keys.size(); p++) dev_idx[p] = keys[p].pair;
        }
        const size_t npd = dev_idx.size();
        const size_t ngroups = (npd + 63) / 64;
        std::vector<AlignGroup> groups(ngroups);
        std::vector<size_t> gbytes(ngroups);
        for (size_t g = 0; g < ngroups; g++) {
            uint32_t md = 0, ms = 0;
            uint64_t ops = 0;
            for (size_t p = g * 64; p < std::min(npd, g * 64 + 64); p++) {
                md = std::max(md, dlen(dev_idx[p]));
                ms = std::max(ms, strips(dev_idx[p]));
                ops += (uint64_t)qlen(dev_idx[p]) + dlen(dev_idx[p]);
            }
            AlignGroup& G = groups[g];
            G = AlignGroup{};
            G.ncb = (md + 3) / 4;
            G.nstrips = ms;
            // residues (both directions), bnd, fin, direction bits, run slots, per-lane words
            gbytes[g] = 2 * ((size_t)G.ncb * 256 + (size_t)G.nstrips * 512) + (size_t)G.ncb * 4 * 512 +
                        (size_t)G.nstrips * 8 * 512 + (size_t)G.nstrips * G.ncb * 512 + ops * 4 +
                        64 * (sizeof(uint2) + sizeof(AlignLane) + 2 * sizeof(int2)) + 2 * sizeof(AlignGroup);
        }
        S.groups = (uint32_t)ngroups;
        S.pack_ms += now_ms() - tp0;

        // the compact matrix, transposed: mt[q][d] = M[d][q], padding row zero
        int8_t mt[kPairsCodes * 32] = {};
        for (int q = 0; q < kDim; q++)
            for (int d = 0; d < kDim; d++) mt[q * 32 + d] = (int8_t)M[(d << 5) + q];

        const size_t chunk_groups = C.pairs_chunk > 0 ? std::max<size_t>(1, (size_t)C.pairs_chunk / 64) : SIZE_MAX;
        for (size_t g0 = 0; g0 < ngroups;) {
            // ---- the chunk: groups [g0, g1) within the byte budget (at least one)
            const double tc0 = now_ms();
            size_t g1 = g0, bytes = 0;
            uint64_t trow = 0, qrow = 0, brow = 0;
            while (g1 < ngroups && g1 - g0 < chunk_groups) {
                if (g1 > g0 && bytes + gbytes[g1] > kChunkBudget) break;
                groups[g1].t_row = (uint32_t)trow;
                groups[g1].q_row = (uint32_t)qrow;
                groups[g1].b_row = (uint32_t)brow;
                trow += groups[g1].ncb;
                qrow += (uint64_t)groups[g1].nstrips * 2;
                brow += (uint64_t)groups[g1].ncb * 4;
                bytes += gbytes[g1];
                g1++;
            }
            const size_t ng = g1 - g0, nl = ng * 64;
            const size_t p0 = g0 * 64, p1 = std::min(npd, g1 * 64);
            // upload block 1: matrix, lens, query and target residues
            const size_t o_lens = align_up(sizeof mt);
            const size_t o_q = o_lens + align_up(nl * sizeof(uint2));
            const size_t o_t = o_q + (size_t)qrow * 256;
            const size_t up_bytes = o_t + (size_t)trow * 256;
            // upload block 2: the later passes' groups and lanes, the reversed prefixes (SW)
            const size_t o_lanes = align_up(ng * sizeof(AlignGroup));
            const size_t o_rq = o_lanes + align_up(nl * sizeof(AlignLane));
            const size_t o_rt = o_rq + (nw ? 0 : (size_t)qrow * 256);
            const size_t up2_bytes = o_rt + (nw ? 0 : (size_t)trow * 256);
            const size_t o_g1 = up_bytes;        // block 1's own copy of the groups (pass 1's extents)
            P.up.need(o_g1 + align_up(ng * sizeof(AlignGroup)), true, "align_pairs residues");
            P.up2.need(up2_bytes, true, "align_pairs lanes");
            P.bnd.need((size_t)brow * 512, false, "align_pairs boundary buffer");
            P.fin.need((size_t)qrow * 4 * 512, false, "align_pairs fin buffer");
            P.out.need(2 * nl * sizeof(int2), true, "align_pairs results");

            // ---- pack, lane-interleaved
            memcpy(P.up.h, mt, sizeof mt);
            memcpy(P.up.h + o_g1, &groups[g0], ng * sizeof(AlignGroup));
            uint2* h_lens = (uint2*)(P.up.h + o_lens);
            parallel_ranges(ng, 1, [&](size_t b, size_t e) {
                for (size_t g = g0 + b; g < g0 + e; g++) {
                    const AlignGroup& G = groups[g];
                    uint8_t* tq = P.up.h + o_q + (size_t)G.q_row * 256;
                    uint8_t* tt = P.up.h + o_t + (size_t)G.t_row * 256;
                    memset(tq, (int)kPairsPad, (size_t)G.nstrips * 2 * 256);
                    memset(tt, (int)kPairsPad, (size_t)G.ncb * 256);
                    for (size_t l = 0; l < 64; l++) {
                        const size_t p = g * 64 + l;
                        uint2& L = h_lens[(g - g0) * 64 + l];
                        if (p >= npd) {
                            L = make_uint2(0, 0);
                            continue;
                        }
                        const uint32_t i = dev_idx[p];
                        L = make_uint2(qlen(i), dlen(i));
                        interleave(tq + l * 4, qc + qoff[i], qlen(i));
                        interleave(tt + l * 4, dc + doff[i], dlen(i));
                    }
                }
            });
            S.pack_ms += now_ms() - tc0;
            check(hipMemcpyAsync(P.up.d, P.up.h, o_g1 + ng * sizeof(AlignGroup), hipMemcpyHostToDevice, stream),
                  "align_pairs upload");
            AlignArgs A{};
            A.mt = (const int8_t*)P.up.d;
            A.lens = (const uint2*)(P.up.d + o_lens);
            A.qres = (const uint32_t*)(P.up.d + o_q);
            A.tres = (const uint32_t*)(P.up.d + o_t);
            A.groups = (const AlignGroup*)(P.up.d + o_g1);
            A.lanes = (const AlignLane*)(P.up2.d + o_lanes);
            A.bnd = (int2*)P.bnd.d;
            A.fin = (int2*)P.fin.d;
            A.out = (int2*)P.out.d;
            A.gap_open = (int32_t)Q;
            A.gap_extend = (int32_t)Ge;
            A.ngroups = (uint32_t)ng;
            const int2* h_out = (const int2*)P.out.h;
            auto fetch = [&](size_t half) {
                check(hipMemcpyAsync(P.out.h + half * nl * sizeof(int2), P.out.d + half * nl * sizeof(int2),
                                     nl * sizeof(int2), hipMemcpyDeviceToHost, stream),
                      "align_pairs results copy");
            };
            auto elapsed = [&](int e) {
                float ms = 0;
                check(hipEventElapsedTime(&ms, P.ev[e], P.ev[e + 1]), "hipEventElapsedTime");
                return (double)ms;
            };

            // the later passes' view of the chunk: per-lane ends / begins, the extents they leave each group
            AlignGroup* groups2 = (AlignGroup*)P.up2.h;
            AlignLane* lanes = (AlignLane*)(P.up2.h + o_lanes);
            memcpy(groups2, &groups[g0], ng * sizeof(AlignGroup));
            memset(lanes, 0, nl * sizeof(AlignLane));
            std::vector<int32_t> best(nl, 0);   // SW: the maximum; < 0: the pair went to the host list
            double tp1 = now_ms();              // start of the host work between two passes

            if (!nw) {
                // ---- pass 1: the end cell
                check(hipEventRecord(P.ev[0], stream), "hipEventRecord");
                check(launch_pairs_align(0, false, A, stream), "pairs_align_fwd");
                check(hipEventRecord(P.ev[1], stream), "hipEventRecord");
                fetch(0);
                check(hipStreamSynchronize(stream), "align_pairs synchronize");
                S.fwd_ms += elapsed(0);
                S.launches++;
                tp1 = now_ms();
                for (size_t p = p0; p < p1; p++) {
                    const size_t l = p - p0;
                    const uint32_t i = dev_idx[p];
                    const int2 r = h_out[l];
                    const uint32_t pos = (uint32_t)r.y;
                    best[l] = r.x;
                    if (r.x <= 0) continue;      // a zero pair: unused from here on
                    if (pos >= kAlignNoPos || (pos & 0xffff) >= qlen(i) || (pos >> 16) >= dlen(i)) {
                        // (cannot happen, pairs_align.hip's header: the host routine decides)
                        best[l] = -1;
                        todo.push_back(i);
                        continue;
                    }
                    lanes[l].a_end = pos & 0xffff;
                    lanes[l].b_end = pos >> 16;
                    lanes[l].best = r.x;
                    lanes[l].used = 1;
                }
                // the reversed prefixes q[a_end..0], d[b_end..0], and the extents they need
                parallel_ranges(ng, 1, [&](size_t b, size_t e) {
                    std::vector<uint8_t> rev;
                    for (size_t g = b; g < e; g++) {
                        AlignGroup& G = groups2[g];
                        uint8_t* tq = P.up2.h + o_rq + (size_t)G.q_row * 256;
                        uint8_t* tt = P.up2.h + o_rt + (size_t)G.t_row * 256;
                        memset(tq, (int)kPairsPad, (size_t)G.nstrips * 2 * 256);
                        memset(tt, (int)kPairsPad, (size_t)G.ncb * 256);
                        uint32_t ma = 0, mb = 0;
                        for (size_t l = 0; l < 64; l++) {
                            const AlignLane& L = lanes[g * 64 + l];
                            if (!L.used) continue;
                            const uint32_t i = dev_idx[p0 + g * 64 + l];
                            ma = std::max(ma, L.a_end + 1);
                            mb = std::max(mb, L.b_end + 1);
                            rev.assign(qc + qoff[i], qc + qoff[i] + L.a_end + 1);
                            std::reverse(rev.begin(), rev.end());
                            interleave(tq + l * 4, rev.data(), L.a_end + 1);
                            rev.assign(dc + doff[i], dc + doff[i] + L.b_end + 1);
                            std::reverse(rev.begin(), rev.end());
                            interleave(tt + l * 4, rev.data(), L.b_end + 1);
                        }
                        G.nstrips = (ma + kPairsRows - 1) / kPairsRows;
                        G.ncb = (mb + 3) / 4;
                    }
                });
            } else {
                for (size_t p = p0; p < p1; p++) {
                    AlignLane& L = lanes[p - p0];
                    L.a_end = qlen(dev_idx[p]) - 1;
                    L.b_end = dlen(dev_idx[p]) - 1;
                    L.used = 1;
                }
            }
            // the direction bits of the (shrunk) extents
            uint64_t drow = 0;
            for (size_t g = 0; g < ng; g++) {
                groups2[g].d_row = (uint32_t)drow;
                drow += (uint64_t)groups2[g].nstrips * groups2[g].ncb;
            }
            P.dir.need((size_t)drow * 512, false, "align_pairs direction bits");
            S.dir_bytes += drow * 512;
            A.dir = (uint2*)P.dir.d;

            if (!nw) {
                S.pack_ms += now_ms() - tp1;
                // ---- pass 2: the begin cell
                check(hipMemcpyAsync(P.up2.d, P.up2.h, up2_bytes, hipMemcpyHostToDevice, stream), "align_pairs upload");
                AlignArgs A2 = A;
                A2.groups = (const AlignGroup*)P.up2.d;
                A2.qres = (const uint32_t*)(P.up2.d + o_rq);
                A2.tres = (const uint32_t*)(P.up2.d + o_rt);
                check(hipEventRecord(P.ev[2], stream), "hipEventRecord");
                check(launch_pairs_align(1, false, A2, stream), "pairs_align_rev");
                check(hipEventRecord(P.ev[3], stream), "hipEventRecord");
                fetch(0);
                check(hipStreamSynchronize(stream), "align_pairs synchronize");
                S.rev_ms += elapsed(2);
                S.launches++;
                tp1 = now_ms();
                for (size_t l = 0; l < p1 - p0; l++) {
                    AlignLane& L = lanes[l];
                    if (!L.used) continue;
                    const uint32_t pos = (uint32_t)h_out[l].x;
                    if (pos >= kAlignNoPos || (pos & 0xffff) > L.a_end || (pos >> 16) > L.b_end) {
                        // no begin found: the host routine decides (it reports the reference's internal error)
                        L.used = 0;
                        best[l] = -1;
                        todo.push_back(dev_idx[p0 + l]);
                        continue;
                    }
                    L.a_begin = L.a_end - (pos & 0xffff);
                    L.b_begin = L.b_end - (pos >> 16);
                }
            }
            // the walk's run slots: a walk makes at most (rows + columns of the region) steps
            uint64_t nruns = 0;
            for (size_t l = 0; l < p1 - p0; l++) {
                AlignLane& L = lanes[l];
                if (!L.used) continue;
                L.cap = (L.a_end - L.a_begin + 1) + (L.b_end - L.b_begin + 1);
                L.slot = (uint32_t)nruns;
                nruns += L.cap;
            }
            P.runs.need(std::max<size_t>(nruns, 1) * sizeof(uint32_t), true, "align_pairs runs");
            A.runs = (uint32_t*)P.runs.d;
            S.pack_ms += now_ms() - tp1;
            // ---- passes 3 and 4: directions, walk
            check(hipMemcpyAsync(P.up2.d, P.up2.h, o_rq, hipMemcpyHostToDevice, stream), "align_pairs upload");
            AlignArgs A3 = A;
            A3.groups = (const AlignGroup*)P.up2.d;
            check(hipEventRecord(P.ev[4], stream), "hipEventRecord");
            check(launch_pairs_align(2, nw, A3, stream), "pairs_align_dir");
            check(hipEventRecord(P.ev[5], stream), "hipEventRecord");
            AlignArgs A4 = A3;
            A4.out = A.out + nl;
            check(launch_pairs_align(3, nw, A4, stream), "pairs_align_walk");
            check(hipEventRecord(P.ev[6], stream), "hipEventRecord");
            fetch(0);
            fetch(1);
            if (nruns)
                check(hipMemcpyAsync(P.runs.h, P.runs.d, nruns * sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
                      "align_pairs runs copy");
            check(hipStreamSynchronize(stream), "align_pairs synchronize");
            S.dir_ms += elapsed(4);
            S.walk_ms += elapsed(5);
            S.launches += 2;

            // ---- text
            const double tt0 = now_ms();
            const uint32_t* h_runs = (const uint32_t*)P.runs.h;
            std::atomic<uint64_t> zeros{0};
            parallel_ranges(p1 - p0, 64, [&](size_t b, size_t e) {
                uint64_t z = 0;
                for (size_t l = b; l < e; l++) {
                    const AlignLane& L = lanes[l];
                    const uint32_t i = dev_idx[p0 + l];
                    if (!L.used && best[l] < 0) continue;      // on the host list
                    ssa_amd_pair_alignment_t& o = out[i];
                    o.cigar_off = coff[i];
                    o.flags = 0;
                    char* text = cigars + coff[i];
                    if (!L.used) {
                        // a zero pair: ssa_amd_align_pair's (0, 0, 0, 0) and an empty CIGAR
                        o.score = 0;
                        for (auto& r : o.region) r = 0;
                        o.cigar_len = 0;
                        text[0] = 0;
                        z++;
                        continue;
                    }
                    o.score = nw ? h_out[l].x : best[l];
                    o.region[0] = L.a_begin;
                    o.region[1] = L.a_end;
                    o.region[2] = L.b_begin;
                    o.region[3] = L.b_end;
                    const uint32_t nr = std::min((uint32_t)h_out[nl + l].x, L.cap);
                    o.cigar_len = format_runs(h_runs + L.slot, nr, text);
                }
                zeros.fetch_add(z);
            });
            S.zero_pairs += zeros.load();
            S.text_ms += now_ms() - tt0;
            S.chunks++;
            g0 = g1;
        }
        if (!todo.empty()) {
            S.device_fallbacks = todo.size();
            run_host(todo);
        }
    }
    S.kernel_ms = S.fwd_ms + S.rev_ms + S.dir_ms + S.walk_ms;
    S.total_ms = now_ms() - t0;
    g_stats = S;
    return 0;
}

}  // namespace ssa
