// pairs.cpp -- ssa_amd_score_pairs: exact scores of a batch of independent
// (query, target) pairs in one call.  Pairs are ordered by
// shape, packed lane-interleaved in groups of 64 (pairs.h) and scored one
// group per wave by pairs_kernel (pairs.hip); what int32 on the device cannot
// score exactly goes through the int64 recurrences below, in parallel on the
// host.  The call owns its stream and buffers: an open DB, its device copy,
// the plan cache and ssa_amd_get_stats are not touched.
// ssa_amd_score_pairs_indexed is the same routine over index
// pairs into two sequence sets; by default its device pairs are packed on the
// device by pairs_gather_kernel (pairs_gather.hip) from the uploaded sets.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "engine.h"
#include "pairs.h"
#include "pairs_align.h"   // parallel_ranges, interleave: shared with the batch aligner
#include "pairs_gather.h"  // the indexed call's device-side packer

namespace ssa {

// ------------------------------------------------------- exact host scoring
// The reference's 64-bit recurrences (smith_waterman_64.c / needleman_wunsch_64.c),
// columns = DB sequence, rows = query, M[d][q]; he = 2 * qn scratch words.
int64_t host_sw(const uint8_t* d, size_t dn, const uint8_t* q, size_t qn, const int64_t* M, int64_t Q, int64_t R,
                int64_t* he) {
    int64_t best = 0;
    std::fill(he, he + 2 * qn, 0);
    for (size_t j = 0; j < dn; j++) {
        const int64_t* row = M + ((size_t)d[j] << 5);
        int64_t h = 0, f = 0;
        for (size_t i = 0; i < qn; i++) {
            const int64_t left = he[2 * i];
            int64_t e = he[2 * i + 1];
            h = std::max<int64_t>(std::max(h + row[q[i]], std::max(e, f)), 0);
            best = std::max(best, h);
            he[2 * i] = h;
            const int64_t open = h + Q + R;
            he[2 * i + 1] = std::max(e + R, open);
            f = std::max(f + R, open);
            h = left;
        }
    }
    return best;
}

int64_t host_nw(const uint8_t* d, size_t dn, const uint8_t* q, size_t qn, const int64_t* M, int64_t Q, int64_t R,
                int64_t* he) {
    // an empty side: the recurrence's own boundary, one gap over the other side
    if (qn == 0 || dn == 0) return qn + dn == 0 ? 0 : Q + (int64_t)(qn + dn) * R;
    for (size_t i = 0; i < qn; i++) {
        he[2 * i] = Q + (int64_t)(i + 1) * R;
        he[2 * i + 1] = 2 * Q + (int64_t)(i + 2) * R;
    }
    for (size_t j = 0; j < dn; j++) {
        const int64_t* row = M + ((size_t)d[j] << 5);
        int64_t f = 2 * Q + (int64_t)(j + 2) * R;
        int64_t h = j == 0 ? 0 : Q + (int64_t)j * R;
        for (size_t i = 0; i < qn; i++) {
            const int64_t left = he[2 * i];
            int64_t e = he[2 * i + 1];
            h = std::max(h + row[q[i]], std::max(e, f));
            he[2 * i] = h;
            const int64_t open = h + Q + R;
            he[2 * i + 1] = std::max(e + R, open);
            f = std::max(f + R, open);
            h = left;
        }
    }
    return he[2 * qn - 2];
}

namespace {

ssa_amd_pairs_stats_t g_stats;

// ------------------------------------------------------------ device state
// Buffers are kept between calls and only ever grow.
struct PairsDevice {
    int device = -1;
    bool probed = false, usable = false;
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {};       // kernel begin, kernel end; [2]: gather begin (the indexed call)
    uint8_t* h_up = nullptr;     // pinned upload block: matrix, groups, then lens, qres, tres or (the
                                 // indexed call's gather path) one descriptor per lane
    uint8_t* d_up = nullptr;
    size_t up_cap = 0;
    int2* d_bnd = nullptr;
    size_t bnd_cap = 0;          // bytes
    int32_t* d_out = nullptr;
    int32_t* h_out = nullptr;    // pinned
    size_t out_cap = 0;          // groups
    // the indexed call's gather path: both pools, and what the gather kernel fills (lens, qres, tres)
    uint8_t* d_pool = nullptr;
    size_t pool_cap = 0;
    uint8_t* d_res = nullptr;
    size_t res_cap = 0;

    void release() {
        if (h_up) (void)hipHostFree(h_up);
        if (d_up) (void)hipFree(d_up);
        if (d_bnd) (void)hipFree(d_bnd);
        if (d_out) (void)hipFree(d_out);
        if (h_out) (void)hipHostFree(h_out);
        if (d_pool) (void)hipFree(d_pool);
        if (d_res) (void)hipFree(d_res);
        d_pool = d_res = nullptr;
        pool_cap = res_cap = 0;
        h_up = d_up = nullptr;
        d_bnd = nullptr;
        d_out = h_out = nullptr;
        up_cap = bnd_cap = out_cap = 0;
    }
};
PairsDevice g_dev;

// The device of this call (ssa_amd_set_device, else the current HIP device),
// made current; false when no HIP device is visible (the host path runs).
bool use_device() {
    PairsDevice& P = g_dev;
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
    const int dev = cfg().device >= 0 ? cfg().device : cur;
    if (dev != cur) check(hipSetDevice(dev), "hipSetDevice");
    if (P.probed && P.device == dev) return P.usable;
    if (P.probed && P.usable) {
        // another device than the last call's: its buffers go, on their own device
        check(hipSetDevice(P.device), "hipSetDevice");
        P.release();
        (void)hipStreamDestroy(P.stream);
        for (auto& e : P.ev) (void)hipEventDestroy(e);
        P.stream = nullptr;
        check(hipSetDevice(dev), "hipSetDevice");
    }
    P.probed = true;
    P.device = dev;
    P.usable = false;
    // the code object holds gfx950 kernels only (as the search path, engine.cpp upload_pack)
    hipDeviceProp_t prop;
    check(hipGetDeviceProperties(&prop, dev), "hipGetDeviceProperties");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        fatal("libssa_amd is built for gfx950 (MI355X) only; device %d is %s", dev, prop.gcnArchName);
    check(hipStreamCreateWithFlags(&P.stream, hipStreamNonBlocking), "hipStreamCreate");
    for (auto& e : P.ev) check(hipEventCreate(&e), "hipEventCreate");
    P.usable = true;
    return true;
}

constexpr size_t kAlign = 256;
size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

// bytes a group of ncb column blocks and nstrips strips takes on the device
size_t group_bytes(uint32_t ncb, uint32_t nstrips) {
    return (size_t)ncb * 256 + (size_t)nstrips * 2 * 256 + (size_t)ncb * 4 * 512 + 64 * 8 + 64 * 4 + sizeof(PairsGroup);
}

// automatic chunk size: device bytes of one chunk (residues, boundary buffer, results)
constexpr size_t kChunkBudget = (size_t)256 << 20;

}  // namespace

bool pairs_use_device(int* device, hipStream_t* stream) {
    if (!use_device()) return false;
    *device = g_dev.device;
    *stream = g_dev.stream;
    return true;
}

const ssa_amd_pairs_stats_t& pairs_stats() {
    g_stats.strip_rows = kPairsRows;
    return g_stats;
}

void set_pairs_stats(const ssa_amd_pairs_stats_t& s) { g_stats = s; }

namespace {

// ------------------------------------------------------------ pair sources
// Where pair p's two sequences lie.  Everything behind the argument checks --
// the device conditions, the ordering, the grouping, the host path, the chunk
// loop -- sees the batch through one of these (score_source below).
// q_start / d_start: the sequence's byte in its pool, for the gather path.

// ssa_amd_score_pairs: pair p is the p-th interval of both offset arrays
struct OffsetPairs {
    const uint8_t *qc, *dc;
    const uint64_t *qoff, *doff;
    const uint8_t* q(size_t p) const { return qc + qoff[p]; }
    const uint8_t* d(size_t p) const { return dc + doff[p]; }
    uint64_t qlen(size_t p) const { return qoff[p + 1] - qoff[p]; }
    uint64_t dlen(size_t p) const { return doff[p + 1] - doff[p]; }
    uint64_t q_start(size_t p) const { return qoff[p] - qoff[0]; }
    uint64_t d_start(size_t p) const { return doff[p] - doff[0]; }
};

// ssa_amd_score_pairs_indexed: pair p is sequence qidx[p] of the q set against didx[p] of the d set
struct IndexedPairs {
    const uint8_t *qc, *dc;
    const uint64_t *qoff, *doff;
    const uint32_t *qidx, *didx;
    const uint8_t* q(size_t p) const { return qc + qoff[qidx[p]]; }
    const uint8_t* d(size_t p) const { return dc + doff[didx[p]]; }
    uint64_t qlen(size_t p) const { return qoff[qidx[p] + 1] - qoff[qidx[p]]; }
    uint64_t dlen(size_t p) const { return doff[didx[p] + 1] - doff[didx[p]]; }
    uint64_t q_start(size_t p) const { return qoff[qidx[p]] - qoff[0]; }
    uint64_t d_start(size_t p) const { return doff[didx[p]] - doff[0]; }
};

// The gather path's pools (host side): q_start / d_start count from q and d.
struct GatherPools {
    const uint8_t *q, *d;
    size_t qbytes, dbytes;
    bool shared;          // one pool for both sides: uploaded once
};

// every residue of [p, p + len) is a code < 32 (the matrix is 32 x 32)
bool codes_valid(const uint8_t* p, size_t len) {
    std::atomic<uint32_t> seen{0};
    parallel_ranges(len, 1 << 20, [&](size_t b, size_t e) {
        uint8_t acc = 0;
        for (size_t i = b; i < e; i++) acc |= p[i];
        seen.fetch_or(acc);
    });
    return seen.load() < (uint32_t)kDim;
}

void reset_stats() {
    ssa_amd_pairs_stats_t& S = g_stats;
    S = ssa_amd_pairs_stats_t{};
    S.strip_rows = kPairsRows;
    S.device = -1;
}

// Scores the n checked pairs of `src`.  pools: the indexed call's sequence
// pools when its device pairs are to be packed by pairs_gather_kernel, NULL
// for host packing (always so for ssa_amd_score_pairs).
template <class Src>
int score_source(const bool nw, const Src& src, const size_t n, int64_t* scores, const GatherPools* pools,
                 const double t0) {
    const Config& C = cfg();
    const int64_t* M = matrix().m;
    const int64_t Q = C.gap_open, Ge = C.gap_extend;

    // what the int32 kernel scores exactly: an int8 matrix, gap penalties <= 0
    // (its value masking of padding cells relies on it), and per pair a score
    // bound well inside int32
    int64_t max_abs = 0;
    bool int8_matrix = true;
    for (int i = 0; i < kDim * kDim; i++) {
        if (M[i] < -128 || M[i] > 127) int8_matrix = false;
        max_abs = std::max<int64_t>(max_abs, std::llabs(M[i]));
    }
    bool device = !C.pairs_host && int8_matrix && Q <= 0 && Ge <= 0;
    if (device) device = use_device();
    // |H|, |E|, |F| <= (qlen + dlen) * (max |M| + |gap_extend|) + 2 * |gap_open|; a group's padded sweep is
    // at most twice its longest pair's, so half of int32's range per pair leaves it exact
    const int64_t per_residue = max_abs + std::llabs(Ge);
    const int64_t residue_limit = per_residue ? (((int64_t)1 << 29) - 2 * std::llabs(Q)) / per_residue : INT64_MAX;

    ssa_amd_pairs_stats_t S{};
    S.pairs = n;
    S.strip_rows = kPairsRows;
    S.device = device ? g_dev.device : -1;
    snprintf(S.kernel, sizeof S.kernel, "%s", nw ? "pairs_nw_i32" : "pairs_sw_i32");

    std::vector<uint32_t> dev_idx;   // the pairs the device scores, by input index
    {
        uint64_t cells = 0;
        for (size_t i = 0; i < n; i++) {
            const uint64_t ql = src.qlen(i), dl = src.dlen(i);
            cells += ql * dl;
            if (device && ql && dl && (int64_t)(ql + dl) <= residue_limit && ql + dl < ((uint64_t)1 << 31) &&
                n <= UINT32_MAX)
                dev_idx.push_back((uint32_t)i);
        }
        S.cells = cells;
    }
    // ---- the host path: everything else
    const double th0 = now_ms();
    if (dev_idx.size() < n) {
        std::vector<uint8_t> on_dev(n, 0);
        for (uint32_t i : dev_idx) on_dev[i] = 1;
        std::vector<size_t> todo;
        for (size_t i = 0; i < n; i++)
            if (!on_dev[i]) todo.push_back(i);
        S.host_pairs = todo.size();
        parallel_ranges(todo.size(), 8, [&](size_t b, size_t e) {
            std::vector<int64_t> he;
            for (size_t k = b; k < e; k++) {
                const size_t i = todo[k];
                const size_t ql = src.qlen(i), dl = src.dlen(i);
                if (he.size() < 2 * ql) he.resize(2 * ql);
                scores[i] = nw ? host_nw(src.d(i), dl, src.q(i), ql, M, Q, Ge, he.data())
                               : host_sw(src.d(i), dl, src.q(i), ql, M, Q, Ge, he.data());
            }
        });
    }
    S.host_ms = now_ms() - th0;

    // ---- the device path
    if (!dev_idx.empty()) {
        PairsDevice& P = g_dev;
        auto qlen = [&](uint32_t i) { return (uint32_t)src.qlen(i); };
        auto dlen = [&](uint32_t i) { return (uint32_t)src.dlen(i); };
        auto strips = [&](uint32_t i) { return (qlen(i) + kPairsRows - 1) / kPairsRows; };
        // a wave sweeps (most strips) x (most columns) of its 64 pairs: order by both, longest first
        // (the last waves of a launch are then the short ones)
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
        const size_t ngroups = (dev_idx.size() + 63) / 64;
        std::vector<PairsGroup> groups(ngroups);
        for (size_t g = 0; g < ngroups; g++) {
            uint32_t md = 0, ms = 0;
            for (size_t p = g * 64; p < std::min(dev_idx.size(), g * 64 + 64); p++) {
                md = std::max(md, dlen(dev_idx[p]));
                ms = std::max(ms, strips(dev_idx[p]));
            }
            groups[g].ncb = (md + 3) / 4;
            groups[g].nstrips = ms;
            S.swept_cells += (uint64_t)ms * kPairsRows * groups[g].ncb * 4 * 64;
        }
        S.groups = (uint32_t)ngroups;
        S.pack_ms += now_ms() - tp0;

        // the compact matrix, transposed: mt[q][d] = M[d][q], padding row zero
        int8_t mt[kPairsCodes * 32] = {};
        for (int q = 0; q < kDim; q++)
            for (int d = 0; d < kDim; d++) mt[q * 32 + d] = (int8_t)M[(d << 5) + q];

        // ---- the gather path: both pools to the device, once per call, each with readable padding behind it
        const uint8_t *d_qpool = nullptr, *d_dpool = nullptr;
        if (pools) {
            const size_t q_room = align_up(pools->qbytes + kGatherPoolPad);
            const size_t d_room = pools->shared ? 0 : align_up(pools->dbytes + kGatherPoolPad);
            if (P.pool_cap < q_room + d_room) {
                if (P.d_pool) check(hipFree(P.d_pool), "hipFree");
                P.d_pool = nullptr;
                P.pool_cap = q_room + d_room + (q_room + d_room) / 4;
                check(hipMalloc((void**)&P.d_pool, P.pool_cap), "pairs pools");
            }
            d_qpool = P.d_pool;
            d_dpool = pools->shared ? P.d_pool : P.d_pool + q_room;
            if (pools->qbytes)
                check(hipMemcpyAsync(P.d_pool, pools->q, pools->qbytes, hipMemcpyHostToDevice, P.stream),
                      "pairs pool upload");
            if (!pools->shared && pools->dbytes)
                check(hipMemcpyAsync(P.d_pool + q_room, pools->d, pools->dbytes, hipMemcpyHostToDevice, P.stream),
                      "pairs pool upload");
            S.pool_bytes = pools->qbytes + (pools->shared ? 0 : pools->dbytes);
        }

        const size_t chunk_groups = C.pairs_chunk > 0 ? std::max<size_t>(1, (size_t)C.pairs_chunk / 64) : SIZE_MAX;
        for (size_t g0 = 0; g0 < ngroups;) {
            // ---- the chunk: groups [g0, g1) within the byte budget (at least one)
            const double tc0 = now_ms();
            size_t g1 = g0, bytes = 0;
            uint64_t trow = 0, qrow = 0, brow = 0;
            while (g1 < ngroups && g1 - g0 < chunk_groups) {
                const size_t gb = group_bytes(groups[g1].ncb, groups[g1].nstrips);
                if (g1 > g0 && C.pairs_chunk <= 0 && bytes + gb > kChunkBudget) break;
                // (row indices are 32-bit: a chunk past them ends here; one group alone cannot reach them)
                if (g1 > g0 && (brow + (uint64_t)groups[g1].ncb * 4 > UINT32_MAX)) break;
                groups[g1].t_row = (uint32_t)trow;
                groups[g1].q_row = (uint32_t)qrow;
                groups[g1].b_row = (uint32_t)brow;
                trow += groups[g1].ncb;
                qrow += (uint64_t)groups[g1].nstrips * 2;
                brow += (uint64_t)groups[g1].ncb * 4;
                bytes += gb;
                g1++;
            }
            const size_t ng = g1 - g0;
            const size_t o_mt = 0;
            const size_t o_groups = align_up(sizeof mt);
            // host packing: lens, qres and tres follow in the upload block; gather path: the upload
            // block ends with one descriptor per lane, and the three lie in d_res, device memory only
            const size_t o_lens = o_groups + align_up(ng * sizeof(PairsGroup));
            const size_t o_desc = o_lens;
            const size_t lens_bytes = align_up(ng * 64 * sizeof(uint2));
            const size_t o_q = pools ? lens_bytes : o_lens + lens_bytes;
            const size_t o_t = o_q + (size_t)qrow * 256;
            const size_t res_end = o_t + (size_t)trow * 256;
            const size_t up_bytes = pools ? o_desc + ng * 64 * sizeof(PairsDesc) : res_end;
            const size_t bnd_bytes = (size_t)brow * 512;
            if (pools && P.res_cap < res_end) {
                if (P.d_res) check(hipFree(P.d_res), "hipFree");
                P.d_res = nullptr;
                P.res_cap = res_end + res_end / 4;
                check(hipMalloc((void**)&P.d_res, P.res_cap), "pairs residues");
            }
            if (P.up_cap < up_bytes) {
                if (P.h_up) check(hipHostFree(P.h_up), "hipHostFree");
                if (P.d_up) check(hipFree(P.d_up), "hipFree");
                P.h_up = P.d_up = nullptr;
                P.up_cap = up_bytes + up_bytes / 4;
                check(hipHostMalloc((void**)&P.h_up, P.up_cap, hipHostMallocDefault), "pairs staging");
                check(hipMalloc((void**)&P.d_up, P.up_cap), "pairs residues");
            }
            if (P.bnd_cap < bnd_bytes) {
                if (P.d_bnd) check(hipFree(P.d_bnd), "hipFree");
                P.d_bnd = nullptr;
                P.bnd_cap = bnd_bytes + bnd_bytes / 4;
                check(hipMalloc((void**)&P.d_bnd, P.bnd_cap), "pairs boundary buffer");
            }
            if (P.out_cap < ng) {
                if (P.d_out) check(hipFree(P.d_out), "hipFree");
                if (P.h_out) check(hipHostFree(P.h_out), "hipHostFree");
                P.d_out = P.h_out = nullptr;
                P.out_cap = ng + ng / 4;
                check(hipMalloc((void**)&P.d_out, P.out_cap * 64 * sizeof(int32_t)), "pairs scores");
                check(hipHostMalloc((void**)&P.h_out, P.out_cap * 64 * sizeof(int32_t), hipHostMallocDefault),
                      "pairs scores");
            }
            // ---- pack, lane-interleaved
            memcpy(P.h_up + o_mt, mt, sizeof mt);
            memcpy(P.h_up + o_groups, &groups[g0], ng * sizeof(PairsGroup));
            auto pack_groups = [&](size_t b, size_t e) {
                uint2* h_lens = (uint2*)(P.h_up + o_lens);
                uint8_t* h_q = P.h_up + o_q;
                uint8_t* h_t = P.h_up + o_t;
                for (size_t g = g0 + b; g < g0 + e; g++) {
                    const PairsGroup& G = groups[g];
                    uint8_t* tq = h_q + (size_t)G.q_row * 256;
                    uint8_t* tt = h_t + (size_t)G.t_row * 256;
                    memset(tq, (int)kPairsPad, (size_t)G.nstrips * 2 * 256);
                    memset(tt, (int)kPairsPad, (size_t)G.ncb * 256);
                    for (size_t l = 0; l < 64; l++) {
                        const size_t p = g * 64 + l;
                        uint2& L = h_lens[(g - g0) * 64 + l];
                        if (p >= dev_idx.size()) {
                            L = make_uint2(0, 0);
                            continue;
                        }
                        const uint32_t i = dev_idx[p];
                        const uint32_t ql = qlen(i), dl = dlen(i);
                        L = make_uint2(ql, dl);
                        const uint8_t* qs = src.q(i);
                        const uint8_t* ds = src.d(i);
                        interleave(tq + l * 4, qs, ql);
                        interleave(tt + l * 4, ds, dl);
                    }
                }
            };
            if (pools) {
                // (the gather path: a descriptor per lane; an unused lane's is all zero)
                PairsDesc* h_desc = (PairsDesc*)(P.h_up + o_desc);
                parallel_ranges(ng * 64, 1 << 14, [&](size_t b, size_t e) {
                    for (size_t l = b; l < e; l++) {
                        const size_t p = g0 * 64 + l;
                        if (p >= dev_idx.size()) {
                            h_desc[l] = PairsDesc{0, 0, 0, 0};
                            continue;
                        }
                        const uint32_t i = dev_idx[p];
                        h_desc[l] = PairsDesc{src.q_start(i), src.d_start(i), qlen(i), dlen(i)};
                    }
                });
            } else {
                parallel_ranges(ng, 1, pack_groups);
            }
            S.pack_ms += now_ms() - tc0;
            // ---- upload, score, copy back
            check(hipMemcpyAsync(P.d_up, P.h_up, up_bytes, hipMemcpyHostToDevice, P.stream), "pairs upload");
            PairsArgs A;
            A.mt = (const int8_t*)(P.d_up + o_mt);
            A.groups = (const PairsGroup*)(P.d_up + o_groups);
            A.lens = (const uint2*)(pools ? P.d_res : P.d_up + o_lens);
            A.qres = (const uint32_t*)((pools ? P.d_res : P.d_up) + o_q);
            A.tres = (const uint32_t*)((pools ? P.d_res : P.d_up) + o_t);
            A.bnd = P.d_bnd;
            A.out = P.d_out;
            A.gap_open = (int32_t)Q;
            A.gap_extend = (int32_t)Ge;
            A.ngroups = (uint32_t)ng;
            if (pools) {
                // lens, qres and tres of the chunk, written on the device; the launch order is the dependency
                GatherArgs T;
                T.desc = (const PairsDesc*)(P.d_up + o_desc);
                T.groups = A.groups;
                T.qpool = d_qpool;
                T.dpool = d_dpool;
                T.qres = (uint32_t*)(P.d_res + o_q);
                T.tres = (uint32_t*)(P.d_res + o_t);
                T.lens = (uint2*)P.d_res;
                T.ngroups = (uint32_t)ng;
                check(hipEventRecord(P.ev[2], P.stream), "hipEventRecord");
                check(launch_pairs_gather(T, P.stream), "pairs_gather_kernel");
                S.launches++;
            }
            check(hipEventRecord(P.ev[0], P.stream), "hipEventRecord");
            check(launch_pairs(nw ? 1 : 0, A, P.stream), "pairs_kernel");
            check(hipEventRecord(P.ev[1], P.stream), "hipEventRecord");
            check(hipMemcpyAsync(P.h_out, P.d_out, ng * 64 * sizeof(int32_t), hipMemcpyDeviceToHost, P.stream),
                  "pairs scores copy");
            check(hipStreamSynchronize(P.stream), "pairs synchronize");
            float ms = 0;
            check(hipEventElapsedTime(&ms, P.ev[0], P.ev[1]), "hipEventElapsedTime");
            S.kernel_ms += ms;
            if (pools) {
                check(hipEventElapsedTime(&ms, P.ev[2], P.ev[0]), "hipEventElapsedTime");
                S.gather_ms += ms;
            }
            for (size_t p = g0 * 64; p < std::min(dev_idx.size(), g1 * 64); p++)
                scores[dev_idx[p]] = P.h_out[p - g0 * 64];
            S.chunks++;
            S.launches++;
            g0 = g1;
        }
    }
    S.total_ms = now_ms() - t0;
    g_stats = S;
    return 0;
}

}  // namespace

int score_pairs(int algo, const uint8_t* qc, const uint64_t* qoff, const uint8_t* dc, const uint64_t* doff, size_t n,
                int64_t* scores) {
    const double t0 = now_ms();
    if (algo != SSA_AMD_SW && algo != SSA_AMD_NW) return 1;
    if (n == 0) {
        reset_stats();
        return 0;
    }
    if (!qc || !qoff || !dc || !doff || !scores) return 1;
    if (!matrix().ready) fatal("Scoring matrix not initialized");
    for (size_t i = 0; i < n; i++)
        if (qoff[i + 1] < qoff[i] || doff[i + 1] < doff[i]) return 1;
    if (!codes_valid(qc + qoff[0], qoff[n] - qoff[0]) || !codes_valid(dc + doff[0], doff[n] - doff[0])) return 1;
    return score_source(algo == SSA_AMD_NW, OffsetPairs{qc, dc, qoff, doff}, n, scores, nullptr, t0);
}

int score_pairs_indexed(int algo, const uint8_t* qc, const uint64_t* qoff, size_t nq, const uint8_t* dc,
                        const uint64_t* doff, size_t nd, const uint32_t* qidx, const uint32_t* didx, size_t n,
                        int64_t* scores) {
    const double t0 = now_ms();
    if (algo != SSA_AMD_SW && algo != SSA_AMD_NW) return 1;
    if (n == 0) {
        reset_stats();
        return 0;
    }
    if (!qc || !qoff || !dc || !doff || !qidx || !didx || !scores) return 1;
    if (!matrix().ready) fatal("Scoring matrix not initialized");
    // both sets whole, referenced by a pair or not: the gather path uploads them as they are
    for (size_t a = 0; a < nq; a++)
        if (qoff[a + 1] < qoff[a]) return 1;
    for (size_t b = 0; b < nd; b++)
        if (doff[b + 1] < doff[b]) return 1;
    const bool shared = qc == dc && qoff == doff && nq == nd;
    const size_t qbytes = qoff[nq] - qoff[0], dbytes = doff[nd] - doff[0];
    if (!codes_valid(qc + qoff[0], qbytes) || (!shared && !codes_valid(dc + doff[0], dbytes))) return 1;
    {
        std::atomic<bool> outside{false};
        parallel_ranges(n, 1 << 18, [&](size_t b, size_t e) {
            bool bad = false;
            for (size_t p = b; p < e; p++) bad |= qidx[p] >= nq || didx[p] >= nd;
            if (bad) outside.store(true);
        });
        if (outside.load()) return 1;
    }
    const Config& C = cfg();
    const IndexedPairs src{qc, dc, qoff, doff, qidx, didx};
    const GatherPools pools{qc + qoff[0], dc + doff[0], qbytes, dbytes, shared};
    const uint64_t uploaded = (uint64_t)qbytes + (shared ? 0 : dbytes);
    const bool gather = C.pairs_gather && uploaded <= (uint64_t)std::max(0, C.pairs_pool_mb) << 20;
    return score_source(algo == SSA_AMD_NW, src, n, scores, gather ? &pools : nullptr, t0);
}

}  // namespace ssa
