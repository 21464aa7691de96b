// align_wave.h -- the wave aligner's device interface (align_wave.hip; host
// side: align_wave.cpp).  One wave aligns one pair: lane l
// holds RL consecutive query rows of the current pass (64 * RL rows), the
// pair's columns sweep through the lanes (at step t lane l is at column
// t - l).  Nothing is lane-interleaved on the host: the codes travel as the
// caller has them, one descriptor per pair says where.
//   codes  the chunk's sequences, byte per residue (code < 32)
//   rec    [pair]                     what the passes find (WaveRec); pass 1 -> 2 -> 3 -> 4 -> host
//   scr    [pair][2][dlen]            int64 (H, F) of a pass's bottom row, per column (pass p -> p + 1)
//   fin    [pair][query row]          int2 (H, E) after the pair's last column (wave_fwd -> wave_rev)
//   dir    [pair][pass][step][lane]   RL x 2 bits per lane and step (wave_dir -> wave_walk): row r of
//                                     the lane at bits 2r (bit 0 LEFT, bit 1 UP); a step's 64 elements
//                                     are one coalesced row of 64 / 128 / 256 bytes (RL <= 4 / <= 8 / <= 16);
//                                     a pass has (columns + 63) steps, cell (i, j) is at step j + lane(i)
//   runs   [pair's slot .. + qlen + dlen)   uint32 count << 2 | op, in traceback order (wave_walk)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ssa {

constexpr uint32_t kWaveNoPos = 0xffff0000u;   // positions travel as col << 16 | row; >= this: no cell
constexpr uint32_t kWaveMaxLen = 65535;        // both lengths below this
constexpr int kWaveRL[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16};   // rows per lane: the instantiated RLs

// bytes of one lane's direction bits of one step
constexpr uint32_t wave_dir_elem(uint32_t rl) { return rl <= 4 ? 1u : rl <= 8 ? 2u : 4u; }
// direction bytes of a pair swept over rows x cols
constexpr uint64_t wave_dir_bytes(uint32_t rl, uint64_t rows, uint64_t cols) {
    return (rows + 64 * rl - 1) / (64 * rl) * (cols + 63) * 64 * wave_dir_elem(rl);
}

struct WavePair {
    uint32_t q_off, d_off;      // first byte of each side in codes
    uint32_t qlen, dlen;        // both >= 1
    uint64_t dir_off;           // first byte of the pair's direction bits in dir
    uint32_t scr_off;           // first int64 of the pair's two scratch rows in scr
    uint32_t fin_off;           // first int2 of the pair's rows in fin
    uint32_t runs_off;          // first word of the pair's slot in runs
    uint32_t reserved;
};

enum : uint32_t { kWaveOk = 0, kWaveZero = 1, kWaveNoCell = 2 };

struct WaveRec {
    int32_t score;              // SW: the maximum (wave_fwd); NW: H of the last cell (wave_dir)
    uint32_t a_begin, a_end;    // the region: query rows
    uint32_t b_begin, b_end;    //             target columns
    uint32_t nruns;             // wave_walk
    uint32_t state;             // kWaveOk; kWaveZero: an SW pair of score 0; kWaveNoCell: a pass found no cell
    uint32_t reserved;
};

struct WaveArgs {
    const uint8_t* codes;
    const WavePair* pairs;
    const int8_t* mt;           // [32][32]: mt[q * 32 + d] = M[d][q]
    WaveRec* rec;
    int64_t* scr;
    int2* fin;
    uint8_t* dir;
    uint32_t* runs;
    int32_t gap_open, gap_extend;
    uint32_t npairs;
    uint32_t rl;                // rows per lane of this call's sweeps (and of the dir layout)
};

// pass: 0 wave_fwd (SW), 1 wave_rev (SW), 2 wave_dir (nw selects the boundaries), 3 wave_walk
hipError_t launch_align_wave(int pass, bool nw, const WaveArgs& a, hipStream_t st);

}  // namespace ssa
