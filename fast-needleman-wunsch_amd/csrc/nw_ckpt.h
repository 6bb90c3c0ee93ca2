// nw_ckpt.h -- shared between the checkpoint sweep kernel (nw_ckpt.hip) and its
// host layer (nw_ckpt.cpp).  Not part of the public ABI (include/nw_hip.h is).
#pragma once
#include <stdint.h>

#include "nw_internal.h"

namespace nw {

constexpr int kCkptC = 4;                        // columns per lane of a sweep wave
constexpr int kCkptCols = kWave * kCkptC;        // columns per strip
constexpr int kCkptWavesPerCU = 4;               // sweep waves per CU (one per SIMD; no LDS ring to fit)
constexpr uint32_t kCkptTag = 1u;                // tag of every checkpoint granule (nw_band.tag of a re-fill)

// Everything one launch of the checkpoint sweep needs.  Plain POD, passed by value.
struct CkptArgs {
    const void *rowpack;       // row packs of s2 (nw_fill.hip nw_rowpack, raw or mapped)
    const uint8_t *s1;         // n1 column characters
    int64_t n1, n2;
    int32_t nstrips;           // ceil(n1 / kCkptCols): the strips start at column 1
    int32_t nblocks;           // ceil((n2 + 1) / 64)
    uint64_t *gran;            // strip-to-strip hand-off granules [M][gstride] {tag:32 | w:32}
    int64_t gstride;           // 64 * nblocks
    int32_t M;                 // slots (workers + 1, or nstrips)
    uint32_t tagbase;          // strip p publishes tag tagbase + p + 1
    uint32_t *ctrl;            // the context's control words: [0] strip ticket, [1] error word
    int32_t perm;              // v_perm score tables allowed (the row packs are then mapped)
    const uint8_t *charmap;
    const uint32_t *nprof;
    int32_t match, mismatch, gap;
    uint64_t timeout_ticks;
    int64_t K;                 // checkpoint rows r * K, r = 1 .. nck (a multiple of 64)
    int32_t nck;
    uint64_t *ckpt;            // [nck][n1 + 1] granules {kCkptTag | t}: row r - 1 = table row r * K
    int32_t *score;            // t[n2][n1]
};

// rows r * K, r = 1 .. nck, of an (n2 + 1)-row table are checkpoints: nck = ceil(n2 / K) - 1
inline int64_t ckpt_rows(int64_t n2, int64_t K) { return n2 <= 0 ? 0 : (n2 + K - 1) / K - 1; }

int launch_ckpt_sweep(const CkptArgs &a, int grid, void *stream);

}  // namespace nw
