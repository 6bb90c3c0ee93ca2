// nw_batch.h -- shared between the batch kernels (nw_batch.hip) and their host
// layer (nw_batch.cpp).  Not part of the public ABI (include/nw_hip.h is).
#pragma once
#include <stdint.h>

#include "nw_ckpt.h"  // (the sweep's strip geometry: kCkptC, kCkptCols, kCkptWavesPerCU)
#include "nw_internal.h"

namespace nw {

// The batch's row characters: one copy of the concatenated s2 (raw, or mapped for the
// v_perm tables), kBatchRowPad bytes in front of it and kBatchRowTail behind.  A lane
// loads the 64 bytes of rows 64it - lane .. + 63 whether or not those rows exist (a
// row outside 1..n2 is never used: the EDGE test), so the loads of the first and the
// last pair reach at most 64 bytes before and 128 bytes past the characters.
constexpr int kBatchRowPad = 128;
constexpr int kBatchRowTail = 256;
constexpr int kBatchDirIter = kWave * kWave;  // direction bytes of one 64-step iteration of a strip (16 dwords per lane)

// 64-step iterations of one strip of a pair with n2 rows: the sweep's nblocks + 1
constexpr int64_t batch_iters(int64_t n2) { return n2 / kWave + 2; }
constexpr int64_t batch_strips(int64_t n1) { return (n1 + kCkptCols - 1) / kCkptCols; }
// int32 words of one worker's column scratch
constexpr int64_t batch_col_words(int64_t max_n2) { return (max_n2 + kWave - 1) / kWave * kWave + kWave; }

// Everything one launch of the batch kernel needs.  Plain POD, passed by value.
struct BatchArgs {
    const uint8_t *s1;      // the concatenated column characters
    const int64_t *off1;    // pair i: s1[off1[i] .. off1[i + 1])
    const uint8_t *rows;    // the row characters (above): row y of pair i at rows[kBatchRowPad + off2[i] + y - 1]
    const int64_t *off2;
    const int32_t *order;   // pair of ticket t (longest first); NULL: pair t
    int32_t npairs;         // tickets of this launch
    int32_t max_n2;         // the column scratch holds this many rows: a longer pair is refused (score INT32_MIN)
    uint32_t *ticket;       // zero at launch
    int32_t *colscr;        // [grid][cstride]: a worker's right column between two strips of its pair
    int64_t cstride;
    int32_t perm;           // v_perm score tables allowed (the rows are then mapped)
    const uint8_t *charmap;
    const uint32_t *nprof;
    int32_t match, mismatch, gap;
    int32_t *scores;        // [pair]
    uint8_t *dirs;          // directions kernel: ticket t's block at dirs + dir_off[t]
    const int64_t *dir_off;
};

// The walk: one thread per ticket, from (n2, n1) to (0, 0) over the direction bits.
struct BatchWalkArgs {
    const int64_t *off1, *off2;
    const int32_t *order;
    int32_t npairs;
    const uint8_t *dirs;
    const int64_t *dir_off;  // [ticket]
    uint8_t *ops;
    const int64_t *ops_off;  // [ticket]: the pair's slot of n1 + n2 bytes
    int64_t *n_ops;          // [ticket]
};

// The affine-gap kernels (nw_batch_affine.hip): the linear launch's arguments, with
// b.gap the cost of extending a gap, b.cstride twice batch_col_words (a worker keeps
// H' and E' of a right column: E' eoff words behind H') and, in the directions kernel,
// 4 bits per cell (twice kBatchDirIter per iteration of a strip).
struct BatchAffineArgs {
    BatchArgs b;
    int32_t gap_open;  // <= 0: what a run of ups or of lefts costs once, whatever its length
    int64_t eoff;
};

// The matrix kernels (nw_batch_matrix.hip): the affine launch's arguments (a.b.match,
// mismatch, perm, charmap and nprof unused; a.b.rows holds LETTERS, launch_batch_matrix_
// rows) and the substitution matrix itself -- no device buffer, no copy.
constexpr int kBatchMatrixLetters = 32;  // NW_SUBMAT_MAX
struct BatchMatrixArgs {
    BatchAffineArgs a;
    int32_t n;     // letters, 1 .. kBatchMatrixLetters
    int32_t wide;  // 0: score holds s - 2 * gap (every one fits int8); 1: s, and the cell adds -2 * gap
    // dword [x * 8 + g], byte b: the score byte of (s1 letter x, s2 letter 4g + b); 0 beyond n
    alignas(16) uint32_t score[kBatchMatrixLetters * kBatchMatrixLetters / 4];
    uint8_t index[256];  // byte -> letter < n
};

// The local kernels (nw_batch_local.hip): the matrix launch's arguments (m.wide 0 and
// m.score the matrix's own bytes: the cells are not in the w form; m.a.b.scores unused)
// and the hits, kBatchLocalHitWords int32 per pair in nw_local_hit's layout.
constexpr int kBatchLocalHitWords = 8;
struct BatchLocalArgs {
    BatchMatrixArgs m;
    int32_t *hits;  // [pair][8]: score, end_i, end_j, begin_i, begin_j, 0, 0, 0
};

// The local walk: from the hit's end cell to the first cell with H == 0, which it writes
// into the hit as the begin cell.
struct BatchLocalWalkArgs {
    BatchWalkArgs w;
    int32_t *hits;
};

// The semi-global kernels (nw_batch_semi.hip): the matrix launch's arguments as the
// matrix kernels take them (the w form: m.wide and m.score as there; m.a.b.scores unused),
// the hits in nw_local_hit's layout, and which end gaps are free (NW_ENDS_*, 0 .. 15).
struct BatchSemiArgs {
    BatchMatrixArgs m;
    int32_t *hits;  // [pair][8]: score, end_i, end_j, begin_i, begin_j, 0, 0, 0
    int32_t ends;
};

// The semi-global walk: from the hit's end cell to the begin cell, which it writes into
// the hit: (0, 0), or where the path meets a free boundary.
struct BatchSemiWalkArgs {
    BatchWalkArgs w;
    int32_t *hits;
    int32_t ends;
};

// The banded kernels (nw_batch_banded.hip): the matrix launch's arguments and the band
// width w >= 0 of the call (include/nw_hip.h: cell (i, j) is in the band iff dlo <= i - j
// <= dhi, dlo = min(0, n2 - n1) - w, dhi = max(0, n2 - n1) + w).
struct BatchBandedArgs {
    BatchMatrixArgs m;
    int32_t band;
};

// The banded walk: the affine walk over direction blocks that hold only the iterations of
// each strip's range.
struct BatchBandedWalkArgs {
    BatchWalkArgs w;
    int32_t band;
};

// The geometry of a banded pair, shared by the sweep, the walk and the host's sizes.
// dlo and dhi are kept within kBandedPad diagonals of the table's own (-n1 .. n2): the
// cells in the band are the same, and every sum below stays in int32 for the pairs the
// range bound admits.  A strip of 256 columns starting at column 256p + 1 has in-band
// cells at steps 256p + 1 + dlo .. 256p + 319 + dhi (rows 256p + 1 + dlo .. 256p + 256 +
// dhi, and lane l computes row r at step r + l); it runs the iterations
//     first(p) = max(0, floor((256p + dlo) / 64))   (one step earlier: the diagonal of the
//                                                     first in-band cell comes in as a feed)
//     .. min(iters - 1, floor((256p + 319 + dhi) / 64) + 1)   (the right column's last
//                                                     block is stored one iteration later)
// which are at most ceil((dhi - dlo + 319) / 64) + 2 -- the slots of a strip in the pair's
// direction block, never more than the unbanded batch_iters(n2).
constexpr int64_t kBandedPad = 1024;
constexpr int64_t batch_banded_dlo(int64_t n1, int64_t n2, int64_t band) {
    const int64_t d = (n2 < n1 ? n2 - n1 : 0) - band;
    return d < -n1 - kBandedPad ? -n1 - kBandedPad : d;
}
constexpr int64_t batch_banded_dhi(int64_t n1, int64_t n2, int64_t band) {
    const int64_t d = (n2 > n1 ? n2 - n1 : 0) + band;
    return d > n2 + kBandedPad ? n2 + kBandedPad : d;
}
constexpr int64_t batch_banded_slots(int64_t n1, int64_t n2, int64_t band) {
    const int64_t span = batch_banded_dhi(n1, n2, band) - batch_banded_dlo(n1, n2, band);
    const int64_t k = (span + 319 + 63) / 64 + 2;
    return k < batch_iters(n2) ? k : batch_iters(n2);
}
constexpr int64_t batch_banded_first(int64_t p, int64_t dlo) {
    const int64_t s = 256 * p + dlo;
    return s > 0 ? s >> 6 : 0;
}

// The two-piece kernels (nw_batch_dual.hip): the matrix launch's arguments as the matrix
// kernels take them (piece 1 = m.a.gap_open, m.a.b.gap; the w form is taken relative to it:
// m.wide and m.score as there) and piece 2.  m.a.b.cstride is three times batch_col_words (a
// worker keeps H', E1' and E2' of a right column: E1' m.a.eoff and E2' eoff2 words behind
// H'), and the directions kernel writes a byte per cell (four times kBatchDirIter per
// iteration of a strip).
struct BatchDualArgs {
    BatchMatrixArgs m;
    int32_t gap_open2;  // <= 0
    int32_t gap2;
    int64_t eoff2;
};

// The two-piece kernels inside a band (nw_batch_dual_banded.hip): the two-piece launch's
// arguments and the band width w >= 0 of the call, as BatchBandedArgs has it.  The directions
// kernel writes a byte per cell for the slots of each strip's range alone (four times
// kBatchDirIter per slot).
struct BatchDualBandedArgs {
    BatchDualArgs d;
    int32_t band;
};

// Its walk: the two-piece walk over direction blocks that hold only the iterations of each
// strip's range.
struct BatchDualBandedWalkArgs {
    BatchWalkArgs w;
    int32_t band;
};

// mapped (perm and at most kMaxPerm distinct column characters) or raw copy of s2cat
int launch_batch_rows(const uint8_t *d_s2, int64_t total2, int32_t perm, const uint8_t *meta, uint8_t *d_rows,
                      void *stream);
int launch_batch(const BatchArgs &a, bool dirs, int grid, void *stream);
// the walk (ops end -> begin, n_ops), then the reversal into begin -> end order
int launch_batch_walk(const BatchWalkArgs &w, void *stream);
// the reversal alone (nw_batch.hip nw_batch_reverse): what every walk below ends with
int launch_batch_reverse(const BatchWalkArgs &w, void *stream);
// the same two for affine gaps: the walk is a machine of three states over 4 bits per cell
int launch_batch_affine(const BatchAffineArgs &a, bool dirs, int grid, void *stream);
int launch_batch_affine_walk(const BatchWalkArgs &w, void *stream);
// substitution by matrix: d_rows[kBatchRowPad + i] = index[s2cat[i]] between zeroed pads;
// the sweep (its directions are the affine kernel's: launch_batch_affine_walk walks them)
int launch_batch_matrix_rows(const uint8_t *d_s2, int64_t total2, const uint8_t *index, uint8_t *d_rows,
                             void *stream);
int launch_batch_matrix(const BatchMatrixArgs &a, bool dirs, int grid, void *stream);
// local alignment (Smith-Waterman) with the matrix: the sweep writes a hit per pair, the
// walk starts at the hit's end cell (then the reversal, as above)
int launch_batch_local(const BatchLocalArgs &a, bool dirs, int grid, void *stream);
int launch_batch_local_walk(const BatchLocalWalkArgs &w, void *stream);
// semi-global alignment (free end gaps per side) with the matrix: the sweep writes a hit
// per pair, the walk starts at the hit's end cell and stops on a free boundary or at (0, 0)
int launch_batch_semi(const BatchSemiArgs &a, bool dirs, int grid, void *stream);
int launch_batch_semi_walk(const BatchSemiWalkArgs &w, void *stream);
// banded global alignment with the matrix: the sweep runs each strip's iteration range
// only, the walk indexes the direction blocks that range leaves
int launch_batch_banded(const BatchBandedArgs &a, bool dirs, int grid, void *stream);
int launch_batch_banded_walk(const BatchBandedWalkArgs &w, void *stream);
// global alignment with the matrix under a two-piece gap cost: the sweep carries five values
// per cell, the walk is a machine of five states over a byte per cell
int launch_batch_dual(const BatchDualArgs &a, bool dirs, int grid, void *stream);
int launch_batch_dual_walk(const BatchWalkArgs &w, void *stream);
// the same inside a band: the two-piece cell under the banded ranges, the five-state walk over
// the slots those ranges leave
int launch_batch_dual_banded(const BatchDualBandedArgs &a, bool dirs, int grid, void *stream);
int launch_batch_dual_banded_walk(const BatchDualBandedWalkArgs &w, void *stream);

}  // namespace nw
