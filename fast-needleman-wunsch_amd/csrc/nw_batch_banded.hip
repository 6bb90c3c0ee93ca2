// nw_batch_banded.hip -- gfx950 (MI355X) batched global alignment with a substitution
// matrix and affine gaps inside a BAND of diagonals (include/nw_hip.h): with n1 columns,
// n2 rows and the call's width w, cell (i, j) is in the band iff dlo <= i - j <= dhi,
// dlo = min(0, n2 - n1) - w, dhi = max(0, n2 - n1) + w; H, E and F outside it are -inf.
// Everything else is nw_batch_matrix.hip's: one wave per pair, 256-column strips with lane
// l on columns 4l .. 4l+3 computing row s - l at step s, MatrixCell<WIDE> over ProfileSub,
// the two-column scratch between strips, 4 direction bits per cell.  The code of that is
// nw_batch_dev.h's sweep_tickets and sweep_iter; this file has its own pair loop
// (banded_pair) where the others call sweep_pair, and adds three things.
//
// 1. The range of a strip.  Lane l of strip p (columns 256p + 4l + 1 .. + 4) has in-band
//    rows cl + dlo .. cl + 3 + dhi, which it computes at steps 256p + 5l + 1 + dlo .. 256p
//    + 5l + 4 + dhi: over the lanes, steps s0 = 256p + 1 + dlo .. s1 = 256p + 319 + dhi.
//    The strip runs the 64-step iterations first(p) = max(0, floor((s0 - 1) / 64)) ..
//    min(nblocks, floor(s1 / 64) + 1) (nw_batch.h batch_banded_first) and nothing else.
//      Before: every cell at a step < s0 lies above the band (i - j < dlo) or in row 0.  When
//    first(p) > 0 the lanes enter with u = f = e = dg = -2^29, which is the state those
//    cells would have left: H and F above the band are -inf, E of a cell outside the band
//    is -inf by the definition, and the diagonal of a cell above the band is above it too.
//    The one step of slack (s0 - 1) is for lane 0's first in-band cell: its diagonal
//    (cl + dlo - 1, 256p) is in the band and arrives as a feed of the step before.  When
//    first(p) = 0 the lanes start on row 0 as in the matrix kernel, with H'[0][c] = -2^29
//    for c > -dlo.
//      After: block b of the right column (rows 64b .. 64b + 63) is complete after lane
//    63's steps of iteration b + 1 and stored there, so the range ends one iteration after
//    s1's; in the last strip the lane of column n1 has computed row n2 (an in-band cell)
//    by then and holds it (EDGE).
//
// 2. The mask.  A computed cell outside the band gets H' = -2^29 exactly, after the
//    matrix cell and before the EDGE hold (BandedCell::cell): per lane t = step - (256p +
//    5l + 1 + dlo) is the cell's diagonal minus dlo for column 0, t - k for column k, and
//    the cell is in the band iff (uint32)(t - k) <= dhi - dlo.  Forcing H alone suffices:
//      E' = max(E'_left, H'_left + go) moves right, i.e. towards smaller i - j.  It can enter
//    the band only from the dhi side (below the band).  There every H' is forced, and the
//    leftmost E' a lane sees is -2^29 (column 0, a masked feed, or the entering state), so
//    E' = max(-2^29, -2^29 + go) = -2^29 by induction along the row: go <= 0.
//      F' = max(F'_up, H'_up + go) moves down, towards larger i - j, and can enter only from
//    the dlo side (above the band), where the same induction runs down the column from
//    F'[0][j] = -2^29 or the entering state.
//      What the in-band cells leak outward -- a finite E' right of the band, a finite F'
//    below it -- moves away from the band and is never read by a cell in it: H' of the
//    cells it reaches is forced, and E' never feeds F' nor F' E'.
//    So every in-band cell sees -2^29 for each predecessor outside the band, and its own
//    diagonal predecessor, being on the same diagonal, is in the band and finite: H' of an
//    in-band inner cell is a real value, its direction bits never choose a predecessor
//    outside the band, and the walk stays inside.  The intermediates -2^29 + go and -2^29
//    + s - 2ge are not accumulated (their inputs are forced values) and stay far from
//    overflow; real values stay above -2^28 by the range bound, which the path "diagonal,
//    then one run" -- always inside the band -- keeps valid.
//      Iterations whose 64 steps lie wholly in the band (64it - 256p - 319 >= dlo and 64it
//    + 62 - 256p <= dhi: wave-uniform, decided like `edge`) run sweep_iter on the
//    MatrixCell base: the matrix kernel's iteration.
//    nw_batch_dual_banded.hip takes the arithmetic of points 1 to 3 from BandRange
//    (nw_batch_dev.h); banded_pair keeps its own text of it: on BandRange the sweeps came out
//    with the strip's set-up in another order and registers renamed after it (resources the
//    same), 15 of 16 fill entries were within the parent's spread and the score kernel's fill
//    of 8000 x 8000 under a covering band measured 16.92 -> 16.98 ms, 1.003 x against a
//    spread of 0.0025, all five runs above all of the parent's
//    (profiles/batch_dual_refactor_ab.json).
//
// 3. The feed is masked where it is read.  Lane x of the feed of block b holds row 64b +
//    x of column 256p (strip 0: of the boundary column, H'[r][0] = go, H'[0][0] = 0); it is
//    replaced by -2^29, H' and E', unless dlo <= 64b + x - 256p <= dhi.  Out-of-band rows --
//    also those the strip before never wrote in this pair, which hold an earlier pair's
//    values or nothing -- therefore read as -inf, and every in-band row of column 256p was
//    computed by lane 63 of strip p - 1 within its range and stored (point 1).  The
//    scratch is read only inside the worker's own allocation (blocks <= lastb).
//
// Directions: a pair's block is [strip][slot][step / 4][step % 4 / 2][lane] dwords, slot =
// iteration - first(strip), with batch_banded_slots(n1, n2, w) slots per strip -- the
// affine layout with the iterations outside the ranges left out.  nw_batch_banded_walk is
// nw_batch_affine_walk with that one subtraction in the index.
//
// Sizes: every int32 sum here is exact while 2 n1 + n2 + 4096 < 2^32, far beyond what the
// range bound admits for any matrix or gap cost that is not all zero.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nw_batch_dev.h"

namespace nw {
namespace {

template <bool WIDE>
struct BandedCell : MatrixCell<WIDE> {
    int32_t tb;     // 256p + 5 lane + 1 + dlo: step - tb - k = (the cell's diagonal) - dlo
    uint32_t span;  // dhi - dlo

    template <class M>
    __device__ __forceinline__ BandedCell(const M &mode, int32_t *out, int lane_) : MatrixCell<WIDE>(mode, out, lane_) {}

    template <int k, int SH, bool EDGE, bool DIRS>
    __device__ __forceinline__ void cell(int32_t d, int32_t &diag, int32_t &left, int32_t &el, bool act, int32_t step,
                                         uint32_t &bits) {
        GlobalCell::template cell<k, SH, EDGE, DIRS>(d, diag, left, el, act, step, bits);
        bool out = (uint32_t)(step - tb - k) > span;
        if constexpr (EDGE) out = out && act;  // (a lane outside rows 1..n2 holds its cells)
        this->u[k] = out ? kNegInf : this->u[k];
        left = this->u[k];
    }
};

// One pair (n1, n2 >= 1) by this wave; the arguments are sweep_pair's.
template <bool WIDE, bool DIRS, class M>
__device__ __forceinline__ void banded_pair(const M &mode, int32_t *out, const uint8_t *__restrict__ s1, int32_t n1,
                                            const uint8_t *__restrict__ rowb, int32_t n2, int32_t *__restrict__ col,
                                            uint32_t *__restrict__ dirs, int lane) {
    using P = BandedCell<WIDE>;
    using Base = MatrixCell<WIDE>;
    const int64_t eoff = mode.affine().eoff;
    const int nstrips = (n1 + kCkptCols - 1) / kCkptCols;
    const int nblocks = n2 / 64 + 1;  // ceil((n2 + 1) / 64)
    const int lastb = nblocks - 1;
    const int32_t dlo = (int32_t)batch_banded_dlo(n1, n2, mode.band);
    const int32_t dhi = (int32_t)batch_banded_dhi(n1, n2, mode.band);
    const int slots = (int)batch_banded_slots(n1, n2, mode.band);
    P S(mode, out, lane);
    S.span = (uint32_t)(dhi - dlo);

    for (int p = 0; p < nstrips; ++p) {
        const int32_t c0 = p * kCkptCols;          // the column the strip is fed from
        const int32_t cl = 1 + c0 + C * lane;      // first column of this lane
        const int it0 = (int)batch_banded_first(p, dlo);
        // (never beyond the strip's slots: the range is that short by its definition, and a
        // store past the pair's direction block must be impossible whatever the arithmetic)
        const int itl = min(min(nblocks, ((c0 + 319 + dhi) >> 6) + 1), it0 + slots - 1);
        S.strip_begin(s1, n1, cl);
        S.tb = c0 + 5 * lane + 1 + dlo;
        if (it0 > 0) {
            // every cell before the range is above the band
#pragma unroll
            for (int k = 0; k < C; ++k) S.u[k] = S.f[k] = kNegInf;
            S.e = S.dg = kNegInf;
        } else {
            // row 0: (0, c) is in the band iff -c >= dlo
#pragma unroll
            for (int k = 0; k < C; ++k) S.u[k] = (cl + k <= -dlo) ? S.u[k] : kNegInf;
        }
        S.acch = S.acce = 0;
        const bool fed = p > 0;            // (strip 0 never reads the scratch)
        const bool pub = p + 1 < nstrips;  // (the last strip's right column has no reader)

        // the feed of block b, masked: lane x holds row 64b + x of column c0
        auto feed = [&](int b, int32_t &h, int32_t &e) {
            const int32_t row = 64 * b + lane;
            h = S.boundary_h(row == 0);
            e = S.boundary_e();
            if (fed) {
                h = col[row];
                e = col[eoff + row];
            }
            const bool in = (uint32_t)(row - c0 - dlo) <= S.span;
            h = in ? h : kNegInf;
            e = in ? e : kNegInf;
        };

        // row words and the feed are loaded one iteration ahead
        u32x4 pkc[4], pkn[4];
        load_rows(rowb, it0, lane, pkc);
        int32_t fnh, fne;
        feed(it0, fnh, fne);  // (it0 <= lastb: 256p + dlo < n2)
        for (int it = it0; it <= itl; ++it) {
            if (it < nblocks) {
                S.fvh = fnh;
                S.fve = fne;
            }
            feed(min(it + 1, lastb), fnh, fne);
            load_rows(rowb, min(it + 1, nblocks), lane, pkn);
            const bool edge = it == 0 || 64 * it + 63 > n2;
            const bool inside = 64 * it - c0 - 319 >= dlo && 64 * it + 62 - c0 <= dhi;
            int32_t *colw = (pub && it > it0) ? col + 64 * (it - 1) : nullptr;
            uint32_t *dq = nullptr;
            if constexpr (DIRS) dq = dirs + ((int64_t)p * slots + (it - it0)) * (32 * kWave);
            if (inside) {
                if (edge)
                    sweep_iter<Base, true, DIRS>(it, pkc, n2, static_cast<Base &>(S), colw, eoff, dq, lane);
                else
                    sweep_iter<Base, false, DIRS>(it, pkc, n2, static_cast<Base &>(S), colw, eoff, dq, lane);
            } else {
                if (edge)
                    sweep_iter<P, true, DIRS>(it, pkc, n2, S, colw, eoff, dq, lane);
                else
                    sweep_iter<P, false, DIRS>(it, pkc, n2, S, colw, eoff, dq, lane);
            }
#pragma unroll
            for (int h = 0; h < 4; ++h) pkc[h] = pkn[h];
        }
        S.strip_end(p == nstrips - 1, cl, n1, n2);
    }
    S.pair_end();
}

struct BandedSweep : GlobalSweep {
    const BatchMatrixArgs &MA;
    uint32_t *pl;  // this lane's dword of profile row 0
    int32_t band;
    template <bool DIRS>
    __device__ __forceinline__ void pair(int32_t *out, const uint8_t *s1, int32_t n1, const uint8_t *rowb, int32_t n2,
                                         int32_t *col, uint32_t *dirs, int lane) const {
        if (MA.wide != 0)
            banded_pair<true, DIRS>(*this, out, s1, n1, rowb, n2, col, dirs, lane);
        else
            banded_pair<false, DIRS>(*this, out, s1, n1, rowb, n2, col, dirs, lane);
    }
};

template <bool DIRS>
__global__ __launch_bounds__(64) void nw_batch_banded_sweep(BatchBandedArgs BA) {
    __shared__ uint32_t prof[kLetters * kWave];  // [row letter][lane], 8 KiB
    sweep_tickets<DIRS>(BandedSweep{{BA.m.a}, BA.m, prof + threadIdx.x, BA.band});
}

// The walk of ticket t's pair from (n2, n1) to (0, 0): nw_batch_affine_walk (its header
// has the machine of three states) over the banded direction block.  Cell (i, j) was
// computed in strip p = (j-1) / 256 by lane l = ((j-1) % 256) / 4, column k = (j-1) % 4,
// at step s = i + l: nibble k % 2 of byte (s % 2) * 2 + k / 2 of dword [p][s / 64 -
// first(p)][s % 64 / 4][s % 4 / 2][l].  The walk reads in-band cells only (the header, point
// 2); the slot is clamped all the same, so that no read can leave the pair's block.
__global__ __launch_bounds__(64) void nw_batch_banded_walk(BatchBandedWalkArgs B) {
    const BatchWalkArgs &W = B.w;
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= W.npairs) return;
    const int pair = W.order != nullptr ? W.order[t] : t;
    int64_t c = W.off1[pair + 1] - W.off1[pair], r = W.off2[pair + 1] - W.off2[pair];
    const int64_t dlo = batch_banded_dlo(c, r, B.band);
    const int64_t slots = batch_banded_slots(c, r, B.band);
    const uint8_t *d = W.dirs + W.dir_off[t];
    uint8_t *ops = W.ops + W.ops_off[t];
    int64_t n = 0;
    uint32_t state = 0;  // 0 H, 1 F, 2 E
    while (r > 0 || c > 0) {
        if (r == 0 || c == 0) {  // (state is H here)
            const uint32_t op = r == 0 ? 2u : 1u;
            ops[n++] = (uint8_t)op;
            r -= op != 2u;
            c -= op != 1u;
            continue;
        }
        const int64_t cj = c - 1;
        const int64_t p = cj >> 8, l = (cj & 255) >> 2, k = cj & 3;
        const int64_t s = r + l;
        const int64_t slot = min(max((s >> 6) - batch_banded_first(p, dlo), (int64_t)0), slots - 1);
        const int64_t idx =
            ((((p * slots + slot) * 16 + ((s & 63) >> 2)) * 2 + ((s & 3) >> 1)) * 64 + l) * 4 + (s & 1) * 2 + (k >> 1);
        const uint32_t bits = ((uint32_t)d[idx] >> (4 * (k & 1))) & 15u;
        if (state == 0) {
            state = bits & 3u;
            if (state == 0) {
                ops[n++] = 0;
                --r;
                --c;
            }
        } else if (state == 1) {
            ops[n++] = 1;
            --r;
            state = (bits & 8u) ? 1u : 0u;
        } else {
            ops[n++] = 2;
            --c;
            state = (bits & 4u) ? 2u : 0u;
        }
    }
    W.n_ops[t] = n;
}

}  // namespace

int launch_batch_banded(const BatchBandedArgs &a, bool dirs, int grid, void *stream) {
    if (dirs)
        hipLaunchKernelGGL(nw_batch_banded_sweep<true>, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(nw_batch_banded_sweep<false>, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_batch_banded_walk(const BatchBandedWalkArgs &w, void *stream) {
    hipLaunchKernelGGL(nw_batch_banded_walk, dim3((unsigned)((w.w.npairs + 63) / 64)), dim3(64), 0,
                       (hipStream_t)stream, w);
    return launch_batch_reverse(w.w, stream);
}

}  // namespace nw
