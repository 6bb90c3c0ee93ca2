// nw_batch_dual_banded.hip -- gfx950 (MI355X) batched global alignment with a substitution
// matrix under the TWO-PIECE gap cost g(k) = max(go1 + k ge1, go2 + k ge2) inside a BAND of
// diagonals (include/nw_hip.h): with n1 columns, n2 rows and the call's width w, cell (i, j)
// counts iff dlo <= i - j <= dhi, dlo = min(0, n2 - n1) - w, dhi = max(0, n2 - n1) + w; H, E1,
// E2, F1 and F2 outside are -inf.  It is nw_batch_dual.hip's cell (five values in the w form
// taken relative to piece 1, three DPP moves, three scratch columns, one direction byte per
// cell; that file's header states the cell and the byte) under nw_batch_banded.hip's pair loop
// (the range of a strip, the entering state, the masked feed, the slots; that file's header,
// points 1 and 3, holds word for word with "H', E1' and E2'" for "H' and E'").  What is new
// here is the mask.
//
// The iteration is nw_batch_dual_dev.h's dual_iter, shared with nw_batch_dual.hip: this file once
// kept a second copy for fear that sharing would change that file's kernels, and compiling both
// ways showed it does not -- the unbanded sweeps call dual_iter with MASK = false and come out
// instruction for instruction as they did from their own text.  The wave-uniformly "inside"
// iterations (BandRange::inside, nw_batch_dev.h) run MASK = false here too, only the others pay
// the mask.
//
// The mask.  Per lane t = step - (256p + 5l + 1 + dlo) is the diagonal of the lane's column 0
// minus dlo, t - k for column k; the cell is in the band iff (uint32)(t - k) <= dhi - dlo.  A
// computed cell outside the band gets H' = E2' = F2' = -2^29 exactly, after the cell and
// before the EDGE hold.  E1' and F1' are left alone.  Why this is enough, and why forcing H'
// alone (which suffices for one piece) is not:
//   Piece 1.  E1' = max(E1'_left, H'_left + go1) extends for free, so a forced value is copied
//   and never accumulated.  It moves right, towards smaller i - j, and can enter the band only
//   from below it (the dhi side).  There every H' is forced and the leftmost E1' a lane sees
//   is -2^29 (column 0, a masked feed, or the entering state), so E1' = max(-2^29, -2^29 +
//   go1) = -2^29 by induction along the row: go1 <= 0.  F1' likewise down a column from
//   F1'[0][j] = -2^29 or the entering state, entering the band from above it (the dlo side).
//   Piece 2.  E2' = max(E2'_left, H'_left + go2) + dge adds dge = ge2 - ge1 per step, of either
//   sign: a chain that starts at a forced value k cells outside the band would arrive as -2^29
//   + k dge, which with dge > 0 and a long chain is no longer "minus infinity", and with dge <
//   0 drifts towards the int32 floor.  So E2' and F2' of an out-of-band cell are forced too:
//   the chain restarts at every such cell, and the first in-band cell of a row or a column
//   sees max(-2^29, -2^29 + go2) + dge = -2^29 + dge: ONE addition to the forced value, as in
//   nw_batch_dual.hip, |dge| < 2^13.  Its right (lower) neighbour takes the maximum with H' +
//   go2 of an in-band cell, a real value above -2^28, and the forced value is gone.
//   (How much the forcing of E2' and F2' buys: the range bound has 2 A (n1 + n2 + 2) < 2^28 with
//   |dge| <= 2 A, so an unforced chain drifts by less than 2^28 in all and stays below -2^28,
//   under every real value, and above the int32 floor.  Within the accepted range it is margin:
//   the sweep without it gives the same scores and ops on every test, DESIGN 6s.  It keeps the
//   statement "added to at most once" true without an appeal to the pair's size.)
//   Leaks.  What the in-band cells leak outward is a finite E1' right of the band (above it)
//   and a finite F1' below it; E2' and F2' leak nothing, they are forced where they arrive.
//   E1' moves right, away from the band, F1' down, away from it; the cells they reach have
//   H', E2' and F2' forced, E_t' never feeds F_t' nor F_t' E_t', and neither is accumulated.  So
//   no in-band cell reads them.
//   So every in-band cell sees -2^29 (or -2^29 + dge) for each predecessor outside the band,
//   and its diagonal predecessor, on the same diagonal, is in the band: H' of an in-band inner
//   cell is a real value (at least the path "diagonal, then one run", which never leaves the
//   band), its source bits never choose a value that came from outside, and a run state of the
//   walk is entered only where the run's value equals a real H', so the walk stays inside.
//   The range bound 3G + (M + A)(n1 + n2 + 2) < 2^28 of the two-piece entries still holds: its
//   lower bound for H needs a path with at most two openings inside the table, and "diagonal,
//   then one run" is such a path inside the band; the upper bound and the E_t / F_t bounds are
//   per step and unchanged; forced cells hold no real value.
//
// The entering state.  first(p) > 0: u, f1, f2, e1, e2, dg = -2^29, the state that the cells
// above the band would have left.  first(p) = 0: row 0 as in nw_batch_dual.hip with H'[0][c] =
// -2^29 for c > -dlo.  The feed of block b, lane x: row 64b + x of column 256p, all three
// values replaced by -2^29 unless dlo <= 64b + x - 256p <= dhi; strip 0 is fed the boundary
// column H'[r][0] = max(go1, go2 + r dge), in the band iff r <= dhi.
//
// Directions: a pair's block is [strip][slot][step][lane] dwords, slot = iteration - first(
// strip), batch_banded_slots(n1, n2, w) slots of 64 * 64 dwords per strip; byte k of a dword is
// column k's cell.  nw_batch_dual_banded_walk is nw_batch_dual_walk over dual_banded_dir_byte.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nw_batch_dual_dev.h"

namespace nw {
namespace {

// One pair (n1, n2 >= 1) by this wave: nw_batch_dual.hip's dual_pair under nw_batch_banded.hip's
// ranges (BandRange).  s1: the pair's column characters; rowb[y] = row y's letter; col: the
// worker's column scratch (H' at col[row], E1' at col[eoff + row], E2' at col[eoff2 + row]);
// dirs: DIRS: this lane's dword of the pair's first slot.
template <bool WIDE, bool DIRS>
__device__ __forceinline__ void dualb_pair(const BatchDualBandedArgs &BA, uint32_t *pl, const uint8_t *__restrict__ s1,
                                           int32_t n1, const uint8_t *__restrict__ rowb, int32_t n2,
                                           int32_t *__restrict__ col, uint32_t *__restrict__ dirs, int32_t *score,
                                           int lane) {
    const BatchDualArgs &DA = BA.d;
    const BatchArgs &A = DA.m.a.b;
    const int32_t ge1 = A.gap;
    const DualCost K{DA.m.a.gap_open, DA.gap_open2, DA.gap2 - ge1, -2 * ge1};
    const int64_t eoff = DA.m.a.eoff, eoff2 = DA.eoff2;
    const int nstrips = (n1 + kCkptCols - 1) / kCkptCols;
    BandRange R(n1, n2, BA.band);
    const int nblocks = R.nblocks, lastb = nblocks - 1;
    ProfileSub P{pl};

    for (int p = 0; p < nstrips; ++p) {
        R.strip(p, lane);
        const int32_t cl = 1 + R.c0 + C * lane;  // first column of this lane
        const int it0 = R.it0;
        DualLane S;
        if (it0 > 0) {
            // every cell before the range is above the band
#pragma unroll
            for (int k = 0; k < C; ++k) S.u[k] = S.f1[k] = S.f2[k] = kNegInf;
            S.dg = kNegInf;
        } else {
#pragma unroll
            for (int k = 0; k < C; ++k) {
                S.u[k] = (cl + k <= -R.dlo) ? K.boundary(cl + k) : kNegInf;  // H'[0][c]: in the band iff -c >= dlo
                S.f1[k] = S.f2[k] = kNegInf;                               // Ft'[0][c]
            }
            S.dg = 0;  // (replaced by H'[0][cl - 1] at the lane's row-0 step, before a cell reads it)
        }
        S.e1 = S.e2 = kNegInf;
        S.acch = S.acc1 = S.acc2 = 0;
        P.build(DA.m, s1, n1, cl);
        const bool fed = p > 0;            // (strip 0 never reads the scratch)
        const bool pub = p + 1 < nstrips;  // (the last strip's right column has no reader)

        // the feed of block b, masked: lane x holds row 64b + x of column c0 (strip 0: of the
        // boundary column, H'[r][0] per row, H'[0][0] = 0, Et'[r][0] = -inf)
        auto feed = [&](int b, int32_t &h, int32_t &e1, int32_t &e2) {
            const int32_t row = 64 * b + lane;
            h = row == 0 ? 0 : K.boundary(row);
            e1 = e2 = kNegInf;
            if (fed) {
                h = col[row];
                e1 = col[eoff + row];
                e2 = col[eoff2 + row];
            }
            const bool in = R.in(row);
            h = in ? h : kNegInf;
            e1 = in ? e1 : kNegInf;
            e2 = in ? e2 : kNegInf;
        };

        // row words and the feed are loaded one iteration ahead
        u32x4 pkc[4], pkn[4];
        load_rows(rowb, it0, lane, pkc);
        int32_t fnh, fn1, fn2;
        feed(it0, fnh, fn1, fn2);  // (it0 <= lastb: 256p + dlo < n2)
        // DIRS: this lane's dword of slot it - it0 of strip p, one slot further per iteration
        uint32_t *dq = nullptr;
        if constexpr (DIRS) dq = dirs + (int64_t)p * R.slots * (64 * kWave);
        for (int it = it0; it <= R.itl; ++it) {
            if (it < nblocks) {
                S.fvh = fnh;
                S.fv1 = fn1;
                S.fv2 = fn2;
            }
            feed(min(it + 1, lastb), fnh, fn1, fn2);
            load_rows(rowb, min(it + 1, nblocks), lane, pkn);
            const bool edge = it == 0 || 64 * it + 63 > n2;
            int32_t *colw = (pub && it > it0) ? col + 64 * (it - 1) : nullptr;
            if (R.inside(it)) {
                if (edge)
                    dual_iter<WIDE, true, false, DIRS>(it, pkc, n2, K, S, P, R.tb, R.span, colw, eoff, eoff2, dq,
                                                       lane);
                else
                    dual_iter<WIDE, false, false, DIRS>(it, pkc, n2, K, S, P, R.tb, R.span, colw, eoff, eoff2, dq,
                                                        lane);
            } else {
                if (edge)
                    dual_iter<WIDE, true, true, DIRS>(it, pkc, n2, K, S, P, R.tb, R.span, colw, eoff, eoff2, dq,
                                                      lane);
                else
                    dual_iter<WIDE, false, true, DIRS>(it, pkc, n2, K, S, P, R.tb, R.span, colw, eoff, eoff2, dq,
                                                       lane);
            }
#pragma unroll
            for (int h = 0; h < 4; ++h) pkc[h] = pkn[h];
            if constexpr (DIRS) dq += 64 * kWave;
        }
        // the lane of column n1 holds row n2 (an in-band cell, computed within the range)
        if (p == nstrips - 1) {
#pragma unroll
            for (int k = 0; k < C; ++k)
                if (cl + k == n1) *score = S.u[k] + ge1 * (n2 + n1);
        }
    }
}

// What the ticket loop below asks of a kernel: sweep_tickets' interface (nw_batch_dev.h),
// DualSweepBase over the launch's two-piece part and the sweep in its wide or narrow form.
struct DualBandedSweep : DualSweepBase {
    const BatchDualBandedArgs &BA;
    template <bool DIRS>
    __device__ __forceinline__ void pair(int32_t *out, const uint8_t *s1, int32_t n1, const uint8_t *rowb, int32_t n2,
                                         int32_t *col, uint32_t *dirs, int lane) const {
        if (BA.d.m.wide != 0)
            dualb_pair<true, DIRS>(BA, pl, s1, n1, rowb, n2, col, dirs, out, lane);
        else
            dualb_pair<false, DIRS>(BA, pl, s1, n1, rowb, n2, col, dirs, out, lane);
    }
};

// The kernel's body is sweep_tickets (nw_batch_dev.h) with one difference: the launch's arguments
// are read through a pointer to the kernel-argument segment that is made opaque once per ticket.
// This launch carries both parents' constants; read from the by-value parameter they are all
// loaded at entry and held across the pair's loops, and the directions kernel then runs out of
// scalar registers (5 spilled to lanes).  Read per ticket where they are used, nothing of the
// ticket loop's state is live across a pair but the segment pointer itself.  BatchDualBandedArgs
// is the kernel's only parameter: offset 0 of the segment.
template <bool DIRS>
__global__ __launch_bounds__(64) void nw_batch_dual_banded_sweep(BatchDualBandedArgs) {
    __shared__ uint32_t prof[kLetters * kWave];  // [row letter][lane], 8 KiB
    const int lane = threadIdx.x;
    for (;;) {
        auto kp = __builtin_amdgcn_kernarg_segment_ptr();  // (a pointer to constant address space)
        asm volatile("" : "+s"(kp));  // (no load of an argument moves above this point)
        const BatchDualBandedArgs &BA = *(const BatchDualBandedArgs *)kp;
        const DualBandedSweep mode{{BA.d, prof + lane}, BA};
        const BatchArgs &A = BA.d.m.a.b;
        const int t = __builtin_amdgcn_readfirstlane(claim_ticket(A.ticket));  // (a call returns in a vector register)
        if (t >= A.npairs) break;
        int pair = t;
        if (A.order != nullptr) pair = __builtin_amdgcn_readfirstlane(A.order[t]);
        const int64_t o1 = uniform64(A.off1[pair]), o2 = uniform64(A.off2[pair]);
        const int64_t len1 = uniform64(A.off1[pair + 1]) - o1, len2 = uniform64(A.off2[pair + 1]) - o2;
        int32_t *out = mode.result(pair);
        if (len1 < 0 || len2 < 0 || len1 >= INT32_MAX || len2 > A.max_n2) {
            mode.refused(out, lane);
        } else if (len1 == 0 || len2 == 0) {
            mode.empty(out, (int32_t)max(len1, len2), lane);
        } else {
            const uint8_t *s1 = A.s1 + o1;
            const uint8_t *rowb = A.rows + kBatchRowPad + o2 - 1;  // rowb[y] = row y's letter
            int32_t *col = A.colscr + (int64_t)blockIdx.x * A.cstride;
            uint32_t *dirs = nullptr;
            if constexpr (DIRS) dirs = (uint32_t *)(A.dirs + uniform64(A.dir_off[t])) + lane;
            mode.template pair<DIRS>(out, s1, (int32_t)len1, rowb, (int32_t)len2, col, dirs, lane);
        }
    }
}

// The walk of ticket t's pair from (n2, n1) to (0, 0): nw_batch_dual_walk (its header has the
// machine of five states) over the banded direction block.  It reads in-band cells only (the
// header); dual_banded_dir_byte clamps the slot all the same, so that no read can leave the
// pair's block.  (A second text, not a shared body: nw_batch_dual.hip's walk has the measurement.)
__global__ __launch_bounds__(64) void nw_batch_dual_banded_walk(BatchDualBandedWalkArgs B) {
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
    uint32_t state = 0;  // 0 H, 1 F1, 2 E1, 3 F2, 4 E2
    while (r > 0 || c > 0) {
        if (r == 0 || c == 0) {  // (state is H here)
            const uint32_t op = r == 0 ? 2u : 1u;
            ops[n++] = (uint8_t)op;
            r -= op != 2u;
            c -= op != 1u;
            continue;
        }
        const uint32_t bits = d[dual_banded_dir_byte(slots, dlo, r, c)];
        if (state == 0) {
            state = bits & 7u;
            if (state == 0) {
                ops[n++] = 0;
                --r;
                --c;
            }
        } else if (state & 1u) {  // F1 (bit 4), F2 (bit 6)
            ops[n++] = 1;
            --r;
            state = (bits & (state == 1u ? 16u : 64u)) ? state : 0u;
        } else {  // E1 (bit 3), E2 (bit 5)
            ops[n++] = 2;
            --c;
            state = (bits & (state == 2u ? 8u : 32u)) ? state : 0u;
        }
    }
    W.n_ops[t] = n;
}

}  // namespace

int launch_batch_dual_banded(const BatchDualBandedArgs &a, bool dirs, int grid, void *stream) {
    if (dirs)
        hipLaunchKernelGGL(nw_batch_dual_banded_sweep<true>, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream,
                           a);
    else
        hipLaunchKernelGGL(nw_batch_dual_banded_sweep<false>, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream,
                           a);
    return (int)hipGetLastError();
}

int launch_batch_dual_banded_walk(const BatchDualBandedWalkArgs &w, void *stream) {
    hipLaunchKernelGGL(nw_batch_dual_banded_walk, dim3((unsigned)((w.w.npairs + 63) / 64)), dim3(64), 0,
                       (hipStream_t)stream, w);
    return launch_batch_reverse(w.w, stream);
}

}  // namespace nw
