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
// The iteration (dualb_iter) is a second copy of nw_batch_dual.hip's dual_iter with a MASK
// parameter, not a shared template: that file's kernels are held to the ISA of their parent
// build, and an iteration moved into nw_batch_dev.h behind a hook is a different inlining
// unit to the optimiser (the NW_DIR_NIBBLE note there records one such move that changed a
// register allocation).  MASK = false is that iteration instruction for instruction in
// source; the wave-uniformly "inside" iterations (64it - 256p - 319 >= dlo and 64it + 62 -
// 256p <= dhi, nw_batch_banded.hip's test) run it, only the others pay the mask.
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

#include "nw_batch_dev.h"

namespace nw {
namespace {

struct DualLane {
    int32_t u[C];   // H' of the lane's current row, column k
    int32_t f1[C];  // F1' of the lane's current row, column k
    int32_t f2[C];  // F2'
    int32_t e1;     // E1' of the lane's current row, last column
    int32_t e2;     // E2'
    int32_t dg;     // H'_diag of column 0 for the next step
    int32_t fvh, fv1, fv2;     // feed: lane x holds H' / E1' / E2' of the left strip's right column at row 64it + x
    int32_t acch, acc1, acc2;  // right column gathered: lane x holds row 64(it-1) + x
};

// what a launch's costs are to the cell
struct DualCost {
    int32_t go1, go2;
    int32_t dge;   // ge2 - ge1
    int32_t bias;  // WIDE: -2 ge1
    // H' of the boundary cell k columns (or rows) from the corner, k >= 1
    __device__ __forceinline__ int32_t boundary(int32_t k) const {
        return max(go1, (int32_t)((uint32_t)go2 + (uint32_t)k * (uint32_t)dge));
    }
};

// 64 steps of iteration `it` (steps 64it + u): lane l computes row 64it + u - l.
//   EDGE : some lane's row is outside 1..n2 in this iteration (it holds its cells)
//   MASK : some cell of this iteration may lie outside the band: tb = 256p + 5 lane + 1 + dlo
//          (step - tb - k = the cell's diagonal - dlo), span = dhi - dlo
//   colw : where H' of the right column of block it - 1 goes, E1' eoff and E2' eoff2 words
//          behind it (NULL: it has no reader)
//   dq   : DIRS: this lane's dword of the iteration's first step
template <bool WIDE, bool EDGE, bool MASK, bool DIRS>
__device__ __forceinline__ void dualb_iter(int it, const u32x4 (&pk)[4], int32_t n2, const DualCost &K, DualLane &S,
                                           ProfileSub &P, int32_t tb, uint32_t span, int32_t *colw, int64_t eoff,
                                           int64_t eoff2, uint32_t *dq, int lane) {
    int32_t rr = 64 * it - lane - 1;  // EDGE: row of this lane before the step
    int32_t tt = 64 * it - tb - 1;    // MASK: column 0's diagonal - dlo before the step
    P.iter_begin(pk);
    static_for<0, 16>([&](auto gc) {
        constexpr int gi = decltype(gc)::value;
        P.template group_begin<gi>(pk);
        static_for<0, 4>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            constexpr int u = 4 * gi + q;
            const int32_t lfh = __builtin_amdgcn_readlane(S.fvh, u);
            const int32_t lf1 = __builtin_amdgcn_readlane(S.fv1, u);
            const int32_t lf2 = __builtin_amdgcn_readlane(S.fv2, u);
            int32_t left = __builtin_amdgcn_update_dpp(lfh, S.u[C - 1], 0x138 /*wave_shr:1*/, 0xF, 0xF, false);
            int32_t el1 = __builtin_amdgcn_update_dpp(lf1, S.e1, 0x138 /*wave_shr:1*/, 0xF, 0xF, false);
            int32_t el2 = __builtin_amdgcn_update_dpp(lf2, S.e2, 0x138 /*wave_shr:1*/, 0xF, 0xF, false);
            int32_t diag = S.dg;
            S.dg = left;
            bool act = true;
            if constexpr (EDGE) {
                rr += 1;
                asm volatile("" : "+v"(rr));  // keep the activity test in the loop
                act = rr >= 1 && rr <= n2;
            }
            if constexpr (MASK) {
                tt += 1;
                asm volatile("" : "+v"(tt));  // (one counter, not 64 constants)
            }
            uint32_t dw = 0;  // DIRS: byte k = column k's cell of this step
            static_for<0, C>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                int32_t d = diag + P.template score_byte<q, k>();
                if constexpr (WIDE) d += K.bias;
                const int32_t up = S.u[k];
                const int32_t fo1 = up + K.go1, eo1 = left + K.go1;  // a run opened from H'
                const int32_t fo2 = up + K.go2, eo2 = left + K.go2;
                const int32_t f1 = max(S.f1[k], fo1);
                const int32_t e1 = max(el1, eo1);
                int32_t f2 = max(S.f2[k], fo2) + K.dge;
                int32_t e2 = max(el2, eo2) + K.dge;
                // H' = max(H'_diag + s - 2 ge1, F1', E1', F2', E2')
                int32_t x = max(max(max(d, f1), e1), max(f2, e2));
                if constexpr (DIRS) {
                    uint32_t code = x == d ? 0u : x == f1 ? 1u : x == e1 ? 2u : x == f2 ? 3u : 4u;
                    code |= el1 > eo1 ? 8u : 0u;
                    code |= S.f1[k] > fo1 ? 16u : 0u;
                    code |= el2 > eo2 ? 32u : 0u;
                    code |= S.f2[k] > fo2 ? 64u : 0u;
                    dw |= code << (8 * k);
                }
                if constexpr (MASK) {
                    // outside the band: H', E2' and F2' are minus infinity (the header)
                    const bool out = (uint32_t)(tt - k) > span;
                    x = out ? kNegInf : x;
                    e2 = out ? kNegInf : e2;
                    f2 = out ? kNegInf : f2;
                }
                diag = up;
                if constexpr (EDGE) {
                    x = act ? x : up;
                    S.f1[k] = act ? f1 : S.f1[k];
                    S.f2[k] = act ? f2 : S.f2[k];
                } else {
                    S.f1[k] = f1;
                    S.f2[k] = f2;
                }
                S.u[k] = x;
                left = x;
                el1 = e1;
                el2 = e2;
            });
            if constexpr (EDGE) {
                S.e1 = act ? el1 : S.e1;
                S.e2 = act ? el2 : S.e2;
            } else {
                S.e1 = el1;
                S.e2 = el2;
            }
            // lane 63 is on row 64(it-1) + u + 1: into lane (u + 1) % 64 of the gathers
            const int32_t rvh = __builtin_amdgcn_readlane(S.u[C - 1], 63);
            const int32_t rv1 = __builtin_amdgcn_readlane(S.e1, 63);
            const int32_t rv2 = __builtin_amdgcn_readlane(S.e2, 63);
            if constexpr (u == 63) {
                // rows 64(it-1) .. + 63 are gathered (lane 0 since the step before this
                // iteration): out, before lane 0 takes row 64it
                if (colw != nullptr) {
                    colw[lane] = S.acch;
                    colw[eoff + lane] = S.acc1;
                    colw[eoff2 + lane] = S.acc2;
                }
            }
            asm("v_writelane_b32 %0, %1, %2" : "+v"(S.acch) : "s"(rvh), "i"((u + 1) & 63));
            asm("v_writelane_b32 %0, %1, %2" : "+v"(S.acc1) : "s"(rv1), "i"((u + 1) & 63));
            asm("v_writelane_b32 %0, %1, %2" : "+v"(S.acc2) : "s"(rv2), "i"((u + 1) & 63));
            if constexpr (DIRS) dq[u * kWave] = dw;
        });
    });
}

// One pair (n1, n2 >= 1) by this wave: nw_batch_dual.hip's dual_pair under nw_batch_banded.hip's
// ranges.  s1: the pair's column characters; rowb[y] = row y's letter; col: the worker's column
// scratch (H' at col[row], E1' at col[eoff + row], E2' at col[eoff2 + row]); dirs: DIRS: this
// lane's dword of the pair's first slot.
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
    const int nblocks = n2 / 64 + 1;  // ceil((n2 + 1) / 64)
    const int lastb = nblocks - 1;
    const int32_t dlo = (int32_t)batch_banded_dlo(n1, n2, BA.band);
    const int32_t dhi = (int32_t)batch_banded_dhi(n1, n2, BA.band);
    const int slots = (int)batch_banded_slots(n1, n2, BA.band);
    const uint32_t span = (uint32_t)(dhi - dlo);
    ProfileSub P{pl};

    for (int p = 0; p < nstrips; ++p) {
        const int32_t c0 = p * kCkptCols;      // the column the strip is fed from
        const int32_t cl = 1 + c0 + C * lane;  // first column of this lane
        const int it0 = (int)batch_banded_first(p, dlo);
        // (never beyond the strip's slots: the range is that short by its definition, and a
        // store past the pair's direction block must be impossible whatever the arithmetic)
        const int itl = min(min(nblocks, ((c0 + 319 + dhi) >> 6) + 1), it0 + slots - 1);
        const int32_t tb = c0 + 5 * lane + 1 + dlo;
        const int32_t fb = lane - c0 - dlo;    // 64b + fb = (row 64b + lane of column c0)'s diagonal - dlo
        // iterations in_lo .. in_hi lie wholly in the band: 64it - c0 - 319 >= dlo and 64it + 62 - c0
        // <= dhi (floor divisions: both numerators may be negative)
        const int in_lo = (c0 + 319 + dlo + 63) >> 6, in_hi = (dhi + c0 - 62) >> 6;
        DualLane S;
        if (it0 > 0) {
            // every cell before the range is above the band
#pragma unroll
            for (int k = 0; k < C; ++k) S.u[k] = S.f1[k] = S.f2[k] = kNegInf;
            S.dg = kNegInf;
        } else {
#pragma unroll
            for (int k = 0; k < C; ++k) {
                S.u[k] = (cl + k <= -dlo) ? K.boundary(cl + k) : kNegInf;  // H'[0][c]: in the band iff -c >= dlo
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
            const bool in = (uint32_t)(64 * b + fb) <= span;
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
        if constexpr (DIRS) dq = dirs + (int64_t)p * slots * (64 * kWave);
        for (int it = it0; it <= itl; ++it) {
            if (it < nblocks) {
                S.fvh = fnh;
                S.fv1 = fn1;
                S.fv2 = fn2;
            }
            feed(min(it + 1, lastb), fnh, fn1, fn2);
            load_rows(rowb, min(it + 1, nblocks), lane, pkn);
            const bool edge = it == 0 || 64 * it + 63 > n2;
            const bool inside = it >= in_lo && it <= in_hi;
            int32_t *colw = (pub && it > it0) ? col + 64 * (it - 1) : nullptr;
            if (inside) {
                if (edge)
                    dualb_iter<WIDE, true, false, DIRS>(it, pkc, n2, K, S, P, tb, span, colw, eoff, eoff2, dq, lane);
                else
                    dualb_iter<WIDE, false, false, DIRS>(it, pkc, n2, K, S, P, tb, span, colw, eoff, eoff2, dq, lane);
            } else {
                if (edge)
                    dualb_iter<WIDE, true, true, DIRS>(it, pkc, n2, K, S, P, tb, span, colw, eoff, eoff2, dq, lane);
                else
                    dualb_iter<WIDE, false, true, DIRS>(it, pkc, n2, K, S, P, tb, span, colw, eoff, eoff2, dq, lane);
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

// What the ticket loop below asks of a kernel: sweep_tickets' interface (nw_batch_dev.h).
struct DualBandedSweep {
    const BatchDualBandedArgs &BA;
    uint32_t *pl;  // this lane's dword of profile row 0
    __device__ __forceinline__ const BatchAffineArgs &affine() const { return BA.d.m.a; }
    __device__ __forceinline__ int32_t *result(int pair) const { return BA.d.m.a.b.scores + pair; }
    // not a pair this launch was sized for: the column scratch would not hold it
    __device__ __forceinline__ void refused(int32_t *score, int lane) const {
        if (lane == 0) *score = INT32_MIN;
    }
    // no cells: the corner of the boundary, one gap of the cheaper piece (none for 0 x 0)
    __device__ __forceinline__ void empty(int32_t *score, int32_t n, int lane) const {
        if (lane == 0)
            *score = n > 0 ? max(BA.d.m.a.gap_open + BA.d.m.a.b.gap * n, BA.d.gap_open2 + BA.d.gap2 * n) : 0;
    }
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
        const DualBandedSweep mode{BA, prof + lane};
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
// pair's block.
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
