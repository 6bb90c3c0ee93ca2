// nw_batch_dual_dev.h -- device code shared by the two two-piece kernel files, nw_batch_dual.hip
// and nw_batch_dual_banded.hip, and private to them (the unnamed namespace, as nw_batch_dev.h):
// the lane's state and the launch's costs (DualLane, DualCost), the 64-step iteration of the
// five-value cell (dual_iter; nw_batch_dual.hip's header states the cell and the direction byte,
// nw_batch_dual_banded.hip's the mask) and what both sweep objects answer alike (DualSweepBase).
// The pair loops, the kernels, the launchers and the five-state walks are the files' own (one
// walk body over an address function was measured and is slower: nw_batch_dual.hip's walk).
#pragma once
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
//          (step - tb - k = the cell's diagonal - dlo), span = dhi - dlo.  Without it tb and
//          span are not read, and the unbanded kernels pass zeros.
//   colw : where H' of the right column of block it - 1 goes, E1' eoff and E2' eoff2 words
//          behind it (NULL: it has no reader)
//   dq   : DIRS: this lane's dword of the iteration's first step
template <bool WIDE, bool EDGE, bool MASK, bool DIRS>
__device__ __forceinline__ void dual_iter(int it, const u32x4 (&pk)[4], int32_t n2, const DualCost &K, DualLane &S,
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
                    // outside the band: H', E2' and F2' are minus infinity (nw_batch_dual_banded.hip)
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

// What a ticket loop asks of a two-piece kernel (sweep_tickets' interface, nw_batch_dev.h) and
// the band does not change: the launch's arguments, where a result goes, the pairs without a
// sweep.  A file's sweep object adds pair<DIRS>, the sweep in its wide or narrow form.
struct DualSweepBase {
    const BatchDualArgs &DA;
    uint32_t *pl;  // this lane's dword of profile row 0
    __device__ __forceinline__ const BatchAffineArgs &affine() const { return DA.m.a; }
    __device__ __forceinline__ int32_t *result(int pair) const { return DA.m.a.b.scores + pair; }
    // not a pair this launch was sized for: the column scratch would not hold it
    __device__ __forceinline__ void refused(int32_t *score, int lane) const {
        if (lane == 0) *score = INT32_MIN;
    }
    // no cells: the corner of the boundary, one gap of the cheaper piece (none for 0 x 0)
    __device__ __forceinline__ void empty(int32_t *score, int32_t n, int lane) const {
        if (lane == 0)
            *score = n > 0 ? max(DA.m.a.gap_open + DA.m.a.b.gap * n, DA.gap_open2 + DA.gap2 * n) : 0;
    }
};

}  // namespace
}  // namespace nw
