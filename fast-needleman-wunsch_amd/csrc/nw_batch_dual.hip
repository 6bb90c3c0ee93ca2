// nw_batch_dual.hip -- gfx950 (MI355X) batched pairwise global alignment under a TWO-PIECE
// affine gap cost with substitution by matrix: a run of k ups or of k lefts costs
//     g(k) = max(go1 + k * ge1, go2 + k * ge2)
// (piece 1 = gap_open, nw_params.gap; piece 2 = gap_open2, gap2; include/nw_hip.h states the
// recurrence and the walk).  The decomposition is the batch's (nw_batch_affine.hip's
// header): a persistent grid of one-wave workgroups claims pairs from the ticket
// (sweep_tickets), a worker sweeps its pair in 256-column strips, lane l owns columns 4l ..
// 4l+3 and at step s computes row s - l, lanes outside rows 1..n2 hold their cells (EDGE);
// the substitution is the matrix kernels' column profile in LDS (ProfileSub, build_profile,
// read one group ahead) over the same row letters and the same matrix bytes, wide or narrow.
// The pair and iteration loops are this file's own, as the affine and the banded files have
// theirs: sweep_iter carries two values from column to column, this cell carries three.
//
// The cell holds FIVE values, all with ge1 * (i + j) subtracted (the w form taken relative
// to piece 1; dge = ge2 - ge1):
//     E1' = max(E1'_left, H'_left + go1)               extending piece 1 is free
//     F1' = max(F1'_up,   H'_up   + go1)
//     E2' = max(E2'_left, H'_left + go2) + dge         piece 2 drifts by dge per step
//     F2' = max(F2'_up,   H'_up   + go2) + dge
//     H'  = max(H'_diag + s - 2 ge1, F1', E1', F2', E2')
//     H'[0][0] = 0, H'[0][c] = max(go1, go2 + c * dge), H'[r][0] likewise with r,
//     Et'[r][0] = Ft'[0][c] = -2^29
// so row 0 is no constant: a lane starts its four columns at their own H'[0][c], and strip
// 0's feed holds H'[r][0] per row.  The table bytes are s - 2 ge1, the matrix kernels'.  F1
// and F2 are lane-local (eight values); H, E1 and E2 of a lane's last column go to the right
// neighbour over DPP wave_shr:1, three moves per step.  The -2^29 is added to at most once
// (go, or dge) before a maximum drops it, and every real value stays above -2^28 (the
// host's dual_range_ok).
//
// Strip to strip, H', E1' and E2' of the right column are gathered (lane x holds row 64b +
// x) and go to the worker's column scratch -- three 256-byte stores per 64 steps, H at
// col[row], E1 at col[eoff + row], E2 at col[eoff2 + row] -- from where the same lanes load
// them back as strip p + 1's feed.  Strip 0 takes the boundary and never reads the scratch.
//
// The DIRECTIONS kernel writes one byte per cell: bits 0-2 the H source (0 diag, 1 F1, 2
// E1, 3 F2, 4 E2: the first in that order that equals H'), bits 3-6 "extended, not opened"
// for E1, F1, E2, F2 (opening wins a tie).  A lane's four cells of a step are one dword,
// stored [strip][iteration][step][lane]: every store instruction writes 256 contiguous
// bytes.  dual_dir_byte (nw_batch_dev.h) is that address; nw_batch_dual_walk, one thread
// per pair and a machine of five states, inverts it.  The reversal is nw_batch.hip's.
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
//   colw : where H' of the right column of block it - 1 goes, E1' eoff and E2' eoff2 words
//          behind it (NULL: it has no reader)
//   dq   : DIRS: this lane's dword of the iteration's first step
template <bool WIDE, bool EDGE, bool DIRS>
__device__ __forceinline__ void dual_iter(int it, const u32x4 (&pk)[4], int32_t n2, const DualCost &K, DualLane &S,
                                          ProfileSub &P, int32_t *colw, int64_t eoff, int64_t eoff2, uint32_t *dq,
                                          int lane) {
    int32_t rr = 64 * it - lane - 1;  // EDGE: row of this lane before the step
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
                const int32_t f2 = max(S.f2[k], fo2) + K.dge;
                const int32_t e2 = max(el2, eo2) + K.dge;
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

// One pair (n1, n2 >= 1), all its strips, by this wave.  s1: the pair's column characters;
// rowb[y] = row y's letter; col: the worker's column scratch (H' at col[row], E1' at col[eoff
// + row], E2' at col[eoff2 + row]); dirs: DIRS: this lane's dword of the pair's first step.
template <bool WIDE, bool DIRS>
__device__ __forceinline__ void dual_pair(const BatchDualArgs &DA, uint32_t *pl, const uint8_t *__restrict__ s1,
                                          int32_t n1, const uint8_t *__restrict__ rowb, int32_t n2,
                                          int32_t *__restrict__ col, uint32_t *__restrict__ dirs, int32_t *score,
                                          int lane) {
    const BatchArgs &A = DA.m.a.b;
    const int32_t ge1 = A.gap;
    const DualCost K{DA.m.a.gap_open, DA.gap_open2, DA.gap2 - ge1, -2 * ge1};
    const int64_t eoff = DA.m.a.eoff, eoff2 = DA.eoff2;
    const int nstrips = (n1 + kCkptCols - 1) / kCkptCols;
    const int nblocks = n2 / 64 + 1;  // ceil((n2 + 1) / 64)
    const int lastb = nblocks - 1;
    ProfileSub P{pl};

    for (int p = 0; p < nstrips; ++p) {
        const int32_t cl = 1 + p * kCkptCols + C * lane;  // first column of this lane
        DualLane S;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            S.u[k] = K.boundary(cl + k);  // H'[0][c]
            S.f1[k] = S.f2[k] = kNegInf;  // Ft'[0][c]
        }
        S.e1 = S.e2 = kNegInf;
        S.dg = 0;  // (replaced by H'[0][cl - 1] at the lane's row-0 step, before a cell reads it)
        S.acch = S.acc1 = S.acc2 = 0;
        P.build(DA.m, s1, n1, cl);
        const bool fed = p > 0;            // (strip 0 never reads the scratch)
        const bool pub = p + 1 < nstrips;  // (the last strip's right column has no reader)

        // row words and the feed are loaded one iteration ahead.  Strip 0: the boundary
        // column, H'[r][0] per row, H'[0][0] = 0 (the diagonal of cell (1, 1)), Et'[r][0] =
        // -inf
        u32x4 pkc[4], pkn[4];
        load_rows(rowb, 0, lane, pkc);
        int32_t fnh = lane == 0 ? 0 : K.boundary(lane), fn1 = kNegInf, fn2 = kNegInf;
        if (fed) {
            fnh = col[lane];
            fn1 = col[eoff + lane];
            fn2 = col[eoff2 + lane];
        }
        // row 64*nblocks - 1 completes on lane 63 in iteration nblocks
        for (int it = 0; it <= nblocks; ++it) {
            if (it < nblocks) {
                S.fvh = fnh;
                S.fv1 = fn1;
                S.fv2 = fn2;
            }
            // block it + 1 was stored by the strip before; this strip's own stores are
            // at block it - 1 and below
            if (fed) {
                const int64_t x = 64 * min(it + 1, lastb) + lane;
                fnh = col[x];
                fn1 = col[eoff + x];
                fn2 = col[eoff2 + x];
            } else {
                fnh = K.boundary(64 * min(it + 1, lastb) + lane);
            }
            load_rows(rowb, min(it + 1, nblocks), lane, pkn);
            const bool edge = it == 0 || 64 * it + 63 > n2;
            int32_t *colw = (pub && it >= 1) ? col + 64 * (it - 1) : nullptr;
            uint32_t *dq = nullptr;
            if constexpr (DIRS) dq = dirs + ((int64_t)p * (nblocks + 1) + it) * (64 * kWave);
            if (edge)
                dual_iter<WIDE, true, DIRS>(it, pkc, n2, K, S, P, colw, eoff, eoff2, dq, lane);
            else
                dual_iter<WIDE, false, DIRS>(it, pkc, n2, K, S, P, colw, eoff, eoff2, dq, lane);
#pragma unroll
            for (int h = 0; h < 4; ++h) pkc[h] = pkn[h];
        }
        // every lane now holds row n2 of its columns
        if (p == nstrips - 1) {
#pragma unroll
            for (int k = 0; k < C; ++k)
                if (cl + k == n1) *score = S.u[k] + ge1 * (n2 + n1);
        }
    }
}

// What sweep_tickets asks of a kernel (nw_batch_dev.h): the launch's arguments, where a
// result goes, the pairs without a sweep, and the sweep in its wide or narrow form.
struct DualSweep {
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
    template <bool DIRS>
    __device__ __forceinline__ void pair(int32_t *out, const uint8_t *s1, int32_t n1, const uint8_t *rowb, int32_t n2,
                                         int32_t *col, uint32_t *dirs, int lane) const {
        if (DA.m.wide != 0)
            dual_pair<true, DIRS>(DA, pl, s1, n1, rowb, n2, col, dirs, out, lane);
        else
            dual_pair<false, DIRS>(DA, pl, s1, n1, rowb, n2, col, dirs, out, lane);
    }
};

template <bool DIRS>
__global__ __launch_bounds__(64) void nw_batch_dual_sweep(BatchDualArgs DA) {
    __shared__ uint32_t prof[kLetters * kWave];  // [row letter][lane], 8 KiB
    sweep_tickets<DIRS>(DualSweep{DA, prof + threadIdx.x});
}

// The walk of ticket t's pair from (n2, n1) to (0, 0): one thread per pair, a machine of
// five states over the cells' bytes (dual_dir_byte).
//   H, on the boundary: row 0 is walked left and column 0 up without reading a byte
//   H, inner cell: bits 0-2: 0 emits a diag; 1 .. 4 switch to F1 / E1 / F2 / E2 and emit
//   nothing
//   F1, F2: emit an up and move; bit 4 / bit 6 of the cell it left: 1 stays, 0 returns to H
//   E1, E2: emit a left and move; bit 3 / bit 5 likewise
// Runs are entered at inner cells only and return to H at the latest when they reach row 1
// / column 1, where they can only have been opened.  Ops go end -> begin into the pair's
// slot; nw_batch_reverse turns them round.
__global__ __launch_bounds__(64) void nw_batch_dual_walk(BatchWalkArgs W) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= W.npairs) return;
    const int pair = W.order != nullptr ? W.order[t] : t;
    int64_t c = W.off1[pair + 1] - W.off1[pair], r = W.off2[pair + 1] - W.off2[pair];
    const int64_t iters = batch_iters(r);
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
        const uint32_t bits = d[dual_dir_byte(iters, r, c)];
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

int launch_batch_dual(const BatchDualArgs &a, bool dirs, int grid, void *stream) {
    if (dirs)
        hipLaunchKernelGGL(nw_batch_dual_sweep<true>, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(nw_batch_dual_sweep<false>, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_batch_dual_walk(const BatchWalkArgs &w, void *stream) {
    hipLaunchKernelGGL(nw_batch_dual_walk, dim3((unsigned)((w.npairs + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                       w);
    return launch_batch_reverse(w, stream);
}

}  // namespace nw
