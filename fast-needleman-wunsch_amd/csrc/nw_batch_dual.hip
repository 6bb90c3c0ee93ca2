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
// The pair loop is this file's own and the iteration (dual_iter) nw_batch_dual_dev.h's, shared
// with nw_batch_dual_banded.hip: sweep_iter carries two values from column to column, this
// cell carries three.
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

#include "nw_batch_dual_dev.h"

namespace nw {
namespace {

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
                dual_iter<WIDE, true, false, DIRS>(it, pkc, n2, K, S, P, 0, 0, colw, eoff, eoff2, dq, lane);
            else
                dual_iter<WIDE, false, false, DIRS>(it, pkc, n2, K, S, P, 0, 0, colw, eoff, eoff2, dq, lane);
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

// What sweep_tickets asks of a kernel (nw_batch_dev.h): DualSweepBase and the sweep in its wide
// or narrow form.
struct DualSweep : DualSweepBase {
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
    sweep_tickets<DIRS>(DualSweep{{DA, prof + threadIdx.x}});
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
// (Its text stands here and again in nw_batch_dual_banded.hip: as one body in
// nw_batch_dual_dev.h over an address function, walk_ms of both came out 0.5 to 1.4 % above the
// parent's where the parent's spread was 0.4 to 1.4 %, the loop with two register pairs
// exchanged and one more v_mov_b64; profiles/batch_dual_refactor_ab.json.)
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
