// nw_batch_local.hip -- gfx950 (MI355X) batched pairwise LOCAL alignment: Smith-Waterman
// under affine gap cost (Gotoh) with substitution by matrix (nw_score_batch_local*,
// nw_align_batch_local; include/nw_hip.h states the recurrence and the walk).
// Everything but the cell is described in nw_batch_matrix.hip's and nw_batch_affine.hip's
// headers and is nw_batch_dev.h's code, the same the matrix kernel runs: the persistent
// grid of one-wave workgroups and the ticket, the 256-column strips with lane l on columns
// 4l .. 4l+3, the EDGE test, the row letters (launch_batch_matrix_rows, that file's), the
// 8 KiB column profile in LDS read one group ahead (ProfileSub), the two-column scratch
// between strips and the layout of the 4 direction bits per cell.  This file adds the
// policy with the local cell, its boundaries, the best cell and the hit, and the walk
// that starts at the hit (its own loop: on one body with the affine walk it came out
// 1 % slower; the two share the index of a cell's bits, NW_DIR_NIBBLE).
//
// The cell.  H, E and F are held UNSHIFTED (not the w form of the global kernels): the
// floor of the local recurrence is then the constant 0 and both boundaries are the
// constant H = 0, where the w form would carry a floor and boundaries of -ge*(i+j) that
// differ from cell to cell.  Every real E and F is >= go + ge, so "minus infinity" is go
// + ge itself, the profile bytes are the matrix's own (no `wide` variant), and no value
// leaves [go + 2ge, M * min(n1, n2)].  A cell forms ho = H + go + ge once; the cell to
// its right takes it as the opening of E and the cell below as the opening of F:
//     d = diag + s;  f = max(F_up + ge, ho_up);  e = max(E_left + ge, ho_left)
//     H = max(max3(d, f, e), 0);  ho = H + (go + ge)
// -- 8 VALU where the global cell has 6.
//
// The best cell.  Per column a lane keeps the largest H seen and the STEP (64 it + u, a
// scalar) at which it first appeared: compare, select, max -- 3 VALU per cell.  Only a
// strictly greater value updates, so a column keeps its earliest row; a held EDGE cell
// repeats the value above it and cannot win; rows outside 1 .. n2 are never active.
// Columns past n1 do compute cells (of column n1's letter): they are dropped when the
// strip ends, where the lane folds its columns (<= n1, value > 0) into its best of the
// pair by (score desc, row asc, column asc).  Once per pair the 64 lanes' bests are
// combined with the same key, over the initial best 0 at (0, 0), and lane 0 writes the
// nw_local_hit.  All of this state is initialised per strip / per pair: nothing of the
// pair a worker ran before is left.
//
// Directions (align kernel): bits 0-1: 3 = H == 0 (tested first), else 0 / 1 / 2 = the
// first of diag, F, E that equals H; bit 2: E was extended (strictly better than
// opening); bit 3: F likewise.  nw_batch_local_walk starts one thread per ticket at the
// hit's end cell and stops in state H on code 3 or on row 0 / column 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nw_batch_dev.h"

namespace nw {
namespace {

struct LocalCell : GotohLane, ProfileSub {
    const BatchMatrixArgs &MA;
    int32_t ge, goe;  // goe: go + ge
    int32_t *hit;
    int lane;
    int32_t ho[C];  // u[k] + go + ge: what a gap opened from that cell holds
    int32_t bv[C];  // largest H of column k so far (>= 0)
    int32_t bs[C];  // the step at which bv[k] first appeared (row = step - lane)
    int32_t pv = 0, pi = 0, pj = 0;  // this lane's best of the pair: 0 at (0, 0)

    template <class M>
    __device__ __forceinline__ LocalCell(const M &mode, int32_t *out, int lane_)
        : ProfileSub{mode.pl},
          MA(mode.LA.m),
          ge(MA.a.b.gap),
          goe(MA.a.gap_open + MA.a.b.gap),
          hit(out),
          lane(lane_) {}
    __device__ __forceinline__ void strip_begin(const uint8_t *__restrict__ s1, int32_t n1, int32_t cl) {
#pragma unroll
        for (int k = 0; k < C; ++k) {
            u[k] = 0;  // H[0][c]
            ho[k] = goe;
            f[k] = goe;  // F[0][c]: "minus infinity"
            bv[k] = 0;
            bs[k] = 0;
        }
        e = goe;
        dg = 0;
        build(MA, s1, n1, cl);  // (past n1: column n1's letter; those cells are dropped in strip_end)
    }
    // H[i][0], E[i][0]
    __device__ __forceinline__ int32_t boundary_h(bool) const { return 0; }
    __device__ __forceinline__ int32_t boundary_e() const { return goe; }
    __device__ __forceinline__ int32_t opening(int32_t left) const { return left + goe; }
    template <int q, int k>
    __device__ __forceinline__ int32_t diag_sub(int32_t diag) const {
        return diag + score_byte<q, k>();
    }
    template <int k, int SH, bool EDGE, bool DIRS>
    __device__ __forceinline__ void cell(int32_t d, int32_t &diag, int32_t &lo, int32_t &el, bool act, int32_t step,
                                         uint32_t &bits) {
        const int32_t up = u[k];
        const int32_t fx = f[k] + ge, ex = el + ge;  // the run goes on
        const int32_t fn = max(fx, ho[k]);
        const int32_t en = max(ex, lo);
        // H = max(0, H_diag + s, F, E)
        int32_t x = max(max(max(d, fn), en), 0);
        if constexpr (DIRS) {
            uint32_t code = x == d ? 0u : x == fn ? 1u : 2u;
            code = x == 0 ? 3u : code;
            code |= ex > lo ? 4u : 0u;
            code |= fx > ho[k] ? 8u : 0u;
            bits |= code << SH;
        }
        diag = up;
        if constexpr (EDGE) {
            x = act ? x : up;
            f[k] = act ? fn : f[k];
        } else {
            f[k] = fn;
        }
        // (a held cell repeats `up`, which bv[k] has seen: it never updates)
        const bool better = x > bv[k];
        bs[k] = better ? step : bs[k];
        bv[k] = max(bv[k], x);
        u[k] = x;
        lo = x + goe;
        ho[k] = lo;
        el = en;
    }
    // The best-cell updates hang off the cells' dependency chain and nothing in the
    // iteration waits for them: left alone, the compiler sinks all of them behind the
    // iteration and keeps every H of its 256 cells alive for that (512 registers and
    // scratch).  The group's updates are done here, and nothing moves across its end.
    __device__ __forceinline__ void group_end() {
#pragma unroll
        for (int k = 0; k < C; ++k) asm volatile("" : "+v"(bv[k]), "+v"(bs[k]));
        __builtin_amdgcn_sched_barrier(0);
    }
    // the strip's columns into the lane's best: real columns with a positive value only
    // (a column that never rose above 0 cannot beat 0 at (0, 0))
    __device__ __forceinline__ void strip_end(bool, int32_t cl, int32_t n1, int32_t) {
        int32_t tv = pv, ti = pi, tj = pj;  // (locals: the updates become selects, not branches)
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const int32_t v = bv[k], i = bs[k] - lane, j = cl + k;
            if (j <= n1 && v > 0 && before(v, i, j, tv, ti, tj)) {
                tv = v;
                ti = i;
                tj = j;
            }
        }
        pv = tv, pi = ti, pj = tj;
    }
    // the 64 lanes' bests, once per pair; lane 0 writes the hit
    __device__ __forceinline__ void pair_end() {
        int32_t tv = pv, ti = pi, tj = pj;
#pragma unroll
        for (int m = 1; m < kWave; m <<= 1) {
            const int32_t ov = __shfl_xor(tv, m), oi = __shfl_xor(ti, m), oj = __shfl_xor(tj, m);
            if (before(ov, oi, oj, tv, ti, tj)) {
                tv = ov;
                ti = oi;
                tj = oj;
            }
        }
        if (lane == 0) {
            hit[0] = tv;
            hit[1] = ti;
            hit[2] = tj;
            hit[3] = -1;  // (the walk writes the begin cell)
            hit[4] = -1;
            hit[5] = hit[6] = hit[7] = 0;
        }
    }
};

struct LocalSweep {
    const BatchLocalArgs &LA;
    uint32_t *pl;  // this lane's dword of profile row 0
    __device__ __forceinline__ const BatchAffineArgs &affine() const { return LA.m.a; }
    __device__ __forceinline__ int32_t *result(int pair) const {
        return LA.hits + (int64_t)pair * kBatchLocalHitWords;
    }
    // not a pair this launch was sized for: the column scratch would not hold it
    __device__ __forceinline__ void refused(int32_t *hit, int lane) const {
        if (lane < kBatchLocalHitWords) hit[lane] = lane == 0 ? INT32_MIN : lane < 5 ? -1 : 0;
    }
    // no cells: 0 at (0, 0)
    __device__ __forceinline__ void empty(int32_t *hit, int32_t, int lane) const {
        if (lane < kBatchLocalHitWords) hit[lane] = (lane == 3 || lane == 4) ? -1 : 0;
    }
    template <bool DIRS>
    __device__ __forceinline__ void pair(int32_t *out, const uint8_t *s1, int32_t n1, const uint8_t *rowb, int32_t n2,
                                         int32_t *col, uint32_t *dirs, int lane) const {
        sweep_pair<LocalCell, DIRS>(*this, out, s1, n1, rowb, n2, col, dirs, lane);
    }
};

template <bool DIRS>
__global__ __launch_bounds__(64) void nw_batch_local_sweep(BatchLocalArgs LA) {
    __shared__ uint32_t prof[kLetters * kWave];  // [row letter][lane], 8 KiB
    sweep_tickets<DIRS>(LocalSweep{LA, prof + threadIdx.x});
}

// The walk: one thread per ticket over the direction bits of nw_batch_local_sweep<true>,
// in nw_batch_affine.hip's layout.  It starts at the hit's end cell in state H.
//   H, on row 0 / column 0 or at a cell with bits 0-1 = 3 (H == 0): stop; that cell is
//     the begin cell
//   H, else: 0 emits a diag; 1 / 2 switch to F / E and emit nothing
//   F: emits an up and moves; bit 3 of the cell it left: 1 stays in F, 0 returns to H
//   E: emits a left and moves; bit 2 likewise
// F and E are entered at inner cells only and return to H at the latest when the run
// reaches row 1 / column 1, where it can only have been opened.  Ops go end -> begin
// into the pair's slot; nw_batch_reverse turns them round.
__global__ __launch_bounds__(64) void nw_batch_local_walk(BatchLocalWalkArgs LW) {
    const BatchWalkArgs &W = LW.w;
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= W.npairs) return;
    const int pair = W.order != nullptr ? W.order[t] : t;
    const int64_t n1 = W.off1[pair + 1] - W.off1[pair], n2 = W.off2[pair + 1] - W.off2[pair];
    int32_t *hit = LW.hits + (int64_t)pair * kBatchLocalHitWords;
    int64_t r = hit[1], c = hit[2];
    if (r < 0 || c < 0 || r > n2 || c > n1) r = c = 0;  // (not a hit of this pair's table: nothing to walk)
    const int64_t iters = batch_iters(n2);
    const uint8_t *d = W.dirs + W.dir_off[t];
    uint8_t *ops = W.ops + W.ops_off[t];
    int64_t n = 0;
    uint32_t state = 0;  // 0 H, 1 F, 2 E
    while (r > 0 && c > 0) {
        NW_DIR_NIBBLE(bits, d, iters, r, c);
        if (state == 0) {
            state = bits & 3u;
            if (state == 3u) break;
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
    hit[3] = (int32_t)r;
    hit[4] = (int32_t)c;
    W.n_ops[t] = n;
}

}  // namespace

int launch_batch_local(const BatchLocalArgs &a, bool dirs, int grid, void *stream) {
    if (dirs)
        hipLaunchKernelGGL(nw_batch_local_sweep<true>, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(nw_batch_local_sweep<false>, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_batch_local_walk(const BatchLocalWalkArgs &w, void *stream) {
    hipLaunchKernelGGL(nw_batch_local_walk, dim3((unsigned)((w.w.npairs + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                       w);
    return launch_batch_reverse(w.w, stream);
}

}  // namespace nw
