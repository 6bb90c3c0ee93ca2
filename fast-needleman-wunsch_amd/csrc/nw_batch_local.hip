// nw_batch_local.hip -- gfx950 (MI355X) batched pairwise LOCAL alignment: Smith-Waterman
// under affine gap cost (Gotoh) with substitution by matrix (nw_score_batch_local*,
// nw_align_batch_local; include/nw_hip.h states the recurrence and the walk).
// Everything but the cell is nw_batch_matrix.hip's, whose header describes it: the
// persistent grid of one-wave workgroups and the ticket, the 256-column strips with lane
// l on columns 4l .. 4l+3, the EDGE test, the row letters (launch_batch_matrix_rows, that
// file's), the 8 KiB column profile in LDS read one group ahead, the two-column scratch
// between strips and the layout of the 4 direction bits per cell.
//
// The sweep's iteration body stands here once more, on purpose: nw_batch.hip,
// nw_batch_affine.hip and nw_batch_matrix.hip stay byte-identical, so their kernels'
// code cannot move with a change made for the local mode.
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

#include <algorithm>
#include <type_traits>

#include "nw_batch.h"
#include "nw_dev.h"
#include "nw_internal.h"
#include "nw_strips.h"  // (u32x4)

namespace nw {
namespace {

constexpr int C = kCkptC;
constexpr int kLetters = kBatchMatrixLetters;

struct LocalLane {
    int32_t u[C];        // H of the lane's current row, column k
    int32_t ho[C];       // the same + go + ge: what a gap opened from that cell holds
    int32_t f[C];        // F of the lane's current row, column k
    int32_t e;           // E of the lane's current row, last column
    int32_t dg;          // H_diag of column 0 for the next step
    int32_t fvh, fve;    // feed: lane x holds H / E of the left strip's right column at row 64it + x
    int32_t acch, acce;  // right column gathered: lane x holds row 64(it-1) + x
    int32_t bv[C];       // largest H of column k so far (>= 0)
    int32_t bs[C];       // the step at which bv[k] first appeared (row = step - lane)
};

// (nw_batch_matrix.hip load_rows)
__device__ __forceinline__ void load_rows(const uint8_t *__restrict__ rowb, int j, int lane, u32x4 (&pk)[4]) {
    const uint8_t *b = rowb + (int64_t)j * 64 - lane;
#pragma unroll
    for (int h = 0; h < 4; ++h) __builtin_memcpy(&pk[h], b + 16 * h, 16);
}

// 64 steps of iteration `it` (nw_batch_matrix.hip matrix_iter).  pl: this lane's dword of
// profile row 0; goe: go + ge.
template <bool EDGE, bool DIRS>
__device__ __forceinline__ void local_iter(int it, const u32x4 (&pk)[4], const uint32_t *pl, int32_t ge, int32_t goe,
                                           int32_t n2, LocalLane &S, int32_t *colw, int64_t eoff, uint32_t *dq,
                                           int lane) {
    int32_t rr = 64 * it - lane - 1;  // EDGE: row of this lane before the step
    // the profile dwords of a group are read one group ahead of their use (matrix_iter)
    uint32_t scn[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) scn[q] = pl[((pk[0][0] >> (8 * q)) & 255u) * kWave];
    static_for<0, 16>([&](auto gc) {
        constexpr int gi = decltype(gc)::value;
        uint32_t sc[4];  // step q (row letter: byte q of the row word): byte k = the score byte of column k
#pragma unroll
        for (int q = 0; q < 4; ++q) sc[q] = scn[q];
        if constexpr (gi < 15) {
            const uint32_t word = pk[(gi + 1) >> 2][(gi + 1) & 3];  // row letters of steps 4gi+4 .. 4gi+7
#pragma unroll
            for (int q = 0; q < 4; ++q) scn[q] = pl[((word >> (8 * q)) & 255u) * kWave];
        }
        uint32_t dw[2] = {0, 0};  // DIRS: 4 bits per cell, dword h halfword q & 1 = step 4gi + q, nibble k = column k
        static_for<0, 4>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            constexpr int u = 4 * gi + q;
            const int32_t step = 64 * it + u;  // (scalar)
            const int32_t lfh = __builtin_amdgcn_readlane(S.fvh, u);
            const int32_t lfe = __builtin_amdgcn_readlane(S.fve, u);
            const int32_t left = __builtin_amdgcn_update_dpp(lfh, S.u[C - 1], 0x138 /*wave_shr:1*/, 0xF, 0xF, false);
            int32_t el = __builtin_amdgcn_update_dpp(lfe, S.e, 0x138 /*wave_shr:1*/, 0xF, 0xF, false);
            int32_t lo = left + goe;
            int32_t diag = S.dg;
            S.dg = left;
            bool act = true;
            if constexpr (EDGE) {
                rr += 1;
                asm volatile("" : "+v"(rr));  // keep the activity test in the loop
                act = rr >= 1 && rr <= n2;
            }
            static_for<0, C>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                const int32_t d = diag + (int32_t)(int8_t)(uint8_t)(sc[q] >> (8 * k));
                const int32_t up = S.u[k];
                const int32_t fx = S.f[k] + ge, ex = el + ge;  // the run goes on
                const int32_t f = max(fx, S.ho[k]);
                const int32_t e = max(ex, lo);
                // H = max(0, H_diag + s, F, E)
                int32_t x = max(max(max(d, f), e), 0);
                if constexpr (DIRS) {
                    uint32_t code = x == d ? 0u : x == f ? 1u : 2u;
                    code = x == 0 ? 3u : code;
                    code |= ex > lo ? 4u : 0u;
                    code |= fx > S.ho[k] ? 8u : 0u;
                    dw[q >> 1] |= code << (16 * (q & 1) + 4 * k);
                }
                diag = up;
                if constexpr (EDGE) {
                    x = act ? x : up;
                    S.f[k] = act ? f : S.f[k];
                } else {
                    S.f[k] = f;
                }
                // (a held cell repeats `up`, which bv[k] has seen: it never updates)
                const bool better = x > S.bv[k];
                S.bs[k] = better ? step : S.bs[k];
                S.bv[k] = max(S.bv[k], x);
                S.u[k] = x;
                lo = x + goe;
                S.ho[k] = lo;
                el = e;
            });
            if constexpr (EDGE)
                S.e = act ? el : S.e;
            else
                S.e = el;
            // lane 63 is on row 64(it-1) + u + 1: into lane (u + 1) % 64 of the gathers
            const int32_t rvh = __builtin_amdgcn_readlane(S.u[C - 1], 63);
            const int32_t rve = __builtin_amdgcn_readlane(S.e, 63);
            if constexpr (u == 63) {
                if (colw != nullptr) {
                    colw[lane] = S.acch;
                    colw[eoff + lane] = S.acce;
                }
            }
            asm("v_writelane_b32 %0, %1, %2" : "+v"(S.acch) : "s"(rvh), "i"((u + 1) & 63));
            asm("v_writelane_b32 %0, %1, %2" : "+v"(S.acce) : "s"(rve), "i"((u + 1) & 63));
        });
        if constexpr (DIRS) {
            dq[(2 * gi) * kWave] = dw[0];
            dq[(2 * gi + 1) * kWave] = dw[1];
        }
        // The best-cell updates hang off the cells' dependency chain and nothing in the
        // iteration waits for them: left alone, the compiler sinks all of them behind the
        // iteration and keeps every H of its 256 cells alive for that (512 registers and
        // scratch).  The group's updates are done here, and nothing moves across its end.
#pragma unroll
        for (int k = 0; k < C; ++k) asm volatile("" : "+v"(S.bv[k]), "+v"(S.bs[k]));
        __builtin_amdgcn_sched_barrier(0);
    });
}

// (nw_batch.hip uniform64)
__device__ __forceinline__ int64_t uniform64(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// The column profile of one strip (nw_batch_matrix.hip build_profile).
__device__ __forceinline__ void build_profile(const BatchMatrixArgs &MA, const uint32_t (&x)[C], uint32_t *pl) {
    static_assert(C == 4, "a profile dword holds the lane's four columns");
    constexpr int G = kLetters / 4;
    uint32_t r[C][G];
#pragma unroll
    for (int k = 0; k < C; ++k)
#pragma unroll
        for (int g = 0; g < G; ++g) r[k][g] = MA.score[x[k] * G + g];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const uint32_t a01l = __builtin_amdgcn_perm(r[1][g], r[0][g], 0x05010400u);  // r0b0 r1b0 r0b1 r1b1
        const uint32_t a01h = __builtin_amdgcn_perm(r[1][g], r[0][g], 0x07030602u);  // r0b2 r1b2 r0b3 r1b3
        const uint32_t a23l = __builtin_amdgcn_perm(r[3][g], r[2][g], 0x05010400u);
        const uint32_t a23h = __builtin_amdgcn_perm(r[3][g], r[2][g], 0x07030602u);
        pl[(4 * g + 0) * kWave] = __builtin_amdgcn_perm(a23l, a01l, 0x05040100u);  // r0b0 r1b0 r2b0 r3b0
        pl[(4 * g + 1) * kWave] = __builtin_amdgcn_perm(a23l, a01l, 0x07060302u);
        pl[(4 * g + 2) * kWave] = __builtin_amdgcn_perm(a23h, a01h, 0x05040100u);
        pl[(4 * g + 3) * kWave] = __builtin_amdgcn_perm(a23h, a01h, 0x07060302u);
    }
}

// a candidate (v, i, j) before the best (bv, bi, bj): score descending, row ascending,
// column ascending
__device__ __forceinline__ bool before(int32_t v, int32_t i, int32_t j, int32_t bv, int32_t bi, int32_t bj) {
    return v > bv || (v == bv && (i < bi || (i == bi && j < bj)));
}

// One pair (n1, n2 >= 1), all its strips, by this wave (nw_batch_matrix.hip matrix_pair);
// lane 0 writes the hit.
template <bool DIRS>
__device__ __forceinline__ void local_pair(const BatchMatrixArgs &MA, const uint8_t *__restrict__ s1, int32_t n1,
                                           const uint8_t *__restrict__ rowb, int32_t n2, int32_t *__restrict__ col,
                                           uint32_t *__restrict__ dirs, int32_t *hit, uint32_t *pl, int lane) {
    const BatchArgs &A = MA.a.b;
    const int32_t ge = A.gap, goe = MA.a.gap_open + A.gap;
    const int64_t eoff = MA.a.eoff;
    const int nstrips = (n1 + kCkptCols - 1) / kCkptCols;
    const int nblocks = n2 / 64 + 1;  // ceil((n2 + 1) / 64)
    const int lastb = nblocks - 1;
    int32_t pv = 0, pi = 0, pj = 0;  // this lane's best of the pair: 0 at (0, 0)

    for (int p = 0; p < nstrips; ++p) {
        const int32_t cl = 1 + p * kCkptCols + C * lane;  // first column of this lane
        LocalLane S;
        uint32_t x[C];  // the columns' letters (past n1: column n1's; those cells are dropped below)
#pragma unroll
        for (int k = 0; k < C; ++k) {
            x[k] = (uint32_t)MA.index[s1[min(cl + k, n1) - 1]];
            S.u[k] = 0;     // H[0][c]
            S.ho[k] = goe;
            S.f[k] = goe;   // F[0][c]: "minus infinity"
            S.bv[k] = 0;
            S.bs[k] = 0;
        }
        build_profile(MA, x, pl);
        S.e = goe;
        S.dg = 0;
        S.acch = S.acce = 0;
        const bool fed = p > 0;            // (strip 0 never reads the scratch)
        const bool pub = p + 1 < nstrips;  // (the last strip's right column has no reader)

        u32x4 pkc[4], pkn[4];
        load_rows(rowb, 0, lane, pkc);
        int32_t fnh = 0, fne = goe;  // H[i][0], E[i][0]
        if (fed) {
            fnh = col[lane];
            fne = col[eoff + lane];
        }
        // row 64*nblocks - 1 completes on lane 63 in iteration nblocks
        for (int it = 0; it <= nblocks; ++it) {
            if (it < nblocks) {
                S.fvh = fnh;
                S.fve = fne;
            }
            if (fed) {
                const int64_t xr = 64 * min(it + 1, lastb) + lane;
                fnh = col[xr];
                fne = col[eoff + xr];
            }
            load_rows(rowb, min(it + 1, nblocks), lane, pkn);
            const bool edge = it == 0 || 64 * it + 63 > n2;
            int32_t *colw = (pub && it >= 1) ? col + 64 * (it - 1) : nullptr;
            uint32_t *dq = nullptr;
            if constexpr (DIRS) dq = dirs + ((int64_t)p * (nblocks + 1) + it) * (32 * kWave);
            if (edge)
                local_iter<true, DIRS>(it, pkc, pl, ge, goe, n2, S, colw, eoff, dq, lane);
            else
                local_iter<false, DIRS>(it, pkc, pl, ge, goe, n2, S, colw, eoff, dq, lane);
#pragma unroll
            for (int h = 0; h < 4; ++h) pkc[h] = pkn[h];
        }
        // the strip's columns into the lane's best: real columns with a positive value
        // only (a column that never rose above 0 cannot beat 0 at (0, 0))
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const int32_t v = S.bv[k], i = S.bs[k] - lane, j = cl + k;
            if (j <= n1 && v > 0 && before(v, i, j, pv, pi, pj)) {
                pv = v;
                pi = i;
                pj = j;
            }
        }
    }
    // the 64 lanes' bests, once per pair
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
        const int32_t ov = __shfl_xor(pv, m), oi = __shfl_xor(pi, m), oj = __shfl_xor(pj, m);
        if (before(ov, oi, oj, pv, pi, pj)) {
            pv = ov;
            pi = oi;
            pj = oj;
        }
    }
    if (lane == 0) {
        hit[0] = pv;
        hit[1] = pi;
        hit[2] = pj;
        hit[3] = -1;  // (the walk writes the begin cell)
        hit[4] = -1;
        hit[5] = hit[6] = hit[7] = 0;
    }
}

// (nw_batch_matrix.hip claim_ticket_matrix: kept out of line for the same reason)
__device__ __noinline__ int claim_ticket_local(uint32_t *ticket) {
    uint32_t t = 0;
    if ((threadIdx.x & 63) == 0) t = atomicAdd(ticket, 1u);
    return (int)__builtin_amdgcn_readfirstlane(t);
}

// Persistent grid of one-wave workgroups; pairs claimed in order from the ticket.
template <bool DIRS>
__global__ __launch_bounds__(64) void nw_batch_local_sweep(BatchLocalArgs LA) {
    __shared__ uint32_t prof[kLetters * kWave];  // [row letter][lane], 8 KiB
    const BatchMatrixArgs &MA = LA.m;
    const BatchArgs &A = MA.a.b;
    const int lane = threadIdx.x;
    uint32_t *pl = prof + lane;
    int32_t *col = A.colscr + (int64_t)blockIdx.x * A.cstride;
    for (;;) {
        const int t = __builtin_amdgcn_readfirstlane(claim_ticket_local(A.ticket));  // (a call returns in a vector register)
        if (t >= A.npairs) break;
        int pair = t;
        if (A.order != nullptr) pair = __builtin_amdgcn_readfirstlane(A.order[t]);
        const int64_t o1 = uniform64(A.off1[pair]), o2 = uniform64(A.off2[pair]);
        const int64_t len1 = uniform64(A.off1[pair + 1]) - o1, len2 = uniform64(A.off2[pair + 1]) - o2;
        int32_t *hit = LA.hits + (int64_t)pair * kBatchLocalHitWords;
        if (len1 < 0 || len2 < 0 || len1 >= INT32_MAX || len2 > A.max_n2) {
            // not a pair this launch was sized for: the column scratch would not hold it
            if (lane < kBatchLocalHitWords) hit[lane] = lane == 0 ? INT32_MIN : lane < 5 ? -1 : 0;
        } else if (len1 == 0 || len2 == 0) {
            // no cells: 0 at (0, 0)
            if (lane < kBatchLocalHitWords) hit[lane] = (lane == 3 || lane == 4) ? -1 : 0;
        } else {
            const uint8_t *s1 = A.s1 + o1;
            const uint8_t *rowb = A.rows + kBatchRowPad + o2 - 1;  // rowb[y] = row y's letter
            uint32_t *dirs = nullptr;
            if constexpr (DIRS) dirs = (uint32_t *)(A.dirs + uniform64(A.dir_off[t])) + lane;
            local_pair<DIRS>(MA, s1, (int32_t)len1, rowb, (int32_t)len2, col, dirs, hit, pl, lane);
        }
    }
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
// into the pair's slot; nw_batch_local_reverse turns them round.
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
        const int64_t cj = c - 1;
        const int64_t p = cj >> 8, l = (cj & 255) >> 2, k = cj & 3;
        const int64_t s = r + l;
        const int64_t idx =
            ((((p * iters + (s >> 6)) * 16 + ((s & 63) >> 2)) * 2 + ((s & 3) >> 1)) * 64 + l) * 4 + (s & 1) * 2 + (k >> 1);
        const uint32_t bits = ((uint32_t)d[idx] >> (4 * (k & 1))) & 15u;
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

// ops of ticket blockIdx.x into begin -> end order (nw_batch.hip nw_batch_reverse)
__global__ __launch_bounds__(64) void nw_batch_local_reverse(BatchLocalWalkArgs LW) {
    const BatchWalkArgs &W = LW.w;
    const int t = blockIdx.x;
    uint8_t *ops = W.ops + W.ops_off[t];
    const int64_t n = W.n_ops[t];
    for (int64_t a = threadIdx.x; a < n / 2; a += 64) {
        const uint8_t x = ops[a], y = ops[n - 1 - a];
        ops[a] = y;
        ops[n - 1 - a] = x;
    }
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
    hipLaunchKernelGGL(nw_batch_local_reverse, dim3((unsigned)w.w.npairs), dim3(64), 0, (hipStream_t)stream, w);
    return (int)hipGetLastError();
}

}  // namespace nw
