// nw_batch.hip -- gfx950 (MI355X) batched pairwise alignment: many small pairs in one
// launch.  The cell is the checkpoint sweep's (nw_ckpt.hip): w = t - GAP*(i+j), lane
// l owns columns 4l .. 4l+3 of a 256-column strip and at step s computes row s - l,
// the left neighbour over DPP wave_shr:1, the substitution by v_perm score tables
// or byte compares (nw_strips.h diag_plus_sub), chosen on the device from nprof,
// lanes outside rows 1..n2 holding their cells (EDGE).
//
// What differs is the decomposition.  A workgroup is ONE wave; a persistent grid of
// them claims PAIRS from the ticket (longest first: BatchArgs::order) and a worker
// computes its pair's whole table alone, strip after strip.  So nothing is handed
// from wave to wave: the right column of strip p is gathered as in the sweep (lane x
// holds row 64b + x) and goes to the worker's own column scratch in device memory --
// one plain 256-byte store per 64 steps -- from where the same lane loads it back as
// strip p + 1's feed.  No tag, no wait, no watchdog: the only operation between
// waves is the ticket's atomicAdd.  Strip 0 takes the boundary column (w = 0) and
// never reads the scratch, which still holds the previous pair's column.
//
// Two instantiations: the SCORE kernel writes scores[pair] = t[n2][n1] and nothing
// else; the DIRECTIONS kernel also writes 2 bits per cell -- 0 diag, 1 up, 2 left, the
// first in that order that reproduces the w-form maximum, which is nw_traceback's
// tie-break since the w-form comparisons are the t-form ones -- packed four cells of
// a lane's step into a byte and four steps into a dword, stored step-major
// ([strip][step / 4][lane]): every store instruction writes 256 contiguous bytes.
// nw_batch_walk inverts that mapping, one thread per pair.
//
// load_rows, uniform64 and claim_ticket are nw_batch_dev.h's, shared with the affine
// family's files; the sweep itself is this file's own (one value per column, 2 bits per
// cell, no E and no F: that header's skeleton does not fit it).  nw_batch_reverse, here,
// serves every walk of the batch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "nw_batch_dev.h"  // (load_rows, uniform64, claim_ticket; nw_strips.h diag_plus_sub)

namespace nw {
namespace {

struct BatchLane {
    int32_t u[C];     // w of the lane's current row, column k
    int32_t dg;       // w_diag of column 0 for the next step
    uint32_t apk;     // raw column characters, byte k = column k
    uint32_t tlo[C];  // SUB_PERM score tables
    uint32_t thi[C];
    int32_t fv;       // feed: lane x holds the left strip's right column at row 64it + x
    int32_t acc;      // right column gathered: lane x holds row 64(it-1) + x
};

// 64 steps of iteration `it` (steps 64it + u): lane l computes row 64it + u - l.
//   EDGE : some lane's row is outside 1..n2 in this iteration (it holds its cells)
//   colw : where the right column of block it - 1 goes (NULL: it has no reader)
//   dq   : DIRS: this lane's dword of the iteration's first 4-step group
template <int MODE, bool EDGE, bool DIRS>
__device__ __forceinline__ void batch_iter(int it, const u32x4 (&pk)[4], int32_t msp, int32_t mmp, int32_t n2,
                                           BatchLane &S, int32_t *colw, uint32_t *dq, int lane) {
    int32_t rr = 64 * it - lane - 1;  // EDGE: row of this lane before the step
    static_for<0, 16>([&](auto gc) {
        constexpr int gi = decltype(gc)::value;
        const uint32_t word = pk[gi >> 2][gi & 3];  // row characters of steps 4gi .. 4gi+3
        uint32_t sc[C];
        if constexpr (MODE == SUB_PERM) {
#pragma unroll
            for (int k = 0; k < C; ++k) sc[k] = __builtin_amdgcn_perm(S.thi[k], S.tlo[k], word);
        }
        uint32_t dw = 0;  // DIRS: 2 bits per cell, byte q = step 4gi + q, bits 2k = column k
        static_for<0, 4>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            constexpr int u = 4 * gi + q;
            const int32_t lf = __builtin_amdgcn_readlane(S.fv, u);
            int32_t left = __builtin_amdgcn_update_dpp(lf, S.u[C - 1], 0x138 /*wave_shr:1*/, 0xF, 0xF, false);
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
                const uint32_t w = MODE == SUB_PERM ? sc[k] : word;
                const int32_t d = diag_plus_sub<q, k, MODE>(w, S.apk, diag, msp, mmp);
                const int32_t up = S.u[k];
                // w = max(w_diag + s - 2 GAP, w_up, w_left)
                int32_t x = max(max(d, up), left);
                if constexpr (DIRS) {
                    const uint32_t code = x == d ? 0u : x == up ? 1u : 2u;
                    dw |= code << (8 * q + 2 * k);
                }
                diag = up;
                if constexpr (EDGE) x = act ? x : up;
                S.u[k] = x;
                left = x;
            });
            // lane 63 is on row 64(it-1) + u + 1: into lane (u + 1) % 64 of the gather
            const int32_t rv = __builtin_amdgcn_readlane(S.u[C - 1], 63);
            if constexpr (u == 63) {
                // rows 64(it-1) .. + 63 are gathered (lane 0 since the step before this
                // iteration): out, before lane 0 takes row 64it
                if (colw != nullptr) colw[lane] = S.acc;
            }
            asm("v_writelane_b32 %0, %1, %2" : "+v"(S.acc) : "s"(rv), "i"((u + 1) & 63));
        });
        if constexpr (DIRS) dq[gi * kWave] = dw;
    });
}

// One pair (n1, n2 >= 1), all its strips, by this wave.  s1: the pair's column
// characters; rowb[y] = row y's character; col: the worker's column scratch; dirs:
// DIRS: this lane's dword of the pair's first 4-step group.
template <int MODE, bool DIRS>
__device__ __forceinline__ void batch_pair(const BatchArgs &A, const uint8_t *__restrict__ s1, int32_t n1,
                                           const uint8_t *__restrict__ rowb, int32_t n2, int32_t *__restrict__ col,
                                           uint32_t *__restrict__ dirs, int32_t *score, int lane) {
    const int32_t gap = A.gap;
    const int32_t msp = A.match - 2 * gap, mmp = A.mismatch - 2 * gap;
    const int nstrips = (n1 + kCkptCols - 1) / kCkptCols;
    const int nblocks = n2 / 64 + 1;  // ceil((n2 + 1) / 64)
    const int lastb = nblocks - 1;

    for (int p = 0; p < nstrips; ++p) {
        const int32_t cl = 1 + p * kCkptCols + C * lane;  // first column of this lane
        BatchLane S;
        S.apk = 0;
        // SUB_PERM tables: T_k[x] = s(a_k, chars[x]) - 2*GAP (nw_strips.h compute_strip)
        const uint32_t mmb = ((uint32_t)mmp & 255u) * 0x01010101u;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const int32_t c = cl + k;
            const uint32_t a = c <= n1 ? (uint32_t)s1[c - 1] : 0u;
            S.apk |= a << (8 * k);
            S.u[k] = 0;  // w[0][c] = t[0][c] - GAP*c = 0
            if constexpr (MODE == SUB_PERM) {
                const uint32_t x = c <= n1 ? (uint32_t)A.charmap[a] : 0xFFu;
                const uint32_t msb = (uint32_t)msp & 255u;
                const uint32_t sh = 8u * (x & 3u), keep = ~(255u << sh), put = msb << sh;
                S.tlo[k] = x < 4u ? ((mmb & keep) | put) : mmb;
                S.thi[k] = (x >= 4u && x < 8u) ? ((mmb & keep) | put) : mmb;
            } else {
                S.tlo[k] = S.thi[k] = 0u;
            }
        }
        S.dg = 0;
        S.fv = 0;  // strip 0: the boundary column, w[r][0] = t[r][0] - GAP*r = 0
        S.acc = 0;
        const bool fed = p > 0;            // (strip 0 never reads the scratch)
        const bool pub = p + 1 < nstrips;  // (the last strip's right column has no reader)

        // row words and the feed are loaded one iteration ahead
        u32x4 pkc[4], pkn[4];
        load_rows(rowb, 0, lane, pkc);
        int32_t fn = 0;
        if (fed) fn = col[lane];
        // row 64*nblocks - 1 completes on lane 63 in iteration nblocks
        for (int it = 0; it <= nblocks; ++it) {
            if (it < nblocks) S.fv = fn;
            // block it + 1 was stored by the strip before; this strip's own stores are
            // at block it - 1 and below
            if (fed) fn = col[64 * min(it + 1, lastb) + lane];
            load_rows(rowb, min(it + 1, nblocks), lane, pkn);
            const bool edge = it == 0 || 64 * it + 63 > n2;
            int32_t *colw = (pub && it >= 1) ? col + 64 * (it - 1) : nullptr;
            uint32_t *dq = nullptr;
            if constexpr (DIRS) dq = dirs + ((int64_t)p * (nblocks + 1) + it) * (16 * kWave);
            if (edge)
                batch_iter<MODE, true, DIRS>(it, pkc, msp, mmp, n2, S, colw, dq, lane);
            else
                batch_iter<MODE, false, DIRS>(it, pkc, msp, mmp, n2, S, colw, dq, lane);
#pragma unroll
            for (int h = 0; h < 4; ++h) pkc[h] = pkn[h];
        }
        // every lane now holds row n2 of its columns
        if (p == nstrips - 1) {
#pragma unroll
            for (int k = 0; k < C; ++k)
                if (cl + k == n1) *score = S.u[k] + gap * (n2 + n1);
        }
    }
}

// Persistent grid of one-wave workgroups; pairs claimed in order from the ticket.
template <bool DIRS>
__global__ __launch_bounds__(64) void nw_batch_sweep(BatchArgs A) {
    const int lane = threadIdx.x;
    // table form when the launch allows it and the batch's s1 holds at most kMaxPerm
    // distinct characters (nw_charmap over the concatenation), else compares
    const uint32_t np = __builtin_amdgcn_readfirstlane(ctrl_load(A.nprof));
    const bool perm = A.perm != 0 && np <= kMaxPerm;
    int32_t *col = A.colscr + (int64_t)blockIdx.x * A.cstride;
    for (;;) {
        const int t = __builtin_amdgcn_readfirstlane(claim_ticket(A.ticket));  // (a call returns in a vector register)
        if (t >= A.npairs) break;
        int pair = t;
        if (A.order != nullptr) pair = __builtin_amdgcn_readfirstlane(A.order[t]);
        const int64_t o1 = uniform64(A.off1[pair]), o2 = uniform64(A.off2[pair]);
        const int64_t len1 = uniform64(A.off1[pair + 1]) - o1, len2 = uniform64(A.off2[pair + 1]) - o2;
        int32_t *score = A.scores + pair;
        if (len1 < 0 || len2 < 0 || len1 >= INT32_MAX || len2 > A.max_n2) {
            // not a pair this launch was sized for: the column scratch would not hold it
            if (lane == 0) *score = INT32_MIN;
        } else if (len1 == 0 || len2 == 0) {
            // no cells: the corner of the boundary
            if (lane == 0) *score = A.gap * (int32_t)max(len1, len2);
        } else {
            const uint8_t *s1 = A.s1 + o1;
            const uint8_t *rowb = A.rows + kBatchRowPad + o2 - 1;  // rowb[y] = row y's character
            uint32_t *dirs = nullptr;
            if constexpr (DIRS) dirs = (uint32_t *)(A.dirs + uniform64(A.dir_off[t])) + lane;
            if (perm)
                batch_pair<SUB_PERM, DIRS>(A, s1, (int32_t)len1, rowb, (int32_t)len2, col, dirs, score, lane);
            else
                batch_pair<SUB_GEN, DIRS>(A, s1, (int32_t)len1, rowb, (int32_t)len2, col, dirs, score, lane);
        }
    }
}

// The batch's row characters: d_rows[kBatchRowPad + i] = s2cat[i], raw, or -- with
// `perm` and at most kMaxPerm distinct column characters -- mapped: charmap[b], 7 for
// a character in no column (the SUB_PERM selector bytes, as nw_rowpack's).  The pads
// are zeroed.
__global__ __launch_bounds__(256) void nw_batch_rows(const uint8_t *__restrict__ s2, int64_t total2,
                                                     const uint8_t *__restrict__ charmap,
                                                     const uint32_t *__restrict__ nprof, int32_t perm,
                                                     uint8_t *__restrict__ rows) {
    const bool map = perm != 0 && *nprof <= kMaxPerm;
    const int64_t len = kBatchRowPad + total2 + kBatchRowTail;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < len; x += stride) {
        const int64_t i = x - kBatchRowPad;
        uint32_t b = 0;
        if (i >= 0 && i < total2) {
            b = s2[i];
            if (map) b = min((uint32_t)charmap[b], 7u);
        }
        rows[x] = (uint8_t)b;
    }
}

// The walk of ticket t's pair from (n2, n1) to (0, 0): one thread per pair.  Cell (i,
// j) was computed in strip p = (j-1) / 256 by lane l = ((j-1) % 256) / 4, column k =
// (j-1) % 4, at step s = i + l: its two bits sit in byte s % 4 of dword [p][s / 4][l].
// Row 0 is walked left and column 0 up without reading bits, as nw_traceback does.
// Ops go end -> begin into the pair's slot; nw_batch_reverse turns them round.  Each
// step waits for one byte whose address the step before decided: latency-bound.
__global__ __launch_bounds__(64) void nw_batch_walk(BatchWalkArgs W) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= W.npairs) return;
    const int pair = W.order != nullptr ? W.order[t] : t;
    int64_t c = W.off1[pair + 1] - W.off1[pair], r = W.off2[pair + 1] - W.off2[pair];
    const int64_t iters = batch_iters(r);
    const uint8_t *d = W.dirs + W.dir_off[t];
    uint8_t *ops = W.ops + W.ops_off[t];
    int64_t n = 0;
    while (r > 0 || c > 0) {
        uint32_t op;
        if (r == 0) {
            op = 2;
        } else if (c == 0) {
            op = 1;
        } else {
            const int64_t cj = c - 1;
            const int64_t p = cj >> 8, l = (cj & 255) >> 2, k = cj & 3;
            const int64_t s = r + l;
            const int64_t idx = ((p * iters + (s >> 6)) * 16 + ((s & 63) >> 2)) * 256 + l * 4 + (s & 3);
            op = ((uint32_t)d[idx] >> (2 * k)) & 3u;
        }
        ops[n++] = (uint8_t)op;
        r -= op != 2u;
        c -= op != 1u;
    }
    W.n_ops[t] = n;
}

// ops of ticket blockIdx.x into begin -> end order: after any of the batch's walks
// (launch_batch_reverse)
__global__ __launch_bounds__(64) void nw_batch_reverse(BatchWalkArgs W) {
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

int launch_batch_rows(const uint8_t *d_s2, int64_t total2, int32_t perm, const uint8_t *meta, uint8_t *d_rows,
                      void *stream) {
    const int64_t len = kBatchRowPad + total2 + kBatchRowTail;
    const int64_t g = std::min<int64_t>(4096, (len + 255) / 256);
    hipLaunchKernelGGL(nw_batch_rows, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, d_s2, total2, meta,
                       (const uint32_t *)(meta + 256), perm, d_rows);
    return (int)hipGetLastError();
}

int launch_batch(const BatchArgs &a, bool dirs, int grid, void *stream) {
    if (dirs)
        hipLaunchKernelGGL(nw_batch_sweep<true>, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(nw_batch_sweep<false>, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_batch_reverse(const BatchWalkArgs &w, void *stream) {
    hipLaunchKernelGGL(nw_batch_reverse, dim3((unsigned)w.npairs), dim3(64), 0, (hipStream_t)stream, w);
    return (int)hipGetLastError();
}

int launch_batch_walk(const BatchWalkArgs &w, void *stream) {
    hipLaunchKernelGGL(nw_batch_walk, dim3((unsigned)((w.npairs + 63) / 64)), dim3(64), 0, (hipStream_t)stream, w);
    return launch_batch_reverse(w, stream);
}

}  // namespace nw
