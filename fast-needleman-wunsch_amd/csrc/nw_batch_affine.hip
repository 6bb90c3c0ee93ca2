// nw_batch_affine.hip -- gfx950 (MI355X) batched pairwise alignment under affine gap
// cost (Gotoh): a run of L ups or of L lefts costs gap_open + L * gap_extend,
// gap_extend = nw_params.gap.  The decomposition is nw_batch.hip's: a persistent grid
// of one-wave workgroups claims pairs from the ticket, a worker computes its pair's
// whole table alone in 256-column strips, lane l owns columns 4l .. 4l+3 and at step s
// computes row s - l, lanes outside rows 1..n2 hold their cells (EDGE), the
// substitution by v_perm score tables or byte compares, chosen from nprof.
//
// The cell holds three values, all with ge*(i+j) subtracted (the w form; go =
// gap_open, ge = gap_extend):
//     E' = max(E'_left, H'_left + go)          a left run ending at the cell
//     F' = max(F'_up,   H'_up   + go)          an up run ending at the cell
//     H' = max(H'_diag + s - 2ge, F', E')
//     H'[0][0] = 0, H'[0][j>=1] = H'[i>=1][0] = go, E'[i][0] = F'[0][j] = -2^29
// The table bytes are s - 2ge as in the linear kernel.  F is lane-local (four values);
// H and E of a lane's last column go to the right neighbour over DPP wave_shr:1, two
// moves per step.  The -2^29 is never added to, and every real value stays above
// -2^28 (the host's affine_range_ok), so it loses every maximum it enters.
//
// Strip to strip, BOTH H' and E' of the right column are gathered (lane x holds row
// 64b + x) and go to the worker's column scratch -- two 256-byte stores per 64 steps,
// H at col[row], E at col[eoff + row] -- from where the same lanes load them back as
// strip p + 1's feed.  Strip 0 takes the boundary and never reads the scratch.
//
// The DIRECTIONS kernel writes 4 bits per cell: bits 0-1 the H choice (0 diag, 1 F, 2
// E: the first in that order that equals H'), bit 2 "E extended" (E'_left > H'_left +
// go: opening wins a tie), bit 3 "F extended".  A lane's four cells of a step are 16
// bits, four steps two dwords, stored [strip][iteration][step / 4][step % 4 / 2][lane]:
// every store instruction writes 256 contiguous bytes.  nw_batch_affine_walk inverts
// that mapping, one thread per pair.
//
// nw_batch_matrix.hip and nw_batch_local.hip run this decomposition from one skeleton
// (nw_batch_dev.h sweep_tickets / sweep_pair / sweep_iter).  This file's sweep is NOT on
// it: on the skeleton the score kernel came out 0.7 % slower at 8000 x 8000, from an ISA
// that differed in a few swapped instructions, so affine_iter, affine_pair and the
// ticket loop stand here in their own text and compile to the ISA they had before the
// skeleton existed.  From that header come load_rows, uniform64, claim_ticket and the
// index of a cell's direction bits (NW_DIR_NIBBLE); the reversal is nw_batch.hip's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nw_batch_dev.h"

namespace nw {
namespace {

struct AffineLane {
    int32_t u[C];     // H' of the lane's current row, column k
    int32_t f[C];     // F' of the lane's current row, column k
    int32_t e;        // E' of the lane's current row, last column
    int32_t dg;       // H'_diag of column 0 for the next step
    uint32_t apk;     // raw column characters, byte k = column k
    uint32_t tlo[C];  // SUB_PERM score tables
    uint32_t thi[C];
    int32_t fvh, fve;  // feed: lane x holds H' / E' of the left strip's right column at row 64it + x
    int32_t acch, acce;  // right column gathered: lane x holds row 64(it-1) + x
};

// 64 steps of iteration `it` (steps 64it + u): lane l computes row 64it + u - l.
//   EDGE : some lane's row is outside 1..n2 in this iteration (it holds its cells)
//   colw : where H' of the right column of block it - 1 goes, E' eoff words behind it
//          (NULL: it has no reader)
//   dq   : DIRS: this lane's first dword of the iteration's first 4-step group
template <int MODE, bool EDGE, bool DIRS>
__device__ __forceinline__ void affine_iter(int it, const u32x4 (&pk)[4], int32_t msp, int32_t mmp, int32_t go,
                                            int32_t n2, AffineLane &S, int32_t *colw, int64_t eoff, uint32_t *dq,
                                            int lane) {
    int32_t rr = 64 * it - lane - 1;  // EDGE: row of this lane before the step
    static_for<0, 16>([&](auto gc) {
        constexpr int gi = decltype(gc)::value;
        const uint32_t word = pk[gi >> 2][gi & 3];  // row characters of steps 4gi .. 4gi+3
        uint32_t sc[C];
        if constexpr (MODE == SUB_PERM) {
#pragma unroll
            for (int k = 0; k < C; ++k) sc[k] = __builtin_amdgcn_perm(S.thi[k], S.tlo[k], word);
        }
        uint32_t dw[2] = {0, 0};  // DIRS: 4 bits per cell, dword h halfword q & 1 = step 4gi + q, nibble k = column k
        static_for<0, 4>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            constexpr int u = 4 * gi + q;
            const int32_t lfh = __builtin_amdgcn_readlane(S.fvh, u);
            const int32_t lfe = __builtin_amdgcn_readlane(S.fve, u);
            int32_t left = __builtin_amdgcn_update_dpp(lfh, S.u[C - 1], 0x138 /*wave_shr:1*/, 0xF, 0xF, false);
            int32_t el = __builtin_amdgcn_update_dpp(lfe, S.e, 0x138 /*wave_shr:1*/, 0xF, 0xF, false);
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
                const int32_t fo = up + go, eo = left + go;  // a run opened from H'
                const int32_t f = max(S.f[k], fo);
                const int32_t e = max(el, eo);
                // H' = max(H'_diag + s - 2 ge, F', E')
                int32_t x = max(max(d, f), e);
                if constexpr (DIRS) {
                    uint32_t code = x == d ? 0u : x == f ? 1u : 2u;
                    code |= el > eo ? 4u : 0u;
                    code |= S.f[k] > fo ? 8u : 0u;
                    dw[q >> 1] |= code << (16 * (q & 1) + 4 * k);
                }
                diag = up;
                if constexpr (EDGE) {
                    x = act ? x : up;
                    S.f[k] = act ? f : S.f[k];
                } else {
                    S.f[k] = f;
                }
                S.u[k] = x;
                left = x;
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
                // rows 64(it-1) .. + 63 are gathered (lane 0 since the step before this
                // iteration): out, before lane 0 takes row 64it
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
    });
}

// One pair (n1, n2 >= 1), all its strips, by this wave.  s1: the pair's column
// characters; rowb[y] = row y's character; col: the worker's column scratch (H' at
// col[row], E' at col[eoff + row]); dirs: DIRS: this lane's first dword of the pair's
// first 4-step group.
template <int MODE, bool DIRS>
__device__ __forceinline__ void affine_pair(const BatchAffineArgs &AA, const uint8_t *__restrict__ s1, int32_t n1,
                                            const uint8_t *__restrict__ rowb, int32_t n2, int32_t *__restrict__ col,
                                            uint32_t *__restrict__ dirs, int32_t *score, int lane) {
    const BatchArgs &A = AA.b;
    const int32_t ge = A.gap, go = AA.gap_open;
    const int64_t eoff = AA.eoff;
    const int32_t msp = A.match - 2 * ge, mmp = A.mismatch - 2 * ge;
    const int nstrips = (n1 + kCkptCols - 1) / kCkptCols;
    const int nblocks = n2 / 64 + 1;  // ceil((n2 + 1) / 64)
    const int lastb = nblocks - 1;

    for (int p = 0; p < nstrips; ++p) {
        const int32_t cl = 1 + p * kCkptCols + C * lane;  // first column of this lane
        AffineLane S;
        S.apk = 0;
        // SUB_PERM tables: T_k[x] = s(a_k, chars[x]) - 2*ge (nw_strips.h compute_strip)
        const uint32_t mmb = ((uint32_t)mmp & 255u) * 0x01010101u;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const int32_t c = cl + k;
            const uint32_t a = c <= n1 ? (uint32_t)s1[c - 1] : 0u;
            S.apk |= a << (8 * k);
            S.u[k] = go;       // H'[0][c] = go + c*ge - ge*c
            S.f[k] = kNegInf;  // F'[0][c]
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
        S.e = kNegInf;
        S.dg = go;
        S.acch = S.acce = 0;
        const bool fed = p > 0;            // (strip 0 never reads the scratch)
        const bool pub = p + 1 < nstrips;  // (the last strip's right column has no reader)

        // row words and the feed are loaded one iteration ahead.  Strip 0: the boundary
        // column, H'[r][0] = go but H'[0][0] = 0 (the diagonal of cell (1, 1)), E'[r][0] =
        // -inf
        u32x4 pkc[4], pkn[4];
        load_rows(rowb, 0, lane, pkc);
        int32_t fnh = lane == 0 ? 0 : go, fne = kNegInf;
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
            // block it + 1 was stored by the strip before; this strip's own stores are
            // at block it - 1 and below
            if (fed) {
                const int64_t x = 64 * min(it + 1, lastb) + lane;
                fnh = col[x];
                fne = col[eoff + x];
            } else {
                fnh = go;
            }
            load_rows(rowb, min(it + 1, nblocks), lane, pkn);
            const bool edge = it == 0 || 64 * it + 63 > n2;
            int32_t *colw = (pub && it >= 1) ? col + 64 * (it - 1) : nullptr;
            uint32_t *dq = nullptr;
            if constexpr (DIRS) dq = dirs + ((int64_t)p * (nblocks + 1) + it) * (32 * kWave);
            if (edge)
                affine_iter<MODE, true, DIRS>(it, pkc, msp, mmp, go, n2, S, colw, eoff, dq, lane);
            else
                affine_iter<MODE, false, DIRS>(it, pkc, msp, mmp, go, n2, S, colw, eoff, dq, lane);
#pragma unroll
            for (int h = 0; h < 4; ++h) pkc[h] = pkn[h];
        }
        // every lane now holds row n2 of its columns
        if (p == nstrips - 1) {
#pragma unroll
            for (int k = 0; k < C; ++k)
                if (cl + k == n1) *score = S.u[k] + ge * (n2 + n1);
        }
    }
}

// Persistent grid of one-wave workgroups; pairs claimed in order from the ticket.
template <bool DIRS>
__global__ __launch_bounds__(64) void nw_batch_affine_sweep(BatchAffineArgs AA) {
    const BatchArgs &A = AA.b;
    const int lane = threadIdx.x;
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
            // no cells: the corner of the boundary, one gap (none for 0 x 0)
            const int32_t n = (int32_t)max(len1, len2);
            if (lane == 0) *score = n > 0 ? AA.gap_open + A.gap * n : 0;
        } else {
            const uint8_t *s1 = A.s1 + o1;
            const uint8_t *rowb = A.rows + kBatchRowPad + o2 - 1;  // rowb[y] = row y's character
            uint32_t *dirs = nullptr;
            if constexpr (DIRS) dirs = (uint32_t *)(A.dirs + uniform64(A.dir_off[t])) + lane;
            if (perm)
                affine_pair<SUB_PERM, DIRS>(AA, s1, (int32_t)len1, rowb, (int32_t)len2, col, dirs, score, lane);
            else
                affine_pair<SUB_GEN, DIRS>(AA, s1, (int32_t)len1, rowb, (int32_t)len2, col, dirs, score, lane);
        }
    }
}

// The walk of ticket t's pair from (n2, n1) to (0, 0): one thread per pair, a machine
// of three states.  Cell (i, j) was computed in strip p = (j-1) / 256 by lane l =
// ((j-1) % 256) / 4, column k = (j-1) % 4, at step s = i + l: its four bits are nibble
// k % 2 of byte (s % 2) * 2 + k / 2 of dword [p][s / 64][s % 64 / 4][s % 4 / 2][l].
//   H, on the boundary: row 0 is walked left and column 0 up without reading bits
//   H, inner cell: bits 0-1: 0 emits a diag; 1 / 2 switch to F / E and emit nothing
//   F: emits an up and moves; bit 3 of the cell it left: 1 stays in F, 0 returns to H
//   E: emits a left and moves; bit 2 likewise
// F and E are entered at inner cells only and return to H at the latest when the run
// reaches row 1 / column 1, where it can only have been opened.  Ops go end -> begin
// into the pair's slot; nw_batch_reverse turns them round.
__global__ __launch_bounds__(64) void nw_batch_affine_walk(BatchWalkArgs W) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= W.npairs) return;
    const int pair = W.order != nullptr ? W.order[t] : t;
    int64_t c = W.off1[pair + 1] - W.off1[pair], r = W.off2[pair + 1] - W.off2[pair];
    const int64_t iters = batch_iters(r);
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
        NW_DIR_NIBBLE(bits, d, iters, r, c);
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

int launch_batch_affine(const BatchAffineArgs &a, bool dirs, int grid, void *stream) {
    if (dirs)
        hipLaunchKernelGGL(nw_batch_affine_sweep<true>, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(nw_batch_affine_sweep<false>, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_batch_affine_walk(const BatchWalkArgs &w, void *stream) {
    hipLaunchKernelGGL(nw_batch_affine_walk, dim3((unsigned)((w.npairs + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                       w);
    return launch_batch_reverse(w, stream);
}

}  // namespace nw
