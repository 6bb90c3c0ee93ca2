// nw_batch_dev.h -- device code shared by the batch kernels' files (nw_batch.hip,
// nw_batch_affine.hip, nw_batch_matrix.hip, nw_batch_local.hip, nw_batch_semi.hip,
// nw_batch_banded.hip, which runs sweep_tickets and sweep_iter under its own pair loop, and
// the two two-piece files nw_batch_dual.hip and nw_batch_dual_banded.hip, which run
// sweep_tickets and ProfileSub under their own pair loops, share their iteration and walk
// through nw_batch_dual_dev.h and find their cells' direction bytes by dual_dir_byte and
// dual_banded_dir_byte).  Private to them: every file compiles its own copy (no relocatable
// device code), so everything here is in the unnamed namespace.
//
// For all of them: load_rows, uniform64, claim_ticket.  For the affine family (all but the
// linear file, which carry H and E from column to column): the index of a cell's direction
// bits (NW_DIR_NIBBLE), used by the three walks over 4 bits per cell; and, for
// nw_batch_matrix.hip, nw_batch_local.hip and nw_batch_semi.hip, build_profile, ProfileSub
// and the sweep skeleton -- sweep_tickets, sweep_pair, sweep_iter -- which a file
// instantiates with its cell policy; for nw_batch_matrix.hip and nw_batch_semi.hip the
// global cell in the w form (GlobalCell, GlobalSweep, MatrixCell); for nw_batch_local.hip and
// nw_batch_semi.hip the order of their candidate cells (before); for a banded pair loop the
// range of a strip, its "inside" test and the feed's mask (BandRange: nw_batch_dual_banded.hip
// uses it, nw_batch_banded.hip keeps the text it was measured with).  The linear kernel
// keeps its own sweep (one value per column, 2 bits per cell, no E and no F) and so does
// the affine kernel (nw_batch_affine.hip says why).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nw_batch.h"
#include "nw_dev.h"
#include "nw_internal.h"
#include "nw_strips.h"  // (diag_plus_sub, u32x4)

namespace nw {
namespace {

constexpr int C = kCkptC;
constexpr int32_t kNegInf = -(1 << 29);
constexpr int kLetters = kBatchMatrixLetters;

// Row characters of iteration j: lane l needs the bytes of rows 64j - l + u, u < 64
// (rowb[y] = row y's character).  The four 16-byte loads are unaligned.
__device__ __forceinline__ void load_rows(const uint8_t *__restrict__ rowb, int j, int lane, u32x4 (&pk)[4]) {
    const uint8_t *b = rowb + (int64_t)j * 64 - lane;
#pragma unroll
    for (int h = 0; h < 4; ++h) __builtin_memcpy(&pk[h], b + 16 * h, 16);
}

// A value every lane holds alike, moved to scalar registers: the pair's offsets and
// lengths are loaded with vector loads (the arrays are not known to be read-only),
// and loop bounds left in vector registers would make every loop of the sweep a
// divergent one.
__device__ __forceinline__ int64_t uniform64(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// The next ticket, in every lane.  Kept out of line: inlined into the ticket loop,
// `lane == 0` is a loop invariant and the optimiser unswitches the loop on it; the
// copy for the other lanes then runs beside lane 0's with a constant ticket 0 (in the
// ISA: a second loop that loads order[0]; on the device: now and then a wrong score
// for the pair of ticket 0).  A call is opaque to that.
__device__ __noinline__ int claim_ticket(uint32_t *ticket) {
    uint32_t t = 0;
    if ((threadIdx.x & 63) == 0) t = atomicAdd(ticket, 1u);
    return (int)__builtin_amdgcn_readfirstlane(t);
}

// The column profile of one strip: pl[y * 64] for every y < 32 (rows at or beyond n hold
// the zeros the host put there; nobody reads them).  Row x of the matrix is 8 dwords
// (byte b of dword g: row letter 4g + b); the lane's four rows are loaded whole -- all
// loads in flight together: the build is once per strip, and a strip of a short pair is
// a few thousand cycles -- and transposed 4 x 4 bytes at a time with v_perm (selector
// 0-3: a byte of the second operand, 4-7: of the first).
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

// ---- the matrix and local sweeps: cell policies ----
//
// A cell policy P is the lane's state of one pair.  The skeleton below reads and writes
// the GotohLane part itself and asks the policy for what differs between the kernels:
//   P(M, out, lane)                per pair; M is the kernel's Sweep (below), out the pair's result
//   strip_begin(s1, n1, cl)        u, f, e, dg of row 0 and the strip's substitution data
//   boundary_h(corner), boundary_e()   column 0, which strip 0 is fed instead of the scratch
//   iter_begin(pk), group_begin<gi>(pk)   substitution data of a 4-step group
//   diag_sub<q, k>(diag)           diag + the cell's substitution score
//   opening(left)                  what the left neighbour's H offers a cell as `lh`
//   cell<k, SH, EDGE, DIRS>(d, diag, lh, el, act, step, bits)   the cell: updates u[k], f[k]
//                                  and the three carried values; DIRS: its 4 direction bits
//                                  into `bits` at bit SH
//   group_end()                    after the group's stores
//   strip_end(last, cl, n1, n2), pair_end()   the results
// and the kernel's Sweep M for
//   affine()                       the BatchAffineArgs of the launch
//   result(pair)                   where the pair's result goes
//   refused(out, lane), empty(out, n, lane)   results of pairs that have no sweep
//   pair<DIRS>(...)                picks the policy's variant and calls sweep_pair

struct GotohLane {
    int32_t u[C];        // H of the lane's current row, column k
    int32_t f[C];        // F of the lane's current row, column k
    int32_t e;           // E of the lane's current row, last column
    int32_t dg;          // H_diag of column 0 for the next step
    int32_t fvh, fve;    // feed: lane x holds H / E of the left strip's right column at row 64it + x
    int32_t acch, acce;  // right column gathered: lane x holds row 64(it-1) + x
};

// Substitution by the lane's column profile in LDS (nw_batch_matrix.hip's header): pl is
// this lane's dword of profile row 0.  The profile dwords of a group are read one group
// ahead of their use: a ds_read_b32 takes some 50 cycles to return, and one wave per SIMD
// has nothing else to run.
struct ProfileSub {
    uint32_t *pl;
    uint32_t sc[4];  // step q (row letter: byte q of the row word): byte k = the score byte of column k
    uint32_t scn[4];

    // The columns' letters (past n1: column n1's, cells nobody reads; no branch, so the
    // four loads and the four lookups overlap) and this strip's profile over the last
    // strip's (or the last pair's): the reads of those are before this point in program
    // order, the reads of this one after it.
    __device__ __forceinline__ void build(const BatchMatrixArgs &MA, const uint8_t *__restrict__ s1, int32_t n1,
                                          int32_t cl) {
        uint32_t x[C];
#pragma unroll
        for (int k = 0; k < C; ++k) x[k] = (uint32_t)MA.index[s1[min(cl + k, n1) - 1]];
        build_profile(MA, x, pl);
    }
    __device__ __forceinline__ void fetch(uint32_t word) {
#pragma unroll
        for (int q = 0; q < 4; ++q) scn[q] = pl[((word >> (8 * q)) & 255u) * kWave];
    }
    __device__ __forceinline__ void iter_begin(const u32x4 (&pk)[4]) { fetch(pk[0][0]); }
    template <int gi>
    __device__ __forceinline__ void group_begin(const u32x4 (&pk)[4]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) sc[q] = scn[q];
        if constexpr (gi < 15) fetch(pk[(gi + 1) >> 2][(gi + 1) & 3]);  // row letters of steps 4gi+4 .. 4gi+7
    }
    template <int q, int k>
    __device__ __forceinline__ int32_t score_byte() const {
        return (int32_t)(int8_t)(uint8_t)(sc[q] >> (8 * k));
    }
};

// ---- the matrix and local sweeps: the skeleton ----

// 64 steps of iteration `it` (steps 64it + u): lane l computes row 64it + u - l.
//   EDGE : some lane's row is outside 1..n2 in this iteration (it holds its cells)
//   colw : where H of the right column of block it - 1 goes, E eoff words behind it
//          (NULL: it has no reader)
//   dq   : DIRS: this lane's first dword of the iteration's first 4-step group
template <class P, bool EDGE, bool DIRS>
__device__ __forceinline__ void sweep_iter(int it, const u32x4 (&pk)[4], int32_t n2, P &S, int32_t *colw, int64_t eoff,
                                           uint32_t *dq, int lane) {
    int32_t rr = 64 * it - lane - 1;  // EDGE: row of this lane before the step
    S.iter_begin(pk);
    static_for<0, 16>([&](auto gc) {
        constexpr int gi = decltype(gc)::value;
        S.template group_begin<gi>(pk);
        uint32_t dw[2] = {0, 0};  // DIRS: 4 bits per cell, dword h halfword q & 1 = step 4gi + q, nibble k = column k
        static_for<0, 4>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            constexpr int u = 4 * gi + q;
            const int32_t lfh = __builtin_amdgcn_readlane(S.fvh, u);
            const int32_t lfe = __builtin_amdgcn_readlane(S.fve, u);
            const int32_t left = __builtin_amdgcn_update_dpp(lfh, S.u[C - 1], 0x138 /*wave_shr:1*/, 0xF, 0xF, false);
            int32_t el = __builtin_amdgcn_update_dpp(lfe, S.e, 0x138 /*wave_shr:1*/, 0xF, 0xF, false);
            int32_t lh = S.opening(left);
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
                const int32_t d = S.template diag_sub<q, k>(diag);
                S.template cell<k, 16 * (q & 1) + 4 * k, EDGE, DIRS>(d, diag, lh, el, act, 64 * it + u, dw[q >> 1]);
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
        S.group_end();
    });
}

// One pair (n1, n2 >= 1), all its strips, by this wave.  s1: the pair's column
// characters; rowb[y] = row y's character; col: the worker's column scratch (H at
// col[row], E at col[eoff + row]); dirs: DIRS: this lane's first dword of the pair's
// first 4-step group.
template <class P, bool DIRS, class M>
__device__ __forceinline__ void sweep_pair(const M &mode, int32_t *out, const uint8_t *__restrict__ s1, int32_t n1,
                                           const uint8_t *__restrict__ rowb, int32_t n2, int32_t *__restrict__ col,
                                           uint32_t *__restrict__ dirs, int lane) {
    const int64_t eoff = mode.affine().eoff;
    const int nstrips = (n1 + kCkptCols - 1) / kCkptCols;
    const int nblocks = n2 / 64 + 1;  // ceil((n2 + 1) / 64)
    const int lastb = nblocks - 1;
    P S(mode, out, lane);

    for (int p = 0; p < nstrips; ++p) {
        const int32_t cl = 1 + p * kCkptCols + C * lane;  // first column of this lane
        S.strip_begin(s1, n1, cl);
        S.acch = S.acce = 0;
        const bool fed = p > 0;            // (strip 0 never reads the scratch)
        const bool pub = p + 1 < nstrips;  // (the last strip's right column has no reader)

        // row words and the feed are loaded one iteration ahead.  Strip 0: the boundary
        // column
        u32x4 pkc[4], pkn[4];
        load_rows(rowb, 0, lane, pkc);
        int32_t fnh = S.boundary_h(lane == 0), fne = S.boundary_e();
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
                fnh = S.boundary_h(false);
            }
            load_rows(rowb, min(it + 1, nblocks), lane, pkn);
            const bool edge = it == 0 || 64 * it + 63 > n2;
            int32_t *colw = (pub && it >= 1) ? col + 64 * (it - 1) : nullptr;
            uint32_t *dq = nullptr;
            if constexpr (DIRS) dq = dirs + ((int64_t)p * (nblocks + 1) + it) * (32 * kWave);
            if (edge)
                sweep_iter<P, true, DIRS>(it, pkc, n2, S, colw, eoff, dq, lane);
            else
                sweep_iter<P, false, DIRS>(it, pkc, n2, S, colw, eoff, dq, lane);
#pragma unroll
            for (int h = 0; h < 4; ++h) pkc[h] = pkn[h];
        }
        S.strip_end(p == nstrips - 1, cl, n1, n2);
    }
    S.pair_end();
}

// The body of a sweep kernel: a persistent grid of one-wave workgroups; pairs claimed in
// order from the ticket.
template <bool DIRS, class M>
__device__ __forceinline__ void sweep_tickets(const M &mode) {
    const BatchArgs &A = mode.affine().b;
    const int lane = threadIdx.x;
    int32_t *col = A.colscr + (int64_t)blockIdx.x * A.cstride;
    for (;;) {
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
            const uint8_t *rowb = A.rows + kBatchRowPad + o2 - 1;  // rowb[y] = row y's character (or letter)
            uint32_t *dirs = nullptr;
            if constexpr (DIRS) dirs = (uint32_t *)(A.dirs + uniform64(A.dir_off[t])) + lane;
            mode.template pair<DIRS>(out, s1, (int32_t)len1, rowb, (int32_t)len2, col, dirs, lane);
        }
    }
}

// ---- the matrix and semi-global sweeps: the global cell in the w form ----

// The global Gotoh cell in the w form (nw_batch_affine.hip's header states it; the cell,
// its boundaries and its results are that file's affine_iter / affine_pair / ticket loop
// in the skeleton's terms), without its substitution.
struct GlobalCell : GotohLane {
    int32_t go, ge;
    int32_t *score;
    int lane;

    __device__ __forceinline__ GlobalCell(const BatchAffineArgs &AA, int32_t *out, int lane_)
        : go(AA.gap_open), ge(AA.b.gap), score(out), lane(lane_) {}
    __device__ __forceinline__ void row0() {
#pragma unroll
        for (int k = 0; k < C; ++k) {
            u[k] = go;       // H'[0][c] = go + c*ge - ge*c
            f[k] = kNegInf;  // F'[0][c]
        }
        e = kNegInf;
        dg = go;
    }
    // H'[r][0] = go but H'[0][0] = 0 (the diagonal of cell (1, 1)), E'[r][0] = -inf
    __device__ __forceinline__ int32_t boundary_h(bool corner) const { return corner ? 0 : go; }
    __device__ __forceinline__ int32_t boundary_e() const { return kNegInf; }
    __device__ __forceinline__ int32_t opening(int32_t left) const { return left; }
    template <int k, int SH, bool EDGE, bool DIRS>
    __device__ __forceinline__ void cell(int32_t d, int32_t &diag, int32_t &left, int32_t &el, bool act, int32_t,
                                         uint32_t &bits) {
        const int32_t up = u[k];
        const int32_t fo = up + go, eo = left + go;  // a run opened from H'
        const int32_t fn = max(f[k], fo);
        const int32_t en = max(el, eo);
        // H' = max(H'_diag + s - 2 ge, F', E')
        int32_t x = max(max(d, fn), en);
        if constexpr (DIRS) {
            uint32_t code = x == d ? 0u : x == fn ? 1u : 2u;
            code |= el > eo ? 4u : 0u;
            code |= f[k] > fo ? 8u : 0u;
            bits |= code << SH;
        }
        diag = up;
        if constexpr (EDGE) {
            x = act ? x : up;
            f[k] = act ? fn : f[k];
        } else {
            f[k] = fn;
        }
        u[k] = x;
        left = x;
        el = en;
    }
    __device__ __forceinline__ void group_end() {}
    // every lane now holds row n2 of its columns
    __device__ __forceinline__ void strip_end(bool last, int32_t cl, int32_t n1, int32_t n2) {
        if (last) {
#pragma unroll
            for (int k = 0; k < C; ++k)
                if (cl + k == n1) *score = u[k] + ge * (n2 + n1);
        }
    }
    __device__ __forceinline__ void pair_end() {}
};

// What the global kernels write for a pair they do not sweep.
struct GlobalSweep {
    const BatchAffineArgs &AA;
    __device__ __forceinline__ const BatchAffineArgs &affine() const { return AA; }
    __device__ __forceinline__ int32_t *result(int pair) const { return AA.b.scores + pair; }
    // not a pair this launch was sized for: the column scratch would not hold it
    __device__ __forceinline__ void refused(int32_t *score, int lane) const {
        if (lane == 0) *score = INT32_MIN;
    }
    // no cells: the corner of the boundary, one gap (none for 0 x 0)
    __device__ __forceinline__ void empty(int32_t *score, int32_t n, int lane) const {
        if (lane == 0) *score = n > 0 ? AA.gap_open + AA.b.gap * n : 0;
    }
};

template <bool WIDE>
struct MatrixCell : GlobalCell, ProfileSub {
    const BatchMatrixArgs &MA;
    int32_t bias;  // WIDE: -2 ge

    template <class M>
    __device__ __forceinline__ MatrixCell(const M &mode, int32_t *out, int lane_)
        : GlobalCell(mode.AA, out, lane_), ProfileSub{mode.pl}, MA(mode.MA), bias(-2 * mode.AA.b.gap) {}
    __device__ __forceinline__ void strip_begin(const uint8_t *__restrict__ s1, int32_t n1, int32_t cl) {
        row0();
        build(MA, s1, n1, cl);
    }
    template <int q, int k>
    __device__ __forceinline__ int32_t diag_sub(int32_t diag) const {
        int32_t d = diag + score_byte<q, k>();
        if constexpr (WIDE) d += bias;
        return d;
    }
};

// ---- the local and semi-global sweeps: the order of their candidates ----

// a candidate (v, i, j) before the best (bv, bi, bj): score descending, row ascending,
// column ascending
__device__ __forceinline__ bool before(int32_t v, int32_t i, int32_t j, int32_t bv, int32_t bi, int32_t bj) {
    return v > bv || (v == bv && (i < bi || (i == bi && j < bj)));
}

// ---- the banded sweeps: the range of a strip ----

// What the band leaves of a pair (n1 columns, n2 rows, the call's width) to sweep, and of
// its strip p once strip(p, lane) was called (nw_batch.h has the geometry, nw_batch_banded.hip's
// header, point 1, the reasons).  dualb_pair loops over it0 .. itl; banded_pair has the same
// arithmetic in its own text (its header says why).
struct BandRange {
    int32_t dlo, dhi;  // cell (i, j) is in the band iff dlo <= i - j <= dhi
    uint32_t span;     // dhi - dlo
    int slots;         // iterations of a strip in the pair's direction block
    int nblocks;       // ceil((n2 + 1) / 64)
    int32_t c0;        // the column the strip is fed from
    int it0, itl;      // the strip's first and last iteration
    int32_t tb;        // 256p + 5 lane + 1 + dlo: step - tb - k = (the diagonal of the lane's column k) - dlo

    __device__ __forceinline__ BandRange(int32_t n1, int32_t n2, int32_t band)
        : dlo((int32_t)batch_banded_dlo(n1, n2, band)), dhi((int32_t)batch_banded_dhi(n1, n2, band)),
          span((uint32_t)(dhi - dlo)), slots((int)batch_banded_slots(n1, n2, band)), nblocks(n2 / 64 + 1) {}
    __device__ __forceinline__ void strip(int p, int lane) {
        c0 = p * kCkptCols;
        it0 = (int)batch_banded_first(p, dlo);
        // (never beyond the strip's slots: the range is that short by its definition, and a
        // store past the pair's direction block must be impossible whatever the arithmetic)
        itl = min(min(nblocks, ((c0 + 319 + dhi) >> 6) + 1), it0 + slots - 1);
        tb = c0 + 5 * lane + 1 + dlo;
    }
    // all 64 steps of iteration `it` lie in the band, on every lane (wave-uniform): its first
    // step's lane 63, column 3, and its last step's lane 0, column 0
    __device__ __forceinline__ bool inside(int it) const {
        return 64 * it - c0 - 319 >= dlo && 64 * it + 62 - c0 <= dhi;
    }
    // row `row` of column c0, the feed's, is in the band
    __device__ __forceinline__ bool in(int32_t row) const { return (uint32_t)(row - c0 - dlo) <= span; }
};

// ---- the affine family: the direction bits of a cell ----

// NW_DIR_NIBBLE(bits, d, iters, r, c): declares `bits`, the four direction bits of cell
// (r, c), r, c >= 1, of the block `d` of a pair whose strips have `iters` iterations.  The
// cell was computed in strip p = (c-1) / 256 by lane l = ((c-1) % 256) / 4, column k =
// (c-1) % 4, at step s = r + l: nibble k % 2 of byte (s % 2) * 2 + k / 2 of dword [p]
// [s / 64][s % 64 / 4][s % 4 / 2][l].  The three walks (nw_batch_affine_walk, nw_batch_local_
// walk, nw_batch_semi_walk) use it.  A macro, not a function: through an inlined function the walks' loops
// came out with another register allocation and one move displaced, and the walks are
// held to the ISA they had when each carried this expression itself.
#define NW_DIR_NIBBLE(bits, d, iters, r, c)                                                                            \
    const int64_t cj = (c) - 1;                                                                                        \
    const int64_t p = cj >> 8, l = (cj & 255) >> 2, k = cj & 3;                                                        \
    const int64_t s = (r) + l;                                                                                         \
    const int64_t idx =                                                                                                \
        ((((p * (iters) + (s >> 6)) * 16 + ((s & 63) >> 2)) * 2 + ((s & 3) >> 1)) * 64 + l) * 4 + (s & 1) * 2 + (k >> 1); \
    const uint32_t bits = ((uint32_t)(d)[idx] >> (4 * (k & 1))) & 15u

// ---- the two-piece kernels (nw_batch_dual.hip): the direction byte of a cell ----

// The index of the byte of cell (r, c), r, c >= 1, in the direction block of a pair whose
// strips have `iters` iterations: one byte per cell, computed in strip p = (c-1) / 256 by
// lane l = ((c-1) % 256) / 4, column k = (c-1) % 4, at step s = r + l: byte k of dword [p][s]
// [l] (a strip has 64 * iters steps).  The sweep stores by it, nw_batch_dual_walk reads by it.
constexpr int64_t dual_dir_byte(int64_t iters, int64_t r, int64_t c) {
    const int64_t cj = c - 1;
    const int64_t p = cj >> 8, l = (cj & 255) >> 2, k = cj & 3;
    return ((p * iters * 64 + r + l) * 64 + l) * 4 + k;
}

// The same in the direction block of a banded pair (nw_batch_dual_banded.hip): a strip holds
// `slots` iterations (batch_banded_slots), the first of them iteration batch_banded_first(p,
// dlo): byte k of dword [p][s / 64 - first(p)][s % 64][l].  The slot is clamped, so that no
// index can leave the pair's block whatever (r, c) is asked for.
constexpr int64_t dual_banded_dir_byte(int64_t slots, int64_t dlo, int64_t r, int64_t c) {
    const int64_t cj = c - 1;
    const int64_t p = cj >> 8, l = (cj & 255) >> 2, k = cj & 3;
    const int64_t s = r + l;
    const int64_t slot = min(max((s >> 6) - batch_banded_first(p, dlo), (int64_t)0), slots - 1);
    return (((p * slots + slot) * 64 + (s & 63)) * 64 + l) * 4 + k;
}

}  // namespace
}  // namespace nw
