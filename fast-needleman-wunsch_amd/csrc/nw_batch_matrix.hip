// nw_batch_matrix.hip -- gfx950 (MI355X) batched pairwise alignment under affine gap
// cost (Gotoh) with substitution by matrix: s(s1[j-1], s2[i-1]) = score[index[s1[j-1]]]
// [index[s2[i-1]]], an int8 matrix over at most 32 letters (nw_submat, include/nw_hip.h).
// Everything but the substitution is nw_batch_affine.hip's, whose header describes it:
// the persistent grid of one-wave workgroups and the ticket, the 256-column strips with
// lane l on columns 4l .. 4l+3, the EDGE test, the w form of H, E and F next to -2^29,
// the two-column scratch between strips and the 4 direction bits per cell in the same
// layout -- so the walk is that file's launch_batch_affine_walk, unchanged.
//
// The sweep's iteration body stands here a SECOND time, on purpose: nw_batch.hip and
// nw_batch_affine.hip stay byte-identical, so their kernels' code cannot move with a
// change made for the matrix.
//
// Substitution.  The matrix and the byte -> letter index travel in the kernel arguments
// (BatchMatrixArgs, 1.5 KiB).  The row characters are the concatenated s2 mapped through
// `index` by nw_batch_matrix_rows, behind the same zeroed pads: every byte of that
// buffer is a letter < n <= 32, also the pads and the neighbours' characters that EDGE
// lanes load and never use.  Per strip a lane builds its column profile in LDS:
//     prof[y][lane], y < 32: one dword, byte k = the score byte of (column 4l + k's
//     letter, row letter y)
// (columns past n1 take column n1's letter).  Per 4-step group the lane extracts the four row
// letters of the row word it already holds and reads the four dwords prof[y][lane], at
// the top of the group, where the affine kernel forms its v_perm tables; the cell's
// diagonal is diag + sext(byte k) of step q's dword.
//   Banks: the byte address is (y * 64 + lane) * 4; ds_read_b32 is served in two groups
//   of 32 lanes with bank (a / 4) mod 32 = lane mod 32: no two lanes of a group share a
//   bank, whatever their rows are.
//   Order: lane l writes and reads only prof[.][l] -- the profile is lane-private data
//   that happens to live in LDS, no lane ever reads what another wrote.  So the build of
//   a strip's profile, its reads, and the build of the next strip's (or next pair's)
//   profile are ordered by program order alone: the LDS executes one wave's operations
//   in the order issued, and the s_waitcnt lgkmcnt the compiler puts before the first
//   use of a read's result is the only wait.  No barrier: there is no second wave.
//
// The table bytes.  The w form needs s - 2 ge per cell.  When every s - 2 ge of the
// matrix fits int8 the host puts those bytes into the arguments and the cell adds
// nothing (WIDE = false; every BLOSUM / PAM with |ge| of a few).  Else the arguments
// hold s itself and the cell adds the wave-uniform -2 ge after the byte (WIDE = true:
// one more v_add per cell).  Both forms are in each kernel, chosen once per launch, as
// the affine kernel holds its two substitution forms.
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
constexpr int32_t kNegInf = -(1 << 29);
constexpr int kLetters = kBatchMatrixLetters;

struct MatrixLane {
    int32_t u[C];        // H' of the lane's current row, column k
    int32_t f[C];        // F' of the lane's current row, column k
    int32_t e;           // E' of the lane's current row, last column
    int32_t dg;          // H'_diag of column 0 for the next step
    int32_t fvh, fve;    // feed: lane x holds H' / E' of the left strip's right column at row 64it + x
    int32_t acch, acce;  // right column gathered: lane x holds row 64(it-1) + x
};

// (nw_batch_affine.hip load_rows)
__device__ __forceinline__ void load_rows(const uint8_t *__restrict__ rowb, int j, int lane, u32x4 (&pk)[4]) {
    const uint8_t *b = rowb + (int64_t)j * 64 - lane;
#pragma unroll
    for (int h = 0; h < 4; ++h) __builtin_memcpy(&pk[h], b + 16 * h, 16);
}

// 64 steps of iteration `it` (nw_batch_affine.hip affine_iter).  pl: this lane's dword
// of profile row 0; bias: WIDE: -2 ge.
template <bool WIDE, bool EDGE, bool DIRS>
__device__ __forceinline__ void matrix_iter(int it, const u32x4 (&pk)[4], const uint32_t *pl, int32_t bias, int32_t go,
                                            int32_t n2, MatrixLane &S, int32_t *colw, int64_t eoff, uint32_t *dq,
                                            int lane) {
    int32_t rr = 64 * it - lane - 1;  // EDGE: row of this lane before the step
    // the profile dwords of a group are read one group ahead of their use: a ds_read_b32
    // takes some 50 cycles to return, and one wave per SIMD has nothing else to run
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
                int32_t d = diag + (int32_t)(int8_t)(uint8_t)(sc[q] >> (8 * k));
                if constexpr (WIDE) d += bias;
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

// (nw_batch.hip uniform64)
__device__ __forceinline__ int64_t uniform64(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
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

// One pair (n1, n2 >= 1), all its strips, by this wave (nw_batch_affine.hip affine_pair).
template <bool WIDE, bool DIRS>
__device__ __forceinline__ void matrix_pair(const BatchMatrixArgs &MA, const uint8_t *__restrict__ s1, int32_t n1,
                                            const uint8_t *__restrict__ rowb, int32_t n2, int32_t *__restrict__ col,
                                            uint32_t *__restrict__ dirs, int32_t *score, uint32_t *pl, int lane) {
    const BatchArgs &A = MA.a.b;
    const int32_t ge = A.gap, go = MA.a.gap_open;
    const int64_t eoff = MA.a.eoff;
    const int32_t bias = -2 * ge;
    const int nstrips = (n1 + kCkptCols - 1) / kCkptCols;
    const int nblocks = n2 / 64 + 1;  // ceil((n2 + 1) / 64)
    const int lastb = nblocks - 1;

    for (int p = 0; p < nstrips; ++p) {
        const int32_t cl = 1 + p * kCkptCols + C * lane;  // first column of this lane
        MatrixLane S;
        uint32_t x[C];  // the columns' letters (past n1: column n1's, cells nobody reads; no branch, so the
                        // four loads and the four lookups overlap)
#pragma unroll
        for (int k = 0; k < C; ++k) {
            x[k] = (uint32_t)MA.index[s1[min(cl + k, n1) - 1]];
            S.u[k] = go;       // H'[0][c] = go + c*ge - ge*c
            S.f[k] = kNegInf;  // F'[0][c]
        }
        // this strip's profile over the last strip's (or the last pair's): the reads of
        // those are before this point in program order, the reads of this one after it
        build_profile(MA, x, pl);
        S.e = kNegInf;
        S.dg = go;
        S.acch = S.acce = 0;
        const bool fed = p > 0;            // (strip 0 never reads the scratch)
        const bool pub = p + 1 < nstrips;  // (the last strip's right column has no reader)

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
            if (fed) {
                const int64_t xr = 64 * min(it + 1, lastb) + lane;
                fnh = col[xr];
                fne = col[eoff + xr];
            } else {
                fnh = go;
            }
            load_rows(rowb, min(it + 1, nblocks), lane, pkn);
            const bool edge = it == 0 || 64 * it + 63 > n2;
            int32_t *colw = (pub && it >= 1) ? col + 64 * (it - 1) : nullptr;
            uint32_t *dq = nullptr;
            if constexpr (DIRS) dq = dirs + ((int64_t)p * (nblocks + 1) + it) * (32 * kWave);
            if (edge)
                matrix_iter<WIDE, true, DIRS>(it, pkc, pl, bias, go, n2, S, colw, eoff, dq, lane);
            else
                matrix_iter<WIDE, false, DIRS>(it, pkc, pl, bias, go, n2, S, colw, eoff, dq, lane);
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

// (nw_batch_affine.hip claim_ticket_affine: kept out of line for the same reason)
__device__ __noinline__ int claim_ticket_matrix(uint32_t *ticket) {
    uint32_t t = 0;
    if ((threadIdx.x & 63) == 0) t = atomicAdd(ticket, 1u);
    return (int)__builtin_amdgcn_readfirstlane(t);
}

// Persistent grid of one-wave workgroups; pairs claimed in order from the ticket.
template <bool DIRS>
__global__ __launch_bounds__(64) void nw_batch_matrix_sweep(BatchMatrixArgs MA) {
    __shared__ uint32_t prof[kLetters * kWave];  // [row letter][lane], 8 KiB
    const BatchArgs &A = MA.a.b;
    const int lane = threadIdx.x;
    uint32_t *pl = prof + lane;
    int32_t *col = A.colscr + (int64_t)blockIdx.x * A.cstride;
    for (;;) {
        const int t = __builtin_amdgcn_readfirstlane(claim_ticket_matrix(A.ticket));  // (a call returns in a vector register)
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
            if (lane == 0) *score = n > 0 ? MA.a.gap_open + A.gap * n : 0;
        } else {
            const uint8_t *s1 = A.s1 + o1;
            const uint8_t *rowb = A.rows + kBatchRowPad + o2 - 1;  // rowb[y] = row y's letter
            uint32_t *dirs = nullptr;
            if constexpr (DIRS) dirs = (uint32_t *)(A.dirs + uniform64(A.dir_off[t])) + lane;
            if (MA.wide != 0)
                matrix_pair<true, DIRS>(MA, s1, (int32_t)len1, rowb, (int32_t)len2, col, dirs, score, pl, lane);
            else
                matrix_pair<false, DIRS>(MA, s1, (int32_t)len1, rowb, (int32_t)len2, col, dirs, score, pl, lane);
        }
    }
}

// The batch's row letters: d_rows[kBatchRowPad + i] = index[s2cat[i]]; the pads are
// zeroed (letter 0).  The index map travels in the arguments.
struct RowIndex {
    uint8_t index[256];
};

__global__ __launch_bounds__(256) void nw_batch_matrix_rows(const uint8_t *__restrict__ s2, int64_t total2,
                                                            RowIndex ix, uint8_t *__restrict__ rows) {
    const int64_t len = kBatchRowPad + total2 + kBatchRowTail;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < len; x += stride) {
        const int64_t i = x - kBatchRowPad;
        uint32_t b = 0;
        if (i >= 0 && i < total2) b = ix.index[s2[i]];
        rows[x] = (uint8_t)b;
    }
}

}  // namespace

int launch_batch_matrix_rows(const uint8_t *d_s2, int64_t total2, const uint8_t *index, uint8_t *d_rows,
                             void *stream) {
    const int64_t len = kBatchRowPad + total2 + kBatchRowTail;
    const int64_t g = std::min<int64_t>(4096, (len + 255) / 256);
    RowIndex ix;
    __builtin_memcpy(ix.index, index, 256);
    hipLaunchKernelGGL(nw_batch_matrix_rows, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, d_s2, total2, ix,
                       d_rows);
    return (int)hipGetLastError();
}

int launch_batch_matrix(const BatchMatrixArgs &a, bool dirs, int grid, void *stream) {
    if (dirs)
        hipLaunchKernelGGL(nw_batch_matrix_sweep<true>, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(nw_batch_matrix_sweep<false>, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace nw
