// nw_batch_semi.hip -- gfx950 (MI355X) batched pairwise SEMI-GLOBAL alignment: Gotoh with
// substitution by matrix and free end gaps per side (nw_score_batch_semi*, nw_align_batch_
// semi; include/nw_hip.h states the table, the end cell and the walk).  Everything but the
// boundaries and the ends is nw_batch_dev.h's code, the same the matrix kernel runs: the
// persistent grid of one-wave workgroups and the ticket, the 256-column strips with lane l
// on columns 4l .. 4l+3, the EDGE test, the row letters (launch_batch_matrix_rows), the
// 8 KiB column profile in LDS read one group ahead (ProfileSub), the two-column scratch
// between strips, the layout of the 4 direction bits per cell -- and the cell itself:
// GlobalCell::cell and MatrixCell<WIDE>::diag_sub as they stand.
//
// The form.  The w form of the global kernels (every value minus ge * (i + j)): there is
// no floor, so nothing of what kept the local kernel out of the w form applies but the
// boundaries.  A boundary that is not free holds go (H[0][j] = go + j ge), as in the
// matrix kernel; a free one holds H = 0, which is -ge * j per column of row 0 (set in
// strip_begin) and -ge * i per row of column 0 (fed to strip 0: boundary_h carries no row
// number, so the policy counts its calls -- call c of a strip is block c, lane x on row
// 64 c + x).  -ge * 0 is the corner's 0.  E[i][0] = F[0][j] = -2^29 as there.
//
// The ends.  Candidates for the end cell are (n2, n1); every (n2, j) with NW_ENDS_S1_END;
// every (i, n1) with NW_ENDS_S2_END.  The key is the local kernel's: score descending, i
// ascending, j ascending.
//   Last row: where a strip ends every lane holds row n2 of its columns.  They are
//   unshifted (+ ge * (n2 + j)) and the columns <= n1 that are candidates are folded into
//   the lane's best of the pair, on local copies as LocalCell does.  Columns past n1
//   compute cells of column n1's letter, which can outscore every real cell: dropped.
//   (n2, 0) is arithmetic (0, or go + n2 ge), added by the lane that holds column 1.
//   Last column (COL = true; only launches with NW_ENDS_S2_END run this variant, the others
//   compile none of it and their iteration is the matrix kernel's): per column a lane keeps
//   the largest unshifted H and the step at which it first appeared -- one add3 (H' + ge *
//   (column - lane) + ge * step), compare, select, max per cell.  Row 0 is the initial value
//   (0, or go + j ge: the candidate (0, n1)); only an active cell with a strictly greater
//   value updates, so a column keeps its earliest row and a held EDGE cell never wins.
//   Column n1's best joins the fold where the last strip ends.
// Once per pair six rounds combine the 64 lanes under the same key and lane 0 writes the
// nw_local_hit.  All of this state is initialised per strip or per pair.
//
// Directions are the global cell's (nw_batch_affine.hip), so with ends = 0 the bytes are
// the matrix kernel's.  nw_batch_semi_walk starts one thread per ticket at the hit's end
// cell; it keeps its own loop as the other two walks do (nw_batch_local.hip says why).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nw_batch_dev.h"

namespace nw {
namespace {

constexpr int32_t kEndsS1Begin = 1, kEndsS1End = 2, kEndsS2Begin = 4, kEndsS2End = 8;  // NW_ENDS_*

template <bool WIDE, bool COL>
struct SemiCell : MatrixCell<WIDE> {
    using Base = MatrixCell<WIDE>;
    int32_t ends;
    int32_t calls;  // boundary_h calls since strip_begin: the next one is block `calls`
    int32_t cb[C];  // COL: ge * (column - lane): H = H' + cb[k] + ge * step
    int32_t bv[C];  // COL: largest H of column k so far, row 0 included
    int32_t bs[C];  // COL: the step at which bv[k] first appeared (row = step - lane)
    int32_t pv = INT32_MIN, pi = INT32_MAX, pj = INT32_MAX;  // this lane's best of the pair: none yet

    template <class M>
    __device__ __forceinline__ SemiCell(const M &mode, int32_t *out, int lane_)
        : Base(mode, out, lane_), ends(mode.SA.ends), calls(0) {}
    __device__ __forceinline__ void strip_begin(const uint8_t *__restrict__ s1, int32_t n1, int32_t cl) {
        const int32_t go = this->go, ge = this->ge;
        const bool free0 = (ends & kEndsS1Begin) != 0;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const int32_t j = cl + k;
            this->u[k] = free0 ? -ge * j : go;  // H'[0][j] of H[0][j] = 0 / go + j ge
            this->f[k] = kNegInf;
            if constexpr (COL) {
                cb[k] = ge * (j - this->lane);
                bv[k] = free0 ? 0 : go + ge * j;
                bs[k] = this->lane;  // row 0
            }
        }
        this->e = kNegInf;
        this->dg = go;  // (replaced at the lane's row 0 by H'[0][cl - 1], before its first cell)
        calls = 0;
        this->build(this->MA, s1, n1, cl);  // (past n1: column n1's letter; those columns are dropped in strip_end)
    }
    // H'[i][0] of the block of this call; a free column holds H = 0, the corner too
    __device__ __forceinline__ int32_t boundary_h(bool corner) {
        const int32_t row = 64 * calls + this->lane;
        ++calls;
        if ((ends & kEndsS2Begin) != 0) return -this->ge * row;
        return corner ? 0 : this->go;
    }
    template <int k, int SH, bool EDGE, bool DIRS>
    __device__ __forceinline__ void cell(int32_t d, int32_t &diag, int32_t &left, int32_t &el, bool act, int32_t step,
                                         uint32_t &bits) {
        this->GlobalCell::template cell<k, SH, EDGE, DIRS>(d, diag, left, el, act, step, bits);
        if constexpr (COL) {
            const int32_t hv = this->u[k] + cb[k] + this->ge * step;
            bool better = hv > bv[k];
            if constexpr (EDGE) {
                // (a held cell repeats H' under another step: not a cell of the table)
                better = better && act;
                bv[k] = better ? hv : bv[k];
            } else {
                bv[k] = max(bv[k], hv);
            }
            bs[k] = better ? step : bs[k];
        }
    }
    // COL: as in LocalCell, the updates hang off the cells' dependency chain; the group's
    // are done here, and nothing moves across its end
    __device__ __forceinline__ void group_end() {
        if constexpr (COL) {
#pragma unroll
            for (int k = 0; k < C; ++k) asm volatile("" : "+v"(bv[k]), "+v"(bs[k]));
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // every lane now holds row n2 of its columns
    __device__ __forceinline__ void strip_end(bool last, int32_t cl, int32_t n1, int32_t n2) {
        const int32_t go = this->go, ge = this->ge;
        const bool row_free = (ends & kEndsS1End) != 0;
        int32_t tv = pv, ti = pi, tj = pj;  // (locals: the updates become selects, not branches)
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const int32_t j = cl + k;
            const int32_t v = this->u[k] + ge * (n2 + j);
            if (j <= n1 && (row_free || j == n1) && before(v, n2, j, tv, ti, tj)) {
                tv = v;
                ti = n2;
                tj = j;
            }
        }
        if (row_free && cl == 1) {  // (n2, 0)
            const int32_t v = (ends & kEndsS2Begin) != 0 ? 0 : go + ge * n2;
            if (before(v, n2, 0, tv, ti, tj)) {
                tv = v;
                ti = n2;
                tj = 0;
            }
        }
        if constexpr (COL) {
            if (last) {
#pragma unroll
                for (int k = 0; k < C; ++k) {
                    const int32_t i = bs[k] - this->lane;
                    if (cl + k == n1 && before(bv[k], i, n1, tv, ti, tj)) {
                        tv = bv[k];
                        ti = i;
                        tj = n1;
                    }
                }
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
        if (this->lane == 0) {
            int32_t *hit = this->score;
            hit[0] = tv;
            hit[1] = ti;
            hit[2] = tj;
            hit[3] = -1;  // (the walk writes the begin cell)
            hit[4] = -1;
            hit[5] = hit[6] = hit[7] = 0;
        }
    }
};

// COL: the launch has NW_ENDS_S2_END (a kernel of its own, so that the launches without
// it keep the matrix kernel's registers)
template <bool COL>
struct SemiSweep {
    const BatchSemiArgs &SA;
    const BatchAffineArgs &AA;  // (what MatrixCell's constructor reads)
    const BatchMatrixArgs &MA;
    uint32_t *pl;  // this lane's dword of profile row 0
    __device__ __forceinline__ const BatchAffineArgs &affine() const { return AA; }
    __device__ __forceinline__ int32_t *result(int pair) const {
        return SA.hits + (int64_t)pair * kBatchLocalHitWords;
    }
    // not a pair this launch was sized for: the column scratch would not hold it
    __device__ __forceinline__ void refused(int32_t *hit, int lane) const {
        if (lane < kBatchLocalHitWords) hit[lane] = lane == 0 ? INT32_MIN : lane < 5 ? -1 : 0;
    }
    // No cells but one boundary of n + 1: B(0) = 0, B(k) = 0 (its begin is free) or go + k
    // ge.  The end is (n) alone, or with that boundary's end free the first maximum: k = 0
    // unless a positive ge lifts go + n ge above 0.  Which side is empty is read from the
    // offsets again (the skeleton passes the longer side's length only).
    __device__ __forceinline__ void empty(int32_t *hit, int32_t n, int lane) const {
        const int pair = (int)((hit - SA.hits) / kBatchLocalHitWords);
        const bool rows = __builtin_amdgcn_readfirstlane((int32_t)(AA.b.off1[pair + 1] - AA.b.off1[pair])) == 0;
        const bool begin_free = (SA.ends & (rows ? kEndsS2Begin : kEndsS1Begin)) != 0;
        const bool end_free = (SA.ends & (rows ? kEndsS2End : kEndsS1End)) != 0;
        const int32_t run = (begin_free || n == 0) ? 0 : AA.gap_open + AA.b.gap * n;
        int32_t v = run, k = n;
        if (end_free && run <= 0) v = k = 0;
        const int32_t ei = rows ? k : 0, ej = rows ? 0 : k;
        if (lane < kBatchLocalHitWords)
            hit[lane] = lane == 0 ? v : lane == 1 ? ei : lane == 2 ? ej : lane < 5 ? -1 : 0;
    }
    template <bool DIRS>
    __device__ __forceinline__ void pair(int32_t *out, const uint8_t *s1, int32_t n1, const uint8_t *rowb, int32_t n2,
                                         int32_t *col, uint32_t *dirs, int lane) const {
        if (MA.wide != 0)
            sweep_pair<SemiCell<true, COL>, DIRS>(*this, out, s1, n1, rowb, n2, col, dirs, lane);
        else
            sweep_pair<SemiCell<false, COL>, DIRS>(*this, out, s1, n1, rowb, n2, col, dirs, lane);
    }
};

template <bool DIRS, bool COL>
__global__ __launch_bounds__(64) void nw_batch_semi_sweep(BatchSemiArgs SA) {
    __shared__ uint32_t prof[kLetters * kWave];  // [row letter][lane], 8 KiB
    sweep_tickets<DIRS>(SemiSweep<COL>{SA, SA.m.a, SA.m, prof + threadIdx.x});
}

// The walk: one thread per ticket over the direction bits of nw_batch_semi_sweep<true>,
// in nw_batch_affine.hip's layout.  It starts at the hit's end cell in state H.
//   at (0, 0): stop
//   H, on row 0: stop if NW_ENDS_S1_BEGIN, else a left without reading bits
//   H, on column 0: stop if NW_ENDS_S2_BEGIN, else an up
//   H, inner cell: bits 0-1: 0 emits a diag; 1 / 2 switch to F / E and emit nothing
//   F: emits an up and moves; bit 3 of the cell it left: 1 stays in F, 0 returns to H
//   E: emits a left and moves; bit 2 likewise
// F and E are entered at inner cells only and return to H at the latest when the run
// reaches row 1 / column 1, where it can only have been opened: on a boundary the state
// is H.  The cell where the walk stops goes into the hit as the begin cell.  Ops go end ->
// begin into the pair's slot; nw_batch_reverse turns them round.
__global__ __launch_bounds__(64) void nw_batch_semi_walk(BatchSemiWalkArgs SW) {
    const BatchWalkArgs &W = SW.w;
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= W.npairs) return;
    const int pair = W.order != nullptr ? W.order[t] : t;
    const int64_t n1 = W.off1[pair + 1] - W.off1[pair], n2 = W.off2[pair + 1] - W.off2[pair];
    int32_t *hit = SW.hits + (int64_t)pair * kBatchLocalHitWords;
    int64_t r = hit[1], c = hit[2];
    if (r < 0 || c < 0 || r > n2 || c > n1) r = c = 0;  // (not a hit of this pair's table: nothing to walk)
    const bool stop_row0 = (SW.ends & kEndsS1Begin) != 0, stop_col0 = (SW.ends & kEndsS2Begin) != 0;
    const int64_t iters = batch_iters(n2);
    const uint8_t *d = W.dirs + W.dir_off[t];
    uint8_t *ops = W.ops + W.ops_off[t];
    int64_t n = 0;
    uint32_t state = 0;  // 0 H, 1 F, 2 E
    while (r > 0 || c > 0) {
        if (r == 0 || c == 0) {  // (state is H here)
            if (r == 0 ? stop_row0 : stop_col0) break;
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
    hit[3] = (int32_t)r;
    hit[4] = (int32_t)c;
    W.n_ops[t] = n;
}

}  // namespace

int launch_batch_semi(const BatchSemiArgs &a, bool dirs, int grid, void *stream) {
    const dim3 g((unsigned)grid), b(64);
    hipStream_t s = (hipStream_t)stream;
    if ((a.ends & kEndsS2End) != 0) {  // the best of column n1 is tracked
        if (dirs)
            hipLaunchKernelGGL((nw_batch_semi_sweep<true, true>), g, b, 0, s, a);
        else
            hipLaunchKernelGGL((nw_batch_semi_sweep<false, true>), g, b, 0, s, a);
    } else {
        if (dirs)
            hipLaunchKernelGGL((nw_batch_semi_sweep<true, false>), g, b, 0, s, a);
        else
            hipLaunchKernelGGL((nw_batch_semi_sweep<false, false>), g, b, 0, s, a);
    }
    return (int)hipGetLastError();
}

int launch_batch_semi_walk(const BatchSemiWalkArgs &w, void *stream) {
    hipLaunchKernelGGL(nw_batch_semi_walk, dim3((unsigned)((w.w.npairs + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                       w);
    return launch_batch_reverse(w.w, stream);
}

}  // namespace nw
