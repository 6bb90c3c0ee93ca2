// nw_ckpt.hip -- gfx950 (MI355X) checkpoint sweep: the Needleman-Wunsch table of
// (s1, s2) computed and NOT stored.  The same cells as the strip kernel
// (nw_strips.h), in the same w form w = t - GAP*(i+j) with the same substitution
// (v_perm score tables or byte compares, chosen on the device from nprof), but HBM
// gets only
//   * the checkpoint rows r*K, r = 1 .. nck (granules {kCkptTag | t}, one per column
//     0..n1: what nw_fill_band_async takes as halo_in),
//   * the strip-to-strip hand-off granules,
//   * the score t[n2][n1].
// So there is no LDS ring and there are no store waves: a workgroup is ONE wave,
// and a CU holds several of them (kCkptWavesPerCU, one per SIMD).
//
// Decomposition: columns 1..n1 in vertical strips of 256 columns, claimed in order
// from the ticket by a persistent grid (a strip's producer is always already
// running).  Lane l owns columns 4l .. 4l+3 of the strip and at step s computes row
// s - l: an anti-diagonal across the lanes, DPP wave_shr:1 for the left neighbour.
//   * Lane 0's left neighbour is the previous strip's right column: the granules of
//     rows 64it .. 64it+63 are loaded one iteration ahead, one per lane, and step u
//     reads lane u's with v_readlane.  A block that is not complete yet is waited
//     for in 16-row chunks (nw_dev.h wait_chunk: the __noinline__ slow path).
//   * The right column (lane 63's last cell) is gathered with v_readlane /
//     v_writelane into one register -- lane x holds row 64b + x of block b -- and
//     published 16 rows at a time, right after the step that completes the chunk.
//   * In an iteration whose rows 64it is a checkpoint, lane u is on that row at
//     step u: it keeps its four cells then, and after the iteration every lane
//     writes its four granules (the wave writes 256 contiguous columns).
//   * Lanes above row 1 hold row 0 (w = 0) and lanes below row n2 keep row n2, so
//     after the last iteration every lane holds its cells of row n2: the score.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "nw_ckpt.h"
#include "nw_dev.h"
#include "nw_internal.h"
#include "nw_strips.h"  // (load_packs, diag_plus_sub: the strips' row words and substitution)

namespace nw {
namespace {

constexpr int C = kCkptC;
constexpr int G = 16;  // rows per published chunk of the right column (Lay::kGran)

struct SweepLane {
    int32_t u[C];     // w of the lane's current row, column k
    int32_t dg;       // w_diag of column 0 for the next step
    uint32_t apk;     // raw column characters, byte k = column k
    uint32_t tlo[C];  // SUB_PERM score tables
    uint32_t thi[C];
    int32_t fv;       // feed: lane x holds the left strip's right column at row 64it + x
    int32_t acc;      // right column gathered: lane x holds row 64(it-1) + x
    int32_t sv[C];    // the lane's cells on the checkpoint row of this iteration
};

// 64 steps of iteration `it` (steps 64it + u): lane l computes row 64it + u - l.
//   EDGE : some lane's row is outside 1..n2 in this iteration (it holds its cells)
//   CK   : row 64it is a checkpoint (lane u keeps its cells at step u)
//   g    : this lane's feed granule of block it (NULL: the boundary column, w = 0);
//          `ready` leading 16-row chunks of it were tagged when it was loaded
//   gp   : this lane's granule of block it - 1 in the strip's own slot (NULL: none)
// Returns false when a wait gave up.
template <int MODE, bool EDGE, bool CK>
__device__ __forceinline__ bool sweep_iter(const CkptArgs &A, int it, const u32x4 (&pk)[4], int32_t msp,
                                           int32_t mmp, SweepLane &S, const uint64_t *g, uint32_t tag, int ready,
                                           uint64_t *gp, uint64_t tagw, int lane) {
    bool ok = true;
    int32_t rr = 64 * it - lane - 1;  // EDGE: row of this lane before the step
    const int32_t n2 = (int32_t)A.n2;
    static_for<0, 16>([&](auto gc) {
        constexpr int gi = decltype(gc)::value;
        // chunk c of the feed is read from step 16c on: wait for it if it was not there
        if constexpr ((4 * gi) % G == 0 && gi > 0) {
            constexpr int c = 4 * gi / G;
            if (g != nullptr && ready <= c) {
                const uint64_t v = wait_chunk<G, 1>(g, tag, c, A.ctrl, 41, A.timeout_ticks);
                ok &= __all(lane / G != c || (uint32_t)(v >> 32) == tag);
                S.fv = (int32_t)(uint32_t)v;
                ready = max(c + 1, chunks_ready<G>(v, tag));
            }
        }
        const uint32_t word = pk[gi >> 2][gi & 3];  // row characters of steps 4gi .. 4gi+3
        uint32_t sc[C];
        if constexpr (MODE == SUB_PERM) {
#pragma unroll
            for (int k = 0; k < C; ++k) sc[k] = __builtin_amdgcn_perm(S.thi[k], S.tlo[k], word);
        }
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
                // w = max(w_diag + s - 2 GAP, w_up, w_left)
                int32_t x = max(max(d, S.u[k]), left);
                diag = S.u[k];
                if constexpr (EDGE) x = act ? x : S.u[k];
                S.u[k] = x;
                left = x;
                if constexpr (CK) S.sv[k] = lane == u ? x : S.sv[k];
            });
            // lane 63 is on row 64(it-1) + u + 1: into lane (u + 1) % 64 of the gather
            const int32_t rv = __builtin_amdgcn_readlane(S.u[C - 1], 63);
            asm("v_writelane_b32 %0, %1, %2" : "+v"(S.acc) : "s"(rv), "i"((u + 1) & 63));
            if constexpr (u % G == G - 2) {
                // rows 64(it-1) + Gc .. + G-1 are gathered (lanes Gc .. Gc+G-1)
                if (gp != nullptr && lane / G == u / G) gran_store(gp, tagw | (uint32_t)S.acc);
            }
        });
    });
    return ok;
}

template <int MODE>
__device__ __forceinline__ void sweep_strip(const CkptArgs &A, int p, int lane) {
    const int32_t gap = A.gap;
    const int32_t msp = A.match - 2 * gap, mmp = A.mismatch - 2 * gap;
    const int64_t cl = 1 + (int64_t)p * kCkptCols + (int64_t)C * lane;  // first column of this lane
    SweepLane S;
    S.apk = 0;
    // SUB_PERM tables: T_k[x] = s(a_k, chars[x]) - 2*GAP (nw_strips.h compute_strip)
    const uint32_t mmb = ((uint32_t)mmp & 255u) * 0x01010101u;
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const int64_t c = cl + k;
        const uint32_t a = c <= A.n1 ? (uint32_t)A.s1[c - 1] : 0u;
        S.apk |= a << (8 * k);
        S.u[k] = 0;  // w[0][c] = t[0][c] - GAP*c = 0
        S.sv[k] = 0;
        if constexpr (MODE == SUB_PERM) {
            const uint32_t x = c <= A.n1 ? (uint32_t)A.charmap[a] : 0xFFu;
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
    const bool fed = p > 0;
    const bool pub = p + 1 < A.nstrips;  // (the last strip's right column has no reader)
    const uint64_t *gin = A.gran + (int64_t)((p + A.M - 1) % A.M) * A.gstride + lane;
    uint64_t *gout = A.gran + (int64_t)(p % A.M) * A.gstride + lane;
    const uint32_t tag = A.tagbase + (uint32_t)p;
    const uint64_t tagw = (uint64_t)(A.tagbase + (uint32_t)p + 1u) << 32;
    const int nblocks = A.nblocks;
    const int lastb = nblocks - 1;
    const u32x4 *pkp = (const u32x4 *)A.rowpack;

    // row words and feed granules are loaded one iteration ahead
    u32x4 pkc[4], pkn[4];
    load_packs(pkp, 0, lane, pkc);
    uint64_t gn = fed ? gran_load(gin) : 0ull;
    bool ok = true;
    // row 64*nblocks - 1 completes on lane 63 in iteration nblocks
    for (int it = 0; it <= nblocks && ok; ++it) {
        const uint64_t *g = nullptr;
        int ready = 64 / G;
        if (fed && it < nblocks) {
            g = gin + (int64_t)it * 64;
            uint64_t gv = gn;
            ready = chunks_ready<G>(gv, tag);
            if (ready == 0) {  // chunk 0 is needed right away
                gv = wait_chunk<G, 1>(g, tag, 0, A.ctrl, 40, A.timeout_ticks);
                ok &= __all(lane >= G || (uint32_t)(gv >> 32) == tag);
                ready = max(1, chunks_ready<G>(gv, tag));
            }
            S.fv = (int32_t)(uint32_t)gv;
        }
        if (fed) gn = gran_load(gin + (int64_t)min(it + 1, lastb) * 64);
        load_packs(pkp, it + 1, lane, pkn);
        const int64_t R = 64 * (int64_t)it;
        const bool ck = it >= 1 && R % A.K == 0 && R / A.K <= A.nck;
        const bool edge = it == 0 || R + 63 > A.n2;
        uint64_t *gp = (pub && it >= 1) ? gout + (int64_t)(it - 1) * 64 : nullptr;
        bool r;
        if (edge)
            r = ck ? sweep_iter<MODE, true, true>(A, it, pkc, msp, mmp, S, g, tag, ready, gp, tagw, lane)
                   : sweep_iter<MODE, true, false>(A, it, pkc, msp, mmp, S, g, tag, ready, gp, tagw, lane);
        else
            r = ck ? sweep_iter<MODE, false, true>(A, it, pkc, msp, mmp, S, g, tag, ready, gp, tagw, lane)
                   : sweep_iter<MODE, false, false>(A, it, pkc, msp, mmp, S, g, tag, ready, gp, tagw, lane);
        ok &= r;
        if (ck && ok) {
            // checkpoint row R: t = w + GAP*(R + c), this lane's columns (and the boundary column 0)
            uint64_t *row = A.ckpt + (R / A.K - 1) * (A.n1 + 1);
            const uint64_t ctag = (uint64_t)kCkptTag << 32;
#pragma unroll
            for (int k = 0; k < C; ++k)
                if (cl + k <= A.n1) row[cl + k] = ctag | (uint32_t)(S.sv[k] + gap * (int32_t)(R + cl + k));
            if (p == 0 && lane == 0) row[0] = ctag | (uint32_t)(gap * (int32_t)R);
        }
#pragma unroll
        for (int h = 0; h < 4; ++h) pkc[h] = pkn[h];
    }
    // every lane now holds row n2 of its columns
    if (ok && p == A.nstrips - 1) {
#pragma unroll
        for (int k = 0; k < C; ++k)
            if (cl + k == A.n1) *A.score = S.u[k] + gap * (int32_t)(A.n2 + A.n1);
    }
}

// Persistent grid of one-wave workgroups; strips claimed in order from the ticket.
__global__ __launch_bounds__(64) void nw_ckpt_sweep(CkptArgs A) {
    const int lane = threadIdx.x;
    // table form when the launch allows it and s1 has at most kMaxPerm distinct
    // characters (nw_charmap), else compares -- as nw_fill_strips decides
    const uint32_t np = __builtin_amdgcn_readfirstlane(ctrl_load(A.nprof));
    const bool perm = A.perm != 0 && np <= kMaxPerm;
    for (;;) {
        int t = 0;
        if (lane == 0) t = (int)atomicAdd(A.ctrl, 1u);
        t = __builtin_amdgcn_readfirstlane(t);
        if (t >= A.nstrips) break;
        if (perm)
            sweep_strip<SUB_PERM>(A, t, lane);
        else
            sweep_strip<SUB_GEN>(A, t, lane);
    }
}

}  // namespace

int launch_ckpt_sweep(const CkptArgs &a, int grid, void *stream) {
    hipLaunchKernelGGL(nw_ckpt_sweep, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace nw
