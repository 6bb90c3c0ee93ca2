// nw_batch_matrix.hip -- gfx950 (MI355X) batched pairwise alignment under affine gap
// cost (Gotoh) with substitution by matrix: s(s1[j-1], s2[i-1]) = score[index[s1[j-1]]]
// [index[s2[i-1]]], an int8 matrix over at most 32 letters (nw_submat, include/nw_hip.h).
// Everything but the substitution is described in nw_batch_affine.hip's header: the
// persistent grid of one-wave workgroups and the ticket, the 256-column strips with lane l
// on columns 4l .. 4l+3, the EDGE test, the w form of H, E and F next to -2^29, the
// two-column scratch between strips and the 4 direction bits per cell in the same layout
// -- so the walk is that file's launch_batch_affine_walk.  The code of all that is the
// sweep skeleton of nw_batch_dev.h, which nw_batch_local.hip and nw_batch_semi.hip run
// too.  The policy is that header's as well since nw_batch_semi.hip builds on it: the
// global Gotoh cell with its boundaries and results (GlobalCell, GlobalSweep) and the
// substitution read from a column profile in LDS (MatrixCell over ProfileSub).  This
// file keeps the choice of the cell's variant (MatrixSweep), the kernels and the kernel
// that makes the row letters.
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

#include "nw_batch_dev.h"

namespace nw {
namespace {

struct MatrixSweep : GlobalSweep {
    const BatchMatrixArgs &MA;
    uint32_t *pl;  // this lane's dword of profile row 0
    template <bool DIRS>
    __device__ __forceinline__ void pair(int32_t *out, const uint8_t *s1, int32_t n1, const uint8_t *rowb, int32_t n2,
                                         int32_t *col, uint32_t *dirs, int lane) const {
        if (MA.wide != 0)
            sweep_pair<MatrixCell<true>, DIRS>(*this, out, s1, n1, rowb, n2, col, dirs, lane);
        else
            sweep_pair<MatrixCell<false>, DIRS>(*this, out, s1, n1, rowb, n2, col, dirs, lane);
    }
};

template <bool DIRS>
__global__ __launch_bounds__(64) void nw_batch_matrix_sweep(BatchMatrixArgs MA) {
    __shared__ uint32_t prof[kLetters * kWave];  // [row letter][lane], 8 KiB
    sweep_tickets<DIRS>(MatrixSweep{{MA.a}, MA, prof + threadIdx.x});
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
