// nw_launch.cpp -- the fill launches of libnwhip.so: argument checks, the context's
// launch workspace, FillArgs, and the kernels of nw_fill.hip / nw_rows.hip /
// nw_finish.hip.  launch_fill serves the whole table and the row, column and
// block-cyclic bands; nw_fill_tband_async the row band in horizontal strips.  Both
// go through one workspace prologue (launch_workspace) and one FillArgs base
// (base_args).
#include <algorithm>
#include <cstring>

#include "nw_host_int.h"

using namespace nwh;

namespace {

bool fits_i8(int32_t x) { return x >= -128 && x <= 127; }

}  // namespace

namespace nwh {  // (shared with the checkpoint sweep's launch, nw_ckpt.cpp)

// The kernels hold w = t - GAP*(i+j) in int32 next to a "minus infinity" of
// -2^29: |w| <= (max|score| + |GAP|) * (i + j) must stay below 2^28, with i_max the
// last GLOBAL row (a band's halo row carries the values of row band->row0).  The same
// bound holds for Smith-Waterman: its cells are in the w form too (strips: the
// 0 floor becomes z = -GAP*(i+j); panels: u = t - GAP*j), so |w|, |z| and the
// store waves' GAP*(i+j) reach (max|score| + |GAP|) * (n1 + n2 + 2) although t
// itself stays in [0, max|score| * (min(n1, n2) + 1)].
bool w_range_ok(const nw_params *p, int64_t n1, int64_t i_max) {
    const long long m = std::max({std::llabs(p->match), std::llabs(p->mismatch), std::llabs(p->gap)});
    return (m + std::llabs(p->gap)) * (long long)(n1 + i_max + 2) < (1LL << 28);
}

// The affine-gap batch kernels hold H', E' and F' (each minus ge*(i+j)) next to the
// same -2^29.  With m = max|score| (ge included) and go = gap_open <= 0:  H <= m*(i+j)
// and H >= 2 go - |ge|*(i+j) (one run up, one run left), so |H'| <= 2|go| + (m +
// |ge|)*(i+j);  E and F lie between H_neighbour + go + ge and H, one more |go|; the
// intermediates H' + go and H'_diag + s - 2ge stay within that.  The -2^29 is never
// added to.  So 3|go| + (m + |ge|)*(n1 + i_max + 2) < 2^28 keeps every real value
// above -2^28, where it beats the -2^29 in every maximum, and far from overflow.
bool affine_range_ok(const nw_params *p, int32_t gap_open, int64_t n1, int64_t i_max) {
    const long long m = std::max({std::llabs(p->match), std::llabs(p->mismatch), std::llabs(p->gap)});
    return 3 * std::llabs((long long)gap_open) + (m + std::llabs(p->gap)) * (long long)(n1 + i_max + 2) < (1LL << 28);
}

// The matrix kernels are the affine ones with s read from an int8 matrix: the bound is
// affine_range_ok's with the matrix's largest |entry| (max_abs, over the n letters) in
// the place of match / mismatch.  Nothing else in the argument above depends on s.
bool matrix_range_ok(const nw_params *p, int32_t gap_open, int64_t max_abs, int64_t n1, int64_t i_max) {
    const long long m = std::max<long long>(max_abs, std::llabs(p->gap));
    return 3 * std::llabs((long long)gap_open) + (m + std::llabs(p->gap)) * (long long)(n1 + i_max + 2) < (1LL << 28);
}

// The two-piece kernels hold H, E1, F1, E2 and F2 minus ge1 * (i + j).  With G = max(|go1|,
// |go2|), A = max(|ge1|, |ge2|) and M = max(A, max_abs): every path to (i, j) has at most i +
// j steps, each worth at most M in absolute value, plus openings; H is at least the score of
// the path "one run up, one run left" (two openings) and at most M * (i + j) (openings are
// <= 0), an Et or Ft is at most H and at least a neighbour's H plus one opening and one
// extension: |X| <= 3 G + M * (i + j + 1) for all five.  The form subtracts ge1 * (i + j),
// which costs at most A * (i + j) more -- this covers the drift of the piece-2 values, which
// is (ge2 - ge1) per step only relative to values that drift by -ge1 themselves -- and the
// cell's sums (H' + go_t, H'_diag + s - 2 ge1, max(..) + ge2 - ge1) add at most one opening
// or 2 A + M once, the "+ 2".  So the matrix bound with G and A in the place of |gap_open|
// and |gap| keeps every real value above -2^28, and the -2^29 is added to at most once.
bool dual_range_ok(const nw_params *p, int32_t gap_open, int32_t gap_open2, int32_t gap2, int64_t max_abs, int64_t n1,
                   int64_t i_max) {
    const long long g = std::max(std::llabs((long long)gap_open), std::llabs((long long)gap_open2));
    const long long a = std::max(std::llabs((long long)p->gap), std::llabs((long long)gap2));
    const long long m = std::max<long long>(max_abs, a);
    return 3 * g + (m + a) * (long long)(n1 + i_max + 2) < (1LL << 28);
}

// v_perm score tables when every substitution score minus `off` fits int8 (the
// kernel falls back to compares on the device when s1 holds more than kMaxPerm
// distinct characters).  off: the table bytes are s - 2 GAP in the w form (NW, and
// SW in the strips), s - GAP for SW in the panels (the u form).
bool perm_allowed(const nw_params *p, int32_t off) {
    return fits_i8(p->match - off) && fits_i8(p->mismatch - off) && !(p->flags & NW_FLAG_NO_PROFILE);
}

// The context's workspace for one launch of `s` that consumes `ntags` hand-off tags
// over nbl row blocks; on NW_OK *qlen = row-pack entries per block.
int launch_workspace(nw_ctx *c, const Shape &s, uint64_t ntags, int32_t nbl, void *stream, int64_t *qlen) {
    int st;
    // Hand-off granules.  (Re)allocation zeroes them; tags are then unique per
    // (launch, strip) as long as tagbase does not wrap -- re-zero when it would.
    // A new buffer is zeroed on the launch stream (ordered before the kernels
    // on any stream, also a non-blocking one): reused device memory may
    // still hold granules whose tags match this context's fresh tagbase.
    const size_t gran_need = (size_t)(s.M * s.gstride) * sizeof(uint64_t);
    bool fresh = false;
    if ((st = grow((void **)&c->gran, &c->gran_cap, gran_need, &fresh)) != NW_OK) return st;
    // tags run up to tagbase + ntags (strip0 + nstrips * nbl: p is the GLOBAL strip index)
    if (fresh || (uint64_t)c->tagbase + ntags + 2u >= 0xFFFFFFF0ull) {
        NW_HIP_TRY(hipMemsetAsync(c->gran, 0, c->gran_cap, (hipStream_t)stream));
        c->tagbase = 1;
    }
    *qlen = nw::rowpack_len((int32_t)s.nblocks);
    if ((st = grow((void **)&c->rowpack, &c->rowpack_cap, (size_t)*qlen * 16 * nbl)) != NW_OK) return st;
    if ((st = grow((void **)&c->scratch, &c->scratch_cap, (size_t)s.waves * nw::kScratchWords * 4)) != NW_OK)
        return st;
    // per-launch control words: reset, keeping a failure not yet reported (nw_link.hip nw_ctrl_reset)
    return nw::launch_ctrl_reset(c->ctrl, stream) == hipSuccess ? NW_OK : NW_ERR_HIP;
}

}  // namespace nwh

namespace {

// What every launch's FillArgs takes from the context, the shape and the
// parameters (after launch_workspace: it may restart tagbase); one table
// (nbl = 1, hin0 = 1), everything else zero.
nw::FillArgs base_args(const nw_ctx *c, const Shape &s, const nw_params *p, bool perm_ok, int64_t qlen,
                       int64_t n1) {
    nw::FillArgs a;
    std::memset(&a, 0, sizeof a);
    a.rowpack = c->rowpack;
    a.nstrips = (int32_t)s.nstrips;
    a.nblocks = (int32_t)s.nblocks;
    a.gran = c->gran;
    a.gstride = s.gstride;
    a.M = (int32_t)s.M;
    a.tagbase = c->tagbase;
    a.ctrl = c->ctrl;
    a.scratch = c->scratch;
    a.perm = perm_ok ? 1 : 0;
    a.charmap = c->meta;
    a.nprof = (const uint32_t *)(c->meta + 256);
    a.trace = c->trace;
    a.match = p->match;
    a.mismatch = p->mismatch;
    a.gap = p->gap;
    a.flags = p->flags;
    a.timeout_ticks = timeout_ticks(p->timeout_ms);
    a.nbl = 1;
    a.hin0 = 1;
    a.qstride = qlen * 16;
    a.hstride = n1 + 1;
    return a;
}

void record_launch(nw_ctx *c, const Shape &s, int64_t col0) {
    c->last_waves = (int)s.waves;
    c->last_strips = (int)s.nstrips;
    c->last_sub = s.K;
    c->last_nc = s.NC;
    c->last_col0 = (int)col0;
    c->last_kernel = s.kernel;
}

int launch_fill(nw_ctx *c, const int8_t *d_s1, int64_t n1, const int8_t *d_s2, int64_t n2, const nw_params *p,
                const nw_band *band, const nw_colband *cb, int32_t *d_t, int64_t pitch, void *stream,
                const nw_band_cycle *cy = nullptr) {
    if (!c || !d_t || n1 < 0 || n2 < 0 || n1 >= INT32_MAX || n2 >= INT32_MAX) return NW_ERR_ARG;
    // block-cyclic row bands: nbl blocks of n2 + 1 rows, checked as a band whose
    // row 0 is the largest of the blocks'
    nw_band cyb;
    const int32_t nbl = cy ? cy->nblk : 1;
    if (cy) {
        if (band || cb || cy->nblk < 1 || (cy->hin_first & ~1) != 0 || (cy->hout_shift & ~1) != 0 ||
            cy->row0_max < 0 || cy->row0_max >= INT32_MAX)
            return NW_ERR_ARG;
        if (!cy->halo_in && (cy->hin_first || cy->nblk > 1)) return NW_ERR_ARG;
        if (cy->nblk > 1 && (cy->t_stride < (n2 + 1) * pitch || cy->t_stride % nw::kWave != 0)) return NW_ERR_ARG;
        if ((int64_t)nbl * n2 >= INT32_MAX) return NW_ERR_ARG;
        cyb.halo_in = cy->halo_in;
        cyb.halo_out = cy->halo_out;
        cyb.tag = cy->tag;
        cyb.row0 = (uint32_t)cy->row0_max;
        band = &cyb;
    }
    if ((n1 > 0 && !d_s1) || (n2 > 0 && !d_s2)) return NW_ERR_ARG;
    if (!valid_params(p)) return NW_ERR_ARG;
    const bool sw = p->mode == NW_MODE_SW;
    if (sw && (band || cb)) return NW_ERR_UNSUPPORTED;  // (local alignment: single table, config 5)
    // the unchained probe leaves no valid table, so no best cell / locate either
    if (sw && (p->flags & NW_FLAG_DEBUG_NO_CHAIN)) return NW_ERR_ARG;
    if ((p->flags & NW_FLAG_DEBUG_NO_CHAIN) && (band || cb)) return NW_ERR_ARG;  // (no fill to hand on)
    if (band && cb) return NW_ERR_ARG;
    if (!w_range_ok(p, n1, n2 + (band ? (int64_t)band->row0 : 0))) return NW_ERR_ARG;
    int64_t col0;
    int64_t strip_first = 0, strip_count = 0, start = 0;
    if (cb) {
        // a column band's local table: the nw_table_offset layout over its n_cols
        // columns (local column 1 starts a 256-byte line, as in every band)
        if (cb->tag == 0 || (((uintptr_t)cb->feed_in | (uintptr_t)cb->feed_out) & 7u) != 0) return NW_ERR_ARG;
        int64_t ncols = 0;
        int st0 = colband_layout(n1, n2, cb->nbands, cb->r, p, c->cus, &strip_first, &strip_count, &start, &ncols);
        if (st0 != NW_OK) return st0;
        if ((cb->r > 0) != (cb->feed_in != nullptr) || (cb->r + 1 < cb->nbands) != (cb->feed_out != nullptr))
            return NW_ERR_ARG;
        if (cb->feed_out && (p->flags & 1)) return NW_ERR_ARG;  // needs the real right column
        if ((((uintptr_t)d_t + 4u) & 255u) != 0 || pitch % nw::kWave != 0 || pitch < ncols + 3) return NW_ERR_ARG;
        col0 = 1;
    } else {
        // any 64-multiple pitch that holds nCols = n1 + 1 (nw_table_pitch adds the
        // slack that lets the strips start at column 1)
        if (pitch < n1 + 1 || pitch % nw::kWave != 0) return NW_ERR_ARG;
        // Strip origin: column 1 when the base is laid out so that column 1 starts a
        // 256-byte line (nw_table_offset), which takes the boundary column 0 out of
        // the sweep; column 0 for a 256-byte aligned base.  Anything else is refused.
        if ((((uintptr_t)d_t + 4u) & 255u) == 0 && n1 >= 1 && pitch >= n1 + 4)
            col0 = 1;
        else if (((uintptr_t)d_t & 255u) == 0)
            col0 = 0;
        else
            return NW_ERR_ARG;
    }
    if (band) {
        if (band->tag == 0 || (((uintptr_t)band->halo_in | (uintptr_t)band->halo_out) & 7u) != 0)
            return NW_ERR_ARG;
        if (band->halo_out && (p->flags & 1)) return NW_ERR_ARG;  // needs the real last row
    }
    NW_HIP_TRY(hipSetDevice(c->device));
    Shape s = make_shape(n1, n2, p->waves, p->substrips, p->strip_waves, c->cus, col0, sw,
                         band || cb ? band_kernel(p->kernel) : p->kernel);
    if (!shape_valid(s)) return NW_ERR_ARG;
    const bool panels = s.kernel == NW_KERNEL_PANELS;
    if (cy && panels) return NW_ERR_UNSUPPORTED;  // (block cycles: the strip kernel)
    if (panels && (p->flags & NW_FLAG_DEBUG_NO_CHAIN)) return NW_ERR_ARG;  // (a strip-kernel probe)
    if ((int64_t)s.nstrips * nbl > INT32_MAX / 2) return NW_ERR_ARG;
    if (nbl > 1) {  // the launch's chain of hand-offs is nstrips * nbl tickets long
        s.waves = std::max<int64_t>(1, std::min<int64_t>(s.waves_max, s.nstrips * nbl));
        s.M = std::min<int64_t>(s.nstrips * nbl, s.waves + 1);
    }
    if (cb) {  // this launch sweeps its band's strips only
        s.nstrips = strip_count;
        s.waves = std::max<int64_t>(1, std::min<int64_t>(s.waves_max, s.nstrips));
        s.M = std::min<int64_t>(s.nstrips, s.waves + 1);
    }
    if (sw && !panels && !nw::sw_shape_ok(s.K, s.NC)) return NW_ERR_UNSUPPORTED;
    // (2, 4): half-word rings, Smith-Waterman only, with at most kHalfFixMax cells of
    // the corner where t may reach 2^16 (nw_sw.hip nw_sw_fixup)
    const bool half = !panels && s.K == 2 && s.NC == 4;
    if (half) {
        int64_t k = 0;
        if (!sw || nw::sw_half_corner(p->match, p->mismatch, n1, n2, &k) > nw::kHalfFixMax) return NW_ERR_UNSUPPORTED;
    }
    if (s.nstrips > INT32_MAX / 2 || s.nblocks > INT32_MAX / 2) return NW_ERR_ARG;

    int st;
    int64_t qlen = 0;
    const uint64_t ntags = (uint64_t)strip_first + (uint64_t)s.nstrips * nbl;
    if ((st = launch_workspace(c, s, ntags, nbl, stream, &qlen)) != NW_OK) return st;
    const uint8_t *s1u = n1 > 0 ? (const uint8_t *)d_s1 : (const uint8_t *)c->ctrl;
    const uint8_t *s2u = n2 > 0 ? (const uint8_t *)d_s2 : (const uint8_t *)c->ctrl;
    const bool perm_ok = perm_allowed(p, sw && panels ? p->gap : 2 * p->gap);
    if (sw) {
        // per-strip best cells (zeroed on the launch stream) + best / key words
        const size_t need = (size_t)(s.nstrips + 8) * sizeof(int32_t);
        if ((st = grow((void **)&c->smax, &c->smax_cap, need)) != NW_OK) return st;
        NW_HIP_TRY(hipMemsetAsync(c->smax, 0, need, (hipStream_t)stream));
    }
    for (int32_t b = 0; b < nbl; ++b)  // (block b's side characters: s2 + b * n2)
        if (nw::launch_rowpack(s1u, n1, s2u + (n2 > 0 ? (int64_t)b * n2 : 0), n2, 0, perm_ok ? 1 : 0, c->meta,
                               (char *)c->rowpack + (int64_t)b * qlen * 16, qlen, stream) != hipSuccess)
            return NW_ERR_HIP;

    nw::FillArgs a = base_args(c, s, p, perm_ok, qlen, n1);
    a.table = d_t - start;  // table + c = global column c (start = 0 but for column bands)
    a.pitch = pitch;
    a.col_end = start + pitch;
    a.strip0 = (int32_t)strip_first;
    a.feed_in = cb ? cb->feed_in : nullptr;
    a.feed_out = cb ? cb->feed_out : nullptr;
    a.feed_tag = cb ? cb->tag : 0u;
    a.s1 = s1u;
    a.n1 = n1;
    a.n2 = n2;
    a.col0 = col0;
    a.halo_in = band ? band->halo_in : nullptr;
    a.halo_out = band ? band->halo_out : nullptr;
    a.halo_tag = band ? band->tag : 0u;
    a.sw = sw ? 1 : 0;
    a.smax = sw ? c->smax : nullptr;
    if (cy) {
        a.nbl = nbl;
        a.hin0 = cy->hin_first;
        a.hoshift = cy->hout_shift;
        a.tstride = cy->t_stride;
    }
    if ((panels ? nw::launch_panels(a, s.K, s.NC, (int)s.waves, stream)
                : nw::launch_fill(a, s.K, s.NC, (int)s.waves, stream)) != hipSuccess)
        return NW_ERR_HIP;
    // a column band's local column 0 (band r-1's last column) from its feed
    if (cb && cb->feed_in &&
        nw::launch_colband_edge(cb->feed_in, d_t, pitch, n2, p->gap, start, stream) != hipSuccess)
        return NW_ERR_HIP;
    c->tagbase += (uint32_t)ntags + 1u;
    record_launch(c, s, col0);
    if (sw) {
        // best cell: max over the strips, then the first row-major cell holding it
        if (!c->swinfo) NW_HIP_TRY(hipMalloc(&c->swinfo, 16 * sizeof(int64_t)));  // [0..9] traceback info, [12] locate key
        int32_t *best = c->smax + s.nstrips;
        uint64_t *key = (uint64_t *)(c->swinfo + 12);
        // (TIMING_ONLY: the strips stored into a scratch tile and the caller's table
        // was never written, so there is no corner to fix up in it)
        if (half && !(p->flags & NW_FLAG_TIMING_ONLY) && nw::launch_sw_fixup(d_t, pitch, n1, n2, (const uint8_t *)d_s1, (const uint8_t *)d_s2, p->match,
                                        p->mismatch, p->gap, col0, (int32_t)(nw::kWave * s.K * s.NC), c->smax,
                                        stream) != hipSuccess)
            return NW_ERR_HIP;
        if (nw::launch_sw_locate(d_t, pitch, n1, n2, col0, (int32_t)(nw::kWave * s.K * s.NC), c->smax,
                                 (int32_t)s.nstrips, key, best, stream) != hipSuccess)
            return NW_ERR_HIP;
    }
    return NW_OK;
}

// Rows Rs + 1 .. Rs + L of a horizontal-strip band (the strips swept Rs), by the
// row-scan finisher after the strips; it publishes the band's last row.
int launch_finisher(nw_ctx *c, const int8_t *d_s1, int64_t n1, const int8_t *d_s2, const nw_params *p,
                    const nw_tband *tb, int32_t *d_t, int64_t pitch, int64_t L, int64_t Rs, uint64_t ticks,
                    void *stream) {
    nw::FinishArgs f;
    std::memset(&f, 0, sizeof f);
    // debug (tests): NW_DEBUG_FINISH_WIDE=1 forces the 8192-column chunks (K = 32),
    // otherwise only chosen above 8 chunks per CU (~4.2M columns on 256 CUs)
    f.chunk_cols = nw::finish_chunk_cols(env_flag("NW_DEBUG_FINISH_WIDE") ? INT64_MAX / 4 : n1, c->cus);
    f.nchunks = (int32_t)((n1 + f.chunk_cols - 1) / f.chunk_cols);
    const size_t need = (size_t)L * (size_t)f.nchunks * sizeof(uint64_t);
    bool fresh = false;
    int st;
    if ((st = grow((void **)&c->look, &c->look_cap, need, &fresh)) != NW_OK) return st;
    if (fresh || (uint64_t)c->look_tag + 2u * (uint64_t)L + 2u >= 0xFFFFFFF0ull) {
        NW_HIP_TRY(hipMemsetAsync(c->look, 0, c->look_cap, (hipStream_t)stream));
        c->look_tag = 1;
    }
    f.table = d_t;
    f.pitch = pitch;
    f.s1 = (const uint8_t *)d_s1;
    f.n1 = n1;
    f.s2 = (const uint8_t *)d_s2;
    f.li0 = Rs + 1;
    f.nrows = L;
    f.grow0 = tb->row0;
    f.match = p->match;
    f.mismatch = p->mismatch;
    f.gap = p->gap;
    f.look = c->look;
    f.tag0 = c->look_tag;
    f.ctrl = c->ctrl;
    f.feed_out = tb->feed_out;
    f.feed_tag = tb->tag;
    f.timeout_ticks = ticks;
    if (nw::launch_finish_rows(f, stream) != hipSuccess) return NW_ERR_HIP;
    c->look_tag += 2u * (uint32_t)L + 2u;
    return NW_OK;
}

// the unfed leading (4, 1) strip of a horizontal band sleeps this many x 64 clocks
// per 64-step iteration (FillArgs::lead_sleep)
constexpr int kTbandLeadSleep = 8;

}  // namespace

extern "C" {

int nw_fill_device_async(nw_ctx *c, const int8_t *d_s1, int64_t n1, const int8_t *d_s2,
                         int64_t n2, const nw_params *p, int32_t *d_t, int64_t pitch,
                         void *stream) {
    return launch_fill(c, d_s1, n1, d_s2, n2, p, nullptr, nullptr, d_t, pitch, stream);
}

int nw_fill_band_async(nw_ctx *c, const int8_t *d_s1, int64_t n1, const int8_t *d_s2_band,
                       int64_t n2_band, const nw_params *p, const nw_band *band, int32_t *d_t,
                       int64_t pitch, void *stream) {
    if (!band) return NW_ERR_ARG;
    return launch_fill(c, d_s1, n1, d_s2_band, n2_band, p, band, nullptr, d_t, pitch, stream);
}

int nw_fill_band_cycle_async(nw_ctx *c, const int8_t *d_s1, int64_t n1, const int8_t *d_s2_blocks,
                             int64_t n2_blk, const nw_params *p, const nw_band_cycle *cy, int32_t *d_t,
                             int64_t pitch, void *stream) {
    if (!cy) return NW_ERR_ARG;
    return launch_fill(c, d_s1, n1, d_s2_blocks, n2_blk, p, nullptr, nullptr, d_t, pitch, stream, cy);
}

int nw_fill_colband_async(nw_ctx *c, const int8_t *d_s1, int64_t n1, const int8_t *d_s2, int64_t n2,
                          const nw_params *p, const nw_colband *band, int32_t *d_t, int64_t pitch,
                          void *stream) {
    if (!band) return NW_ERR_ARG;
    return launch_fill(c, d_s1, n1, d_s2, n2, p, nullptr, band, d_t, pitch, stream);
}

// Row band in horizontal strips: the (4, 1) strip kernel on the TRANSPOSED band
// (the NW table of (s2_band, s1) is the band's transpose, the scores being
// symmetric), in global row numbers: its "columns" are global rows row0 + 1 ..
// row0 + R (strips of 256 rows from row0 + 1), its "rows" the band's columns
// 0..n1; the store waves write the row-major band table (store_strip_tr).
int nw_fill_tband_async(nw_ctx *c, const int8_t *d_s1, int64_t n1, const int8_t *d_s2, int64_t R,
                        const nw_params *p, const nw_tband *tb, int32_t *d_t, int64_t pitch, void *stream) {
    if (!c || !d_t || !tb || !d_s1 || !d_s2 || n1 < 1 || R < 1 || n1 >= INT32_MAX || R >= INT32_MAX ||
        tb->row0 < 0 || tb->row0 + R >= INT32_MAX)
        return NW_ERR_ARG;
    if (!valid_params(p)) return NW_ERR_ARG;
    // shapes: (4, 1) (the default) or (2, 2) -- 256-row strips either way
    if (p->mode != NW_MODE_NW || p->kernel == NW_KERNEL_PANELS) return NW_ERR_UNSUPPORTED;
    int tC = 4, tNC = 1;
    if (p->substrips != 0 || p->strip_waves != 0) {
        tC = p->substrips ? p->substrips : 4;
        tNC = p->strip_waves ? p->strip_waves : 1;
        if (!((tC == 4 && tNC == 1) || (tC == 2 && tNC == 2))) return NW_ERR_UNSUPPORTED;
    }
    if (tb->tag == 0 || (((uintptr_t)tb->feed_in | (uintptr_t)tb->feed_out) & 7u) != 0) return NW_ERR_ARG;
    if ((tb->flags & ~(uint32_t)NW_TBAND_DENSE_POLLS) != 0) return NW_ERR_ARG;
    if ((tb->row0 > 0) != (tb->feed_in != nullptr)) return NW_ERR_ARG;
    if (tb->feed_out && (p->flags & 1)) return NW_ERR_ARG;  // needs the real last row
    if ((p->flags & NW_FLAG_DEBUG_NO_CHAIN) && (tb->feed_in || tb->feed_out)) return NW_ERR_ARG;  // (no fill to hand on)
    if ((((uintptr_t)d_t + 4u) & 255u) != 0 || pitch % nw::kWave != 0 || pitch < n1 + 4) return NW_ERR_ARG;
    if (!w_range_ok(p, n1, tb->row0 + R)) return NW_ERR_ARG;  // (with the global row)
    NW_HIP_TRY(hipSetDevice(c->device));
    // the transposed band: R + 1 "columns" (global rows row0 .. row0 + R, the first
    // one the feed), n1 + 1 "rows" (the band's columns)
    Shape s = make_shape(R, n1, p->waves, tC, tNC, c->cus, 1, false, NW_KERNEL_STRIPS);
    if (!shape_valid(s) || s.nstrips > INT32_MAX / 2 || s.nblocks > INT32_MAX / 2) return NW_ERR_ARG;
    // Leftover rows: when the band's last strip would run ALONE as one more pass over
    // all n1 columns (strips = k * workers + 1, e.g. config 4's last band: 65537 rows =
    // 257 strips on 256 CUs), its rows are computed by the row-scan finisher after the
    // strips instead (nw_finish.hip: one prefix-max scan per row across the width).
    int64_t Rs = R, L = 0;
    if (s.nstrips > s.waves && (s.nstrips - 1) % s.waves == 0 && !(p->flags & NW_FLAG_NO_FINISH) &&
        !(p->flags & 1)) {
        L = R - 256 * (s.nstrips - 1);
        Rs = R - L;
        s = make_shape(Rs, n1, p->waves, tC, tNC, c->cus, 1, false, NW_KERNEL_STRIPS);
        if (!shape_valid(s)) return NW_ERR_ARG;
    }
    int st;
    int64_t qlen = 0;
    const uint64_t ntags = (uint64_t)s.nstrips;
    if ((st = launch_workspace(c, s, ntags, 1, stream, &qlen)) != NW_OK) return st;
    const bool perm_ok = perm_allowed(p, 2 * p->gap);
    // lanes carry the band's row characters (charmap of s2_band), the row packs the columns' (s1)
    if (nw::launch_rowpack((const uint8_t *)d_s2, R, (const uint8_t *)d_s1, n1, 0, perm_ok ? 1 : 0, c->meta,
                           c->rowpack, qlen, stream) != hipSuccess)
        return NW_ERR_HIP;
    nw::FillArgs a = base_args(c, s, p, perm_ok, qlen, n1);
    a.table = d_t;
    a.pitch = pitch;
    a.col_end = INT64_MAX;
    a.feed_in = tb->feed_in;
    a.feed_out = L > 0 ? nullptr : tb->feed_out;  // (with a finisher, it publishes the last row)
    a.feed_tag = tb->tag;
    a.s1 = (const uint8_t *)d_s2 - tb->row0;  // s1[y - 1] = global row y's character
    a.n1 = tb->row0 + Rs;                     // global last row the strips sweep
    a.n2 = n1;
    a.col0 = tb->row0 + 1;                    // first swept global row
    a.tr = 1;
    a.tr_y0 = tb->row0;
    a.tr_pub = (int32_t)(Rs - 1 - 256 * (s.nstrips - 1));  // the last row's column in the last strip
    static const bool compute_pub = env_flag("NW_TR_PUB_COMPUTE");
    a.tr_store_pub = compute_pub && tNC == 1 ? 0 : 1;  // ((2, 2): the store waves publish)
    // With sparse polls the band's unfed leading strip (band 0's strip 0: the whole
    // chain's leader) sleeps 8 x 64 clocks per 64-step iteration (~8 %): followers that
    // run 1-2 % slower for a while then keep up instead of delaying every strip below
    // them (mean strip-to-strip lag 16.3-17.4 -> 12.5 us, leader 25.8 -> 27.0-28.0 ms;
    // profiles/r06f_lead_sleep.txt).  Dense polls slow the leader by themselves and
    // need no throttle (lag 10.0 us at a leader of 28.0-28.5 ms with none, 29.7-29.8
    // with 8: profiles/r06n_lead_dense.txt).  NW_LEAD_SLEEP overrides both (A/B).
    a.tr_dense = (tb->flags & NW_TBAND_DENSE_POLLS) != 0 ? 1 : 0;
    static const int lead_env = env_int("NW_LEAD_SLEEP", -1);
    a.lead_sleep = lead_env >= 0 ? lead_env : tNC != 1 ? 0 : a.tr_dense ? 0 : kTbandLeadSleep;
    if (nw::launch_fill(a, tC, tNC, (int)s.waves, stream) != hipSuccess) return NW_ERR_HIP;
    if (nw::launch_tband_edges(tb->feed_in, d_t, pitch, n1, R + 1, p->gap, tb->row0, stream) != hipSuccess)
        return NW_ERR_HIP;
    c->tagbase += (uint32_t)ntags + 1u;
    c->last_finish_rows = (int)L;
    if (L > 0 && (st = launch_finisher(c, d_s1, n1, d_s2, p, tb, d_t, pitch, L, Rs, a.timeout_ticks, stream)) != NW_OK)
        return st;
    record_launch(c, s, 1);
    return NW_OK;
}

int nw_fill_device(nw_ctx *c, const int8_t *d_s1, int64_t n1, const int8_t *d_s2, int64_t n2,
                   const nw_params *p, int32_t *d_t, int64_t pitch, void *stream,
                   nw_result *out) {
    if (!c) return NW_ERR_ARG;
    NW_HIP_TRY(hipSetDevice(c->device));
    if (out) NW_HIP_TRY(hipEventRecord(c->ev0, (hipStream_t)stream));
    int st = nw_fill_device_async(c, d_s1, n1, d_s2, n2, p, d_t, pitch, stream);
    if (st != NW_OK || !out) return st;
    NW_HIP_TRY(hipEventRecord(c->ev1, (hipStream_t)stream));
    st = nw_ctx_status(c, stream);
    std::memset(out, 0, sizeof *out);
    out->status = st;
    float ms = 0.f;
    NW_HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    out->kernel_ms = ms;
    out->cells = n1 * n2;
    out->table_bytes = (double)(n1 + 1) * (double)(n2 + 1) * 4.0;
    out->strips = c->last_strips;
    out->waves = c->last_waves;
    out->substrips = c->last_sub;
    out->strip_waves = c->last_nc;
    out->kernel = c->last_kernel;
    int32_t score = 0;
    if (p->mode == NW_MODE_SW) {
        // best cell (nw_sw.hip locate): score and its first row-major position
        uint64_t key = 0;
        NW_HIP_TRY(hipMemcpy(&score, c->smax + c->last_strips, 4, hipMemcpyDeviceToHost));
        NW_HIP_TRY(hipMemcpy(&key, c->swinfo + 12, 8, hipMemcpyDeviceToHost));
        out->end_i = score > 0 ? (int64_t)(key >> 32) : 0;
        out->end_j = score > 0 ? (int64_t)(key & 0xFFFFFFFFull) : 0;
    } else {
        NW_HIP_TRY(hipMemcpy(&score, d_t + n2 * pitch + n1, 4, hipMemcpyDeviceToHost));
        out->end_i = n2;
        out->end_j = n1;
    }
    out->score = score;
    return st;
}

}  // extern "C"
