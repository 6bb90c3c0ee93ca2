// nw_batch.cpp -- batched pairwise global alignment: the checks, the longest-first
// order, the launches of the batch kernels (nw_batch.hip), nw_score_batch_async,
// nw_score_batch and nw_align_batch (the directions kernel and the walk, in chunks
// that fit the device budget).  The affine-gap entries (nw_score_batch_affine_async,
// nw_score_batch_affine, nw_align_batch_affine; kernels in nw_batch_affine.hip) are
// the same three bodies: a Cost tells them which kernels to launch and that a worker's
// column scratch and a pair's direction bytes are twice the linear ones.  The matrix
// entries (nw_score_batch_matrix_async, nw_score_batch_matrix, nw_align_batch_matrix;
// kernels in nw_batch_matrix.hip) are the affine ones with the substitution read from an
// nw_submat: the Cost carries the matrix, batch_prepare maps the rows through its index
// instead of running the charmap, and batch_run launches the matrix sweep.  The local
// entries (nw_score_batch_local_async, nw_score_batch_local, nw_align_batch_local; kernels
// in nw_batch_local.hip) are the matrix ones in mode NW_MODE_SW: a pair's result is an
// nw_local_hit where the others have an int32 score, the matrix goes into the arguments
// as it is, and the walk starts at the hit the sweep left on the device.  The semi-global
// entries (nw_score_batch_semi_async, nw_score_batch_semi, nw_align_batch_semi; kernels in
// nw_batch_semi.hip) are the matrix ones with an `ends` set: mode, matrix bytes, range and
// refusals as there, hits as the result like the local ones, and empty pairs answered here
// from the definition.  The banded entries (nw_score_batch_banded_async, nw_score_batch_
// banded, nw_align_batch_banded; kernels in nw_batch_banded.hip) are the matrix ones with a
// band width: the Cost carries it, a pair's direction bytes are nw_batch_banded_dir_bytes,
// and the sweep and the walk are that file's.  The two-piece entries (nw_score_batch_dual_
// async, nw_score_batch_dual, nw_align_batch_dual; kernels in nw_batch_dual.hip) are the
// matrix ones with a second (open, extend) piece: the Cost carries it, a worker's column
// scratch is three columns, a pair's direction bytes are nw_batch_dual_dir_bytes, and the
// sweep and the walk are that file's.  The two-piece banded entries (nw_score_batch_dual_banded_
// async, nw_score_batch_dual_banded, nw_align_batch_dual_banded; kernels in nw_batch_dual_
// banded.hip) are the two-piece ones with a band width: the Cost is both dual and banded, a
// pair's direction bytes are nw_batch_dual_banded_dir_bytes.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "nw_batch.h"
#include "nw_host_int.h"

using namespace nwh;

namespace {

// the gap cost of a call: linear (L * gap) or affine (open + L * gap); the
// substitution: match / mismatch, or a matrix
struct Cost {
    bool affine = false;
    int32_t open = 0;
    bool matrix = false;  // substitution by *mat (affine is then true): matrix_cost()
    const nw_submat *mat = nullptr;
    int64_t mat_abs = 0;  // max |score[x][y]| over x, y < n
    bool local = false;   // Smith-Waterman (matrix is then true): a result is an nw_local_hit
    bool semi = false;    // free end gaps per side (matrix is then true): a result is an nw_local_hit
    int32_t ends = 0;     // semi: NW_ENDS_* bits
    bool banded = false;  // cells within `band` diagonals only (matrix is then true)
    int32_t band = 0;
    bool dual = false;  // gap cost max(open + L * gap, open2 + L * gap2) (matrix is then true)
    int32_t open2 = 0, gap2 = 0;
    bool hits() const { return local || semi; }
    size_t out_bytes() const { return hits() ? sizeof(nw_local_hit) : sizeof(int32_t); }
    int64_t col_words(int64_t max_n2) const { return nw::batch_col_words(max_n2) * (dual ? 3 : affine ? 2 : 1); }
    int64_t dir_bytes(int64_t n1, int64_t n2) const {
        if (banded && dual) return nw_batch_dual_banded_dir_bytes(n1, n2, band);
        if (banded) return nw_batch_banded_dir_bytes(n1, n2, band);
        if (dual) return nw_batch_dual_dir_bytes(n1, n2);
        return affine ? nw_batch_affine_dir_bytes(n1, n2) : nw_batch_dir_bytes(n1, n2);
    }
    // a pair without cells: one run along the boundary
    int32_t empty_score(const nw_params *p, int64_t n) const {
        const int64_t g1 = (n > 0 ? open : 0) + p->gap * n;
        return (int32_t)(dual && n > 0 ? std::max<int64_t>(g1, open2 + gap2 * n) : g1);
    }
    bool range_ok(const nw_params *p, int64_t n1, int64_t i_max) const {
        if (dual) return dual_range_ok(p, open, open2, gap2, mat_abs, n1, i_max);
        if (matrix) return matrix_range_ok(p, open, mat_abs, n1, i_max);
        return affine ? affine_range_ok(p, open, n1, i_max) : w_range_ok(p, n1, i_max);
    }
};

// a matrix the kernels can index without a bounds test: n letters, every byte mapped
// to one of them
bool valid_submat(const nw_submat *m) {
    if (!m || m->n < 1 || m->n > NW_SUBMAT_MAX) return false;
    for (int k = 0; k < 3; ++k)
        if (m->reserved[k] != 0) return false;
    for (int b = 0; b < 256; ++b)
        if (m->index[b] >= m->n) return false;
    return true;
}

Cost matrix_cost(const nw_submat *m, int32_t gap_open) {
    Cost c;
    c.affine = c.matrix = true;
    c.open = gap_open;
    c.mat = m;
    if (valid_submat(m))  // (an invalid one is refused by params_check before the range is looked at)
        for (int x = 0; x < m->n; ++x)
            for (int y = 0; y < m->n; ++y)
                c.mat_abs = std::max<int64_t>(c.mat_abs, std::abs((int)m->score[x * NW_SUBMAT_MAX + y]));
    return c;
}

Cost local_cost(const nw_submat *m, int32_t gap_open) {
    Cost c = matrix_cost(m, gap_open);
    c.local = true;
    return c;
}

Cost semi_cost(const nw_submat *m, int32_t gap_open, int32_t ends) {
    Cost c = matrix_cost(m, gap_open);
    c.semi = true;
    c.ends = ends;
    return c;
}

Cost banded_cost(const nw_submat *m, int32_t gap_open, int32_t band) {
    Cost c = matrix_cost(m, gap_open);
    c.banded = true;
    c.band = band;
    return c;
}

Cost dual_cost(const nw_submat *m, int32_t gap_open, int32_t gap_open2, int32_t gap2) {
    Cost c = matrix_cost(m, gap_open);
    c.dual = true;
    c.open2 = gap_open2;
    c.gap2 = gap2;
    return c;
}

Cost dual_banded_cost(const nw_submat *m, int32_t gap_open, int32_t gap_open2, int32_t gap2, int32_t band) {
    Cost c = dual_cost(m, gap_open, gap_open2, gap2);
    c.banded = true;
    c.band = band;
    return c;
}

// the hit of a pair without cells, or whose best is 0: nothing aligned
nw_local_hit empty_hit(int32_t begin) {
    nw_local_hit h;
    std::memset(&h, 0, sizeof h);
    h.begin_i = h.begin_j = begin;
    return h;
}

// The semi-global hit of a pair with an empty side, from the definition: the table is one
// boundary of n + 1 cells, B(0) = 0 and B(k) = 0 (its begin is free) or go + k * gap.  The
// end is cell n, or with that boundary's end free the first maximum; the walk stops there
// if the begin is free, else it runs to (0, 0).  walked: the align entry (begin cell and
// *n_ops); the score entries write -1.
nw_local_hit semi_empty_hit(const Cost &cost, const nw_params *p, int64_t n1, int64_t n2, bool walked,
                            int64_t *n_ops) {
    const bool rows = n1 == 0;  // the cells are (k, 0); else (0, k)
    const int64_t n = std::max(n1, n2);
    const bool begin_free = (cost.ends & (rows ? NW_ENDS_S2_BEGIN : NW_ENDS_S1_BEGIN)) != 0;
    const bool end_free = (cost.ends & (rows ? NW_ENDS_S2_END : NW_ENDS_S1_END)) != 0;
    auto B = [&](int64_t k) { return (k == 0 || begin_free) ? (int64_t)0 : (int64_t)cost.open + (int64_t)p->gap * k; };
    int64_t k = n;
    if (end_free) {  // (B is linear from 1 to n: the first maximum is at 0, 1 or n)
        k = 0;
        if (n >= 1 && B(1) > B(k)) k = 1;
        if (B(n) > B(k)) k = n;
    }
    nw_local_hit h;
    std::memset(&h, 0, sizeof h);
    h.score = (int32_t)B(k);
    (rows ? h.end_i : h.end_j) = (int32_t)k;
    h.begin_i = h.begin_j = -1;
    if (walked) {
        h.begin_i = h.begin_j = 0;
        if (begin_free) (rows ? h.begin_i : h.begin_j) = (int32_t)k;
        *n_ops = begin_free ? 0 : k;
    }
    return h;
}

// The matrix into the launch's arguments.  The cells hold the w form, which adds s - 2
// gap per diagonal: those bytes when every one of them fits int8 (the kernel then adds
// nothing), else s itself and the kernel adds -2 gap per cell (wide).  Entries beyond n
// are 0 whatever the caller left there.
void submat_args(const nw_submat *m, int32_t gap, bool local, nw::BatchMatrixArgs *ma) {
    if (local) gap = 0;  // (the local cells are not in the w form: the bytes are s itself, and fit)
    bool fits = true;
    for (int x = 0; x < m->n && fits; ++x)
        for (int y = 0; y < m->n; ++y) {
            const int v = (int)m->score[x * NW_SUBMAT_MAX + y] - 2 * gap;
            if (v < -128 || v > 127) fits = false;
        }
    int8_t bytes[NW_SUBMAT_MAX * NW_SUBMAT_MAX];
    std::memset(bytes, 0, sizeof bytes);
    for (int x = 0; x < m->n; ++x)
        for (int y = 0; y < m->n; ++y)
            bytes[x * NW_SUBMAT_MAX + y] = (int8_t)(m->score[x * NW_SUBMAT_MAX + y] - (fits ? 2 * gap : 0));
    static_assert(sizeof bytes == sizeof ma->score && NW_SUBMAT_MAX == nw::kBatchMatrixLetters, "nw_submat layout");
    std::memcpy(ma->score, bytes, sizeof bytes);
    std::memcpy(ma->index, m->index, 256);
    ma->n = m->n;
    ma->wide = fits ? 0 : 1;
}

// what every batch entry refuses in its parameters, judged without a device
// (NW_KERNEL_PANELS, which is NW_ERR_UNSUPPORTED, comes after every NW_ERR_ARG)
int params_check(const nw_params *p, int64_t npairs, const Cost &cost) {
    if (!valid_params(p) || p->mode != (cost.local ? NW_MODE_SW : NW_MODE_NW)) return NW_ERR_ARG;
    if ((p->flags & ~NW_FLAG_NO_PROFILE) != 0) return NW_ERR_ARG;
    // with a positive gap_open the walk would open a new gap at every step, and the ops
    // would no longer determine the score
    if (cost.affine && cost.open > 0) return NW_ERR_ARG;
    if (npairs < 0 || npairs >= INT32_MAX) return NW_ERR_ARG;
    if (cost.matrix && !valid_submat(cost.mat)) return NW_ERR_ARG;
    if (cost.semi && (cost.ends < 0 || cost.ends > NW_ENDS_OVERLAP)) return NW_ERR_ARG;
    // piece 2 as piece 1: no positive opening, the extension within nw_params.gap's range
    if (cost.dual && (cost.open2 > 0 || !valid_gap(cost.gap2))) return NW_ERR_ARG;
    // (after the two-piece refusals; the banded entries have none of those)
    if (cost.banded && cost.band < 0) return NW_ERR_ARG;
    return NW_OK;
}

// a batch from host buffers: its sizes and the pairs that have cells, longest first
struct Batch {
    int64_t total1 = 0, total2 = 0, max_n2 = 0, cells = 0;
    std::vector<int32_t> order;
};

int batch_check(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2, int64_t npairs,
                const nw_params *p, const Cost &cost, const void *scores, Batch *b) {
    int st = params_check(p, npairs, cost);
    if (st != NW_OK) return st;
    if (npairs == 0) return NW_OK;
    if (!off1 || !off2 || !scores) return NW_ERR_ARG;
    if (off1[0] != 0 || off2[0] != 0) return NW_ERR_ARG;
    for (int64_t i = 0; i < npairs; ++i) {
        const int64_t n1 = off1[i + 1] - off1[i], n2 = off2[i + 1] - off2[i];
        if (n1 < 0 || n2 < 0 || n1 >= INT32_MAX || n2 >= INT32_MAX) return NW_ERR_ARG;
        if (!cost.range_ok(p, n1, n2)) return NW_ERR_ARG;
        b->max_n2 = std::max(b->max_n2, n2);
        b->cells += n1 * n2;
    }
    b->total1 = off1[npairs];
    b->total2 = off2[npairs];
    if ((b->total1 > 0 && !s1cat) || (b->total2 > 0 && !s2cat)) return NW_ERR_ARG;
    return NW_OK;
}

void batch_order(const int64_t *off1, const int64_t *off2, int64_t npairs, Batch *b) {
    for (int64_t i = 0; i < npairs; ++i)
        if (off1[i + 1] > off1[i] && off2[i + 1] > off2[i]) b->order.push_back((int32_t)i);
    auto cells = [&](int32_t i) { return (off1[i + 1] - off1[i]) * (off2[i + 1] - off2[i]); };
    std::stable_sort(b->order.begin(), b->order.end(), [&](int32_t x, int32_t y) { return cells(x) > cells(y); });
}

// the workers of a launch: nw_params.waves (0: kCkptWavesPerCU per CU) capped at `tickets`
int64_t workers(const nw_ctx *c, const nw_params *p, int64_t tickets) {
    const int64_t w = p->waves > 0 ? p->waves : (int64_t)c->cus * nw::kCkptWavesPerCU;
    return std::max<int64_t>(1, std::min<int64_t>(w, tickets));
}

// The context's workspace of a batch launch, the charmap over the concatenated s1 and
// the row characters of the concatenated s2 (three small launches per batch, whatever
// its number of pairs; with a matrix: one launch, the rows as letters, and the matrix
// into *ma); *ma gets everything but the tickets, the scores and the
// directions, *grid the workers.
int batch_prepare(nw_ctx *c, const int8_t *d_s1, const int64_t *d_off1, int64_t total1, const int8_t *d_s2,
                  const int64_t *d_off2, int64_t total2, int64_t max_n2, const nw_params *p, const Cost &cost,
                  int64_t tickets, void *stream, nw::BatchMatrixArgs *ma, int *grid) {
    int st;
    const int64_t waves = workers(c, p, tickets);
    const int64_t cstride = cost.col_words(max_n2);
    const int64_t rows_len = nw::kBatchRowPad + total2 + nw::kBatchRowTail;
    if ((st = grow((void **)&c->rowpack, &c->rowpack_cap, (size_t)rows_len)) != NW_OK) return st;
    if ((st = grow((void **)&c->scratch, &c->scratch_cap, (size_t)(waves * cstride) * 4)) != NW_OK) return st;
    const bool perm_ok = !cost.matrix && perm_allowed(p, 2 * p->gap);
    std::memset(ma, 0, sizeof *ma);
    nw::BatchAffineArgs *aa = &ma->a;
    if (cost.matrix) {
        // the matrix is the alphabet: no charmap pass, the rows become letters
        if (nw::launch_batch_matrix_rows((const uint8_t *)d_s2, total2, cost.mat->index, (uint8_t *)c->rowpack,
                                         stream) != hipSuccess)
            return NW_ERR_HIP;
        submat_args(cost.mat, p->gap, cost.local, ma);
    } else {
        if (nw::launch_charmap((const uint8_t *)d_s1, total1, c->meta, stream) != hipSuccess) return NW_ERR_HIP;
        if (nw::launch_batch_rows((const uint8_t *)d_s2, total2, perm_ok ? 1 : 0, c->meta, (uint8_t *)c->rowpack,
                                  stream) != hipSuccess)
            return NW_ERR_HIP;
    }
    aa->gap_open = cost.open;
    aa->eoff = nw::batch_col_words(max_n2);
    nw::BatchArgs *a = &aa->b;
    a->s1 = (const uint8_t *)d_s1;
    a->off1 = d_off1;
    a->rows = (const uint8_t *)c->rowpack;
    a->off2 = d_off2;
    a->max_n2 = (int32_t)max_n2;
    a->ticket = c->ctrl;  // word [0], zeroed by launch_ctrl_reset
    a->colscr = c->scratch;
    a->cstride = cstride;
    a->perm = perm_ok ? 1 : 0;
    a->charmap = c->meta;
    a->nprof = (const uint32_t *)(c->meta + 256);
    a->match = p->match;
    a->mismatch = p->mismatch;
    a->gap = p->gap;
    *grid = (int)waves;
    return NW_OK;
}

// one launch of the batch kernel over a->npairs tickets (local and semi: ma.a.b.scores
// holds the hits)
int batch_run(nw_ctx *c, const nw::BatchMatrixArgs &ma, const Cost &cost, bool dirs, int grid, void *stream) {
    if (nw::launch_ctrl_reset(c->ctrl, stream) != hipSuccess) return NW_ERR_HIP;
    const nw::BatchAffineArgs &aa = ma.a;
    const int g = std::min(grid, std::max(aa.b.npairs, 1));
    int e;
    if (cost.local) {
        nw::BatchLocalArgs la;
        la.m = ma;
        la.hits = ma.a.b.scores;
        la.m.a.b.scores = nullptr;
        e = nw::launch_batch_local(la, dirs, g, stream);
    } else if (cost.semi) {
        nw::BatchSemiArgs sa;
        sa.m = ma;
        sa.hits = ma.a.b.scores;
        sa.m.a.b.scores = nullptr;
        sa.ends = cost.ends;
        e = nw::launch_batch_semi(sa, dirs, g, stream);
    } else if (cost.banded && cost.dual) {
        nw::BatchDualBandedArgs ba;
        ba.d.m = ma;
        ba.d.gap_open2 = cost.open2;
        ba.d.gap2 = cost.gap2;
        ba.d.eoff2 = 2 * ma.a.eoff;
        ba.band = cost.band;
        e = nw::launch_batch_dual_banded(ba, dirs, g, stream);
    } else if (cost.banded) {
        nw::BatchBandedArgs ba;
        ba.m = ma;
        ba.band = cost.band;
        e = nw::launch_batch_banded(ba, dirs, g, stream);
    } else if (cost.dual) {
        nw::BatchDualArgs da;
        da.m = ma;
        da.gap_open2 = cost.open2;
        da.gap2 = cost.gap2;
        da.eoff2 = 2 * ma.a.eoff;
        e = nw::launch_batch_dual(da, dirs, g, stream);
    } else
        e = cost.matrix ? nw::launch_batch_matrix(ma, dirs, g, stream)
            : cost.affine ? nw::launch_batch_affine(aa, dirs, g, stream)
                          : nw::launch_batch(aa.b, dirs, g, stream);
    if (e != hipSuccess) return NW_ERR_HIP;
    c->last_waves = grid;
    c->last_kernel = NW_KERNEL_STRIPS;
    return NW_OK;
}

// sequences, offsets and the order of a batch on the device: one copy each
struct BatchDev {
    int8_t *s1 = nullptr, *s2 = nullptr;
    int64_t *off1 = nullptr, *off2 = nullptr;
    int32_t *order = nullptr, *scores = nullptr;
    int64_t bytes = 0;
    int upload(DevBufs &bufs, const int8_t *s1cat, const int64_t *h_off1, const int8_t *s2cat, const int64_t *h_off2,
               int64_t npairs, const Batch &b, const Cost &cost) {
        int st;
        const size_t ob = (size_t)(npairs + 1) * 8, cnt = b.order.size();
        if ((st = bufs.alloc((void **)&s1, (size_t)b.total1)) != NW_OK) return st;
        if ((st = bufs.alloc((void **)&s2, (size_t)b.total2)) != NW_OK) return st;
        if ((st = bufs.alloc((void **)&off1, ob)) != NW_OK) return st;
        if ((st = bufs.alloc((void **)&off2, ob)) != NW_OK) return st;
        if ((st = bufs.alloc((void **)&order, cnt * 4)) != NW_OK) return st;
        if ((st = bufs.alloc((void **)&scores, (size_t)npairs * cost.out_bytes())) != NW_OK) return st;
        if (b.total1 > 0) NW_HIP_TRY(hipMemcpy(s1, s1cat, (size_t)b.total1, hipMemcpyHostToDevice));
        if (b.total2 > 0) NW_HIP_TRY(hipMemcpy(s2, s2cat, (size_t)b.total2, hipMemcpyHostToDevice));
        NW_HIP_TRY(hipMemcpy(off1, h_off1, ob, hipMemcpyHostToDevice));
        NW_HIP_TRY(hipMemcpy(off2, h_off2, ob, hipMemcpyHostToDevice));
        NW_HIP_TRY(hipMemcpy(order, b.order.data(), cnt * 4, hipMemcpyHostToDevice));
        return NW_OK;
    }
    static int64_t need(int64_t npairs, const Batch &b, const Cost &cost) {
        return b.total1 + b.total2 + 2 * (npairs + 1) * 8 + (int64_t)b.order.size() * 4 +
               npairs * (int64_t)cost.out_bytes();
    }
};

// what batch_prepare makes the context hold
int64_t workspace_need(const Batch &b, int64_t waves, const Cost &cost) {
    return nw::kBatchRowPad + b.total2 + nw::kBatchRowTail + waves * cost.col_words(b.max_n2) * 4 +
           nw::kMetaBytes + nw::kCtrlWords * 4;
}

int score_batch_async(nw_ctx *c, const int8_t *d_s1cat, const int64_t *d_off1, const int8_t *d_s2cat,
                      const int64_t *d_off2, int64_t npairs, int64_t total1, int64_t total2, int64_t max_n2,
                      const nw_params *p, const Cost &cost, void *d_scores, void *stream) {
    int st = params_check(p, npairs, cost);
    if (st != NW_OK) return st;
    if (total1 < 0 || total2 < 0 || max_n2 < 0 || max_n2 >= INT32_MAX || max_n2 > total2) return NW_ERR_ARG;
    if (!cost.range_ok(p, 0, max_n2)) return NW_ERR_ARG;
    if (p->kernel == NW_KERNEL_PANELS) return NW_ERR_UNSUPPORTED;
    if (!c) return NW_ERR_ARG;
    if (npairs == 0) return NW_OK;
    if (!d_off1 || !d_off2 || !d_scores || (total1 > 0 && !d_s1cat) || (total2 > 0 && !d_s2cat)) return NW_ERR_ARG;
    NW_HIP_TRY(hipSetDevice(c->device));
    nw::BatchMatrixArgs ma;
    int grid = 0;
    if ((st = batch_prepare(c, d_s1cat, d_off1, total1, d_s2cat, d_off2, total2, max_n2, p, cost, npairs, stream, &ma,
                            &grid)) != NW_OK)
        return st;
    ma.a.b.npairs = (int32_t)npairs;  // (tickets in index order: the lengths are on the device)
    ma.a.b.scores = (int32_t *)d_scores;
    return batch_run(c, ma, cost, false, grid, stream);
}

int score_batch(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2, int64_t npairs,
                const nw_params *p, const Cost &cost, void *out, nw_batch_stats *stats) {
    int32_t *scores = (int32_t *)out;          // (global entries)
    nw_local_hit *hits = (nw_local_hit *)out;  // (local and semi-global entries)
    nw_params def;
    if (!p) {
        nw_params_default(&def);
        if (cost.local) def.mode = NW_MODE_SW;
        p = &def;
    }
    Batch b;
    int st = batch_check(s1cat, off1, s2cat, off2, npairs, p, cost, out, &b);
    if (st != NW_OK) return st;
    if (p->kernel == NW_KERNEL_PANELS) return NW_ERR_UNSUPPORTED;
    int dev;
    if ((st = have_device(p, &dev)) != NW_OK) return st;
    nw_batch_stats bs;
    std::memset(&bs, 0, sizeof bs);
    bs.pairs = npairs;
    bs.cells = b.cells;
    if (stats) *stats = bs;
    if (npairs == 0) return NW_OK;
    batch_order(off1, off2, npairs, &b);
    for (int64_t i = 0; i < npairs; ++i) {  // no cells: the corner of the boundary
        const int64_t n1 = off1[i + 1] - off1[i], n2 = off2[i + 1] - off2[i];
        if (n1 != 0 && n2 != 0) continue;
        if (cost.local)
            hits[i] = empty_hit(-1);
        else if (cost.semi)
            hits[i] = semi_empty_hit(cost, p, n1, n2, false, nullptr);
        else
            scores[i] = cost.empty_score(p, std::max(n1, n2));
    }
    const int64_t cnt = (int64_t)b.order.size();
    if (cnt == 0) return NW_OK;

    Lease L;
    if ((st = L.acquire(dev)) != NW_OK) return st;
    nw_ctx *c = L.c;
    NW_HIP_TRY(hipSetDevice(dev));
    DevBufs bufs;
    BatchDev d;
    if ((st = d.upload(bufs, s1cat, off1, s2cat, off2, npairs, b, cost)) != NW_OK) return st;
    nw::BatchMatrixArgs ma;
    int grid = 0;
    if ((st = batch_prepare(c, d.s1, d.off1, b.total1, d.s2, d.off2, b.total2, b.max_n2, p, cost, cnt, nullptr, &ma,
                            &grid)) != NW_OK)
        return st;
    ma.a.b.order = d.order;
    ma.a.b.npairs = (int32_t)cnt;
    ma.a.b.scores = d.scores;
    NW_HIP_TRY(hipEventRecord(c->ev0, nullptr));
    if ((st = batch_run(c, ma, cost, false, grid, nullptr)) != NW_OK) return st;
    NW_HIP_TRY(hipEventRecord(c->ev1, nullptr));
    const size_t ob = cost.out_bytes();
    std::vector<uint8_t> got((size_t)npairs * ob);
    NW_HIP_TRY(hipMemcpy(got.data(), d.scores, got.size(), hipMemcpyDeviceToHost));
    for (int32_t i : b.order) std::memcpy((uint8_t *)out + (size_t)i * ob, got.data() + (size_t)i * ob, ob);
    float ms = 0.f;
    NW_HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    bs.chunks = 1;
    bs.waves = grid;
    bs.fill_ms = ms;
    bs.peak_bytes = BatchDev::need(npairs, b, cost) + workspace_need(b, grid, cost);
    if (stats) *stats = bs;
    return NW_OK;
}

int align_batch(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2, int64_t npairs,
                const nw_params *p, const Cost &cost, const nw_batch_opts *o, void *out, uint8_t *ops,
                const int64_t *ops_off, int64_t *n_ops, nw_batch_stats *stats) {
    int32_t *scores = (int32_t *)out;          // (global entries)
    nw_local_hit *hits = (nw_local_hit *)out;  // (local and semi-global entries)
    nw_params def;
    if (!p) {
        nw_params_default(&def);
        if (cost.local) def.mode = NW_MODE_SW;
        p = &def;
    }
    Batch b;
    int st = batch_check(s1cat, off1, s2cat, off2, npairs, p, cost, out, &b);
    if (st != NW_OK) return st;
    int64_t mem = 0;
    if (o) {
        if (o->mem_bytes < 0) return NW_ERR_ARG;
        for (int k = 0; k < 6; ++k)
            if (o->reserved[k] != 0) return NW_ERR_ARG;
        mem = o->mem_bytes;
    }
    if (npairs > 0) {
        if (!ops_off || !n_ops) return NW_ERR_ARG;
        for (int64_t i = 0; i < npairs; ++i) {
            const int64_t need = (off1[i + 1] - off1[i]) + (off2[i + 1] - off2[i]);
            if (ops_off[i] < 0 || ops_off[i + 1] - ops_off[i] < need) return NW_ERR_ARG;
        }
        if (ops_off[npairs] > 0 && !ops) return NW_ERR_ARG;
    }
    if (p->kernel == NW_KERNEL_PANELS) return NW_ERR_UNSUPPORTED;
    int dev;
    if ((st = have_device(p, &dev)) != NW_OK) return st;
    nw_batch_stats bs;
    std::memset(&bs, 0, sizeof bs);
    bs.pairs = npairs;
    bs.cells = b.cells;
    if (stats) *stats = bs;
    if (npairs == 0) return NW_OK;
    batch_order(off1, off2, npairs, &b);
    for (int64_t i = 0; i < npairs; ++i) {  // no cells: all ups or all lefts
        const int64_t n1 = off1[i + 1] - off1[i], n2 = off2[i + 1] - off2[i];
        if (n1 != 0 && n2 != 0) continue;
        if (cost.local) {  // nothing aligned
            hits[i] = empty_hit(0);
            n_ops[i] = 0;
            continue;
        }
        if (cost.semi) {  // the part of the boundary between the begin and the end cell
            hits[i] = semi_empty_hit(cost, p, n1, n2, true, &n_ops[i]);
            if (n_ops[i] > 0) std::memset(ops + ops_off[i], n2 > 0 ? 1 : 2, (size_t)n_ops[i]);
            continue;
        }
        const int64_t n = std::max(n1, n2);
        scores[i] = cost.empty_score(p, n);
        n_ops[i] = n;
        if (n > 0) std::memset(ops + ops_off[i], n2 > 0 ? 1 : 2, (size_t)n);
    }
    const int64_t cnt = (int64_t)b.order.size();
    if (cnt == 0) return NW_OK;

    Lease L;
    if ((st = L.acquire(dev)) != NW_OK) return st;
    nw_ctx *c = L.c;
    NW_HIP_TRY(hipSetDevice(dev));
    if (mem == 0) {
        size_t free_b = 0, total_b = 0;
        NW_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        mem = (int64_t)((double)free_b * 0.8);
    }
    // The chunks: consecutive runs of the longest-first order whose direction blocks
    // and ops slots fit what the budget leaves after everything else the call holds.
    const int64_t waves = workers(c, p, cnt);
    const int64_t fixed = BatchDev::need(npairs, b, cost) + workspace_need(b, waves, cost) + cnt * 3 * 8;
    std::vector<int64_t> dir_off((size_t)cnt), loc_off((size_t)cnt);
    std::vector<int64_t> chunk_first;  // ticket where each chunk starts (+ the end)
    int64_t cur_dir = 0, cur_ops = 0, max_dir = 0, max_ops = 0;
    for (int64_t t = 0; t < cnt; ++t) {
        const int32_t i = b.order[(size_t)t];
        const int64_t n1 = off1[i + 1] - off1[i], n2 = off2[i + 1] - off2[i];
        const int64_t db = cost.dir_bytes(n1, n2), ob = n1 + n2;
        bs.dir_bytes += db;
        if (fixed + db + ob > mem) return NW_ERR_OOM;  // (this pair alone: nw_align_ckpt's case)
        if (t == 0 || fixed + cur_dir + cur_ops + db + ob > mem) {
            chunk_first.push_back(t);
            cur_dir = cur_ops = 0;
        }
        dir_off[(size_t)t] = cur_dir;
        loc_off[(size_t)t] = cur_ops;
        cur_dir += db;
        cur_ops += ob;
        max_dir = std::max(max_dir, cur_dir);
        max_ops = std::max(max_ops, cur_ops);
        bs.peak_bytes = std::max(bs.peak_bytes, fixed + cur_dir + cur_ops);
    }
    chunk_first.push_back(cnt);
    bs.chunks = (int64_t)chunk_first.size() - 1;
    bs.waves = (int32_t)waves;

    DevBufs bufs;
    BatchDev d;
    Events ef, ew;
    if ((st = d.upload(bufs, s1cat, off1, s2cat, off2, npairs, b, cost)) != NW_OK) return st;
    uint8_t *d_dirs = nullptr, *d_ops = nullptr;
    int64_t *d_dir_off = nullptr, *d_loc_off = nullptr, *d_nops = nullptr;
    if ((st = bufs.alloc((void **)&d_dirs, (size_t)max_dir)) != NW_OK) return st;
    if ((st = bufs.alloc((void **)&d_ops, (size_t)max_ops)) != NW_OK) return st;
    if ((st = bufs.alloc((void **)&d_dir_off, (size_t)cnt * 8)) != NW_OK) return st;
    if ((st = bufs.alloc((void **)&d_loc_off, (size_t)cnt * 8)) != NW_OK) return st;
    if ((st = bufs.alloc((void **)&d_nops, (size_t)cnt * 8)) != NW_OK) return st;
    NW_HIP_TRY(hipMemcpy(d_dir_off, dir_off.data(), (size_t)cnt * 8, hipMemcpyHostToDevice));
    NW_HIP_TRY(hipMemcpy(d_loc_off, loc_off.data(), (size_t)cnt * 8, hipMemcpyHostToDevice));
    NW_HIP_TRY(hipEventCreate(&ef.a));
    NW_HIP_TRY(hipEventCreate(&ef.b));
    NW_HIP_TRY(hipEventCreate(&ew.b));
    nw::BatchMatrixArgs ma;
    nw::BatchArgs &a = ma.a.b;
    int grid = 0;
    if ((st = batch_prepare(c, d.s1, d.off1, b.total1, d.s2, d.off2, b.total2, b.max_n2, p, cost, cnt, nullptr, &ma,
                            &grid)) != NW_OK)
        return st;
    a.scores = d.scores;
    a.dirs = d_dirs;
    std::vector<uint8_t> stage((size_t)max_ops);
    for (size_t k = 0; k + 1 < chunk_first.size(); ++k) {
        const int64_t t0 = chunk_first[k], nt = chunk_first[k + 1] - t0;
        a.order = d.order + t0;
        a.dir_off = d_dir_off + t0;
        a.npairs = (int32_t)nt;
        nw::BatchWalkArgs w;
        w.off1 = d.off1;
        w.off2 = d.off2;
        w.order = a.order;
        w.npairs = a.npairs;
        w.dirs = d_dirs;
        w.dir_off = a.dir_off;
        w.ops = d_ops;
        w.ops_off = d_loc_off + t0;
        w.n_ops = d_nops + t0;
        NW_HIP_TRY(hipEventRecord(ef.a, nullptr));
        if ((st = batch_run(c, ma, cost, true, grid, nullptr)) != NW_OK) return st;
        NW_HIP_TRY(hipEventRecord(ef.b, nullptr));
        int e;
        if (cost.local) {  // the walk reads its start from the hit on the device and adds the begin cell
            nw::BatchLocalWalkArgs lw;
            lw.w = w;
            lw.hits = d.scores;
            e = nw::launch_batch_local_walk(lw, nullptr);
        } else if (cost.semi) {  // the same, stopping on a free boundary
            nw::BatchSemiWalkArgs sw;
            sw.w = w;
            sw.hits = d.scores;
            sw.ends = cost.ends;
            e = nw::launch_batch_semi_walk(sw, nullptr);
        } else if (cost.banded && cost.dual) {  // five states over the strips' ranges
            nw::BatchDualBandedWalkArgs bw;
            bw.w = w;
            bw.band = cost.band;
            e = nw::launch_batch_dual_banded_walk(bw, nullptr);
        } else if (cost.banded) {  // the affine walk over the strips' ranges
            nw::BatchBandedWalkArgs bw;
            bw.w = w;
            bw.band = cost.band;
            e = nw::launch_batch_banded_walk(bw, nullptr);
        } else if (cost.dual)  // five states over a byte per cell
            e = nw::launch_batch_dual_walk(w, nullptr);
        else
            e = cost.affine ? nw::launch_batch_affine_walk(w, nullptr) : nw::launch_batch_walk(w, nullptr);
        if (e != hipSuccess) return NW_ERR_HIP;
        NW_HIP_TRY(hipEventRecord(ew.b, nullptr));
        // the chunk's ops: one copy (which also orders the next chunk's launches after
        // this chunk's walk), then each pair's slot into the caller's
        const int32_t last = b.order[(size_t)(t0 + nt - 1)];
        const int64_t chunk_ops =
            loc_off[(size_t)(t0 + nt - 1)] + (off1[last + 1] - off1[last]) + (off2[last + 1] - off2[last]);
        NW_HIP_TRY(hipMemcpy(stage.data(), d_ops, (size_t)chunk_ops, hipMemcpyDeviceToHost));
        for (int64_t t = t0; t < t0 + nt; ++t) {
            const int32_t i = b.order[(size_t)t];
            const int64_t len = (off1[i + 1] - off1[i]) + (off2[i + 1] - off2[i]);
            std::memcpy(ops + ops_off[i], stage.data() + loc_off[(size_t)t], (size_t)len);
        }
        float ms = 0.f;
        NW_HIP_TRY(hipEventElapsedTime(&ms, ef.a, ef.b));
        bs.fill_ms += ms;
        NW_HIP_TRY(hipEventElapsedTime(&ms, ef.b, ew.b));
        bs.walk_ms += ms;
    }
    const size_t ob = cost.out_bytes();
    std::vector<uint8_t> got((size_t)npairs * ob);
    std::vector<int64_t> gotn((size_t)cnt);
    NW_HIP_TRY(hipMemcpy(got.data(), d.scores, got.size(), hipMemcpyDeviceToHost));
    NW_HIP_TRY(hipMemcpy(gotn.data(), d_nops, (size_t)cnt * 8, hipMemcpyDeviceToHost));
    for (int64_t t = 0; t < cnt; ++t) {
        const int32_t i = b.order[(size_t)t];
        std::memcpy((uint8_t *)out + (size_t)i * ob, got.data() + (size_t)i * ob, ob);
        n_ops[i] = gotn[(size_t)t];
    }
    if (stats) *stats = bs;
    return NW_OK;
}

}  // namespace

extern "C" {

int64_t nw_batch_dir_bytes(int64_t n1, int64_t n2) {
    if (n1 < 0 || n2 < 0) return -1;
    if (n1 == 0 || n2 == 0) return 0;
    return nw::batch_strips(n1) * nw::batch_iters(n2) * nw::kBatchDirIter;
}

int64_t nw_batch_affine_dir_bytes(int64_t n1, int64_t n2) {
    const int64_t b = nw_batch_dir_bytes(n1, n2);
    return b < 0 ? b : 2 * b;
}

int64_t nw_batch_banded_dir_bytes(int64_t n1, int64_t n2, int32_t band) {
    if (n1 < 0 || n2 < 0 || band < 0) return -1;
    if (n1 == 0 || n2 == 0) return 0;
    return nw::batch_strips(n1) * nw::batch_banded_slots(n1, n2, band) * 2 * nw::kBatchDirIter;
}

int64_t nw_batch_dual_dir_bytes(int64_t n1, int64_t n2) {
    const int64_t b = nw_batch_affine_dir_bytes(n1, n2);
    return b < 0 ? b : 2 * b;
}

int64_t nw_batch_dual_banded_dir_bytes(int64_t n1, int64_t n2, int32_t band) {
    const int64_t b = nw_batch_banded_dir_bytes(n1, n2, band);
    return b < 0 ? b : 2 * b;
}

int nw_score_batch_async(nw_ctx *c, const int8_t *d_s1cat, const int64_t *d_off1, const int8_t *d_s2cat,
                         const int64_t *d_off2, int64_t npairs, int64_t total1, int64_t total2, int64_t max_n2,
                         const nw_params *p, int32_t *d_scores, void *stream) {
    return score_batch_async(c, d_s1cat, d_off1, d_s2cat, d_off2, npairs, total1, total2, max_n2, p, Cost{}, d_scores,
                             stream);
}

int nw_score_batch(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                   int64_t npairs, const nw_params *p, int32_t *scores, nw_batch_stats *stats) {
    return score_batch(s1cat, off1, s2cat, off2, npairs, p, Cost{}, scores, stats);
}

int nw_align_batch(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                   int64_t npairs, const nw_params *p, const nw_batch_opts *o, int32_t *scores, uint8_t *ops,
                   const int64_t *ops_off, int64_t *n_ops, nw_batch_stats *stats) {
    return align_batch(s1cat, off1, s2cat, off2, npairs, p, Cost{}, o, scores, ops, ops_off, n_ops, stats);
}

int nw_score_batch_affine_async(nw_ctx *c, const int8_t *d_s1cat, const int64_t *d_off1, const int8_t *d_s2cat,
                                const int64_t *d_off2, int64_t npairs, int64_t total1, int64_t total2,
                                int64_t max_n2, const nw_params *p, int32_t gap_open, int32_t *d_scores,
                                void *stream) {
    return score_batch_async(c, d_s1cat, d_off1, d_s2cat, d_off2, npairs, total1, total2, max_n2, p,
                             Cost{true, gap_open}, d_scores, stream);
}

int nw_score_batch_affine(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                          int64_t npairs, const nw_params *p, int32_t gap_open, int32_t *scores,
                          nw_batch_stats *stats) {
    return score_batch(s1cat, off1, s2cat, off2, npairs, p, Cost{true, gap_open}, scores, stats);
}

int nw_align_batch_affine(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                          int64_t npairs, const nw_params *p, int32_t gap_open, const nw_batch_opts *o,
                          int32_t *scores, uint8_t *ops, const int64_t *ops_off, int64_t *n_ops,
                          nw_batch_stats *stats) {
    return align_batch(s1cat, off1, s2cat, off2, npairs, p, Cost{true, gap_open}, o, scores, ops, ops_off, n_ops,
                       stats);
}

int nw_score_batch_matrix_async(nw_ctx *c, const int8_t *d_s1cat, const int64_t *d_off1, const int8_t *d_s2cat,
                                const int64_t *d_off2, int64_t npairs, int64_t total1, int64_t total2,
                                int64_t max_n2, const nw_params *p, const nw_submat *m, int32_t gap_open,
                                int32_t *d_scores, void *stream) {
    return score_batch_async(c, d_s1cat, d_off1, d_s2cat, d_off2, npairs, total1, total2, max_n2, p,
                             matrix_cost(m, gap_open), d_scores, stream);
}

int nw_score_batch_matrix(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                          int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open, int32_t *scores,
                          nw_batch_stats *stats) {
    return score_batch(s1cat, off1, s2cat, off2, npairs, p, matrix_cost(m, gap_open), scores, stats);
}

int nw_align_batch_matrix(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                          int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open,
                          const nw_batch_opts *o, int32_t *scores, uint8_t *ops, const int64_t *ops_off,
                          int64_t *n_ops, nw_batch_stats *stats) {
    return align_batch(s1cat, off1, s2cat, off2, npairs, p, matrix_cost(m, gap_open), o, scores, ops, ops_off,
                       n_ops, stats);
}

int nw_score_batch_local_async(nw_ctx *c, const int8_t *d_s1cat, const int64_t *d_off1, const int8_t *d_s2cat,
                               const int64_t *d_off2, int64_t npairs, int64_t total1, int64_t total2,
                               int64_t max_n2, const nw_params *p, const nw_submat *m, int32_t gap_open,
                               nw_local_hit *d_hits, void *stream) {
    return score_batch_async(c, d_s1cat, d_off1, d_s2cat, d_off2, npairs, total1, total2, max_n2, p,
                             local_cost(m, gap_open), d_hits, stream);
}

int nw_score_batch_local(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                         int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open,
                         nw_local_hit *hits, nw_batch_stats *stats) {
    return score_batch(s1cat, off1, s2cat, off2, npairs, p, local_cost(m, gap_open), hits, stats);
}

int nw_align_batch_local(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                         int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open,
                         const nw_batch_opts *o, nw_local_hit *hits, uint8_t *ops, const int64_t *ops_off,
                         int64_t *n_ops, nw_batch_stats *stats) {
    return align_batch(s1cat, off1, s2cat, off2, npairs, p, local_cost(m, gap_open), o, hits, ops, ops_off, n_ops,
                       stats);
}

int nw_score_batch_semi_async(nw_ctx *c, const int8_t *d_s1cat, const int64_t *d_off1, const int8_t *d_s2cat,
                              const int64_t *d_off2, int64_t npairs, int64_t total1, int64_t total2, int64_t max_n2,
                              const nw_params *p, const nw_submat *m, int32_t gap_open, int32_t ends,
                              nw_local_hit *d_hits, void *stream) {
    return score_batch_async(c, d_s1cat, d_off1, d_s2cat, d_off2, npairs, total1, total2, max_n2, p,
                             semi_cost(m, gap_open, ends), d_hits, stream);
}

int nw_score_batch_semi(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                        int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open, int32_t ends,
                        nw_local_hit *hits, nw_batch_stats *stats) {
    return score_batch(s1cat, off1, s2cat, off2, npairs, p, semi_cost(m, gap_open, ends), hits, stats);
}

int nw_align_batch_semi(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                        int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open, int32_t ends,
                        const nw_batch_opts *o, nw_local_hit *hits, uint8_t *ops, const int64_t *ops_off,
                        int64_t *n_ops, nw_batch_stats *stats) {
    return align_batch(s1cat, off1, s2cat, off2, npairs, p, semi_cost(m, gap_open, ends), o, hits, ops, ops_off,
                       n_ops, stats);
}

int nw_score_batch_banded_async(nw_ctx *c, const int8_t *d_s1cat, const int64_t *d_off1, const int8_t *d_s2cat,
                                const int64_t *d_off2, int64_t npairs, int64_t total1, int64_t total2,
                                int64_t max_n2, const nw_params *p, const nw_submat *m, int32_t gap_open,
                                int32_t band, int32_t *d_scores, void *stream) {
    return score_batch_async(c, d_s1cat, d_off1, d_s2cat, d_off2, npairs, total1, total2, max_n2, p,
                             banded_cost(m, gap_open, band), d_scores, stream);
}

int nw_score_batch_banded(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                          int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open, int32_t band,
                          int32_t *scores, nw_batch_stats *stats) {
    return score_batch(s1cat, off1, s2cat, off2, npairs, p, banded_cost(m, gap_open, band), scores, stats);
}

int nw_align_batch_banded(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                          int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open, int32_t band,
                          const nw_batch_opts *o, int32_t *scores, uint8_t *ops, const int64_t *ops_off,
                          int64_t *n_ops, nw_batch_stats *stats) {
    return align_batch(s1cat, off1, s2cat, off2, npairs, p, banded_cost(m, gap_open, band), o, scores, ops, ops_off,
                       n_ops, stats);
}

int nw_score_batch_dual_async(nw_ctx *c, const int8_t *d_s1cat, const int64_t *d_off1, const int8_t *d_s2cat,
                              const int64_t *d_off2, int64_t npairs, int64_t total1, int64_t total2, int64_t max_n2,
                              const nw_params *p, const nw_submat *m, int32_t gap_open, int32_t gap_open2,
                              int32_t gap2, int32_t *d_scores, void *stream) {
    return score_batch_async(c, d_s1cat, d_off1, d_s2cat, d_off2, npairs, total1, total2, max_n2, p,
                             dual_cost(m, gap_open, gap_open2, gap2), d_scores, stream);
}

int nw_score_batch_dual(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                        int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open, int32_t gap_open2,
                        int32_t gap2, int32_t *scores, nw_batch_stats *stats) {
    return score_batch(s1cat, off1, s2cat, off2, npairs, p, dual_cost(m, gap_open, gap_open2, gap2), scores, stats);
}

int nw_align_batch_dual(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                        int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open, int32_t gap_open2,
                        int32_t gap2, const nw_batch_opts *o, int32_t *scores, uint8_t *ops, const int64_t *ops_off,
                        int64_t *n_ops, nw_batch_stats *stats) {
    return align_batch(s1cat, off1, s2cat, off2, npairs, p, dual_cost(m, gap_open, gap_open2, gap2), o, scores, ops,
                       ops_off, n_ops, stats);
}

int nw_score_batch_dual_banded_async(nw_ctx *c, const int8_t *d_s1cat, const int64_t *d_off1, const int8_t *d_s2cat,
                                     const int64_t *d_off2, int64_t npairs, int64_t total1, int64_t total2,
                                     int64_t max_n2, const nw_params *p, const nw_submat *m, int32_t gap_open,
                                     int32_t gap_open2, int32_t gap2, int32_t band, int32_t *d_scores, void *stream) {
    return score_batch_async(c, d_s1cat, d_off1, d_s2cat, d_off2, npairs, total1, total2, max_n2, p,
                             dual_banded_cost(m, gap_open, gap_open2, gap2, band), d_scores, stream);
}

int nw_score_batch_dual_banded(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                               int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open,
                               int32_t gap_open2, int32_t gap2, int32_t band, int32_t *scores, nw_batch_stats *stats) {
    return score_batch(s1cat, off1, s2cat, off2, npairs, p, dual_banded_cost(m, gap_open, gap_open2, gap2, band),
                       scores, stats);
}

int nw_align_batch_dual_banded(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                               int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open,
                               int32_t gap_open2, int32_t gap2, int32_t band, const nw_batch_opts *o, int32_t *scores,
                               uint8_t *ops, const int64_t *ops_off, int64_t *n_ops, nw_batch_stats *stats) {
    return align_batch(s1cat, off1, s2cat, off2, npairs, p, dual_banded_cost(m, gap_open, gap_open2, gap2, band), o,
                       scores, ops, ops_off, n_ops, stats);
}

}  // extern "C"
