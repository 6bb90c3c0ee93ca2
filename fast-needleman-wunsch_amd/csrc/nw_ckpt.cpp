// nw_ckpt.cpp -- checkpointed (linear-memory) global alignment: the planner, the
// launch of the checkpoint sweep (kernel: nw_ckpt.hip), nw_score and nw_align_ckpt
// (sweep once, then re-fill and walk one K-row block at a time, last to first).
#include <algorithm>
#include <cstring>
#include <vector>

#include "nw_ckpt.h"
#include "nw_host_int.h"

using namespace nwh;

namespace {

constexpr int kPlanCus = 256;  // the planner makes no HIP call: MI355X's CU count

// what nwh::grow allocates for `need` bytes
int64_t grown(int64_t need) { return need <= 0 ? 0 : round_up(need, 1 << 21); }

// The sweep's chain: strips of kCkptCols columns from column 1, one-wave workers.
Shape sweep_shape(int64_t n1, int64_t n2, int32_t waves_req, int cus) {
    Shape s;
    std::memset(&s, 0, sizeof s);
    s.kernel = NW_KERNEL_STRIPS;
    s.K = nw::kCkptC;
    s.NC = 1;
    s.nRows = n2 + 1;
    s.nCols = n1 + 1;
    s.nstrips = std::max<int64_t>(1, (n1 + nw::kCkptCols - 1) / nw::kCkptCols);
    s.nblocks = (s.nRows + nw::kWave - 1) / nw::kWave;
    const int64_t w = waves_req > 0 ? waves_req : (int64_t)cus * nw::kCkptWavesPerCU;
    s.waves_max = std::max<int64_t>(1, w);
    s.waves = std::max<int64_t>(1, std::min<int64_t>(w, s.nstrips));
    // strip p publishes into slot p % M; when it is claimed every strip <= p - waves
    // has finished (nw_shape.cpp make_shape)
    s.M = std::min<int64_t>(s.nstrips, s.waves + 1);
    s.gstride = s.nblocks * nw::kWave;
    return s;
}

// launch_workspace's three buffers for a shape, as grow rounds them
void workspace_bytes(const Shape &s, int64_t *gran, int64_t *rowpack, int64_t *scratch) {
    *gran = std::max(*gran, grown(s.M * s.gstride * 8));
    *rowpack = std::max(*rowpack, grown(nw::rowpack_len((int32_t)s.nblocks) * 16));
    *scratch = std::max(*scratch, grown(s.waves * nw::kScratchWords * 4));
}

// Device memory of an alignment with block height K (default nw_params, `cus`
// CUs): the block table, the checkpoints, and what the context grows to over the
// sweep, the re-fills and the block tracebacks.
void ckpt_need(int64_t n1, int64_t n2, int64_t K, int cus, nw_ckpt_stats *st) {
    const int64_t rows = std::min(K, n2);
    const int64_t blocks = std::max<int64_t>(1, (n2 + K - 1) / K);
    st->block_rows = K;
    st->blocks = blocks;
    st->block_bytes = nw_table_bytes(n1, rows) + 256;
    st->ckpt_bytes = nw_ckpt_bytes(n1, n2, K);
    int64_t gran = 0, rowpack = 0, scratch = 0;
    if (n1 > 0 && n2 > 0) {
        if (blocks > 1) workspace_bytes(sweep_shape(n1, n2, 0, cus), &gran, &rowpack, &scratch);
        workspace_bytes(make_shape(n1, rows, 0, 0, 0, cus, 1, false, blocks > 1 ? NW_KERNEL_STRIPS : NW_KERNEL_AUTO),
                        &gran, &rowpack, &scratch);
    }
    const int64_t seqs = std::max<int64_t>(n1, 1) + std::max<int64_t>(n2, 1);
    const int64_t ops = grown(std::max<int64_t>(n1 + rows, 1));
    const int32_t maxwin = (int32_t)std::min<int64_t>(nw::kTbMaxWinDefault, rows / 64 + 1);
    const int64_t tb = grown((int64_t)nw::sw_tb_scratch_bytes(maxwin, nw::kTbBandDefault));
    const int64_t misc = 4096;  // control words, charmap, the score word
    st->peak_bytes = st->block_bytes + st->ckpt_bytes + gran + rowpack + scratch + seqs + ops + tb + misc;
}

// what the sweep refuses, judged without a device
int sweep_check(int64_t n1, int64_t n2, const nw_params *p, int64_t K) {
    if (n1 < 0 || n2 < 0 || n1 >= INT32_MAX || n2 >= INT32_MAX) return NW_ERR_ARG;
    if (!valid_params(p) || p->mode != NW_MODE_NW) return NW_ERR_ARG;
    if ((p->flags & ~NW_FLAG_NO_PROFILE) != 0) return NW_ERR_ARG;
    if (K <= 0 || K % nw::kWave != 0) return NW_ERR_ARG;
    if (!w_range_ok(p, n1, n2)) return NW_ERR_ARG;
    if (p->kernel == NW_KERNEL_PANELS) return NW_ERR_UNSUPPORTED;
    return NW_OK;
}

int align_blocks(int dev, const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, const nw_params *p,
                 const nw_tb_opts *o, int64_t K, uint8_t *host_ops, int64_t ops_cap, nw_alignment *out,
                 nw_ckpt_stats *cs);

}  // namespace

extern "C" {

int64_t nw_ckpt_bytes(int64_t n1, int64_t n2, int64_t K) {
    if (n1 < 0 || n2 < 0 || K <= 0) return 0;
    return nw::ckpt_rows(n2, K) * (n1 + 1) * (int64_t)sizeof(uint64_t);
}

int64_t nw_ckpt_peak_bytes(int64_t n1, int64_t n2, int64_t K) {
    if (n1 < 0 || n2 < 0 || n1 >= INT32_MAX || n2 >= INT32_MAX || K <= 0 || K % 64 != 0) return -1;
    nw_ckpt_stats st;
    std::memset(&st, 0, sizeof st);
    ckpt_need(n1, n2, K, kPlanCus, &st);
    return st.peak_bytes;
}

int nw_ckpt_plan(int64_t n1, int64_t n2, int64_t mem_bytes, nw_ckpt_stats *plan) {
    if (!plan || n1 < 0 || n2 < 0 || mem_bytes < 0 || n1 >= INT32_MAX || n2 >= INT32_MAX) return NW_ERR_ARG;
    std::memset(plan, 0, sizeof *plan);
    // the largest K that fits: the block table grows with K while the checkpoints
    // shrink, so the need is not monotonic -- scan down from the whole table
    for (int64_t K = std::max<int64_t>(64, round_up(n2, 64)); K >= 64; K -= 64) {
        nw_ckpt_stats st;
        std::memset(&st, 0, sizeof st);
        ckpt_need(n1, n2, K, kPlanCus, &st);
        if (st.peak_bytes <= mem_bytes) {
            *plan = st;
            return NW_OK;
        }
    }
    return NW_ERR_OOM;
}

int nw_ckpt_sweep_async(nw_ctx *c, const int8_t *d_s1, int64_t n1, const int8_t *d_s2, int64_t n2,
                        const nw_params *p, int64_t K, void *d_ckpt, int32_t *d_score, void *stream) {
    int st = sweep_check(n1, n2, p, K);
    if (st != NW_OK) return st;
    if (!c || n1 < 1 || n2 < 1 || !d_s1 || !d_s2 || !d_score) return NW_ERR_ARG;
    const int64_t nck = nw::ckpt_rows(n2, K);
    if ((nck > 0 && !d_ckpt) || ((uintptr_t)d_ckpt & 7u) != 0) return NW_ERR_ARG;
    NW_HIP_TRY(hipSetDevice(c->device));
    const Shape s = sweep_shape(n1, n2, p->waves, c->cus);
    int64_t qlen = 0;
    if ((st = launch_workspace(c, s, (uint64_t)s.nstrips, 1, stream, &qlen)) != NW_OK) return st;
    const bool perm_ok = perm_allowed(p, 2 * p->gap);
    if (nw::launch_rowpack((const uint8_t *)d_s1, n1, (const uint8_t *)d_s2, n2, 0, perm_ok ? 1 : 0, c->meta,
                           c->rowpack, qlen, stream) != hipSuccess)
        return NW_ERR_HIP;
    nw::CkptArgs a;
    std::memset(&a, 0, sizeof a);
    a.rowpack = c->rowpack;
    a.s1 = (const uint8_t *)d_s1;
    a.n1 = n1;
    a.n2 = n2;
    a.nstrips = (int32_t)s.nstrips;
    a.nblocks = (int32_t)s.nblocks;
    a.gran = c->gran;
    a.gstride = s.gstride;
    a.M = (int32_t)s.M;
    a.tagbase = c->tagbase;
    a.ctrl = c->ctrl;
    a.perm = perm_ok ? 1 : 0;
    a.charmap = c->meta;
    a.nprof = (const uint32_t *)(c->meta + 256);
    a.match = p->match;
    a.mismatch = p->mismatch;
    a.gap = p->gap;
    a.timeout_ticks = timeout_ticks(p->timeout_ms);
    a.K = K;
    a.nck = (int32_t)nck;
    a.ckpt = (uint64_t *)d_ckpt;
    a.score = d_score;
    if (nw::launch_ckpt_sweep(a, (int)s.waves, stream) != hipSuccess) return NW_ERR_HIP;
    c->tagbase += (uint32_t)s.nstrips + 1u;
    c->last_waves = (int)s.waves;
    c->last_strips = (int)s.nstrips;
    c->last_sub = s.K;
    c->last_nc = s.NC;
    c->last_col0 = 1;
    c->last_kernel = NW_KERNEL_STRIPS;
    return NW_OK;
}

int nw_score(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, const nw_params *p, nw_result *out) {
    nw_params def;
    if (!p) {
        nw_params_default(&def);
        p = &def;
    }
    if (!out || (n1 > 0 && !s1) || (n2 > 0 && !s2)) return NW_ERR_ARG;
    int st = sweep_check(n1, n2, p, 64);
    if (st != NW_OK) return st;
    int dev;
    if ((st = have_device(p, &dev)) != NW_OK) return st;
    std::memset(out, 0, sizeof *out);
    out->end_i = n2;
    out->end_j = n1;
    out->kernel = NW_KERNEL_STRIPS;
    if (n1 == 0 || n2 == 0) {  // no cells: the corner of the boundary
        out->score = (int32_t)(p->gap * std::max(n1, n2));
        return NW_OK;
    }
    Lease L;
    if ((st = L.acquire(dev)) != NW_OK) return st;
    nw_ctx *c = L.c;
    NW_HIP_TRY(hipSetDevice(dev));
    DevBufs bufs;
    int8_t *d_s1 = nullptr, *d_s2 = nullptr;
    int32_t *d_score = nullptr;
    if ((st = bufs.alloc((void **)&d_s1, (size_t)n1)) != NW_OK) return st;
    if ((st = bufs.alloc((void **)&d_s2, (size_t)n2)) != NW_OK) return st;
    if ((st = bufs.alloc((void **)&d_score, 4)) != NW_OK) return st;
    NW_HIP_TRY(hipMemcpy(d_s1, s1, (size_t)n1, hipMemcpyHostToDevice));
    NW_HIP_TRY(hipMemcpy(d_s2, s2, (size_t)n2, hipMemcpyHostToDevice));
    NW_HIP_TRY(hipEventRecord(c->ev0, nullptr));
    // K beyond n2: no checkpoint rows
    if ((st = nw_ckpt_sweep_async(c, d_s1, n1, d_s2, n2, p, round_up(n2, 64), nullptr, d_score, nullptr)) != NW_OK)
        return st;
    NW_HIP_TRY(hipEventRecord(c->ev1, nullptr));
    st = nw_ctx_status(c, nullptr);
    out->status = st;
    if (st != NW_OK) return st;
    float ms = 0.f;
    NW_HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    NW_HIP_TRY(hipMemcpy(&out->score, d_score, 4, hipMemcpyDeviceToHost));
    out->kernel_ms = ms;
    out->cells = n1 * n2;
    out->table_bytes = 0;
    out->strips = c->last_strips;
    out->waves = c->last_waves;
    out->substrips = c->last_sub;
    out->strip_waves = c->last_nc;
    return NW_OK;
}

int nw_align_ckpt(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, const nw_params *p,
                  const nw_ckpt_opts *co, const nw_tb_opts *o, uint8_t *host_ops, int64_t ops_cap, nw_alignment *out,
                  nw_ckpt_stats *stats) {
    nw_params def;
    if (!p) {
        nw_params_default(&def);
        p = &def;
    }
    int32_t band = 0, maxwin = 0, aim = 0;
    int st = tb_args(n1, n2, p, o, host_ops, ops_cap, out, &band, &maxwin, &aim);
    if (st != NW_OK) return st;
    if ((n1 > 0 && !s1) || (n2 > 0 && !s2)) return NW_ERR_ARG;
    int64_t K = 0, mem = 0;
    if (co) {
        if (co->block_rows < 0 || co->block_rows % 64 != 0 || co->mem_bytes < 0) return NW_ERR_ARG;
        for (int k = 0; k < 4; ++k)
            if (co->reserved[k] != 0) return NW_ERR_ARG;
        K = co->block_rows;
        mem = co->mem_bytes;
    }
    if ((st = sweep_check(n1, n2, p, K > 0 ? K : 64)) != NW_OK) return st;
    int dev;
    if ((st = have_device(p, &dev)) != NW_OK) return st;
    nw_ckpt_stats cs;
    std::memset(&cs, 0, sizeof cs);
    nw_tb_stats ts;
    std::memset(&ts, 0, sizeof ts);
    if (n1 > 0 && n2 > 0) {
        if (K > 0) {
            ckpt_need(n1, n2, K, kPlanCus, &cs);
        } else {
            if (mem == 0) {
                size_t free_b = 0, total_b = 0;
                NW_HIP_TRY(hipSetDevice(dev));
                NW_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
                mem = (int64_t)((double)free_b * 0.8);
            }
            if ((st = nw_ckpt_plan(n1, n2, mem, &cs)) != NW_OK) return st;
            K = cs.block_rows;
        }
    } else {
        cs.blocks = 1;
        cs.block_rows = std::max<int64_t>(K, 64);
    }
    if (cs.blocks <= 1) {
        // the table fits (or has no cells): nw_align's path, no sweep
        st = nw_align(s1, n1, s2, n2, p, o, host_ops, ops_cap, out, &ts);
        if (st == NW_OK) {
            cs.refill_ms = out->fill_ms;
            cs.traceback_ms = out->traceback_ms;
            cs.refill_cells = n1 * n2;
            cs.rounds = ts.rounds;
            cs.windows = ts.windows;
        }
        if (stats) *stats = cs;
        return st;
    }

    st = align_blocks(dev, s1, n1, s2, n2, p, o, K, host_ops, ops_cap, out, &cs);
    out->status = st;
    if (stats) *stats = cs;
    return st;
}

}  // extern "C"

namespace {

// nw_align_ckpt with more than one block: the sweep, then the blocks last to first
int align_blocks(int dev, const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, const nw_params *p,
                 const nw_tb_opts *o, int64_t K, uint8_t *host_ops, int64_t ops_cap, nw_alignment *out,
                 nw_ckpt_stats *csp) {
    nw_ckpt_stats &cs = *csp;
    nw_tb_stats ts;
    std::memset(&ts, 0, sizeof ts);
    int st;
    Lease L;
    if ((st = L.acquire(dev)) != NW_OK) return st;
    nw_ctx *c = L.c;
    NW_HIP_TRY(hipSetDevice(dev));
    DevBufs bufs;
    Events ev;
    int8_t *d_s1 = nullptr, *d_s2 = nullptr;
    int32_t *d_score = nullptr, *d_tab = nullptr;
    uint64_t *d_ckpt = nullptr;
    if ((st = bufs.alloc((void **)&d_s1, (size_t)n1)) != NW_OK) return st;
    if ((st = bufs.alloc((void **)&d_s2, (size_t)n2)) != NW_OK) return st;
    if ((st = bufs.alloc((void **)&d_score, 4)) != NW_OK) return st;
    if ((st = bufs.alloc((void **)&d_ckpt, (size_t)cs.ckpt_bytes)) != NW_OK) return st;
    if ((st = bufs.alloc((void **)&d_tab, (size_t)cs.block_bytes)) != NW_OK) return st;
    NW_HIP_TRY(hipEventCreate(&ev.a));
    NW_HIP_TRY(hipEventCreate(&ev.b));
    NW_HIP_TRY(hipMemcpy(d_s1, s1, (size_t)n1, hipMemcpyHostToDevice));
    NW_HIP_TRY(hipMemcpy(d_s2, s2, (size_t)n2, hipMemcpyHostToDevice));
    const int64_t pitch = nw_table_pitch(n1);
    int32_t *d_t = d_tab + nw_table_offset();  // column 1 on a 256-byte line

    // the sweep: checkpoint rows K, 2K, .. and the score
    float ms = 0.f;
    NW_HIP_TRY(hipEventRecord(ev.a, nullptr));
    if ((st = nw_ckpt_sweep_async(c, d_s1, n1, d_s2, n2, p, K, d_ckpt, d_score, nullptr)) != NW_OK) return st;
    NW_HIP_TRY(hipEventRecord(ev.b, nullptr));
    if ((st = nw_ctx_status(c, nullptr)) != NW_OK) return st;
    NW_HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
    cs.sweep_ms = ms;
    int32_t score = 0;
    NW_HIP_TRY(hipMemcpy(&score, d_score, 4, hipMemcpyDeviceToHost));

    // blocks, last to first.  The ops of block b (begin -> end) land right below
    // those of the blocks after it, at the end of the caller's buffer: before
    // block b's walk from column cj the path so far has at most (n1 - cj) + (n2 -
    // row_end) ops, so cj + rows bytes are free below it.
    std::memset(out, 0, sizeof *out);
    int64_t tail = ops_cap, cj = n1;
    for (int64_t b = cs.blocks - 1; b >= 0; --b) {
        const int64_t row0 = b * K, rows = std::min((b + 1) * K, n2) - row0;
        if (cj == 0) {
            // the path is on column 0: every remaining row is an up
            const int64_t n = row0 + rows;
            std::memset(host_ops + tail - n, 1, (size_t)n);
            tail -= n;
            break;
        }
        nw_band bd;
        std::memset(&bd, 0, sizeof bd);
        bd.halo_in = b > 0 ? d_ckpt + (b - 1) * (n1 + 1) : nullptr;
        bd.tag = NW_CKPT_TAG;
        bd.row0 = (uint32_t)row0;
        NW_HIP_TRY(hipEventRecord(ev.a, nullptr));
        if ((st = nw_fill_band_async(c, d_s1, cj, d_s2 + row0, rows, p, &bd, d_t, pitch, nullptr)) != NW_OK)
            return st;
        NW_HIP_TRY(hipEventRecord(ev.b, nullptr));
        if ((st = nw_ctx_status(c, nullptr)) != NW_OK) return st;
        NW_HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
        cs.refill_ms += ms;
        cs.refill_cells += rows * cj;
        nw_alignment al;
        uint8_t *spot = host_ops + tail - (cj + rows);
        st = nw_traceback_block(c, d_s1, cj, d_s2 + row0, rows, row0, p, d_t, pitch, o, nullptr, spot, cj + rows, &al,
                                &ts);
        if (st != NW_OK) return st;
        // the last block's corner is the sweep's score, or the checkpoints are not this table's
        if (b == cs.blocks - 1 && al.score != score) return NW_ERR_TABLE;
        cs.traceback_ms += al.traceback_ms;
        cs.rounds += ts.rounds;
        cs.windows += ts.windows;
        std::memmove(host_ops + tail - al.n_ops, spot, (size_t)al.n_ops);
        tail -= al.n_ops;
        cj = al.begin_j;
    }
    const int64_t n_ops = ops_cap - tail;
    std::memmove(host_ops, host_ops + tail, (size_t)n_ops);
    out->score = score;
    out->end_i = n2;
    out->end_j = n1;
    out->n_ops = n_ops;
    out->fill_ms = cs.sweep_ms + cs.refill_ms;
    out->traceback_ms = cs.traceback_ms;
    return NW_OK;
}

}  // namespace
