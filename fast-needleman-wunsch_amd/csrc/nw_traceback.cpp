// nw_traceback.cpp -- tracebacks of a device table (kernels: nw_sw.hip):
// nw_sw_traceback from a local alignment's best cell, on the null stream, and
// nw_traceback of a global table from (n2, n1), ordered on the caller's stream.
// They share the context's ops / window workspace, the event pair that times the
// walk and how its info[] becomes an nw_alignment.
#include <algorithm>
#include <cstring>

#include "nw_host_int.h"

using namespace nwh;

namespace {

// Device buffers for a walk of up to `ops` moves over `rows` table rows; *maxwin
// is clamped to the windows (64 rows each) that many rows can use.
int tb_workspace(nw_ctx *c, size_t ops, int64_t rows, int32_t band, int32_t *maxwin) {
    int st;
    if ((st = grow((void **)&c->ops, &c->ops_cap, ops)) != NW_OK) return st;
    *maxwin = (int32_t)std::min<int64_t>(*maxwin, rows / 64 + 1);
    return grow((void **)&c->tbscratch, &c->tbscratch_cap, nw::sw_tb_scratch_bytes(*maxwin, band));
}

// the walk's time: ev0 (recorded on `s` before it) to here, waiting for `s`
int tb_elapsed(nw_ctx *c, hipStream_t s, float *ms) {
    NW_HIP_TRY(hipEventRecord(c->ev1, s));
    NW_HIP_TRY(hipStreamSynchronize(s));
    NW_HIP_TRY(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return NW_OK;
}

// info[] of run_sw_traceback / run_nw_traceback (nw_internal.h) into the alignment
// (score and fill_ms are the caller's)
void set_alignment(nw_alignment *out, int64_t end_i, int64_t end_j, const int64_t *info, float ms, int status) {
    out->end_i = end_i;
    out->end_j = end_j;
    out->n_ops = info[0];
    out->begin_i = info[1];
    out->begin_j = info[2];
    out->traceback_ms = ms;
    out->status = status;
}

}  // namespace

extern "C" {

int nw_sw_traceback(nw_ctx *c, const int8_t *d_s1, int64_t n1, const int8_t *d_s2, int64_t n2,
                    const nw_params *p, const int32_t *d_t, int64_t pitch, int64_t end_i, int64_t end_j,
                    uint8_t *host_ops, int64_t ops_cap, nw_alignment *out) {
    if (!c || !d_t || !p || !out || n1 < 0 || n2 < 0 || end_i < 0 || end_j < 0 || end_i > n2 || end_j > n1)
        return NW_ERR_ARG;
    if ((end_j > 0 && !d_s1) || (end_i > 0 && !d_s2) || (ops_cap > 0 && !host_ops) || ops_cap < 0)
        return NW_ERR_ARG;
    if (!valid_params(p) || p->mode != NW_MODE_SW) return NW_ERR_ARG;
    NW_HIP_TRY(hipSetDevice(c->device));
    // the table may have been filled on any stream (nw_fill_device_async on a
    // non-blocking stream has no ordering with the null stream used below)
    NW_HIP_TRY(hipDeviceSynchronize());
    // window geometry: band half-width and windows per round (NW_TB_BAND /
    // NW_TB_MAXWIN override them, read on every call: narrow bands and short rounds
    // for the tests)
    const int32_t band = std::max(1, std::min(256, env_int("NW_TB_BAND", nw::kTbBandDefault)));
    int32_t maxwin = std::max(1, env_int("NW_TB_MAXWIN", nw::kTbMaxWinDefault));
    int st;
    const size_t need = (size_t)std::max<int64_t>(end_i + end_j + 1, 1);
    if ((st = tb_workspace(c, need, end_i, band, &maxwin)) != NW_OK) return st;
    NW_HIP_TRY(hipEventRecord(c->ev0, nullptr));
    int64_t info[10];
    const int he = nw::run_sw_traceback(d_t, pitch, n1, (const uint8_t *)d_s1, (const uint8_t *)d_s2, p->match,
                                        p->mismatch, p->gap, end_i, end_j, c->ops, (int64_t)need, c->tbscratch,
                                        maxwin, band, info, nullptr);
    if (he != hipSuccess) {
        std::fprintf(stderr, "libnwhip: SW traceback failed: %s\n", hipGetErrorString((hipError_t)he));
        return NW_ERR_HIP;
    }
    float ms = 0.f;
    if ((st = tb_elapsed(c, nullptr, &ms)) != NW_OK) return st;
    if (env_set("NW_TB_DEBUG"))
        std::fprintf(stderr, "nw_sw_traceback: %lld moves, %lld rounds, %lld windows (band %d)\n", (long long)info[0],
                     (long long)info[4], (long long)info[5], band);
    std::memset(out, 0, sizeof *out);
    set_alignment(out, end_i, end_j, info, ms, info[3] == 0 ? NW_OK : NW_ERR_HIP);
    NW_HIP_TRY(hipMemcpy(&out->score, d_t + end_i * pitch + end_j, 4, hipMemcpyDeviceToHost));
    if (info[3] != 0) return out->status;
    if (info[0] > ops_cap) return NW_ERR_ARG;
    if (info[0] > 0) {
        // the kernel walks end -> begin; hand the ops over begin -> end
        NW_HIP_TRY(hipMemcpy(host_ops, c->ops, (size_t)info[0], hipMemcpyDeviceToHost));
        std::reverse(host_ops, host_ops + info[0]);
    }
    return NW_OK;
}

int nw_traceback(nw_ctx *c, const int8_t *d_s1, int64_t n1, const int8_t *d_s2, int64_t n2, const nw_params *p,
                 const int32_t *d_t, int64_t pitch, const nw_tb_opts *o, void *stream, uint8_t *host_ops,
                 int64_t ops_cap, nw_alignment *out, nw_tb_stats *stats) {
    int32_t band = 0, maxwin = 0, aim = 0;
    int st = tb_args(n1, n2, p, o, host_ops, ops_cap, out, &band, &maxwin, &aim);
    if (st != NW_OK) return st;
    if (!c || !d_t || pitch < n1 + 1 || (n1 > 0 && !d_s1) || (n2 > 0 && !d_s2)) return NW_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    NW_HIP_TRY(hipSetDevice(c->device));
    if ((st = tb_workspace(c, (size_t)std::max<int64_t>(n1 + n2, 1), n2, band, &maxwin)) != NW_OK) return st;
    // everything below is ordered on the caller's stream, after its fill
    NW_HIP_TRY(hipEventRecord(c->ev0, s));
    int64_t info[10];
    const int he = nw::run_nw_traceback(d_t, pitch, n1, n2, (const uint8_t *)d_s1, (const uint8_t *)d_s2, p->match,
                                        p->mismatch, p->gap, c->ops, n1 + n2, c->tbscratch, maxwin, band, aim, info,
                                        stream);
    if (he != hipSuccess) {
        std::fprintf(stderr, "libnwhip: traceback failed: %s\n", hipGetErrorString((hipError_t)he));
        return NW_ERR_HIP;
    }
    std::memset(out, 0, sizeof *out);
    out->end_i = n2;
    out->end_j = n1;
    if (stats) {
        stats->rounds = (int32_t)info[4];
        stats->windows = (int32_t)info[5];
        stats->band = band;
        stats->max_windows = maxwin;
        stats->tail_ops = info[6];
    }
    // a global path never has more than n1 + n2 ops: a full buffer (1) is a bad table too
    const bool ok = info[3] == 0;
    NW_HIP_TRY(hipMemcpyAsync(&out->score, d_t + n2 * pitch + n1, 4, hipMemcpyDeviceToHost, s));
    if (ok && info[0] > 0) NW_HIP_TRY(hipMemcpyAsync(host_ops, c->ops, (size_t)info[0], hipMemcpyDeviceToHost, s));
    float ms = 0.f;
    if ((st = tb_elapsed(c, s, &ms)) != NW_OK) return st;
    if (!ok) {  // (no walk to report)
        out->traceback_ms = ms;
        out->status = NW_ERR_TABLE;
        return NW_ERR_TABLE;
    }
    set_alignment(out, n2, n1, info, ms, NW_OK);  // (info[1..2] = (0, 0): the walk ended in the corner)
    // the kernels walk end -> begin; hand the ops over begin -> end
    std::reverse(host_ops, host_ops + info[0]);
    return NW_OK;
}

// One row block of a checkpointed alignment (nw_align_ckpt): the table holds global
// rows row0 .. row0 + rows (local row 0 = the checkpoint row, as nw_fill_band_async
// leaves it).  With row0 = 0 the block is the top of the table and the walk is
// nw_traceback's.
int nw_traceback_block(nw_ctx *c, const int8_t *d_s1, int64_t n1, const int8_t *d_s2_block, int64_t rows,
                       int64_t row0, const nw_params *p, const int32_t *d_t, int64_t pitch, const nw_tb_opts *o,
                       void *stream, uint8_t *host_ops, int64_t ops_cap, nw_alignment *out, nw_tb_stats *stats) {
    int32_t band = 0, maxwin = 0, aim = 0;
    int st = tb_args(n1, rows, p, o, host_ops, ops_cap, out, &band, &maxwin, &aim);
    if (st != NW_OK) return st;
    if (row0 < 0 || row0 + rows >= INT32_MAX) return NW_ERR_ARG;
    if (!c || !d_t || pitch < n1 + 1 || (n1 > 0 && !d_s1) || (rows > 0 && !d_s2_block)) return NW_ERR_ARG;
    if (row0 == 0) {
        st = nw_traceback(c, d_s1, n1, d_s2_block, rows, p, d_t, pitch, o, stream, host_ops, ops_cap, out, stats);
        return st;
    }
    hipStream_t s = (hipStream_t)stream;
    NW_HIP_TRY(hipSetDevice(c->device));
    if ((st = tb_workspace(c, (size_t)std::max<int64_t>(n1 + rows, 1), rows, band, &maxwin)) != NW_OK) return st;
    NW_HIP_TRY(hipEventRecord(c->ev0, s));
    int64_t info[10];
    const int he = nw::run_nw_traceback_block(d_t, pitch, n1, rows, row0, (const uint8_t *)d_s1,
                                              (const uint8_t *)d_s2_block, p->match, p->mismatch, p->gap, c->ops,
                                              n1 + rows, c->tbscratch, maxwin, band, aim, info, stream);
    if (he != hipSuccess) {
        std::fprintf(stderr, "libnwhip: traceback failed: %s\n", hipGetErrorString((hipError_t)he));
        return NW_ERR_HIP;
    }
    std::memset(out, 0, sizeof *out);
    if (stats) {
        stats->rounds = (int32_t)info[4];
        stats->windows = (int32_t)info[5];
        stats->band = band;
        stats->max_windows = maxwin;
        stats->tail_ops = info[6];
    }
    const bool ok = info[3] == 0;
    NW_HIP_TRY(hipMemcpyAsync(&out->score, d_t + rows * pitch + n1, 4, hipMemcpyDeviceToHost, s));
    if (ok && info[0] > 0) NW_HIP_TRY(hipMemcpyAsync(host_ops, c->ops, (size_t)info[0], hipMemcpyDeviceToHost, s));
    float ms = 0.f;
    if ((st = tb_elapsed(c, s, &ms)) != NW_OK) return st;
    if (!ok) {
        out->end_i = row0 + rows;
        out->end_j = n1;
        out->traceback_ms = ms;
        out->status = NW_ERR_TABLE;
        return NW_ERR_TABLE;
    }
    // info[1..2] = (0, the column where the walk reached local row 0)
    set_alignment(out, row0 + rows, n1, info, ms, NW_OK);
    out->begin_i = row0 + info[1];
    std::reverse(host_ops, host_ops + info[0]);
    return NW_OK;
}

int64_t nw_debug_tb_shift(int64_t k, int64_t is, int64_t js, int32_t band, int32_t aim, int64_t row0) {
    return nw::tb_shift_host(k, is, js, band, aim, row0);
}

}  // extern "C"
