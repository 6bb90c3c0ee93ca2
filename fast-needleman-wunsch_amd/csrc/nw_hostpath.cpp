// nw_hostpath.cpp -- host-buffer entry points of libnwhip.so (the drop-in path).
// The one-shot nw_fill() is what the reference-signature TU
// (dropin/needleman-wunsch-hip.cpp) calls; it replaces the reference fills'
// needlemanWunsch() (serial.cpp:4, sentinel-mt.cpp:4, idxarray-mt.cpp:4) as called
// from driver.cpp:28.
//
// One HostPath per device, created on first use and kept: the context, the
// device table and sequence buffers (grow-only: a caller looping over pairs pays
// no hipMalloc / hipFree of the table per call), a non-blocking copy stream and
// three pinned staging chunks.  The table comes back to the caller's (pageable)
// buffer through the staging chunks: DMA of chunk k+1 overlaps the threaded
// memcpy of chunk k into the caller's rows (tools/d2h_bench.cpp measured the
// alternatives; DESIGN.md "drop-in path").  The chunk plan, the thread count and
// the threaded memcpy are csrc/nw_hostcopy.h (no HIP: a CPU program can run them).
// nw_host_release frees it all.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "nw_host_int.h"
#include "nw_hostcopy.h"

using namespace nwh;

extern "C" {  // (HostPath's helpers have been in the library's symbol table from the start: kept so)
namespace {

struct HostPath {
    std::mutex mu;
    nw_ctx *c = nullptr;
    int32_t *tab = nullptr;  // 256-byte aligned allocation; the table starts nw_table_offset() in
    size_t tab_cap = 0;
    int8_t *s1 = nullptr, *s2 = nullptr;
    size_t s1_cap = 0, s2_cap = 0;
    char *stage[kStages] = {nullptr, nullptr, nullptr};
    size_t stage_cap = 0;  // bytes per staging chunk (grow-only: nw_hostcopy.h copy_plan)
    hipStream_t copy = nullptr;
    hipEvent_t ev[kStages] = {nullptr, nullptr, nullptr};
};

// tables up to this size stay cached between calls; a larger one is released
// when its call returns (it would crowd out the caller's own device work)
constexpr size_t kKeepTableBytes = 16ull << 30;
HostPath g_host[64];

void host_trim(HostPath &h) {
    if (h.tab && h.tab_cap > kKeepTableBytes) {
        (void)hipFree(h.tab);
        h.tab = nullptr;
        h.tab_cap = 0;
    }
}

void host_free(HostPath &h) {
    if (h.c) (void)hipSetDevice(h.c->device);
    if (h.tab) (void)hipFree(h.tab);
    if (h.s1) (void)hipFree(h.s1);
    if (h.s2) (void)hipFree(h.s2);
    for (int k = 0; k < kStages; ++k) {
        if (h.stage[k]) (void)hipHostFree(h.stage[k]);
        if (h.ev[k]) (void)hipEventDestroy(h.ev[k]);
        h.stage[k] = nullptr;
        h.ev[k] = nullptr;
    }
    h.stage_cap = 0;
    if (h.copy) (void)hipStreamDestroy(h.copy);
    nw_ctx_destroy(h.c);
    h.c = nullptr;
    h.tab = nullptr;
    h.s1 = h.s2 = nullptr;
    h.tab_cap = h.s1_cap = h.s2_cap = 0;
    h.copy = nullptr;
}

// Device and sequence buffers for an n1 x n2 table; copies s1 / s2 in.
int host_prepare(HostPath &h, int dev, const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2,
                 int32_t **d_t, int64_t *pitch) {
    int st;
    if (!h.c && (st = nw_ctx_create(dev, &h.c)) != NW_OK) return st;
    NW_HIP_TRY(hipSetDevice(dev));
    *pitch = nw_table_pitch(n1);
    // column 1 on a 256-byte line: the allocation (256-byte aligned) + nw_table_offset
    const size_t need = (size_t)nw_table_bytes(n1, n2) + 256;
    if (need > h.tab_cap) {  // (grow drops the old buffer first: one table at a time)
        if ((st = grow((void **)&h.tab, &h.tab_cap, need)) != NW_OK) return st;
    }
    if ((st = grow((void **)&h.s1, &h.s1_cap, (size_t)std::max<int64_t>(n1, 1))) != NW_OK) return st;
    if ((st = grow((void **)&h.s2, &h.s2_cap, (size_t)std::max<int64_t>(n2, 1))) != NW_OK) return st;
    if (n1 > 0) NW_HIP_TRY(hipMemcpy(h.s1, s1, (size_t)n1, hipMemcpyHostToDevice));
    if (n2 > 0) NW_HIP_TRY(hipMemcpy(h.s2, s2, (size_t)n2, hipMemcpyHostToDevice));
    *d_t = h.tab + (n1 >= 1 ? nw_table_offset() : 0);  // (no column 1 when n1 = 0)
    return NW_OK;
}

int copy_threads() { return copy_threads_of(std::getenv("NW_COPY_THREADS"), std::thread::hardware_concurrency()); }

// Rows 0..n2 (n1 + 1 int32 each) of the device table into host rows of
// `stride` int32 (the reference layout: stride = n1 + 1), through the pinned
// staging chunks.
int host_staging(HostPath &h, size_t want) {  // want: bytes per chunk (copy_plan, stage_want)
    if (want > h.stage_cap) {
        for (int k = 0; k < kStages; ++k) {
            if (h.stage[k]) (void)hipHostFree(h.stage[k]);
            h.stage[k] = nullptr;
        }
        h.stage_cap = 0;
        for (int k = 0; k < kStages; ++k)
            NW_HIP_TRY(hipHostMalloc((void **)&h.stage[k], want, hipHostMallocCoherent));
        h.stage_cap = want;
    }
    for (int k = 0; k < kStages; ++k)
        if (!h.ev[k]) NW_HIP_TRY(hipEventCreateWithFlags(&h.ev[k], hipEventDisableTiming));
    if (!h.copy) NW_HIP_TRY(hipStreamCreateWithFlags(&h.copy, hipStreamNonBlocking));
    return NW_OK;
}

int host_copy_back(HostPath &h, const int32_t *d_t, int64_t pitch, int64_t n1, int64_t n2, int32_t *host,
                   int64_t stride) {
    int st;
    const size_t w = (size_t)(n1 + 1) * 4;
    const int64_t rows = n2 + 1;
    const CopyPlan plan = copy_plan(w * (size_t)rows, w, rows, h.stage_cap);
    if ((st = host_staging(h, plan.stage_cap)) != NW_OK) return st;
    if (plan.direct) {  // one row wider than a chunk
        NW_HIP_TRY(hipMemcpy2D(host, (size_t)stride * 4, d_t, (size_t)pitch * 4, w, (size_t)rows,
                               hipMemcpyDeviceToHost));
        return NW_OK;
    }
    const int64_t nch = plan.nch;
    const int threads = copy_threads();
    auto issue = [&](int64_t ch) -> hipError_t {
        const int64_t r0 = plan.first_row(ch), nr = plan.rows_of(ch, rows);
        hipError_t e = hipMemcpy2DAsync(h.stage[ch % kStages], w, d_t + r0 * pitch, (size_t)pitch * 4, w,
                                        (size_t)nr, hipMemcpyDeviceToHost, h.copy);
        return e == hipSuccess ? hipEventRecord(h.ev[ch % kStages], h.copy) : e;
    };
    // the fill ran on the null stream (synchronous), so the copy stream sees the table
    for (int64_t ch = 0; ch < std::min<int64_t>(kStages, nch); ++ch) NW_HIP_TRY(issue(ch));
    double t_dma = 0, t_cpy = 0;
    auto tnow = [] { return std::chrono::steady_clock::now(); };
    auto sec = [](auto a, auto b) { return std::chrono::duration<double>(b - a).count(); };
    for (int64_t ch = 0; ch < nch; ++ch) {
        const auto a0 = tnow();
        NW_HIP_TRY(hipEventSynchronize(h.ev[ch % kStages]));
        const auto a1 = tnow();
        t_dma += sec(a0, a1);
        const int64_t r0 = plan.first_row(ch), nr = plan.rows_of(ch, rows);
        const char *src = h.stage[ch % kStages];
        if (stride * 4 == (int64_t)w) {
            par_memcpy((char *)(host + r0 * stride), src, (size_t)nr * w, threads);
        } else {
            for (int64_t r = 0; r < nr; ++r) std::memcpy(host + (r0 + r) * stride, src + (size_t)r * w, w);
        }
        t_cpy += sec(a1, tnow());
        if (ch + kStages < nch) NW_HIP_TRY(issue(ch + kStages));
    }
    if (env_set("NW_HOST_TIMING"))
        std::fprintf(stderr, "  copy back: %lld chunks of %zu MiB, %d threads: waiting on DMA %.1f ms, copying %.1f ms\n",
                     (long long)nch, h.stage_cap >> 20, threads, t_dma * 1e3, t_cpy * 1e3);
    return NW_OK;
}

// device < 0: the current one; the path keeps one HostPath for each of devices 0..63
int host_device(int device, int *dev) {
    *dev = device;
    if (*dev < 0 && hipGetDevice(dev) != hipSuccess) return NW_ERR_NODEVICE;
    if (*dev < 0 || *dev >= 64) return NW_ERR_ARG;
    return NW_OK;
}

}  // namespace
}  // extern "C"

namespace {

using Clock = std::chrono::steady_clock;
double ms_between(Clock::time_point a, Clock::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
}

// What every one-shot entry does around its own step: under device dev's lock
// (host_device: the entries call it themselves, its refusal leaves *out untouched), the
// buffers and the sequences' copy in, the fill on the null stream (*r: its result),
// then -- if all went well -- `then(h, d_t, pitch, *r)`, the entry's own step on
// the filled device table.  phase_ms (optional): host time of the prepare and of
// the fill.
template <class Then>
int host_run(int dev, const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, const nw_params *p,
             nw_result *r, Then then, double *phase_ms = nullptr) {
    HostPath &h = g_host[dev];
    std::lock_guard<std::mutex> lock(h.mu);
    int32_t *d_t = nullptr;
    int64_t pitch = 0;
    std::memset(r, 0, sizeof *r);
    const auto t0 = Clock::now();
    int st = host_prepare(h, dev, s1, n1, s2, n2, &d_t, &pitch);
    const auto t1 = Clock::now();
    if (st == NW_OK) st = nw_fill_device(h.c, h.s1, n1, h.s2, n2, p, d_t, pitch, nullptr, r);
    if (phase_ms) {
        phase_ms[0] = ms_between(t0, t1);
        phase_ms[1] = ms_between(t1, Clock::now());
    }
    if (st == NW_OK) st = then(h, d_t, pitch, *r);
    host_trim(h);
    return st;
}

}  // namespace

namespace nwh {

int host_device_of(int device, int *dev) { return host_device(device, dev); }

int host_ctx_acquire(int dev, nw_ctx **c) {
    HostPath &h = g_host[dev];
    h.mu.lock();
    int st = NW_OK;
    if (!h.c) st = nw_ctx_create(dev, &h.c);
    if (st != NW_OK) {
        h.mu.unlock();
        return st;
    }
    *c = h.c;
    return NW_OK;
}

void host_ctx_release(int dev) { g_host[dev].mu.unlock(); }

}  // namespace nwh

extern "C" {

int nw_host_warmup(int device) {
    int dev, st;
    if ((st = host_device(device, &dev)) != NW_OK) return st;
    HostPath &h = g_host[dev];
    std::lock_guard<std::mutex> lock(h.mu);
    if (!h.c && (st = nw_ctx_create(dev, &h.c)) != NW_OK) return st;
    NW_HIP_TRY(hipSetDevice(dev));
    return host_staging(h, stage_want(kStageMax * kStages));
}

void nw_host_release(int device) {
    for (int d = 0; d < 64; ++d) {
        if (device >= 0 && d != device) continue;
        std::lock_guard<std::mutex> lock(g_host[d].mu);
        host_free(g_host[d]);
    }
}

int nw_sw_align(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, const nw_params *p,
                uint8_t *host_ops, int64_t ops_cap, nw_alignment *out) {
    if (!p || p->mode != NW_MODE_SW || !out || n1 < 0 || n2 < 0 || (n1 > 0 && !s1) || (n2 > 0 && !s2))
        return NW_ERR_ARG;
    int dev, st;
    if ((st = host_device(p->device, &dev)) != NW_OK) return st;
    nw_result r;
    st = host_run(dev, s1, n1, s2, n2, p, &r, [&](HostPath &h, int32_t *d_t, int64_t pitch, const nw_result &res) {
        return nw_sw_traceback(h.c, h.s1, n1, h.s2, n2, p, d_t, pitch, res.end_i, res.end_j, host_ops, ops_cap, out);
    });
    if (st == NW_OK) out->fill_ms = r.kernel_ms;
    out->status = st;
    return st;
}

int nw_align(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, const nw_params *p, const nw_tb_opts *o,
             uint8_t *host_ops, int64_t ops_cap, nw_alignment *out, nw_tb_stats *stats) {
    nw_params def;
    if (!p) {
        nw_params_default(&def);
        p = &def;
    }
    int32_t band = 0, maxwin = 0, aim = 0;
    int st = tb_args(n1, n2, p, o, host_ops, ops_cap, out, &band, &maxwin, &aim);
    if (st != NW_OK) return st;
    if ((n1 > 0 && !s1) || (n2 > 0 && !s2)) return NW_ERR_ARG;
    int dev, ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return NW_ERR_NODEVICE;
    if ((st = host_device(p->device, &dev)) != NW_OK) return st;  // (also for a table with no cells)
    if (n1 == 0 || n2 == 0) {
        // no table: the path runs along row 0 (lefts) or column 0 (ups)
        const int64_t n = std::max(n1, n2);
        std::memset(out, 0, sizeof *out);
        if (n > 0) std::memset(host_ops, n2 > 0 ? 1 : 2, (size_t)n);
        out->score = (int32_t)(p->gap * n);
        out->end_i = n2;
        out->end_j = n1;
        out->n_ops = n;
        if (stats) {
            std::memset(stats, 0, sizeof *stats);
            stats->band = band;
            stats->max_windows = maxwin;
            stats->tail_ops = n;
        }
        return NW_OK;
    }
    nw_result r;
    st = host_run(dev, s1, n1, s2, n2, p, &r, [&](HostPath &h, int32_t *d_t, int64_t pitch, const nw_result &) {
        return nw_traceback(h.c, h.s1, n1, h.s2, n2, p, d_t, pitch, o, nullptr, host_ops, ops_cap, out, stats);
    });
    if (st == NW_OK) out->fill_ms = r.kernel_ms;
    out->status = st;
    return st;
}

int nw_fill(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, const nw_params *p,
            int32_t *host_t, nw_result *out) {
    nw_params def;
    if (!p) {
        nw_params_default(&def);
        p = &def;
    }
    if (n1 < 0 || n2 < 0 || (n1 > 0 && !s1) || (n2 > 0 && !s2)) return NW_ERR_ARG;
    int dev, st;
    if ((st = host_device(p->device, &dev)) != NW_OK) return st;
    nw_result r;
    double phase_ms[2] = {0, 0}, copy_ms = 0;
    st = host_run(dev, s1, n1, s2, n2, p, &r, [&](HostPath &h, int32_t *d_t, int64_t pitch, const nw_result &) {
        const auto t2 = Clock::now();
        const int cs = host_t ? host_copy_back(h, d_t, pitch, n1, n2, host_t, n1 + 1) : NW_OK;
        copy_ms = ms_between(t2, Clock::now());
        return cs;
    }, phase_ms);
    if (env_set("NW_HOST_TIMING"))
        std::fprintf(stderr, "nw_fill: prepare (context, buffers, H2D) %.1f ms, fill %.1f ms (kernel %.1f), "
                     "copy back %.1f ms (%.1f GB/s)\n", phase_ms[0], phase_ms[1], r.kernel_ms, copy_ms,
                     host_t ? (double)(n1 + 1) * (n2 + 1) * 4 / (copy_ms * 1e6) : 0.0);
    r.status = st;
    if (out) *out = r;
    return st;
}

int nw_fill_emb(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, const nw_params *p,
                int32_t *host_t, nw_result *out) {
    // The emb layout of src/idxarray/idxarray-emb-mt.cpp:7-37 / src/common/driver2.cpp:20-22:
    // nCols = n1 + 2; column 0 holds each row's progress counter, which the reference
    // fill leaves at its final value nCols (:49, the row loop's `int& j`, and :36 for
    // row 0); columns 1 .. n1+1 hold the serial table.  Fill as nw_fill, copy the
    // table into columns 1.., then write column 0.
    nw_params def;
    if (!p) {
        nw_params_default(&def);
        p = &def;
    }
    if (!host_t || n1 < 0 || n2 < 0 || (n1 > 0 && !s1) || (n2 > 0 && !s2)) return NW_ERR_ARG;
    int dev, st;
    if ((st = host_device(p->device, &dev)) != NW_OK) return st;
    nw_result r;
    st = host_run(dev, s1, n1, s2, n2, p, &r, [&](HostPath &h, int32_t *d_t, int64_t pitch, const nw_result &) {
        const int cs = host_copy_back(h, d_t, pitch, n1, n2, host_t + 1, n1 + 2);
        if (cs == NW_OK)
            for (int64_t i = 0; i <= n2; ++i) host_t[i * (n1 + 2)] = (int32_t)(n1 + 2);
        return cs;
    });
    r.status = st;
    if (out) *out = r;
    return st;
}

}  // extern "C"
