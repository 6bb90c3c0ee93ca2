// nw_host_int.h -- private to the host .cpp files of libnwhip.so (nw_capi, nw_shape,
// nw_launch, nw_links, nw_traceback, nw_hostpath, nw_ckpt): the context, the small helpers they
// share and the internal functions that cross files.  Nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nw_hip.h"
#include "nw_internal.h"

struct nw_ctx {
    int device = 0;
    int cus = 256;
    uint64_t *gran = nullptr;
    size_t gran_cap = 0;  // bytes
    void *rowpack = nullptr;
    size_t rowpack_cap = 0;
    uint8_t *meta = nullptr;   // charmap / nprof (nw::kMetaBytes)
    int32_t *scratch = nullptr;
    size_t scratch_cap = 0;
    uint32_t *ctrl = nullptr;  // nw::kCtrlWords: [0..7] per launch, [8..12] failure since the last status read
    uint32_t tagbase = 1;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int last_waves = 0;
    int last_strips = 0;
    int last_sub = 0;
    int last_nc = 0;
    uint64_t *trace = nullptr;  // debug: per-strip timestamps (nw_debug_set_trace)
    int32_t *smax = nullptr;    // SW: per-strip best cell + best / key words
    size_t smax_cap = 0;
    uint8_t *ops = nullptr;     // traceback ops (device)
    size_t ops_cap = 0;
    int64_t *swinfo = nullptr;  // SW locate key ([12])
    void *tbscratch = nullptr;  // traceback windows (nw::sw_tb_scratch_bytes)
    size_t tbscratch_cap = 0;
    int last_col0 = 0;
    int last_kernel = NW_KERNEL_STRIPS;
    uint32_t last_failure[5] = {0, 0, 0, 0, 0};  // ctrl[8..12] as the last nw_ctx_status read them
    uint64_t *look = nullptr;   // row-scan finisher look-back granules (nw_finish.hip)
    size_t look_cap = 0;
    uint32_t look_tag = 1;
    int last_finish_rows = 0;   // rows the last horizontal-band launch left to the finisher
};

#define NW_HIP_TRY(expr)                                                         \
    do {                                                                         \
        hipError_t e_ = (expr);                                                  \
        if (e_ != hipSuccess) {                                                  \
            std::fprintf(stderr, "libnwhip: %s failed: %s (%s:%d)\n", #expr,     \
                         hipGetErrorString(e_), __FILE__, __LINE__);             \
            return e_ == hipErrorOutOfMemory ? NW_ERR_OOM : NW_ERR_HIP;          \
        }                                                                        \
    } while (0)

#pragma GCC visibility push(hidden)
namespace nwh {

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// (Re)allocate a workspace buffer; returns NW_OK and sets *fresh when it is new.
inline int grow(void **p, size_t *cap, size_t need, bool *fresh = nullptr) {
    if (fresh) *fresh = false;
    if (need <= *cap) return NW_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    need = (size_t)round_up((int64_t)need, 1 << 21);
    NW_HIP_TRY(hipMalloc(p, need));
    *cap = need;
    if (fresh) *fresh = true;
    return NW_OK;
}

// Environment switches.  A caller that wants a switch fixed for the process keeps
// the value in a function-local static (NW_LINK_COARSE, NW_TR_PUB_COMPUTE,
// NW_LEAD_SLEEP); the others are read on every call, so that a test can set them
// after the library is loaded.
inline bool env_set(const char *name) { return std::getenv(name) != nullptr; }
inline bool env_flag(const char *name) {  // on = first character '1'
    const char *e = std::getenv(name);
    return e != nullptr && e[0] == '1';
}
inline int env_int(const char *name, int unset) {
    const char *e = std::getenv(name);
    return e != nullptr ? std::atoi(e) : unset;
}

// bound of an in-kernel wait: s_memrealtime runs at 100 MHz, 100000 ticks per ms
// (0 ms = the default of 20 s)
inline uint64_t timeout_ticks(int32_t ms) { return (uint64_t)(ms > 0 ? ms : 20000) * 100000ull; }

// ---- nw_shape.cpp: every decision that needs no device
struct Shape {
    int64_t nRows, nCols, nstrips, nblocks, waves, M, gstride;
    int64_t waves_max;  // resident strip workgroups (before capping at nstrips)
    int32_t K, NC;
    int32_t kernel;     // NW_KERNEL_STRIPS or NW_KERNEL_PANELS
};
Shape make_shape(int64_t n1, int64_t n2, int32_t waves_req, int32_t sub_req, int32_t nc_req, int cus,
                 int64_t col0, bool sw = false, int32_t kernel_req = NW_KERNEL_AUTO);
int32_t band_kernel(int32_t k);
bool shape_valid(const Shape &s);
bool valid_params(const nw_params *p);
bool valid_gap(int32_t gap);  // what valid_params admits as nw_params.gap in NW_MODE_NW
int tb_args(int64_t n1, int64_t n2, const nw_params *p, const nw_tb_opts *o, const uint8_t *ops, int64_t ops_cap,
            const nw_alignment *out, int32_t *band, int32_t *maxwin, int32_t *aim);
// ---- nw_launch.cpp: what every strip-chain launch shares
bool w_range_ok(const nw_params *p, int64_t n1, int64_t i_max);
bool affine_range_ok(const nw_params *p, int32_t gap_open, int64_t n1, int64_t i_max);
bool matrix_range_ok(const nw_params *p, int32_t gap_open, int64_t max_abs, int64_t n1, int64_t i_max);
bool dual_range_ok(const nw_params *p, int32_t gap_open, int32_t gap_open2, int32_t gap2, int64_t max_abs, int64_t n1,
                   int64_t i_max);
bool perm_allowed(const nw_params *p, int32_t off);
int launch_workspace(nw_ctx *c, const Shape &s, uint64_t ntags, int32_t nbl, void *stream, int64_t *qlen);
// ---- nw_hostpath.cpp: the one-shot entries' device and its kept context, held
// (locked) from host_ctx_acquire to host_ctx_release
int host_device_of(int device, int *dev);
int host_ctx_acquire(int dev, nw_ctx **c);
void host_ctx_release(int dev);
int colband_layout(int64_t n1, int64_t n2, int32_t nb, int32_t r, const nw_params *p, int cus, int64_t *sf,
                   int64_t *sc, int64_t *start, int64_t *ncols);

// ---- what the one-shot entries from host buffers share (nw_ckpt.cpp, nw_batch.cpp)
// device buffers of one call, freed when it returns
struct DevBufs {
    std::vector<void *> v;
    ~DevBufs() {
        for (void *q : v) (void)hipFree(q);
    }
    int alloc(void **q, size_t bytes) {
        *q = nullptr;
        NW_HIP_TRY(hipMalloc(q, bytes > 0 ? bytes : 1));
        v.push_back(*q);
        return NW_OK;
    }
};
struct Events {
    hipEvent_t a = nullptr, b = nullptr;
    ~Events() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};
// the one-shot entries' context of a device, held until the call returns
struct Lease {
    int dev = 0;
    bool held = false;
    nw_ctx *c = nullptr;
    int acquire(int d) {
        const int st = host_ctx_acquire(d, &c);
        dev = d;
        held = st == NW_OK;
        return st;
    }
    ~Lease() {
        if (held) host_ctx_release(dev);
    }
};
inline int have_device(const nw_params *p, int *dev) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return NW_ERR_NODEVICE;
    return host_device_of(p->device, dev);
}

}  // namespace nwh
#pragma GCC visibility pop
