// nw_capi.cpp -- C ABI of libnwhip.so (declared in include/nw_hip.h): parameters,
// status texts, the table layout, the context and the debug hooks.  The rest of
// the ABI lives next to what it does: nw_shape.cpp (shapes, band layouts),
// nw_launch.cpp (the fills on device buffers), nw_links.cpp (halo / feed / link
// buffers, IPC), nw_traceback.cpp, nw_hostpath.cpp (host-buffer entry points) and
// nw_bdna.cpp (.bdna I/O); nw_host_int.h is what they share.
#include <cstring>

#include "nw_host_int.h"

using namespace nwh;

extern "C" {

void nw_params_default(nw_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->match = 1;      // needleman-wunsch.hpp:11
    p->mismatch = 0;   // needleman-wunsch.hpp:12
    p->gap = -1;       // needleman-wunsch.hpp:13
    p->mode = NW_MODE_NW;
    p->waves = 0;
    p->device = -1;
}

const char *nw_strerror(int status) {
    switch (status) {
        case NW_OK: return "ok";
        case NW_ERR_ARG: return "invalid argument";
        case NW_ERR_HIP: return "HIP runtime error";
        case NW_ERR_OOM: return "out of device memory";
        case NW_ERR_TIMEOUT: return "in-kernel hand-off watchdog expired";
        case NW_ERR_NODEVICE: return "no gfx950 device";
        case NW_ERR_UNSUPPORTED: return "unsupported";
        case NW_ERR_TABLE: return "traceback met a cell no move reproduces (not a table of these parameters)";
        default: return "unknown status";
    }
}

const char *nw_version(void) {
    static char buf[256];
    std::snprintf(buf, sizeof buf, "libnwhip gfx950 %s", nw::kernel_variant());
    return buf;
}

// nCols = n1 + 1 rounded up to 64, with >= 3 columns of slack after column n1 so
// that the 16-byte store holding column n1 stays inside the row when the strips
// start at column 1 (nw_table_offset)
int64_t nw_table_pitch(int64_t n1) { return round_up(n1 + 4, nw::kWave); }

int64_t nw_table_bytes(int64_t n1, int64_t n2) {
    return round_up(n2 + 1, nw::kWave) * nw_table_pitch(n1) * (int64_t)sizeof(int32_t);
}

int64_t nw_table_offset(void) { return nw::kWave - 1; }

int64_t nw_strip_lds_bytes(int32_t substrips, int32_t strip_waves) {
    if (!nw::shape_ok(substrips, strip_waves)) return -1;
    return nw::lds_bytes(substrips, strip_waves);
}

int64_t nw_panel_lds_bytes(int32_t substrips, int32_t strip_waves) {
    if (!nw::panel_shape_ok(substrips, strip_waves)) return -1;
    return nw::panel_lds_bytes(substrips, strip_waves);
}

int64_t nw_ctx_workspace_bytes(int64_t n1, int64_t n2, int32_t waves) {
    Shape s = make_shape(n1, n2, waves, 0, 0, 256, 1);
    return s.M * s.gstride * 8 + nw::rowpack_len((int32_t)s.nblocks) * 16 +
           s.waves * nw::kScratchWords * 4 + 16;
}

int nw_ctx_create(int device, nw_ctx **out) {
    if (!out) return NW_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return NW_ERR_NODEVICE;
    if (device < 0) NW_HIP_TRY(hipGetDevice(&device));
    if (device >= ndev) return NW_ERR_ARG;
    NW_HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    NW_HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        std::fprintf(stderr, "libnwhip: device %d is %s, kernels are built for gfx950\n", device,
                     prop.gcnArchName);
        return NW_ERR_NODEVICE;
    }
    nw_ctx *c = new nw_ctx();
    c->device = device;
    c->cus = prop.multiProcessorCount;
    if (hipMalloc(&c->ctrl, nw::kCtrlWords * 4) != hipSuccess || hipMemset(c->ctrl, 0, nw::kCtrlWords * 4) != hipSuccess ||
        hipMalloc(&c->meta, nw::kMetaBytes) != hipSuccess || hipMemset(c->meta, 0, nw::kMetaBytes) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
        nw_ctx_destroy(c);
        return NW_ERR_HIP;
    }
    *out = c;
    return NW_OK;
}

void nw_ctx_destroy(nw_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->gran) (void)hipFree(c->gran);
    if (c->rowpack) (void)hipFree(c->rowpack);
    if (c->meta) (void)hipFree(c->meta);
    if (c->scratch) (void)hipFree(c->scratch);
    if (c->ctrl) (void)hipFree(c->ctrl);
    if (c->smax) (void)hipFree(c->smax);
    if (c->ops) (void)hipFree(c->ops);
    if (c->swinfo) (void)hipFree(c->swinfo);
    if (c->tbscratch) (void)hipFree(c->tbscratch);
    if (c->look) (void)hipFree(c->look);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    delete c;
}

int nw_ctx_status(nw_ctx *c, void *stream) {
    if (!c) return NW_ERR_ARG;
    NW_HIP_TRY(hipSetDevice(c->device));
    uint32_t w[nw::kCtrlWords] = {};
    NW_HIP_TRY(hipMemcpyAsync(w, c->ctrl, sizeof w, hipMemcpyDeviceToHost, (hipStream_t)stream));
    NW_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    // the last launch's error word, or a failure any earlier launch (or a link wait)
    // recorded since the last read -- read and cleared (nw_link.hip nw_ctrl_reset)
    const bool failed = (w[1] != 0 && w[13] == 0) || w[8] != 0;
    if (w[8] != 0 || w[12] != 0) {
        for (int k = 0; k < 5; ++k) c->last_failure[k] = w[8 + k];
        // the last launch (poisoned by the folded failure, or failed on its own) is
        // not folded into [12] until the next reset: count it here
        if (w[1] != 0 && w[13] == 0) c->last_failure[4] = w[12] + 1;
    } else if (w[1] != 0 && w[13] == 0) {  // the last launch failed (not folded in yet)
        c->last_failure[0] = w[1];
        c->last_failure[1] = w[2];
        c->last_failure[2] = w[3];
        c->last_failure[3] = w[4];
        c->last_failure[4] = 1;
    }
    if (failed) {
        // clear the record and mark the last launch's words as read (ctrl[13])
        static const uint32_t cleared[nw::kCtrlWords - 8] = {0, 0, 0, 0, 0, 1, 0, 0};
        NW_HIP_TRY(hipMemcpyAsync(c->ctrl + 8, cleared, sizeof cleared, hipMemcpyHostToDevice, (hipStream_t)stream));
        NW_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    }
    return failed ? NW_ERR_TIMEOUT : NW_OK;
}

// Debug hook: the control words of the last launch (ticket, error code, watchdog
// site / need / seen -- nw_fill.hip give_up); include/nw_hip.h documents them.
int nw_debug_ctrl(nw_ctx *c, uint32_t *out8) {
    if (!c || !out8) return NW_ERR_ARG;
    NW_HIP_TRY(hipSetDevice(c->device));
    NW_HIP_TRY(hipDeviceSynchronize());
    NW_HIP_TRY(hipMemcpy(out8, c->ctrl, 32, hipMemcpyDeviceToHost));
    return NW_OK;
}

// Debug hook: the first failure recorded since the status before last was read
// (code, site word, need, seen, failed launches) -- what nw_ctx_status cleared
// when it last reported NW_ERR_TIMEOUT -- or, before any such read, the live words.
int nw_debug_failure(nw_ctx *c, uint32_t *out5) {
    if (!c || !out5) return NW_ERR_ARG;
    NW_HIP_TRY(hipSetDevice(c->device));
    NW_HIP_TRY(hipDeviceSynchronize());
    uint32_t w[nw::kCtrlWords] = {};
    NW_HIP_TRY(hipMemcpy(w, c->ctrl, sizeof w, hipMemcpyDeviceToHost));
    if (w[8] != 0 || w[12] != 0) {
        for (int k = 0; k < 5; ++k) out5[k] = w[8 + k];
        if (w[1] != 0 && w[13] == 0) out5[4] = w[12] + 1;  // + the last launch (nw_ctx_status)
    } else
        for (int k = 0; k < 5; ++k) out5[k] = c->last_failure[k];
    return NW_OK;
}

// Debug hook: per-strip trace buffer, device memory of at least
// strips * nw_debug_trace_words() uint64 (see nwhip.Context.set_trace); NULL = off.
int nw_debug_set_trace(nw_ctx *c, void *d_trace) {
    if (!c) return NW_ERR_ARG;
    c->trace = (uint64_t *)d_trace;
    return NW_OK;
}

int32_t nw_debug_trace_words(void) { return nw::kTraceWords; }

}  // extern "C"
