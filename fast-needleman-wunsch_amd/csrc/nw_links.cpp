// nw_links.cpp -- what bands on different GPUs or in different processes share:
// halo, feed and link buffers (allocation, flow control) and their HIP IPC handles.
#include <cstring>

#include "nw_host_int.h"

using namespace nwh;

namespace {

// A halo / feed buffer: its own allocation (so that HIP IPC exports exactly it),
// fine-grained -- the producing kernel on ANOTHER GPU writes it over xGMI with
// system-scope stores while this GPU's kernel polls it with system-scope loads,
// and system-scope coherence between agents is what fine-grained memory gives
// (coarse-grained memory is only coherent at agent scope).
// NW_LINK_COARSE=1 (diagnostics, one device and one process only): plain
// coarse-grained memory, to tell the feed's uncached-memory cost from the
// protocol's.  Coarse-grained memory is coherent at agent
// scope only, so such a buffer is never exported (nw_ipc_get_handle refuses).
bool link_coarse() {
    static const bool coarse = [] {
        const bool on = env_flag("NW_LINK_COARSE");
        if (on)
            std::fprintf(stderr, "libnwhip: NW_LINK_COARSE=1: halo / feed / link buffers are coarse-grained "
                                 "(single-device diagnostics; IPC export refused)\n");
        return on;
    }();
    return coarse;
}

// `bytes` of zeroed link memory on `device` (< 0: the current one)
int alloc_zeroed_link(int device, size_t bytes, void **out) {
    if (device >= 0) NW_HIP_TRY(hipSetDevice(device));
    void *q = nullptr;
    hipError_t e = link_coarse() ? hipMalloc(&q, bytes) : hipExtMallocWithFlags(&q, bytes, hipDeviceMallocFinegrained);
    if (e != hipSuccess) return e == hipErrorOutOfMemory ? NW_ERR_OOM : NW_ERR_HIP;
    if (hipMemset(q, 0, bytes) != hipSuccess) {
        (void)hipFree(q);
        return NW_ERR_HIP;
    }
    *out = q;
    return NW_OK;
}

}  // namespace

extern "C" {

int64_t nw_feed_bytes(int64_t n2) {
    return n2 < 0 ? 0 : round_up(n2 + 1, nw::kWave) * (int64_t)sizeof(uint64_t);
}

int nw_feed_alloc(int device, int64_t n2, uint64_t **d_feed) {
    if (!d_feed || n2 < 0) return NW_ERR_ARG;
    *d_feed = nullptr;
    return alloc_zeroed_link(device, (size_t)nw_feed_bytes(n2), (void **)d_feed);
}

int64_t nw_halo_bytes(int64_t n1) { return n1 < 0 ? 0 : (n1 + 1) * (int64_t)sizeof(uint64_t); }

int nw_halo_alloc(int device, int64_t n1, uint64_t **d_halo) { return nw_halo_alloc_regions(device, n1, 1, d_halo); }

int nw_halo_alloc_regions(int device, int64_t n1, int32_t nregions, uint64_t **d_halo) {
    if (!d_halo || n1 < 0 || nregions < 1) return NW_ERR_ARG;
    *d_halo = nullptr;
    return alloc_zeroed_link(device, (size_t)nw_halo_bytes(n1) * (size_t)nregions, (void **)d_halo);
}

int nw_halo_free(uint64_t *d_halo) {
    if (!d_halo) return NW_ERR_ARG;
    NW_HIP_TRY(hipFree(d_halo));
    return NW_OK;
}

int nw_link_alloc(int device, uint32_t **d_word) {
    if (!d_word) return NW_ERR_ARG;
    *d_word = nullptr;
    return alloc_zeroed_link(device, 256, (void **)d_word);
}

int nw_link_wait_async(uint32_t *d_word, uint32_t value, int32_t timeout_ms, void *stream) {
    return nw_link_wait_ctx_async(nullptr, d_word, value, timeout_ms, stream);
}

int nw_link_wait_ctx_async(nw_ctx *c, uint32_t *d_word, uint32_t value, int32_t timeout_ms, void *stream) {
    if (!d_word || timeout_ms < 0) return NW_ERR_ARG;
    return nw::launch_link_wait(d_word, value, timeout_ticks(timeout_ms), c ? c->ctrl : nullptr, stream) == hipSuccess
               ? NW_OK
               : NW_ERR_HIP;
}

int nw_link_signal_async(uint32_t *d_word, uint32_t value, void *stream) {
    if (!d_word) return NW_ERR_ARG;
    return nw::launch_link_signal(d_word, value, stream) == hipSuccess ? NW_OK : NW_ERR_HIP;
}

int nw_link_status(const uint32_t *d_word, uint32_t *out) {
    if (!d_word || !out) return NW_ERR_ARG;
    NW_HIP_TRY(hipMemcpy(out, d_word + 1, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return NW_OK;
}

int nw_ipc_get_handle(const void *d_ptr, void *handle) {
    if (!d_ptr || !handle) return NW_ERR_ARG;
    if (link_coarse()) return NW_ERR_UNSUPPORTED;  // (a peer would see stale data)
    hipIpcMemHandle_t h;
    NW_HIP_TRY(hipIpcGetMemHandle(&h, const_cast<void *>(d_ptr)));
    std::memcpy(handle, &h, sizeof h < NW_IPC_HANDLE_BYTES ? sizeof h : NW_IPC_HANDLE_BYTES);
    return NW_OK;
}

int nw_ipc_open_handle(const void *handle, void **d_ptr) {
    if (!handle || !d_ptr) return NW_ERR_ARG;
    hipIpcMemHandle_t h;
    std::memset(&h, 0, sizeof h);
    std::memcpy(&h, handle, sizeof h < NW_IPC_HANDLE_BYTES ? sizeof h : NW_IPC_HANDLE_BYTES);
    NW_HIP_TRY(hipIpcOpenMemHandle(d_ptr, h, hipIpcMemLazyEnablePeerAccess));
    return NW_OK;
}

int nw_ipc_close_handle(void *d_ptr) {
    if (!d_ptr) return NW_ERR_ARG;
    NW_HIP_TRY(hipIpcCloseMemHandle(d_ptr));
    return NW_OK;
}

}  // extern "C"
