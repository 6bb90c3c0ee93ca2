// nw_hostcopy.h -- the parts of nw_fill's copy-back (nw_hostpath.cpp) that need no
// device: how a table is cut into staging chunks, how many threads move a chunk,
// and the threaded memcpy itself.  No HIP here, so that a plain C++ program can
// include the file and run it under the host sanitizers (tests/test_sanitizers.py);
// tests/nw_hostcopy.py restates the arithmetic in Python.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#pragma GCC visibility push(hidden)
namespace nwh {

constexpr int kStages = 3;
// staging chunk: up to 256 MiB (a third of the table, at least 16 MiB), pinned
// with hipHostMallocCoherent (tools/d2h_bench.cpp on the box: 40 GB through 3 x
// 256 MiB coherent chunks and 8 copy threads at 56.6 GB/s, the bare pinned
// hipMemcpy2D's 56.4; 128 MiB default-flag chunks 45-53)
constexpr size_t kStageMax = 256u << 20, kStageMin = 16u << 20;
constexpr size_t kParMin = 8u << 20;  // a smaller copy is one memcpy
constexpr int kCopyThreadsMax = 64;

// Thread t copies [t * per, t * per + min(per, bytes - t * per)), per = the ceiling
// of bytes / threads rounded up to 4096: threads * per >= bytes for every
// (bytes, threads), the spans are disjoint and the last one ends at `bytes`.
inline size_t par_span(size_t bytes, int threads) {
    const size_t n = (size_t)threads;
    return ((bytes + n - 1) / n + 4095) & ~(size_t)4095;
}

inline void par_memcpy(char *dst, const char *src, size_t bytes, int threads) {
    if (threads <= 1 || bytes < kParMin) {
        std::memcpy(dst, src, bytes);
        return;
    }
    std::vector<std::thread> ts;
    const size_t per = par_span(bytes, threads);
    for (int t = 1; t < threads; ++t) {
        const size_t o = (size_t)t * per;
        if (o >= bytes) break;
        ts.emplace_back([=] { std::memcpy(dst + o, src + o, std::min(per, bytes - o)); });
    }
    std::memcpy(dst, src, std::min(per, bytes));
    for (auto &t : ts) t.join();
}

// The copy threads: NW_COPY_THREADS (`env`, nullptr when unset) clamped to
// 1..kCopyThreadsMax -- 0, a negative or a non-numeric value is 1 -- else
// min(8, cores).
inline int copy_threads_of(const char *env, unsigned cores) {
    if (env) return (int)std::min<long>(kCopyThreadsMax, std::max<long>(1, std::strtol(env, nullptr, 10)));
    return (int)std::min<unsigned>(8u, std::max(1u, cores));
}

// How a table of `rows` rows of `row_bytes` comes back through the staging ring.
struct CopyPlan {
    size_t stage_cap;  // bytes per staging chunk once the ring has grown for this table
    int64_t rpc;       // rows per chunk
    int64_t nch;       // chunks
    bool direct;       // one row is wider than a chunk: no staging, one hipMemcpy2D
    int64_t first_row(int64_t ch) const { return ch * rpc; }
    int64_t rows_of(int64_t ch, int64_t rows) const { return std::min(rpc, rows - ch * rpc); }
};

// the chunk a table asks for: a third of it in whole 2 MiB, within [kStageMin, kStageMax]
inline size_t stage_want(size_t table_bytes) {
    return std::min(kStageMax, std::max(kStageMin, (table_bytes / kStages + (2u << 20) - 1) & ~((size_t)(2u << 20) - 1)));
}

// stage_cap: what the ring holds now (0: nothing yet); it only grows
inline CopyPlan copy_plan(size_t table_bytes, size_t row_bytes, int64_t rows, size_t stage_cap) {
    CopyPlan p;
    p.stage_cap = std::max(stage_cap, stage_want(table_bytes));
    p.rpc = std::max<int64_t>(1, (int64_t)(p.stage_cap / row_bytes));
    p.direct = (size_t)p.rpc * row_bytes > p.stage_cap;
    p.nch = (rows + p.rpc - 1) / p.rpc;
    return p;
}

}  // namespace nwh
#pragma GCC visibility pop
