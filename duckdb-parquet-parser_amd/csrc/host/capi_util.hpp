// capi_util.hpp — helpers shared by the C ABI's translation units (capi.hip,
// capi_upload.hip, capi_decode.hip, capi_regex.hip): error plumbing, the
// device guard, the timers, and the few functions one file defines for another.
#pragma once

#include "host/capi_state.hpp"

namespace pqcapi __attribute__((visibility("hidden"))) {

// Host threads of an upload or copy-out: the box's CPU share for one GPU.
inline int host_threads() { return static_cast<int>(std::min(16u, std::max(1u, std::thread::hardware_concurrency()))); }

// fn(0 .. n-1) on up to hardware_concurrency host threads (inline when n == 1).
template <class Fn>
void parallel_for(int n, Fn&& fn) {
    if (n <= 1) {
        if (n == 1) fn(0);
        return;
    }
    const int nt = std::max(1, std::min<int>(n, static_cast<int>(std::thread::hardware_concurrency())));
    std::atomic<int> next{0};
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++)
        th.emplace_back([&]() {
            for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) fn(i);
        });
    for (auto& x : th) x.join();
}

inline int set_err(pq_ctx* ctx, int code, const std::string& m) {
    if (ctx) ctx->err = m;
    return code;
}

inline int hip_check(pq_ctx* ctx, hipError_t e, const char* what) {
    if (e == hipSuccess) return 0;
    return set_err(ctx, PQ_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// Every entry point that touches the GPU runs on its context's device: a host
// thread may drive contexts on several devices, and HIP's
// current device is per thread.  Restores the caller's device on return.
struct DevGuard {
    int prev = -1;
    explicit DevGuard(const pq_ctx* c) : DevGuard(c ? c->device : -1) {}
    explicit DevGuard(int device) {
        int cur = 0;
        if (device >= 0 && hipGetDevice(&cur) == hipSuccess && cur != device && hipSetDevice(device) == hipSuccess) prev = cur;
    }
    ~DevGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

inline int plain_width_of(int32_t type) {
    switch (type) {
        case PQ_BOOLEAN: return 1;
        case PQ_INT32: case PQ_FLOAT: return 4;
        case PQ_INT64: case PQ_DOUBLE: return 8;
        case PQ_INT96: return 12;
        default: return 0;
    }
}

// Launch bracket for per-kernel HIP-event timing on the context stream.
struct Timed {
    pq_ctx* ctx;
    PendingTimer t{};
    bool on;
    hipStream_t st;
    Timed(pq_ctx* c, const char* name, hipStream_t s = nullptr) : ctx(c), on(c->timing), st(s ? s : c->stream) {
        if (!on) return;
        t.name = name;
        if (!ctx->free_events.empty()) {
            t.a = ctx->free_events.back().first;
            t.b = ctx->free_events.back().second;
            ctx->free_events.pop_back();
        } else {
            (void)hipEventCreate(&t.a);
            (void)hipEventCreate(&t.b);
        }
        (void)hipEventRecord(t.a, st);
    }
    ~Timed() {
        if (!on) return;
        (void)hipEventRecord(t.b, st);
        ctx->pending.push_back(t);
    }
};

// Host-side phase timer (wall ms) filed under `name` in the same table as the
// kernel timers while timing is on (upload phases: up_walk, up_plan,
// up_alloc, up_h2d).
struct HostTimed {
    pq_ctx* ctx;
    const char* name;
    std::chrono::steady_clock::time_point t0;
    HostTimed(pq_ctx* c, const char* n) : ctx(c), name(n), t0(std::chrono::steady_clock::now()) {}
    ~HostTimed() {
        if (!ctx->timing) return;
        auto& e = ctx->timers[name];
        e.first += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        e.second += 1;
    }
};

inline void resolve_timers(pq_ctx* ctx) {
    if (ctx->pending.empty()) return;
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& p : ctx->pending) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, p.a, p.b);
        auto& e = ctx->timers[p.name];
        e.first += ms;
        e.second += 1;
        ctx->free_events.push_back({p.a, p.b});
    }
    ctx->pending.clear();
}

inline std::string format_error(const DevErr& e) {
    switch (e.code) {
        case PQ_ERR_BUFFER:
            return "ByteBuffer: read beyond end (pos=" + std::to_string(static_cast<uint32_t>(e.pos)) +
                   " need=" + std::to_string(static_cast<uint32_t>(e.need)) +
                   " size=" + std::to_string(static_cast<uint32_t>(e.size)) + ")";
        case PQ_ERR_FLBA: return "FIXED_LEN_BYTE_ARRAY not supported without type_length";
        case PQ_ERR_UNSUPPORTED: return "page encoding outside the supported parity scope";
        default: return "decode error " + std::to_string(e.code);
    }
}

// capi_upload.hip
void free_chunk_device(pq_chunk* c);

// capi_decode.hip (capi_regex.hip scans over the decode's launches)
pqk::PipeLaunch pipe_launch(pq_ctx* ctx, pq_chunk* c, pq_column* out);
void launch_dicts(pq_chunk* c, hipStream_t s, int32_t* err_any);
void pipe_front(pq_ctx* ctx, pq_chunk* c, const pqk::PipeLaunch& P, bool dict_on_side, bool dict_in_runs);
int collect(pq_ctx* ctx, pq_chunk* c, pq_column* out);

}  // namespace pqcapi
