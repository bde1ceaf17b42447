// capi.hip — the C ABI declared in include/pq_gpu.h: devices, contexts and
// their options, device buffers and timers.  Uploads are in capi_upload.hip,
// decodes in capi_decode.hip, the regex page filter in capi_regex.hip and the
// pq_file_* functions in host/capi_file.cpp.
#include "host/capi_util.hpp"

using namespace pqcapi;

extern "C" {

int pq_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int pq_plan_page_ranges(const pq_page_desc* table, int64_t ntable, int world, int64_t* ranges) {
    if ((!table && ntable) || ntable < 0 || world <= 0 || !ranges) return PQ_ERR_ARG;
    // cumulative payload bytes of the data pages (shard.py page_ranges)
    std::vector<int64_t> cum;
    cum.reserve(static_cast<size_t>(ntable));
    int64_t acc = 0;
    for (int64_t i = 0; i < ntable; i++) {
        if (table[i].page_type != PQ_DATA_PAGE) continue;
        acc += std::max<int64_t>(table[i].payload_size, 0);
        cum.push_back(acc);
    }
    const int64_t n = static_cast<int64_t>(cum.size());
    int64_t prev = 0;
    for (int k = 0; k < world; k++) {
        int64_t cut = n;
        if (k + 1 < world) {
            if (n == 0) {
                cut = 0;
            } else {
                // first page whose running total reaches (k + 1) / world of the sum, plus one
                // (the float64 quotient of the exact product, as shard.py computes it)
                const double target = static_cast<double>(acc * (k + 1)) / world;
                const int64_t c = static_cast<int64_t>(
                    std::lower_bound(cum.begin(), cum.end(), target,
                                     [](int64_t v, double t) { return static_cast<double>(v) < t; }) -
                    cum.begin()) + 1;
                cut = std::min(std::max(c, prev), n);
            }
        }
        ranges[2 * k] = prev;
        ranges[2 * k + 1] = cut;
        prev = cut;
    }
    return 0;
}

pq_ctx* pq_ctx_create(int device) {
    try {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= device || device < 0) return nullptr;
        DevGuard dg(device);  // the caller's current device comes back on return
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess || cur != device) return nullptr;
        auto* c = new pq_ctx();
        c->device = device;
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
            c->cus = cus;
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
            hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess ||
            hipStreamCreateWithFlags(&c->copy, hipStreamNonBlocking) != hipSuccess ||
            hipStreamCreateWithFlags(&c->copy2, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) {
            if (c->side) (void)hipStreamDestroy(c->side);
            if (c->copy) (void)hipStreamDestroy(c->copy);
            if (c->copy2) (void)hipStreamDestroy(c->copy2);
            if (c->stream) (void)hipStreamDestroy(c->stream);
            delete c;
            return nullptr;
        }
        return c;
    } catch (...) {
        return nullptr;
    }
}

void pq_ctx_destroy(pq_ctx* ctx) {
    if (!ctx) return;
    {
    DevGuard dg(ctx);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& p : ctx->pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto& p : ctx->free_events) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    if (ctx->d_prof) (void)hipFree(ctx->d_prof);
    (void)hipStreamSynchronize(ctx->side);
    (void)hipEventDestroy(ctx->ev_fork);
    (void)hipEventDestroy(ctx->ev_join);
    (void)hipStreamDestroy(ctx->side);
    ctx->stager.release();
    if (ctx->d_raw) (void)hipFree(ctx->d_raw);
    if (ctx->d_walk) (void)hipFree(ctx->d_walk);
    if (ctx->h_walk) (void)hipHostFree(ctx->h_walk);
    if (ctx->d_relay) (void)hipFree(ctx->d_relay);
    if (ctx->d_codec) (void)hipFree(ctx->d_codec);
    if (ctx->d_codec_st) (void)hipFree(ctx->d_codec_st);
    if (ctx->d_zsrc) (void)hipFree(ctx->d_zsrc);
    if (ctx->d_chunker) (void)hipFree(ctx->d_chunker);
    (void)hipStreamSynchronize(ctx->copy);
    (void)hipStreamDestroy(ctx->copy);
    (void)hipStreamSynchronize(ctx->copy2);
    (void)hipStreamDestroy(ctx->copy2);
    (void)hipStreamDestroy(ctx->stream);
    }
    delete ctx;
}

int pq_ctx_set_option(pq_ctx* ctx, const char* key, int64_t value) {
    if (!ctx || !key) return PQ_ERR_ARG;
    DevGuard dg(ctx);
    auto ranged = [&](int* opt, int64_t lo, int64_t hi, const char* range) {  // an integer option within its range
        if (value < lo || value > hi) return set_err(ctx, PQ_ERR_ARG, range);
        *opt = static_cast<int>(value);
        return 0;
    };
    if (std::strcmp(key, "fused_ba") == 0) { ctx->opt_fused = value != 0; return 0; }
    if (std::strcmp(key, "wide_rows") == 0) { ctx->opt_wide_rows = value != 0; return 0; }
    if (std::strcmp(key, "pipe_wide") == 0) { ctx->opt_pipe_wide = value != 0; return 0; }
    if (std::strcmp(key, "levels_small") == 0) { ctx->opt_levels_small = value != 0; return 0; }
    if (std::strcmp(key, "gather_rows") == 0) { ctx->opt_gather_rows = value != 0; return 0; }
    if (std::strcmp(key, "fused_debug") == 0) { ctx->opt_debug = static_cast<int>(value); return 0; }
    if (std::strcmp(key, "fused_waves") == 0) { ctx->opt_waves = static_cast<int>(value); return 0; }
    if (std::strcmp(key, "fused_claim") == 0) return ranged(&ctx->opt_claim, 1, 64, "fused_claim: 1..64");
    if (std::strcmp(key, "regex_dfa") == 0) { ctx->opt_regex_dfa = value != 0; return 0; }
    if (std::strcmp(key, "regex_debug") == 0) { ctx->opt_regex_debug = static_cast<int>(value); return 0; }
    if (std::strcmp(key, "regex_plain") == 0) { ctx->opt_regex_plain = value != 0; return 0; }
    if (std::strcmp(key, "regex_codes") == 0) { ctx->opt_regex_codes = value != 0; return 0; }
    if (std::strcmp(key, "regex_reuse") == 0) { ctx->opt_regex_reuse = value != 0; return 0; }
    if (std::strcmp(key, "regex_index") == 0) return ranged(&ctx->opt_regex_index, 0, 2, "regex_index: 0, 1 or 2");
    if (std::strcmp(key, "zflip") == 0) { ctx->opt_zflip = value != 0; return 0; }
    if (std::strcmp(key, "write_waves") == 0) return ranged(&ctx->opt_write_waves, 1, 16, "write_waves: 1..16");
    if (std::strcmp(key, "big_all") == 0) { ctx->opt_big_all = value != 0; return 0; }
    if (std::strcmp(key, "fixed_plain") == 0) { ctx->opt_fixed_plain = value != 0; return 0; }
    if (std::strcmp(key, "fixed_fused") == 0) { ctx->opt_fixed_fused = value != 0; return 0; }
    if (std::strcmp(key, "dict_pipe") == 0) { ctx->opt_pipe = value != 0; return 0; }
    if (std::strcmp(key, "plain_ba") == 0) { ctx->opt_plain = value != 0; return 0; }
    if (std::strcmp(key, "plain_fused") == 0) { ctx->opt_plain_fused = value != 0; return 0; }
    if (std::strcmp(key, "pipe_run_dict") == 0) { ctx->opt_run_dict = value != 0; return 0; }
    if (std::strcmp(key, "write_bpc") == 0) return ranged(&ctx->opt_write_bpc, 0, 4, "write_bpc: 0..4");
    if (std::strcmp(key, "pipe_run_pages") == 0) return ranged(&ctx->opt_run_pages, 0, 32, "pipe_run_pages: 0 (auto) .. 32");
    if (std::strcmp(key, "stage_bufs") == 0) {
        if (value < 2 || value > pqstage::kMaxBufs) return set_err(ctx, PQ_ERR_ARG, "stage_bufs: 2..16");
        ctx->stager.configure(static_cast<int>(value), ctx->stager.piece());
        ctx->opt_stage_bufs = static_cast<int>(value);
        return 0;
    }
    if (std::strcmp(key, "raw_upload") == 0) { ctx->opt_raw = value != 0; return 0; }
    if (std::strcmp(key, "device_walk") == 0) { ctx->opt_dev_walk = value != 0; return 0; }
    if (std::strcmp(key, "stage_streams") == 0) return ranged(&ctx->opt_stage_streams, 1, 2, "stage_streams: 1..2");
    if (std::strcmp(key, "stage_piece_kb") == 0) {
        if (value < 64 || value > 65536) return set_err(ctx, PQ_ERR_ARG, "stage_piece_kb: 64..65536");
        ctx->stager.configure(ctx->opt_stage_bufs, static_cast<size_t>(value) << 10);
        return 0;
    }
    if (std::strcmp(key, "regex_win") == 0) {
        if (value < 1024 || value > 32768 || value % 16) return set_err(ctx, PQ_ERR_ARG, "regex_win: 1024..32768, multiple of 16");
        ctx->opt_regex_win = static_cast<int>(value);
        return 0;
    }
    if (std::strcmp(key, "fused_prof") == 0) {
        if (value && !ctx->d_prof) {
            if (hipMalloc(reinterpret_cast<void**>(&ctx->d_prof), 64 * sizeof(uint64_t)) != hipSuccess)
                return set_err(ctx, PQ_ERR_HIP, "hipMalloc failed (prof)");
            (void)hipMemset(ctx->d_prof, 0, 64 * sizeof(uint64_t));
        } else if (!value && ctx->d_prof) {
            (void)hipFree(ctx->d_prof);
            ctx->d_prof = nullptr;
        }
        return 0;
    }
    return set_err(ctx, PQ_ERR_ARG, std::string("unknown option ") + key);
}

const char* pq_last_error(const pq_ctx* ctx) { return ctx ? ctx->err.c_str() : "no context"; }
void* pq_ctx_stream(pq_ctx* ctx) { return ctx ? static_cast<void*>(ctx->stream) : nullptr; }
int pq_ctx_sync(pq_ctx* ctx) {
    if (!ctx) return PQ_ERR_ARG;
    DevGuard dg(ctx);
    return hip_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
}

int pq_device_buffer(pq_ctx* ctx, const uint8_t* host, size_t n, void** d_out) {
    if (!ctx || !d_out || (!host && n)) return PQ_ERR_ARG;
    DevGuard dg(ctx);
    uint8_t* d = nullptr;
    if (int rc = hip_check(ctx, hipMalloc(reinterpret_cast<void**>(&d), n + 64), "hipMalloc (device buffer)")) return rc;
    int rc = hip_check(ctx, hipMemset(d + n, 0, 64), "device buffer pad");
    if (!rc && n) rc = hip_check(ctx, hipMemcpy(d, host, n, hipMemcpyHostToDevice), "device buffer copy");
    if (rc) {
        (void)hipFree(d);
        return rc;
    }
    *d_out = d;
    return 0;
}

void pq_device_buffer_free(pq_ctx* ctx, void* d) {
    if (!ctx || !d) return;
    DevGuard dg(ctx);
    (void)hipFree(d);
}

void pq_timing_enable(pq_ctx* ctx, int enable) { if (ctx) ctx->timing = enable != 0; }
void pq_timing_reset(pq_ctx* ctx) {
    if (!ctx) return;
    DevGuard dg(ctx);
    resolve_timers(ctx);
    ctx->timers.clear();
}
int pq_timing_get(pq_ctx* ctx, const char* name, double* total_ms, int64_t* launches) {
    if (!ctx || !name) return 0;
    DevGuard dg(ctx);
    resolve_timers(ctx);
    auto it = ctx->timers.find(name);
    if (it == ctx->timers.end()) return 0;
    if (total_ms) *total_ms = it->second.first;
    if (launches) *launches = it->second.second;
    return 1;
}

int pq_fused_prof_read(pq_ctx* ctx, uint64_t* out, int n) {
    if (!ctx || !ctx->d_prof) return 0;
    DevGuard dg(ctx);
    const int k = pqk::fused_prof_slots();
    std::vector<uint64_t> h(static_cast<size_t>(k));
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return 0;
    if (hipMemcpy(h.data(), ctx->d_prof, k * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    (void)hipMemset(ctx->d_prof, 0, k * sizeof(uint64_t));
    for (int i = 0; i < std::min(n, k); i++) out[i] = h[static_cast<size_t>(i)];
    return k;
}

}  // extern "C"
