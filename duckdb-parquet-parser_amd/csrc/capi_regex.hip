// capi_regex.hip — the regex page filter of the C ABI (include/pq_gpu.h):
// pattern compile and upload, the scan launches (regex/regex.hip) and the
// decode that filters in the same pass.
#include "host/capi_util.hpp"

using namespace pqcapi;

// The compiled pattern (cached per chunk), page flags and the per-entry
// match buffer of a BYTE_ARRAY chunk.
static int regex_prepare(pq_ctx* ctx, pq_chunk* c, const char* pattern) {
    if (c->type != PQ_BYTE_ARRAY) return set_err(ctx, PQ_ERR_ARG, "regex page filter needs a BYTE_ARRAY column");
    try {
        std::string msg;
        pqre::Program prog;
        int rc = pqre::compile(pattern, &prog, &msg);
        if (rc) return set_err(ctx, PQ_ERR_REGEX, msg);
        if (!c->d_page_flags && dalloc(&c->d_page_flags, static_cast<size_t>(c->npages)))
            return set_err(ctx, PQ_ERR_HIP, "hipMalloc failed (page flags)");
        int64_t dict_cap = std::max<int64_t>(c->nentries, 1);
        if (c->dict_match_cap < dict_cap) {
            dfree(c->d_dict_match);
            if (dalloc(&c->d_dict_match, static_cast<size_t>(dict_cap)))
                return set_err(ctx, PQ_ERR_HIP, "hipMalloc failed (dict match)");
            c->dict_match_cap = dict_cap;
        }
        // compiled programs are cached per chunk by pattern (the bench and the
        // CLI rescan with one pattern)
        const std::string key = std::string(pattern) + (ctx->opt_regex_dfa ? "|dfa" : "|nfa");
        if (!c->d_prog || c->prog_pattern != key) {
            if (c->d_prog) pqre::free_device_program(c->d_prog);
            c->d_prog = pqre::upload_program(prog, ctx->stream);
            if (!c->d_prog) return set_err(ctx, PQ_ERR_HIP, "regex program upload failed");
            std::vector<uint8_t> img;
            dfree(c->d_dfa);
            c->dfa_bytes = 0;
            c->dfa_sink = false;
            if (ctx->opt_regex_dfa && pqre::build_dfa(prog, &img)) {
                if (dalloc(&c->d_dfa, img.size())) return set_err(ctx, PQ_ERR_HIP, "hipMalloc failed (dfa)");
                if (int rc2 = hip_check(ctx, hipMemcpy(c->d_dfa, img.data(), img.size(), hipMemcpyHostToDevice), "dfa upload"))
                    return rc2;
                c->dfa_bytes = static_cast<uint32_t>(img.size());
                c->dfa_full = reinterpret_cast<const pqre::DevDfa*>(img.data())->full != 0;
                c->dfa_sink = c->dfa_full && reinterpret_cast<const pqre::DevDfa*>(img.data())->anchored != 0;
            }
            c->prog_pattern = key;
        }
        return 0;
    } catch (const std::exception& e) {
        return set_err(ctx, PQ_ERR_ALLOC, e.what());
    }
}

extern "C" {

int pq_regex_compile_check(const char* pattern, char* err, size_t errlen) {
    std::string msg;
    int rc = pqre::check(pattern ? pattern : "", &msg);
    if (err && errlen) {
        std::strncpy(err, msg.c_str(), errlen - 1);
        err[errlen - 1] = 0;
    }
    return rc;
}

int pq_regex_pages_async(pq_ctx* ctx, pq_chunk* c, const char* pattern, int neg) {
    if (!ctx || !c || !pattern) return PQ_ERR_ARG;
    DevGuard dg(ctx);
    if (int rc = regex_prepare(ctx, c, pattern)) return rc;
    try {
        hipStream_t s = ctx->stream;
        pqk::ColumnParams cp{c->type, c->max_def, c->max_rep, c->width, c->plain_width};
        const bool on_codes = c->pipe && (!c->pipe_wide || pqk::pipe_match_wide_ok(c->pipe_ecap)) && ctx->opt_pipe &&
                              ctx->opt_regex_codes;
        const bool reuse = on_codes && ctx->opt_regex_reuse && c->codes_ok;
        // over a checked decode's codes: k_regex_dict clears the status words
        // and sets the page flags itself (no fill kernels)
        const bool fold = reuse && c->ndicts && c->entries_ok && c->zero_bytes % 4 == 0;
        if (!fold) (void)hipMemsetAsync(c->d_flags, 0, c->zero_bytes, s);
        if (c->ndicts) {
            if (!(ctx->opt_regex_reuse && c->entries_ok)) {
                c->entries_pending = true;
                Timed t(ctx, "dict_index");
                launch_dicts(c, s, c->d_flags);
            }
            Timed t(ctx, "regex_dict");
            pqre::launch_regex_dict(s, c->d_prog, c->d_bytes, c->d_dicts, c->ndicts, c->d_entries,
                                    c->d_dict_count, c->d_dict_match, fold ? c->d_page_flags : nullptr,
                                    fold ? c->npages : 0, fold ? reinterpret_cast<uint32_t*>(c->d_flags) : nullptr,
                                    fold ? static_cast<int64_t>(c->zero_bytes / 4) : 0);
        }
        if (on_codes) {
            // dictionary-first on the decode's own codes: the pattern ran on
            // every entry above; the pipe passes give each row its index
            // (or a checked earlier decode already did)
            const pqk::PipeLaunch P = pipe_launch(ctx, c, nullptr);
            if (!reuse) {
                pipe_front(ctx, c, P, false, false);
                c->codes_pending = true;
            }
            Timed t(ctx, "regex_codes");
            pqk::launch_pipe_match(s, P, c->d_dict_match + c->pipe_entry_base, neg, c->d_page_flags, fold);
        } else if (c->d_dfa && ctx->opt_regex_plain && c->ndicts == 0 && pqre::regex_plain_lds_ok() &&
                   plan_regex_windows(ctx, c)) {
            // REQUIRED chunks: the first error-free scan files every string's
            // window offset (row-indexed); later scans read it instead of
            // walking the length chains (same windows: same window size)
            const uint16_t* idx_in = nullptr;
            uint16_t* idx_out = nullptr;
            if (ctx->opt_regex_index && c->max_def == 0 && c->max_rep == 0 && c->nrows > 0 && !ctx->opt_regex_debug) {
                if (c->rx_index_ok && c->rx_index_win == c->rwin_bytes && ctx->opt_regex_index != 2) {
                    idx_in = c->d_rx_index;
                } else {
                    c->rx_index_ok = false;
                    if (c->d_rx_index || !dalloc(&c->d_rx_index, static_cast<size_t>(c->nrows))) {
                        idx_out = c->d_rx_index;
                        c->rx_index_pending = true;
                        c->rx_index_win = c->rwin_bytes;
                    }
                }
            }
            Timed t(ctx, "regex_plain");
            pqre::launch_regex_plain(s, c->d_dfa, c->dfa_bytes, c->rwin_bytes, c->d_bytes, c->d_pages, c->d_rwins,
                                     static_cast<int>(c->hrwins.size()), c->d_rwin_ticket, c->rwin_grid, cp,
                                     (neg ? 1 : 0) | ((ctx->opt_regex_debug & 0xFF) << 8),
                                     c->d_page_flags, c->d_page_err, c->d_flags, idx_in, idx_out, c->dfa_sink);
        } else if (c->d_dfa) {
            Timed t(ctx, "regex_lanes");
            pqre::launch_regex_lanes(s, c->d_dfa, c->dfa_bytes, c->d_bytes, c->d_pages, c->npages, c->d_dicts,
                                     c->d_dict_count, c->d_dict_match, cp, neg, c->d_page_flags,
                                     c->d_page_err, c->d_flags);
        } else {
            Timed t(ctx, "regex_pages");
            pqre::launch_regex_pages(s, c->d_prog, c->d_bytes, c->d_pages, c->npages, c->d_dicts,
                                     c->d_entries, c->d_dict_count, c->d_dict_match, cp, neg,
                                     c->d_page_flags, c->d_page_err, c->d_flags);
        }
        return hip_check(ctx, hipGetLastError(), "regex launch");
    } catch (const std::exception& e) {
        return set_err(ctx, PQ_ERR_ALLOC, e.what());
    }
}

int pq_regex_pages_result(pq_ctx* ctx, pq_chunk* c, uint8_t* page_flags) {
    if (!ctx || !c) return PQ_ERR_ARG;
    DevGuard dg(ctx);
    if (int rc = collect(ctx, c, nullptr)) return rc;
    if (page_flags && c->npages)
        return hip_check(ctx, hipMemcpy(page_flags, c->d_page_flags, static_cast<size_t>(c->npages), hipMemcpyDeviceToHost), "copy page flags");
    return 0;
}

int pq_decode_regex_async(pq_ctx* ctx, pq_chunk* c, pq_column* out, const char* pattern, int neg) {
    if (!ctx || !c || !out || !pattern) return PQ_ERR_ARG;
    DevGuard dg(ctx);
    if (int rc = regex_prepare(ctx, c, pattern)) return rc;
    // one pass when the decode takes the pipe (dictionary pages only, one
    // dictionary of < 32 KiB: the writer keeps each entry's match bit beside
    // its length); else the decode, then the scan over its codes
    const bool plain_go = c->plain && ctx->opt_plain;
    const bool one = c->pipe && !c->pipe_wide && ctx->opt_pipe && ctx->opt_regex_codes && !plain_go && c->ndicts > 0 &&
                     c->pipe_dict_payload < pqk::kArmDictBytes;
    if (!one) {
        // the scan clears d_flags, which still holds this decode's status
        // (err_any, char overflow, the PLAIN redo flags): check the decode
        // first, so its redo / growth / error runs before the scan starts
        if (int rc = pq_decode_async(ctx, c, out)) return rc;
        if (int rc = collect(ctx, c, out)) return rc;
        return pq_regex_pages_async(ctx, c, pattern, neg);
    }
    c->arm = true;
    c->arm_neg = neg ? 1 : 0;
    const int rc = pq_decode_async(ctx, c, out);
    c->arm = false;
    return rc;
}

int pq_regex_pages(pq_ctx* ctx, pq_chunk* c, const char* pattern, int neg, uint8_t* page_flags) {
    DevGuard dg(ctx);
    if (int rc = pq_regex_pages_async(ctx, c, pattern, neg)) return rc;
    return pq_regex_pages_result(ctx, c, page_flags);
}

}  // extern "C"
