// capi_decode.hip — the decode side of the C ABI (include/pq_gpu.h): output
// buffers, one launcher per decode path, the path choice (decode_launch), the
// error collection and re-runs (collect), copy-out and the chunker.  A decode
// is a short, allocation-free sequence of launches on the context's stream.
#include <cstdio>
#include <cstdlib>

#include "host/capi_util.hpp"

namespace pqcapi __attribute__((visibility("hidden"))) {

static int ensure_output(pq_ctx* ctx, pq_chunk* c, pq_column* out, int64_t char_cap) {
    int64_t rows_needed = c->nrows;
    int64_t bytes_needed = c->type == PQ_BYTE_ARRAY ? char_cap : c->nrows * c->width;
    if (out->capacity_rows < rows_needed + 1 || out->d_validity == nullptr) {
        dfree(out->d_validity);
        dfree(out->d_offsets);
        int64_t cap = rows_needed + 1;
        if (dalloc(&out->d_validity, static_cast<size_t>(cap / 32 + 4)))
            return set_err(ctx, PQ_ERR_HIP, "hipMalloc failed (validity)");
        if (c->type == PQ_BYTE_ARRAY && dalloc(&out->d_offsets, static_cast<size_t>(cap)))
            return set_err(ctx, PQ_ERR_HIP, "hipMalloc failed (offsets)");
        out->capacity_rows = cap;
    }
    if (c->type == PQ_BYTE_ARRAY && out->d_offsets == nullptr) {
        if (dalloc(&out->d_offsets, static_cast<size_t>(out->capacity_rows)))
            return set_err(ctx, PQ_ERR_HIP, "hipMalloc failed (offsets)");
    }
    if (out->capacity_bytes < bytes_needed || out->d_values == nullptr) {
        dfree(out->d_values);
        if (dalloc(&out->d_values, static_cast<size_t>(bytes_needed + 64)))
            return set_err(ctx, PQ_ERR_HIP, "hipMalloc failed (values)");
        out->capacity_bytes = bytes_needed;
    }
    out->num_rows = c->nrows;
    out->type = c->type;
    out->value_width = c->type == PQ_BYTE_ARRAY ? 0 : c->width;
    return 0;
}

// Launch parameters of the three-pass dictionary path (dict_pipe.hip); `out`
// may be null when only the codes are wanted (regex page filter).
pqk::PipeLaunch pipe_launch(pq_ctx* ctx, pq_chunk* c, pq_column* out) {
    pqk::PipeLaunch P{};
    P.bytes = c->d_bytes; P.pages = c->d_pages; P.npages = c->npages; P.tiles = c->d_tiles;
    P.ntiles = c->ntiles; P.page_tile0 = c->d_page_tile0; P.max_def = c->max_def; P.max_rep = c->max_rep;
    P.dicts = c->d_dicts; P.dict_id = c->pipe_dict; P.entries = c->d_entries; P.dict_count = c->d_dict_count;
    P.runs = c->d_runs; P.info = c->d_info; P.flist = c->d_flist; P.tile_nn = c->d_tile_nn; P.codes = c->d_codes;
    if (c->pipe_wide) {
        P.codes32 = reinterpret_cast<uint32_t*>(c->d_codes);
        P.codes = nullptr;
        for (const auto& b : c->hbigd)
            if (b.di == c->pipe_dict) {
                P.lens8 = c->d_bigd + b.lens_off;
                P.lens8_cap = static_cast<uint32_t>(dict_entry_cap(std::max(b.d.nvals, 0), b.d.size));
                P.pad16 = reinterpret_cast<const uint4*>(c->d_bigd + b.pad_off);
            }
    }
    P.tile_chars = c->d_tile_chars; P.bsum = c->d_bsum; P.total = c->d_total;
    P.nrows_total = c->nrows; P.overflow = c->d_flags + 1;
    if (out) {
        P.capacity = out->capacity_bytes;
        P.validity = out->d_validity; P.offsets = out->d_offsets; P.chars = out->d_values;
    }
    P.page_err = c->d_page_err; P.err_any = c->d_flags;
    P.dict_chars_bytes = c->pipe_dict_chars_bytes; P.dict_bytes = c->pipe_dict_bytes; P.lds = c->pipe_lds;
    P.grid = c->pipe_grid; P.debug = ctx->opt_debug; P.dict_entries_cap = c->pipe_ecap;
    P.cus = c->pipe_cus; P.has_small = c->pipe_small; P.write_waves = c->pipe_wpw;
    return P;
}

// k_dict_index for every dictionary page of a BYTE_ARRAY chunk, and the
// multi-workgroup index for pages too large for its LDS.
void launch_dicts(pq_chunk* c, hipStream_t s, int32_t* err_any) {
    if (c->hbigd.size() < static_cast<size_t>(c->ndicts))  // k_dict_index leaves the large pages alone
        pqk::launch_dict_index(s, c->d_bytes, c->d_dicts, c->ndicts, c->d_entries, c->d_dict_count, c->d_dict_err, err_any,
                           c->max_dict_bytes);
    for (const auto& b : c->hbigd)
        pqk::launch_dict_big(s, c->d_bytes + b.d.off, static_cast<uint32_t>(b.d.size), static_cast<uint32_t>(std::max(b.d.nvals, 0)),
                             c->d_entries + b.d.entry_base, c->d_bigd + b.lens_off,
                             reinterpret_cast<uint4*>(c->d_bigd + b.pad_off), c->d_dict_count + b.di,
                             c->d_dict_err + b.di, err_any, reinterpret_cast<uint32_t*>(c->d_bigd + b.scr_off));
}

// Run tables and per-row codes (k_pipe_runs, k_pipe_big, k_pipe_codes3; the
// exact decoder for pages outside the fast shape).  With dict_on_side the
// dictionary decodes on ctx->side and the codes wait for it (ev_join).
// With dict_in_runs the dictionary pages decode in k_pipe_runs' leading
// workgroups (same launch, main stream: ordered after the previous decode's
// readers of the entry table, no side-stream events).
void pipe_front(pq_ctx* ctx, pq_chunk* c, const pqk::PipeLaunch& P, bool dict_on_side, bool dict_in_runs) {
    hipStream_t s = ctx->stream;
    {
        Timed t(ctx, "pipe_runs");
        const pqk::RunDicts rd{c->d_dicts, c->ndicts, c->d_entries, c->d_dict_count, c->d_dict_err, c->d_dflag};
        pqk::launch_pipe_runs(s, c->d_bytes, c->d_pages, c->pipe_small ? c->npages : 0, c->max_def, c->max_rep,
                              c->d_runs, c->d_info, ctx->opt_run_pages, c->d_flist,  // flist[0], bsum: cleared with d_flags
                              ctx->opt_debug, dict_in_runs ? &rd : nullptr, 0u,
                              static_cast<uint32_t>(slot_bytes(c->pipe_small_bytes)), c->max_dict_bytes, ctx->cus);
    }
    // the wide pipe's k_pipe_big writes raw indices and needs no dictionary:
    // it runs beside the dictionary's decode, k_wide_chars after both
    if (dict_on_side && c->ndicts && !c->pipe_wide) (void)hipStreamWaitEvent(s, ctx->ev_join, 0);
    if (!c->hbig.empty()) {
        Timed t(ctx, "pipe_big");
        pqk::launch_pipe_big(s, P, c->d_bigp, static_cast<int>(c->hbig.size()), c->big_max_bytes);
    }
    if (c->pipe_wide) {
        if (dict_on_side && c->ndicts) (void)hipStreamWaitEvent(s, ctx->ev_join, 0);
        Timed t(ctx, "wide_chars");
        pqk::launch_wide_chars(s, P);
    }
    if (c->pipe_count) {
        Timed t(ctx, "pipe_count");
        pqk::launch_pipe_codes(s, P, true);
    }
    Timed t(ctx, "pipe_codes");
    pqk::launch_pipe_codes(s, P, false);
}

// ── one launcher per decode path (decode_launch chooses) ────────────────────

// The dictionary pages' decode, unless k_pipe_runs does it (dict_in_runs).
static void place_dicts(pq_ctx* ctx, pq_chunk* c, bool pipe) {
    hipStream_t s = ctx->stream;
    if (c->type == PQ_BYTE_ARRAY && pipe) {
        // the dictionary (one workgroup) decodes on the side stream while the
        // run-table pass runs; k_pipe_codes waits for both (ev_join).  The
        // side stream first waits for everything already on the main stream
        // (ev_fork): the previous decode's k_pipe_write / regex k_pipe_match
        // read the entry table this k_dict_index rewrites.  Its error flag is
        // its own sticky word (d_dflag), not the per-decode flags the main
        // stream clears.
        (void)hipEventRecord(ctx->ev_fork, s);
        (void)hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0);
        {
            Timed t(ctx, "dict_index", ctx->side);
            launch_dicts(c, ctx->side, c->d_dflag);
        }
        (void)hipEventRecord(ctx->ev_join, ctx->side);
    } else if (c->type == PQ_BYTE_ARRAY) {
        Timed t(ctx, "dict_index");
        launch_dicts(c, s, c->d_flags);
    } else {
        Timed t(ctx, "dict_entries");
        pqk::launch_dict_entries(s, c->d_bytes, c->d_dicts, c->ndicts, c->d_entries, c->d_dict_count,
                                 c->d_dict_err, c->d_flags, c->type, c->plain_width);
    }
}

// What the REQUIRED and the OPTIONAL PLAIN launches share (plain_ba.hip); the
// callers add pages, row count, outputs, error records and window mode.
static pqk::PlainLaunch plain_launch(pq_chunk* c, pq_column* out) {
    pqk::PlainLaunch P{};
    P.bytes = c->d_bytes; P.wins = c->d_pwins; P.nwins = static_cast<int32_t>(c->hpwins.size());
    P.rowinfo = c->d_rowinfo; P.wchars = c->d_wchars; P.bsum = c->d_pbsum; P.grid = c->plain_grid;
    P.total = c->d_total; P.capacity = out->capacity_bytes; P.overflow = c->d_flags + 1; P.chars = out->d_values;
    return P;
}

// ... and the speculative chunk chains of pages larger than a window
// (k_plain_spec); the callers add the error records.
static pqk::SpecLaunch spec_launch(pq_chunk* c) {
    pqk::SpecLaunch S{};
    S.bytes = c->d_bytes; S.pages = c->d_pages; S.npages = c->npages; S.chunk_base = c->d_chunk_base;
    S.chunks = c->d_chunks; S.nchunks = static_cast<int32_t>(c->hchunks.size()); S.cand = c->d_cand;
    S.ppages = c->d_ppages; S.fallback = c->d_flags + 2;
    return S;
}

// OPTIONAL chunk on the PLAIN kernels: levels -> value-section pages -> one
// pass over them -> row offsets; any error or misfit sets d_flags[3] and
// collect() re-runs the chunk on the general path (which reports the
// reference's errors)
static void launch_plain_opt(pq_ctx* ctx, pq_chunk* c, pq_column* out, const pqk::ColumnParams& cp) {
    hipStream_t s = ctx->stream;
    int32_t* redo = c->d_flags + 3;
    Timed t(ctx, "plain_opt");
    (void)hipMemsetAsync(c->d_operr, 0, static_cast<size_t>(c->npages) * sizeof(DevErr), s);
    if (c->opt_lane_levels)
        pqk::launch_opt_levels(s, c->d_bytes, c->d_pages, c->npages, c->d_page_tile0, c->max_def, out->d_validity,
                               c->d_tile_rank, c->d_page_pos, c->d_page_nn, c->d_operr, redo);
    else
        pqk::launch_fixed_levels(s, c->d_bytes, c->d_pages, c->npages, c->d_page_tile0, cp, out->d_validity,
                                 c->d_tile_rank, c->d_page_pos, c->d_page_nn, c->d_operr, redo, ctx->opt_levels_small);
    pqk::OptLaunch O{};
    O.pages = c->d_pages; O.npages = c->npages; O.page_nn = c->d_page_nn; O.page_pos = c->d_page_pos;
    O.lerr = c->d_operr; O.nnv = c->d_onnv; O.chv = c->d_ochv; O.pdense = c->d_opdense; O.pbase = c->d_opbase;
    O.scratch = c->d_scan_scratch; O.tot_nn = c->d_otot; O.tot_ch = c->d_otot + 1; O.vpages = c->d_vpages;
    O.doffs = c->d_doffs; O.redo = redo;
    pqk::launch_opt_pages(s, O);
    pqk::PlainLaunch P = plain_launch(c, out);
    P.pages = c->d_vpages; P.nrows_total = -1; P.validity = nullptr; P.offsets = c->d_doffs;
    P.page_err = c->d_operr; P.err_any = redo; P.redo = redo; P.gate = c->d_flags + 2;
    P.wmode = pqk::kWinOpt; P.pbase = c->d_opbase; P.pdense = c->d_opdense; P.ppos = c->d_page_pos;
    if (c->plain_spec) {
        pqk::SpecLaunch S = spec_launch(c);
        S.page_err = c->d_operr; S.err_any = redo; S.ppos = c->d_page_pos; S.vpages = c->d_vpages;
        pqk::launch_plain_spec(s, S);
        P.pages = c->d_ppages;
        P.wmode = pqk::kWinOptPseudo; P.wpage = c->d_pwpage; P.rpages = c->d_pages;
    }
    pqk::launch_plain_ba(s, P);
    pqk::launch_opt_offsets(s, c->d_pages, c->d_tiles, c->ntiles, c->d_tile_rank, c->d_opdense, out->d_validity,
                            c->d_doffs, out->d_offsets, redo);
    (void)hipMemcpyAsync(c->d_total, c->d_otot + 1, sizeof(int64_t), hipMemcpyDeviceToDevice, s);
    (void)hipMemcpyAsync(out->d_offsets + c->nrows, c->d_otot + 1, sizeof(int64_t), hipMemcpyDeviceToDevice, s);
}

// REQUIRED PLAIN BYTE_ARRAY chunk (plain_ba.hip): one pass when the windows'
// character counts are known, else two.
static void launch_plain_req(pq_ctx* ctx, pq_chunk* c, pq_column* out) {
    hipStream_t s = ctx->stream;
    pqk::PlainLaunch P = plain_launch(c, out);
    P.pages = c->d_pages; P.nrows_total = c->nrows; P.validity = out->d_validity; P.offsets = out->d_offsets;
    P.page_err = c->d_page_err; P.err_any = c->d_flags;
    if (c->nrows == 0) {
        (void)hipMemsetAsync(out->d_offsets, 0, sizeof(int64_t), s);
        (void)hipMemsetAsync(c->d_total, 0, sizeof(int64_t), s);
    }
    const bool one_pass = c->d_pwbase && ctx->opt_plain_fused && !c->pfused_failed;
    if (one_pass) {
        P.wbase = c->d_pwbase;
        P.redo = c->d_flags + 3;
    }
    if (c->plain_spec) {
        // pseudo pages from speculative chunk chains; a fallback flag
        // (d_flags[2]) skips the two passes and collect() re-runs the
        // chunk on the generic path
        pqk::SpecLaunch S = spec_launch(c);
        S.page_err = c->d_page_err; S.err_any = c->d_flags;
        {
            Timed t(ctx, "plain_spec");
            pqk::launch_plain_spec(s, S);
        }
        P.pages = c->d_ppages;
        P.page_err = c->d_perr;
        P.gate = c->d_flags + 2;
        if (one_pass) P.wmode = pqk::kWinPseudo;
    }
    Timed t(ctx, "plain_ba");
    pqk::launch_plain_ba(s, P);
}

// Three-pass dictionary path (dict_pipe.hip); with c->arm the regex page
// filter runs in the same pass.
static void launch_pipe(pq_ctx* ctx, pq_chunk* c, pq_column* out, bool dict_in_runs) {
    hipStream_t s = ctx->stream;
    pqk::PipeLaunch P = pipe_launch(ctx, c, out);
    pipe_front(ctx, c, P, !dict_in_runs, dict_in_runs);
    if (c->arm) {  // the page filter in the same pass: match bits per entry, then the writer tests them
        Timed t(ctx, "regex_dict");
        pqre::launch_regex_dict(s, c->d_prog, c->d_bytes, c->d_dicts, c->ndicts, c->d_entries, c->d_dict_count,
                                c->d_dict_match, c->d_page_flags, c->npages);
        P.match = c->d_dict_match + c->pipe_entry_base;
        P.match_neg = c->arm_neg;
        P.page_flags = c->d_page_flags;
    }
    if (c->ntiles == 0) {
        (void)hipMemsetAsync(out->d_offsets, 0, sizeof(int64_t), s);
        (void)hipMemsetAsync(c->d_total, 0, sizeof(int64_t), s);
    }
    if (c->d_zero) {  // k_pipe_write clears the other block for the next decode
        P.znext = reinterpret_cast<uint32_t*>(c->d_zero + static_cast<size_t>(c->zsel ^ 1) * c->zfull);
        P.znext_words = static_cast<uint32_t>(c->zero_bytes / 4);
    }
    {
        Timed t(ctx, "pipe_write");
        pqk::launch_pipe_write(s, P);
    }
    // the other block is clear only if k_pipe_write ran (it returns early on a chunk without tiles)
    if (c->d_zero) c->next_zeroed = c->ntiles > 0;
}

// Fused BYTE_ARRAY path (dict_fused.hip): one launch per input chunk.
static void launch_fused(pq_ctx* ctx, pq_chunk* c, pq_column* out) {
    hipStream_t s = ctx->stream;
    const size_t nr = c->ranges.size();
    (void)hipMemsetAsync(c->d_status, 0, std::max<size_t>(c->npages, 1) * sizeof(uint64_t), s);
    (void)hipMemsetAsync(c->d_tickets, 0, nr * sizeof(int32_t), s);
    (void)hipMemsetAsync(c->d_bases, 0, (nr + 1) * sizeof(int64_t), s);
    for (size_t k = 0; k < nr; k++) {
        const auto& r = c->ranges[k];
        if (r.np == 0) {
            (void)hipMemcpyAsync(c->d_bases + k + 1, c->d_bases + k, sizeof(int64_t), hipMemcpyDeviceToDevice, s);
            continue;
        }
        pqk::FusedLaunch L{};
        L.bytes = c->d_bytes; L.pages = c->d_pages; L.p0 = r.p0; L.np = r.np;
        L.dicts = c->d_dicts; L.dict_id = r.dict_id; L.entries = c->d_entries;
        L.dict_count = c->d_dict_count; L.max_def = c->max_def; L.max_rep = c->max_rep;
        L.rows_cap = r.rows_cap; L.stage_bytes = r.stage_bytes; L.wave_bytes = r.wave_bytes;
        L.dict_bytes = r.dict_bytes; L.dict_chars_bytes = r.dict_chars_bytes;
        L.status = c->d_status + r.p0; L.ticket = c->d_tickets + k;
        L.base_in = c->d_bases + k; L.base_out = c->d_bases + k + 1; L.nrows_total = c->nrows;
        L.validity = out->d_validity; L.offsets = out->d_offsets; L.chars = out->d_values;
        L.capacity = out->capacity_bytes; L.overflow = c->d_flags + 1;
        L.page_err = c->d_page_err; L.err_any = c->d_flags; L.grid = r.grid; L.waves_per_block = r.waves;
        L.debug = ctx->opt_debug;
        L.prof = ctx->d_prof;
        L.claim = ctx->opt_claim;
        Timed t(ctx, "ba_fused");
        pqk::launch_ba_fused(s, L);
    }
    (void)hipMemcpyAsync(c->d_total, c->d_bases + nr, sizeof(int64_t), hipMemcpyDeviceToDevice, s);
    (void)hipMemcpyAsync(out->d_offsets + c->nrows, c->d_bases + nr, sizeof(int64_t), hipMemcpyDeviceToDevice, s);
}

// Generic BYTE_ARRAY path: rows -> scan -> gather.
static void launch_ba_generic(pq_ctx* ctx, pq_chunk* c, pq_column* out, const pqk::ColumnParams& cp) {
    hipStream_t s = ctx->stream;
    {
        Timed t(ctx, "ba_rows");
        const uint32_t big = (c->max_def == 0 && c->max_rep == 0 && ctx->opt_plain) ? pqk::ba_rows_stage_bytes() : 0u;
        pqk::launch_ba_rows(s, c->d_bytes, c->d_pages, c->npages, c->d_dicts, c->d_entries,
                            c->d_dict_count, cp, c->d_row_codes, c->d_tile_chars,
                            c->d_page_tile0, c->d_page_err, c->d_flags, big, c->max_page_bytes,
                            ctx->opt_wide_rows && c->ndicts > 0, ctx->d_prof);
        if (big)
            pqk::launch_plain_big_rows(s, c->d_bytes, c->d_pages, c->npages, big, c->d_row_codes,
                                       c->d_tile_chars, c->d_page_tile0, c->d_page_err, c->d_flags);
    }
    {
        Timed t(ctx, "scan");
        pqk::launch_scan_i64(s, c->d_tile_chars, c->d_tile_base, c->ntiles, c->d_total, c->d_scan_scratch);
    }
    if (c->ntiles == 0) (void)hipMemsetAsync(out->d_offsets, 0, sizeof(int64_t), s);
    Timed t(ctx, "ba_gather");
    pqk::launch_ba_gather(s, c->d_bytes, c->d_pages, c->d_tiles, c->ntiles, c->d_dicts,
                          c->d_entries, c->d_row_codes, c->d_tile_base, c->nrows, c->d_total,
                          out->capacity_bytes, c->d_flags + 1, out->d_validity, out->d_offsets,
                          out->d_values, !ctx->opt_gather_rows);
}

// Fixed-width types: the tile-parallel PLAIN kernels (fixed_fast.hip), or the
// general kernel (dictionary pages, BOOLEAN).
static void launch_fixed_width(pq_ctx* ctx, pq_chunk* c, pq_column* out, const pqk::ColumnParams& cp) {
    hipStream_t s = ctx->stream;
    if (c->fixed_plain && ctx->opt_fixed_plain) {
        Timed t(ctx, "fixed_plain");
        pqk::launch_fixed_plain(s, c->d_bytes, c->d_pages, c->npages, c->d_tiles, c->ntiles, c->d_page_tile0, cp,
                                out->d_validity, out->d_values, c->d_tile_rank, c->d_page_pos, c->d_page_err,
                                c->d_flags, ctx->opt_fixed_fused, ctx->opt_levels_small);
    } else {
        Timed t(ctx, "fixed");
        pqk::launch_fixed(s, c->d_bytes, c->d_pages, c->npages, c->d_dicts, c->d_dict_count, cp,
                          out->d_validity, out->d_values, c->d_page_err, c->d_flags);
    }
}

static int decode_launch(pq_ctx* ctx, pq_chunk* c, pq_column* out) {
    hipStream_t s = ctx->stream;
    pqk::ColumnParams cp{c->type, c->max_def, c->max_rep, c->width, c->plain_width};
    const bool pipe = c->pipe && ctx->opt_pipe;
    // OPTIONAL chunks take the PLAIN kernels only in their one-pass form
    const bool plain_go = c->plain && ctx->opt_plain && !(c->plain_spec && c->spec_failed) &&
                          !(c->plain_opt && (c->popt_failed || !ctx->opt_plain_fused));
    const bool pipe_path = pipe && !plain_go;
    if (pipe_path) c->codes_pending = true;
    if (c->ndicts && c->type == PQ_BYTE_ARRAY) c->entries_pending = true;
    if (pipe_path && c->d_zero && ctx->opt_zflip) {
        // flags, bsum and flist[0] of this decode: the other block, which the
        // previous decode's k_pipe_write cleared (else one fill)
        c->zsel ^= 1;
        uint8_t* zb = c->d_zero + static_cast<size_t>(c->zsel) * c->zfull;
        c->d_flags = reinterpret_cast<int32_t*>(zb);
        c->d_bsum = reinterpret_cast<unsigned long long*>(zb + c->z_bsum);
        c->d_flist = reinterpret_cast<int32_t*>(zb + c->z_flist);
        if (!c->next_zeroed) (void)hipMemsetAsync(c->d_flags, 0, c->zero_bytes, s);
        c->next_zeroed = false;
    } else {
        (void)hipMemsetAsync(c->d_flags, 0, c->zero_bytes, s);  // pipe chunks: flags, bsum and flist[0] at once
    }
    // k_pipe_write stores whole validity words when every tile starts on a
    // 32-row boundary; other paths OR bits into zeroed words
    if (!(pipe_path && c->tiles_aligned32))
        (void)hipMemsetAsync(out->d_validity, 0, static_cast<size_t>(c->nrows / 32 + 4) * 4, s);
    // dictionary pages small enough for k_pipe_runs' workgroups decode there
    const bool dict_in_runs = pipe && !plain_go && ctx->opt_run_dict && c->ndicts &&
                              c->type == PQ_BYTE_ARRAY && c->d_dflag && c->max_dict_bytes <= pqk::kRunDictMax;
    if (c->ndicts && !dict_in_runs) place_dicts(ctx, c, pipe);
    if (plain_go && c->plain_opt) launch_plain_opt(ctx, c, out, cp);
    else if (plain_go) launch_plain_req(ctx, c, out);
    else if (pipe) launch_pipe(ctx, c, out, dict_in_runs);
    else if (c->fused) launch_fused(ctx, c, out);
    else if (c->type == PQ_BYTE_ARRAY) launch_ba_generic(ctx, c, out, cp);
    else launch_fixed_width(ctx, c, out, cp);
    return hip_check(ctx, hipGetLastError(), "kernel launch");
}

// PQ_DEBUG_SPEC: why a PLAIN fast path gave up (opt: the OPTIONAL form's page
// records; then the speculative chains' candidates).
static void debug_spec(const pq_chunk* c, const int32_t* flags, bool opt) {
    if (!std::getenv("PQ_DEBUG_SPEC")) return;
    if (opt) {
        std::fprintf(stderr, "plain opt redo: fallback %d flag %d\n", flags[2], flags[3]);
        std::vector<DevErr> e(static_cast<size_t>(c->npages));
        std::vector<int32_t> pp(e.size()), pn(e.size());
        (void)hipMemcpy(e.data(), c->d_operr, e.size() * sizeof(DevErr), hipMemcpyDeviceToHost);
        (void)hipMemcpy(pp.data(), c->d_page_pos, pp.size() * 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(pn.data(), c->d_page_nn, pn.size() * 4, hipMemcpyDeviceToHost);
        for (size_t i = 0; i < e.size() && i < 8; i++)
            std::fprintf(stderr, "  page %zu: err %d pos %d need %d size %d; values at %d, %d non-null\n", i, e[i].code,
                         e[i].pos, e[i].need, e[i].size, pp[i], pn[i]);
        if (!c->plain_spec) return;
    } else {
        std::fprintf(stderr, "plain spec fallback: flags %d (reason %d, chunk %d)\n", flags[2], flags[2] & 0xFF, flags[2] >> 8);
    }
    std::vector<uint4> cd(std::min<size_t>(c->hchunks.size(), opt ? 8 : 4) * pqk::kPCand);
    (void)hipMemcpy(cd.data(), c->d_cand, cd.size() * sizeof(uint4), hipMemcpyDeviceToHost);
    for (size_t i = 0; i < cd.size(); i++)
        if (!opt || cd[i].x != 0xFFFFFFFFu)
            std::fprintf(stderr, "  cand chunk %zu slot %zu: entry %u err %u exit %u cnt %u w %u\n", i / pqk::kPCand,
                         i % pqk::kPCand, cd[i].x & 0x7FFFFFFFu, cd[i].x >> 31, cd[i].y, cd[i].z, cd[i].w);
}

// A fast path gave up on this chunk (the caller set its *_failed flag): the
// decode runs again on the path that now applies, and is checked.
static int rerun(pq_ctx* ctx, pq_chunk* c, pq_column* out, bool clear_page_err) {
    if (clear_page_err && c->npages) (void)hipMemsetAsync(c->d_page_err, 0, c->npages * sizeof(DevErr), ctx->stream);
    if (!out) out = c->last_out;
    if (!out) return set_err(ctx, PQ_ERR_ARG, "decode check without an output column");
    if (int rc = pq_decode_async(ctx, c, out)) return rc;
    return collect(ctx, c, out);
}

// Synchronise and turn device error records into the reference's first error.
int collect(pq_ctx* ctx, pq_chunk* c, pq_column* out) {
    int32_t flags[4] = {0, 0, 0, 0}, dflag = 0;
    if (int rc = hip_check(ctx, hipMemcpyAsync(flags, c->d_flags, sizeof flags, hipMemcpyDeviceToHost, ctx->stream), "flags"))
        return rc;
    if (c->d_dflag)
        if (int rc = hip_check(ctx, hipMemcpyAsync(&dflag, c->d_dflag, sizeof dflag, hipMemcpyDeviceToHost, ctx->stream), "flags"))
            return rc;
    if (int rc = hip_check(ctx, hipStreamSynchronize(ctx->stream), "sync")) return rc;
    flags[0] |= dflag;
    if ((flags[2] || flags[3]) && c->plain && c->plain_opt && !c->popt_failed) {
        // the OPTIONAL chunk did not fit the PLAIN kernels' form (an error,
        // or value sections their strings do not fill): the general path
        // decodes it from now on and reports any error
        debug_spec(c, flags, true);
        c->popt_failed = true;
        return rerun(ctx, c, out, true);
    }
    if (flags[3] && c->plain && !c->plain_opt && !c->pfused_failed && !(flags[2] && c->plain_spec)) {
        // a page's strings did not fill it exactly (or its chain failed): the
        // one-pass PLAIN kernel's character placement does not hold; the two
        // passes decode the chunk from now on (and report any error)
        c->pfused_failed = true;
        return rerun(ctx, c, out, false);
    }
    if (flags[2] && c->plain_spec && !c->spec_failed) {
        // the speculative chunk chains did not resolve (strings longer than
        // the candidate range or the window): this chunk takes the generic
        // path from now on; decode it again
        debug_spec(c, flags, false);
        c->spec_failed = true;
        return rerun(ctx, c, out, true);
    }
    int64_t best_seq = c->walk_error ? c->walk_error_seq : INT64_MAX;
    int best_code = c->walk_error;
    std::string best_msg = c->walk_message;
    if (flags[0]) {
        std::vector<DevErr> pe(c->npages), de(c->ndicts);
        if (c->npages) (void)hipMemcpy(pe.data(), c->d_page_err, pe.size() * sizeof(DevErr), hipMemcpyDeviceToHost);
        if (c->ndicts) (void)hipMemcpy(de.data(), c->d_dict_err, de.size() * sizeof(DevErr), hipMemcpyDeviceToHost);
        auto first = [&](const DevErr& e, int64_t seq) {  // the error earliest in walk order
            if (!e.code || seq >= best_seq) return;
            best_seq = seq;
            best_code = e.code;
            best_msg = format_error(e);
        };
        for (int i = 0; i < c->npages; i++) first(pe[i], c->page_seq[i]);
        for (int i = 0; i < c->ndicts; i++) first(de[i], c->dict_seq[i]);
        // clear records for the next call
        if (c->npages) (void)hipMemsetAsync(c->d_page_err, 0, c->npages * sizeof(DevErr), ctx->stream);
        // (dictionary records of chunks decoded on the side stream stay: the
        // next decode's dictionary pass may already be writing them again)
        if (c->ndicts && !c->d_dflag) (void)hipMemsetAsync(c->d_dict_err, 0, c->ndicts * sizeof(DevErr), ctx->stream);
    }
    if (best_code) {
        c->codes_pending = c->entries_pending = c->rx_index_pending = false;
        return set_err(ctx, best_code, best_msg);
    }
    if (c->codes_pending) c->codes_ok = true;
    if (c->entries_pending) c->entries_ok = true;
    if (c->rx_index_pending) c->rx_index_ok = true;
    c->codes_pending = c->entries_pending = c->rx_index_pending = false;
    if (c->type == PQ_BYTE_ARRAY && out) {
        int64_t total = 0;
        (void)hipMemcpy(&total, c->d_total, sizeof total, hipMemcpyDeviceToHost);
        out->num_bytes = total;
        if (flags[1]) {  // chars overflowed the estimate: grow and run again
            dfree(out->d_values);
            if (dalloc(&out->d_values, static_cast<size_t>(total + 64)))
                return set_err(ctx, PQ_ERR_HIP, "hipMalloc failed (chars)");
            out->capacity_bytes = total;
            if (int rc = pq_decode_async(ctx, c, out)) return rc;  // every path writes the whole column
            return hip_check(ctx, hipStreamSynchronize(ctx->stream), "sync");
        }
    } else if (out) {
        out->num_bytes = c->nrows * c->width;
    }
    return 0;
}

}  // namespace pqcapi

using namespace pqcapi;

extern "C" {

int pq_decode_async(pq_ctx* ctx, pq_chunk* c, pq_column* out) {
    if (!ctx || !c || !out) return PQ_ERR_ARG;
    DevGuard dg(ctx);
    const int64_t char_cap = c->type == PQ_BYTE_ARRAY ? std::max<int64_t>(out->capacity_bytes, c->char_estimate) : 0;
    if (int rc = ensure_output(ctx, c, out, char_cap)) return rc;
    c->last_out = out;
    return decode_launch(ctx, c, out);
}

int pq_decode_check(pq_ctx* ctx, pq_chunk* c) {
    if (!ctx || !c) return PQ_ERR_ARG;
    DevGuard dg(ctx);
    // the column of the chunk's last async decode gets its byte count (and
    // grows and decodes again if its characters overflowed the estimate)
    // (the column is the caller's: once collected, no later call touches it)
    const int rc = collect(ctx, c, c->last_out);
    c->last_out = nullptr;
    return rc;
}

int pq_decode(pq_ctx* ctx, pq_chunk* c, pq_column* out) {
    DevGuard dg(ctx);
    if (int rc = pq_decode_async(ctx, c, out)) return rc;
    const int rc = collect(ctx, c, out);
    c->last_out = nullptr;
    return rc;
}

int pq_column_copy_out(pq_ctx* ctx, const pq_column* col, uint32_t* validity, uint8_t* values,
                       int64_t* offsets) {
    if (!ctx || !col) return PQ_ERR_ARG;
    // a column a failed decode left behind (its byte count past its buffer)
    if (col->num_bytes < 0 || col->num_rows < 0 || (col->num_bytes && (!col->d_values || col->num_bytes > col->capacity_bytes)))
        return set_err(ctx, PQ_ERR_ARG, "column bytes past its buffer");
    DevGuard dg(ctx);
    hipStream_t s = ctx->stream;
    int rc = hip_check(ctx, hipStreamSynchronize(s), "copy sync");  // (the decode that made the column)
    // large arrays through the pinned ring (DMA of piece i + k while host
    // threads copy piece i out: pageable destinations would take the
    // runtime's bounce buffer at a fraction of PCIe bandwidth, one thread)
    const int hw = host_threads();
    auto get = [&](void* dst, const void* src, size_t n, const char* what) {
        if (!dst || !n || rc) return;
        if (n < (4u << 20)) {
            rc |= hip_check(ctx, hipMemcpy(dst, src, n, hipMemcpyDeviceToHost), what);
            return;
        }
        uint8_t* d = static_cast<uint8_t*>(dst);
        rc |= hip_check(ctx, ctx->stager.download(static_cast<const uint8_t*>(src), n, ctx->copy, hw,
                                                  [&](const uint8_t* b, size_t a, size_t z) { std::memcpy(d + a, b, z - a); }),
                        what);
    };
    if (col->num_rows) get(validity, col->d_validity, static_cast<size_t>((col->num_rows + 31) / 32) * 4, "copy validity");
    if (col->num_bytes) get(values, col->d_values, static_cast<size_t>(col->num_bytes), "copy values");
    if (col->d_offsets) get(offsets, col->d_offsets, static_cast<size_t>(col->num_rows + 1) * 8, "copy offsets");
    return rc ? PQ_ERR_HIP : 0;
}

int pq_chunk_assign(pq_ctx* ctx, const pq_column* col, int64_t chunk_bytes, int64_t* d_tuple_to_chunk,
                    int64_t* h_tuple_to_chunk, int64_t* num_chunks) {
    if (!ctx || !col || !num_chunks || chunk_bytes < 0) return PQ_ERR_ARG;
    DevGuard dg(ctx);
    if (col->type != PQ_BYTE_ARRAY || (col->num_rows > 0 && (!col->d_validity || !col->d_offsets)))
        return set_err(ctx, PQ_ERR_ARG, "pq_chunk_assign: a decoded BYTE_ARRAY column is required");
    (void)hipSetDevice(ctx->device);
    const int64_t n = col->num_rows;
    const size_t out_bytes = d_tuple_to_chunk ? 0 : (static_cast<size_t>(std::max<int64_t>(n, 1)) * 8 + 255) / 256 * 256;
    const size_t need = pqk::chunk_assign_scratch(n) + out_bytes;
    if (!dgrow(ctx->d_chunker, ctx->chunker_cap, need)) return set_err(ctx, PQ_ERR_HIP, "hipMalloc failed (chunker)");
    int64_t* out = d_tuple_to_chunk ? d_tuple_to_chunk : reinterpret_cast<int64_t*>(ctx->d_chunker);
    int rc = pqk::chunk_assign(ctx->stream, col->d_validity, col->d_offsets, n, chunk_bytes, out,
                               ctx->d_chunker + out_bytes, num_chunks);
    if (rc == -2) return set_err(ctx, PQ_ERR_UNSUPPORTED, "pq_chunk_assign: column too large");
    if (rc) return set_err(ctx, PQ_ERR_HIP, "pq_chunk_assign: HIP failure");
    if (h_tuple_to_chunk && n > 0)
        return hip_check(ctx, hipMemcpy(h_tuple_to_chunk, out, static_cast<size_t>(n) * 8, hipMemcpyDeviceToHost),
                         "chunker copy-out");
    return 0;
}

void pq_column_free(pq_ctx* ctx, pq_column* col) {
    DevGuard dg(ctx);
    if (!col) return;
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    dfree(col->d_validity);
    dfree(col->d_values);
    dfree(col->d_offsets);
    std::memset(col, 0, sizeof *col);
}

}  // extern "C"
