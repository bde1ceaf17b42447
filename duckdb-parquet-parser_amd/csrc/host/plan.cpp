// plan.cpp — host-side planning of a device chunk's launches: which kernel
// path a chunk takes (dict_pipe.hip, plain_ba.hip, dict_fused.hip), its
// LDS carve-up and grid, the page and tile tables of a walk, and the windows
// of the windowed regex scan.  No launches here (capi_upload.hip,
// capi_decode.hip and capi_regex.hip run them).
#include <algorithm>
#include <cstring>

#include "host/capi_state.hpp"

namespace pqcapi __attribute__((visibility("hidden"))) {

// The three-pass dictionary path (dict_pipe.hip) takes a BYTE_ARRAY chunk
// whose data pages all use one dictionary page that fits in LDS.
// Dictionaries the writer's LDS cannot hold (or of more than 65,535 entries):
// every page through k_pipe_big<true> (32-bit codes, index bit widths up to
// 24, entry lengths from HBM), then k_pipe_wwide, which reads the entry words
// and characters from HBM/L2.  Called by plan_pipe after its page checks
// (dictionary-encoded pages of one dictionary).
static void plan_pipe_wide(pq_ctx* ctx, pq_chunk* c, const PVec<DevPage>& pages, const DevDict& d, int32_t dict_id) {
    if (!ctx->opt_pipe_wide) return;
    std::vector<int32_t> big;
    uint32_t big_bytes = 0;
    big.reserve(pages.size());
    for (size_t i = 0; i < pages.size(); i++) {
        const DevPage& pg = pages[i];
        if (pg.nvals > pqk::kBigTiles * pqk::kTileRows || static_cast<uint32_t>(pg.size) > pqk::kBigMaxBytes) return;
        big.push_back(static_cast<int32_t>(i));
        big_bytes = std::max(big_bytes, static_cast<uint32_t>(pg.size));
    }
    if (pqk::pipe_big_lds(big_bytes, 0) > 160u * 1024) return;
    // a dictionary page past k_dict_index's LDS decodes in launch_dict_big,
    // which also files its 16-byte entry slots: the writer keeps one per row
    // of its tile in LDS (10 KiB per wave: four waves per workgroup, three
    // workgroups per CU; five per workgroup measured 82 vs 58 µs, r4e)
    const bool pad = static_cast<uint64_t>(std::max(d.size, 0)) + 32 > pqk::kDictLdsCap;
    const int wpw = std::max(1, std::min(pad ? 4 : 16, ctx->opt_write_waves));
    pqk::PipePlan pl = pqk::plan_pipe_wide(wpw, pad);
    if (pl.blocks_per_cu == 0) return;
    if (ctx->opt_write_bpc > 0) pl.blocks_per_cu = std::min(pl.blocks_per_cu, ctx->opt_write_bpc);
    c->pipe = true;
    c->pipe_wide = true;
    c->pipe_small = false;
    c->pipe_small_bytes = 0;
    c->pipe_count = false;
    c->hbig = std::move(big);
    c->big_max_bytes = big_bytes;
    c->pipe_dict = dict_id;
    c->pipe_dict_payload = static_cast<uint32_t>(d.size);
    c->pipe_entry_base = d.entry_base;
    c->pipe_dict_chars_bytes = 0;
    c->pipe_dict_bytes = 0;
    c->pipe_lds = pl.lds;
    c->pipe_grid = ctx->cus * pl.blocks_per_cu;
    c->pipe_ecap = static_cast<uint32_t>(dict_entry_cap(d.nvals, d.size));
    c->pipe_cus = ctx->cus;
    c->pipe_wpw = wpw;
}

void plan_pipe(pq_ctx* ctx, pq_chunk* c, const PVec<DevPage>& pages, const std::vector<DevDict>& dicts) {
    c->pipe = false;
    c->pipe_wide = false;
    c->pipe_count = false;
    c->pipe_small = false;
    c->hbig.clear();
    c->big_max_bytes = 0;
    if (c->type != PQ_BYTE_ARRAY || c->max_def > 254 || c->max_def < 0 || c->max_rep < 0 || pages.empty()) return;
    int32_t dict_id = -1;
    bool multi = false, small = false;
    std::vector<int32_t> big;
    uint32_t big_bytes = 0, small_bytes = 0;
    for (size_t i = 0; i < pages.size(); i++) {
        const DevPage& pg = pages[i];
        if (pg.mode != pqk::MODE_DICT || pg.size > (1 << 27) || pg.size < 0) return;
        if (pg.nvals > pqk::kPipeSmallRows || ctx->opt_big_all) {
            // k_pipe_big: the page's jump table and up to kBigTiles tiles in one workgroup
            if (pg.nvals > pqk::kBigTiles * pqk::kTileRows || static_cast<uint32_t>(pg.size) > pqk::kBigMaxBytes) return;
            big.push_back(static_cast<int32_t>(i));
            big_bytes = std::max(big_bytes, static_cast<uint32_t>(pg.size));
        } else {
            small = true;
            multi |= pg.nvals > pqk::kTileRows;
            small_bytes = std::max(small_bytes, static_cast<uint32_t>(pg.size));
        }
        if (dict_id >= 0 && pg.dict != dict_id) return;
        dict_id = pg.dict;
    }
    const DevDict& d = dicts[dict_id];
    if (d.size < 0 || d.nvals < 0) return;
    if (d.size > 65536 - 64 || d.nvals > 65535) return plan_pipe_wide(ctx, c, pages, d, dict_id);
    const int64_t ecap = dict_entry_cap(d.nvals, d.size);
    if (!big.empty() && pqk::pipe_big_lds(big_bytes, std::min<uint32_t>(static_cast<uint32_t>(ecap), pqk::kBigLens)) > 160u * 1024)
        return;
    const uint32_t chars_bytes = (static_cast<uint32_t>(d.size) + 15) / 16 * 16 + 16;
    const uint32_t dict_bytes = 16 + chars_bytes + static_cast<uint32_t>((4 * ecap + 15) / 16 * 16);
    const int wpw = std::max(1, std::min(16, ctx->opt_write_waves));
    pqk::PipePlan pl = pqk::plan_pipe_lds(dict_bytes, wpw);
    if (pl.blocks_per_cu == 0) return plan_pipe_wide(ctx, c, pages, d, dict_id);
    if (ctx->opt_write_bpc > 0) pl.blocks_per_cu = std::min(pl.blocks_per_cu, ctx->opt_write_bpc);
    const int cus = ctx->cus;
    c->pipe = true;
    c->pipe_small = small;
    c->pipe_small_bytes = small_bytes;
    c->pipe_count = multi && c->max_def > 0;
    c->hbig = std::move(big);
    c->big_max_bytes = big_bytes;
    c->pipe_dict = dict_id;
    c->pipe_dict_payload = static_cast<uint32_t>(d.size);
    c->pipe_entry_base = d.entry_base;
    c->pipe_dict_chars_bytes = chars_bytes;
    c->pipe_dict_bytes = dict_bytes;
    c->pipe_lds = pl.lds;
    c->pipe_grid = cus * pl.blocks_per_cu;
    c->pipe_ecap = static_cast<uint32_t>(ecap);
    c->pipe_cus = cus;
    c->pipe_wpw = wpw;
}

static uint64_t page_slot(const DevPage& p) { return static_cast<uint64_t>(slot_bytes(std::max(p.size, 0))); }

// The window of consecutive page slots that starts at page p: <= 64 pages of
// [p, end) and <= win bytes of image (p's slot fits).  *chars gets its
// characters if every page's strings fill it exactly (size - 4 * num_values,
// verified on the device); *known goes false when a page's cannot.
static pqk::DevBatch page_window(const DevPage* pages, size_t p, size_t end, uint64_t win, int64_t* chars, bool* known) {
    pqk::DevBatch b{};
    b.p0 = static_cast<int32_t>(p);
    b.img_lo = pages[p].off;
    uint64_t hi = b.img_lo;
    size_t q = p;
    for (; q < end && q - p < 64 && pages[q].off >= b.img_lo; q++) {
        const uint64_t e = pages[q].off + page_slot(pages[q]);
        if (e - b.img_lo > win) break;
        hi = e;
        const int64_t x = static_cast<int64_t>(pages[q].size) - 4 * static_cast<int64_t>(pages[q].nvals);
        *known &= x >= 0;
        *chars += x;
        b.nrows += static_cast<uint32_t>(std::max(pages[q].nvals, 0));
    }
    b.row0 = pages[p].first_row;
    b.np = static_cast<int32_t>(q - p);
    b.img_bytes = static_cast<uint32_t>(hi - b.img_lo);
    return b;
}

// plan_plain with a page larger than a window: every page in kPChunk-byte
// chunks, windows of kPChunkGroup chunks (the pseudo pages k_plain_link
// writes, one per chunk).  False: too many pages or chunks.
static bool plan_plain_chunks(pq_chunk* c, const PVec<DevPage>& pages, bool opt) {
    if (pages.size() > (1u << 24)) return false;
    int64_t nch = 0;
    for (size_t p = 0; p < pages.size(); p++) {
        const uint32_t size = static_cast<uint32_t>(std::max(pages[p].size, 0));
        const uint32_t k = std::max<uint32_t>(1, (size + pqk::kPChunk - 1) / pqk::kPChunk);
        c->hchunk_base.push_back(static_cast<int32_t>(nch));
        for (uint32_t i = 0; i < k; i++) c->hchunks.push_back(make_uint2(static_cast<uint32_t>(p), i));
        const uint64_t se = pages[p].off + page_slot(pages[p]);
        for (uint32_t g = 0; g < k; g += pqk::kPChunkGroup) {
            pqk::DevBatch b{};
            b.p0 = static_cast<int32_t>(nch + g);
            b.np = static_cast<int32_t>(std::min(pqk::kPChunkGroup, k - g));
            b.img_lo = pages[p].off + static_cast<uint64_t>(g) * pqk::kPChunk;
            b.img_bytes = static_cast<uint32_t>(std::min<uint64_t>(pqk::kPWin, se - b.img_lo));
            c->hpwins.push_back(b);
        }
        nch += k;
        if (nch > (1ll << 30)) return false;
    }
    c->hchunk_base.push_back(static_cast<int32_t>(nch));
    c->plain_spec = true;
    for (const auto& b : c->hpwins) c->hpwpage.push_back(static_cast<int32_t>(c->hchunks[static_cast<size_t>(b.p0)].x));
    // one-pass form over the pseudo pages (k_plain_fused, kWinPseudo): per
    // window, its page's first output byte (pages whose strings fill them
    // exactly: size - 4 * num_values each, verified on the device) minus
    // the page's image offset plus 4 x its first row
    bool known = true;
    std::vector<int64_t> pbase(pages.size());
    int64_t acc = 0;
    for (size_t p = 0; p < pages.size(); p++) {
        pbase[p] = acc;
        const int64_t x = static_cast<int64_t>(pages[p].size) - 4 * static_cast<int64_t>(pages[p].nvals);
        known &= x >= 0;
        acc += x;
    }
    if (known && !opt) {
        c->hpwbase.reserve(c->hpwins.size());
        for (const auto& b : c->hpwins) {
            const uint2 ch = c->hchunks[static_cast<size_t>(b.p0)];
            const DevPage& pg = pages[ch.x];
            c->hpwbase.push_back(pbase[ch.x] - static_cast<int64_t>(pg.off) + 4 * pg.first_row);
        }
    }
    return true;
}

// ... and with pages that all fit: greedy windows from the start of each page
// range (one range per host thread; a range start also starts a window), with
// each window's characters for the one-pass form (k_plain_fused).
static void plan_plain_windows(pq_chunk* c, const PVec<DevPage>& pages, bool opt) {
    const size_t NP = pages.size();
    const int T = static_cast<int>(std::min<size_t>(16, std::max<size_t>(1, NP / 16384)));
    const size_t per = (NP + static_cast<size_t>(T) - 1) / static_cast<size_t>(T);
    std::vector<std::vector<pqk::DevBatch>> wparts(static_cast<size_t>(T));
    std::vector<std::vector<int64_t>> cparts(static_cast<size_t>(T));
    std::vector<char> kparts(static_cast<size_t>(T), 1);
    pqfmt::parallel_run(T, T, [&](int t) {
        auto& W = wparts[static_cast<size_t>(t)];
        auto& C = cparts[static_cast<size_t>(t)];
        const size_t end = std::min(NP, (static_cast<size_t>(t) + 1) * per);
        W.reserve((end - std::min(end, static_cast<size_t>(t) * per)) / 4 + 1);
        C.reserve(W.capacity());
        bool known = true;
        for (size_t p = static_cast<size_t>(t) * per; p < end; p += static_cast<size_t>(W.back().np)) {
            int64_t ch = 0;
            W.push_back(page_window(pages.data(), p, end, pqk::kPWin, &ch, &known));
            C.push_back(ch);
        }
        kparts[static_cast<size_t>(t)] = known;
    });
    bool known = true;
    size_t nw = 0;
    for (int t = 0; t < T; t++) {
        nw += wparts[static_cast<size_t>(t)].size();
        known &= kparts[static_cast<size_t>(t)] != 0;
    }
    c->hpwins.reserve(nw);
    for (const auto& W : wparts) c->hpwins.insert(c->hpwins.end(), W.begin(), W.end());
    if (known && !opt) {
        c->hpwbase.reserve(nw + 1);
        c->hpwbase.push_back(0);
        for (const auto& C : cparts)
            for (int64_t ch : C) c->hpwbase.push_back(c->hpwbase.back() + ch);
    }
}

// PLAIN BYTE_ARRAY chunks without levels go through plain_ba.hip: windows of
// consecutive page slots of at most kPWin bytes.
void plan_plain(pq_ctx* ctx, pq_chunk* c, const PVec<DevPage>& pages) {
    c->plain = false;
    c->plain_spec = false;
    c->plain_opt = false;
    c->hpwins.clear();
    c->hpwbase.clear();
    c->hpwpage.clear();
    c->hchunk_base.clear();
    c->hchunks.clear();
    if (c->type != PQ_BYTE_ARRAY || c->max_def < 0 || c->max_rep != 0 || pages.empty()) return;
    // OPTIONAL: the value sections (after the levels) are decoded as
    // REQUIRED-shaped pages of their non-null values; the windows and chunks
    // cover the whole slots, which hold them
    const bool opt = c->max_def > 0;
    bool big = false;
    for (const auto& pg : pages) {
        if (pg.mode != pqk::MODE_PLAIN || pg.nvals < 0) return;
        big |= page_slot(pg) > pqk::kPWin;
    }
    if (!big) plan_plain_windows(c, pages, opt);
    else if (!plan_plain_chunks(c, pages, opt)) return;
    c->plain_opt = opt;
    c->opt_lane_levels = true;
    for (const auto& pg : pages) c->opt_lane_levels &= pg.nvals <= pqk::kOptLaneRows;
    c->plain_grid = ctx->cus * pqk::plain_write_blocks_per_cu();
    c->plain = true;
}

// Decide whether every chunk of the column can take the fused BYTE_ARRAY
// path (dict_fused.hip) and size its LDS carve-up; otherwise the generic
// rows -> scan -> gather path runs.
void plan_fused(pq_ctx* ctx, pq_chunk* c, const PVec<DevPage>& pages,
                const std::vector<DevDict>& dicts) {
    c->fused = false;
    if (!ctx->opt_fused || c->type != PQ_BYTE_ARRAY || c->max_def > 255 || c->max_def < 0 || c->ranges.empty()) return;
    const int cus = ctx->cus;
    const uint32_t kLds = 160 * 1024;
    for (auto& r : c->ranges) {
        int32_t dict_id = -1;
        uint32_t maxn = 0, maxs = 0;
        for (int p = r.p0; p < r.p0 + r.np; p++) {
            const DevPage& pg = pages[p];
            if (pg.mode == pqk::MODE_DICT) {
                if (dict_id >= 0 && pg.dict != dict_id) return;  // several dictionaries in force
                dict_id = pg.dict;
            }
            maxn = std::max(maxn, static_cast<uint32_t>(std::max(pg.nvals, 0)));
            maxs = std::max(maxs, static_cast<uint32_t>(std::max(pg.size, 0)));
        }
        if (maxn > 4096 || maxs > 16384) return;
        r.dict_id = dict_id;
        r.rows_cap = (std::max(maxn, 64u) + 63) / 64 * 64;
        r.stage_bytes = (maxs + 15) / 16 * 16 + 16;
        r.wave_bytes = pqk::fused_wave_bytes(r.rows_cap, r.stage_bytes);
        r.dict_chars_bytes = r.dict_bytes = 0;
        if (dict_id >= 0) {
            const DevDict& d = dicts[dict_id];
            if (d.size > 65536 - 64 || d.nvals < 0 || d.nvals > 65535) return;
            int64_t ecap = dict_entry_cap(d.nvals, d.size);
            r.dict_chars_bytes = (static_cast<uint32_t>(d.size) + 15) / 16 * 16 + 16;
            r.dict_bytes = r.dict_chars_bytes + static_cast<uint32_t>((4 * ecap + 15) / 16 * 16);
        }
        if (r.dict_bytes + r.wave_bytes > kLds) return;
        // producer/writer pairs per workgroup (dict_fused.hip)
        int pairs = static_cast<int>(std::min<uint32_t>(8, (kLds - r.dict_bytes) / r.wave_bytes));
        if (ctx->opt_waves > 0) pairs = std::max(1, std::min(pairs, ctx->opt_waves / 2));
        const int W = 2 * pairs;
        r.waves = W;
        uint32_t lds = r.dict_bytes + static_cast<uint32_t>(pairs) * r.wave_bytes;
        int per_cu = pqk::fused_occupancy_waves(lds, W);
        if (per_cu < 1) per_cu = 1;
        int need = (r.np + pairs - 1) / pairs;
        r.grid = std::max(1, std::min(per_cu * cus, need));
    }
    c->fused = true;
}

// A dictionary page of `size` payload bytes filed in the chunk: its slots in
// the entry table, the largest dictionary.  The caller sets its image offset.
static DevDict add_dict(pq_chunk* c, int32_t size, int32_t nvals) {
    DevDict d{};
    d.size = size;
    d.nvals = nvals;
    d.entry_base = static_cast<int32_t>(c->nentries);
    c->max_dict_bytes = std::max<uint32_t>(c->max_dict_bytes, static_cast<uint32_t>(std::max(size, 0)));
    const int64_t cap = c->type == PQ_BYTE_ARRAY ? dict_entry_cap(nvals, size) : 0;
    c->nentries += std::max<int64_t>(cap, 0);
    return d;
}

// The data page `p` at image offset `at` with `size` payload bytes; dict_dev
// is the device index of its dictionary page (-1: none), which it decodes
// through when its encoding says so.
static DevPage dev_page(const pq_chunk* c, const pq_chunk_desc& desc, const pq_page_desc& p, int64_t at, int32_t size,
                        int64_t row_base, int32_t dict_dev) {
    DevPage d{};
    d.off = static_cast<uint64_t>(at);
    d.size = size;
    d.nvals = p.num_values;
    d.first_row = row_base + p.first_row;
    const bool enc_dict = p.encoding == 2 || p.encoding == 8;
    d.mode = (enc_dict && dict_dev >= 0) ? pqk::MODE_DICT
             : (c->type == PQ_BOOLEAN ? ((desc.ext_flags && p.encoding == 3) ? pqk::MODE_BOOL_RLE : pqk::MODE_BOOL)
                                      : pqk::MODE_PLAIN);
    d.dict = d.mode == pqk::MODE_DICT ? dict_dev : -1;
    return d;
}

// The host page tables of one walk (dictionary and data pages, their image
// slots and copy list) on host threads: per-range counts, then every page
// written at its index.  Same tables as plan_pages_serial, which runs
// instead when a page goes through the codec pass (returns false).
bool plan_pages_parallel(pq_chunk* c, const pq_chunk_desc& desc, const pqfmt::WalkResult& w, bool keep_walk, int hw,
                         UploadPlan& up) {
    const int64_t seq = up.seq;
    const size_t N = w.pages.size();
    const int T = static_cast<int>(std::min<size_t>(static_cast<size_t>(hw), std::max<size_t>(1, N / 16384)));
    const size_t per = (N + static_cast<size_t>(T) - 1) / static_cast<size_t>(T);
    struct Part {
        int64_t nslot = 0, ndata = 0, bytes = 0, rows = 0, payload = 0;
        bool codec = false;
        std::vector<size_t> dicts;
    };
    std::vector<Part> parts(static_cast<size_t>(T));
    pqfmt::parallel_run(T, T, [&](int t) {
        Part& P = parts[static_cast<size_t>(t)];
        const size_t a = static_cast<size_t>(t) * per, b = std::min(N, a + per);
        for (size_t i = a; i < b; i++) {
            const pq_page_desc& p = w.pages[i];
            const bool dict = p.page_type == PQ_DICTIONARY_PAGE, data = p.page_type == PQ_DATA_PAGE;
            if (!dict && !data) continue;
            P.codec |= (p.flags & (PQ_PAGE_COMPRESSED | PQ_PAGE_V2)) != 0;
            P.nslot++;
            P.bytes += slot_bytes(p.payload_size);
            P.payload += p.payload_size;
            if (dict) P.dicts.push_back(i);
            else {
                P.ndata++;
                P.rows += p.num_values;
            }
        }
    });
    for (const auto& P : parts)
        if (P.codec) return false;
    // dictionary pages (few) in walk order: device index, entry base
    std::vector<size_t> dpos;  // walk index of each, ascending
    const int32_t d0 = static_cast<int32_t>(up.hdicts.size());
    for (const auto& P : parts)
        for (size_t i : P.dicts) {
            up.hdicts.push_back(add_dict(c, w.pages[i].payload_size, w.pages[i].num_values));
            c->dict_seq.push_back(seq + static_cast<int64_t>(i));
            dpos.push_back(i);
        }
    auto dict_dev = [&](int64_t walk_idx) -> int32_t {
        auto it = std::lower_bound(dpos.begin(), dpos.end(), static_cast<size_t>(walk_idx));
        return (walk_idx >= 0 && it != dpos.end() && *it == static_cast<size_t>(walk_idx))
                   ? d0 + static_cast<int32_t>(it - dpos.begin())
                   : -1;
    };
    // bases of each range
    std::vector<int64_t> img0(static_cast<size_t>(T)), slot0(static_cast<size_t>(T)), data0(static_cast<size_t>(T));
    int64_t ti = 0, ts = 0, td = 0, rows = 0;
    for (int t = 0; t < T; t++) {
        const Part& P = parts[static_cast<size_t>(t)];
        img0[static_cast<size_t>(t)] = ti;
        slot0[static_cast<size_t>(t)] = ts;
        data0[static_cast<size_t>(t)] = td;
        ti += P.bytes;
        ts += P.nslot;
        td += P.ndata;
        rows += P.rows;
        c->payload_bytes += P.payload;
    }
    const size_t cp0 = up.copies.size(), hp0 = up.hpages.size(), ps0 = c->page_seq.size(), wk0 = c->walked.size();
    up.copies.resize(cp0 + static_cast<size_t>(ts));
    up.copy_size.resize(cp0 + static_cast<size_t>(ts));
    up.hpages.resize(hp0 + static_cast<size_t>(td));
    c->page_seq.resize(ps0 + static_cast<size_t>(td));
    if (keep_walk) c->walked.resize(wk0 + N);
    const int64_t img_base = up.img, rb = up.row_base;
    pqfmt::parallel_run(T, T, [&](int t) {
        const size_t a = static_cast<size_t>(t) * per, b = std::min(N, a + per);
        int64_t at = img_base + img0[static_cast<size_t>(t)];
        size_t si = cp0 + static_cast<size_t>(slot0[static_cast<size_t>(t)]);
        size_t di = hp0 + static_cast<size_t>(data0[static_cast<size_t>(t)]);
        for (size_t i = a; i < b; i++) {
            pq_page_desc p = w.pages[i];
            if (p.page_type == PQ_DICTIONARY_PAGE || p.page_type == PQ_DATA_PAGE) {
                up.copies[si] = {p.payload_offset, at};
                up.copy_size[si] = p.payload_size;
                si++;
                if (p.page_type == PQ_DICTIONARY_PAGE) {
                    up.hdicts[static_cast<size_t>(dict_dev(static_cast<int64_t>(i)))].off = static_cast<uint64_t>(at);
                } else {
                    const int32_t dd = p.dict_page >= 0 ? dict_dev(p.dict_page) : -1;
                    c->page_seq[ps0 + (di - hp0)] = seq + static_cast<int64_t>(i);
                    up.hpages[di++] = dev_page(c, desc, p, at, p.payload_size, rb, dd);
                }
                at += slot_bytes(p.payload_size);
            }
            if (keep_walk) {
                p.first_row += rb;
                c->walked[wk0 + i] = p;
            }
        }
    });
    up.img += ti;
    up.row_base += rows;
    return true;
}

// The same tables page by page, for a walk with pages the codec pass rebuilds
// (compressed or DATA_PAGE_V2): such a page's slot has the size of its
// V1-layout payload, and a codec entry instead of a file offset to copy from.
void plan_pages_serial(pq_chunk* c, const pq_chunk_desc& desc, const pqfmt::WalkResult& w, bool keep_walk,
                       size_t file_len, UploadPlan& up) {
    auto codec_page = [&](const pq_page_desc& p, int32_t* out_len) -> bool {
        if (!(p.flags & (PQ_PAGE_COMPRESSED | PQ_PAGE_V2))) return false;
        const bool v2 = (p.flags & PQ_PAGE_V2) != 0, comp = (p.flags & PQ_PAGE_COMPRESSED) != 0;
        const int64_t lv = v2 ? static_cast<int64_t>(p.v2_def_len) + p.v2_rep_len : 0;
        const int64_t vals = (comp ? static_cast<int64_t>(p.uncompressed_size) : static_cast<int64_t>(p.payload_size)) - lv;
        const int64_t n = vals + (v2 && desc.max_def_level > 0 ? 4 + p.v2_def_len : 0) +
                          (v2 && desc.max_rep_level > 0 ? 4 + p.v2_rep_len : 0);
        if (vals < 0 || n > (1ll << 31) - 64 || p.payload_size < 0)
            throw pqfmt::Error(PQ_ERR_DECOMPRESS, "page header: uncompressed_page_size out of range");
        pqk::CodecEntry e{};
        e.src_len = static_cast<uint32_t>(std::max<int64_t>(0, std::min<int64_t>(p.payload_size, static_cast<int64_t>(file_len) - p.payload_offset)));
        e.out_len = static_cast<uint32_t>(n);
        e.def_len = v2 ? static_cast<uint32_t>(p.v2_def_len) : 0u;
        e.rep_len = v2 ? static_cast<uint32_t>(p.v2_rep_len) : 0u;
        e.codec = comp ? static_cast<uint32_t>((p.flags >> 8) & 0xFF) : 0u;
        e.flags = v2 ? (pqk::kCodecV2 | (desc.max_def_level > 0 ? pqk::kCodecDefPrefix : 0u) |
                        (desc.max_rep_level > 0 ? pqk::kCodecRepPrefix : 0u))
                     : 0u;
        up.cents.push_back(e);
        up.cent_file.push_back(p.payload_offset);
        *out_len = static_cast<int32_t>(n);
        return true;
    };
    auto slot = [&](int64_t file_off, int32_t size) {
        int64_t at = up.img;
        if (!up.cents.empty() && up.cents.back().dst == ~0ull) {  // the codec entry just made
            up.cents.back().dst = static_cast<uint64_t>(at);
            file_off = -1;
        }
        up.copies.push_back({file_off, at});
        up.copy_size.push_back(size);
        up.img += slot_bytes(size);
        return at;
    };
    std::vector<int32_t> dict_of_walk(w.pages.size(), -1);
    int64_t rows = 0;
    for (size_t i = 0; i < w.pages.size(); i++) {
        pq_page_desc p = w.pages[i];
        const int64_t sq = up.seq + static_cast<int64_t>(i);
        int32_t psize = p.payload_size;
        if ((p.page_type == PQ_DICTIONARY_PAGE || p.page_type == PQ_DATA_PAGE) && codec_page(p, &psize))
            up.cents.back().dst = ~0ull;  // placed by slot()
        if (p.page_type == PQ_DICTIONARY_PAGE) {
            DevDict d = add_dict(c, psize, p.num_values);
            d.off = static_cast<uint64_t>(slot(p.payload_offset, psize));
            dict_of_walk[i] = static_cast<int32_t>(up.hdicts.size());
            up.hdicts.push_back(d);
            c->dict_seq.push_back(sq);
            c->payload_bytes += psize;
        } else if (p.page_type == PQ_DATA_PAGE) {
            const int32_t dict_dev = p.dict_page >= 0 ? dict_of_walk[p.dict_page] : -1;
            up.hpages.push_back(dev_page(c, desc, p, slot(p.payload_offset, psize), psize, up.row_base, dict_dev));
            c->page_seq.push_back(sq);
            c->payload_bytes += psize;
            rows += p.num_values;
        }
        p.first_row += up.row_base;
        if (keep_walk) c->walked.push_back(p);
    }
    up.row_base += rows;
}

// The tile tables (up to kTileRows rows of one page each) per page range on
// host threads: tile counts, then the tiles at their indices, with the
// chunk-wide flags reduced per range.
void plan_tiles(pq_chunk* c, int hw, UploadPlan& up) {
    const PVec<DevPage>& hpages = up.hpages;
    const size_t NP = hpages.size();
    const int T = static_cast<int>(std::min<size_t>(static_cast<size_t>(hw), std::max<size_t>(1, NP / 16384)));
    const size_t per = (NP + static_cast<size_t>(T) - 1) / static_cast<size_t>(T);
    struct TPart {
        size_t nt = 0;
        bool aligned = true, plain = true;
        uint32_t maxb = 0;
    };
    std::vector<TPart> tp(static_cast<size_t>(T));
    pqfmt::parallel_run(T, T, [&](int t) {
        TPart& P = tp[static_cast<size_t>(t)];
        for (size_t p = static_cast<size_t>(t) * per; p < std::min(NP, (static_cast<size_t>(t) + 1) * per); p++) {
            P.nt += static_cast<size_t>((std::max(hpages[p].nvals, 0) + pqk::kTileRows - 1) / pqk::kTileRows);
            P.maxb = std::max<uint32_t>(P.maxb, static_cast<uint32_t>(std::max(hpages[p].size, 0)));
            P.plain &= hpages[p].mode == pqk::MODE_PLAIN;
        }
    });
    std::vector<size_t> tb(static_cast<size_t>(T));
    size_t nt = 0;
    for (int t = 0; t < T; t++) {
        tb[static_cast<size_t>(t)] = nt;
        nt += tp[static_cast<size_t>(t)].nt;
    }
    up.htiles.resize(nt);
    up.tile0.resize(NP);
    pqfmt::parallel_run(T, T, [&](int t) {
        TPart& P = tp[static_cast<size_t>(t)];
        size_t k = tb[static_cast<size_t>(t)];
        for (size_t p = static_cast<size_t>(t) * per; p < std::min(NP, (static_cast<size_t>(t) + 1) * per); p++) {
            up.tile0[p] = static_cast<int32_t>(k);
            const DevPage& pg = hpages[p];
            for (int32_t r = 0; r < pg.nvals; r += pqk::kTileRows) {
                up.htiles[k++] = DevTile{static_cast<int32_t>(p), r, std::min(pqk::kTileRows, pg.nvals - r), 0};
                P.aligned &= ((pg.first_row + r) & 31) == 0;
            }
        }
    });
    c->ntiles = static_cast<int>(nt);
    c->tiles_aligned32 = true;
    // every data page PLAIN, a fixed-width type whose bytes are copied as is
    c->fixed_plain = (c->type == PQ_INT32 || c->type == PQ_INT64 || c->type == PQ_FLOAT ||
                      c->type == PQ_DOUBLE || c->type == PQ_INT96) &&
                     c->width == c->plain_width && c->max_def >= 0 && c->max_rep >= 0;
    for (const auto& P : tp) {
        c->tiles_aligned32 &= P.aligned;
        c->max_page_bytes = std::max(c->max_page_bytes, P.maxb);
        c->fixed_plain &= P.plain;
    }
}

// Windows of consecutive pages for the windowed PLAIN regex kernel (regex.hip
// k_regex_plain): <= 64 pages and <= win bytes of image each.  False when a
// page does not fit (the lane-per-page kernel runs then).
bool plan_regex_windows(pq_ctx* ctx, pq_chunk* c) {
    if (c->d_rwins && c->rwin_for_dfa == c->dfa_bytes && c->rwin_opt == ctx->opt_regex_win) return true;
    const uint32_t maxslot = c->npages ? static_cast<uint32_t>(slot_bytes(c->max_page_bytes)) : 0u;
    const uint32_t win = std::max<uint32_t>(static_cast<uint32_t>(ctx->opt_regex_win), maxslot);
    // the kernel lists strings by u16 window offsets (and the string index
    // keeps them): pages whose slot leaves no room take k_regex_lanes
    if (win + 32 > 65535u) return false;
    if (pqre::regex_plain_waves(c->dfa_bytes, win) == 0) return false;
    const uint32_t lds = pqre::regex_plain_lds(c->dfa_bytes, win);
    if (lds > 160 * 1024) return false;
    c->hrwins.clear();
    // the PLAIN decode's windows are the same kind (<= 64 consecutive page
    // slots, <= kPWin bytes; planned on host threads at upload): no page
    // table read back
    const bool same = c->plain && !c->plain_spec && win == pqk::kPWin && !c->hpwins.empty();
    std::vector<DevPage> hp(same ? 0 : static_cast<size_t>(c->npages));
    if (same) c->hrwins = c->hpwins;
    else if (c->npages && hipMemcpy(hp.data(), c->d_pages, hp.size() * sizeof(DevPage), hipMemcpyDeviceToHost) != hipSuccess)
        return false;
    int64_t chars = 0;  // (not used by the scan)
    bool known = true;
    for (size_t p = 0; p < hp.size(); p += static_cast<size_t>(c->hrwins.back().np))
        c->hrwins.push_back(page_window(hp.data(), p, hp.size(), win, &chars, &known));
    dfree(c->d_rwins);
    if (!c->d_rwin_ticket && dalloc(&c->d_rwin_ticket, 1)) return false;
    if (dalloc(&c->d_rwins, std::max<size_t>(c->hrwins.size(), 1))) return false;
    if (!c->hrwins.empty() &&
        hipMemcpy(c->d_rwins, c->hrwins.data(), c->hrwins.size() * sizeof(pqk::DevBatch), hipMemcpyHostToDevice) != hipSuccess)
        return false;
    const int cus = ctx->cus;
    const int per_cu = std::max(1, pqre::regex_plain_occupancy(lds));
    c->rwin_bytes = win;
    c->rwin_for_dfa = c->dfa_bytes;
    c->rwin_opt = ctx->opt_regex_win;
    const int scan = static_cast<int>(pqre::regex_plain_waves(c->dfa_bytes, win));  // waves per workgroup
    c->rwin_grid = std::max(1, std::min<int>(per_cu * cus, static_cast<int>((c->hrwins.size() + scan - 1) / scan)));
    return true;
}
}  // namespace pqcapi
