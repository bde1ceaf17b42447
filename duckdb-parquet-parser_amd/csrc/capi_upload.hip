// capi_upload.hip — the upload side of the C ABI (include/pq_gpu.h): the page
// walk runs on the CPU (pqfmt) or the GPU (walk.hip), page bytes are uploaded
// to HBM once per chunk, and upload_walked builds the device chunk in named
// stages over one UploadPlan.  No C++ exception crosses an extern "C" function.
#include <cstdio>
#include <cstdlib>

#include "host/capi_util.hpp"

namespace pqcapi __attribute__((visibility("hidden"))) {

// ── the chunk's device memory: alloc_chunk_device and free_chunk_device list
// the same pointers in the same order (the regex scans add theirs later) ──
static int alloc_chunk_device(pq_chunk* c, const UploadPlan& up) {
    const size_t np = up.hpages.size(), nd = up.hdicts.size(), nt = up.htiles.size();
    int rc = 0;
    rc |= dalloc(&c->d_bytes, c->nbytes); rc |= dalloc(&c->d_pages, np); rc |= dalloc(&c->d_dicts, nd);
    rc |= dalloc(&c->d_tiles, nt); rc |= dalloc(&c->d_page_tile0, up.tile0.size());
    rc |= dalloc(&c->d_entries, static_cast<size_t>(c->nentries)); rc |= dalloc(&c->d_dict_count, nd);
    rc |= dalloc(&c->d_page_err, np); rc |= dalloc(&c->d_dict_err, nd);
    if (c->pipe) {  // flags | bsum | flist, cleared together
        // (bsum: pipe_grid k_pipe_write workgroup sums)
        const size_t fb = 4 * sizeof(int32_t), bb = static_cast<size_t>(c->pipe_grid) * sizeof(unsigned long long);
        c->z_bsum = fb;
        c->z_flist = (fb + bb + 15) / 16 * 16;
        // cleared per decode (through flist[0]): a multiple of 16 bytes (an
        // odd size takes a second fill kernel for the tail)
        const size_t zb = (c->z_flist + sizeof(int32_t) + 15) / 16 * 16;
        // two such blocks: a decode uses one while its k_pipe_write clears
        // the other for the next decode (no fill kernel per decode)
        const size_t zfull = (std::max(zb, c->z_flist + (np + 1) * sizeof(int32_t)) + 255) / 256 * 256;
        rc |= dalloc(&c->d_zero, 2 * zfull);
        if (c->d_zero) {
            c->zfull = zfull;
            c->zsel = 0;
            c->d_flags = reinterpret_cast<int32_t*>(c->d_zero);
            c->d_bsum = reinterpret_cast<unsigned long long*>(c->d_zero + c->z_bsum);
            c->d_flist = reinterpret_cast<int32_t*>(c->d_zero + c->z_flist);
            c->zero_bytes = zb;
        }
    } else {
        rc |= dalloc(&c->d_flags, 4);
    }
    if (c->pipe && nd) rc |= dalloc(&c->d_dflag, 1);
    {
        size_t off = 0;
        for (size_t i = 0; i < nd; i++) {
            const uint32_t sz = static_cast<uint32_t>(std::max(up.hdicts[i].size, 0));
            if (static_cast<uint64_t>(sz) + 32 <= pqk::kDictLdsCap) continue;
            pq_chunk::BigDict b{static_cast<int>(i), up.hdicts[i], off, 0, 0};
            off += (pqk::dict_big_scratch(sz) + 255) / 256 * 256;
            const size_t nv = static_cast<size_t>(dict_entry_cap(std::max(up.hdicts[i].nvals, 0), sz));
            b.lens_off = off;  // entry lengths as bytes (+ 16: k_wide_chars stages whole blocks)
            off += (nv + 16 + 255) / 256 * 256;
            b.pad_off = off;   // 16-byte entry slots (k_pipe_wwide)
            off += (nv * 16 + 255) / 256 * 256;
            c->hbigd.push_back(b);
        }
        if (off) rc |= dalloc(&c->d_bigd, off);
    }
    rc |= dalloc(&c->d_tile_chars, nt);
    if (c->fixed_plain || c->plain_opt) {
        rc |= dalloc(&c->d_tile_rank, nt);
        rc |= dalloc(&c->d_page_pos, np);
    }
    if (c->plain_opt) {
        rc |= dalloc(&c->d_page_nn, np); rc |= dalloc(&c->d_onnv, np); rc |= dalloc(&c->d_ochv, np);
        rc |= dalloc(&c->d_opdense, np); rc |= dalloc(&c->d_opbase, np); rc |= dalloc(&c->d_otot, 2);
        rc |= dalloc(&c->d_vpages, np); rc |= dalloc(&c->d_doffs, static_cast<size_t>(c->nrows) + 1);
        rc |= dalloc(&c->d_operr, np);
        if (!c->hpwpage.empty()) rc |= dalloc(&c->d_pwpage, c->hpwpage.size());
    }
    rc |= dalloc(&c->d_tile_base, nt); rc |= dalloc(&c->d_total, 1);
    rc |= dalloc(&c->d_scan_scratch, std::max(nt, np) / 8192 + 16);
    if (c->type == PQ_BYTE_ARRAY && !c->fused) rc |= dalloc(&c->d_row_codes, static_cast<size_t>(c->nrows));
    if (c->pipe) {
        rc |= dalloc(&c->d_runs, np * 2 * pqk::kPipeRunCap); rc |= dalloc(&c->d_info, np);
        // u16 codes, or u32 on the wide pipe (d_codes then holds 2 per row)
        rc |= dalloc(&c->d_codes, static_cast<size_t>(c->nrows) * (c->pipe_wide ? 2 : 1) + 64);
        rc |= dalloc(&c->d_tile_nn, nt);
        if (!c->hbig.empty()) rc |= dalloc(&c->d_bigp, c->hbig.size());
    }
    if (c->plain) {
        rc |= dalloc(&c->d_pwins, c->hpwins.size());
        if (!c->hpwbase.empty()) rc |= dalloc(&c->d_pwbase, c->hpwbase.size());
        rc |= dalloc(&c->d_rowinfo, static_cast<size_t>(c->nrows) + 64); rc |= dalloc(&c->d_wchars, c->hpwins.size());
        rc |= dalloc(&c->d_pbsum, static_cast<size_t>(c->plain_grid));
        if (c->plain_spec) {
            const size_t nch = c->hchunks.size();
            rc |= dalloc(&c->d_chunk_base, c->hchunk_base.size()); rc |= dalloc(&c->d_chunks, nch);
            rc |= dalloc(&c->d_cand, nch * pqk::kPCand); rc |= dalloc(&c->d_ppages, nch); rc |= dalloc(&c->d_perr, nch);
        }
    }
    if (c->fused) {
        rc |= dalloc(&c->d_status, np); rc |= dalloc(&c->d_tickets, c->ranges.size());
        rc |= dalloc(&c->d_bases, c->ranges.size() + 1);
    }
    return rc;
}

void free_chunk_device(pq_chunk* c) {
    dfree(c->d_bytes); dfree(c->d_pages); dfree(c->d_dicts); dfree(c->d_tiles); dfree(c->d_page_tile0);
    dfree(c->d_entries); dfree(c->d_dict_count); dfree(c->d_page_err); dfree(c->d_dict_err);
    if (c->d_zero) {  // d_flags, d_bsum and d_flist live in it
        dfree(c->d_zero);
        c->d_flags = nullptr;
        c->d_bsum = nullptr;
        c->d_flist = nullptr;
    }
    dfree(c->d_flags);
    dfree(c->d_dflag);
    dfree(c->d_bigd);
    dfree(c->d_tile_chars); dfree(c->d_tile_rank); dfree(c->d_page_pos);
    // plain_opt
    dfree(c->d_page_nn); dfree(c->d_onnv); dfree(c->d_ochv); dfree(c->d_opdense); dfree(c->d_opbase);
    dfree(c->d_otot); dfree(c->d_vpages); dfree(c->d_doffs); dfree(c->d_operr); dfree(c->d_pwpage);
    dfree(c->d_tile_base); dfree(c->d_total); dfree(c->d_scan_scratch); dfree(c->d_row_codes);
    // pipe
    dfree(c->d_runs); dfree(c->d_info); dfree(c->d_codes); dfree(c->d_tile_nn); dfree(c->d_bigp);
    // plain, plain_spec
    dfree(c->d_pwins); dfree(c->d_pwbase); dfree(c->d_rowinfo); dfree(c->d_wchars); dfree(c->d_pbsum);
    dfree(c->d_chunk_base); dfree(c->d_chunks); dfree(c->d_cand); dfree(c->d_ppages); dfree(c->d_perr);
    // fused
    dfree(c->d_status); dfree(c->d_tickets); dfree(c->d_bases);
    // the regex scans' (capi_regex.hip regex_prepare, plan.cpp plan_regex_windows)
    dfree(c->d_rx_index); dfree(c->d_page_flags); dfree(c->d_dict_match); dfree(c->d_dfa);
    dfree(c->d_rwins); dfree(c->d_rwin_ticket);
    if (c->d_prog) { pqre::free_device_program(c->d_prog); c->d_prog = nullptr; }
}

// The device walk (walk.hip) of one chunk over d_bytes = file bytes
// [base, base + len): the page table to `host` (pinned staging, then `sink`)
// and the page count.  PQ_ERR_UNSUPPORTED: refused (the host walk decides).
template <class Sink>
static int device_walk(pq_ctx* ctx, const uint8_t* d_bytes, size_t len, int64_t base, const pq_chunk_desc* chunk,
                       int64_t seg_bytes, int64_t rec_cap, int64_t* npages, Sink&& sink) {
    *npages = 0;
    if (chunk->codec != 0 || chunk->ext_flags != 0 || chunk->num_values <= 0) return PQ_ERR_UNSUPPORTED;
    int64_t off = chunk->data_page_offset;
    if (chunk->has_dictionary_page_offset) off = std::min(off, chunk->dictionary_page_offset);
    if (off < base || off >= base + static_cast<int64_t>(len)) return PQ_ERR_UNSUPPORTED;
    const uint64_t seg = seg_bytes ? static_cast<uint64_t>(seg_bytes) : 8192u;
    if (seg > (1u << 30) || rec_cap < 0 || rec_cap > (int64_t{1} << 20)) return PQ_ERR_UNSUPPORTED;
    const uint32_t rc = static_cast<uint32_t>(rec_cap ? rec_cap : std::max<int64_t>(1, static_cast<int64_t>(seg) / 128));
    const uint64_t start = static_cast<uint64_t>(off), end = static_cast<uint64_t>(base) + len;
    const uint64_t nseg64 = (end - start + seg - 1) / seg;
    if (nseg64 > (1u << 30) / rc) return PQ_ERR_UNSUPPORTED;
    const uint32_t nseg = static_cast<uint32_t>(nseg64);
    pqk::WalkLaunch W{};
    W.bytes = d_bytes; W.base = static_cast<uint64_t>(base); W.len = len;
    W.start = start; W.end = end; W.seg = seg; W.nseg = nseg; W.cap = rc;
    W.num_values = chunk->num_values;
    const size_t nrec = static_cast<size_t>(nseg) * rc;
    // one device buffer, kept by the context: records, segments, links, bases, the page table
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t o_recs = 0, o_segs = o_recs + al(nrec * sizeof(pqk::WalkRec));
    const size_t o_links = o_segs + al(nseg * pqk::walk_seg_bytes());
    const size_t o_bases = o_links + al(nseg * pqk::walk_link_bytes());
    const size_t o_out = o_bases + al(3 * static_cast<size_t>(nseg) * 8);
    const size_t o_pages = o_out + 256, total = o_pages + al(nrec * sizeof(pq_page_desc));
    if (ctx->walk_cap < total) {
        if (ctx->d_walk) (void)hipFree(ctx->d_walk);
        ctx->d_walk = nullptr;
        ctx->walk_cap = 0;
        if (int e = hip_check(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->d_walk), total), "hipMalloc (device walk)")) return e;
        ctx->walk_cap = total;
    }
    uint8_t* mem = ctx->d_walk;
    W.recs = reinterpret_cast<pqk::WalkRec*>(mem + o_recs);
    W.segs = mem + o_segs;
    W.links = mem + o_links;
    W.base_pg = reinterpret_cast<int64_t*>(mem + o_bases);
    W.base_val = W.base_pg + nseg;
    W.dict_in = W.base_val + nseg;
    W.out = reinterpret_cast<int64_t*>(mem + o_out);
    W.pages = reinterpret_cast<pq_page_desc*>(mem + o_pages);
    {
        Timed t(ctx, "walk");
        pqk::launch_walk(ctx->stream, W);
    }
    int64_t res[8] = {-1, -1, 0, 0, 0, 0, 0, 0};
    int rc2 = hip_check(ctx, hipGetLastError(), "walk launch");
    if (!rc2) rc2 = hip_check(ctx, hipMemcpyAsync(res, W.out, sizeof res, hipMemcpyDeviceToHost, ctx->stream), "walk result");
    if (!rc2) rc2 = hip_check(ctx, hipStreamSynchronize(ctx->stream), "walk sync");
    if (std::getenv("PQ_WALK_DEBUG"))
        std::fprintf(stderr, "walk: pages %lld cut %lld entry %lld n %lld exit %lld bad %lld prev_exit %lld first %lld (start %llu seg %llu)\n",
                     (long long)res[0], (long long)res[1], (long long)res[2], (long long)res[3], (long long)res[4],
                     (long long)res[5], (long long)res[6], (long long)res[7], (unsigned long long)start,
                     (unsigned long long)seg);
    if (rc2) return rc2;
    if (res[0] < 0) return PQ_ERR_UNSUPPORTED;
    *npages = res[0];
    const size_t k = static_cast<size_t>(res[0]);
    if (k) {
        if (ctx->h_walk_cap < k) {
            if (ctx->h_walk) (void)hipHostFree(ctx->h_walk);
            ctx->h_walk = nullptr;
            ctx->h_walk_cap = 0;
            if (int e = hip_check(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->h_walk), k * sizeof(pq_page_desc)),
                                  "hipHostMalloc (device walk)"))
                return e;
            ctx->h_walk_cap = k;
        }
        if (int e = hip_check(ctx, hipMemcpyAsync(ctx->h_walk, W.pages, k * sizeof(pq_page_desc), hipMemcpyDeviceToHost,
                                                  ctx->stream), "walk copy"))
            return e;
        if (int e = hip_check(ctx, hipStreamSynchronize(ctx->stream), "walk copy sync")) return e;
    }
    sink(ctx->h_walk, k);
    return 0;
}

// Bytes [a, z) of a staged buffer into dst.  The buffer holds n pieces in
// ascending order, piece(k) = {offset in the buffer, bytes, file offset they
// come from}; everything between and after the pieces is zero.
struct Piece {
    size_t at, len;
    int64_t src;
};
template <class PieceFn>
static void fill_pieces(const uint8_t* file, size_t n, PieceFn piece, uint8_t* dst, size_t a, size_t z) {
    size_t lo = 0, hi = n;  // the first piece that starts after a
    while (lo < hi) {
        const size_t m = (lo + hi) / 2;
        if (piece(m).at <= a) lo = m + 1;
        else hi = m;
    }
    size_t at = a;
    for (size_t k = lo ? lo - 1 : 0; k < n && at < z; k++) {
        const Piece p = piece(k);
        if (p.at > at) {
            const size_t g = std::min(z, p.at) - at;
            std::memset(dst + (at - a), 0, g);
            at += g;
        }
        const size_t e = std::min(z, p.at + p.len);
        if (at < e) {
            std::memcpy(dst + (at - a), file + p.src + (at - p.at), e - at);
            at = e;
        }
    }
    if (at < z) std::memset(dst + (at - a), 0, z - at);
}

// Bytes of an n-byte payload at file offset lo that the file holds (lo < 0: a
// codec page, nothing to copy).
static int64_t payload_avail(int64_t lo, int64_t n, size_t file_len) {
    return lo < 0 ? 0 : std::max<int64_t>(0, std::min<int64_t>(n, static_cast<int64_t>(file_len) - lo));
}

namespace {
// Raw path of an upload: the chunk's byte extents, exactly
// as the file holds them, go to HBM (ctx->d_raw) through the pinned ring on a
// host thread that starts before the page walk, so the H2D overlaps the walk
// and the planning; a GPU pass (k_relayout) then builds the slot image.
struct RawStage {
    std::vector<std::pair<int64_t, int64_t>> ext;  // (file offset, bytes), in d_raw order
    std::vector<int64_t> base;                     // d_raw offset of each extent
    int64_t total = 0;
    std::thread th;
    hipError_t err = hipSuccess;
    bool active = false;
    void join() {
        if (th.joinable()) th.join();
    }
    ~RawStage() { join(); }
    // d_raw offset of file bytes [lo, lo + n): the extent that holds them,
    // tried first at `hint` (extents and payloads both ascend, mostly)
    bool locate(int64_t lo, int64_t n, size_t& hint, uint64_t* src) const {
        auto in = [&](size_t j) { return lo >= ext[j].first && lo + n <= ext[j].first + ext[j].second; };
        if (!in(hint)) {
            size_t j = 0;
            while (j < ext.size() && !in(j)) j++;
            if (j == ext.size()) return false;
            hint = j;
        }
        *src = static_cast<uint64_t>(base[hint] + (lo - ext[hint].first));
        return true;
    }
};
}  // namespace

static void raw_start(pq_ctx* ctx, const uint8_t* file, size_t file_len, RawStage& R) {
    R.active = false;
    if (!ctx->opt_raw || R.ext.empty()) return;
    R.total = 0;
    R.base.clear();
    for (auto& e : R.ext) {
        e.first = std::max<int64_t>(0, e.first);
        e.second = std::max<int64_t>(0, std::min<int64_t>(e.second, static_cast<int64_t>(file_len) - e.first));
        R.base.push_back(R.total);
        R.total += (e.second + 15) / 16 * 16;  // each extent 16-byte aligned in d_raw
    }
    if (R.total <= 0) return;
    if (!dgrow(ctx->d_raw, ctx->raw_cap, static_cast<size_t>(R.total) + 64)) return;
    R.active = true;
    const int hw = host_threads();
    R.th = std::thread([ctx, file, &R, hw]() {
        (void)hipSetDevice(ctx->device);  // a new host thread starts on device 0
        auto extent = [&R](size_t k) {
            return Piece{static_cast<size_t>(R.base[k]), static_cast<size_t>(R.ext[k].second), R.ext[k].first};
        };
        auto fill = [&](uint8_t* dst, size_t a, size_t z) { fill_pieces(file, R.ext.size(), extent, dst, a, z); };
        R.err = ctx->stager.upload(ctx->d_raw, static_cast<size_t>(R.total), ctx->copy, hw, fill,
                                   ctx->opt_stage_streams > 1 ? ctx->copy2 : nullptr);
    });
}

// ── the stages of upload_walked ─────────────────────────────────────────────

// 1) The page tables of every walk: each payload gets a 16-byte aligned slot
// in one image.  A later chunk is not planned after a walk error (the
// reference never reaches it).
static void plan_pages(pq_chunk* c, const pq_chunk_desc& desc, std::vector<pqfmt::WalkResult>& walks, size_t file_len,
                       UploadPlan& up) {
    const bool many = walks.size() > 1;
    up.hpages.clear();
    up.copies.clear();
    up.copy_size.clear();
    size_t tot = 0;
    for (const auto& w : walks) tot += w.pages.size();
    up.hpages.reserve(tot);
    up.copies.reserve(tot);
    up.copy_size.reserve(tot);
    if (many) c->walked.reserve(tot);
    c->page_seq.reserve(tot);
    for (pqfmt::WalkResult& w : walks) {
        pq_chunk::Range rg;
        rg.p0 = static_cast<int32_t>(up.hpages.size());
        if (!plan_pages_parallel(c, desc, w, many, host_threads(), up)) plan_pages_serial(c, desc, w, many, file_len, up);
        rg.np = static_cast<int32_t>(up.hpages.size()) - rg.p0;
        c->ranges.push_back(rg);
        up.seq += static_cast<int64_t>(w.pages.size());
        if (w.error) {
            c->walk_error = w.error;
            c->walk_message = w.message;
            c->walk_error_seq = up.seq;
            break;
        }
    }
    if (!many) c->walked = std::move(walks[0].pages);  // rows start at 0: the walk's table as is
    c->nrows = up.row_base;
    c->nbytes = static_cast<size_t>(up.img) + 64;
}

// The relayout entries (d_raw offset -> slot) of every payload, on host
// threads.  False: a payload lies outside the raw extents.
static bool relayout_entries(const RawStage& raw, size_t file_len, UploadPlan& up) {
    up.ents.resize(up.copies.size());
    std::atomic<bool> inside_all{true};
    const size_t NC = up.copies.size();
    const int T = static_cast<int>(std::min<size_t>(static_cast<size_t>(host_threads()), std::max<size_t>(1, NC / 16384)));
    const size_t per = (NC + static_cast<size_t>(T) - 1) / static_cast<size_t>(T);
    pqfmt::parallel_run(T, T, [&](int t) {
        size_t e = 0;
        for (size_t k = static_cast<size_t>(t) * per; k < std::min(NC, (static_cast<size_t>(t) + 1) * per); k++) {
            const int64_t lo = up.copies[k].first, n = up.copy_size[k], avail = payload_avail(lo, n, file_len);
            pqk::RelayoutEntry r{};
            r.dst = static_cast<uint64_t>(up.copies[k].second);
            r.avail = static_cast<uint32_t>(avail);
            r.slot = static_cast<uint32_t>(slot_bytes(n));
            if (avail > 0 && !raw.locate(lo, avail, e, &r.src)) {
                inside_all = false;
                return;
            }
            up.ents[k] = r;
        }
    });
    return inside_all;
}

// 4) The image into c->d_bytes: by k_relayout from the raw bytes the side
// thread put in HBM (returns true), else filled piece by piece straight into
// pinned buffers by host threads while earlier pieces are in flight.
static bool upload_image(pq_ctx* ctx, pq_chunk* c, const uint8_t* file, size_t file_len, RawStage* raw, UploadPlan& up,
                         int* rc) {
    hipStream_t s = ctx->copy;
    bool relaid = false;
    if (raw && raw->active) {
        raw->join();  // the raw bytes are in HBM (the ring is free again)
        if (raw->err != hipSuccess) {
            *rc = hip_check(ctx, raw->err, "raw upload");
        } else if (relayout_entries(*raw, file_len, up)) {
            if (dgrow(ctx->d_relay, ctx->relay_cap, std::max<size_t>(up.ents.size(), 1))) {
                *rc = hip_check(ctx, hipMemcpyAsync(ctx->d_relay, up.ents.data(), up.ents.size() * sizeof(pqk::RelayoutEntry),
                                                    hipMemcpyHostToDevice, s),
                                "upload");
                if (!*rc) {
                    {
                        Timed rt(ctx, "relayout", s);
                        pqk::launch_relayout(s, ctx->d_raw, c->d_bytes, ctx->d_relay, static_cast<int32_t>(up.ents.size()));
                    }
                    (void)hipMemsetAsync(c->d_bytes + up.img, 0, c->nbytes - static_cast<size_t>(up.img), s);
                    relaid = true;
                }
            }
        }
    }
    if (*rc || relaid) return relaid;
    // payload k in its slot: the bytes the file holds, the rest of the slot
    // zero (a codec page: all zero until the codec pass)
    auto payload = [&](size_t k) {
        const int64_t lo = up.copies[k].first;
        return Piece{static_cast<size_t>(up.copies[k].second), static_cast<size_t>(payload_avail(lo, up.copy_size[k], file_len)), lo};
    };
    const size_t n = up.copies.size();
    *rc = hip_check(ctx, ctx->stager.upload(c->d_bytes, c->nbytes, s, n > 64 ? host_threads() : 1,
                                            [&](uint8_t* dst, size_t a, size_t z) { fill_pieces(file, n, payload, dst, a, z); },
                                            ctx->opt_stage_streams > 1 ? ctx->copy2 : nullptr),
                    "upload");
    return false;
}

// 5) Compressed / DATA_PAGE_V2 pages: their payloads (in
// d_raw when `raw` holds this upload's bytes, else gathered and uploaded) are
// rebuilt into their slots by the codec pass (codec.hip).
static int run_codec_pass(pq_ctx* ctx, pq_chunk* c, const uint8_t* file, const RawStage* raw, UploadPlan& up) {
    hipStream_t s = ctx->copy;
    auto& cents = up.cents;
    const size_t n = cents.size();
    int rc = 0;
    bool in_raw = raw != nullptr;
    for (size_t k = 0, e = 0; k < n && in_raw; k++) in_raw = raw->locate(up.cent_file[k], cents[k].src_len, e, &cents[k].src);
    if (!in_raw) {  // gather the payloads, each 16-byte aligned
        std::vector<int64_t> at(n);
        int64_t tot = 0;
        for (size_t k = 0; k < n; k++) {
            at[k] = tot;
            cents[k].src = static_cast<uint64_t>(tot);
            tot += (static_cast<int64_t>(cents[k].src_len) + 15) / 16 * 16;
        }
        const size_t need = static_cast<size_t>(tot) + 64;
        auto gathered = [&](size_t k) { return Piece{static_cast<size_t>(at[k]), cents[k].src_len, up.cent_file[k]}; };
        if (!dgrow(ctx->d_zsrc, ctx->zsrc_cap, need)) rc = set_err(ctx, PQ_ERR_HIP, "hipMalloc failed (compressed pages)");
        if (!rc)
            rc = hip_check(ctx, ctx->stager.upload(ctx->d_zsrc, need, s, n > 64 ? host_threads() : 1,
                                                   [&](uint8_t* dst, size_t a, size_t z) { fill_pieces(file, n, gathered, dst, a, z); }),
                           "upload");
    }
    const uint8_t* csrc = in_raw ? ctx->d_raw : ctx->d_zsrc;
    if (!rc && ctx->codec_cap < n) {
        dfree(ctx->d_codec);
        dfree(ctx->d_codec_st);
        ctx->codec_cap = 0;
        if (dalloc(&ctx->d_codec, n) == 0 && dalloc(&ctx->d_codec_st, n) == 0) ctx->codec_cap = n;
        else rc = set_err(ctx, PQ_ERR_HIP, "hipMalloc failed (compressed pages)");
    }
    if (!rc)
        rc = hip_check(ctx, ctx->stager.upload(reinterpret_cast<uint8_t*>(ctx->d_codec), n * sizeof(pqk::CodecEntry), s, 1,
                                               [&](uint8_t* dst, size_t a, size_t z) {
                                                   std::memcpy(dst, reinterpret_cast<const uint8_t*>(cents.data()) + a, z - a);
                                               }),
                       "upload");
    // every status word starts non-OK: an entry the pass never reached (a
    // failed launch) cannot read as a clean decode
    if (!rc) rc = hip_check(ctx, hipMemsetAsync(ctx->d_codec_st, 0xFF, n * sizeof(uint32_t), s), "codec status");
    if (rc) return rc;
    Timed ct(ctx, "codec", s);
    auto any = [&](auto pred) { return std::any_of(cents.begin(), cents.end(), pred); };
    const bool gz = any([](const pqk::CodecEntry& e) { return e.codec == 2; });
    const bool other = any([](const pqk::CodecEntry& e) { return e.codec != 2 && e.codec != 0; });
    const bool zstd = any([](const pqk::CodecEntry& e) { return e.codec == 6; });
    const bool zother = any([](const pqk::CodecEntry& e) { return e.codec != 6 && e.codec != 0; });
    if (gz && other) return set_err(ctx, PQ_ERR_CODEC, "GZIP pages mixed with other codecs in one upload");
    if (zstd && zother) return set_err(ctx, PQ_ERR_CODEC, "ZSTD pages mixed with other codecs in one upload");
    const int32_t nsmall = static_cast<int32_t>(std::count_if(
        cents.begin(), cents.end(), [](const pqk::CodecEntry& e) { return e.out_len < pqk::codec_small_bytes(); }));
    pqk::launch_codec(s, csrc, c->d_bytes, ctx->d_codec, static_cast<int32_t>(n), ctx->d_codec_st, ctx->cus,
                      gz ? 1 : (zstd ? 2 : 0), nsmall);
    return hip_check(ctx, hipGetLastError(), "codec launch");
}

// ... and its status words, read back once the upload stream has synchronised.
static int codec_status(pq_ctx* ctx, const UploadPlan& up) {
    std::vector<uint32_t> st(up.cents.size());
    int rc = hip_check(ctx, hipMemcpy(st.data(), ctx->d_codec_st, st.size() * sizeof(uint32_t), hipMemcpyDeviceToHost),
                       "codec status");
    for (size_t k = 0; k < st.size() && !rc; k++) {
        if (!st[k]) continue;
        static const char* what[] = {"", "corrupt compressed data", "decompressed size differs from the page header",
                                     "unsupported codec", "decompression pass did not run"};
        rc = set_err(ctx, PQ_ERR_DECOMPRESS,
                     "page at file offset " + std::to_string(up.cent_file[k]) + " (codec " +
                         std::to_string(up.cents[k].codec) + "): " + what[std::min<uint32_t>(st[k], 4)]);
    }
    return rc;
}

// 6) The host tables into the chunk's device memory, the error records and
// flag blocks cleared, then the upload stream synchronised: also after an
// error (rc != 0 on entry skips the copies), as the pinned tables may still
// be in flight.
static int upload_tables(pq_ctx* ctx, pq_chunk* c, const UploadPlan& up, int rc) {
    hipStream_t s = ctx->copy;
    auto put = [&](void* d, const void* h, size_t bytes) {
        if (rc || bytes == 0) return;
        rc = hip_check(ctx, ctx->stager.upload(static_cast<uint8_t*>(d), bytes, s, bytes > (32u << 20) ? host_threads() : 1,
                                               [&](uint8_t* dst, size_t a, size_t z) {
                                                   std::memcpy(dst, static_cast<const uint8_t*>(h) + a, z - a);
                                               }),
                       "upload");
    };
    auto put_pinned = [&](void* d, const void* h, size_t bytes) {
        if (rc || bytes == 0) return;
        rc = hip_check(ctx, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s), "upload");
    };
    put_pinned(c->d_pages, up.hpages.data(), up.hpages.size() * sizeof(DevPage));
    put(c->d_dicts, up.hdicts.data(), up.hdicts.size() * sizeof(DevDict));
    put_pinned(c->d_tiles, up.htiles.data(), up.htiles.size() * sizeof(DevTile));
    put_pinned(c->d_page_tile0, up.tile0.data(), up.tile0.size() * sizeof(int32_t));
    if (!rc) (void)hipMemsetAsync(c->d_page_err, 0, std::max<size_t>(up.hpages.size(), 1) * sizeof(DevErr), s);
    if (!rc) (void)hipMemsetAsync(c->d_dict_err, 0, std::max<size_t>(up.hdicts.size(), 1) * sizeof(DevErr), s);
    if (!rc && c->d_dflag) (void)hipMemsetAsync(c->d_dflag, 0, sizeof(int32_t), s);
    if (!rc && c->d_zero) {
        (void)hipMemsetAsync(c->d_zero, 0, 2 * c->zfull, s);
        c->next_zeroed = true;
    }
    if (!rc && c->d_chunks) {
        put(c->d_chunks, c->hchunks.data(), c->hchunks.size() * sizeof(uint2));
        put(c->d_chunk_base, c->hchunk_base.data(), c->hchunk_base.size() * sizeof(int32_t));
        if (!rc) (void)hipMemsetAsync(c->d_perr, 0, c->hchunks.size() * sizeof(DevErr), s);
    }
    if (c->d_bigp) put(c->d_bigp, c->hbig.data(), c->hbig.size() * sizeof(int32_t));
    if (c->d_pwins) put(c->d_pwins, c->hpwins.data(), c->hpwins.size() * sizeof(pqk::DevBatch));
    if (c->d_pwbase) put(c->d_pwbase, c->hpwbase.data(), c->hpwbase.size() * sizeof(int64_t));
    if (c->d_pwpage) put(c->d_pwpage, c->hpwpage.data(), c->hpwpage.size() * sizeof(int32_t));
    const hipError_t e = hipStreamSynchronize(s);
    return rc ? rc : hip_check(ctx, e, "upload sync");
}

// 7) Output size estimate for BYTE_ARRAY chars: plain pages are bounded by
// their payload; dictionary pages by rows x mean entry length.
static int64_t char_estimate(const UploadPlan& up) {
    int64_t est = 0;
    for (const auto& p : up.hpages) {
        if (p.mode == pqk::MODE_DICT) {
            const DevDict& d = up.hdicts[p.dict];
            int64_t mean = d.nvals > 0 ? (d.size / d.nvals) + 1 : 1;
            est += static_cast<int64_t>(p.nvals) * mean;
        } else {
            est += p.size;
        }
    }
    return est + est / 8 + 64;
}

// Builds the device chunk from page walks already made on the host: one walk
// per input chunk (pq_chunk_upload) or one page-range walk (pq_chunk_upload_range).
static int upload_walked(pq_ctx* ctx, const uint8_t* file, size_t file_len, const pq_chunk_desc& desc,
                         std::vector<pqfmt::WalkResult>& walks, int64_t row_offset, pq_chunk** out,
                         RawStage* raw) {
    try {
        (void)hipSetDevice(ctx->device);
        auto c = std::make_unique<pq_chunk>();
        c->type = desc.type;
        c->max_def = desc.max_def_level;
        c->max_rep = desc.max_rep_level;
        c->plain_width = plain_width_of(c->type);
        c->width = c->plain_width;
        c->row_offset = row_offset;
        UploadPlan up(ctx);
        std::unique_ptr<HostTimed> plan_timer(new HostTimed(ctx, "up_plan"));
        std::unique_ptr<HostTimed> sub_timer(new HostTimed(ctx, "up_plan_pages"));
        plan_pages(c.get(), desc, walks, file_len, up);
        sub_timer.reset(new HostTimed(ctx, "up_plan_fused"));
        plan_fused(ctx, c.get(), up.hpages, up.hdicts);
        sub_timer.reset(new HostTimed(ctx, "up_plan_pipe"));
        plan_pipe(ctx, c.get(), up.hpages, up.hdicts);
        sub_timer.reset(new HostTimed(ctx, "up_plan_plain"));
        plan_plain(ctx, c.get(), up.hpages);
        sub_timer.reset(new HostTimed(ctx, "up_plan_rest"));
        c->npages = static_cast<int>(up.hpages.size());
        c->ndicts = static_cast<int>(up.hdicts.size());
        plan_tiles(c.get(), host_threads(), up);
        sub_timer.reset();
        plan_timer.reset();
        std::unique_ptr<HostTimed> alloc_timer(new HostTimed(ctx, "up_alloc"));
        if (alloc_chunk_device(c.get(), up)) {
            free_chunk_device(c.get());
            return set_err(ctx, PQ_ERR_HIP, "hipMalloc failed (chunk upload)");
        }
        alloc_timer.reset();
        HostTimed h2d_timer(ctx, "up_h2d");
        int rc = 0;
        const bool relaid = upload_image(ctx, c.get(), file, file_len, raw, up, &rc);
        if (!rc && !up.cents.empty()) rc = run_codec_pass(ctx, c.get(), file, relaid ? raw : nullptr, up);
        if (ctx->timing) {
            auto& f = ctx->timers["up_fill"];
            f.first += ctx->stager.fill_ms;
            f.second += 1;
            auto& w = ctx->timers["up_wait"];
            w.first += ctx->stager.wait_ms;
            w.second += 1;
        }
        rc = upload_tables(ctx, c.get(), up, rc);
        if (!rc && !up.cents.empty()) rc = codec_status(ctx, up);
        if (rc) {
            free_chunk_device(c.get());
            return rc;
        }
        c->char_estimate = char_estimate(up);
        *out = c.release();
        return 0;
    } catch (const pqfmt::Error& e) {
        return set_err(ctx, e.code, e.what());
    } catch (const std::exception& e) {
        return set_err(ctx, PQ_ERR_ALLOC, e.what());
    }
}

}  // namespace pqcapi

using namespace pqcapi;

extern "C" {

int pq_build_page_table(const uint8_t* file, size_t file_len, const pq_chunk_desc* chunk,
                        pq_page_desc* pages, int64_t cap, int64_t* npages, char* err,
                        size_t errlen) {
    if (!file || !chunk || !npages) return PQ_ERR_ARG;
    try {
        pqfmt::WalkResult w = pqfmt::walk_chunk(file, file_len, *chunk);
        *npages = static_cast<int64_t>(w.pages.size());
        for (int64_t i = 0; i < cap && i < *npages; i++) pages[i] = w.pages[i];
        if (err && errlen) {
            std::strncpy(err, w.message.c_str(), errlen - 1);
            err[errlen - 1] = 0;
        }
        return w.error;
    } catch (...) {
        return PQ_ERR_ALLOC;
    }
}

int pq_build_page_table_device(pq_ctx* ctx, const uint8_t* d_bytes, size_t len, int64_t base,
                               const pq_chunk_desc* chunk, int64_t seg_bytes, int64_t rec_cap,
                               pq_page_desc* pages, int64_t cap, int64_t* npages) {
    if (!ctx || !chunk || !npages || (!d_bytes && len) || base < 0 || seg_bytes < 0 || seg_bytes > (int64_t{1} << 30) ||
        rec_cap < 0 || rec_cap > (int64_t{1} << 20) || cap < 0 || (cap && !pages))
        return PQ_ERR_ARG;
    *npages = 0;
    DevGuard dg(ctx);
    try {
        return device_walk(ctx, d_bytes, len, base, chunk, seg_bytes, rec_cap, npages,
                           [&](const pq_page_desc* h, size_t k) {
                               std::memcpy(pages, h, std::min<size_t>(k, static_cast<size_t>(cap)) * sizeof(pq_page_desc));
                           });
    } catch (const std::exception& e) {
        return set_err(ctx, PQ_ERR_ALLOC, e.what());
    }
}

int pq_chunk_upload(pq_ctx* ctx, const uint8_t* file, size_t file_len, const pq_chunk_desc* chunks,
                    int nchunks, pq_chunk** out) {
    if (!ctx || !file || !chunks || nchunks <= 0 || !out) return PQ_ERR_ARG;
    DevGuard dg(ctx);
    *out = nullptr;
    try {
        // the chunks' page walks are independent: host threads
        std::vector<pqfmt::WalkResult> walks(static_cast<size_t>(nchunks));
        const int per = std::max(1, host_threads() / nchunks);  // threads per chunk walk
        // chunk extents known from the footer: their bytes start for HBM now
        RawStage raw;
        bool extents = true;
        for (int k = 0; k < nchunks && extents; k++) {
            int64_t lo = chunks[k].data_page_offset;
            if (chunks[k].has_dictionary_page_offset) lo = std::min(lo, chunks[k].dictionary_page_offset);
            extents = chunks[k].total_compressed_size > 0 && lo >= 0;
            raw.ext.push_back({lo, chunks[k].total_compressed_size});
        }
        if (extents) raw_start(ctx, file, file_len, raw);
        {
            HostTimed ht(ctx, "up_walk");
            // option device_walk: the page walk on the GPU over the raw bytes
            // once they are in HBM (walk.hip); a chunk it refuses (or any
            // chunk the raw upload does not cover) walks on the host, which
            // also reports the reference's errors
            std::vector<char> done(static_cast<size_t>(nchunks), 0);
            if (ctx->opt_dev_walk && raw.active) {
                raw.join();
                if (raw.err == hipSuccess) {
                    for (int k = 0; k < nchunks; k++) {
                        int64_t np = 0;
                        pqfmt::WalkResult& w = walks[static_cast<size_t>(k)];
                        const int rc = device_walk(ctx, ctx->d_raw + raw.base[static_cast<size_t>(k)],
                                                   static_cast<size_t>(raw.ext[static_cast<size_t>(k)].second),
                                                   raw.ext[static_cast<size_t>(k)].first, &chunks[k], 0, 0, &np,
                                                   [&](const pq_page_desc* h, size_t n) { w.pages.assign(h, h + n); });
                        done[static_cast<size_t>(k)] = rc == 0;
                    }
                }
            }
            parallel_for(nchunks, [&](int k) {
                if (!done[static_cast<size_t>(k)]) walks[static_cast<size_t>(k)] = pqfmt::walk_chunk(file, file_len, chunks[k], per);
            });
        }
        return upload_walked(ctx, file, file_len, chunks[0], walks, 0, out, &raw);
    } catch (const std::exception& e) {
        return set_err(ctx, PQ_ERR_ALLOC, e.what());
    }
}

int pq_chunk_upload_range(pq_ctx* ctx, const uint8_t* file, size_t file_len, const pq_chunk_desc* chunk,
                          const pq_page_desc* table, int64_t ntable, int64_t data_begin, int64_t data_end,
                          pq_chunk** out) {
    if (!ctx || !file || !chunk || (!table && ntable) || ntable < 0 || !out || data_begin < 0 ||
        data_end < data_begin)
        return PQ_ERR_ARG;
    DevGuard dg(ctx);
    *out = nullptr;
    try {
        // the data pages of the range, in walk order, and the dictionary pages they use
        std::vector<int64_t> data_idx;
        int64_t k = 0, row0 = -1, rows_before = 0;  // row0: chunk row of data page `data_begin`
        for (int64_t i = 0; i < ntable; i++) {
            if (table[i].page_type != PQ_DATA_PAGE) continue;
            if (k == data_begin) row0 = table[i].first_row;
            if (k >= data_begin && k < data_end) data_idx.push_back(i);
            rows_before = table[i].first_row + table[i].num_values;
            k++;
        }
        if (row0 < 0) row0 = rows_before;  // empty range at the end
        if (data_end > k) return set_err(ctx, PQ_ERR_ARG, "page range past the chunk's data pages");
        std::vector<int32_t> remap(static_cast<size_t>(ntable), -1);
        pqfmt::WalkResult w;
        for (int64_t i : data_idx) {
            const int32_t d = table[i].dict_page;
            if (d < 0) continue;
            if (d >= ntable || d >= i || table[d].page_type != PQ_DICTIONARY_PAGE)
                return set_err(ctx, PQ_ERR_ARG, "page table: bad dictionary page index");
            remap[static_cast<size_t>(d)] = 0;
        }
        for (int64_t i = 0; i < ntable; i++)  // dictionary pages first, in walk order
            if (remap[static_cast<size_t>(i)] == 0) {
                remap[static_cast<size_t>(i)] = static_cast<int32_t>(w.pages.size());
                w.pages.push_back(table[i]);
            }
        for (int64_t i : data_idx) {
            pq_page_desc p = table[i];
            p.first_row -= row0;
            if (p.dict_page >= 0) p.dict_page = remap[static_cast<size_t>(p.dict_page)];
            w.pages.push_back(p);
        }
        // extents: each page's header + payload, contiguous runs merged
        RawStage raw;
        for (const auto& p : w.pages) {
            const int64_t lo = p.header_offset, hi = p.payload_offset + std::max(p.payload_size, 0);
            if (!raw.ext.empty() && raw.ext.back().first + raw.ext.back().second == lo)
                raw.ext.back().second += hi - lo;
            else
                raw.ext.push_back({lo, hi - lo});
        }
        raw_start(ctx, file, file_len, raw);
        std::vector<pqfmt::WalkResult> walks(1);
        walks[0] = std::move(w);
        return upload_walked(ctx, file, file_len, *chunk, walks, row0, out, &raw);
    } catch (const std::exception& e) {
        return set_err(ctx, PQ_ERR_ALLOC, e.what());
    }
}

void pq_chunk_free(pq_ctx* ctx, pq_chunk* c) {
    if (!c) return;
    DevGuard dg(ctx);
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    free_chunk_device(c);
    delete c;
}

int64_t pq_chunk_num_rows(const pq_chunk* c) { return c ? c->nrows : 0; }
int64_t pq_chunk_first_row(const pq_chunk* c) { return c ? c->row_offset : 0; }
int64_t pq_chunk_num_pages(const pq_chunk* c) { return c ? c->npages : 0; }
int64_t pq_chunk_payload_bytes(const pq_chunk* c) { return c ? c->payload_bytes : 0; }
int pq_chunk_pages(const pq_chunk* c, pq_page_desc* pages, int64_t cap, int64_t* npages) {
    if (!c || !npages) return PQ_ERR_ARG;
    *npages = static_cast<int64_t>(c->walked.size());
    for (int64_t i = 0; i < cap && i < *npages; i++) pages[i] = c->walked[i];
    return 0;
}

}  // extern "C"
