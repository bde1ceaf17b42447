// capi_file.cpp — the pq_file_* functions of the C ABI (include/pq_gpu.h): a
// parsed footer, its leaf columns and the page index.  Host only.
#include <array>
#include <cstring>
#include <memory>

#include "host/format.hpp"
#include "pq_gpu.h"

struct pq_file {
    pqfmt::FileMeta meta;
    std::vector<pqfmt::LeafColumn> cols;
    std::vector<std::array<int64_t, 4>> pidx;
};

extern "C" {

int pq_file_open(const uint8_t* file, size_t file_len, pq_file** out, char* err, size_t errlen) {
    if (!file || !out) return PQ_ERR_ARG;
    *out = nullptr;
    try {
        auto f = std::make_unique<pq_file>();
        f->meta = pqfmt::parse_footer(file, file_len);
        f->cols = pqfmt::leaf_columns(f->meta);
        f->pidx = pqfmt::page_index(file, file_len, f->meta);
        *out = f.release();
        return 0;
    } catch (const pqfmt::Error& e) {
        if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
        return e.code;
    } catch (const std::exception& e) {
        if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
        return PQ_ERR_ALLOC;
    }
}
void pq_file_close(pq_file* f) { delete f; }
int64_t pq_file_num_rows(const pq_file* f) { return f ? f->meta.num_rows : 0; }
int pq_file_num_row_groups(const pq_file* f) { return f ? static_cast<int>(f->meta.row_groups.size()) : 0; }
int pq_file_num_columns(const pq_file* f) { return f ? static_cast<int>(f->cols.size()) : 0; }
int pq_file_column_name(const pq_file* f, int col, char* buf, size_t buflen) {
    if (!f || col < 0 || col >= static_cast<int>(f->cols.size()) || !buf || !buflen) return PQ_ERR_ARG;
    std::strncpy(buf, f->cols[col].name.c_str(), buflen - 1);
    buf[buflen - 1] = 0;
    return 0;
}
int pq_file_find_column(const pq_file* f, const char* name) {  // last match wins (build_column_index)
    if (!f || !name) return -1;
    int found = -1;
    for (size_t i = 0; i < f->cols.size(); i++)
        if (f->cols[i].name == name) found = static_cast<int>(i);
    return found;
}
int pq_file_column_info(const pq_file* f, int col, int32_t* type, int16_t* max_def,
                        int16_t* max_rep, int32_t* repetition, int32_t* converted_type) {
    if (!f || col < 0 || col >= static_cast<int>(f->cols.size())) return PQ_ERR_ARG;
    const auto& c = f->cols[col];
    if (type) *type = c.type;
    if (max_def) *max_def = c.max_def;
    if (max_rep) *max_rep = c.max_rep;
    if (repetition) *repetition = c.repetition.value_or(-1);
    if (converted_type) *converted_type = c.converted_type.value_or(-1);
    return 0;
}

int pq_file_chunk(const pq_file* f, int rg, int col, pq_chunk_desc* out) {
    if (!f || !out || rg < 0 || rg >= static_cast<int>(f->meta.row_groups.size()) || col < 0 ||
        col >= static_cast<int>(f->cols.size()))
        return PQ_ERR_ARG;
    const auto& lc = f->cols[col];
    const auto& r = f->meta.row_groups[rg];
    if (lc.column_index >= static_cast<int>(r.columns.size())) return PQ_ERR_ARG;
    const auto& cc = r.columns[lc.column_index];
    if (!cc.meta) return PQ_ERR_OPTIONAL;  // "ColumnChunk has no metadata"
    std::memset(out, 0, sizeof *out);
    out->num_values = cc.meta->num_values;
    out->data_page_offset = cc.meta->data_page_offset;
    out->has_dictionary_page_offset = cc.meta->dictionary_page_offset.has_value();
    out->dictionary_page_offset = cc.meta->dictionary_page_offset.value_or(0);
    out->codec = cc.meta->codec;
    out->type = lc.type;
    out->max_def_level = lc.max_def;
    out->max_rep_level = lc.max_rep;
    out->total_compressed_size = cc.meta->total_compressed;
    return 0;
}
int64_t pq_file_row_group_rows(const pq_file* f, int rg) {
    if (!f || rg < 0 || rg >= static_cast<int>(f->meta.row_groups.size())) return 0;
    return f->meta.row_groups[rg].num_rows;
}
int64_t pq_file_num_pages(const pq_file* f) { return f ? static_cast<int64_t>(f->pidx.size()) : 0; }
int pq_file_page_index(const pq_file* f, int64_t* entries, int64_t cap) {
    if (!f || !entries) return PQ_ERR_ARG;
    for (int64_t i = 0; i < cap && i < static_cast<int64_t>(f->pidx.size()); i++)
        for (int k = 0; k < 4; k++) entries[4 * i + k] = f->pidx[i][k];
    return 0;
}

}  // extern "C"
