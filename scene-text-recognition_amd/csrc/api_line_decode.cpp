// api_line_decode.cpp -- the C ABI, part 8l: the line decoder (str_er_set_line_decode beside STR_ER_WANT_WORD_DECODE behind the decoder
// in api_run_read.cpp, str_er_decode_lines on the caller's cost rows; the contract is at str_er_line_decode in str_er.h).  The rules are
// line_decode_rules.h: the pure host entry points here run them as they stand; k_line_decode (line_decode_kernels.h) takes the table as
// the caller gave it.
#include "str_er_ctx.h"
#include "line_decode_rules.h"

namespace wd = str_er_wd;
namespace ld = str_er_ld;

static_assert(sizeof(str_er_line_decode) == 24, "line decode layout");
static_assert(ld::MAX_ROWS == 1024 && LD_BP_ROW >= wd::STATES + 1, "the kernel's limits are the rules'");

namespace str_er_host {

LnTab ln_layout(uint8_t *base, size_t at, size_t n_rows, size_t n_lines, bool windows, bool map, bool margin, bool marginals)
{
    LnTab t{};
    Carve cv{at};
    t.o_up = cv.take(2 * n_rows);
    const size_t o_first = cv.take(windows ? 4 * n_lines : 0), o_nof = cv.take(windows ? 4 * n_lines : 0),
                 o_map = cv.take(map ? 4 * n_rows : 0);
    t.up_bytes = cv.off - t.o_up;
    t.o_dec = cv.take(sizeof(str_er_line_decode) * n_lines);
    const size_t o_chars = cv.take(ld::PER_ROW * n_rows), o_src = cv.take(2 * ld::PER_ROW * n_rows), o_wor = cv.take(4 * n_rows);
    // (behind the labels: all of it is preset with bytes of 0xFF, which read -1 in the margins' tables too)
    const size_t o_lm = cv.take(margin ? sizeof(str_er_line_margin) * n_lines : 0), o_rm = cv.take(margin ? 4 * n_rows : 0), o_gm = cv.take(margin ? 4 * n_rows : 0),
                 o_rr = cv.take(margin ? n_rows : 0), o_ra = cv.take(margin ? n_rows : 0), o_gv = cv.take(margin ? n_rows : 0),
                 o_mg = cv.take(margin && marginals ? 4 * (size_t)LM_MARGINALS * n_rows : 0);
    t.bytes = cv.off;
    t.down_bytes = cv.off - t.o_dec;
    if (base) {
        t.gaps = base + t.o_up; t.first = reinterpret_cast<int32_t *>(base + o_first); t.n_of = reinterpret_cast<int32_t *>(base + o_nof);
        t.row_map = map ? reinterpret_cast<int32_t *>(base + o_map) : nullptr;
        t.dec = reinterpret_cast<str_er_line_decode *>(base + t.o_dec); t.chars = base + o_chars; t.src = reinterpret_cast<uint16_t *>(base + o_src);
        t.word_of_row = reinterpret_cast<int32_t *>(base + o_wor);
        if (margin) {
            t.margins = reinterpret_cast<str_er_line_margin *>(base + o_lm); t.row_margin = reinterpret_cast<int32_t *>(base + o_rm);
            t.gap_margin = reinterpret_cast<int32_t *>(base + o_gm); t.row_read = base + o_rr; t.row_alt = base + o_ra; t.gap_move = base + o_gv;
            t.marginals = marginals ? reinterpret_cast<int32_t *>(base + o_mg) : nullptr;
        }
    }
    return t;
}

int line_decode_enqueue(str_er_ctx *c, hipStream_t s, size_t at, const uint8_t *d_rows, size_t n_rows, const uint8_t *gaps, const int32_t *first, const int32_t *n_of,
                        const int32_t *d_first, const int32_t *d_n_of, size_t n_lines, const int32_t *row_map, LnTab &H, LnTab &D, bool margin, bool marginals)
{
    const bool windows = first != nullptr, map = row_map != nullptr;
    if (const int rc = c->ln_tab.ensure(c, ln_layout(nullptr, at, n_rows, n_lines, windows, map, margin, marginals).bytes, "line decode tables"); rc != STR_ER_OK) return rc;
    if (const int rc = c->ln_bp.ensure(c, 2 * (size_t)LD_BP_ROW * n_rows, "line decode back pointers"); rc != STR_ER_OK) return rc;
    if (margin) {
        if ((uint64_t)n_rows > 0x7FFFFFFFull / (4 * LM_FW_ROW)) return fail(c, STR_ER_ECAPACITY, "line margins: too many rows");
        if (const int rc = c->ln_fw.ensure(c, 4 * (size_t)LM_FW_ROW * n_rows, "line margin forward values"); rc != STR_ER_OK) return rc;
    }
    H = ln_layout(c->ln_tab.h(), at, n_rows, n_lines, windows, map, margin, marginals); D = ln_layout(c->ln_tab.d(), at, n_rows, n_lines, windows, map, margin, marginals);
    if (n_rows > 0) std::memcpy(H.gaps, gaps, 2 * n_rows);
    if (map && n_rows > 0) std::memcpy(H.row_map, row_map, 4 * n_rows);
    if (windows && n_lines > 0) { std::memcpy(H.first, first, 4 * n_lines); std::memcpy(H.n_of, n_of, 4 * n_lines); }
    if (H.up_bytes > 0) HIP_TRY(c, hipMemcpyAsync(c->ln_tab.d() + H.o_up, c->ln_tab.h() + H.o_up, H.up_bytes, hipMemcpyHostToDevice, s));
    // what lies in no line reads 0xFF, 0xFFFF and -1: the labels, the sources and the words of the rows are all bytes of 0xFF
    if (n_rows > 0) HIP_TRY(c, hipMemsetAsync(D.chars, 0xFF, (size_t)(c->ln_tab.d() + D.bytes - D.chars), s));
    launch_line_decode(s, c->bigram.d(), c->wd_ins, c->wd_del, d_rows, D.gaps, windows ? D.first : d_first, windows ? D.n_of : d_n_of, D.row_map, (int)n_lines, c->ln_bp.d<uint16_t>(),
                       D.dec, D.chars, D.src, D.word_of_row);
    if (margin)          // the decoder's rows, gaps and windows, its records, labels and sources where it left them
        launch_line_margin(s, c->bigram.d(), c->wd_ins, c->wd_del, d_rows, D.gaps, windows ? D.first : d_first, windows ? D.n_of : d_n_of, D.row_map, (int)n_lines, D.dec, D.chars,
                           D.src, c->ln_fw.d<uint32_t>(), D.margins, D.row_margin, D.row_read, D.row_alt, D.gap_margin, D.gap_move, D.marginals);
    return STR_ER_OK;
}

} // namespace str_er_host

namespace {

bool args_ok(const uint8_t *costs, int32_t n_rows, const uint8_t *gaps, const int32_t *first_row, const int32_t *n_of, int32_t n_lines, const str_er_line_decode *dec,
             const uint8_t *chars, const uint16_t *src, const int32_t *word_of_row)
{
    return n_rows >= 0 && n_lines >= 0 && (n_rows == 0 || (costs && gaps && chars && src && word_of_row)) && (n_lines == 0 || (first_row && n_of && dec));
}

} // namespace

extern "C" {

int str_er_set_line_decode(str_er_ctx *c, int32_t on, int32_t weight)
try {
    if (!c) return STR_ER_EINVAL;
    if (!ld::weight_ok(weight)) return fail(c, STR_ER_EINVAL, "line decode: the weight is in 0 .. 127");
    c->ln_on = on != 0; c->ln_weight = weight;
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_line_gap_costs(const str_er_line_run *runs, int32_t n_runs, const int32_t *row_run, int32_t n_rows, const int32_t *first_row, const int32_t *n_rows_of_line,
                          const uint32_t *colmax, int32_t n_lines, int32_t num, int32_t den, int32_t weight, uint8_t *gaps)
{
    if (n_runs < 0 || n_rows < 0 || n_lines < 0 || (n_runs > 0 && !runs) || (n_rows > 0 && !gaps) || (n_lines > 0 && (!first_row || !n_rows_of_line || !colmax)))
        return STR_ER_EINVAL;
    if (!word_gap_ok(num, den) || !ld::weight_ok(weight) || !ld::lines_in_rows(n_rows, first_row, n_rows_of_line, n_lines)) return STR_ER_EINVAL;
    return ld::gap_costs(runs, n_runs, row_run, n_rows, first_row, n_rows_of_line, colmax, n_lines, num, den, weight, gaps) ? STR_ER_OK : STR_ER_EINVAL;
}

int str_er_decode_lines(str_er_ctx *c, const uint8_t *costs, int32_t n_rows, const uint8_t *gaps, const int32_t *first_row, const int32_t *n_rows_of_line, int32_t n_lines,
                        str_er_line_decode *dec, uint8_t *chars, uint16_t *src, int32_t *word_of_row)
try {
    if (!c) return STR_ER_EINVAL;
    if (!args_ok(costs, n_rows, gaps, first_row, n_rows_of_line, n_lines, dec, chars, src, word_of_row)) return fail(c, STR_ER_EINVAL, "bad arguments");
    if (!c->bigram_set) return fail(c, STR_ER_ESTATE, "str_er_decode_lines needs a bigram table (str_er_set_bigram)");
    if (!ld::lines_in_rows(n_rows, first_row, n_rows_of_line, n_lines)) return fail(c, STR_ER_EINVAL, "line decode: a line outside the cost rows, or the lines out of order");
    if (!ld::gaps_ok(gaps, first_row, n_rows_of_line, n_lines)) return fail(c, STR_ER_EINVAL, "line decode: a gap with both moves off");
    if ((uint64_t)n_rows > 0x7FFFFFFFull / (2 * LD_BP_ROW)) return fail(c, STR_ER_ECAPACITY, "line decode: too many rows");
    const size_t nr = (size_t)n_rows, nl = (size_t)n_lines;
    if (nl == 0) {
        if (nr > 0) { std::memset(chars, 0xFF, ld::PER_ROW * nr); std::memset(src, 0xFF, 2 * ld::PER_ROW * nr); std::memset(word_of_row, 0xFF, 4 * nr); }
        return STR_ER_OK;
    }
    const size_t at = rows_in_layout(nullptr, 0, nr, nl, false).bytes;
    if (const int rc = c->ln_tab.ensure(c, ln_layout(nullptr, at, nr, nl, false, false).bytes, "line decode tables"); rc != STR_ER_OK) return rc;
    hipStream_t s = c->stream;
    RowsIn      I{};
    if (const int rc = rows_in_upload(c, s, c->ln_tab, nullptr, costs, nr, nullptr, 0, first_row, n_rows_of_line, nullptr, nl, I); rc != STR_ER_OK) return rc;
    LnTab H{}, D{};
    if (const int rc = line_decode_enqueue(c, s, at, I.costs, nr, gaps, nullptr, nullptr, I.first, I.n_of, nl, nullptr, H, D); rc != STR_ER_OK) return rc;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->ln_tab.h() + H.o_dec, c->ln_tab.d() + H.o_dec, H.down_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    std::memcpy(dec, H.dec, sizeof(str_er_line_decode) * nl);
    if (nr > 0) { std::memcpy(chars, H.chars, ld::PER_ROW * nr); std::memcpy(src, H.src, 2 * ld::PER_ROW * nr); std::memcpy(word_of_row, H.word_of_row, 4 * nr); }
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_decode_lines_host(const uint8_t *costs, int32_t n_rows, const uint8_t *gaps, const int32_t *first_row, const int32_t *n_rows_of_line, int32_t n_lines,
                             const uint8_t *bigram, int32_t ins, int32_t del, str_er_line_decode *dec, uint8_t *chars, uint16_t *src, int32_t *word_of_row)
try {
    if (!args_ok(costs, n_rows, gaps, first_row, n_rows_of_line, n_lines, dec, chars, src, word_of_row) || !bigram) return STR_ER_EINVAL;
    if (!wd::params_ok(ins, del) || !ld::lines_in_rows(n_rows, first_row, n_rows_of_line, n_lines) || !ld::gaps_ok(gaps, first_row, n_rows_of_line, n_lines))
        return STR_ER_EINVAL;
    const size_t nr = (size_t)n_rows;
    if (nr > 0) { std::memset(chars, 0xFF, ld::PER_ROW * nr); std::memset(src, 0xFF, 2 * ld::PER_ROW * nr); std::memset(word_of_row, 0xFF, 4 * nr); }
    for (int32_t t = 0; t < n_lines; ++t) {
        const size_t f = (size_t)first_row[t];
        dec[t] = ld::decode_line(costs + f * wd::ALPHABET, gaps + 2 * f, n_rows_of_line[t], bigram, ins, del, chars + ld::PER_ROW * f, src + ld::PER_ROW * f, word_of_row + f);
    }
    return STR_ER_OK;
} catch (...) { return STR_ER_ENOMEM; }

int str_er_line_decode_stats(const str_er_ctx *c, uint64_t *table_bytes)
{
    if (!c) return STR_ER_EINVAL;
    if (table_bytes) *table_bytes = c->ln_bp.size();
    return STR_ER_OK;
}

const str_er_line_decode *str_er_result_line_decodes(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_line_decodes, &str_er_result::line_decodes, n);
}
const uint8_t *str_er_result_line_decode_chars(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_line_decodes, &str_er_result::line_decode_chars, n_bytes);
}
const uint16_t *str_er_result_line_decode_src(const str_er_result *r, uint64_t *n)
{
    return result_table(r, r && r->have_line_decodes, &str_er_result::line_decode_src, n);
}
const int32_t *str_er_result_line_decode_word_of_row(const str_er_result *r, uint64_t *n)
{
    return result_table(r, r && r->have_line_decodes, &str_er_result::line_decode_word_of_row, n);
}
const uint8_t *str_er_result_line_gap_costs(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_line_decodes, &str_er_result::line_gap_costs, n_bytes);
}
const int32_t *str_er_result_line_decode_windows(const str_er_result *r, uint64_t *n)
{
    return result_table(r, r && r->have_line_decodes, &str_er_result::line_decode_windows, n);
}

} // extern "C"
