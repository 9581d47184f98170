// api_line_margin.cpp -- the C ABI, part 8m: the margins of the line decoder (str_er_set_line_margin beside str_er_set_line_decode behind
// the line decode in api_run_read.cpp, str_er_line_margins on the caller's cost rows; the contract is at str_er_line_margin in
// str_er.h).  The rules are line_margin_rules.h: the pure host entry point here runs them as they stand; k_line_margin
// (line_margin_kernels.h) reads what k_line_decode left for the same lines, in the tables of line_decode_enqueue (api_line_decode.cpp).
#include "str_er_ctx.h"
#include "line_margin_rules.h"

namespace wd = str_er_wd;
namespace ld = str_er_ld;
namespace lm = str_er_lm;

static_assert(sizeof(str_er_line_margin) == 32, "line margin layout");
static_assert(lm::MARGINALS == LM_MARGINALS && LM_FW_ROW >= 2 * wd::STATES + 2, "the kernel's rows are the rules'");

namespace {

bool args_ok(const uint8_t *costs, int32_t n_rows, const uint8_t *gaps, const int32_t *first_row, const int32_t *n_of, int32_t n_lines, const str_er_line_margin *margins,
             const int32_t *row_margin, const uint8_t *row_read, const uint8_t *row_alt, const int32_t *gap_margin, const uint8_t *gap_move)
{
    return n_rows >= 0 && n_lines >= 0 && (n_rows == 0 || (costs && gaps && row_margin && row_read && row_alt && gap_margin && gap_move)) &&
           (n_lines == 0 || (first_row && n_of && margins));
}

// what lies in no line
void preset(size_t nr, int32_t *row_margin, uint8_t *row_read, uint8_t *row_alt, int32_t *gap_margin, uint8_t *gap_move, int32_t *marginals)
{
    if (nr == 0) return;
    std::memset(row_margin, 0xFF, 4 * nr); std::memset(gap_margin, 0xFF, 4 * nr);
    std::memset(row_read, 0xFF, nr); std::memset(row_alt, 0xFF, nr); std::memset(gap_move, 0xFF, nr);
    if (marginals) std::memset(marginals, 0xFF, 4 * (size_t)lm::MARGINALS * nr);
}

} // namespace

extern "C" {

int str_er_set_line_margin(str_er_ctx *c, int32_t on)
try {
    if (!c) return STR_ER_EINVAL;
    c->ln_margin = on != 0;
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_line_margins(str_er_ctx *c, const uint8_t *costs, int32_t n_rows, const uint8_t *gaps, const int32_t *first_row, const int32_t *n_rows_of_line, int32_t n_lines,
                        str_er_line_margin *margins, int32_t *row_margin, uint8_t *row_read, uint8_t *row_alt, int32_t *gap_margin, uint8_t *gap_move, int32_t *marginals)
try {
    if (!c) return STR_ER_EINVAL;
    if (!args_ok(costs, n_rows, gaps, first_row, n_rows_of_line, n_lines, margins, row_margin, row_read, row_alt, gap_margin, gap_move)) return fail(c, STR_ER_EINVAL, "bad arguments");
    if (!c->bigram_set) return fail(c, STR_ER_ESTATE, "str_er_line_margins needs a bigram table (str_er_set_bigram)");
    if (!ld::lines_in_rows(n_rows, first_row, n_rows_of_line, n_lines)) return fail(c, STR_ER_EINVAL, "line margins: a line outside the cost rows, or the lines out of order");
    if (!ld::gaps_ok(gaps, first_row, n_rows_of_line, n_lines)) return fail(c, STR_ER_EINVAL, "line margins: a gap with both moves off");
    const size_t nr = (size_t)n_rows, nl = (size_t)n_lines;
    const bool   mg = marginals != nullptr;
    if (nl == 0) { preset(nr, row_margin, row_read, row_alt, gap_margin, gap_move, marginals); return STR_ER_OK; }
    const size_t at = rows_in_layout(nullptr, 0, nr, nl, false).bytes;
    if (const int rc = c->ln_tab.ensure(c, ln_layout(nullptr, at, nr, nl, false, false, true, mg).bytes, "line decode tables"); rc != STR_ER_OK) return rc;
    hipStream_t s = c->stream;
    RowsIn      I{};
    if (const int rc = rows_in_upload(c, s, c->ln_tab, nullptr, costs, nr, nullptr, 0, first_row, n_rows_of_line, nullptr, nl, I); rc != STR_ER_OK) return rc;
    LnTab H{}, D{};
    // (STR_ER_ECAPACITY where the forward table would not fit: line_decode_enqueue holds the bound for this path and the detect call's)
    if (const int rc = line_decode_enqueue(c, s, at, I.costs, nr, gaps, nullptr, nullptr, I.first, I.n_of, nl, nullptr, H, D, true, mg); rc != STR_ER_OK) return rc;
    HIP_TRY(c, hipGetLastError());
    const size_t o_out = (size_t)(reinterpret_cast<uint8_t *>(H.margins) - c->ln_tab.h());          // (the decoder's tables stay on the device)
    HIP_TRY(c, hipMemcpyAsync(c->ln_tab.h() + o_out, c->ln_tab.d() + o_out, H.bytes - o_out, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    std::memcpy(margins, H.margins, sizeof(str_er_line_margin) * nl);
    if (nr > 0) {
        std::memcpy(row_margin, H.row_margin, 4 * nr); std::memcpy(gap_margin, H.gap_margin, 4 * nr);
        std::memcpy(row_read, H.row_read, nr); std::memcpy(row_alt, H.row_alt, nr); std::memcpy(gap_move, H.gap_move, nr);
        if (mg) std::memcpy(marginals, H.marginals, 4 * (size_t)lm::MARGINALS * nr);
    }
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_line_margins_host(const uint8_t *costs, int32_t n_rows, const uint8_t *gaps, const int32_t *first_row, const int32_t *n_rows_of_line, int32_t n_lines,
                             const uint8_t *bigram, int32_t ins, int32_t del, str_er_line_margin *margins, int32_t *row_margin, uint8_t *row_read, uint8_t *row_alt,
                             int32_t *gap_margin, uint8_t *gap_move, int32_t *marginals)
try {
    if (!args_ok(costs, n_rows, gaps, first_row, n_rows_of_line, n_lines, margins, row_margin, row_read, row_alt, gap_margin, gap_move) || !bigram) return STR_ER_EINVAL;
    if (!wd::params_ok(ins, del) || !ld::lines_in_rows(n_rows, first_row, n_rows_of_line, n_lines) || !ld::gaps_ok(gaps, first_row, n_rows_of_line, n_lines))
        return STR_ER_EINVAL;
    preset((size_t)n_rows, row_margin, row_read, row_alt, gap_margin, gap_move, marginals);
    std::vector<uint8_t>  chars;
    std::vector<uint16_t> src;
    std::vector<int32_t>  wor;
    for (int32_t t = 0; t < n_lines; ++t) {
        const size_t f = (size_t)first_row[t], n = (size_t)n_rows_of_line[t];
        chars.assign(ld::PER_ROW * n + 1, 0xFF); src.assign(ld::PER_ROW * n + 1, 0xFFFF); wor.assign(n + 1, -1);
        const str_er_line_decode d = ld::decode_line(costs + f * wd::ALPHABET, gaps + 2 * f, (int)n, bigram, ins, del, chars.data(), src.data(), wor.data());
        margins[t] = lm::margins_line(costs + f * wd::ALPHABET, gaps + 2 * f, (int)n, bigram, ins, del, chars.data(), src.data(), d.n_chars, row_margin + f, row_read + f,
                                      row_alt + f, gap_margin + f, gap_move + f, marginals ? marginals + f * lm::MARGINALS : nullptr);
    }
    return STR_ER_OK;
} catch (...) { return STR_ER_ENOMEM; }

int str_er_line_margin_stats(const str_er_ctx *c, uint64_t *table_bytes)
{
    if (!c) return STR_ER_EINVAL;
    if (table_bytes) *table_bytes = c->ln_fw.size();
    return STR_ER_OK;
}

const str_er_line_margin *str_er_result_line_margins(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_line_margins, &str_er_result::line_margins, n);
}
const int32_t *str_er_result_line_row_margins(const str_er_result *r, uint64_t *n_bytes)
{
    const int32_t *p = result_table(r, r && r->have_line_margins, &str_er_result::line_row_margins, n_bytes);
    if (n_bytes) *n_bytes *= 4;
    return p;
}
const uint8_t *str_er_result_line_row_reads(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_line_margins, &str_er_result::line_row_reads, n_bytes);
}
const uint8_t *str_er_result_line_row_alts(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_line_margins, &str_er_result::line_row_alts, n_bytes);
}
const int32_t *str_er_result_line_gap_margins(const str_er_result *r, uint64_t *n_bytes)
{
    const int32_t *p = result_table(r, r && r->have_line_margins, &str_er_result::line_gap_margins, n_bytes);
    if (n_bytes) *n_bytes *= 4;
    return p;
}
const uint8_t *str_er_result_line_gap_moves(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_line_margins, &str_er_result::line_gap_moves, n_bytes);
}

} // extern "C"
