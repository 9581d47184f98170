// api_word_margin.cpp -- the C ABI, part 8k: the margins of the open-vocabulary word decoder (str_er_set_word_margin beside
// STR_ER_WANT_WORD_DECODE behind the decoder in api_run_read.cpp, str_er_word_margins on the caller's cost rows; the contract is at
// str_er_word_margin in str_er.h).  The rules are word_margin_rules.h: the pure host entry point here runs them as they stand;
// k_word_margin (word_margin_kernels.h) reads what k_word_decode left for the same words.
#include "str_er_ctx.h"
#include "word_margin_rules.h"

namespace wd = str_er_wd;

static_assert(sizeof(str_er_word_margin) == 16, "word margin layout");

namespace str_er_host {

WgTab wg_layout(uint8_t *base, size_t at, size_t n_words, bool marginals)
{
    WgTab t{};
    Carve cv{at};
    t.o_out = cv.take(sizeof(str_er_word_margin) * n_words);
    const size_t o_rm = cv.take(4 * wd::MAX_RUNS * n_words), o_rr = cv.take(wd::MAX_RUNS * n_words), o_ra = cv.take(wd::MAX_RUNS * n_words),
                 o_mg = cv.take(marginals ? 4 * (size_t)wd::MAX_RUNS * wd::MARGINALS * n_words : 0);
    t.bytes = cv.off;
    t.down_bytes = cv.off - t.o_out;
    if (base) {
        t.margins = reinterpret_cast<str_er_word_margin *>(base + t.o_out); t.row_margin = reinterpret_cast<int32_t *>(base + o_rm);
        t.row_read = base + o_rr; t.row_alt = base + o_ra; t.marginals = marginals ? reinterpret_cast<int32_t *>(base + o_mg) : nullptr;
    }
    return t;
}

} // namespace str_er_host

namespace {

bool args_ok(const uint8_t *costs, int32_t n_runs, const int32_t *first_run, const int32_t *n_of, int32_t n_words, const str_er_word_margin *margins,
             const int32_t *row_margin, const uint8_t *row_read, const uint8_t *row_alt)
{
    return n_runs >= 0 && n_words >= 0 && (n_runs == 0 || costs) && (n_words == 0 || (first_run && n_of && margins && row_margin && row_read && row_alt));
}

} // namespace

extern "C" {

int str_er_set_word_margin(str_er_ctx *c, int32_t on)
try {
    if (!c) return STR_ER_EINVAL;
    c->wd_margin = on != 0;
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_word_margins(str_er_ctx *c, const uint8_t *costs, int32_t n_runs, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words,
                        str_er_word_margin *margins, int32_t *row_margin, uint8_t *row_read, uint8_t *row_alt, int32_t *marginals)
try {
    if (!c) return STR_ER_EINVAL;
    if (!args_ok(costs, n_runs, first_run, n_runs_of_word, n_words, margins, row_margin, row_read, row_alt)) return fail(c, STR_ER_EINVAL, "bad arguments");
    if (!c->bigram_set) return fail(c, STR_ER_ESTATE, "str_er_word_margins needs a bigram table (str_er_set_bigram)");
    if (!words_in_rows(n_runs, first_run, n_runs_of_word, n_words)) return fail(c, STR_ER_EINVAL, "word margins: a word outside the cost rows");
    if (n_words == 0) return STR_ER_OK;
    // the rows and words | the decoder's tables (scratch: they stay on the device) | the margins' tables
    const size_t nw = (size_t)n_words, at_dec = rows_in_layout(nullptr, 0, (size_t)n_runs, nw, false).bytes, at = wd_layout(nullptr, at_dec, nw).bytes;
    if (const int rc = c->wg_tab.ensure(c, wg_layout(nullptr, at, nw, marginals != nullptr).bytes, "word margin tables"); rc != STR_ER_OK) return rc;
    const WdTab W = wd_layout(c->wg_tab.d(), at_dec, nw);
    const WgTab H = wg_layout(c->wg_tab.h(), at, nw, marginals != nullptr), D = wg_layout(c->wg_tab.d(), at, nw, marginals != nullptr);
    hipStream_t s = c->stream;
    RowsIn      I{};
    if (const int rc = rows_in_upload(c, s, c->wg_tab, nullptr, costs, (size_t)n_runs, nullptr, 0, first_run, n_runs_of_word, nullptr, nw, I); rc != STR_ER_OK) return rc;
    launch_word_decode(s, c->bigram.d(), c->wd_ins, c->wd_del, I.costs, I.first, I.n_of, n_words, W.dec, W.chars, W.src);
    launch_word_margin(s, c->bigram.d(), c->wd_ins, c->wd_del, I.costs, I.first, I.n_of, n_words, W.dec, W.chars, W.src, D.margins, D.row_margin, D.row_read, D.row_alt,
                       D.marginals);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->wg_tab.h() + H.o_out, c->wg_tab.d() + H.o_out, H.down_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    std::memcpy(margins, H.margins, sizeof(str_er_word_margin) * nw);
    std::memcpy(row_margin, H.row_margin, 4 * wd::MAX_RUNS * nw);
    std::memcpy(row_read, H.row_read, wd::MAX_RUNS * nw);
    std::memcpy(row_alt, H.row_alt, wd::MAX_RUNS * nw);
    if (marginals) std::memcpy(marginals, H.marginals, 4 * (size_t)wd::MAX_RUNS * wd::MARGINALS * nw);
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_word_margins_host(const uint8_t *costs, int32_t n_runs, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, const uint8_t *bigram,
                             int32_t ins, int32_t del, str_er_word_margin *margins, int32_t *row_margin, uint8_t *row_read, uint8_t *row_alt, int32_t *marginals)
{
    if (!args_ok(costs, n_runs, first_run, n_runs_of_word, n_words, margins, row_margin, row_read, row_alt) || !bigram) return STR_ER_EINVAL;
    if (!wd::params_ok(ins, del) || !words_in_rows(n_runs, first_run, n_runs_of_word, n_words)) return STR_ER_EINVAL;
    for (int32_t w = 0; w < n_words; ++w) {
        const uint8_t *C = costs + (size_t)first_run[w] * wd::ALPHABET;
        uint8_t        chars[wd::MAX_CHARS], src[wd::MAX_CHARS];
        const str_er_word_decode d = wd::decode_word(C, n_runs_of_word[w], bigram, ins, del, chars, src);
        margins[w] = wd::margins_word(C, n_runs_of_word[w], bigram, ins, del, chars, src, d.n_chars, row_margin + (size_t)w * wd::MAX_RUNS,
                                      row_read + (size_t)w * wd::MAX_RUNS, row_alt + (size_t)w * wd::MAX_RUNS,
                                      marginals ? marginals + (size_t)w * wd::MAX_RUNS * wd::MARGINALS : nullptr);
    }
    return STR_ER_OK;
}

const str_er_word_margin *str_er_result_word_margins(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_word_margins, &str_er_result::word_margins, n);
}
const int32_t *str_er_result_word_row_margins(const str_er_result *r, uint64_t *n_bytes)
{
    const int32_t *p = result_table(r, r && r->have_word_margins, &str_er_result::word_row_margins, n_bytes);
    if (n_bytes) *n_bytes *= 4;
    return p;
}
const uint8_t *str_er_result_word_row_reads(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_word_margins, &str_er_result::word_row_reads, n_bytes);
}
const uint8_t *str_er_result_word_row_alts(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_word_margins, &str_er_result::word_row_alts, n_bytes);
}

} // extern "C"
