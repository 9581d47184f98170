// api_word_decode.cpp -- the C ABI, part 8e: the open-vocabulary word decoder (STR_ER_WANT_WORD_DECODE behind the reading of the runs in
// api_run_read.cpp, str_er_decode_words on the caller's cost rows; the contract is at str_er_word_decode in str_er.h).  The rules are
// word_decode_rules.h: the pure host entry points here run them as they stand; k_word_decode (word_decode_kernels.h) takes the table as
// the caller gave it.
#include "str_er_ctx.h"
#include "word_decode_rules.h"

namespace wd = str_er_wd;

static_assert(sizeof(str_er_word_decode) == 24, "word decode layout");

namespace str_er_host {

WdTab wd_layout(uint8_t *base, size_t at, size_t n_words)
{
    WdTab t{};
    Carve cv{at};
    t.o_dec = cv.take(sizeof(str_er_word_decode) * n_words);
    const size_t o_chars = cv.take(wd::MAX_CHARS * n_words), o_src = cv.take(wd::MAX_CHARS * n_words);
    t.bytes = cv.off;
    t.down_bytes = cv.off - t.o_dec;
    if (base) { t.dec = reinterpret_cast<str_er_word_decode *>(base + t.o_dec); t.chars = base + o_chars; t.src = base + o_src; }
    return t;
}

} // namespace str_er_host

namespace {

bool args_ok(const uint8_t *costs, int32_t n_runs, const int32_t *first_run, const int32_t *n_of, int32_t n_words, const str_er_word_decode *dec,
             const uint8_t *chars, const uint8_t *src)
{
    return n_runs >= 0 && n_words >= 0 && (n_runs == 0 || costs) && (n_words == 0 || (first_run && n_of && dec && chars && src));
}

} // namespace

extern "C" {

int str_er_set_bigram(str_er_ctx *c, const uint8_t *cost)
try {
    if (!c) return STR_ER_EINVAL;
    HIP_TRY(c, hipStreamSynchronize(c->stream));       // (a call in flight still reads the table that is replaced)
    ++c->decode_pool_gen;          // (a decode pool is bound to the table it was made with: str_er_pool_decode)
    if (!cost) {
        c->bigram = DevBuf();
        c->bigram_set = false;
        return STR_ER_OK;
    }
    DevBuf fresh;
    if (const int rc = fresh.ensure(c, wd::TABLE, "bigram table"); rc != STR_ER_OK) return rc;
    HIP_TRY(c, hipMemcpy(fresh.d(), cost, wd::TABLE, hipMemcpyHostToDevice));
    c->bigram = std::move(fresh);
    c->bigram_set = true;
    c->bigram_ee = cost[wd::E * wd::STATES + wd::E];
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_bigram_info(const str_er_ctx *c, int32_t *set, uint64_t *device_bytes)
{
    if (!c) return STR_ER_EINVAL;
    if (set) *set = c->bigram_set ? 1 : 0;
    if (device_bytes) *device_bytes = c->bigram_set ? c->bigram.size() : 0;
    return STR_ER_OK;
}

int str_er_set_word_decode(str_er_ctx *c, int32_t ins, int32_t del)
try {
    if (!c) return STR_ER_EINVAL;
    if (!wd::params_ok(ins, del)) return fail(c, STR_ER_EINVAL, "word decode: INS and DEL are in 0 .. 255");
    c->wd_ins = ins; c->wd_del = del;
    ++c->decode_pool_gen;          // (a decode pool is bound to them: str_er_pool_decode)
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_bigram_from_probs(const double *tp, const double *start, const double *end, uint8_t out[4356])
{
    if (!tp || !out) return STR_ER_EINVAL;
    wd::table_from_probs(tp, start, end, out);
    return STR_ER_OK;
}

int str_er_decode_words(str_er_ctx *c, const uint8_t *costs, int32_t n_runs, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words,
                        str_er_word_decode *dec, uint8_t *chars, uint8_t *src)
try {
    if (!c) return STR_ER_EINVAL;
    if (!args_ok(costs, n_runs, first_run, n_runs_of_word, n_words, dec, chars, src)) return fail(c, STR_ER_EINVAL, "bad arguments");
    if (!c->bigram_set) return fail(c, STR_ER_ESTATE, "str_er_decode_words needs a bigram table (str_er_set_bigram)");
    if (!words_in_rows(n_runs, first_run, n_runs_of_word, n_words)) return fail(c, STR_ER_EINVAL, "word decode: a word outside the cost rows");
    if (n_words == 0) return STR_ER_OK;
    const size_t at = rows_in_layout(nullptr, 0, (size_t)n_runs, (size_t)n_words, false).bytes;
    if (const int rc = c->wd_tab.ensure(c, wd_layout(nullptr, at, (size_t)n_words).bytes, "word decode tables"); rc != STR_ER_OK) return rc;
    const WdTab H = wd_layout(c->wd_tab.h(), at, (size_t)n_words), D = wd_layout(c->wd_tab.d(), at, (size_t)n_words);
    hipStream_t s = c->stream;
    RowsIn      I{};
    if (const int rc = rows_in_upload(c, s, c->wd_tab, nullptr, costs, (size_t)n_runs, nullptr, 0, first_run, n_runs_of_word, nullptr, (size_t)n_words, I); rc != STR_ER_OK) return rc;
    launch_word_decode(s, c->bigram.d(), c->wd_ins, c->wd_del, I.costs, I.first, I.n_of, n_words, D.dec, D.chars, D.src);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->wd_tab.h() + H.o_dec, c->wd_tab.d() + H.o_dec, H.down_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    std::memcpy(dec, H.dec, sizeof(str_er_word_decode) * (size_t)n_words);
    std::memcpy(chars, H.chars, wd::MAX_CHARS * (size_t)n_words);
    std::memcpy(src, H.src, wd::MAX_CHARS * (size_t)n_words);
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_decode_words_host(const uint8_t *costs, int32_t n_runs, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words,
                             const uint8_t *bigram, int32_t ins, int32_t del, str_er_word_decode *dec, uint8_t *chars, uint8_t *src)
{
    if (!args_ok(costs, n_runs, first_run, n_runs_of_word, n_words, dec, chars, src) || !bigram) return STR_ER_EINVAL;
    if (!wd::params_ok(ins, del) || !words_in_rows(n_runs, first_run, n_runs_of_word, n_words)) return STR_ER_EINVAL;
    for (int32_t w = 0; w < n_words; ++w)
        dec[w] = wd::decode_word(costs + (size_t)first_run[w] * wd::ALPHABET, n_runs_of_word[w], bigram, ins, del, chars + (size_t)w * wd::MAX_CHARS,
                                 src + (size_t)w * wd::MAX_CHARS);
    return STR_ER_OK;
}

const str_er_word_decode *str_er_result_word_decodes(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_word_decodes, &str_er_result::word_decodes, n);
}
const uint8_t *str_er_result_word_decode_chars(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_word_decodes, &str_er_result::word_decode_chars, n_bytes);
}
const uint8_t *str_er_result_word_decode_src(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_word_decodes, &str_er_result::word_decode_src, n_bytes);
}

} // extern "C"
