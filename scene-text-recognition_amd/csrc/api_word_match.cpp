// api_word_match.cpp -- the C ABI, part 8d: the lexicon matcher (STR_ER_WANT_WORD_MATCH behind the reading of the runs in api_run_read.cpp,
// str_er_match_words on the caller's cost rows, str_er_run_costs on the caller's probabilities; the contract is at str_er_word_match in
// str_er.h).  The rules are word_match_rules.h: the pure host entry points here run them as they stand, and set_lexicon lays the lexicon
// out for k_word_match (word_match_kernels.h: sorted by length, stable by index, padded to whole groups of 64, four characters a word).
#include "str_er_ctx.h"
#include "word_match_rules.h"

namespace wm = str_er_wm;

static_assert(sizeof(str_er_word_match) == 24, "word match layout");
static_assert(WM_GROUP == 64, "a lane an entry");

namespace str_er_host {

RowsIn rows_in_layout(uint8_t *base, size_t n_splits, size_t n_rows, size_t n_words, bool slots)
{
    RowsIn t{};
    Carve  cv;
    const size_t o_sp = cv.take(sizeof(str_er_run_split) * n_splits), o_costs = cv.take(wm::ALPHABET * n_rows);
    const size_t o_first = cv.take(4 * n_words), o_nof = cv.take(4 * n_words), o_slot = cv.take(slots ? 4 * n_words : 0);
    t.bytes = cv.off;
    if (base) {
        t.splits = reinterpret_cast<str_er_run_split *>(base + o_sp); t.costs = base + o_costs;
        t.first = reinterpret_cast<int32_t *>(base + o_first); t.n_of = reinterpret_cast<int32_t *>(base + o_nof); t.slot = reinterpret_cast<int32_t *>(base + o_slot);
    }
    return t;
}

int rows_in_upload(str_er_ctx *c, hipStream_t s, PairBuf &buf, const str_er_run_split *splits, const uint8_t *run_costs, size_t n_runs, const uint8_t *piece_costs,
                   size_t n_pieces, const int32_t *first, const int32_t *n_of, const int32_t *slot, size_t n_words, RowsIn &D)
{
    const size_t n_splits = splits ? n_runs : 0, n_rows = n_runs + n_pieces;
    const RowsIn H = rows_in_layout(buf.h(), n_splits, n_rows, n_words, slot != nullptr);
    D = rows_in_layout(buf.d(), n_splits, n_rows, n_words, slot != nullptr);
    if (n_splits > 0) std::memcpy(H.splits, splits, sizeof(str_er_run_split) * n_splits);
    if (n_runs > 0) std::memcpy(H.costs, run_costs, wm::ALPHABET * n_runs);
    if (n_pieces > 0) std::memcpy(H.costs + wm::ALPHABET * n_runs, piece_costs, wm::ALPHABET * n_pieces);          // (the pieces' rows behind the runs')
    if (n_words > 0) {
        std::memcpy(H.first, first, 4 * n_words); std::memcpy(H.n_of, n_of, 4 * n_words);
        if (slot) std::memcpy(H.slot, slot, 4 * n_words);
    }
    HIP_TRY(c, hipMemcpyAsync(buf.d(), buf.h(), H.bytes, hipMemcpyHostToDevice, s));
    return STR_ER_OK;
}

WmTab wm_layout(uint8_t *base, size_t at, size_t n_words, int n_chunks)
{
    WmTab t{};
    Carve cv{at};
    const size_t o_part = cv.take(16 * n_words * (size_t)n_chunks);
    t.o_matches = cv.take(sizeof(str_er_word_match) * n_words);
    t.bytes = cv.off;
    if (base) { t.partial = reinterpret_cast<uint64_t *>(base + o_part); t.matches = reinterpret_cast<str_er_word_match *>(base + t.o_matches); }
    return t;
}

std::vector<uint8_t> lexicon_labels(const char *bytes, const int32_t *offsets, int32_t n)
{
    std::vector<uint8_t> lab(n > 0 ? (size_t)offsets[n] : 0);
    for (size_t i = 0; i < lab.size(); ++i) lab[i] = (uint8_t)wm::char_label((unsigned char)bytes[i]);
    return lab;
}

} // namespace str_er_host

extern "C" {

int str_er_set_lexicon(str_er_ctx *c, const char *bytes, const int32_t *offsets, int32_t n, uint32_t flags)
try {
    if (!c) return STR_ER_EINVAL;
    const char *why = nullptr;
    if (const int rc = wm::lexicon_check(bytes, offsets, n, flags, &why); rc != STR_ER_OK) return fail(c, rc, why);
    HIP_TRY(c, hipStreamSynchronize(c->stream));       // (a call in flight still reads the lexicon that is replaced)
    ++c->pool_gen;          // (a track pool is bound to the lexicon it was made with: str_er_pool_match)
    if (n == 0) {
        c->lexicon = DevBuf();
        c->lex = WmLexDev{};
        c->lex_n = 0; c->lex_flags = 0;
        return STR_ER_OK;
    }
    // the groups: the entries of every length in the order given, 64 a group
    WmLexDev L{};
    int32_t  count[34] = {}, len_first[34] = {}, len_count[34] = {};
    for (int32_t e = 0; e < n; ++e) ++count[offsets[e + 1] - offsets[e]];
    size_t n_words32 = 0;
    for (int len = 1; len <= 32; ++len) {
        const int32_t groups = (count[len] + WM_GROUP - 1) / WM_GROUP;
        len_first[len + 1] = len_first[len] + groups;
        len_count[len + 1] = len_count[len] + count[len];
        n_words32 += (size_t)groups * WM_GROUP * ((len + 3) / 4);
    }
    L.n_groups = len_first[33];      // ([0] = [1] = 0: no entry is shorter than 1)
    L.fold = (flags & STR_ER_LEXICON_FOLD_CASE) ? 1 : 0;
    const size_t o_lens = 0, o_goff = 512, o_index = align_up(o_goff + 4 * (size_t)L.n_groups, 256), o_chars = align_up(o_index + 4 * (size_t)L.n_groups * WM_GROUP, 256),
                 o_pos = align_up(o_chars + 4 * n_words32, 256), total = o_pos + 4 * (size_t)n;
    std::vector<uint8_t> img(total, 0);
    uint32_t *goff = reinterpret_cast<uint32_t *>(img.data() + o_goff), *chars = reinterpret_cast<uint32_t *>(img.data() + o_chars);
    int32_t  *index = reinterpret_cast<int32_t *>(img.data() + o_index), *pos = reinterpret_cast<int32_t *>(img.data() + o_pos);
    std::fill(index, index + (size_t)L.n_groups * WM_GROUP, -1);
    std::memcpy(img.data() + o_lens, len_first, sizeof(len_first));
    std::memcpy(img.data() + o_lens + sizeof(len_first), len_count, sizeof(len_count));
    {
        size_t at = 0;
        for (int len = 1; len <= 32; ++len)
            for (int32_t g = len_first[len]; g < len_first[len + 1]; ++g) { goff[g] = (uint32_t)at; at += (size_t)WM_GROUP * ((len + 3) / 4); }
    }
    int32_t placed[34] = {};
    for (int32_t e = 0; e < n; ++e) {
        const int     len = offsets[e + 1] - offsets[e];
        const int32_t slot = placed[len]++, g = len_first[len] + slot / WM_GROUP, lane = slot % WM_GROUP;
        index[(size_t)g * WM_GROUP + lane] = e;
        pos[e] = g * WM_GROUP + lane;
        for (int j = 0; j < len; ++j)
            chars[goff[g] + (size_t)(j / 4) * WM_GROUP + lane] |= (uint32_t)wm::char_label((unsigned char)bytes[offsets[e] + j]) << (8 * (j % 4));
    }
    DevBuf fresh;
    if (const int rc = fresh.ensure(c, total, "lexicon"); rc != STR_ER_OK) return rc;
    HIP_TRY(c, hipMemcpy(fresh.d(), img.data(), total, hipMemcpyHostToDevice));
    c->lexicon = std::move(fresh);
    L.len_first = reinterpret_cast<const int32_t *>(c->lexicon.d() + o_lens); L.len_count = L.len_first + 34;
    L.goff = reinterpret_cast<const uint32_t *>(c->lexicon.d() + o_goff);
    L.index = reinterpret_cast<const int32_t *>(c->lexicon.d() + o_index);
    L.chars = reinterpret_cast<const uint32_t *>(c->lexicon.d() + o_chars);
    L.pos = reinterpret_cast<const int32_t *>(c->lexicon.d() + o_pos);
    c->lex = L;
    c->lex_n = n; c->lex_flags = flags;
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_lexicon_info(const str_er_ctx *c, int32_t *n, uint32_t *flags, int32_t *chunk_entries, uint64_t *device_bytes)
{
    if (!c) return STR_ER_EINVAL;
    if (n) *n = c->lex_n;
    if (flags) *flags = c->lex_flags;
    if (chunk_entries) *chunk_entries = WM_CHUNK;
    if (device_bytes) *device_bytes = c->lex_n > 0 ? c->lexicon.size() : 0;
    return STR_ER_OK;
}

int str_er_set_word_match(str_er_ctx *c, int32_t ins, int32_t del, int32_t band)
try {
    if (!c) return STR_ER_EINVAL;
    if (!wm::params_ok(ins, del, band)) return fail(c, STR_ER_EINVAL, "word match: INS and DEL are in 1 .. 255 and the band in 0 .. 31");
    c->wm_prm = WmParams{ins, del, band};
    ++c->pool_gen;          // (a track pool is bound to them: str_er_pool_match)
    return STR_ER_OK;
} ABI_GUARD(c)

void str_er_cost_thresholds(double out[255])
{
    if (out) wm::thresholds(out);
}

int str_er_prob_costs(const double *prob, int32_t n, int32_t k, const int32_t *labels, int32_t fold, uint8_t *cost_out)
{
    if (n < 0 || k < 0 || (n > 0 && (!cost_out || (k > 0 && (!prob || !labels))))) return STR_ER_EINVAL;
    double T[wm::N_THRESH];
    wm::thresholds(T);
    for (int32_t i = 0; i < n; ++i) wm::cost_row(prob + (size_t)i * k, k, labels, fold != 0, T, cost_out + (size_t)i * wm::ALPHABET);
    return STR_ER_OK;
}

int str_er_run_costs(str_er_ctx *c, const double *prob, int32_t n, uint8_t *cost_out)
try {
    if (!c) return STR_ER_EINVAL;
    if (n < 0 || (n > 0 && (!prob || !cost_out))) return fail(c, STR_ER_EINVAL, "bad arguments");
    if (!c->svm_loaded) return fail(c, STR_ER_ESTATE, "str_er_run_costs needs an SVM model (str_er_load_svm_model): the cost rows follow its labels");
    if (n == 0) return STR_ER_OK;
    const size_t k = (size_t)c->svm.k, in_bytes = align_up(8 * k * (size_t)n, 256), out_bytes = (size_t)n * wm::ALPHABET;
    if (const int rc = c->wm_tab.ensure(c, in_bytes + out_bytes, "word match tables"); rc != STR_ER_OK) return rc;
    hipStream_t s = c->stream;
    std::memcpy(c->wm_tab.h(), prob, 8 * k * (size_t)n);
    HIP_TRY(c, hipMemcpyAsync(c->wm_tab.d(), c->wm_tab.h(), 8 * k * (size_t)n, hipMemcpyHostToDevice, s));
    launch_run_costs(s, c->wm_tab.d<double>(), n, (int)k, c->svm.label, (c->lex_flags & STR_ER_LEXICON_FOLD_CASE) != 0, c->wm_tab.d() + in_bytes);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->wm_tab.h() + in_bytes, c->wm_tab.d() + in_bytes, out_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    std::memcpy(cost_out, c->wm_tab.h() + in_bytes, out_bytes);
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_match_words(str_er_ctx *c, const uint8_t *costs, int32_t n_runs, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words,
                       str_er_word_match *matches)
try {
    if (!c) return STR_ER_EINVAL;
    if (n_runs < 0 || n_words < 0 || (n_runs > 0 && !costs) || (n_words > 0 && (!first_run || !n_runs_of_word || !matches)))
        return fail(c, STR_ER_EINVAL, "bad arguments");
    if (c->lex_n <= 0) return fail(c, STR_ER_ESTATE, "str_er_match_words needs a lexicon (str_er_set_lexicon)");
    if (!words_in_rows(n_runs, first_run, n_runs_of_word, n_words)) return fail(c, STR_ER_EINVAL, "word match: a word outside the cost rows");
    if (n_words == 0) return STR_ER_OK;
    const int    n_chunks = wm_chunks(c->lex);
    const size_t at = rows_in_layout(nullptr, 0, (size_t)n_runs, (size_t)n_words, false).bytes;
    if (const int rc = c->wm_tab.ensure(c, wm_layout(nullptr, at, (size_t)n_words, n_chunks).bytes, "word match tables"); rc != STR_ER_OK) return rc;
    const WmTab H = wm_layout(c->wm_tab.h(), at, (size_t)n_words, n_chunks), D = wm_layout(c->wm_tab.d(), at, (size_t)n_words, n_chunks);
    hipStream_t s = c->stream;
    RowsIn      I{};
    if (const int rc = rows_in_upload(c, s, c->wm_tab, nullptr, costs, (size_t)n_runs, nullptr, 0, first_run, n_runs_of_word, nullptr, (size_t)n_words, I); rc != STR_ER_OK) return rc;
    launch_word_match(s, c->lex, c->wm_prm, I.costs, I.first, I.n_of, n_words, D.partial, D.matches);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(H.matches, D.matches, sizeof(str_er_word_match) * (size_t)n_words, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    std::memcpy(matches, H.matches, sizeof(str_er_word_match) * (size_t)n_words);
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_match_words_host(const uint8_t *costs, int32_t n_runs, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, const char *bytes,
                            const int32_t *offsets, int32_t n, uint32_t flags, int32_t ins, int32_t del, int32_t band, str_er_word_match *matches)
try {
    if (n_runs < 0 || n_words < 0 || (n_runs > 0 && !costs) || (n_words > 0 && (!first_run || !n_runs_of_word || !matches))) return STR_ER_EINVAL;
    if (const int rc = wm::lexicon_check(bytes, offsets, n, flags, nullptr); rc != STR_ER_OK) return rc;
    if (!wm::params_ok(ins, del, band) || !words_in_rows(n_runs, first_run, n_runs_of_word, n_words)) return STR_ER_EINVAL;
    const std::vector<uint8_t> lab = lexicon_labels(bytes, offsets, n);
    const int32_t          zero = 0;
    const wm::MatchParams  p{ins, del, band};
    for (int32_t w = 0; w < n_words; ++w)
        matches[w] = wm::match_word(costs + (size_t)first_run[w] * wm::ALPHABET, n_runs_of_word[w], lab.data(), n > 0 ? offsets : &zero, n, p,
                                    (flags & STR_ER_LEXICON_FOLD_CASE) != 0);
    return STR_ER_OK;
} catch (...) { return STR_ER_ENOMEM; }

const str_er_word_match *str_er_result_word_matches(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_word_matches, &str_er_result::word_matches, n);
}
const uint8_t *str_er_result_run_costs(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && (r->have_word_matches || r->have_word_decodes || r->have_run_splits), &str_er_result::run_costs, n_bytes);
}
const double *str_er_result_run_probs(const str_er_result *r, uint64_t *n_values)
{
    return result_table(r, r && (r->have_word_matches || r->have_word_decodes), &str_er_result::run_probs, n_values);
}

} // extern "C"
