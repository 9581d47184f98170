// api_lattice_match.cpp -- the C ABI, part 8i: the lexicon match of a word over its piece lattice (STR_ER_WANT_LATTICE_MATCH behind the
// reading of the runs in api_run_read.cpp, str_er_lattice_match_words on the caller's rows; the contract is at str_er_lattice_match in
// str_er.h).  The rules are lattice_match_rules.h: the pure host entry point here runs them as they stand; k_lattice_match
// (lattice_match_kernels.h) reads what k_split_words reads and the lexicon as str_er_set_lexicon laid it out for the matcher.
#include "str_er_ctx.h"
#include "lattice_match_kernels.h"
#include "lattice_match_rules.h"

namespace lm = str_er_lm;
namespace rs = str_er_rs;
namespace wm = str_er_wm;

static_assert(sizeof(str_er_lattice_match) == 40, "lattice match layout");
static_assert(lm::MAX_NODES == rs::MAX_PARTS && lm::SRC_BYTES == wm::MAX_LEN, "a matched word's parts fit the matcher's limit, a source byte a character");

namespace str_er_host {

LmTab lm_layout(uint8_t *base, size_t at, size_t n_words, size_t n_slots, int n_chunks)
{
    LmTab t{};
    Carve cv{at};
    const size_t o_part = cv.take(16 * n_words * (size_t)n_chunks);
    t.o_matches = cv.take(sizeof(str_er_lattice_match) * n_words);
    const size_t o_src = cv.take(lm::SRC_BYTES * n_words), o_parts = cv.take(sizeof(str_er_split_part) * n_slots);
    t.bytes = cv.off;
    t.down_bytes = cv.off - t.o_matches;
    if (base) {
        t.partial = reinterpret_cast<uint64_t *>(base + o_part); t.matches = reinterpret_cast<str_er_lattice_match *>(base + t.o_matches);
        t.src = base + o_src; t.parts = reinterpret_cast<str_er_split_part *>(base + o_parts);
    }
    return t;
}

bool lm_compact(const LmTab &H, const std::vector<int32_t> &slot, uint64_t n_slots, str_er_lattice_match *matches, str_er_split_part *parts, uint64_t *n_parts)
{
    const size_t nw = slot.size();
    uint64_t     at = 0;
    for (size_t w = 0; w < nw; ++w) {
        const int32_t  np_w = H.matches[w].n_parts;
        const uint64_t atoms = (w + 1 < nw ? (uint64_t)slot[w + 1] : n_slots) - (uint64_t)slot[w];
        if (np_w < 0 || (uint64_t)np_w > atoms) return false;
        if (matches) { matches[w] = H.matches[w]; matches[w].first_part = (int32_t)at; }
        if (parts && np_w > 0) std::memcpy(parts + at, H.parts + (size_t)slot[w], sizeof(str_er_split_part) * (size_t)np_w);
        at += (uint64_t)np_w;
    }
    *n_parts = at;
    return true;
}

} // namespace str_er_host

namespace {

bool args_ok(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces, const int32_t *first_run,
             const int32_t *n_of, int32_t n_words, const str_er_lattice_match *matches, const uint8_t *src, const str_er_split_part *parts, int32_t cap_parts,
             const int32_t *n_parts)
{
    return n_runs >= 0 && n_pieces >= 0 && n_words >= 0 && cap_parts >= 0 && n_parts && (n_runs == 0 || (splits && run_costs)) && (n_pieces == 0 || piece_costs) &&
           (n_words == 0 || (first_run && n_of && matches && src)) && (cap_parts == 0 || parts);
}

} // namespace

extern "C" {

int str_er_lattice_match_stats(const str_er_ctx *c, uint64_t *table_bytes)
{
    if (!c) return STR_ER_EINVAL;
    if (table_bytes) *table_bytes = c->lm_tab.size();
    return STR_ER_OK;
}

int str_er_lattice_match_words(str_er_ctx *c, const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                               const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, str_er_lattice_match *matches, uint8_t *src,
                               str_er_split_part *parts, int32_t cap_parts, int32_t *n_parts)
try {
    using namespace str_er_host;
    if (!c) return STR_ER_EINVAL;
    if (!args_ok(splits, n_runs, run_costs, piece_costs, n_pieces, first_run, n_runs_of_word, n_words, matches, src, parts, cap_parts, n_parts))
        return fail(c, STR_ER_EINVAL, "bad arguments");
    *n_parts = 0;
    if (c->lex_n <= 0) return fail(c, STR_ER_ESTATE, "str_er_lattice_match_words needs a lexicon (str_er_set_lexicon)");
    if (!rs::splits_ok(splits, n_runs, n_pieces)) return fail(c, STR_ER_EINVAL, "lattice match: a record with cuts or pieces that are none");
    if (!words_in_rows(n_runs, first_run, n_runs_of_word, n_words)) return fail(c, STR_ER_EINVAL, "lattice match: a word outside the glyph runs");
    if (n_words == 0) return STR_ER_OK;
    std::vector<int32_t> slot;
    uint64_t             n_slots = 0;
    if (!rs_word_slots(splits, first_run, n_runs_of_word, (size_t)n_words, slot, &n_slots)) return fail(c, STR_ER_ECAPACITY, "lattice match: more than 2^31 parts to reserve");
    const size_t nr = (size_t)n_runs, np = (size_t)n_pieces, nw = (size_t)n_words;
    if (nr + np > 0x7FFFFFFFull / 65 || nw > 0x7FFFFFFFull / 64) return fail(c, STR_ER_ECAPACITY, "lattice match: too many rows or words");
    const int    n_chunks = wm_chunks(c->lex);
    const size_t at = rows_in_layout(nullptr, nr, nr + np, nw, true).bytes;
    if (const int rc = c->lm_tab.ensure(c, lm_layout(nullptr, at, nw, (size_t)n_slots, n_chunks).bytes, "lattice match tables"); rc != STR_ER_OK) return rc;
    const LmTab H = lm_layout(c->lm_tab.h(), at, nw, (size_t)n_slots, n_chunks), D = lm_layout(c->lm_tab.d(), at, nw, (size_t)n_slots, n_chunks);
    hipStream_t s = c->stream;
    RowsIn      I{};
    if (const int rc = rows_in_upload(c, s, c->lm_tab, splits, run_costs, nr, piece_costs, np, first_run, n_runs_of_word, slot.data(), nw, I); rc != STR_ER_OK) return rc;
    launch_lattice_match(s, c->lex, c->wm_prm, c->rs_split, I.splits, I.costs, I.costs + rs::ALPHABET * nr, I.first, I.n_of, I.slot, n_words, D.partial,
                         reinterpret_cast<int32_t *>(D.matches), D.src, reinterpret_cast<int32_t *>(D.parts));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->lm_tab.h() + H.o_matches, c->lm_tab.d() + H.o_matches, H.down_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    uint64_t total = 0;
    if (!lm_compact(H, slot, n_slots, nullptr, nullptr, &total)) return fail(c, STR_ER_EHIP, "lattice match: a word's parts outside its slots (internal error)");
    *n_parts = (int32_t)total;
    if (total > (uint64_t)cap_parts) return fail(c, STR_ER_ECAPACITY, std::to_string(total) + " parts, cap_parts is " + std::to_string(cap_parts));
    lm_compact(H, slot, n_slots, matches, parts, &total);
    std::memcpy(src, H.src, lm::SRC_BYTES * nw);
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_lattice_match_words_host(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                                    const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, const char *bytes, const int32_t *offsets, int32_t n,
                                    uint32_t flags, int32_t ins, int32_t del, int32_t band, int32_t split_cost, str_er_lattice_match *matches, uint8_t *src,
                                    str_er_split_part *parts, int32_t cap_parts, int32_t *n_parts)
try {
    using namespace str_er_host;
    if (!args_ok(splits, n_runs, run_costs, piece_costs, n_pieces, first_run, n_runs_of_word, n_words, matches, src, parts, cap_parts, n_parts)) return STR_ER_EINVAL;
    *n_parts = 0;
    if (const int rc = wm::lexicon_check(bytes, offsets, n, flags, nullptr); rc != STR_ER_OK) return rc;
    if (!lm::params_ok(ins, del, band, split_cost) || !rs::splits_ok(splits, n_runs, n_pieces) || !words_in_rows(n_runs, first_run, n_runs_of_word, n_words))
        return STR_ER_EINVAL;
    // every word once, its parts behind those of the words before it; the count is set even where cap_parts is too small, and nothing
    // is written to the caller's arrays before it is known to fit
    const std::vector<uint8_t> lab = lexicon_labels(bytes, offsets, n);
    const int32_t              zero = 0;
    const lm::Params           p{ins, del, band, split_cost};
    std::vector<str_er_lattice_match> recs((size_t)n_words);
    std::vector<str_er_split_part>    all;
    std::vector<uint8_t>              from(lm::SRC_BYTES * (size_t)n_words);
    for (int32_t w = 0; w < n_words; ++w) {
        const size_t at = all.size();
        all.resize(at + lm::MAX_NODES);
        str_er_lattice_match &R = recs[(size_t)w];
        R = lm::match_word(splits, run_costs, piece_costs, first_run[w], n_runs_of_word[w], lab.data(), n > 0 ? offsets : &zero, n, p,
                           (flags & STR_ER_LEXICON_FOLD_CASE) != 0, from.data() + lm::SRC_BYTES * (size_t)w, all.data() + at);
        R.first_part = (int32_t)at;
        all.resize(at + (size_t)R.n_parts);
        if (all.size() > 0x7FFFFFFFull) return STR_ER_ECAPACITY;
    }
    *n_parts = (int32_t)all.size();
    if (all.size() > (size_t)cap_parts) return STR_ER_ECAPACITY;
    if (n_words > 0) {
        std::memcpy(matches, recs.data(), sizeof(str_er_lattice_match) * recs.size());
        std::memcpy(src, from.data(), from.size());
    }
    if (!all.empty()) std::memcpy(parts, all.data(), sizeof(str_er_split_part) * all.size());
    return STR_ER_OK;
} catch (...) { return STR_ER_ENOMEM; }

const str_er_lattice_match *str_er_result_lattice_matches(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_lattice_matches, &str_er_result::lattice_matches, n);
}
const uint8_t *str_er_result_lattice_match_src(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_lattice_matches, &str_er_result::lattice_match_src, n_bytes);
}
const str_er_split_part *str_er_result_lattice_match_parts(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_lattice_matches, &str_er_result::lattice_match_parts, n);
}

} // extern "C"
