// api_lattice_decode.cpp -- the C ABI, part 8h: the joint decode of a word over its piece lattice and the bigram table
// (STR_ER_WANT_LATTICE_DECODE behind the reading of the runs in api_run_read.cpp, str_er_lattice_decode_words on the caller's rows; the
// contract is at str_er_lattice_decode in str_er.h).  The rules are lattice_decode_rules.h: the pure host entry point here runs them as
// they stand; k_lattice_decode (lattice_decode_kernels.h) reads what k_split_words reads and the table as the caller gave it.
#include "str_er_ctx.h"
#include "lattice_decode_kernels.h"
#include "lattice_decode_rules.h"

namespace ld = str_er_ld;
namespace rs = str_er_rs;

static_assert(sizeof(str_er_lattice_decode) == 32, "lattice decode layout");
static_assert(ld::MAX_NODES == rs::MAX_PARTS, "a decoded word's parts fit the limit of the matcher and the decoder");

namespace str_er_host {

LdTab ld_layout(uint8_t *base, size_t at, size_t n_words, size_t n_slots)
{
    LdTab t{};
    Carve cv{at};
    t.o_dec = cv.take(sizeof(str_er_lattice_decode) * n_words);
    const size_t o_chars = cv.take(ld::MAX_CHARS * n_words), o_src = cv.take(ld::MAX_CHARS * n_words), o_parts = cv.take(sizeof(str_er_split_part) * n_slots);
    t.bytes = cv.off;
    t.down_bytes = cv.off - t.o_dec;
    if (base) {
        t.dec = reinterpret_cast<str_er_lattice_decode *>(base + t.o_dec); t.chars = base + o_chars; t.src = base + o_src;
        t.parts = reinterpret_cast<str_er_split_part *>(base + o_parts);
    }
    return t;
}

bool ld_compact(const LdTab &H, const std::vector<int32_t> &slot, uint64_t n_slots, str_er_lattice_decode *dec, str_er_split_part *parts, uint64_t *n_parts)
{
    const size_t nw = slot.size();
    uint64_t     at = 0;
    for (size_t w = 0; w < nw; ++w) {
        const int32_t  np_w = H.dec[w].n_parts;
        const uint64_t atoms = (w + 1 < nw ? (uint64_t)slot[w + 1] : n_slots) - (uint64_t)slot[w];
        if (np_w < 0 || (uint64_t)np_w > atoms) return false;
        if (dec) { dec[w] = H.dec[w]; dec[w].first_part = (int32_t)at; }
        if (parts && np_w > 0) std::memcpy(parts + at, H.parts + (size_t)slot[w], sizeof(str_er_split_part) * (size_t)np_w);
        at += (uint64_t)np_w;
    }
    *n_parts = at;
    return true;
}

} // namespace str_er_host

namespace {

bool args_ok(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces, const int32_t *first_run,
             const int32_t *n_of, int32_t n_words, const str_er_lattice_decode *dec, const uint8_t *chars, const uint8_t *src, const str_er_split_part *parts,
             int32_t cap_parts, const int32_t *n_parts)
{
    return n_runs >= 0 && n_pieces >= 0 && n_words >= 0 && cap_parts >= 0 && n_parts && (n_runs == 0 || (splits && run_costs)) && (n_pieces == 0 || piece_costs) &&
           (n_words == 0 || (first_run && n_of && dec && chars && src)) && (cap_parts == 0 || parts);
}

} // namespace

extern "C" {

int str_er_lattice_decode_stats(const str_er_ctx *c, uint64_t *table_bytes)
{
    if (!c) return STR_ER_EINVAL;
    if (table_bytes) *table_bytes = c->ld_tab.size();
    return STR_ER_OK;
}

int str_er_lattice_decode_words(str_er_ctx *c, const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                                const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, str_er_lattice_decode *dec, uint8_t *chars, uint8_t *src,
                                str_er_split_part *parts, int32_t cap_parts, int32_t *n_parts)
try {
    using namespace str_er_host;
    if (!c) return STR_ER_EINVAL;
    if (!args_ok(splits, n_runs, run_costs, piece_costs, n_pieces, first_run, n_runs_of_word, n_words, dec, chars, src, parts, cap_parts, n_parts))
        return fail(c, STR_ER_EINVAL, "bad arguments");
    *n_parts = 0;
    if (!c->bigram_set) return fail(c, STR_ER_ESTATE, "str_er_lattice_decode_words needs a bigram table (str_er_set_bigram)");
    if (!rs::splits_ok(splits, n_runs, n_pieces)) return fail(c, STR_ER_EINVAL, "lattice decode: a record with cuts or pieces that are none");
    if (!words_in_rows(n_runs, first_run, n_runs_of_word, n_words)) return fail(c, STR_ER_EINVAL, "lattice decode: a word outside the glyph runs");
    if (n_words == 0) return STR_ER_OK;
    std::vector<int32_t> slot;
    uint64_t             n_slots = 0;
    if (!rs_word_slots(splits, first_run, n_runs_of_word, (size_t)n_words, slot, &n_slots)) return fail(c, STR_ER_ECAPACITY, "lattice decode: more than 2^31 parts to reserve");
    const size_t nr = (size_t)n_runs, np = (size_t)n_pieces, nw = (size_t)n_words;
    if (nr + np > 0x7FFFFFFFull / 65 || nw > 0x7FFFFFFFull / 64) return fail(c, STR_ER_ECAPACITY, "lattice decode: too many rows or words");
    const size_t at = rows_in_layout(nullptr, nr, nr + np, nw, true).bytes;
    if (const int rc = c->ld_tab.ensure(c, ld_layout(nullptr, at, nw, (size_t)n_slots).bytes, "lattice decode tables"); rc != STR_ER_OK) return rc;
    const LdTab H = ld_layout(c->ld_tab.h(), at, nw, (size_t)n_slots), D = ld_layout(c->ld_tab.d(), at, nw, (size_t)n_slots);
    hipStream_t s = c->stream;
    RowsIn      I{};
    if (const int rc = rows_in_upload(c, s, c->ld_tab, splits, run_costs, nr, piece_costs, np, first_run, n_runs_of_word, slot.data(), nw, I); rc != STR_ER_OK) return rc;
    launch_lattice_decode(s, c->bigram.d(), c->wd_ins, c->wd_del, c->rs_split, I.splits, I.costs, I.costs + rs::ALPHABET * nr, I.first, I.n_of, I.slot, n_words,
                          reinterpret_cast<int32_t *>(D.dec), D.chars, D.src, reinterpret_cast<int32_t *>(D.parts));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->ld_tab.h() + H.o_dec, c->ld_tab.d() + H.o_dec, H.down_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    uint64_t total = 0;
    if (!ld_compact(H, slot, n_slots, nullptr, nullptr, &total)) return fail(c, STR_ER_EHIP, "lattice decode: a word's parts outside its slots (internal error)");
    *n_parts = (int32_t)total;
    if (total > (uint64_t)cap_parts) return fail(c, STR_ER_ECAPACITY, std::to_string(total) + " parts, cap_parts is " + std::to_string(cap_parts));
    ld_compact(H, slot, n_slots, dec, parts, &total);
    std::memcpy(chars, H.chars, ld::MAX_CHARS * nw);
    std::memcpy(src, H.src, ld::MAX_CHARS * nw);
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_lattice_decode_words_host(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                                     const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, int32_t split_cost, const uint8_t *bigram,
                                     int32_t ins, int32_t del, str_er_lattice_decode *dec, uint8_t *chars, uint8_t *src, str_er_split_part *parts,
                                     int32_t cap_parts, int32_t *n_parts)
try {
    if (!args_ok(splits, n_runs, run_costs, piece_costs, n_pieces, first_run, n_runs_of_word, n_words, dec, chars, src, parts, cap_parts, n_parts) || !bigram)
        return STR_ER_EINVAL;
    *n_parts = 0;
    if (!ld::params_ok(ins, del, split_cost) || !rs::splits_ok(splits, n_runs, n_pieces) || !words_in_rows(n_runs, first_run, n_runs_of_word, n_words)) return STR_ER_EINVAL;
    // every word once, its parts behind those of the words before it; the count is set even where cap_parts is too small, and nothing
    // is written to the caller's arrays before it is known to fit
    std::vector<str_er_lattice_decode> recs((size_t)n_words);
    std::vector<str_er_split_part>     all;
    std::vector<uint8_t>               lab(ld::MAX_CHARS * (size_t)n_words), from(ld::MAX_CHARS * (size_t)n_words);
    for (int32_t w = 0; w < n_words; ++w) {
        const size_t at = all.size();
        all.resize(at + ld::MAX_NODES);
        str_er_lattice_decode &R = recs[(size_t)w];
        R = ld::decode_word(splits, run_costs, piece_costs, first_run[w], n_runs_of_word[w], bigram, ins, del, split_cost, lab.data() + ld::MAX_CHARS * (size_t)w,
                            from.data() + ld::MAX_CHARS * (size_t)w, all.data() + at);
        R.first_part = (int32_t)at;
        all.resize(at + (size_t)R.n_parts);
        if (all.size() > 0x7FFFFFFFull) return STR_ER_ECAPACITY;
    }
    *n_parts = (int32_t)all.size();
    if (all.size() > (size_t)cap_parts) return STR_ER_ECAPACITY;
    if (n_words > 0) {
        std::memcpy(dec, recs.data(), sizeof(str_er_lattice_decode) * recs.size());
        std::memcpy(chars, lab.data(), lab.size());
        std::memcpy(src, from.data(), from.size());
    }
    if (!all.empty()) std::memcpy(parts, all.data(), sizeof(str_er_split_part) * all.size());
    return STR_ER_OK;
} catch (...) { return STR_ER_ENOMEM; }

const str_er_lattice_decode *str_er_result_lattice_decodes(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_lattice_decodes, &str_er_result::lattice_decodes, n);
}
const uint8_t *str_er_result_lattice_decode_chars(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_lattice_decodes, &str_er_result::lattice_decode_chars, n_bytes);
}
const uint8_t *str_er_result_lattice_decode_src(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_lattice_decodes, &str_er_result::lattice_decode_src, n_bytes);
}
const str_er_split_part *str_er_result_lattice_parts(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_lattice_decodes, &str_er_result::lattice_parts, n);
}

} // extern "C"
