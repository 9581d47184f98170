// api_lattice_margin.cpp -- the C ABI, part 8l: the margins of the lattice decoder (str_er_set_lattice_margin beside
// STR_ER_WANT_LATTICE_DECODE behind the decoder in api_run_read.cpp, str_er_lattice_margins on the caller's rows; the contract is at
// str_er_lattice_margin in str_er.h).  The rules are lattice_margin_rules.h: the pure host entry point here runs them as they stand;
// k_lattice_margin (lattice_margin_kernels.h) reads what k_lattice_decode read and left for the same words.
#include "str_er_ctx.h"
#include "lattice_decode_kernels.h"
#include "lattice_margin_rules.h"

namespace ld = str_er_ld;
namespace rs = str_er_rs;

static_assert(sizeof(str_er_lattice_margin) == 32, "lattice margin layout");
static_assert(ld::MAX_PARTS == str_er::LM_PARTS && ld::MAX_FROM == str_er::LM_FROM && ld::MARGINALS == str_er::LM_READINGS, "the kernel's layout is the rules'");

namespace str_er_host {

LgTab lg_layout(uint8_t *base, size_t at, size_t n_words, bool edge_min, bool marginals)
{
    LgTab t{};
    Carve cv{at};
    t.o_out = cv.take(sizeof(str_er_lattice_margin) * n_words);
    const size_t o_rm = cv.take(4 * ld::MAX_PARTS * n_words), o_cm = cv.take(4 * ld::MAX_PARTS * n_words), o_rd = cv.take(ld::MAX_PARTS * n_words),
                 o_al = cv.take(ld::MAX_PARTS * n_words), o_ca = cv.take(ld::MAX_PARTS * n_words),
                 o_em = cv.take(edge_min ? 4 * (size_t)ld::MAX_NODES * ld::MAX_FROM * n_words : 0),
                 o_mg = cv.take(marginals ? 4 * (size_t)ld::MAX_NODES * ld::MAX_FROM * ld::MARGINALS * n_words : 0);
    t.bytes = cv.off;
    t.down_bytes = cv.off - t.o_out;
    if (base) {
        t.margins = reinterpret_cast<str_er_lattice_margin *>(base + t.o_out);
        t.read_margin = reinterpret_cast<int32_t *>(base + o_rm); t.cut_margin = reinterpret_cast<int32_t *>(base + o_cm);
        t.read = base + o_rd; t.alt = base + o_al; t.cut_alt = base + o_ca;
        t.edge_min = edge_min ? reinterpret_cast<int32_t *>(base + o_em) : nullptr;
        t.marginals = marginals ? reinterpret_cast<int32_t *>(base + o_mg) : nullptr;
    }
    return t;
}

} // namespace str_er_host

namespace {

bool args_ok(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces, const int32_t *first_run,
             const int32_t *n_of, int32_t n_words, const str_er_lattice_margin *margins, const int32_t *read_margin, const int32_t *cut_margin, const uint8_t *read,
             const uint8_t *alt, const uint8_t *cut_alt)
{
    return n_runs >= 0 && n_pieces >= 0 && n_words >= 0 && (n_runs == 0 || (splits && run_costs)) && (n_pieces == 0 || piece_costs) &&
           (n_words == 0 || (first_run && n_of && margins && read_margin && cut_margin && read && alt && cut_alt));
}

} // namespace

extern "C" {

int str_er_set_lattice_margin(str_er_ctx *c, int32_t on)
try {
    if (!c) return STR_ER_EINVAL;
    c->ld_margin = on != 0;
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_lattice_margins(str_er_ctx *c, const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                           const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, str_er_lattice_margin *margins, int32_t *read_margin,
                           int32_t *cut_margin, uint8_t *read, uint8_t *alt, uint8_t *cut_alt, int32_t *edge_min, int32_t *marginals)
try {
    using namespace str_er_host;
    if (!c) return STR_ER_EINVAL;
    if (!args_ok(splits, n_runs, run_costs, piece_costs, n_pieces, first_run, n_runs_of_word, n_words, margins, read_margin, cut_margin, read, alt, cut_alt))
        return fail(c, STR_ER_EINVAL, "bad arguments");
    if (!c->bigram_set) return fail(c, STR_ER_ESTATE, "str_er_lattice_margins needs a bigram table (str_er_set_bigram)");
    if (!rs::splits_ok(splits, n_runs, n_pieces)) return fail(c, STR_ER_EINVAL, "lattice margins: a record with cuts or pieces that are none");
    if (!words_in_rows(n_runs, first_run, n_runs_of_word, n_words)) return fail(c, STR_ER_EINVAL, "lattice margins: a word outside the glyph runs");
    if (n_words == 0) return STR_ER_OK;
    std::vector<int32_t> slot;
    uint64_t             n_slots = 0;
    if (!rs_word_slots(splits, first_run, n_runs_of_word, (size_t)n_words, slot, &n_slots)) return fail(c, STR_ER_ECAPACITY, "lattice margins: more than 2^31 parts to reserve");
    const size_t nr = (size_t)n_runs, np = (size_t)n_pieces, nw = (size_t)n_words;
    if (nr + np > 0x7FFFFFFFull / 65 || nw > 0x7FFFFFFFull / 64) return fail(c, STR_ER_ECAPACITY, "lattice margins: too many rows or words");
    // the rows and words | the decoder's tables (scratch: they stay on the device) | the margins' tables
    const size_t at_dec = rows_in_layout(nullptr, nr, nr + np, nw, true).bytes, at = ld_layout(nullptr, at_dec, nw, (size_t)n_slots).bytes;
    const bool   em = edge_min != nullptr, mg = marginals != nullptr;
    if (const int rc = c->lg_tab.ensure(c, lg_layout(nullptr, at, nw, em, mg).bytes, "lattice margin tables"); rc != STR_ER_OK) return rc;
    const LdTab W = ld_layout(c->lg_tab.d(), at_dec, nw, (size_t)n_slots);
    const LgTab H = lg_layout(c->lg_tab.h(), at, nw, em, mg), D = lg_layout(c->lg_tab.d(), at, nw, em, mg);
    hipStream_t s = c->stream;
    RowsIn      I{};
    if (const int rc = rows_in_upload(c, s, c->lg_tab, splits, run_costs, nr, piece_costs, np, first_run, n_runs_of_word, slot.data(), nw, I); rc != STR_ER_OK) return rc;
    str_er::launch_lattice_decode(s, c->bigram.d(), c->wd_ins, c->wd_del, c->rs_split, I.splits, I.costs, I.costs + rs::ALPHABET * nr, I.first, I.n_of, I.slot, n_words,
                                  reinterpret_cast<int32_t *>(W.dec), W.chars, W.src, reinterpret_cast<int32_t *>(W.parts));
    str_er::launch_lattice_margin(s, c->bigram.d(), c->wd_ins, c->wd_del, c->rs_split, I.splits, I.costs, I.costs + rs::ALPHABET * nr, I.first, I.n_of, I.slot, n_words,
                                  reinterpret_cast<const int32_t *>(W.dec), W.chars, W.src, reinterpret_cast<const int32_t *>(W.parts), D.margins, D.read_margin, D.cut_margin,
                                  D.read, D.alt, D.cut_alt, D.edge_min, D.marginals);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->lg_tab.h() + H.o_out, c->lg_tab.d() + H.o_out, H.down_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    std::memcpy(margins, H.margins, sizeof(str_er_lattice_margin) * nw);
    std::memcpy(read_margin, H.read_margin, 4 * ld::MAX_PARTS * nw);
    std::memcpy(cut_margin, H.cut_margin, 4 * ld::MAX_PARTS * nw);
    std::memcpy(read, H.read, ld::MAX_PARTS * nw);
    std::memcpy(alt, H.alt, ld::MAX_PARTS * nw);
    std::memcpy(cut_alt, H.cut_alt, ld::MAX_PARTS * nw);
    if (em) std::memcpy(edge_min, H.edge_min, 4 * (size_t)ld::MAX_NODES * ld::MAX_FROM * nw);
    if (mg) std::memcpy(marginals, H.marginals, 4 * (size_t)ld::MAX_NODES * ld::MAX_FROM * ld::MARGINALS * nw);
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_lattice_margins_host(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                                const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, int32_t split_cost, const uint8_t *bigram, int32_t ins,
                                int32_t del, str_er_lattice_margin *margins, int32_t *read_margin, int32_t *cut_margin, uint8_t *read, uint8_t *alt, uint8_t *cut_alt,
                                int32_t *edge_min, int32_t *marginals)
{
    using namespace str_er_host;
    if (!args_ok(splits, n_runs, run_costs, piece_costs, n_pieces, first_run, n_runs_of_word, n_words, margins, read_margin, cut_margin, read, alt, cut_alt) || !bigram)
        return STR_ER_EINVAL;
    if (!ld::params_ok(ins, del, split_cost) || !rs::splits_ok(splits, n_runs, n_pieces) || !words_in_rows(n_runs, first_run, n_runs_of_word, n_words)) return STR_ER_EINVAL;
    for (int32_t w = 0; w < n_words; ++w) {
        uint8_t           chars[ld::MAX_CHARS], src[ld::MAX_CHARS];
        str_er_split_part parts[ld::MAX_NODES];
        const size_t      at = (size_t)w * ld::MAX_PARTS, at_e = (size_t)w * ld::MAX_NODES * ld::MAX_FROM;
        const str_er_lattice_decode d = ld::decode_word(splits, run_costs, piece_costs, first_run[w], n_runs_of_word[w], bigram, ins, del, split_cost, chars, src, parts);
        margins[w] = ld::margins_word(splits, run_costs, piece_costs, first_run[w], n_runs_of_word[w], bigram, ins, del, split_cost, chars, src, d.n_chars, parts, d.n_parts,
                                      read_margin + at, cut_margin + at, read + at, alt + at, cut_alt + at, edge_min ? edge_min + at_e : nullptr,
                                      marginals ? marginals + at_e * ld::MARGINALS : nullptr);
    }
    return STR_ER_OK;
}

const str_er_lattice_margin *str_er_result_lattice_margins(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_lattice_margins, &str_er_result::lattice_margins, n);
}
const int32_t *str_er_result_lattice_read_margins(const str_er_result *r, uint64_t *n_bytes)
{
    const int32_t *p = result_table(r, r && r->have_lattice_margins, &str_er_result::lattice_read_margins, n_bytes);
    if (n_bytes) *n_bytes *= 4;
    return p;
}
const int32_t *str_er_result_lattice_cut_margins(const str_er_result *r, uint64_t *n_bytes)
{
    const int32_t *p = result_table(r, r && r->have_lattice_margins, &str_er_result::lattice_cut_margins, n_bytes);
    if (n_bytes) *n_bytes *= 4;
    return p;
}
const uint8_t *str_er_result_lattice_part_reads(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_lattice_margins, &str_er_result::lattice_part_reads, n_bytes);
}
const uint8_t *str_er_result_lattice_part_alts(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_lattice_margins, &str_er_result::lattice_part_alts, n_bytes);
}
const uint8_t *str_er_result_lattice_cut_alts(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_lattice_margins, &str_er_result::lattice_cut_alts, n_bytes);
}

} // extern "C"
