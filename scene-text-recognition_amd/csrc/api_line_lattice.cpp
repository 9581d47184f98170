// api_line_lattice.cpp -- the C ABI, part 8m: the joint decode of a text line over the piece lattices of its runs
// (str_er_lattice_decode_lines on the caller's rows; the contract is at str_er_line_lattice_decode in str_er.h).  The rules are
// line_lattice_rules.h: the pure host entry point here runs them as they stand; k_line_lattice_decode (line_lattice_kernels.h) reads
// what k_lattice_decode reads, a gap pair per run and the table as the caller gave it.
#include "str_er_ctx.h"
#include "line_lattice_kernels.h"
#include "line_lattice_rules.h"

namespace ld = str_er_ld;
namespace rs = str_er_rs;
namespace wd = str_er_wd;

static_assert(sizeof(str_er_line_lattice_decode) == 32, "line lattice decode layout");
static_assert(ld::LL_MAX_RUNS == 1024 && str_er::LL_BP_ROW >= wd::STATES + 2, "the kernel's limits are the rules'");

namespace str_er_host {

LlTab ll_layout(uint8_t *base, size_t at, size_t n_runs, size_t n_lines, size_t n_slots)
{
    LlTab t{};
    Carve cv{at};
    t.o_up = cv.take(2 * n_runs);
    const size_t o_first = cv.take(4 * n_lines), o_nof = cv.take(4 * n_lines), o_slot = cv.take(4 * n_lines);
    t.up_bytes = cv.off - t.o_up;
    t.o_dec = cv.take(sizeof(str_er_line_lattice_decode) * n_lines);
    const size_t o_chars = cv.take(ld::LL_PER_NODE * n_slots), o_src = cv.take(2 * ld::LL_PER_NODE * n_slots), o_parts = cv.take(sizeof(str_er_split_part) * n_slots),
                 o_wop = cv.take(4 * n_slots);
    t.bytes = cv.off;
    t.down_bytes = cv.off - t.o_dec;
    if (base) {
        t.gaps = base + t.o_up; t.first = reinterpret_cast<int32_t *>(base + o_first); t.n_of = reinterpret_cast<int32_t *>(base + o_nof);
        t.slot = reinterpret_cast<int32_t *>(base + o_slot);
        t.dec = reinterpret_cast<str_er_line_lattice_decode *>(base + t.o_dec); t.chars = base + o_chars;
        t.src = reinterpret_cast<uint16_t *>(base + o_src); t.parts = reinterpret_cast<str_er_split_part *>(base + o_parts);
        t.word_of_part = reinterpret_cast<int32_t *>(base + o_wop);
    }
    return t;
}

int line_lattice_enqueue(str_er_ctx *c, hipStream_t s, size_t at, const str_er_run_split *d_splits, const uint8_t *d_run_costs, const uint8_t *d_piece_costs, size_t n_runs,
                         const uint8_t *gaps, const int32_t *first, const int32_t *n_of, const int32_t *slot, size_t n_lines, size_t n_slots, LlTab &H, LlTab &D)
{
    if (const int rc = c->ll_tab.ensure(c, ll_layout(nullptr, at, n_runs, n_lines, n_slots).bytes, "line lattice decode tables"); rc != STR_ER_OK) return rc;
    if (const int rc = c->ll_bp.ensure(c, 4 * (size_t)LL_BP_ROW * n_slots, "line lattice decode back pointers"); rc != STR_ER_OK) return rc;
    H = ll_layout(c->ll_tab.h(), at, n_runs, n_lines, n_slots); D = ll_layout(c->ll_tab.d(), at, n_runs, n_lines, n_slots);
    if (n_runs > 0) std::memcpy(H.gaps, gaps, 2 * n_runs);
    if (n_lines > 0) { std::memcpy(H.first, first, 4 * n_lines); std::memcpy(H.n_of, n_of, 4 * n_lines); std::memcpy(H.slot, slot, 4 * n_lines); }
    if (H.up_bytes > 0) HIP_TRY(c, hipMemcpyAsync(c->ll_tab.d() + H.o_up, c->ll_tab.h() + H.o_up, H.up_bytes, hipMemcpyHostToDevice, s));
    // what lies in no line reads 0xFF, 0xFFFF, {-1, -1} and -1: labels, sources, parts and the parts' words are all bytes of 0xFF
    if (n_slots > 0) HIP_TRY(c, hipMemsetAsync(D.chars, 0xFF, (size_t)(c->ll_tab.d() + D.bytes - D.chars), s));
    launch_line_lattice_decode(s, c->bigram.d(), c->wd_ins, c->wd_del, c->rs_split, d_splits, d_run_costs, d_piece_costs, D.gaps, D.first, D.n_of, D.slot, (int)n_lines,
                               c->ll_bp.d<uint32_t>(), reinterpret_cast<int32_t *>(D.dec), D.chars, D.src, reinterpret_cast<int32_t *>(D.parts), D.word_of_part);
    return STR_ER_OK;
}

bool ll_compact(const str_er_line_lattice_decode *from, const str_er_split_part *from_parts, const int32_t *from_wop, const int32_t *slot, const int32_t *slot_end, size_t n_lines,
                str_er_line_lattice_decode *dec, str_er_split_part *parts, int32_t *word_of_part, uint64_t *n_parts)
{
    uint64_t at = 0;
    for (size_t t = 0; t < n_lines; ++t) {
        const int32_t np = from[t].n_parts;
        if (np < 0 || np > slot_end[t] - slot[t]) return false;
        if (dec) { dec[t] = from[t]; dec[t].first_part = (int32_t)at; }
        if (parts && np > 0) {
            std::memcpy(parts + at, from_parts + (size_t)slot[t], sizeof(str_er_split_part) * (size_t)np);
            std::memcpy(word_of_part + at, from_wop + (size_t)slot[t], 4 * (size_t)np);
        }
        at += (uint64_t)np;
    }
    *n_parts = at;
    return true;
}

} // namespace str_er_host

namespace {

bool args_ok(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces, const uint8_t *gaps,
             const int32_t *first_run, const int32_t *n_of, int32_t n_lines, const str_er_line_lattice_decode *dec, const uint8_t *chars, const uint16_t *src,
             const str_er_split_part *parts, int32_t cap_parts, const int32_t *n_parts, const int32_t *word_of_part)
{
    return n_runs >= 0 && n_pieces >= 0 && n_lines >= 0 && cap_parts >= 0 && n_parts && (n_runs == 0 || (splits && run_costs && gaps && chars && src)) &&
           (n_pieces == 0 || piece_costs) && (n_lines == 0 || (first_run && n_of && dec)) && (cap_parts == 0 || (parts && word_of_part));
}

// the node slot of every line and the slot behind its last run, from the slots of the runs
void line_slots(const std::vector<int32_t> &run_slot, const int32_t *first_run, const int32_t *n_of, size_t n_lines, std::vector<int32_t> &slot, std::vector<int32_t> &slot_end)
{
    slot.resize(n_lines); slot_end.resize(n_lines);
    for (size_t t = 0; t < n_lines; ++t) { slot[t] = run_slot[(size_t)first_run[t]]; slot_end[t] = run_slot[(size_t)first_run[t] + (size_t)n_of[t]]; }
}

} // namespace

extern "C" {

int str_er_set_line_lattice_decode(str_er_ctx *c, int32_t on, int32_t weight)
try {
    if (!c) return STR_ER_EINVAL;
    if (!ld::weight_ok(weight)) return fail(c, STR_ER_EINVAL, "line lattice decode: the weight is in 0 .. 127");
    c->ll_on = on != 0; c->ll_weight = weight;
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_line_lattice_decode_stats(const str_er_ctx *c, uint64_t *table_bytes)
{
    if (!c) return STR_ER_EINVAL;
    if (table_bytes) *table_bytes = c->ll_bp.size();
    return STR_ER_OK;
}

int str_er_lattice_decode_lines(str_er_ctx *c, const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                                const uint8_t *gaps, const int32_t *first_run, const int32_t *n_runs_of_line, int32_t n_lines, str_er_line_lattice_decode *dec,
                                uint8_t *chars, uint16_t *src, str_er_split_part *parts, int32_t cap_parts, int32_t *n_parts, int32_t *word_of_part)
try {
    using namespace str_er_host;
    if (!c) return STR_ER_EINVAL;
    if (!args_ok(splits, n_runs, run_costs, piece_costs, n_pieces, gaps, first_run, n_runs_of_line, n_lines, dec, chars, src, parts, cap_parts, n_parts, word_of_part))
        return fail(c, STR_ER_EINVAL, "bad arguments");
    *n_parts = 0;
    if (!c->bigram_set) return fail(c, STR_ER_ESTATE, "str_er_lattice_decode_lines needs a bigram table (str_er_set_bigram)");
    if (!rs::splits_ok(splits, n_runs, n_pieces)) return fail(c, STR_ER_EINVAL, "line lattice decode: a record with cuts or pieces that are none");
    if (!ld::lines_in_rows(n_runs, first_run, n_runs_of_line, n_lines)) return fail(c, STR_ER_EINVAL, "line lattice decode: a line outside the glyph runs, or the lines out of order");
    if (!ld::ll_gaps_ok(gaps, first_run, n_runs_of_line, n_lines)) return fail(c, STR_ER_EINVAL, "line lattice decode: a gap with both moves off");
    const size_t nr = (size_t)n_runs, np = (size_t)n_pieces, nl = (size_t)n_lines;
    std::vector<int32_t> run_slot, slot, slot_end;
    if (nr + np > 0x7FFFFFFFull / 65 || !ld::ll_node_slots(splits, n_runs, run_slot) || (uint64_t)run_slot[nr] > 0x7FFFFFFFull / (4 * LL_BP_ROW))
        return fail(c, STR_ER_ECAPACITY, "line lattice decode: too many rows or nodes");
    const size_t ns = (size_t)run_slot[nr];
    if (nl == 0) {
        if (ns > 0) { std::memset(chars, 0xFF, ld::LL_PER_NODE * ns); std::memset(src, 0xFF, 2 * ld::LL_PER_NODE * ns); }
        return STR_ER_OK;
    }
    line_slots(run_slot, first_run, n_runs_of_line, nl, slot, slot_end);
    const size_t at = rows_in_layout(nullptr, nr, nr + np, 0, false).bytes;
    if (const int rc = c->ll_tab.ensure(c, ll_layout(nullptr, at, nr, nl, ns).bytes, "line lattice decode tables"); rc != STR_ER_OK) return rc;
    hipStream_t s = c->stream;
    RowsIn      I{};
    if (const int rc = rows_in_upload(c, s, c->ll_tab, splits, run_costs, nr, piece_costs, np, nullptr, nullptr, nullptr, 0, I); rc != STR_ER_OK) return rc;
    LlTab H{}, D{};
    if (const int rc = line_lattice_enqueue(c, s, at, I.splits, I.costs, I.costs + rs::ALPHABET * nr, nr, gaps, first_run, n_runs_of_line, slot.data(), nl, ns, H, D); rc != STR_ER_OK)
        return rc;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->ll_tab.h() + H.o_dec, c->ll_tab.d() + H.o_dec, H.down_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    uint64_t total = 0;
    if (!ll_compact(H.dec, H.parts, H.word_of_part, slot.data(), slot_end.data(), nl, nullptr, nullptr, nullptr, &total))
        return fail(c, STR_ER_EHIP, "line lattice decode: a line's parts outside its slots (internal error)");
    *n_parts = (int32_t)total;
    if (total > (uint64_t)cap_parts) return fail(c, STR_ER_ECAPACITY, std::to_string(total) + " parts, cap_parts is " + std::to_string(cap_parts));
    ll_compact(H.dec, H.parts, H.word_of_part, slot.data(), slot_end.data(), nl, dec, parts, word_of_part, &total);
    if (ns > 0) { std::memcpy(chars, H.chars, ld::LL_PER_NODE * ns); std::memcpy(src, H.src, 2 * ld::LL_PER_NODE * ns); }
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_lattice_decode_lines_host(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                                     const uint8_t *gaps, const int32_t *first_run, const int32_t *n_runs_of_line, int32_t n_lines, int32_t split_cost,
                                     const uint8_t *bigram, int32_t ins, int32_t del, str_er_line_lattice_decode *dec, uint8_t *chars, uint16_t *src,
                                     str_er_split_part *parts, int32_t cap_parts, int32_t *n_parts, int32_t *word_of_part)
try {
    if (!args_ok(splits, n_runs, run_costs, piece_costs, n_pieces, gaps, first_run, n_runs_of_line, n_lines, dec, chars, src, parts, cap_parts, n_parts, word_of_part) || !bigram)
        return STR_ER_EINVAL;
    *n_parts = 0;
    if (!ld::params_ok(ins, del, split_cost) || !rs::splits_ok(splits, n_runs, n_pieces) || !ld::lines_in_rows(n_runs, first_run, n_runs_of_line, n_lines) ||
        !ld::ll_gaps_ok(gaps, first_run, n_runs_of_line, n_lines))
        return STR_ER_EINVAL;
    std::vector<int32_t> run_slot, slot, slot_end;
    if (!ld::ll_node_slots(splits, n_runs, run_slot)) return STR_ER_ECAPACITY;
    const size_t nl = (size_t)n_lines, ns = (size_t)run_slot[(size_t)n_runs];
    line_slots(run_slot, first_run, n_runs_of_line, nl, slot, slot_end);
    // every line once, into tables of its own; the count is set even where cap_parts is too small, and nothing is written to the
    // caller's arrays before it is known to fit
    std::vector<str_er_line_lattice_decode> recs(nl);
    std::vector<uint8_t>                    lab(ld::LL_PER_NODE * ns, 0xFF);
    std::vector<uint16_t>                   from(ld::LL_PER_NODE * ns, 0xFFFF);
    std::vector<str_er_split_part>          all(ns, str_er_split_part{-1, -1});
    std::vector<int32_t>                    wop(ns, -1);
    for (size_t t = 0; t < nl; ++t) {
        const size_t f = (size_t)slot[t];
        recs[t] = ld::decode_line_lattice(splits, run_costs, piece_costs, gaps, first_run[t], n_runs_of_line[t], bigram, ins, del, split_cost, lab.data() + ld::LL_PER_NODE * f,
                                          from.data() + ld::LL_PER_NODE * f, all.data() + f, wop.data() + f);
    }
    uint64_t total = 0;
    if (!ll_compact(recs.data(), all.data(), wop.data(), slot.data(), slot_end.data(), nl, nullptr, nullptr, nullptr, &total)) return STR_ER_EINVAL;
    *n_parts = (int32_t)total;
    if (total > (uint64_t)cap_parts) return STR_ER_ECAPACITY;
    ll_compact(recs.data(), all.data(), wop.data(), slot.data(), slot_end.data(), nl, dec, parts, word_of_part, &total);
    if (ns > 0) { std::memcpy(chars, lab.data(), lab.size()); std::memcpy(src, from.data(), 2 * from.size()); }
    return STR_ER_OK;
} catch (...) { return STR_ER_ENOMEM; }

const str_er_line_lattice_decode *str_er_result_line_lattice_decodes(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_line_lattice_decodes, &str_er_result::line_lattice_decodes, n);
}
const uint8_t *str_er_result_line_lattice_chars(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_line_lattice_decodes, &str_er_result::line_lattice_chars, n_bytes);
}
const uint16_t *str_er_result_line_lattice_src(const str_er_result *r, uint64_t *n)
{
    return result_table(r, r && r->have_line_lattice_decodes, &str_er_result::line_lattice_src, n);
}
const str_er_split_part *str_er_result_line_lattice_parts(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_line_lattice_decodes, &str_er_result::line_lattice_parts, n);
}
const int32_t *str_er_result_line_lattice_word_of_part(const str_er_result *r, uint64_t *n)
{
    return result_table(r, r && r->have_line_lattice_decodes, &str_er_result::line_lattice_word_of_part, n);
}
const uint8_t *str_er_result_line_lattice_gap_costs(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_line_lattice_decodes, &str_er_result::line_lattice_gap_costs, n_bytes);
}
const int32_t *str_er_result_line_lattice_windows(const str_er_result *r, uint64_t *n)
{
    return result_table(r, r && r->have_line_lattice_decodes, &str_er_result::line_lattice_windows, n);
}

} // extern "C"
