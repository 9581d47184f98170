// api_run_split.cpp -- the C ABI, part 8f: the splitting of touching glyphs (str_er_feet_split on uploaded footprints, str_er_split_words
// on the caller's cost rows; the contract is at str_er_run_split in str_er.h).  The rules are run_split_rules.h: the pure host entry
// points here run them as they stand.  k_run_cuts (run_split_kernels.h) works from the run slots of k_foot_words on the device, so its
// records come down with the line stage's wait (run_cuts_enqueue / run_cuts_collect, called by feet_words_read in
// api_frame_lines.cpp); the host forms the pieces from the atoms, and run_read_stage (api_run_read.cpp) reads them behind the runs.
#include "str_er_ctx.h"
#include "run_split_kernels.h"
#include "run_split_rules.h"

namespace rs = str_er_rs;

static_assert(sizeof(str_er_run_split) == 32, "run split layout");
static_assert(sizeof(str_er_run_piece) == 32, "run piece layout");
static_assert(sizeof(str_er_split_part) == 8, "split part layout");
static_assert(sizeof(str_er_word_split) == 16, "word split layout");
static_assert(rs::MAX_W == STR_ER_RUN_SPLIT_MAX_W && rs::MAX_W == str_er::RS_MAX_W, "RUN_SPLIT_MAX_W");

namespace str_er_host {

int run_cuts_enqueue(str_er_ctx *c, hipStream_t s, const FootLine *d_lines, int32_t n_lines, const uint8_t *words, size_t o_rec, size_t o_elem, size_t n_slots)
{
    if (n_lines <= 0 || n_slots == 0) return STR_ER_OK;
    if (const int rc = c->rs_out.ensure(c, sizeof(RunCutRec) * n_slots, "run split output"); rc != STR_ER_OK) return rc;
    launch_run_cuts(s, d_lines, n_lines, reinterpret_cast<const WordsSlot *>(words), reinterpret_cast<const WordsRec *>(words + o_rec),
                    reinterpret_cast<const WordsRun *>(words + o_elem), c->foot_bits.d<uint64_t>(), c->rs_num, c->rs_den,
                    reinterpret_cast<RunCutRec *>(c->rs_out.d()));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->rs_out.h(), c->rs_out.d(), sizeof(RunCutRec) * n_slots, hipMemcpyDeviceToHost, s));
    return STR_ER_OK;
}

int run_cuts_collect(str_er_ctx *c, const std::vector<str_er_line_run> &runs, const std::vector<uint32_t> &slot_of, std::vector<str_er_run_split> &splits,
                     std::vector<str_er_run_piece> &pieces)
{
    splits.assign(runs.size(), str_er_run_split{0, {-1, -1, -1}, 0, 0, 0, 0});
    pieces.clear();
    for (size_t r = 0; r < runs.size(); ++r) {
        if (((size_t)slot_of[r] + 1) * sizeof(RunCutRec) > c->rs_out.size()) return fail(c, STR_ER_EHIP, "run split: a run outside the cut records (internal error)");
        RunCutRec K;
        std::memcpy(&K, c->rs_out.h() + sizeof(RunCutRec) * slot_of[r], sizeof K);
        const str_er_line_run &R = runs[r];
        str_er_run_split      &S = splits[r];
        bool ok = K.n_cuts >= 0 && K.n_cuts <= rs::MAX_CUTS;
        for (int k = 0; ok && k < K.n_cuts; ++k) ok = K.cut[k] > (k ? K.cut[k - 1] : R.x0) && K.cut[k] < R.x1;
        for (int q = 0; ok && q <= K.n_cuts; ++q) ok = K.px[q] > 0 && K.y0[q] >= R.y0 && K.y0[q] < K.y1[q] && K.y1[q] <= R.y1;
        if (!ok) return fail(c, STR_ER_EHIP, "run split: the device's cuts are not cuts (internal error)");
        S.n_cuts = K.n_cuts; S.thr = K.thr;
        for (int k = 0; k < K.n_cuts; ++k) S.cut[k] = K.cut[k];
        S.first_piece = (int32_t)pieces.size(); S.n_pieces = rs::n_pieces(K.n_cuts);
        if (pieces.size() + (size_t)S.n_pieces > 0x7FFFFFFFull) return fail(c, STR_ER_ECAPACITY, "run split: more than 2^31 pieces");
        const int     A = K.n_cuts + 1;
        const int32_t node[rs::MAX_ATOMS + 1] = {R.x0, A > 1 ? K.cut[0] : R.x1, A > 2 ? K.cut[1] : R.x1, A > 3 ? K.cut[2] : R.x1, R.x1};
        for (int i = 0; i < A && S.n_pieces > 0; ++i)
            for (int j = i + 1; j <= A; ++j) {
                if (i == 0 && j == A) continue;
                str_er_run_piece Q{(int32_t)r, i, j, node[i], j == A ? R.x1 : node[j], K.y0[i], K.y1[i], 0};
                for (int q = i; q < j; ++q) { Q.y0 = std::min(Q.y0, K.y0[q]); Q.y1 = std::max(Q.y1, K.y1[q]); Q.pixels += K.px[q]; }
                pieces.push_back(Q);
            }
    }
    return STR_ER_OK;
}

RsTab rs_layout(uint8_t *base, size_t at, size_t n_words, size_t n_slots, bool part_rows)
{
    RsTab t{};
    Carve cv{at};
    t.o_out = cv.take(16 * n_words);
    const size_t o_parts = cv.take(8 * n_slots);
    t.down_tables = cv.off - t.o_out;
    const size_t o_rows = cv.take(part_rows ? rs::ALPHABET * n_slots : 0);
    t.down_bytes = cv.off - t.o_out;
    const size_t o_np = cv.take(4 * n_words);
    t.bytes = cv.off;
    if (base) {
        t.word_out = reinterpret_cast<int32_t *>(base + t.o_out); t.parts = reinterpret_cast<int32_t *>(base + o_parts); t.part_costs = base + o_rows;
        t.n_parts = reinterpret_cast<int32_t *>(base + o_np);
    }
    return t;
}

bool rs_word_slots(const str_er_run_split *splits, const int32_t *first_run, const int32_t *n_of, size_t n_words, std::vector<int32_t> &slot, uint64_t *n_slots)
{
    slot.assign(n_words, 0);
    uint64_t at = 0;
    for (size_t w = 0; w < n_words; ++w) {
        slot[w] = (int32_t)at;
        for (int32_t r = first_run[w]; r < first_run[w] + n_of[w]; ++r) at += (uint64_t)splits[r].n_cuts + 1u;
        if (at > 0x7FFFFFFFull) return false;
    }
    *n_slots = at;
    return true;
}

bool rs_compact(const RsTab &H, const std::vector<int32_t> &slot, uint64_t n_slots, str_er_word_split *word_splits, str_er_split_part *parts, uint8_t *part_costs,
                uint64_t *n_parts)
{
    const size_t nw = slot.size();
    uint64_t     at = 0;
    for (size_t w = 0; w < nw; ++w) {
        const int32_t  np_w = H.word_out[4 * w];
        const uint64_t atoms = (w + 1 < nw ? (uint64_t)slot[w + 1] : n_slots) - (uint64_t)slot[w];
        if (np_w < 0 || (uint64_t)np_w > atoms) return false;
        if (word_splits) word_splits[w] = str_er_word_split{(int32_t)at, np_w, H.word_out[4 * w + 1], H.word_out[4 * w + 2]};
        if (parts && np_w > 0) std::memcpy(parts + at, H.parts + 2 * (size_t)slot[w], 8 * (size_t)np_w);
        if (part_costs && np_w > 0) std::memcpy(part_costs + rs::ALPHABET * at, H.part_costs + rs::ALPHABET * (size_t)slot[w], rs::ALPHABET * (size_t)np_w);
        at += (uint64_t)np_w;
    }
    *n_parts = at;
    return true;
}

namespace {

bool args_ok(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces, const int32_t *first_run,
             const int32_t *n_of, int32_t n_words, const str_er_word_split *word_splits, const str_er_split_part *parts, int32_t cap_parts, const int32_t *n_parts)
{
    return n_runs >= 0 && n_pieces >= 0 && n_words >= 0 && cap_parts >= 0 && n_parts && (n_runs == 0 || (splits && run_costs)) && (n_pieces == 0 || piece_costs) &&
           (n_words == 0 || (first_run && n_of && word_splits)) && (cap_parts == 0 || parts);
}

} // namespace

} // namespace str_er_host

extern "C" {

int str_er_set_run_split(str_er_ctx *c, int32_t num, int32_t den, int32_t split_cost)
try {
    if (!c) return STR_ER_EINVAL;
    if (!rs::params_ok(num, den, split_cost)) return fail(c, STR_ER_EINVAL, "str_er_set_run_split: 1 <= num, den <= 65535 and split_cost in 0 .. 255");
    c->rs_num = num; c->rs_den = den; c->rs_split = split_cost;
    ++c->pool_gen;          // (a track pool is bound to SPLIT: str_er_pool_match)
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_run_split_stats(const str_er_ctx *c, uint64_t *cut_bytes, uint64_t *table_bytes)
{
    if (!c) return STR_ER_EINVAL;
    if (cut_bytes) *cut_bytes = c->rs_out.size();
    if (table_bytes) *table_bytes = c->rs_tab.size();
    return STR_ER_OK;
}

int str_er_cuts_from_counts(const uint32_t *n, int32_t W, int32_t H, int32_t num, int32_t den, int32_t cut[3], int32_t *n_cuts, uint32_t *thr)
{
    if (!n || !cut || !n_cuts || W < 1 || H < 1 || !rs::params_ok(num, den, 0)) return STR_ER_EINVAL;
    *n_cuts = rs::cuts_from_counts(n, W, H, num, den, cut);
    if (thr) *thr = rs::threshold(H, num, den);
    return STR_ER_OK;
}

int str_er_feet_split(str_er_ctx *c, int32_t W, int32_t H, const str_er_line_foot *feet, const uint32_t *bits, const double *slopes, int32_t n,
                      str_er_line_words *line_words, str_er_line_run *runs, int32_t cap_runs, int32_t *n_runs, str_er_line_word *words, int32_t cap_words,
                      int32_t *n_words, str_er_run_read *reads, uint8_t *q_out, str_er_run_split *splits, str_er_run_piece *pieces, int32_t cap_pieces,
                      int32_t *n_pieces, str_er_run_read *piece_reads, uint8_t *piece_q)
try {
    if (!c) return STR_ER_EINVAL;
    const FeetSplitOut out{splits, pieces, cap_pieces, n_pieces, piece_reads, piece_q};
    return feet_words_read(c, W, H, feet, bits, n, line_words, runs, cap_runs, n_runs, words, cap_words, n_words, true, slopes, reads, q_out, &out);
} ABI_GUARD(c)

int str_er_split_words(str_er_ctx *c, const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                       const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, str_er_word_split *word_splits, str_er_split_part *parts,
                       int32_t cap_parts, int32_t *n_parts, uint8_t *part_costs)
try {
    if (!c) return STR_ER_EINVAL;
    if (!args_ok(splits, n_runs, run_costs, piece_costs, n_pieces, first_run, n_runs_of_word, n_words, word_splits, parts, cap_parts, n_parts))
        return fail(c, STR_ER_EINVAL, "bad arguments");
    *n_parts = 0;
    if (!rs::splits_ok(splits, n_runs, n_pieces)) return fail(c, STR_ER_EINVAL, "run split: a record with cuts or pieces that are none");
    if (!words_in_rows(n_runs, first_run, n_runs_of_word, n_words)) return fail(c, STR_ER_EINVAL, "run split: a word outside the glyph runs");
    if (n_words == 0) return STR_ER_OK;
    std::vector<int32_t> slot;
    uint64_t             n_slots = 0;
    if (!rs_word_slots(splits, first_run, n_runs_of_word, (size_t)n_words, slot, &n_slots)) return fail(c, STR_ER_ECAPACITY, "run split: more than 2^31 parts to reserve");
    const size_t nr = (size_t)n_runs, np = (size_t)n_pieces, nw = (size_t)n_words;
    const size_t at = rows_in_layout(nullptr, nr, nr + np, nw, true).bytes;
    if (const int rc = c->rs_tab.ensure(c, rs_layout(nullptr, at, nw, (size_t)n_slots, true).bytes, "run split tables"); rc != STR_ER_OK) return rc;
    const RsTab H = rs_layout(c->rs_tab.h(), at, nw, (size_t)n_slots, true), D = rs_layout(c->rs_tab.d(), at, nw, (size_t)n_slots, true);
    hipStream_t s = c->stream;
    RowsIn      I{};
    if (const int rc = rows_in_upload(c, s, c->rs_tab, splits, run_costs, nr, piece_costs, np, first_run, n_runs_of_word, slot.data(), nw, I); rc != STR_ER_OK) return rc;
    launch_split_words(s, I.splits, I.costs, I.costs + rs::ALPHABET * nr, I.first, I.n_of, I.slot, n_words, c->rs_split, D.word_out, D.parts, D.part_costs);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->rs_tab.h() + H.o_out, c->rs_tab.d() + H.o_out, H.down_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    uint64_t total = 0;
    if (!rs_compact(H, slot, n_slots, nullptr, nullptr, nullptr, &total)) return fail(c, STR_ER_EHIP, "run split: a word's parts outside its slots (internal error)");
    *n_parts = (int32_t)total;
    if (total > (uint64_t)cap_parts) return fail(c, STR_ER_ECAPACITY, std::to_string(total) + " parts, cap_parts is " + std::to_string(cap_parts));
    rs_compact(H, slot, n_slots, word_splits, parts, part_costs, &total);
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_split_words_host(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                            const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, int32_t split_cost, str_er_word_split *word_splits,
                            str_er_split_part *parts, int32_t cap_parts, int32_t *n_parts, uint8_t *part_costs)
try {
    using namespace str_er_host;
    if (!args_ok(splits, n_runs, run_costs, piece_costs, n_pieces, first_run, n_runs_of_word, n_words, word_splits, parts, cap_parts, n_parts)) return STR_ER_EINVAL;
    *n_parts = 0;
    if (!rs::params_ok(1, 1, split_cost) || !rs::splits_ok(splits, n_runs, n_pieces) || !words_in_rows(n_runs, first_run, n_runs_of_word, n_words)) return STR_ER_EINVAL;
    // every word once, its parts behind those of the words before it; the count is set even where cap_parts is too small
    std::vector<str_er_word_split> ws((size_t)n_words);
    std::vector<str_er_split_part> all;
    std::vector<uint8_t>           rows;
    for (int32_t w = 0; w < n_words; ++w) {
        const size_t at = all.size(), atoms = (size_t)rs::MAX_ATOMS * (size_t)n_runs_of_word[w];
        all.resize(at + atoms);
        if (part_costs) rows.resize(rs::ALPHABET * (at + atoms));
        ws[(size_t)w] = rs::split_word(splits, run_costs, piece_costs, first_run[w], n_runs_of_word[w], split_cost, all.data() + at,
                                       part_costs ? rows.data() + rs::ALPHABET * at : nullptr);
        ws[(size_t)w].first_part = (int32_t)at;
        all.resize(at + (size_t)ws[(size_t)w].n_parts);
        if (all.size() > 0x7FFFFFFFull) return STR_ER_ECAPACITY;
    }
    *n_parts = (int32_t)all.size();
    if (all.size() > (size_t)cap_parts) return STR_ER_ECAPACITY;
    if (n_words > 0) std::memcpy(word_splits, ws.data(), sizeof(str_er_word_split) * ws.size());
    if (!all.empty()) {
        std::memcpy(parts, all.data(), sizeof(str_er_split_part) * all.size());
        if (part_costs) std::memcpy(part_costs, rows.data(), rs::ALPHABET * all.size());
    }
    return STR_ER_OK;
} catch (...) { return STR_ER_ENOMEM; }

const str_er_run_split *str_er_result_run_splits(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_run_splits, &str_er_result::run_splits, n);
}
const str_er_run_piece *str_er_result_run_pieces(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_run_splits, &str_er_result::run_pieces, n);
}
const str_er_run_read *str_er_result_piece_reads(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_run_splits, &str_er_result::piece_reads, n);
}
const uint8_t *str_er_result_piece_costs(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_run_splits, &str_er_result::piece_costs, n_bytes);
}
const str_er_split_part *str_er_result_split_parts(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_run_splits, &str_er_result::split_parts, n);
}
const str_er_word_split *str_er_result_word_splits(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_run_splits, &str_er_result::word_splits, n);
}

} // extern "C"
