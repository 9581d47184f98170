// api_lattice_track.cpp -- the C ABI, part 8j: the track match over the members' piece lattices (STR_ER_WANT_LATTICE_TRACK behind the
// lattice match in api_run_read.cpp, str_er_lattice_match_tracks on the caller's rows and tracks; the contract is at
// str_er_lattice_track_member in str_er.h).  The rules are lattice_track_rules.h: the pure host entry point here runs them as they stand
// after the checks of both parents; the kernels (lattice_track_kernels.h) read what k_lattice_match reads and the tracks as
// k_track_match takes them.
#include "str_er_ctx.h"
#include "lattice_track_kernels.h"
#include "lattice_track_rules.h"

namespace lt = str_er_lt;
namespace lm = str_er_lm;
namespace rs = str_er_rs;
namespace tr = str_er_tr;
namespace wm = str_er_wm;

static_assert(sizeof(str_er_lattice_track_member) == 24 && sizeof(str_er_track_match) == 32, "lattice track layout");

namespace str_er_host {

LtTab lt_layout(uint8_t *base, size_t at, size_t n_words, size_t n_tracks, size_t n_members, size_t n_pslots, int n_chunks)
{
    LtTab t{};
    Carve cv{at};
    t.o_up = cv.take(4 * n_tracks);
    const size_t o_count = cv.take(4 * n_tracks), o_mem = cv.take(4 * n_members), o_st = cv.take(4 * n_members), o_ps = cv.take(4 * n_members);
    t.up_bytes = cv.off - t.o_up;
    const size_t o_tab = cv.take(4 * (size_t)str_er::LT_TAB_INTS * n_words), o_part = cv.take(16 * n_tracks * (size_t)n_chunks);
    t.o_matches = cv.take(sizeof(str_er_track_match) * n_tracks);
    const size_t o_mrec = cv.take(sizeof(str_er_lattice_track_member) * n_members), o_src = cv.take(lm::SRC_BYTES * n_members),
                 o_parts = cv.take(sizeof(str_er_split_part) * n_pslots);
    t.down_bytes = cv.off - t.o_matches;
    const size_t o_free = cv.take(4 * n_members);
    t.bytes = cv.off;
    if (base) {
        const auto i32 = [&](size_t o) { return reinterpret_cast<int32_t *>(base + o); };
        t.first = i32(t.o_up); t.count = i32(o_count); t.members = i32(o_mem); t.slot_track = i32(o_st); t.pslot = i32(o_ps); t.tab = i32(o_tab);
        t.partial = reinterpret_cast<uint64_t *>(base + o_part); t.matches = reinterpret_cast<str_er_track_match *>(base + t.o_matches);
        t.mrec = reinterpret_cast<str_er_lattice_track_member *>(base + o_mrec); t.src = base + o_src;
        t.parts = reinterpret_cast<str_er_split_part *>(base + o_parts); t.mfree = i32(o_free);
    }
    return t;
}

int lattice_track_enqueue(str_er_ctx *c, hipStream_t s, size_t at, const str_er_run_split *d_splits, const uint8_t *d_run_costs, const uint8_t *d_piece_costs,
                          const int32_t *d_first, const int32_t *d_n_of, const str_er_run_split *splits, const int32_t *first_run, const int32_t *n_of, size_t n_words,
                          const int32_t *track_first, const int32_t *track_count, const int32_t *members, size_t n_members, size_t n_tracks, std::vector<int32_t> &pslot,
                          uint64_t *n_pslots, LtTab &H, LtTab &D)
{
    const int n_chunks = tm_chunks(c->lex);
    if (n_tracks > 0x7FFFFFFFull / (size_t)n_chunks / 2) return fail(c, STR_ER_ECAPACITY, "lattice track: too many tracks for this lexicon");
    if (n_words > 0x7FFFFFFFull / (4 * (size_t)str_er::LT_TAB_INTS) || n_members > 0x7FFFFFFFull / 32) return fail(c, STR_ER_ECAPACITY, "lattice track: too many words or members");
    // the part slots of a member slot: its word's nodes, none for an unusable member and for a slot of no track
    std::vector<int32_t> slot_track(n_members, -1);
    for (size_t g = 0; g < n_tracks; ++g)
        for (int32_t j = 0; j < track_count[g]; ++j) slot_track[(size_t)track_first[g] + (size_t)j] = (int32_t)g;
    pslot.assign(n_members, 0);
    uint64_t total = 0;
    for (size_t i = 0; i < n_members; ++i) {
        pslot[i] = (int32_t)total;
        const int32_t w = members[i];
        const int64_t N = slot_track[i] < 0 ? 0 : lm::word_nodes(splits, first_run[w], n_of[w]);
        total += N <= lm::MAX_NODES ? (uint64_t)N : 0;
        if (total > 0x7FFFFFFFull) return fail(c, STR_ER_ECAPACITY, "lattice track: more than 2^31 parts to reserve");
    }
    *n_pslots = total;
    if (const int rc = c->lt_tab.ensure(c, lt_layout(nullptr, at, n_words, n_tracks, n_members, (size_t)total, n_chunks).bytes, "lattice track tables"); rc != STR_ER_OK) return rc;
    H = lt_layout(c->lt_tab.h(), at, n_words, n_tracks, n_members, (size_t)total, n_chunks);
    D = lt_layout(c->lt_tab.d(), at, n_words, n_tracks, n_members, (size_t)total, n_chunks);
    if (n_tracks > 0) {
        std::memcpy(H.first, track_first, 4 * n_tracks);
        std::memcpy(H.count, track_count, 4 * n_tracks);
    }
    if (n_members > 0) {
        std::memcpy(H.members, members, 4 * n_members);
        std::memcpy(H.slot_track, slot_track.data(), 4 * n_members);
        std::memcpy(H.pslot, pslot.data(), 4 * n_members);
    }
    HIP_TRY(c, hipMemcpyAsync(c->lt_tab.d() + H.o_up, c->lt_tab.h() + H.o_up, H.up_bytes, hipMemcpyHostToDevice, s));
    launch_lattice_track(s, c->lex, c->wm_prm, c->rs_split, d_splits, d_run_costs, d_piece_costs, d_first, d_n_of, (int)n_words, D.first, D.count, D.members, D.slot_track,
                         D.pslot, (int)n_members, (int)n_tracks, D.tab, D.partial, reinterpret_cast<int32_t *>(D.matches), reinterpret_cast<int32_t *>(D.mrec), D.src,
                         reinterpret_cast<int32_t *>(D.parts), D.mfree);
    HIP_TRY(c, hipGetLastError());
    return STR_ER_OK;
}

bool lt_compact(const LtTab &H, const std::vector<int32_t> &pslot, uint64_t n_pslots, str_er_lattice_track_member *mrec, str_er_split_part *parts, uint64_t *n_parts)
{
    const size_t nm = pslot.size();
    uint64_t     at = 0;
    for (size_t i = 0; i < nm; ++i) {
        const int32_t  np_i = H.mrec[i].n_parts;
        const uint64_t room = (i + 1 < nm ? (uint64_t)pslot[i + 1] : n_pslots) - (uint64_t)pslot[i];
        if (np_i < 0 || (uint64_t)np_i > room) return false;
        if (mrec) { mrec[i] = H.mrec[i]; mrec[i].first_part = (int32_t)at; }
        if (parts && np_i > 0) std::memcpy(parts + at, H.parts + (size_t)pslot[i], sizeof(str_er_split_part) * (size_t)np_i);
        at += (uint64_t)np_i;
    }
    *n_parts = at;
    return true;
}

} // namespace str_er_host

namespace {

bool args_ok(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces, const int32_t *first_run,
             const int32_t *n_of, int32_t n_words, const int32_t *track_first, const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks,
             const str_er_track_match *out, const str_er_lattice_track_member *members_out, const uint8_t *src, const str_er_split_part *parts, int32_t cap_parts,
             const int32_t *n_parts)
{
    return n_runs >= 0 && n_pieces >= 0 && n_words >= 0 && n_members >= 0 && n_tracks >= 0 && cap_parts >= 0 && n_parts && (n_runs == 0 || (splits && run_costs)) &&
           (n_pieces == 0 || piece_costs) && (n_words == 0 || (first_run && n_of)) && (n_tracks == 0 || (track_first && track_count && out)) &&
           (n_members == 0 || (members && members_out && src)) && (cap_parts == 0 || parts);
}

} // namespace

extern "C" {

int str_er_lattice_track_stats(const str_er_ctx *c, uint64_t *table_bytes)
{
    if (!c) return STR_ER_EINVAL;
    if (table_bytes) *table_bytes = c->lt_tab.size();
    return STR_ER_OK;
}

int str_er_lattice_match_tracks(str_er_ctx *c, const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                                const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, const int32_t *track_first, const int32_t *track_count,
                                const int32_t *members, int32_t n_members, int32_t n_tracks, str_er_track_match *out, str_er_lattice_track_member *members_out,
                                uint8_t *src, str_er_split_part *parts, int32_t cap_parts, int32_t *n_parts)
try {
    using namespace str_er_host;
    if (!c) return STR_ER_EINVAL;
    if (!args_ok(splits, n_runs, run_costs, piece_costs, n_pieces, first_run, n_runs_of_word, n_words, track_first, track_count, members, n_members, n_tracks, out,
                 members_out, src, parts, cap_parts, n_parts))
        return fail(c, STR_ER_EINVAL, "bad arguments");
    *n_parts = 0;
    if (c->lex_n <= 0) return fail(c, STR_ER_ESTATE, "str_er_lattice_match_tracks needs a lexicon (str_er_set_lexicon)");
    if (!rs::splits_ok(splits, n_runs, n_pieces)) return fail(c, STR_ER_EINVAL, "lattice track: a record with cuts or pieces that are none");
    if (!words_in_rows(n_runs, first_run, n_runs_of_word, n_words)) return fail(c, STR_ER_EINVAL, "lattice track: a word outside the glyph runs");
    if (const int rc = tr::tracks_check(track_first, track_count, members, n_members, n_tracks, n_words); rc != STR_ER_OK)
        return fail(c, rc, rc == STR_ER_ECAPACITY ? "lattice track: a track of more than 65536 members"
                                                  : "lattice track: a member outside the words, or tracks that do not ascend in the member array");
    if (n_tracks == 0 && n_members == 0) return STR_ER_OK;
    const size_t nr = (size_t)n_runs, np = (size_t)n_pieces, nw = (size_t)n_words, nm = (size_t)n_members, nt = (size_t)n_tracks;
    if (nr + np > 0x7FFFFFFFull / 65 || nw > 0x7FFFFFFFull / 64) return fail(c, STR_ER_ECAPACITY, "lattice track: too many rows or words");
    // the rows and the words' (first, n) at the front of the buffer; the tracks' tables behind them.  The buffer is sized for both before
    // anything goes up: the second ensure must not move what the first upload reads
    const size_t at = rows_in_layout(nullptr, nr, nr + np, nw, false).bytes;
    {
        uint64_t need = 0;
        for (size_t i = 0; i < nm; ++i) {
            const int64_t N = lm::word_nodes(splits, first_run[members[i]], n_runs_of_word[members[i]]);
            need += N <= lm::MAX_NODES ? (uint64_t)N : 0;
        }
        if (need > 0x7FFFFFFFull) return fail(c, STR_ER_ECAPACITY, "lattice track: more than 2^31 parts to reserve");
        if (const int rc = c->lt_tab.ensure(c, lt_layout(nullptr, at, nw, nt, nm, (size_t)need, tm_chunks(c->lex)).bytes, "lattice track tables"); rc != STR_ER_OK) return rc;
    }
    hipStream_t s = c->stream;
    RowsIn      I{};
    if (const int rc = rows_in_upload(c, s, c->lt_tab, splits, run_costs, nr, piece_costs, np, first_run, n_runs_of_word, nullptr, nw, I); rc != STR_ER_OK) return rc;
    std::vector<int32_t> pslot;
    uint64_t             n_pslots = 0;
    LtTab                H{}, D{};
    if (const int rc = lattice_track_enqueue(c, s, at, I.splits, I.costs, I.costs + rs::ALPHABET * nr, I.first, I.n_of, splits, first_run, n_runs_of_word, nw, track_first,
                                             track_count, members, nm, nt, pslot, &n_pslots, H, D);
        rc != STR_ER_OK)
        return rc;
    HIP_TRY(c, hipMemcpyAsync(c->lt_tab.h() + H.o_matches, c->lt_tab.d() + H.o_matches, H.down_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    uint64_t total = 0;
    if (!lt_compact(H, pslot, n_pslots, nullptr, nullptr, &total)) return fail(c, STR_ER_EHIP, "lattice track: a member's parts outside its slots (internal error)");
    *n_parts = (int32_t)total;
    if (total > (uint64_t)cap_parts) return fail(c, STR_ER_ECAPACITY, std::to_string(total) + " parts, cap_parts is " + std::to_string(cap_parts));
    lt_compact(H, pslot, n_pslots, members_out, parts, &total);
    if (nt > 0) std::memcpy(out, H.matches, sizeof(str_er_track_match) * nt);
    if (nm > 0) std::memcpy(src, H.src, lm::SRC_BYTES * nm);
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_lattice_match_tracks_host(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                                     const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, const int32_t *track_first,
                                     const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks, const char *bytes,
                                     const int32_t *offsets, int32_t n, uint32_t flags, int32_t ins, int32_t del, int32_t band, int32_t split_cost,
                                     str_er_track_match *out, str_er_lattice_track_member *members_out, uint8_t *src, str_er_split_part *parts,
                                     int32_t cap_parts, int32_t *n_parts)
try {
    using namespace str_er_host;
    if (!args_ok(splits, n_runs, run_costs, piece_costs, n_pieces, first_run, n_runs_of_word, n_words, track_first, track_count, members, n_members, n_tracks, out,
                 members_out, src, parts, cap_parts, n_parts))
        return STR_ER_EINVAL;
    *n_parts = 0;
    if (const int rc = wm::lexicon_check(bytes, offsets, n, flags, nullptr); rc != STR_ER_OK) return rc;
    if (!lm::params_ok(ins, del, band, split_cost) || !rs::splits_ok(splits, n_runs, n_pieces) || !words_in_rows(n_runs, first_run, n_runs_of_word, n_words))
        return STR_ER_EINVAL;
    if (const int rc = tr::tracks_check(track_first, track_count, members, n_members, n_tracks, n_words); rc != STR_ER_OK) return rc;
    // every track once, its members' parts behind those of the slots before; the count is set even where cap_parts is too small, and
    // nothing is written to the caller's arrays before it is known to fit
    const std::vector<uint8_t> lab = lexicon_labels(bytes, offsets, n);
    const int32_t              zero = 0;
    const lm::Params           p{ins, del, band, split_cost};
    std::vector<str_er_track_match>          recs((size_t)n_tracks);
    std::vector<str_er_lattice_track_member> mrec((size_t)n_members, str_er_lattice_track_member{-1, 0, 0, 0, 0, -1});
    std::vector<uint8_t>                     from(lm::SRC_BYTES * (size_t)n_members, 0xFF);
    std::vector<str_er_split_part>           all;
    for (int32_t g = 0; g < n_tracks; ++g) {
        const size_t f = (size_t)track_first[g];
        recs[(size_t)g] = lt::match_track(splits, run_costs, piece_costs, first_run, n_runs_of_word, members + f, track_count[g], lab.data(), n > 0 ? offsets : &zero, n, p,
                                          (flags & STR_ER_LEXICON_FOLD_CASE) != 0, mrec.data() + f, from.data() + lm::SRC_BYTES * f, all);
        if (all.size() > 0x7FFFFFFFull) return STR_ER_ECAPACITY;
    }
    {          // the first part of every slot (a slot of no track: where the parts of the slots before it end)
        size_t fp = 0;
        for (size_t i = 0; i < mrec.size(); ++i) { mrec[i].first_part = (int32_t)fp; fp += (size_t)mrec[i].n_parts; }
    }
    *n_parts = (int32_t)all.size();
    if (all.size() > (size_t)cap_parts) return STR_ER_ECAPACITY;
    if (n_tracks > 0) std::memcpy(out, recs.data(), sizeof(str_er_track_match) * recs.size());
    if (n_members > 0) {
        std::memcpy(members_out, mrec.data(), sizeof(str_er_lattice_track_member) * mrec.size());
        std::memcpy(src, from.data(), from.size());
    }
    if (!all.empty()) std::memcpy(parts, all.data(), sizeof(str_er_split_part) * all.size());
    return STR_ER_OK;
} catch (...) { return STR_ER_ENOMEM; }

const str_er_track_match *str_er_result_lattice_track_matches(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_lattice_track, &str_er_result::lattice_track_matches, n);
}
const str_er_lattice_track_member *str_er_result_lattice_track_members(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_lattice_track, &str_er_result::lattice_track_members, n);
}
const uint8_t *str_er_result_lattice_track_src(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_lattice_track, &str_er_result::lattice_track_src, n_bytes);
}
const str_er_split_part *str_er_result_lattice_track_parts(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_lattice_track, &str_er_result::lattice_track_parts, n);
}

} // extern "C"
