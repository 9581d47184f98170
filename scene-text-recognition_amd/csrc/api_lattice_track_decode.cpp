// api_lattice_track_decode.cpp -- the C ABI, part 8m: the track decode over the members' piece lattices (str_er_set_lattice_track_decode
// beside STR_ER_WANT_TRACK_DECODE and STR_ER_WANT_LATTICE_DECODE behind the lattice decode in api_run_read.cpp,
// str_er_lattice_decode_tracks on the caller's rows and tracks; the contract is at str_er_lattice_track_decode in str_er.h).  The rules
// are lattice_track_decode_rules.h: the pure host entry point here runs them as they stand after the checks of both parents; the kernels
// (lattice_track_decode_kernels.h) read what k_lattice_decode reads and left, and the tracks as k_track_decode takes them.
#include "str_er_ctx.h"
#include "lattice_decode_kernels.h"
#include "lattice_track_decode_kernels.h"
#include "lattice_track_decode_rules.h"

namespace ltd = str_er_ltd;
namespace ld = str_er_ld;
namespace lm = str_er_lm;
namespace rs = str_er_rs;
namespace td = str_er_td;

static_assert(sizeof(str_er_lattice_track_member) == 24 && sizeof(str_er_track_decode) == 32, "lattice track decode layout");

namespace str_er_host {

LtdTab ltd_layout(uint8_t *base, size_t at, size_t n_words, size_t n_tracks, size_t n_members, size_t n_pslots)
{
    LtdTab t{};
    Carve  cv{at};
    t.o_up = cv.take(4 * n_tracks);
    const size_t o_count = cv.take(4 * n_tracks), o_mem = cv.take(4 * n_members), o_st = cv.take(4 * n_members), o_ps = cv.take(4 * n_members);
    t.up_bytes = cv.off - t.o_up;
    const size_t o_tab = cv.take(4 * (size_t)str_er::LT_TAB_INTS * n_words);
    t.o_out = cv.take(sizeof(str_er_track_decode) * n_tracks);
    const size_t o_chars = cv.take(ltd::MAX_LEN * n_tracks), o_mrec = cv.take(sizeof(str_er_lattice_track_member) * n_members), o_src = cv.take(lm::SRC_BYTES * n_members),
                 o_parts = cv.take(sizeof(str_er_split_part) * n_pslots);
    t.down_bytes = cv.off - t.o_out;
    t.bytes = cv.off;
    if (base) {
        const auto i32 = [&](size_t o) { return reinterpret_cast<int32_t *>(base + o); };
        t.first = i32(t.o_up); t.count = i32(o_count); t.members = i32(o_mem); t.slot_track = i32(o_st); t.pslot = i32(o_ps); t.tab = i32(o_tab);
        t.out = reinterpret_cast<str_er_track_decode *>(base + t.o_out); t.chars = base + o_chars;
        t.mrec = reinterpret_cast<str_er_lattice_track_member *>(base + o_mrec); t.src = base + o_src; t.parts = reinterpret_cast<str_er_split_part *>(base + o_parts);
    }
    return t;
}

// the part slots of a member slot: its word's nodes, none for an unusable member and for a slot of no track; false above 2^31 - 1
static bool ltd_part_slots(const str_er_run_split *splits, const int32_t *first_run, const int32_t *n_of, const int32_t *track_first, const int32_t *track_count,
                           const int32_t *members, size_t n_members, size_t n_tracks, std::vector<int32_t> &slot_track, std::vector<int32_t> &pslot, uint64_t *n_pslots)
{
    slot_track.assign(n_members, -1);
    for (size_t g = 0; g < n_tracks; ++g)
        for (int32_t j = 0; j < track_count[g]; ++j) slot_track[(size_t)track_first[g] + (size_t)j] = (int32_t)g;
    pslot.assign(n_members, 0);
    uint64_t total = 0;
    for (size_t i = 0; i < n_members; ++i) {
        pslot[i] = (int32_t)total;
        const int32_t w = members[i];
        const int64_t N = slot_track[i] < 0 ? 0 : lm::word_nodes(splits, first_run[w], n_of[w]);
        total += N <= lm::MAX_NODES ? (uint64_t)N : 0;
        if (total > 0x7FFFFFFFull) return false;
    }
    *n_pslots = total;
    return true;
}

int lattice_track_decode_enqueue(str_er_ctx *c, hipStream_t s, size_t at, const str_er_run_split *d_splits, const uint8_t *d_run_costs, const uint8_t *d_piece_costs,
                                 const int32_t *d_first, const int32_t *d_n_of, const void *d_dec, const uint8_t *d_dchars, const str_er_run_split *splits,
                                 const int32_t *first_run, const int32_t *n_of, size_t n_words, const int32_t *track_first, const int32_t *track_count,
                                 const int32_t *members, size_t n_members, size_t n_tracks, std::vector<int32_t> &pslot, uint64_t *n_pslots, LtdTab &H, LtdTab &D)
{
    if (n_tracks > 0x7FFFFFFFull / 32 || n_words > 0x7FFFFFFFull / (4 * (size_t)str_er::LT_TAB_INTS) || n_members > 0x7FFFFFFFull / 32)
        return fail(c, STR_ER_ECAPACITY, "lattice track decode: too many tracks, words or members");
    std::vector<int32_t> slot_track;
    if (!ltd_part_slots(splits, first_run, n_of, track_first, track_count, members, n_members, n_tracks, slot_track, pslot, n_pslots))
        return fail(c, STR_ER_ECAPACITY, "lattice track decode: more than 2^31 parts to reserve");
    if (const int rc = c->ltd_tab.ensure(c, ltd_layout(nullptr, at, n_words, n_tracks, n_members, (size_t)*n_pslots).bytes, "lattice track decode tables"); rc != STR_ER_OK)
        return rc;
    H = ltd_layout(c->ltd_tab.h(), at, n_words, n_tracks, n_members, (size_t)*n_pslots);
    D = ltd_layout(c->ltd_tab.d(), at, n_words, n_tracks, n_members, (size_t)*n_pslots);
    if (n_tracks > 0) {
        std::memcpy(H.first, track_first, 4 * n_tracks);
        std::memcpy(H.count, track_count, 4 * n_tracks);
    }
    if (n_members > 0) {
        std::memcpy(H.members, members, 4 * n_members);
        std::memcpy(H.slot_track, slot_track.data(), 4 * n_members);
        std::memcpy(H.pslot, pslot.data(), 4 * n_members);
    }
    HIP_TRY(c, hipMemcpyAsync(c->ltd_tab.d() + H.o_up, c->ltd_tab.h() + H.o_up, H.up_bytes, hipMemcpyHostToDevice, s));
    launch_lattice_track_decode(s, c->bigram.d(), c->td_ins, c->td_del, c->td_rounds, c->rs_split, d_splits, d_run_costs, d_piece_costs, d_first, d_n_of, (int)n_words, d_dec,
                                d_dchars, D.first, D.count, D.members, D.slot_track, D.pslot, (int)n_members, (int)n_tracks, D.tab, D.out, D.chars,
                                reinterpret_cast<int32_t *>(D.mrec), D.src, reinterpret_cast<int32_t *>(D.parts));
    HIP_TRY(c, hipGetLastError());
    return STR_ER_OK;
}

bool ltd_compact(const LtdTab &H, const std::vector<int32_t> &pslot, uint64_t n_pslots, str_er_lattice_track_member *mrec, str_er_split_part *parts, uint64_t *n_parts)
{
    LtTab V{};          // (the member records and their part slots are laid out as the lattice track match's)
    V.mrec = H.mrec; V.parts = H.parts;
    return lt_compact(V, pslot, n_pslots, mrec, parts, n_parts);
}

} // namespace str_er_host

namespace {

bool args_ok(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces, const int32_t *first_run,
             const int32_t *n_of, int32_t n_words, const int32_t *track_first, const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks,
             const str_er_track_decode *out, const uint8_t *chars, const str_er_lattice_track_member *members_out, const uint8_t *src, const str_er_split_part *parts,
             int32_t cap_parts, const int32_t *n_parts)
{
    return n_runs >= 0 && n_pieces >= 0 && n_words >= 0 && n_members >= 0 && n_tracks >= 0 && cap_parts >= 0 && n_parts && (n_runs == 0 || (splits && run_costs)) &&
           (n_pieces == 0 || piece_costs) && (n_words == 0 || (first_run && n_of)) && (n_tracks == 0 || (track_first && track_count && out && chars)) &&
           (n_members == 0 || (members && members_out && src)) && (cap_parts == 0 || parts);
}

} // namespace

extern "C" {

int str_er_set_lattice_track_decode(str_er_ctx *c, int32_t on)
try {
    if (!c) return STR_ER_EINVAL;
    if (on != 0 && on != 1) return fail(c, STR_ER_EINVAL, "lattice track decode: the setting is 0 or 1");
    c->ltd_on = on != 0;
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_lattice_track_decode_stats(const str_er_ctx *c, uint64_t *table_bytes)
{
    if (!c) return STR_ER_EINVAL;
    if (table_bytes) *table_bytes = c->ltd_tab.size();
    return STR_ER_OK;
}

int str_er_lattice_decode_tracks(str_er_ctx *c, const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                                 const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, const int32_t *track_first, const int32_t *track_count,
                                 const int32_t *members, int32_t n_members, int32_t n_tracks, str_er_track_decode *out, uint8_t *chars,
                                 str_er_lattice_track_member *members_out, uint8_t *src, str_er_split_part *parts, int32_t cap_parts, int32_t *n_parts)
try {
    using namespace str_er_host;
    if (!c) return STR_ER_EINVAL;
    if (!args_ok(splits, n_runs, run_costs, piece_costs, n_pieces, first_run, n_runs_of_word, n_words, track_first, track_count, members, n_members, n_tracks, out, chars,
                 members_out, src, parts, cap_parts, n_parts))
        return fail(c, STR_ER_EINVAL, "bad arguments");
    *n_parts = 0;
    if (!c->bigram_set) return fail(c, STR_ER_ESTATE, "str_er_lattice_decode_tracks needs a bigram table (str_er_set_bigram)");
    if (!rs::splits_ok(splits, n_runs, n_pieces)) return fail(c, STR_ER_EINVAL, "lattice track decode: a record with cuts or pieces that are none");
    if (!words_in_rows(n_runs, first_run, n_runs_of_word, n_words)) return fail(c, STR_ER_EINVAL, "lattice track decode: a word outside the glyph runs");
    if (const int rc = td::tracks_check(track_first, track_count, members, n_members, n_tracks, n_words); rc != STR_ER_OK)
        return fail(c, rc, rc == STR_ER_ECAPACITY ? "lattice track decode: a track of more than 1024 members"
                                                  : "lattice track decode: a member outside the words, or tracks that do not ascend in the member array");
    if (n_tracks == 0 && n_members == 0) return STR_ER_OK;
    const size_t nr = (size_t)n_runs, np = (size_t)n_pieces, nw = (size_t)n_words, nm = (size_t)n_members, nt = (size_t)n_tracks;
    if (nr + np > 0x7FFFFFFFull / 65 || nw > 0x7FFFFFFFull / 64) return fail(c, STR_ER_ECAPACITY, "lattice track decode: too many rows or words");
    std::vector<int32_t> slot;
    uint64_t             n_slots = 0;
    if (!rs_word_slots(splits, first_run, n_runs_of_word, nw, slot, &n_slots)) return fail(c, STR_ER_ECAPACITY, "lattice track decode: more than 2^31 parts to reserve");
    // the rows and the words' (first, n, slot) at the front of the buffer, the lattice decoder's tables behind them, the tracks' behind
    // those.  The buffer is sized for all of it before anything goes up: a later ensure must not move what the first upload reads
    const size_t at_dec = rows_in_layout(nullptr, nr, nr + np, nw, true).bytes, at = ld_layout(nullptr, at_dec, nw, (size_t)n_slots).bytes;
    {
        uint64_t need = 0;
        for (size_t i = 0; i < nm; ++i) {
            const int64_t N = lm::word_nodes(splits, first_run[members[i]], n_runs_of_word[members[i]]);
            need += N <= lm::MAX_NODES ? (uint64_t)N : 0;
        }
        if (need > 0x7FFFFFFFull) return fail(c, STR_ER_ECAPACITY, "lattice track decode: more than 2^31 parts to reserve");
        if (const int rc = c->ltd_tab.ensure(c, ltd_layout(nullptr, at, nw, nt, nm, (size_t)need).bytes, "lattice track decode tables"); rc != STR_ER_OK) return rc;
    }
    const LdTab W = ld_layout(c->ltd_tab.d(), at_dec, nw, (size_t)n_slots);
    hipStream_t s = c->stream;
    RowsIn      I{};
    if (const int rc = rows_in_upload(c, s, c->ltd_tab, splits, run_costs, nr, piece_costs, np, first_run, n_runs_of_word, slot.data(), nw, I); rc != STR_ER_OK) return rc;
    if (n_words > 0)          // the seeds: the lattice decoder on every word
        launch_lattice_decode(s, c->bigram.d(), c->wd_ins, c->wd_del, c->rs_split, I.splits, I.costs, I.costs + rs::ALPHABET * nr, I.first, I.n_of, I.slot, n_words,
                              reinterpret_cast<int32_t *>(W.dec), W.chars, W.src, reinterpret_cast<int32_t *>(W.parts));
    HIP_TRY(c, hipGetLastError());
    std::vector<int32_t> pslot;
    uint64_t             n_pslots = 0;
    LtdTab               H{}, D{};
    if (const int rc = lattice_track_decode_enqueue(c, s, at, I.splits, I.costs, I.costs + rs::ALPHABET * nr, I.first, I.n_of, W.dec, W.chars, splits, first_run,
                                                    n_runs_of_word, nw, track_first, track_count, members, nm, nt, pslot, &n_pslots, H, D);
        rc != STR_ER_OK)
        return rc;
    HIP_TRY(c, hipMemcpyAsync(c->ltd_tab.h() + H.o_out, c->ltd_tab.d() + H.o_out, H.down_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    uint64_t total = 0;
    if (!ltd_compact(H, pslot, n_pslots, nullptr, nullptr, &total)) return fail(c, STR_ER_EHIP, "lattice track decode: a member's parts outside its slots (internal error)");
    *n_parts = (int32_t)total;
    if (total > (uint64_t)cap_parts) return fail(c, STR_ER_ECAPACITY, std::to_string(total) + " parts, cap_parts is " + std::to_string(cap_parts));
    ltd_compact(H, pslot, n_pslots, members_out, parts, &total);
    if (nt > 0) {
        std::memcpy(out, H.out, sizeof(str_er_track_decode) * nt);
        std::memcpy(chars, H.chars, ltd::MAX_LEN * nt);
    }
    if (nm > 0) std::memcpy(src, H.src, lm::SRC_BYTES * nm);
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_lattice_decode_tracks_host(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                                      const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, const int32_t *track_first,
                                      const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks, const uint8_t *bigram,
                                      int32_t dec_ins, int32_t dec_del, int32_t ins, int32_t del, int32_t rounds, int32_t split_cost, str_er_track_decode *out,
                                      uint8_t *chars, str_er_lattice_track_member *members_out, uint8_t *src, str_er_split_part *parts, int32_t cap_parts,
                                      int32_t *n_parts)
try {
    using namespace str_er_host;
    if (!args_ok(splits, n_runs, run_costs, piece_costs, n_pieces, first_run, n_runs_of_word, n_words, track_first, track_count, members, n_members, n_tracks, out, chars,
                 members_out, src, parts, cap_parts, n_parts) ||
        !bigram)
        return STR_ER_EINVAL;
    *n_parts = 0;
    if (!ld::params_ok(dec_ins, dec_del, split_cost) || !ltd::params_ok(ins, del, rounds, split_cost) || !rs::splits_ok(splits, n_runs, n_pieces) ||
        !words_in_rows(n_runs, first_run, n_runs_of_word, n_words))
        return STR_ER_EINVAL;
    if (const int rc = td::tracks_check(track_first, track_count, members, n_members, n_tracks, n_words); rc != STR_ER_OK) return rc;
    // the seeds' strings: the lattice decoder on every word, as the device entry point makes them
    std::vector<str_er_lattice_decode> dec((size_t)n_words);
    std::vector<uint8_t>               dchars((size_t)n_words * ld::MAX_CHARS), dsrc(ld::MAX_CHARS);
    str_er_split_part                  dparts[ld::MAX_NODES];
    for (int32_t w = 0; w < n_words; ++w)
        dec[(size_t)w] = ld::decode_word(splits, run_costs, piece_costs, first_run[w], n_runs_of_word[w], bigram, dec_ins, dec_del, split_cost,
                                         dchars.data() + (size_t)w * ld::MAX_CHARS, dsrc.data(), dparts);
    // every track once, its members' parts behind those of the slots before; the count is set even where cap_parts is too small, and
    // nothing is written to the caller's arrays before it is known to fit
    const lm::Params                         p{ins, del, 0, split_cost};
    std::vector<str_er_track_decode>         recs((size_t)n_tracks);
    std::vector<uint8_t>                     lab(ltd::MAX_LEN * (size_t)n_tracks, 0xFF);
    std::vector<str_er_lattice_track_member> mrec((size_t)n_members, str_er_lattice_track_member{-1, 0, 0, 0, 0, -1});
    std::vector<uint8_t>                     from(lm::SRC_BYTES * (size_t)n_members, 0xFF);
    std::vector<str_er_split_part>           all;
    for (int32_t g = 0; g < n_tracks; ++g) {
        const size_t f = (size_t)track_first[g];
        recs[(size_t)g] = ltd::decode_track(splits, run_costs, piece_costs, first_run, n_runs_of_word, members + f, track_count[g], dec.data(), dchars.data(), bigram, p,
                                            rounds, lab.data() + ltd::MAX_LEN * (size_t)g, mrec.data() + f, from.data() + lm::SRC_BYTES * f, all);
        if (all.size() > 0x7FFFFFFFull) return STR_ER_ECAPACITY;
    }
    {          // the first part of every slot (a slot of no track: where the parts of the slots before it end)
        size_t fp = 0;
        for (size_t i = 0; i < mrec.size(); ++i) { mrec[i].first_part = (int32_t)fp; fp += (size_t)mrec[i].n_parts; }
    }
    *n_parts = (int32_t)all.size();
    if (all.size() > (size_t)cap_parts) return STR_ER_ECAPACITY;
    if (n_tracks > 0) {
        std::memcpy(out, recs.data(), sizeof(str_er_track_decode) * recs.size());
        std::memcpy(chars, lab.data(), lab.size());
    }
    if (n_members > 0) {
        std::memcpy(members_out, mrec.data(), sizeof(str_er_lattice_track_member) * mrec.size());
        std::memcpy(src, from.data(), from.size());
    }
    if (!all.empty()) std::memcpy(parts, all.data(), sizeof(str_er_split_part) * all.size());
    return STR_ER_OK;
} catch (...) { return STR_ER_ENOMEM; }

const str_er_track_decode *str_er_result_lattice_track_decodes(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_lattice_track_decodes, &str_er_result::lattice_track_decodes, n);
}
const uint8_t *str_er_result_lattice_track_decode_chars(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_lattice_track_decodes, &str_er_result::lattice_track_decode_chars, n_bytes);
}
const str_er_lattice_track_member *str_er_result_lattice_track_decode_members(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_lattice_track_decodes, &str_er_result::lattice_track_decode_members, n);
}
const uint8_t *str_er_result_lattice_track_decode_src(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_lattice_track_decodes, &str_er_result::lattice_track_decode_src, n_bytes);
}
const str_er_split_part *str_er_result_lattice_track_decode_parts(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_lattice_track_decodes, &str_er_result::lattice_track_decode_parts, n);
}

} // extern "C"
