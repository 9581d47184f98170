// api_track_read.cpp -- the C ABI, part 8g: the word tracks and the track match (STR_ER_WANT_TRACK_READ behind the matcher in
// api_run_read.cpp, str_er_word_links / str_er_word_tracks_from_links on the caller's tables, str_er_match_tracks on the caller's cost
// rows; the contract is at str_er_word_link in str_er.h).  The rules are track_read_rules.h: the pure host entry points here run them
// as they stand after checking their arguments; the device side is track_match_kernels.h on the matcher's lexicon.
#include "str_er_ctx.h"
#include "track_read_rules.h"

namespace wm = str_er_wm;
namespace tr = str_er_tr;

static_assert(sizeof(str_er_word_link) == 16 && sizeof(str_er_word_track) == 24 && sizeof(str_er_track_match) == 32, "track read layout");

namespace str_er_host {

TmTab tm_layout(uint8_t *base, size_t n_tracks, size_t n_members, int n_chunks)
{
    TmTab t{};
    Carve cv;
    const size_t o_first = cv.take(4 * n_tracks), o_count = cv.take(4 * n_tracks), o_mem = cv.take(4 * n_members);
    t.up_bytes = cv.off;
    const size_t o_part = cv.take(16 * n_tracks * (size_t)n_chunks);
    t.o_matches = cv.take(sizeof(str_er_track_match) * n_tracks);
    t.o_mcost = cv.take(4 * n_members);
    t.bytes = cv.off;
    if (base) {
        t.first = reinterpret_cast<int32_t *>(base + o_first); t.count = reinterpret_cast<int32_t *>(base + o_count);
        t.members = reinterpret_cast<int32_t *>(base + o_mem); t.partial = reinterpret_cast<uint64_t *>(base + o_part);
        t.matches = reinterpret_cast<str_er_track_match *>(base + t.o_matches); t.member_cost = reinterpret_cast<int32_t *>(base + t.o_mcost);
    }
    return t;
}

int track_match_enqueue(str_er_ctx *c, hipStream_t s, const uint8_t *d_rows, const int32_t *d_first, const int32_t *d_n_of, const int32_t *track_first,
                        const int32_t *track_count, const int32_t *members, size_t n_members, size_t n_tracks, TmTab &D)
{
    const int n_chunks = tm_chunks(c->lex);
    if (n_tracks > 0x7FFFFFFFull / (size_t)n_chunks / 2) return fail(c, STR_ER_ECAPACITY, "track match: too many tracks for this lexicon");
    if (const int rc = c->tm_tab.ensure(c, tm_layout(nullptr, n_tracks, n_members, n_chunks).bytes, "track match tables"); rc != STR_ER_OK) return rc;
    const TmTab H = tm_layout(c->tm_tab.h(), n_tracks, n_members, n_chunks);
    D = tm_layout(c->tm_tab.d(), n_tracks, n_members, n_chunks);
    std::memcpy(H.first, track_first, 4 * n_tracks);
    std::memcpy(H.count, track_count, 4 * n_tracks);
    if (n_members > 0) std::memcpy(H.members, members, 4 * n_members);
    HIP_TRY(c, hipMemcpyAsync(c->tm_tab.d(), c->tm_tab.h(), H.up_bytes, hipMemcpyHostToDevice, s));
    if (n_members > 0) HIP_TRY(c, hipMemsetAsync(D.member_cost, 0xFF, 4 * n_members, s));          // (-1 in a slot of no track)
    launch_track_match(s, c->lex, c->wm_prm, d_rows, d_first, d_n_of, D.first, D.count, D.members, (int)n_tracks, D.partial, D.matches, D.member_cost);
    HIP_TRY(c, hipGetLastError());
    return STR_ER_OK;
}

} // namespace str_er_host

namespace {

using tr::tracks_check;

bool track_args_ok(const uint8_t *costs, int32_t n_rows, const int32_t *first_run, const int32_t *n_of, int32_t n_words, const int32_t *track_first,
                   const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks, const str_er_track_match *out,
                   const int32_t *member_cost)
{
    return n_rows >= 0 && n_words >= 0 && n_members >= 0 && n_tracks >= 0 && (n_rows == 0 || costs) && (n_words == 0 || (first_run && n_of)) &&
           (n_tracks == 0 || (track_first && track_count && out)) && (n_members == 0 || (members && member_cost));
}

} // namespace

extern "C" {

int str_er_set_word_link(str_er_ctx *c, int32_t num, int32_t den)
try {
    if (!c) return STR_ER_EINVAL;
    if (!tr::link_params_ok(num, den)) return fail(c, STR_ER_EINVAL, "word link: num and den are in 1 .. 65535");
    c->wlink_num = num; c->wlink_den = den;
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_word_links(const str_er_line_foot *feet, const uint32_t *frames_of_lines, const int32_t *line_tracks, int32_t n_lines, const int32_t *frame_wh,
                      int32_t n_frames, const str_er_line_word *words, int32_t n_words, int32_t num, int32_t den, uint8_t *reading, str_er_word_link *links,
                      int32_t cap_links, int32_t *n_links)
try {
    if (n_lines < 0 || n_frames < 0 || n_words < 0 || !n_links || !tr::link_params_ok(num, den) || (links && cap_links < 0)) return STR_ER_EINVAL;
    if ((n_lines > 0 && (!feet || !frames_of_lines || !line_tracks || !reading)) || (n_frames > 0 && !frame_wh) || (n_words > 0 && !words)) return STR_ER_EINVAL;
    for (int32_t t = 0; t < n_lines; ++t)
        if (frames_of_lines[t] >= (uint32_t)n_frames || line_tracks[t] < 0) return STR_ER_EINVAL;
    for (int32_t w = 0; w < n_words; ++w)
        if (words[w].line < 0 || words[w].line >= n_lines || !tr::box_ok(words[w])) return STR_ER_EINVAL;
    tr::reading_lines(feet, frames_of_lines, line_tracks, n_lines, reading);
    std::vector<str_er_word_link> out;
    tr::word_links(frames_of_lines, line_tracks, reading, n_lines, frame_wh, words, n_words, num, den, out);
    if (out.size() > 0x7FFFFFFFull) return STR_ER_ECAPACITY;
    *n_links = (int32_t)out.size();
    if (!links) return STR_ER_OK;
    if ((int32_t)out.size() > cap_links) return STR_ER_ECAPACITY;
    if (!out.empty()) std::memcpy(links, out.data(), sizeof(str_er_word_link) * out.size());
    return STR_ER_OK;
} catch (...) { return STR_ER_ENOMEM; }

int str_er_word_tracks_from_links(const uint32_t *frames_of_lines, const int32_t *line_tracks, const uint8_t *reading, int32_t n_lines,
                                  const str_er_line_word *words, int32_t n_words, const str_er_word_link *links, int32_t n_links, int32_t *track_of_words,
                                  str_er_word_track *tracks, int32_t cap_tracks, int32_t *n_tracks, int32_t *members)
try {
    if (n_lines < 0 || n_words < 0 || n_links < 0 || !n_tracks || (tracks && cap_tracks < 0)) return STR_ER_EINVAL;
    if ((n_lines > 0 && (!frames_of_lines || !line_tracks || !reading)) || (n_words > 0 && (!words || !track_of_words)) || (n_links > 0 && !links) ||
        (tracks && n_words > 0 && !members))
        return STR_ER_EINVAL;
    for (int32_t w = 0; w < n_words; ++w)
        if (words[w].line < 0 || words[w].line >= n_lines) return STR_ER_EINVAL;
    for (int32_t k = 0; k < n_links; ++k) {
        const str_er_word_link &P = links[k];
        if (P.a < 0 || P.a >= n_words || P.b < 0 || P.b >= n_words || !reading[words[P.a].line] || !reading[words[P.b].line]) return STR_ER_EINVAL;
    }
    std::vector<int32_t>           track_of, mem;
    std::vector<str_er_word_track> out;
    tr::word_tracks(frames_of_lines, line_tracks, reading, words, n_words, links, n_links, track_of, out, mem);
    if (n_words > 0) std::memcpy(track_of_words, track_of.data(), 4 * (size_t)n_words);
    *n_tracks = (int32_t)out.size();
    if (!tracks) return STR_ER_OK;
    if ((int32_t)out.size() > cap_tracks) return STR_ER_ECAPACITY;
    if (!out.empty()) std::memcpy(tracks, out.data(), sizeof(str_er_word_track) * out.size());
    if (!mem.empty()) std::memcpy(members, mem.data(), 4 * mem.size());
    return STR_ER_OK;
} catch (...) { return STR_ER_ENOMEM; }

int str_er_match_tracks(str_er_ctx *c, const uint8_t *costs, int32_t n_rows, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words,
                        const int32_t *track_first, const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks,
                        str_er_track_match *out, int32_t *member_cost)
try {
    if (!c) return STR_ER_EINVAL;
    if (!track_args_ok(costs, n_rows, first_run, n_runs_of_word, n_words, track_first, track_count, members, n_members, n_tracks, out, member_cost))
        return fail(c, STR_ER_EINVAL, "bad arguments");
    if (c->lex_n <= 0) return fail(c, STR_ER_ESTATE, "str_er_match_tracks needs a lexicon (str_er_set_lexicon)");
    if (!words_in_rows(n_rows, first_run, n_runs_of_word, n_words)) return fail(c, STR_ER_EINVAL, "track match: a word outside the cost rows");
    if (const int rc = tracks_check(track_first, track_count, members, n_members, n_tracks, n_words); rc != STR_ER_OK)
        return fail(c, rc, rc == STR_ER_ECAPACITY ? "track match: a track of more than 65536 members"
                                                  : "track match: a member outside the words, or tracks that do not ascend in the member array");
    for (int32_t i = 0; i < n_members; ++i) member_cost[i] = -1;
    if (n_tracks == 0) return STR_ER_OK;
    // the rows and the words' (first, n) in the matcher's buffer, as for str_er_match_words
    if (const int rc = c->wm_tab.ensure(c, rows_in_layout(nullptr, 0, (size_t)n_rows, (size_t)n_words, false).bytes, "word match tables"); rc != STR_ER_OK) return rc;
    hipStream_t s = c->stream;
    RowsIn      I{};
    if (const int rc = rows_in_upload(c, s, c->wm_tab, nullptr, costs, (size_t)n_rows, nullptr, 0, first_run, n_runs_of_word, nullptr, (size_t)n_words, I); rc != STR_ER_OK) return rc;
    TmTab T{};
    if (const int rc = track_match_enqueue(c, s, I.costs, I.first, I.n_of, track_first, track_count, members, (size_t)n_members, (size_t)n_tracks, T); rc != STR_ER_OK)
        return rc;
    const size_t down = T.o_mcost + 4 * (size_t)n_members - T.o_matches;          // (matches | member costs lie back to back)
    HIP_TRY(c, hipMemcpyAsync(c->tm_tab.h() + T.o_matches, c->tm_tab.d() + T.o_matches, down, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    std::memcpy(out, c->tm_tab.h() + T.o_matches, sizeof(str_er_track_match) * (size_t)n_tracks);
    if (n_members > 0) std::memcpy(member_cost, c->tm_tab.h() + T.o_mcost, 4 * (size_t)n_members);
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_match_tracks_host(const uint8_t *costs, int32_t n_rows, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words,
                             const int32_t *track_first, const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks,
                             const char *bytes, const int32_t *offsets, int32_t n, uint32_t flags, int32_t ins, int32_t del, int32_t band,
                             str_er_track_match *out, int32_t *member_cost)
try {
    if (!track_args_ok(costs, n_rows, first_run, n_runs_of_word, n_words, track_first, track_count, members, n_members, n_tracks, out, member_cost))
        return STR_ER_EINVAL;
    if (const int rc = wm::lexicon_check(bytes, offsets, n, flags, nullptr); rc != STR_ER_OK) return rc;
    if (!wm::params_ok(ins, del, band) || !words_in_rows(n_rows, first_run, n_runs_of_word, n_words)) return STR_ER_EINVAL;
    if (const int rc = tracks_check(track_first, track_count, members, n_members, n_tracks, n_words); rc != STR_ER_OK) return rc;
    const std::vector<uint8_t> lab = lexicon_labels(bytes, offsets, n);
    const int32_t         zero = 0;
    const wm::MatchParams p{ins, del, band};
    for (int32_t i = 0; i < n_members; ++i) member_cost[i] = -1;
    for (int32_t g = 0; g < n_tracks; ++g)
        out[g] = tr::match_track(costs, first_run, n_runs_of_word, members + track_first[g], track_count[g], lab.data(), n > 0 ? offsets : &zero, n, p,
                                 (flags & STR_ER_LEXICON_FOLD_CASE) != 0, member_cost + track_first[g]);
    return STR_ER_OK;
} catch (...) { return STR_ER_ENOMEM; }

const str_er_word_link *str_er_result_word_links(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_word_tracks, &str_er_result::word_links, n);
}
const str_er_word_track *str_er_result_word_tracks(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_word_tracks, &str_er_result::word_tracks, n);
}
const int32_t *str_er_result_word_track_members(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_word_tracks, &str_er_result::word_track_members, n);
}
const int32_t *str_er_result_word_track_of_words(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_word_tracks, &str_er_result::word_track_of_words, n);
}
const str_er_track_match *str_er_result_track_matches(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_track_read, &str_er_result::track_matches, n);
}
const int32_t *str_er_result_track_member_costs(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_track_read, &str_er_result::track_member_costs, n);
}

} // extern "C"
