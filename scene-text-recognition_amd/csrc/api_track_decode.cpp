// api_track_decode.cpp -- the C ABI, part 8k: the track decode (STR_ER_WANT_TRACK_DECODE behind the decoder in api_run_read.cpp,
// str_er_decode_tracks on the caller's cost rows; the contract is at str_er_track_decode in str_er.h).  The rules are
// track_decode_rules.h: the pure host entry point here runs them as they stand after checking its arguments; the device side is
// track_decode_kernels.h behind k_word_decode, whose strings are the seeds.
#include "str_er_ctx.h"
#include "track_decode_kernels.h"
#include "track_decode_rules.h"

namespace td = str_er_td;
namespace wd = str_er_wd;

static_assert(sizeof(str_er_track_decode) == 32, "track decode layout");

namespace str_er_host {

TdTab td_layout(uint8_t *base, size_t at, size_t n_tracks, size_t n_members)
{
    TdTab t{};
    Carve cv{at};
    t.o_up = cv.take(4 * n_tracks);
    const size_t o_count = cv.take(4 * n_tracks), o_mem = cv.take(4 * n_members);
    t.up_bytes = cv.off - t.o_up;
    t.o_out = cv.take(sizeof(str_er_track_decode) * n_tracks);
    const size_t o_chars = cv.take(td::MAX_LEN * n_tracks), o_mcost = cv.take(4 * n_members);
    t.bytes = cv.off;
    t.down_bytes = cv.off - t.o_out;
    if (base) {
        t.first = reinterpret_cast<int32_t *>(base + t.o_up); t.count = reinterpret_cast<int32_t *>(base + o_count);
        t.members = reinterpret_cast<int32_t *>(base + o_mem); t.out = reinterpret_cast<str_er_track_decode *>(base + t.o_out);
        t.chars = base + o_chars; t.member_cost = reinterpret_cast<int32_t *>(base + o_mcost);
    }
    return t;
}

int track_decode_enqueue(str_er_ctx *c, hipStream_t s, size_t at, const uint8_t *d_rows, const int32_t *d_first, const int32_t *d_n_of, const void *d_dec,
                         const uint8_t *d_dchars, const int32_t *track_first, const int32_t *track_count, const int32_t *members, size_t n_members, size_t n_tracks,
                         TdTab &H, TdTab &D)
{
    if (n_tracks > 0x7FFFFFFFull / 32) return fail(c, STR_ER_ECAPACITY, "track decode: too many tracks");
    if (const int rc = c->td_tab.ensure(c, td_layout(nullptr, at, n_tracks, n_members).bytes, "track decode tables"); rc != STR_ER_OK) return rc;
    H = td_layout(c->td_tab.h(), at, n_tracks, n_members);
    D = td_layout(c->td_tab.d(), at, n_tracks, n_members);
    std::memcpy(H.first, track_first, 4 * n_tracks);
    std::memcpy(H.count, track_count, 4 * n_tracks);
    if (n_members > 0) std::memcpy(H.members, members, 4 * n_members);
    HIP_TRY(c, hipMemcpyAsync(c->td_tab.d() + H.o_up, c->td_tab.h() + H.o_up, H.up_bytes, hipMemcpyHostToDevice, s));
    if (n_members > 0) HIP_TRY(c, hipMemsetAsync(D.member_cost, 0xFF, 4 * n_members, s));          // (-1 in a slot of no track)
    launch_track_decode(s, c->bigram.d(), c->td_ins, c->td_del, c->td_rounds, d_rows, d_first, d_n_of, d_dec, d_dchars, D.first, D.count, D.members, (int)n_tracks,
                        D.out, D.chars, D.member_cost);
    HIP_TRY(c, hipGetLastError());
    return STR_ER_OK;
}

} // namespace str_er_host

namespace {

bool args_ok(const uint8_t *costs, int32_t n_rows, const int32_t *first_run, const int32_t *n_of, int32_t n_words, const int32_t *track_first,
             const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks, const str_er_track_decode *out, const uint8_t *chars,
             const int32_t *member_cost)
{
    return n_rows >= 0 && n_words >= 0 && n_members >= 0 && n_tracks >= 0 && (n_rows == 0 || costs) && (n_words == 0 || (first_run && n_of)) &&
           (n_tracks == 0 || (track_first && track_count && out && chars)) && (n_members == 0 || (members && member_cost));
}

} // namespace

extern "C" {

int str_er_set_track_decode(str_er_ctx *c, int32_t ins, int32_t del, int32_t rounds)
try {
    if (!c) return STR_ER_EINVAL;
    if (!td::params_ok(ins, del, rounds)) return fail(c, STR_ER_EINVAL, "track decode: INS and DEL are in 1 .. 255, rounds in 0 .. 64");
    c->td_ins = ins; c->td_del = del; c->td_rounds = rounds;
    ++c->decode_pool_gen;          // (a decode pool is bound to them: str_er_pool_decode)
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_decode_tracks(str_er_ctx *c, const uint8_t *costs, int32_t n_rows, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words,
                         const int32_t *track_first, const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks,
                         str_er_track_decode *out, uint8_t *chars, int32_t *member_cost)
try {
    if (!c) return STR_ER_EINVAL;
    if (!args_ok(costs, n_rows, first_run, n_runs_of_word, n_words, track_first, track_count, members, n_members, n_tracks, out, chars, member_cost))
        return fail(c, STR_ER_EINVAL, "bad arguments");
    if (!c->bigram_set) return fail(c, STR_ER_ESTATE, "str_er_decode_tracks needs a bigram table (str_er_set_bigram)");
    if (!words_in_rows(n_rows, first_run, n_runs_of_word, n_words)) return fail(c, STR_ER_EINVAL, "track decode: a word outside the cost rows");
    if (const int rc = td::tracks_check(track_first, track_count, members, n_members, n_tracks, n_words); rc != STR_ER_OK)
        return fail(c, rc, rc == STR_ER_ECAPACITY ? "track decode: a track of more than 1024 members"
                                                  : "track decode: a member outside the words, or tracks that do not ascend in the member array");
    for (int32_t i = 0; i < n_members; ++i) member_cost[i] = -1;
    if (n_tracks == 0) return STR_ER_OK;
    // the rows and the words' (first, n) at the front of the buffer, the decoder's tables behind them, the tracks' behind those
    const size_t at_dec = rows_in_layout(nullptr, 0, (size_t)n_rows, (size_t)n_words, false).bytes, at_tracks = wd_layout(nullptr, at_dec, (size_t)n_words).bytes;
    if (const int rc = c->td_tab.ensure(c, td_layout(nullptr, at_tracks, (size_t)n_tracks, (size_t)n_members).bytes, "track decode tables"); rc != STR_ER_OK) return rc;
    const WdTab W = wd_layout(c->td_tab.d(), at_dec, (size_t)n_words);
    hipStream_t s = c->stream;
    RowsIn      I{};
    if (const int rc = rows_in_upload(c, s, c->td_tab, nullptr, costs, (size_t)n_rows, nullptr, 0, first_run, n_runs_of_word, nullptr, (size_t)n_words, I); rc != STR_ER_OK) return rc;
    launch_word_decode(s, c->bigram.d(), c->wd_ins, c->wd_del, I.costs, I.first, I.n_of, n_words, W.dec, W.chars, W.src);
    HIP_TRY(c, hipGetLastError());
    TdTab H{}, D{};
    if (const int rc = track_decode_enqueue(c, s, at_tracks, I.costs, I.first, I.n_of, W.dec, W.chars, track_first, track_count, members, (size_t)n_members,
                                            (size_t)n_tracks, H, D);
        rc != STR_ER_OK)
        return rc;
    HIP_TRY(c, hipMemcpyAsync(c->td_tab.h() + H.o_out, c->td_tab.d() + H.o_out, H.down_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    std::memcpy(out, H.out, sizeof(str_er_track_decode) * (size_t)n_tracks);
    std::memcpy(chars, H.chars, td::MAX_LEN * (size_t)n_tracks);
    if (n_members > 0) std::memcpy(member_cost, H.member_cost, 4 * (size_t)n_members);
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_decode_tracks_host(const uint8_t *costs, int32_t n_rows, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words,
                              const int32_t *track_first, const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks,
                              const uint8_t *bigram, int32_t dec_ins, int32_t dec_del, int32_t ins, int32_t del, int32_t rounds,
                              str_er_track_decode *out, uint8_t *chars, int32_t *member_cost)
try {
    if (!args_ok(costs, n_rows, first_run, n_runs_of_word, n_words, track_first, track_count, members, n_members, n_tracks, out, chars, member_cost) || !bigram)
        return STR_ER_EINVAL;
    if (!wd::params_ok(dec_ins, dec_del) || !td::params_ok(ins, del, rounds) || !str_er_host::words_in_rows(n_rows, first_run, n_runs_of_word, n_words))
        return STR_ER_EINVAL;
    if (const int rc = td::tracks_check(track_first, track_count, members, n_members, n_tracks, n_words); rc != STR_ER_OK) return rc;
    for (int32_t i = 0; i < n_members; ++i) member_cost[i] = -1;
    if (n_tracks == 0) return STR_ER_OK;
    // the seeds' strings: the decoder on every word, as the device entry point makes them
    std::vector<str_er_word_decode> dec((size_t)n_words);
    std::vector<uint8_t>            dchars((size_t)n_words * wd::MAX_CHARS), dsrc(wd::MAX_CHARS);
    for (int32_t w = 0; w < n_words; ++w)
        dec[(size_t)w] = wd::decode_word(costs + (size_t)first_run[w] * wd::ALPHABET, n_runs_of_word[w], bigram, dec_ins, dec_del,
                                         dchars.data() + (size_t)w * wd::MAX_CHARS, dsrc.data());
    for (int32_t g = 0; g < n_tracks; ++g)
        out[g] = td::decode_track(costs, first_run, n_runs_of_word, members + track_first[g], track_count[g], dec.data(), dchars.data(), bigram, ins, del, rounds,
                                  chars + (size_t)g * td::MAX_LEN, member_cost + track_first[g]);
    return STR_ER_OK;
} catch (...) { return STR_ER_ENOMEM; }

const str_er_track_decode *str_er_result_track_decodes(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_track_decodes, &str_er_result::track_decodes, n);
}
const uint8_t *str_er_result_track_decode_chars(const str_er_result *r, uint64_t *n_bytes)
{
    return result_table(r, r && r->have_track_decodes, &str_er_result::track_decode_chars, n_bytes);
}
const int32_t *str_er_result_track_decode_member_costs(const str_er_result *r, int32_t *n)
{
    return result_table(r, r && r->have_track_decodes, &str_er_result::track_decode_member_costs, n);
}

} // extern "C"
