// api_track_pool.cpp -- the C ABI, part 8k: the track pool (str_er_track_pool_*; the contract is at str_er_pool_match in str_er.h).  The
// rules are track_pool_rules.h: the checks of an addition's slots, of a join and of the member limit run from there on the host's mirror
// of the slots' member counts, before anything is launched; the device side is track_pool_kernels.h on the matcher's lexicon.  The pool
// owns its device memory in two on-demand buffers: the accumulator rows with the slots' state, and the tables of one call.
#include "str_er_ctx.h"
#include "track_pool_kernels.h"
#include "track_pool_rules.h"

namespace rs = str_er_rs;
namespace tp = str_er_tp;
namespace tr = str_er_tr;

static_assert(sizeof(str_er_pool_match) == 32 && sizeof(tp::SlotState) == 4 * TP_STATE_INTS, "track pool layout");

struct str_er_track_pool {
    str_er_ctx *c = nullptr;
    int32_t     cap = 0;
    uint32_t    flags = 0;
    uint64_t    gen = 0;            // c->pool_gen when the pool was bound
    WmLexDev    lex{};              // what it is bound to: the lexicon on the device, INS / DEL / band, SPLIT
    WmParams    prm{};
    int32_t     split = 0, lex_n = 0;
    DevBuf      rows;               // cap accumulator rows | cap states
    PairBuf     tab;                // of one call: (the rows and words of an addition | its tracks, slots and members | the words' structure) or (slots | chunk keys | records)
    TpPoolDev   dev{};
    std::vector<int32_t> n_members; // the host's mirror of the slots' member counts
    std::vector<uint8_t> seen;      // scratch of the checks: cap zeroes
};

namespace {

constexpr uint64_t MAX_POOL_BYTES = 1ull << 40;

// the pool bound to the context as it is now, every slot empty
int bind(str_er_track_pool *P)
{
    str_er_ctx *c = P->c;
    if (c->lex_n <= 0) return fail(c, STR_ER_ESTATE, "a track pool needs a lexicon (str_er_set_lexicon)");
    const uint64_t row_ints = (uint64_t)c->lex.n_groups * WM_GROUP;
    if (row_ints * 4 * (uint64_t)P->cap > MAX_POOL_BYTES) return fail(c, STR_ER_ECAPACITY, "track pool: more than 2^40 bytes of accumulators");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    TpPoolDev D{nullptr, nullptr, (int32_t)row_ints};
    const size_t o_state = align_up(4 * (size_t)P->cap * (size_t)row_ints, 256), bytes = o_state + 4 * (size_t)TP_STATE_INTS * (size_t)P->cap;
    if (P->dev.row_ints != D.row_ints) P->rows = DevBuf();          // (the lexicon's size changed: the rows are laid out anew)
    if (const int rc = P->rows.ensure(c, bytes, "track pool accumulators"); rc != STR_ER_OK) { P->dev = TpPoolDev{}; return rc; }
    D.acc = P->rows.d<int32_t>(); D.state = reinterpret_cast<int32_t *>(P->rows.d() + o_state);
    HIP_TRY(c, hipMemsetAsync(P->rows.d(), 0, bytes, c->stream));
    HIP_TRY(c, wait_stream(c, c->stream));
    P->dev = D; P->lex = c->lex; P->prm = c->wm_prm; P->split = c->rs_split; P->lex_n = c->lex_n; P->gen = c->pool_gen;
    std::fill(P->n_members.begin(), P->n_members.end(), 0);
    return STR_ER_OK;
}

bool stale(const str_er_track_pool *P) { return P->gen != P->c->pool_gen || !P->dev.acc; }

int usable(str_er_track_pool *P, bool lattice_call)
{
    if (stale(P)) return fail(P->c, STR_ER_ESTATE, "track pool: the lexicon or the match parameters changed since the pool was bound (str_er_track_pool_reset)");
    if (lattice_call != ((P->flags & STR_ER_POOL_LATTICE) != 0))
        return fail(P->c, STR_ER_ESTATE, lattice_call ? "str_er_track_pool_add_lattice on a pool of rows" : "str_er_track_pool_add on a lattice pool");
    return STR_ER_OK;
}

// the tables of an addition behind the rows (from byte `at` on): first member, member count and slot per track | members | in lattice
// mode the structure of the words
struct AddTab {
    int32_t *first, *count, *slots, *members, *tab;
    size_t   o_up, up_bytes, bytes;
};
AddTab add_layout(uint8_t *base, size_t at, size_t n_tracks, size_t n_members, size_t n_tab_words)
{
    AddTab t{};
    Carve  cv{at};
    t.o_up = cv.take(4 * n_tracks);
    const size_t o_count = cv.take(4 * n_tracks), o_slots = cv.take(4 * n_tracks), o_mem = cv.take(4 * n_members);
    t.up_bytes = cv.off - t.o_up;
    const size_t o_tab = cv.take(4 * (size_t)LT_TAB_INTS * n_tab_words);
    t.bytes = cv.off;
    if (base) {
        const auto i32 = [&](size_t o) { return reinterpret_cast<int32_t *>(base + o); };
        t.first = i32(t.o_up); t.count = i32(o_count); t.slots = i32(o_slots); t.members = i32(o_mem); t.tab = i32(o_tab);
    }
    return t;
}

// the checks both additions share, then the upload of the rows and tables; I and D receive the device side
int add_common(str_er_track_pool *P, const str_er_run_split *splits, const uint8_t *run_costs, size_t n_runs, const uint8_t *piece_costs, size_t n_pieces,
               const int32_t *first_run, const int32_t *n_of, int32_t n_words, const int32_t *track_first, const int32_t *track_count, const int32_t *members,
               int32_t n_members, int32_t n_tracks, const int32_t *slots, RowsIn &I, AddTab &D)
{
    str_er_ctx *c = P->c;
    if (const int rc = tr::tracks_check(track_first, track_count, members, n_members, n_tracks, n_words); rc != STR_ER_OK)
        return fail(c, rc, rc == STR_ER_ECAPACITY ? "track pool: a track of more than 65536 members"
                                                  : "track pool: a member outside the words, or tracks that do not ascend in the member array");
    if (const int rc = tp::add_check(slots, track_count, n_tracks, P->n_members.data(), P->cap, P->seen); rc != STR_ER_OK)
        return fail(c, rc, rc == STR_ER_ECAPACITY ? "track pool: a slot would hold more than 65536 members" : "track pool: a slot outside the pool, or named twice in one call");
    if (n_tracks == 0) return STR_ER_OK;          // (checked, and nothing to add: the caller returns)
    const size_t nw = (size_t)n_words, nm = (size_t)n_members, nt = (size_t)n_tracks;
    if (n_runs + n_pieces > 0x7FFFFFFFull / 65 || nw > 0x7FFFFFFFull / (4 * (size_t)LT_TAB_INTS)) return fail(c, STR_ER_ECAPACITY, "track pool: too many rows or words");
    const size_t at = rows_in_layout(nullptr, splits ? n_runs : 0, n_runs + n_pieces, nw, false).bytes;
    if (const int rc = P->tab.ensure(c, add_layout(nullptr, at, nt, nm, splits ? nw : 0).bytes, "track pool tables"); rc != STR_ER_OK) return rc;
    hipStream_t s = c->stream;
    if (const int rc = rows_in_upload(c, s, P->tab, splits, run_costs, n_runs, piece_costs, n_pieces, first_run, n_of, nullptr, nw, I); rc != STR_ER_OK) return rc;
    const AddTab H = add_layout(P->tab.h(), at, nt, nm, splits ? nw : 0);
    D = add_layout(P->tab.d(), at, nt, nm, splits ? nw : 0);
    std::memcpy(H.first, track_first, 4 * nt); std::memcpy(H.count, track_count, 4 * nt); std::memcpy(H.slots, slots, 4 * nt);
    if (nm > 0) std::memcpy(H.members, members, 4 * nm);
    HIP_TRY(c, hipMemcpyAsync(P->tab.d() + H.o_up, P->tab.h() + H.o_up, H.up_bytes, hipMemcpyHostToDevice, s));
    return STR_ER_OK;
}

// behind the launches of an addition: the wait, then the host's mirror
int add_done(str_er_track_pool *P, const int32_t *track_count, int32_t n_tracks, const int32_t *slots)
{
    str_er_ctx *c = P->c;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, wait_stream(c, c->stream));
    for (int32_t g = 0; g < n_tracks; ++g) P->n_members[(size_t)slots[g]] += track_count[g];
    return STR_ER_OK;
}

// a list of slots up into the front of the call's tables; `more`: bytes behind it
int slots_upload(str_er_track_pool *P, const int32_t *slots, size_t n, size_t more)
{
    str_er_ctx *c = P->c;
    if (const int rc = P->tab.ensure(c, align_up(4 * n, 256) + more, "track pool tables"); rc != STR_ER_OK) return rc;
    std::memcpy(P->tab.h(), slots, 4 * n);
    HIP_TRY(c, hipMemcpyAsync(P->tab.d(), P->tab.h(), 4 * n, hipMemcpyHostToDevice, c->stream));
    return STR_ER_OK;
}

} // namespace

extern "C" {

int str_er_track_pool_create(str_er_ctx *c, int32_t cap_tracks, uint32_t flags, str_er_track_pool **pool)
try {
    if (!c) return STR_ER_EINVAL;
    if (!pool || cap_tracks < 1 || (flags & ~STR_ER_POOL_LATTICE)) return fail(c, STR_ER_EINVAL, "str_er_track_pool_create: bad arguments");
    *pool = nullptr;
    str_er_track_pool *P = new str_er_track_pool;
    P->c = c; P->cap = cap_tracks; P->flags = flags;
    int rc = STR_ER_OK;
    try {
        P->n_members.assign((size_t)cap_tracks, 0); P->seen.assign((size_t)cap_tracks, 0);
        rc = bind(P);
    } catch (...) { delete P; throw; }
    if (rc != STR_ER_OK) { delete P; return rc; }
    *pool = P;
    return STR_ER_OK;
} ABI_GUARD(c)

void str_er_track_pool_destroy(str_er_track_pool *P)
{
    if (!P) return;
    (void)hipStreamSynchronize(P->c->stream);
    delete P;
}

int str_er_track_pool_reset(str_er_track_pool *P)
try {
    if (!P) return STR_ER_EINVAL;
    return bind(P);
} ABI_GUARD(P ? P->c : nullptr)

int str_er_track_pool_info(const str_er_track_pool *P, int32_t *cap_tracks, uint32_t *flags, int32_t *n_entries, uint64_t *device_bytes, int32_t *n_in_use, int32_t *is_stale)
{
    if (!P) return STR_ER_EINVAL;
    if (cap_tracks) *cap_tracks = P->cap;
    if (flags) *flags = P->flags;
    if (n_entries) *n_entries = P->lex_n;
    if (device_bytes) *device_bytes = P->rows.size() + P->tab.size();
    if (n_in_use) *n_in_use = (int32_t)std::count_if(P->n_members.begin(), P->n_members.end(), [](int32_t v) { return v > 0; });
    if (is_stale) *is_stale = stale(P) ? 1 : 0;
    return STR_ER_OK;
}

int str_er_track_pool_add(str_er_track_pool *P, const uint8_t *costs, int32_t n_rows, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words,
                          const int32_t *track_first, const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks, const int32_t *slots)
try {
    if (!P) return STR_ER_EINVAL;
    str_er_ctx *c = P->c;
    if (!(n_rows >= 0 && n_words >= 0 && n_members >= 0 && n_tracks >= 0 && (n_rows == 0 || costs) && (n_words == 0 || (first_run && n_runs_of_word)) &&
          (n_tracks == 0 || (track_first && track_count && slots)) && (n_members == 0 || members)))
        return fail(c, STR_ER_EINVAL, "bad arguments");
    if (const int rc = usable(P, false); rc != STR_ER_OK) return rc;
    if (!words_in_rows(n_rows, first_run, n_runs_of_word, n_words)) return fail(c, STR_ER_EINVAL, "track pool: a word outside the cost rows");
    RowsIn I{};
    AddTab D{};
    if (const int rc = add_common(P, nullptr, costs, (size_t)n_rows, nullptr, 0, first_run, n_runs_of_word, n_words, track_first, track_count, members, n_members, n_tracks,
                                  slots, I, D);
        rc != STR_ER_OK)
        return rc;
    if (n_tracks == 0) return STR_ER_OK;
    launch_pool_add(c->stream, P->lex, P->prm, P->dev, I.costs, I.first, I.n_of, D.first, D.count, D.members, D.slots, n_tracks);
    return add_done(P, track_count, n_tracks, slots);
} ABI_GUARD(P ? P->c : nullptr)

int str_er_track_pool_add_lattice(str_er_track_pool *P, const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs,
                                  int32_t n_pieces, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, const int32_t *track_first,
                                  const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks, const int32_t *slots)
try {
    if (!P) return STR_ER_EINVAL;
    str_er_ctx *c = P->c;
    if (!(n_runs >= 0 && n_pieces >= 0 && n_words >= 0 && n_members >= 0 && n_tracks >= 0 && (n_runs == 0 || (splits && run_costs)) && (n_pieces == 0 || piece_costs) &&
          (n_words == 0 || (first_run && n_runs_of_word)) && (n_tracks == 0 || (track_first && track_count && slots)) && (n_members == 0 || members)))
        return fail(c, STR_ER_EINVAL, "bad arguments");
    if (const int rc = usable(P, true); rc != STR_ER_OK) return rc;
    if (!rs::splits_ok(splits, n_runs, n_pieces)) return fail(c, STR_ER_EINVAL, "track pool: a record with cuts or pieces that are none");
    if (!words_in_rows(n_runs, first_run, n_runs_of_word, n_words)) return fail(c, STR_ER_EINVAL, "track pool: a word outside the glyph runs");
    // (without runs there are no split records to go up: the words are then all empty, and the kernels read none)
    static const str_er_run_split no_split{};
    RowsIn I{};
    AddTab D{};
    if (const int rc = add_common(P, splits ? splits : &no_split, run_costs, (size_t)n_runs, piece_costs, (size_t)n_pieces, first_run, n_runs_of_word, n_words, track_first,
                                  track_count, members, n_members, n_tracks, slots, I, D);
        rc != STR_ER_OK)
        return rc;
    if (n_tracks == 0) return STR_ER_OK;
    launch_pool_add_lattice(c->stream, P->lex, P->prm, P->split, P->dev, I.splits, I.costs, I.costs + rs::ALPHABET * (size_t)n_runs, I.first, I.n_of, n_words, D.first, D.count,
                            D.members, D.slots, n_tracks, D.tab);
    return add_done(P, track_count, n_tracks, slots);
} ABI_GUARD(P ? P->c : nullptr)

int str_er_track_pool_join(str_er_track_pool *P, int32_t dst, const int32_t *srcs, int32_t n_srcs)
try {
    if (!P) return STR_ER_EINVAL;
    str_er_ctx *c = P->c;
    if (n_srcs < 0 || (n_srcs > 0 && !srcs)) return fail(c, STR_ER_EINVAL, "bad arguments");
    if (stale(P)) return usable(P, (P->flags & STR_ER_POOL_LATTICE) != 0);
    if (const int rc = tp::join_check(dst, srcs, n_srcs, P->n_members.data(), P->cap, P->seen); rc != STR_ER_OK)
        return fail(c, rc, rc == STR_ER_ECAPACITY ? "track pool: the joined slot would hold more than 65536 members"
                                                  : "track pool: a slot outside the pool, a repeated slot, or dst among the srcs");
    if (n_srcs == 0) return STR_ER_OK;
    if (const int rc = slots_upload(P, srcs, (size_t)n_srcs, 0); rc != STR_ER_OK) return rc;
    launch_pool_join(c->stream, P->dev, dst, P->tab.d<int32_t>(), n_srcs);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, wait_stream(c, c->stream));
    for (int32_t k = 0; k < n_srcs; ++k) { P->n_members[(size_t)dst] += P->n_members[(size_t)srcs[k]]; P->n_members[(size_t)srcs[k]] = 0; }
    return STR_ER_OK;
} ABI_GUARD(P ? P->c : nullptr)

int str_er_track_pool_clear(str_er_track_pool *P, const int32_t *slots, int32_t n)
try {
    if (!P) return STR_ER_EINVAL;
    str_er_ctx *c = P->c;
    if (n < 0 || (n > 0 && !slots)) return fail(c, STR_ER_EINVAL, "bad arguments");
    if (stale(P)) return usable(P, (P->flags & STR_ER_POOL_LATTICE) != 0);
    for (int32_t i = 0; i < n; ++i)
        if (slots[i] < 0 || slots[i] >= P->cap) return fail(c, STR_ER_EINVAL, "track pool: a slot outside the pool");
    if (n == 0) return STR_ER_OK;
    if (const int rc = slots_upload(P, slots, (size_t)n, 0); rc != STR_ER_OK) return rc;
    launch_pool_clear(c->stream, P->dev, P->tab.d<int32_t>(), n);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, wait_stream(c, c->stream));
    for (int32_t i = 0; i < n; ++i) P->n_members[(size_t)slots[i]] = 0;
    return STR_ER_OK;
} ABI_GUARD(P ? P->c : nullptr)

int str_er_track_pool_read(str_er_track_pool *P, const int32_t *slots, int32_t n, str_er_pool_match *out)
try {
    if (!P) return STR_ER_EINVAL;
    str_er_ctx *c = P->c;
    if (n < 0 || (n > 0 && (!slots || !out))) return fail(c, STR_ER_EINVAL, "bad arguments");
    if (stale(P)) return usable(P, (P->flags & STR_ER_POOL_LATTICE) != 0);
    for (int32_t i = 0; i < n; ++i)
        if (slots[i] < 0 || slots[i] >= P->cap) return fail(c, STR_ER_EINVAL, "track pool: a slot outside the pool");
    if (n == 0) return STR_ER_OK;
    const int n_chunks = tm_chunks(P->lex);
    if ((size_t)n > 0x7FFFFFFFull / (size_t)n_chunks / 2) return fail(c, STR_ER_ECAPACITY, "track pool: too many slots to read at once for this lexicon");
    const size_t o_part = align_up(4 * (size_t)n, 256), o_out = o_part + align_up(16 * (size_t)n * (size_t)n_chunks, 256), out_bytes = sizeof(str_er_pool_match) * (size_t)n;
    if (const int rc = slots_upload(P, slots, (size_t)n, o_out + out_bytes - o_part); rc != STR_ER_OK) return rc;
    hipStream_t s = c->stream;
    launch_pool_read(s, P->lex, P->dev, P->tab.d<int32_t>(), n, reinterpret_cast<uint64_t *>(P->tab.d() + o_part), reinterpret_cast<int32_t *>(P->tab.d() + o_out));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(P->tab.h() + o_out, P->tab.d() + o_out, out_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    std::memcpy(out, P->tab.h() + o_out, out_bytes);
    return STR_ER_OK;
} ABI_GUARD(P ? P->c : nullptr)

} // extern "C"
