// api_track_pool.cpp -- the C ABI, part 8k: the track pool (str_er_track_pool_*; the contract is at str_er_pool_match in str_er.h).  The
// rules are track_pool_rules.h: the checks of an addition's slots, of a join and of the member limit run from there on the host's mirror
// of the slots' member counts, before anything is launched; the device side is track_pool_kernels.h on the matcher's lexicon.  The pool
// owns its device memory in two on-demand buffers: the accumulator rows with the slots' state, and the tables of one call.
//   A decode pool (str_er_track_pool_create_decode; the contract is at str_er_pool_decode) is the same object of another kind: the
// rules are decode_pool_rules.h, the device side decode_pool_kernels.h in front of k_word_decode (an addition) and k_track_decode (a
// read).  Its first buffer is the store of the kept members; the checks of the slots and of the member limit are the same.
//   A lattice decode pool (str_er_track_pool_create_lattice_decode; the contract is at "The lattice decode pool" in str_er.h) is the
// third kind: the rules are lattice_decode_pool_rules.h, the device side lattice_decode_pool_kernels.h behind k_lattice_decode (an
// addition) and in front of k_lattice_track_decode (a read).  Its store keeps per cell what launch_lattice_track_decode_tab takes.
#include "str_er_ctx.h"
#include "decode_pool_kernels.h"
#include "decode_pool_rules.h"
#include "lattice_decode_kernels.h"
#include "lattice_decode_pool_kernels.h"
#include "lattice_decode_pool_rules.h"
#include "lattice_track_decode_kernels.h"
#include "track_decode_kernels.h"
#include "track_pool_kernels.h"
#include "track_pool_rules.h"
#include "word_decode_kernels.h"

namespace dp = str_er_dp;
namespace ldp = str_er_ldp;
namespace lm = str_er_lm;
namespace rs = str_er_rs;
namespace tp = str_er_tp;
namespace tr = str_er_tr;

static_assert(sizeof(str_er_pool_decode) == 40 && sizeof(str_er_word_decode) == 24 && dp::CELL_ROW_BYTES == DP_CELL_ROW_BYTES, "decode pool layout");
static_assert(ldp::MAX_CELLS == LDP_MAX_CELLS && ldp::CELL_RUN_BYTES == LDP_CELL_RUN_BYTES && ldp::CELL_PIECE_BYTES == LDP_CELL_PIECE_BYTES && ldp::TAB_BYTES == 4 * LT_TAB_INTS &&
                  sizeof(str_er_lattice_decode) == 32 && sizeof(str_er_lattice_track_member) == 24 && sizeof(str_er_split_part) == 8,
              "lattice decode pool layout");
static_assert(sizeof(str_er_pool_match) == 32 && sizeof(tp::SlotState) == 4 * TP_STATE_INTS, "track pool layout");

struct str_er_track_pool {
    str_er_ctx *c = nullptr;
    int32_t     cap = 0;
    uint32_t    flags = 0;
    uint64_t    gen = 0;            // c->pool_gen (a decode pool: c->decode_pool_gen) when the pool was bound
    WmLexDev    lex{};              // what it is bound to: the lexicon on the device, INS / DEL / band, SPLIT
    WmParams    prm{};
    int32_t     split = 0, lex_n = 0;
    DevBuf      rows;               // cap accumulator rows | cap states
    PairBuf     tab;                // of one call: (the rows and words of an addition | its tracks, slots and members | the words' structure) or (slots | chunk keys | records)
    TpPoolDev   dev{};
    // a decode pool (flags & STR_ER_POOL_DECODE): `rows` is the store of the kept members
    int32_t     keep = 0;
    uint32_t    serial = 0;         // of the last addition
    DpPoolDev   store{};
    LdpPoolDev  lstore{};           // a lattice decode pool (STR_ER_POOL_DECODE | STR_ER_POOL_LATTICE): `rows` is this store, and `split` the SPLIT it is bound to
    const uint8_t *bigram = nullptr;        // what it is bound to: the table on the device, the decoder's INS / DEL, the track decode's INS / DEL / rounds
    int32_t     wd_ins = 0, wd_del = 0, td_ins = 0, td_del = 0, td_rounds = 0;
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

bool is_decode(const str_er_track_pool *P) { return (P->flags & STR_ER_POOL_DECODE) != 0; }
bool is_lattice_decode(const str_er_track_pool *P) { return is_decode(P) && (P->flags & STR_ER_POOL_LATTICE) != 0; }

// the store of a decode pool: rows | keys | first rows | run counts | decoder records | labels of the cells, then the slots' counts
DpPoolDev store_layout(uint8_t *base, int32_t cap, int32_t keep, size_t *bytes)
{
    const size_t n = (size_t)cap * (size_t)keep;
    Carve        cv{};
    const size_t o_rows = cv.take(n * DP_CELL_ROW_BYTES), o_key = cv.take(8 * n), o_first = cv.take(4 * n), o_n = cv.take(4 * n),
                 o_dec = cv.take(sizeof(str_er_word_decode) * n), o_chars = cv.take(64 * n), o_mem = cv.take(4 * (size_t)cap);
    if (bytes) *bytes = cv.off;
    DpPoolDev D{};
    D.cap = cap; D.keep = keep;
    if (base) {
        const auto i32 = [&](size_t o) { return reinterpret_cast<int32_t *>(base + o); };
        D.costs = base + o_rows; D.key = reinterpret_cast<uint64_t *>(base + o_key); D.first_run = i32(o_first); D.n_of = i32(o_n); D.dec = i32(o_dec);
        D.dchars = base + o_chars; D.n_members = i32(o_mem);
    }
    return D;
}

// the store of a lattice decode pool: run rows | piece rows | split records | structure rows | keys | first runs | run counts | decoder
// records | labels of the cells, then the slots' counts.  Every block of a cell is a multiple of 16 bytes and every array starts at a
// multiple of 256: cells start on 16-byte boundaries.
LdpPoolDev lattice_store_layout(uint8_t *base, int32_t cap, int32_t keep, size_t *bytes)
{
    const size_t n = (size_t)cap * (size_t)keep;
    Carve        cv{};
    const size_t o_runs = cv.take(n * LDP_CELL_RUN_BYTES), o_pieces = cv.take(n * LDP_CELL_PIECE_BYTES), o_splits = cv.take(n * ldp::CELL_SPLIT_BYTES),
                 o_tab = cv.take(n * ldp::TAB_BYTES), o_key = cv.take(8 * n), o_first = cv.take(4 * n), o_n = cv.take(4 * n),
                 o_dec = cv.take(sizeof(str_er_lattice_decode) * n), o_chars = cv.take(64 * n), o_mem = cv.take(4 * (size_t)cap);
    if (bytes) *bytes = cv.off;
    LdpPoolDev D{};
    D.cap = cap; D.keep = keep;
    if (base) {
        const auto i32 = [&](size_t o) { return reinterpret_cast<int32_t *>(base + o); };
        D.run_rows = base + o_runs; D.piece_rows = base + o_pieces; D.splits = reinterpret_cast<str_er_run_split *>(base + o_splits); D.tab = i32(o_tab);
        D.key = reinterpret_cast<uint64_t *>(base + o_key); D.first_run = i32(o_first); D.n_of = i32(o_n); D.dec = i32(o_dec); D.dchars = base + o_chars;
        D.n_members = i32(o_mem);
    }
    return D;
}

// the decode pool bound to the context as it is now, every slot empty
int bind_decode(str_er_track_pool *P)
{
    str_er_ctx *c = P->c;
    if (!c->bigram_set) return fail(c, STR_ER_ESTATE, "a decode pool needs a bigram table (str_er_set_bigram)");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (is_lattice_decode(P)) {
        size_t bytes = 0;
        lattice_store_layout(nullptr, P->cap, P->keep, &bytes);
        if (const int rc = P->rows.ensure(c, bytes, "lattice decode pool store"); rc != STR_ER_OK) { P->lstore = LdpPoolDev{}; return rc; }
        const LdpPoolDev D = lattice_store_layout(P->rows.d(), P->cap, P->keep, nullptr);
        HIP_TRY(c, hipMemsetAsync(P->rows.d(), 0, bytes, c->stream));
        launch_ldpool_reset(c->stream, D);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, wait_stream(c, c->stream));
        P->lstore = D; P->bigram = c->bigram.d(); P->wd_ins = c->wd_ins; P->wd_del = c->wd_del; P->td_ins = c->td_ins; P->td_del = c->td_del; P->td_rounds = c->td_rounds;
        P->split = c->rs_split; P->gen = c->decode_pool_gen; P->serial = 0;
        std::fill(P->n_members.begin(), P->n_members.end(), 0);
        return STR_ER_OK;
    }
    size_t bytes = 0;
    store_layout(nullptr, P->cap, P->keep, &bytes);
    if (const int rc = P->rows.ensure(c, bytes, "decode pool store"); rc != STR_ER_OK) { P->store = DpPoolDev{}; return rc; }
    const DpPoolDev D = store_layout(P->rows.d(), P->cap, P->keep, nullptr);
    HIP_TRY(c, hipMemsetAsync(P->rows.d(), 0, bytes, c->stream));          // (the rows too: what str_er_track_pool_members hands out is the same bytes every run)
    launch_dpool_reset(c->stream, D);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, wait_stream(c, c->stream));
    P->store = D; P->bigram = c->bigram.d(); P->wd_ins = c->wd_ins; P->wd_del = c->wd_del; P->td_ins = c->td_ins; P->td_del = c->td_del; P->td_rounds = c->td_rounds;
    P->gen = c->decode_pool_gen; P->serial = 0;
    std::fill(P->n_members.begin(), P->n_members.end(), 0);
    return STR_ER_OK;
}

// (a lattice decode pool is also bound to SPLIT, by value: the context keeps no generation for it, and num / den of the run split do not enter)
bool stale(const str_er_track_pool *P)
{
    if (is_lattice_decode(P)) return P->gen != P->c->decode_pool_gen || !P->lstore.run_rows || P->split != P->c->rs_split;
    return is_decode(P) ? P->gen != P->c->decode_pool_gen || !P->store.costs : P->gen != P->c->pool_gen || !P->dev.acc;
}

int usable(str_er_track_pool *P, bool lattice_call)
{
    if (is_decode(P)) {
        if (stale(P))
            return fail(P->c, STR_ER_ESTATE,
                        is_lattice_decode(P) ? "lattice decode pool: the bigram table, the decode parameters or SPLIT changed since the pool was bound (str_er_track_pool_reset)"
                                             : "decode pool: the bigram table or the decode parameters changed since the pool was bound (str_er_track_pool_reset)");
        if (lattice_call != is_lattice_decode(P))
            return fail(P->c, STR_ER_ESTATE, lattice_call ? "str_er_track_pool_add_lattice on a decode pool of rows" : "str_er_track_pool_add on a lattice decode pool");
        return STR_ER_OK;
    }
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

// the checks the additions share, then the upload of the rows and tables; I and D receive the device side; `more`: bytes behind them
int add_common(str_er_track_pool *P, const str_er_run_split *splits, const uint8_t *run_costs, size_t n_runs, const uint8_t *piece_costs, size_t n_pieces,
               const int32_t *first_run, const int32_t *n_of, int32_t n_words, const int32_t *track_first, const int32_t *track_count, const int32_t *members,
               int32_t n_members, int32_t n_tracks, const int32_t *slots, RowsIn &I, AddTab &D, size_t more = 0, const int32_t *word_slot = nullptr)
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
    // (word_slot: the part slots of the words, for the lattice decoder in front of a lattice decode pool, which needs no structure table)
    const size_t n_tab = splits && !word_slot ? nw : 0;
    const size_t at = rows_in_layout(nullptr, splits ? n_runs : 0, n_runs + n_pieces, nw, word_slot != nullptr).bytes;
    if (const int rc = P->tab.ensure(c, add_layout(nullptr, at, nt, nm, n_tab).bytes + more, "track pool tables"); rc != STR_ER_OK) return rc;
    hipStream_t s = c->stream;
    if (const int rc = rows_in_upload(c, s, P->tab, splits, run_costs, n_runs, piece_costs, n_pieces, first_run, n_of, word_slot, nw, I); rc != STR_ER_OK) return rc;
    const AddTab H = add_layout(P->tab.h(), at, nt, nm, n_tab);
    D = add_layout(P->tab.d(), at, nt, nm, n_tab);
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

// A read of a lattice decode pool: the plan on the store's keys, the track tables and the structure rows of the cells named, the track
// decode over lattices on the store, the records.  Every pointer behind member_cost may be null; n_parts is null for _read_decode.
int read_lattice(str_er_track_pool *P, const int32_t *slots, int32_t n, str_er_pool_decode *out, uint8_t *chars, int32_t *member_cost,
                 str_er_lattice_track_member *members_out, uint8_t *src, str_er_split_part *parts, int32_t cap_parts, int32_t *n_parts)
{
    str_er_ctx *c = P->c;
    for (int32_t i = 0; i < n; ++i)
        if (slots[i] < 0 || slots[i] >= P->cap) return fail(c, STR_ER_EINVAL, "lattice decode pool: a slot outside the pool");
    if (n == 0) return STR_ER_OK;
    const size_t ns = (size_t)n, nk = ns * (size_t)P->keep, np = nk * (size_t)lm::MAX_NODES;
    if (nk > (1ull << 25)) return fail(c, STR_ER_ECAPACITY, "lattice decode pool: too many slots to read at once for this keep");
    // slots | whether a request is the first that names its slot | first member, member count per request | cells in age order | age rank
    // per cell | track and part slot per member slot | the track decode's records, and what comes down: records | labels | member costs |
    // member records | sources | parts
    Carve        cv{};
    const size_t o_slots = cv.take(4 * ns), o_lead = cv.take(4 * ns), o_first = cv.take(4 * ns), o_count = cv.take(4 * ns), o_mem = cv.take(4 * nk), o_rank = cv.take(4 * nk),
                 o_st = cv.take(4 * nk), o_ps = cv.take(4 * nk), o_rec = cv.take(sizeof(str_er_track_decode) * ns), o_out = cv.take(sizeof(str_er_pool_decode) * ns),
                 o_chars = cv.take(32 * ns), o_mcost = cv.take(4 * nk), o_mrec = cv.take(sizeof(str_er_lattice_track_member) * nk), o_src = cv.take(lm::SRC_BYTES * nk),
                 o_parts = cv.take(sizeof(str_er_split_part) * np);
    if (const int rc = slots_upload(P, slots, ns, cv.off - align_up(4 * ns, 256)); rc != STR_ER_OK) return rc;
    (void)o_slots;
    uint8_t          *d = P->tab.d(), *h = P->tab.h();
    const auto        i32 = [&](size_t o) { return reinterpret_cast<int32_t *>(d + o); };
    hipStream_t       s = c->stream;
    const LdpPoolDev &S = P->lstore;
    {          // a slot named more than once: the structure rows of its cells are made by the first request alone (one writer a row)
        int32_t *lead = reinterpret_cast<int32_t *>(h + o_lead);
        for (int32_t i = 0; i < n; ++i) { lead[i] = P->seen[(size_t)slots[i]] ? 0 : 1; P->seen[(size_t)slots[i]] = 1; }
        for (int32_t i = 0; i < n; ++i) P->seen[(size_t)slots[i]] = 0;
        HIP_TRY(c, hipMemcpyAsync(d + o_lead, h + o_lead, 4 * ns, hipMemcpyHostToDevice, s));
    }
    launch_dpool_plan(s, ldpool_keys(S), i32(0), n, i32(o_first), i32(o_count), i32(o_mem), i32(o_rank), i32(o_mcost));
    launch_ldpool_tracks(s, S, P->td_del, P->split, n, i32(o_lead), i32(o_count), i32(o_mem), i32(o_st), i32(o_ps));
    launch_lattice_track_decode_tab(s, P->bigram, P->td_ins, P->td_del, P->td_rounds, P->split, S.splits, S.run_rows, S.piece_rows, S.first_run, S.n_of, S.dec, S.dchars,
                                    i32(o_first), i32(o_count), i32(o_mem), i32(o_st), i32(o_ps), (int)nk, n, S.tab, d + o_rec, d + o_chars, i32(o_mrec), d + o_src,
                                    i32(o_parts));
    launch_ldpool_records(s, S, i32(0), n, i32(o_rec), i32(o_count), i32(o_mem), i32(o_rank), i32(o_ps), i32(o_out), i32(o_mrec), i32(o_parts), i32(o_mcost));
    HIP_TRY(c, hipGetLastError());
    const bool want_members = n_parts != nullptr;
    HIP_TRY(c, hipMemcpyAsync(h + o_out, d + o_out, (want_members ? cv.off : o_mrec) - o_out, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    if (want_members) {          // the parts back to back in slot order; nothing is written before they are known to fit
        const str_er_lattice_track_member *hm = reinterpret_cast<const str_er_lattice_track_member *>(h + o_mrec);
        const str_er_split_part           *hp = reinterpret_cast<const str_er_split_part *>(h + o_parts);
        uint64_t total = 0;
        for (size_t i = 0; i < nk; ++i) {
            if (hm[i].n_parts < 0 || hm[i].n_parts > lm::MAX_NODES) return fail(c, STR_ER_EHIP, "lattice decode pool: a member's parts outside its slots (internal error)");
            total += (uint64_t)hm[i].n_parts;
        }
        *n_parts = (int32_t)total;
        if (total > (uint64_t)cap_parts) return fail(c, STR_ER_ECAPACITY, std::to_string(total) + " parts, cap_parts is " + std::to_string(cap_parts));
        size_t at = 0;
        for (size_t i = 0; i < nk; ++i) {
            const size_t k = (size_t)hm[i].n_parts;
            if (members_out) { members_out[i] = hm[i]; members_out[i].first_part = (int32_t)at; }
            if (parts && k > 0) std::memcpy(parts + at, hp + i * (size_t)lm::MAX_NODES, sizeof(str_er_split_part) * k);
            at += k;
        }
        if (src) std::memcpy(src, h + o_src, lm::SRC_BYTES * nk);
    }
    std::memcpy(out, h + o_out, sizeof(str_er_pool_decode) * ns);
    std::memcpy(chars, h + o_chars, 32 * ns);
    std::memcpy(member_cost, h + o_mcost, 4 * nk);
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

int str_er_track_pool_create_decode(str_er_ctx *c, int32_t cap_tracks, int32_t keep, str_er_track_pool **pool)
try {
    if (!c) return STR_ER_EINVAL;
    if (!pool || !dp::create_ok(cap_tracks, keep)) return fail(c, STR_ER_EINVAL, "str_er_track_pool_create_decode: cap_tracks >= 1 and 1 <= keep <= 1024");
    *pool = nullptr;
    if (!dp::cells_fit(cap_tracks, keep)) return fail(c, STR_ER_ECAPACITY, "decode pool: more than 2^24 kept members");
    str_er_track_pool *P = new str_er_track_pool;
    P->c = c; P->cap = cap_tracks; P->flags = STR_ER_POOL_DECODE; P->keep = keep;
    int rc = STR_ER_OK;
    try {
        P->n_members.assign((size_t)cap_tracks, 0); P->seen.assign((size_t)cap_tracks, 0);
        rc = bind_decode(P);
    } catch (...) { delete P; throw; }
    if (rc != STR_ER_OK) { delete P; return rc; }
    *pool = P;
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_track_pool_create_lattice_decode(str_er_ctx *c, int32_t cap_tracks, int32_t keep, str_er_track_pool **pool)
try {
    if (!c) return STR_ER_EINVAL;
    if (!pool || !ldp::create_ok(cap_tracks, keep)) return fail(c, STR_ER_EINVAL, "str_er_track_pool_create_lattice_decode: cap_tracks >= 1 and 1 <= keep <= 1024");
    *pool = nullptr;
    if (!ldp::cells_fit(cap_tracks, keep)) return fail(c, STR_ER_ECAPACITY, "lattice decode pool: more than 13421772 kept members (80 piece rows each, below 2^30) or 2^40 bytes");
    str_er_track_pool *P = new str_er_track_pool;
    P->c = c; P->cap = cap_tracks; P->flags = STR_ER_POOL_DECODE | STR_ER_POOL_LATTICE; P->keep = keep;
    int rc = STR_ER_OK;
    try {
        P->n_members.assign((size_t)cap_tracks, 0); P->seen.assign((size_t)cap_tracks, 0);
        rc = bind_decode(P);
    } catch (...) { delete P; throw; }
    if (rc != STR_ER_OK) { delete P; return rc; }
    *pool = P;
    return STR_ER_OK;
} ABI_GUARD(c)

int str_er_track_pool_keep(const str_er_track_pool *P, int32_t *keep)
{
    if (!P || !keep) return STR_ER_EINVAL;
    *keep = P->keep;
    return STR_ER_OK;
}

void str_er_track_pool_destroy(str_er_track_pool *P)
{
    if (!P) return;
    (void)hipStreamSynchronize(P->c->stream);
    delete P;
}

int str_er_track_pool_reset(str_er_track_pool *P)
try {
    if (!P) return STR_ER_EINVAL;
    return is_decode(P) ? bind_decode(P) : bind(P);
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
    const bool decode = is_decode(P);
    if (decode && n_tracks > 0 && P->serial == UINT32_MAX) return fail(c, STR_ER_ECAPACITY, "decode pool: the serials of its additions are used up (str_er_track_pool_reset)");
    if (const int rc = add_common(P, nullptr, costs, (size_t)n_rows, nullptr, 0, first_run, n_runs_of_word, n_words, track_first, track_count, members, n_members, n_tracks,
                                  slots, I, D, decode ? wd_layout(nullptr, 0, (size_t)n_words).bytes : 0);
        rc != STR_ER_OK)
        return rc;
    if (n_tracks == 0) return STR_ER_OK;
    if (decode) {          // the seeds' strings once, when the members come; then the members into their slots
        const WdTab W = wd_layout(P->tab.d(), D.bytes, (size_t)n_words);
        launch_word_decode(c->stream, P->bigram, P->wd_ins, P->wd_del, I.costs, I.first, I.n_of, n_words, W.dec, W.chars, W.src);
        launch_dpool_keep(c->stream, P->store, P->serial + 1, I.costs, I.first, I.n_of, W.dec, W.chars, D.first, D.count, D.members, D.slots, n_tracks);
        if (const int rc = add_done(P, track_count, n_tracks, slots); rc != STR_ER_OK) return rc;
        ++P->serial;
        return STR_ER_OK;
    }
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
    if (is_lattice_decode(P)) {          // the seeds' strings once, when the members come (k_lattice_decode on the call's words); then the members into their slots
        if (n_tracks > 0 && P->serial == UINT32_MAX) return fail(c, STR_ER_ECAPACITY, "lattice decode pool: the serials of its additions are used up (str_er_track_pool_reset)");
        std::vector<int32_t> slot;
        uint64_t             n_slots = 0;
        if (!rs_word_slots(splits ? splits : &no_split, first_run, n_runs_of_word, (size_t)n_words, slot, &n_slots))
            return fail(c, STR_ER_ECAPACITY, "lattice decode pool: more than 2^31 parts to reserve");
        slot.push_back(0);          // (never null: it says that the slots go up)
        if ((size_t)n_words > 0x7FFFFFFFull / 64) return fail(c, STR_ER_ECAPACITY, "track pool: too many rows or words");
        if (const int rc = add_common(P, splits ? splits : &no_split, run_costs, (size_t)n_runs, piece_costs, (size_t)n_pieces, first_run, n_runs_of_word, n_words, track_first,
                                      track_count, members, n_members, n_tracks, slots, I, D, ld_layout(nullptr, 0, (size_t)n_words, (size_t)n_slots).bytes, slot.data());
            rc != STR_ER_OK)
            return rc;
        if (n_tracks == 0) return STR_ER_OK;
        const LdTab    W = ld_layout(P->tab.d(), D.bytes, (size_t)n_words, (size_t)n_slots);
        const uint8_t *pieces = I.costs + rs::ALPHABET * (size_t)n_runs;
        if (n_words > 0)
            launch_lattice_decode(c->stream, P->bigram, P->wd_ins, P->wd_del, P->split, I.splits, I.costs, pieces, I.first, I.n_of, I.slot, n_words,
                                  reinterpret_cast<int32_t *>(W.dec), W.chars, W.src, reinterpret_cast<int32_t *>(W.parts));
        launch_ldpool_keep(c->stream, P->lstore, P->serial + 1, I.splits, I.costs, pieces, I.first, I.n_of, W.dec, W.chars, D.first, D.count, D.members, D.slots, n_tracks);
        if (const int rc = add_done(P, track_count, n_tracks, slots); rc != STR_ER_OK) return rc;
        ++P->serial;
        return STR_ER_OK;
    }
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
    if (is_lattice_decode(P)) launch_ldpool_join(c->stream, P->lstore, dst, P->tab.d<int32_t>(), n_srcs);
    else if (is_decode(P)) launch_dpool_join(c->stream, P->store, dst, P->tab.d<int32_t>(), n_srcs);
    else launch_pool_join(c->stream, P->dev, dst, P->tab.d<int32_t>(), n_srcs);
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
    if (is_decode(P)) launch_dpool_clear(c->stream, is_lattice_decode(P) ? ldpool_keys(P->lstore) : P->store, P->tab.d<int32_t>(), n);
    else launch_pool_clear(c->stream, P->dev, P->tab.d<int32_t>(), n);
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
    if (is_decode(P)) return fail(c, STR_ER_ESTATE, "str_er_track_pool_read on a decode pool (str_er_track_pool_read_decode)");
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

int str_er_track_pool_read_decode(str_er_track_pool *P, const int32_t *slots, int32_t n, str_er_pool_decode *out, uint8_t *chars, int32_t *member_cost)
try {
    if (!P) return STR_ER_EINVAL;
    str_er_ctx *c = P->c;
    if (n < 0 || (n > 0 && (!slots || !out || !chars || !member_cost))) return fail(c, STR_ER_EINVAL, "bad arguments");
    if (stale(P)) return usable(P, is_lattice_decode(P));
    if (!is_decode(P)) return fail(c, STR_ER_ESTATE, "str_er_track_pool_read_decode on a lexicon pool (str_er_track_pool_read)");
    if (is_lattice_decode(P)) return read_lattice(P, slots, n, out, chars, member_cost, nullptr, nullptr, nullptr, 0, nullptr);
    for (int32_t i = 0; i < n; ++i)
        if (slots[i] < 0 || slots[i] >= P->cap) return fail(c, STR_ER_EINVAL, "decode pool: a slot outside the pool");
    if (n == 0) return STR_ER_OK;
    const size_t ns = (size_t)n, nk = ns * (size_t)P->keep;
    if (nk > 0x7FFFFFFFull / 4) return fail(c, STR_ER_ECAPACITY, "decode pool: too many slots to read at once for this keep");
    // slots | first member, member count per request | cells in age order | age rank per cell | the track decode's records, and what
    // comes down: records | labels | member costs
    Carve        cv{};
    const size_t o_slots = cv.take(4 * ns), o_first = cv.take(4 * ns), o_count = cv.take(4 * ns), o_mem = cv.take(4 * nk), o_rank = cv.take(4 * nk),
                 o_rec = cv.take(sizeof(str_er_track_decode) * ns), o_out = cv.take(sizeof(str_er_pool_decode) * ns), o_chars = cv.take(32 * ns), o_mcost = cv.take(4 * nk);
    if (const int rc = slots_upload(P, slots, ns, cv.off - align_up(4 * ns, 256)); rc != STR_ER_OK) return rc;
    (void)o_slots;
    uint8_t    *d = P->tab.d(), *h = P->tab.h();
    const auto  i32 = [&](size_t o) { return reinterpret_cast<int32_t *>(d + o); };
    hipStream_t s = c->stream;
    launch_dpool_plan(s, P->store, i32(0), n, i32(o_first), i32(o_count), i32(o_mem), i32(o_rank), i32(o_mcost));
    launch_track_decode(s, P->bigram, P->td_ins, P->td_del, P->td_rounds, P->store.costs, P->store.first_run, P->store.n_of, P->store.dec, P->store.dchars, i32(o_first),
                        i32(o_count), i32(o_mem), n, d + o_rec, d + o_chars, i32(o_mcost));
    launch_dpool_records(s, P->store, i32(0), n, i32(o_rec), i32(o_count), i32(o_rank), i32(o_out));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(h + o_out, d + o_out, cv.off - o_out, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    std::memcpy(out, h + o_out, sizeof(str_er_pool_decode) * ns);
    std::memcpy(chars, h + o_chars, 32 * ns);
    std::memcpy(member_cost, h + o_mcost, 4 * nk);
    return STR_ER_OK;
} ABI_GUARD(P ? P->c : nullptr)

int str_er_track_pool_members(str_er_track_pool *P, int32_t slot, uint64_t *keys, int32_t *n_runs, uint8_t *rows, int32_t *n_kept)
try {
    if (!P) return STR_ER_EINVAL;
    str_er_ctx *c = P->c;
    if (!n_kept) return fail(c, STR_ER_EINVAL, "bad arguments");
    if (stale(P)) return usable(P, is_lattice_decode(P));
    if (!is_decode(P)) return fail(c, STR_ER_ESTATE, "str_er_track_pool_members on a lexicon pool");
    if (is_lattice_decode(P)) return fail(c, STR_ER_ESTATE, "str_er_track_pool_members on a lattice decode pool (str_er_track_pool_lattice_members)");
    if (slot < 0 || slot >= P->cap) return fail(c, STR_ER_EINVAL, "decode pool: a slot outside the pool");
    const size_t k = (size_t)P->keep, c0 = (size_t)slot * k;
    Carve        cv{};
    const size_t o_key = cv.take(8 * k), o_n = cv.take(4 * k), o_rows = cv.take(DP_CELL_ROW_BYTES * k);
    if (const int rc = P->tab.ensure(c, cv.off, "track pool tables"); rc != STR_ER_OK) return rc;
    uint8_t    *h = P->tab.h();
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemcpyAsync(h + o_key, P->store.key + c0, 8 * k, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(h + o_n, P->store.n_of + c0, 4 * k, hipMemcpyDeviceToHost, s));
    if (rows) HIP_TRY(c, hipMemcpyAsync(h + o_rows, P->store.costs + c0 * DP_CELL_ROW_BYTES, DP_CELL_ROW_BYTES * k, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    const uint64_t *hk = reinterpret_cast<const uint64_t *>(h + o_key);
    const int32_t  *hn = reinterpret_cast<const int32_t *>(h + o_n);
    std::vector<int32_t> order;          // the kept cells in age order
    for (size_t q = 0; q < k; ++q)
        if (hk[q] != 0) order.push_back((int32_t)q);
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return hk[a] < hk[b]; });
    for (size_t i = 0; i < order.size(); ++i) {
        const size_t q = (size_t)order[i];
        if (keys) keys[i] = hk[q];
        if (n_runs) n_runs[i] = hn[q];
        if (rows) std::memcpy(rows + i * DP_CELL_ROW_BYTES, h + o_rows + q * DP_CELL_ROW_BYTES, DP_CELL_ROW_BYTES);
    }
    *n_kept = (int32_t)order.size();
    return STR_ER_OK;
} ABI_GUARD(P ? P->c : nullptr)

int str_er_track_pool_read_lattice_decode(str_er_track_pool *P, const int32_t *slots, int32_t n, str_er_pool_decode *out, uint8_t *chars, int32_t *member_cost,
                                          str_er_lattice_track_member *members_out, uint8_t *src, str_er_split_part *parts, int32_t cap_parts, int32_t *n_parts)
try {
    if (!P) return STR_ER_EINVAL;
    str_er_ctx *c = P->c;
    if (n < 0 || cap_parts < 0 || !n_parts || (n > 0 && (!slots || !out || !chars || !member_cost))) return fail(c, STR_ER_EINVAL, "bad arguments");
    *n_parts = 0;
    if (stale(P)) return usable(P, (P->flags & STR_ER_POOL_LATTICE) != 0);
    if (!is_lattice_decode(P)) return fail(c, STR_ER_ESTATE, "str_er_track_pool_read_lattice_decode on a pool that is no lattice decode pool");
    return read_lattice(P, slots, n, out, chars, member_cost, members_out, src, parts, parts ? cap_parts : INT32_MAX, n_parts);
} ABI_GUARD(P ? P->c : nullptr)

int str_er_track_pool_lattice_members(str_er_track_pool *P, int32_t slot, uint64_t *keys, int32_t *n_runs, str_er_run_split *splits, uint8_t *run_rows,
                                      uint8_t *piece_rows, int32_t *n_kept)
try {
    if (!P) return STR_ER_EINVAL;
    str_er_ctx *c = P->c;
    if (!n_kept) return fail(c, STR_ER_EINVAL, "bad arguments");
    if (stale(P)) return usable(P, (P->flags & STR_ER_POOL_LATTICE) != 0);
    if (!is_lattice_decode(P)) return fail(c, STR_ER_ESTATE, "str_er_track_pool_lattice_members on a pool that is no lattice decode pool");
    if (slot < 0 || slot >= P->cap) return fail(c, STR_ER_EINVAL, "lattice decode pool: a slot outside the pool");
    const size_t k = (size_t)P->keep, c0 = (size_t)slot * k;
    Carve        cv{};
    const size_t o_key = cv.take(8 * k), o_n = cv.take(4 * k), o_sp = cv.take(ldp::CELL_SPLIT_BYTES * k), o_runs = cv.take(LDP_CELL_RUN_BYTES * k),
                 o_pieces = cv.take(LDP_CELL_PIECE_BYTES * k);
    if (const int rc = P->tab.ensure(c, cv.off, "track pool tables"); rc != STR_ER_OK) return rc;
    uint8_t          *h = P->tab.h();
    hipStream_t       s = c->stream;
    const LdpPoolDev &S = P->lstore;
    HIP_TRY(c, hipMemcpyAsync(h + o_key, S.key + c0, 8 * k, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(h + o_n, S.n_of + c0, 4 * k, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(h + o_sp, S.splits + c0 * LDP_CELL_RUNS, ldp::CELL_SPLIT_BYTES * k, hipMemcpyDeviceToHost, s));
    if (run_rows) HIP_TRY(c, hipMemcpyAsync(h + o_runs, S.run_rows + c0 * LDP_CELL_RUN_BYTES, LDP_CELL_RUN_BYTES * k, hipMemcpyDeviceToHost, s));
    if (piece_rows) HIP_TRY(c, hipMemcpyAsync(h + o_pieces, S.piece_rows + c0 * LDP_CELL_PIECE_BYTES, LDP_CELL_PIECE_BYTES * k, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    const uint64_t         *hk = reinterpret_cast<const uint64_t *>(h + o_key);
    const int32_t          *hn = reinterpret_cast<const int32_t *>(h + o_n);
    const str_er_run_split *hs = reinterpret_cast<const str_er_run_split *>(h + o_sp);
    std::vector<int32_t> order;          // the kept cells in age order
    for (size_t q = 0; q < k; ++q)
        if (hk[q] != 0) order.push_back((int32_t)q);
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return hk[a] < hk[b]; });
    for (size_t i = 0; i < order.size(); ++i) {
        // a member's own bytes, what lies behind them zeroed: the same bytes whatever the cell held before
        const size_t  q = (size_t)order[i];
        const int32_t m = std::min(std::max(hn[q], 0), (int32_t)LDP_CELL_RUNS), cell_first = (int32_t)((c0 + q) * LDP_CELL_PIECES);
        int32_t       used = 0;
        for (int32_t t = 0; t < m; ++t) used = std::max(used, hs[q * LDP_CELL_RUNS + t].first_piece - cell_first + hs[q * LDP_CELL_RUNS + t].n_pieces);
        used = std::min(std::max(used, 0), (int32_t)LDP_CELL_PIECES);
        if (keys) keys[i] = hk[q];
        if (n_runs) n_runs[i] = hn[q];
        if (splits) {
            str_er_run_split *o = splits + i * LDP_CELL_RUNS;
            std::memset(o, 0, ldp::CELL_SPLIT_BYTES);
            for (int32_t t = 0; t < m; ++t) { o[t] = hs[q * LDP_CELL_RUNS + t]; o[t].first_piece -= cell_first; }
        }
        if (run_rows) {
            std::memset(run_rows + i * LDP_CELL_RUN_BYTES, 0, LDP_CELL_RUN_BYTES);
            std::memcpy(run_rows + i * LDP_CELL_RUN_BYTES, h + o_runs + q * LDP_CELL_RUN_BYTES, (size_t)m * 65);
        }
        if (piece_rows) {
            std::memset(piece_rows + i * LDP_CELL_PIECE_BYTES, 0, LDP_CELL_PIECE_BYTES);
            std::memcpy(piece_rows + i * LDP_CELL_PIECE_BYTES, h + o_pieces + q * LDP_CELL_PIECE_BYTES, (size_t)used * 65);
        }
    }
    *n_kept = (int32_t)order.size();
    return STR_ER_OK;
} ABI_GUARD(P ? P->c : nullptr)

} // extern "C"
