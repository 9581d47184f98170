// api_run_read.cpp -- the C ABI, part 8c: the reading of the glyph runs of text lines (STR_ER_WANT_RUN_READ behind the line stage of
// api_frame_lines.cpp, str_er_feet_read on uploaded footprints; the contract is at str_er_run_read in str_er.h).  Only the host knows
// the compacted runs, so after the line stage's wait it lays their tiles out in an atlas (pack_run_tiles, words_host.cpp), k_run_tiles
// expands the footprint words still in c->foot_bits into it, and the scorer's launch chain reads the atlas as a device plane
// (run_read_stage: a second enqueue and wait).  With pieces (str_er_run_split, api_run_split.cpp) their tiles lie behind the runs' in
// the same atlas.  Behind the scorer, on the same stream and with the same wait, the consumers of a detect call; read_plan.h decides
// what the call makes for them, in c->read_rows, and what each reads:
//
//   rows   A: present iff match, folded iff the lexicon folds;  U: unfolded, needed iff decode || lattice || (split && !match), and
//          U IS A where match && !fold.  n_rows each: the runs', and with split the pieces' behind them
//   k_run_costs    A if match, then U if it is needed and is not A
//   k_split_words  on A iff match && split, then on U iff split && (decode || !match) and U is not A; the last one's records come down
//
//   consumer         reads
//   matcher          A's part rows with (slot, n_parts) if split, else A with (first, n_of)
//   track match      the same window as the matcher
//   decoder          U's part rows (A's where U is A) with (slot, n_parts) if split, else U with (first, n_of)
//   lattice decode   U's rows (runs first, pieces from row n_run on) with (first, n_of, slot) and the split records
//   lattice match    A's rows (runs first, pieces from row n_run on) with (first, n_of, slot) and the split records; iff match && split
//   lattice track    the same rows and records as the lattice match, with the track match's tracks; iff the lattice match and the track match run
//   track decode     the same window as the decoder, with the decoder's records and labels where it left them; iff decode
//   lattice track decode  what the lattice decode read, with its records and labels where it left them and the track decode's tracks; iff both run and the context's setting
//   lattice margins  what the lattice decode read, with its records, labels, sources and parts where it left them; iff the lattice decode and the context's setting
//   margins          the same window as the decoder, with the decoder's records, labels and sources where it left them; iff decode and the context's setting
//   line decode      the decoder's rows, every line one window from the first row of its first word to the last of its last, with the gap costs the host makes from the runs; iff decode
//                    and the context's setting.  With split the rows are the parts' rows of U (A's where U is A), which lie at the words' slots and whose number only the device
//                    knows: the line decode is then enqueued behind the stage's wait, once the parts are down, with the cost row of every part, and has a wait of its own
//   line lattice decode  what the lattice decode read (U's rows of the runs and pieces, the split records), every line one window of runs from the first run of its first word to
//                    the last of its last, with a gap pair per run the host makes from the runs and the node slots it makes from the split records; iff the lattice decode and
//                    the context's setting.  All of it is known before the scorer is enqueued: behind k_lattice_decode on the same stream, down with the stage's one wait
//
//   result table     source
//   run_costs        A if match, else U
//   piece_costs      A if match, else U
//   run_probs        present iff match or decode
//
// The words' (first, n_of, slot) and the split records go up once, behind the tiles in c->run_tab; wm_tab, wd_tab, wg_tab, rs_tab, ld_tab, lg_tab, lm_tab,
// lt_tab, tm_tab, td_tab, ltd_tab, ln_tab and ll_tab hold what their kernels leave.
#include "str_er_ctx.h"
#include "line_decode_rules.h"
#include "line_lattice_rules.h"
#include "lattice_decode_kernels.h"
#include "line_lattice_kernels.h"
#include "lattice_match_kernels.h"
#include "run_split_kernels.h"

namespace str_er_host {

void ReadChainOut::preset(const ReadPlan &p, size_t n_run, size_t n_pc, size_t k) const
{
    const size_t n_words = p.any() ? words->size() : 0;
    if (p.result_set != SET_NONE) run_costs->assign(65 * n_run, 0);
    if (p.run_probs) run_probs->assign(k * n_run, 0.0);
    if (p.match) matches->assign(n_words, str_er_word_match{-1, -1, -1, -1, 0, 0});
    if (p.track) { track_matches->assign(tracks->size(), str_er_track_match{-1, -1, -1, -1, 0, 0, 0, -1}); track_member_costs->assign(track_members->size(), -1); }
    if (p.decode) { decodes->assign(n_words, str_er_word_decode{}); decode_chars->assign(64 * n_words, 0xFF); decode_src->assign(64 * n_words, 0xFF); }
    if (p.margin) {
        margins->assign(n_words, str_er_word_margin{-1, -1, -1, -1}); row_margins->assign(32 * n_words, -1);
        row_reads->assign(32 * n_words, 0xFF); row_alts->assign(32 * n_words, 0xFF);
    }
    if (p.tdecode) {
        track_decodes->assign(tracks->size(), str_er_track_decode{-1, -1, 0, 0, 0, 0, -1, -1}); track_decode_chars->assign(32 * tracks->size(), 0xFF);
        track_decode_member_costs->assign(track_members->size(), -1);
    }
    if (p.ltdecode) {
        lattice_track_decodes->assign(tracks->size(), str_er_track_decode{-1, -1, 0, 0, 0, 0, -1, -1}); lattice_track_decode_chars->assign(32 * tracks->size(), 0xFF);
        lattice_track_decode_members->assign(track_members->size(), str_er_lattice_track_member{-1, 0, 0, 0, 0, -1});
        lattice_track_decode_src->assign(32 * track_members->size(), 0xFF); lattice_track_decode_parts->clear();
    }
    if (p.split) { piece_costs->assign(65 * n_pc, 0); parts->clear(); word_splits->assign(n_words, str_er_word_split{0, 0, 0, 0}); }
    if (p.ldecode) {          // (a line without rows is the empty line: B[E][E])
        const size_t lr = p.split ? 0 : n_run;          // (with split the rows are the parts: sized once they are known)
        line_decodes->assign(n_lines, str_er_line_decode{line_bee, 0, 0, 0, 0, 0}); line_chars->assign(3 * lr, 0xFF); line_src->assign(3 * lr, 0xFFFF);
        line_word_of_row->assign(lr, -1); line_gaps->assign(2 * lr, 0); line_windows->assign(2 * n_lines, 0);
    }
    if (p.lnmargin) {          // (a line without rows has no margin)
        const size_t lr = p.split ? 0 : n_run;
        line_margins->assign(n_lines, str_er_line_margin{-1, -1, -1, -1, -1, -1, -1, -1}); line_row_margins->assign(lr, -1); line_gap_margins->assign(lr, -1);
        line_row_reads->assign(lr, 0xFF); line_row_alts->assign(lr, 0xFF); line_gap_moves->assign(lr, 0xFF);
    }
    if (p.lldecode) {          // (a line without runs is the empty line: B[E][E]; labels, sources and gap costs are sized once the atoms are known)
        ll_decodes->assign(n_lines, str_er_line_lattice_decode{line_bee, 0, 0, 0, 0, 0, 0, 0}); ll_chars->clear(); ll_src->clear(); ll_parts->clear(); ll_word_of_part->clear();
        ll_gaps->assign(2 * n_run, 0); ll_windows->assign(2 * n_lines, 0);
    }
    if (p.lattice) {
        lattice_decodes->assign(n_words, str_er_lattice_decode{}); lattice_chars->assign(64 * n_words, 0xFF); lattice_src->assign(64 * n_words, 0xFF);
        lattice_parts->clear();
    }
    if (p.lmargin) {
        lattice_margins->assign(n_words, str_er_lattice_margin{-1, -1, -1, -1, -1, -1, -1, 0});
        lattice_read_margins->assign(32 * n_words, -1); lattice_cut_margins->assign(32 * n_words, -1);
        lattice_part_reads->assign(32 * n_words, 0xFF); lattice_part_alts->assign(32 * n_words, 0xFF); lattice_cut_alts->assign(32 * n_words, 0xFF);
    }
    if (p.lmatch) {
        lattice_matches->assign(n_words, str_er_lattice_match{-1, -1, -1, -1, 0, 0, 0, 0, 0, 0}); lattice_match_src->assign(32 * n_words, 0xFF);
        lattice_match_parts->clear();
    }
    if (p.ltrack) {
        lattice_track_matches->assign(tracks->size(), str_er_track_match{-1, -1, -1, -1, 0, 0, 0, -1});
        lattice_track_members->assign(track_members->size(), str_er_lattice_track_member{-1, 0, 0, 0, 0, -1}); lattice_track_src->assign(32 * track_members->size(), 0xFF);
        lattice_track_parts->clear();
    }
}

namespace {

// c->run_tab (base: either side of the pair, or null for the size alone): tiles | boxes | rotations of the n tiles | first run, run
// count and (n_slot_words) part slot of the words | the runs' split records
struct RunTab {
    RunTile *tiles; int32_t *boxes; RotGeom *rot; int32_t *first, *n_of, *slot; str_er_run_split *splits;
    size_t   bytes;
};
RunTab run_tab_layout(uint8_t *base, size_t n, size_t n_words, size_t n_slot_words, size_t n_splits)
{
    RunTab t{};
    Carve  cv;
    const size_t o_tile = cv.take(sizeof(RunTile) * n), o_box = cv.take(16 * n), o_rot = cv.take(sizeof(RotGeom) * n), o_first = cv.take(4 * n_words),
                 o_nof = cv.take(4 * n_words), o_slot = cv.take(4 * n_slot_words), o_sp = cv.take(sizeof(str_er_run_split) * n_splits);
    t.bytes = cv.off;
    if (base) {
        t.tiles = reinterpret_cast<RunTile *>(base + o_tile); t.boxes = reinterpret_cast<int32_t *>(base + o_box); t.rot = reinterpret_cast<RotGeom *>(base + o_rot);
        t.first = reinterpret_cast<int32_t *>(base + o_first); t.n_of = reinterpret_cast<int32_t *>(base + o_nof); t.slot = reinterpret_cast<int32_t *>(base + o_slot);
        t.splits = reinterpret_cast<str_er_run_split *>(base + o_sp);
    }
    return t;
}

// one call of the stage: its phases in their order
struct ReadCall {
    str_er_ctx *c; hipStream_t s;
    const ReadPlan      p;
    const ReadChainOut &o;
    const SvmDev       *m;                           // null: the features only
    const size_t        n_run, n_pc, n, n_rows, n_words;      // n tiles: the runs' and behind them the pieces'; n_rows cost rows a set
    // on the host: the geometry, the tracks and with split the part slot of every word
    std::vector<RunTile> tiles; std::vector<RotGeom> rot; std::vector<int32_t> boxes, slot, tfirst, tcount, pslot, qslot;
    RunAtlas             A{}; size_t atlas_bytes = 0;
    uint64_t             n_slots = 0, n_pslots = 0, n_qslots = 0;
    // the buffers (device, H: page-locked): the tables, the scorer's scratch, the row sets and their part rows in c->read_rows, what the consumers' kernels leave
    RunTab   TH{}, TD{};
    OcrBuf   buf{};
    uint8_t *rows[2] = {nullptr, nullptr}, *parts[2] = {nullptr, nullptr};
    LnTab    NH{}, ND{};
    LlTab    YH{}, YD{}; std::vector<int32_t> ll_first, ll_n_of, ll_slot, ll_slot_end; size_t ll_atoms = 0;      // (the line lattice decode: its windows and node slots)
    const std::vector<str_er_line_words> *lines_of = nullptr; const std::vector<str_er_line_run> *runs_of = nullptr;      // (geometry keeps them for the line decode)
    RsTab    SH{}, SD{}; LdTab LH{}, LD{}; LmTab MH{}, MD{}; LtTab GH{}, GD{}; WmTab WD{}; WdTab DD{}; WgTab GM{}; LgTab LG{}; TmTab KD{}; TdTab EH{}, ED{}; LtdTab QH{}, QD{};

    // phase 1 (host alone): the tiles and rotations of the runs and pieces, every box checked, and their places in the atlas
    int geometry(const std::vector<FootLine> &lines, const std::vector<str_er_line_words> &line_words, const std::vector<str_er_line_run> &runs, const double *slopes,
                 const RunPieces *pieces)
    {
        if (n > 0x7FFFFFFFull / 1800) return fail(c, STR_ER_ECAPACITY, "run read: too many glyph runs");
        lines_of = &line_words; runs_of = &runs;
        tiles.resize(n); rot.resize(n);
        std::vector<int32_t> line_of(n_pc ? n_run : 0);
        const auto           tile = [&](size_t i, const FootLine &L, int32_t x0, int32_t x1, int32_t y0, int32_t y1, double slope) {
            RunTile &T = tiles[i];
            T.bit_off = L.word_off + (uint64_t)(y0 - L.y) * L.pitch; T.pitch = L.pitch; T.c0 = (uint32_t)(x0 - L.x);
            T.w = (uint32_t)(x1 - x0); T.h = (uint32_t)(y1 - y0);
            rot[i] = make_rot_geom((int)T.w, (int)T.h, slope);
        };
        const auto slope_of = [&](size_t t) { return slopes && std::isfinite(slopes[t]) ? slopes[t] : 0.0; };
        for (size_t t = 0; t < lines.size(); ++t) {
            const FootLine &L = lines[t];
            for (int32_t k = 0; k < line_words[t].n_runs; ++k) {
                const size_t           i = (size_t)line_words[t].first_run + (size_t)k;
                const str_er_line_run &Q = runs[i];
                // (the kernel reads the rows and columns of the run in its line's words: they must lie inside the foot box)
                if (i >= n_run || Q.x0 < L.x || Q.x1 <= Q.x0 || Q.x1 > L.x + L.w || Q.y0 < L.y || Q.y1 <= Q.y0 || Q.y1 > L.y + L.h)
                    return fail(c, STR_ER_EHIP, "run read: a glyph run outside its line's footprint (internal error)");
                tile(i, L, Q.x0, Q.x1, Q.y0, Q.y1, slope_of(t));
                if (n_pc) line_of[i] = (int32_t)t;
            }
        }
        for (size_t k = 0; k < n_pc; ++k) {          // a piece: a box inside its run's, in the same line's words, with the line's slope
            const str_er_run_piece &Q = (*pieces->pieces)[k];
            if (Q.run < 0 || (size_t)Q.run >= n_run) return fail(c, STR_ER_EHIP, "run split: a piece outside the glyph runs (internal error)");
            const str_er_line_run &U = runs[(size_t)Q.run];
            const size_t           t = (size_t)line_of[(size_t)Q.run];
            if (Q.x0 < U.x0 || Q.x1 <= Q.x0 || Q.x1 > U.x1 || Q.y0 < U.y0 || Q.y1 <= Q.y0 || Q.y1 > U.y1)
                return fail(c, STR_ER_EHIP, "run split: a piece outside its glyph run (internal error)");
            tile(n_run + k, lines[t], Q.x0, Q.x1, Q.y0, Q.y1, slope_of(t));
        }
        if (!pack_run_tiles(tiles.data(), n, RUN_SHELF_W, A)) return fail(c, STR_ER_ECAPACITY, "run read: the tiles of the glyph runs do not fit an atlas");
        boxes.resize(4 * n);
        for (size_t i = 0; i < n; ++i) {
            const RunTile &T = tiles[i];
            if ((uint64_t)T.ax + (T.w + 3u) / 4u * 4u > A.width || (uint64_t)T.ay + T.h > A.height)
                return fail(c, STR_ER_EHIP, "run read: a tile outside the atlas (internal error)");
            boxes[4 * i] = (int32_t)T.ax; boxes[4 * i + 1] = (int32_t)T.ay; boxes[4 * i + 2] = (int32_t)T.w; boxes[4 * i + 3] = (int32_t)T.h;
        }
        atlas_bytes = (size_t)A.width * A.height;
        return STR_ER_OK;
    }

    // phase 2: every buffer of the plan sized and carved; the words (straight into the page-locked table), split records and tracks checked
    int buffers()
    {
        int rc = STR_ER_OK;
        if (n_words > 0x7FFFFFFFull / 64) return fail(c, STR_ER_ECAPACITY, "run read: too many words");          // (n <= 2^31 / 1800: the rows' byte counts fit 31 bits)
        const size_t n_sw = p.split ? n_words : 0, n_sp = p.split ? n_run : 0;
        if ((rc = c->run_tab.ensure(c, run_tab_layout(nullptr, n, n_words, n_sw, n_sp).bytes, "run tile tables")) != STR_ER_OK) return rc;
        TH = run_tab_layout(c->run_tab.h(), n, n_words, n_sw, n_sp); TD = run_tab_layout(c->run_tab.d(), n, n_words, n_sw, n_sp);
        for (size_t w = 0; w < n_words; ++w) { TH.first[w] = (*o.words)[w].first_run; TH.n_of[w] = (*o.words)[w].n_runs; }
        if (!words_in_rows((int64_t)n_run, TH.first, TH.n_of, (int64_t)n_words)) return fail(c, STR_ER_EHIP, "run read: a word outside the glyph runs (internal error)");
        if (p.split) {
            if (o.splits->size() != n_run) return fail(c, STR_ER_EHIP, "run split: the split records are not the runs' (internal error)");
            for (const str_er_run_split &S : *o.splits)
                if (S.n_cuts < 0 || S.n_cuts > 3 || (S.n_pieces > 0 && (S.first_piece < 0 || (size_t)S.first_piece + (size_t)S.n_pieces > n_pc)))
                    return fail(c, STR_ER_EHIP, "run split: a run's pieces outside the piece table (internal error)");
            if (!rs_word_slots(o.splits->data(), TH.first, TH.n_of, n_words, slot, &n_slots)) return fail(c, STR_ER_ECAPACITY, "run split: more than 2^31 parts to reserve");
        }
        if (p.track || p.tdecode) {
            const size_t n_members = o.track_members->size();
            for (const str_er_word_track &G : *o.tracks) {
                if (G.first < 0 || G.count < 0 || (size_t)G.first + (size_t)G.count > n_members)
                    return fail(c, STR_ER_EHIP, "track read: a track outside the member array (internal error)");
                tfirst.push_back(G.first); tcount.push_back(G.count);
            }
            for (const int32_t w : *o.track_members)
                if (w < 0 || (size_t)w >= n_words) return fail(c, STR_ER_EHIP, "track read: a member outside the words (internal error)");
        }
        if (atlas_bytes > c->run_atlas.size()) {
            if ((rc = c->run_atlas.ensure(c, atlas_bytes, "run tile atlas")) != STR_ER_OK) return rc;
            ++c->n_atlas_grown;
        }
        if ((rc = ensure_scratch(c, ocr_layout(nullptr, n, m, true, false, p.any()).bytes)) != STR_ER_OK) return rc;
        buf = ocr_layout(c->scratch.d(), n, m, true, false, p.any());
        Carve  cv;
        size_t o_rows[2], o_parts[2];
        for (int set = 0; set < 2; ++set) o_rows[set] = cv.take(p.rows[set] ? 65 * n_rows : 0);
        for (int set = 0; set < 2; ++set) o_parts[set] = cv.take(p.parts[set] ? 65 * (size_t)n_slots : 0);
        if (cv.off > 0) {
            if ((rc = c->read_rows.ensure(c, cv.off, "reading chain rows")) != STR_ER_OK) return rc;
            for (int set = 0; set < 2; ++set) { rows[set] = c->read_rows.d() + o_rows[set]; parts[set] = c->read_rows.d() + o_parts[set]; }
        }
        const int n_chunks = p.match ? wm_chunks(c->lex) : 0;
        if ((p.match && (rc = c->wm_tab.ensure(c, wm_layout(nullptr, 0, n_words, n_chunks).bytes, "word match tables")) != STR_ER_OK) ||
            (p.decode && (rc = c->wd_tab.ensure(c, wd_layout(nullptr, 0, n_words).bytes, "word decode tables")) != STR_ER_OK) ||
            (p.margin && (rc = c->wg_tab.ensure(c, wg_layout(nullptr, 0, n_words, false).bytes, "word margin tables")) != STR_ER_OK) ||
            (p.split && (rc = c->rs_tab.ensure(c, rs_layout(nullptr, 0, n_words, (size_t)n_slots, false).bytes, "run split tables")) != STR_ER_OK) ||
            (p.lattice && (rc = c->ld_tab.ensure(c, ld_layout(nullptr, 0, n_words, (size_t)n_slots).bytes, "lattice decode tables")) != STR_ER_OK) ||
            (p.lmargin && (rc = c->lg_tab.ensure(c, lg_layout(nullptr, 0, n_words, false, false).bytes, "lattice margin tables")) != STR_ER_OK) ||
            (p.lmatch && (rc = c->lm_tab.ensure(c, lm_layout(nullptr, 0, n_words, (size_t)n_slots, n_chunks).bytes, "lattice match tables")) != STR_ER_OK))
            return rc;
        if (p.ldecode && !p.split && (rc = line_windows()) != STR_ER_OK) return rc;
        if (p.lldecode && (rc = line_lattice_windows()) != STR_ER_OK) return rc;
        if (p.match) WD = wm_layout(c->wm_tab.d(), 0, n_words, n_chunks);
        if (p.decode) DD = wd_layout(c->wd_tab.d(), 0, n_words);
        if (p.margin) GM = wg_layout(c->wg_tab.d(), 0, n_words, false);
        if (p.split) { SH = rs_layout(c->rs_tab.h(), 0, n_words, (size_t)n_slots, false); SD = rs_layout(c->rs_tab.d(), 0, n_words, (size_t)n_slots, false); }
        if (p.lattice) { LH = ld_layout(c->ld_tab.h(), 0, n_words, (size_t)n_slots); LD = ld_layout(c->ld_tab.d(), 0, n_words, (size_t)n_slots); }
        if (p.lmargin) LG = lg_layout(c->lg_tab.d(), 0, n_words, false, false);
        if (p.lmatch) { MH = lm_layout(c->lm_tab.h(), 0, n_words, (size_t)n_slots, n_chunks); MD = lm_layout(c->lm_tab.d(), 0, n_words, (size_t)n_slots, n_chunks); }
        return STR_ER_OK;
    }

    // the line decode's windows and gap costs, where the word windows are made: a line runs from the first row of its first word to
    // the last row of its last word -- the words of a line lie back to back and cover its runs -- and a gap costs what the runs say
    int line_windows()
    {
        const std::vector<str_er_line_words> &LW = *lines_of;
        std::vector<int32_t> &win = *o.line_windows;
        std::vector<uint32_t> colmax(LW.size());
        std::vector<int32_t>  first(LW.size()), n_of(LW.size());
        for (size_t t = 0; t < LW.size(); ++t) {
            int64_t at = LW[t].first_run;
            if (LW[t].n_words < 0 || (size_t)LW[t].first_word + (size_t)LW[t].n_words > n_words) return fail(c, STR_ER_EHIP, "line decode: a line's words outside the words (internal error)");
            for (int32_t k = 0; k < LW[t].n_words; ++k) {
                const str_er_line_word &W = (*o.words)[(size_t)LW[t].first_word + (size_t)k];
                if (W.first_run != at) return fail(c, STR_ER_EHIP, "line decode: the words of a line do not lie back to back (internal error)");
                at += W.n_runs;
            }
            if (at != (int64_t)LW[t].first_run + LW[t].n_runs) return fail(c, STR_ER_EHIP, "line decode: the words of a line do not cover its runs (internal error)");
            first[t] = win[2 * t] = LW[t].first_run; n_of[t] = win[2 * t + 1] = LW[t].n_runs; colmax[t] = LW[t].colmax;
        }
        if (!str_er_ld::lines_in_rows((int64_t)n_run, first.data(), n_of.data(), (int64_t)LW.size()) ||
            !str_er_ld::gap_costs(runs_of->data(), (int64_t)n_run, nullptr, (int64_t)n_run, first.data(), n_of.data(), colmax.data(), (int64_t)LW.size(), c->word_num, c->word_den,
                                  c->ln_weight, o.line_gaps->data()))
            return fail(c, STR_ER_EHIP, "line decode: a line outside the glyph runs (internal error)");
        return STR_ER_OK;
    }

    // the line lattice decode's windows, gap costs and node slots: a line runs from the first run of its first word to the last run of
    // its last word (the same check as line_windows), a gap costs what the runs say at this setting's weight, and a line's node slot
    // is the atoms of all runs before its first, from the split records the host holds
    int line_lattice_windows()
    {
        const std::vector<str_er_line_words> &LW = *lines_of;
        std::vector<int32_t> &win = *o.ll_windows;
        std::vector<uint32_t> colmax(LW.size());
        ll_first.resize(LW.size()); ll_n_of.resize(LW.size()); ll_slot.resize(LW.size()); ll_slot_end.resize(LW.size());
        for (size_t t = 0; t < LW.size(); ++t) {
            int64_t at = LW[t].first_run;
            if (LW[t].n_words < 0 || (size_t)LW[t].first_word + (size_t)LW[t].n_words > n_words) return fail(c, STR_ER_EHIP, "line lattice decode: a line's words outside the words (internal error)");
            for (int32_t k = 0; k < LW[t].n_words; ++k) {
                const str_er_line_word &W = (*o.words)[(size_t)LW[t].first_word + (size_t)k];
                if (W.first_run != at) return fail(c, STR_ER_EHIP, "line lattice decode: the words of a line do not lie back to back (internal error)");
                at += W.n_runs;
            }
            if (at != (int64_t)LW[t].first_run + LW[t].n_runs) return fail(c, STR_ER_EHIP, "line lattice decode: the words of a line do not cover its runs (internal error)");
            ll_first[t] = win[2 * t] = LW[t].first_run; ll_n_of[t] = win[2 * t + 1] = LW[t].n_runs; colmax[t] = LW[t].colmax;
        }
        std::vector<int32_t> run_slot;
        if (!str_er_ld::lines_in_rows((int64_t)n_run, ll_first.data(), ll_n_of.data(), (int64_t)LW.size()) ||
            !str_er_ld::gap_costs(runs_of->data(), (int64_t)n_run, nullptr, (int64_t)n_run, ll_first.data(), ll_n_of.data(), colmax.data(), (int64_t)LW.size(), c->word_num, c->word_den,
                                  c->ll_weight, o.ll_gaps->data()))
            return fail(c, STR_ER_EHIP, "line lattice decode: a line outside the glyph runs (internal error)");
        if (!str_er_ld::ll_node_slots(o.splits->data(), (int64_t)n_run, run_slot) || (uint64_t)run_slot[n_run] > 0x7FFFFFFFull / (4 * LL_BP_ROW))
            return fail(c, STR_ER_ECAPACITY, "line lattice decode: too many nodes");
        ll_atoms = (size_t)run_slot[n_run];
        for (size_t t = 0; t < LW.size(); ++t) { ll_slot[t] = run_slot[(size_t)ll_first[t]]; ll_slot_end[t] = run_slot[(size_t)ll_first[t] + (size_t)ll_n_of[t]]; }
        o.ll_chars->assign(str_er_ld::LL_PER_NODE * ll_atoms, 0xFF); o.ll_src->assign(str_er_ld::LL_PER_NODE * ll_atoms, 0xFFFF);
        return STR_ER_OK;
    }

    // the line decode's launch on n_lrows rows of `from` (row_map, null: row r is cost row r) with the windows and gap costs of o, and
    // its tables back after the wait
    int line_enqueue(const uint8_t *from, size_t n_lrows, const int32_t *row_map)
    {
        const std::vector<int32_t> &win = *o.line_windows;
        std::vector<int32_t>        first(win.size() / 2), n_of(win.size() / 2);
        for (size_t t = 0; t < first.size(); ++t) { first[t] = win[2 * t]; n_of[t] = win[2 * t + 1]; }
        return line_decode_enqueue(c, s, 0, from, n_lrows, o.line_gaps->data(), first.data(), n_of.data(), nullptr, nullptr, first.size(), row_map, NH, ND, p.lnmargin, false);
    }
    void line_collect(size_t n_lrows)
    {
        std::memcpy(o.line_decodes->data(), NH.dec, sizeof(str_er_line_decode) * o.line_decodes->size());
        if (p.lnmargin) std::memcpy(o.line_margins->data(), NH.margins, sizeof(str_er_line_margin) * o.line_margins->size());
        if (n_lrows == 0) return;
        std::memcpy(o.line_chars->data(), NH.chars, 3 * n_lrows); std::memcpy(o.line_src->data(), NH.src, 2 * 3 * n_lrows);
        std::memcpy(o.line_word_of_row->data(), NH.word_of_row, 4 * n_lrows);
        if (p.lnmargin) {
            std::memcpy(o.line_row_margins->data(), NH.row_margin, 4 * n_lrows); std::memcpy(o.line_gap_margins->data(), NH.gap_margin, 4 * n_lrows);
            std::memcpy(o.line_row_reads->data(), NH.row_read, n_lrows); std::memcpy(o.line_row_alts->data(), NH.row_alt, n_lrows);
            std::memcpy(o.line_gap_moves->data(), NH.gap_move, n_lrows);
        }
    }

    // With split, behind the stage's wait: the rows of a line are the parts of its words in word order (the compacted part table of the
    // call), part k of word w has the cost row slot[w] + k of the decoder's part rows, and rows of one run get no blank between them.
    // One more upload, launch, copy back and wait.
    int line_pass_split()
    {
        const std::vector<str_er_line_words> &LW = *lines_of;
        const size_t          n_lrows = o.parts->size();
        std::vector<int32_t> &win = *o.line_windows;
        std::vector<uint32_t> colmax(LW.size());
        std::vector<int32_t>  first(LW.size()), n_of(LW.size()), row_run(n_lrows), row_map(n_lrows);
        int64_t               at = 0;
        for (size_t t = 0; t < LW.size(); ++t) {
            if (LW[t].n_words < 0 || (size_t)LW[t].first_word + (size_t)LW[t].n_words > n_words) return fail(c, STR_ER_EHIP, "line decode: a line's words outside the words (internal error)");
            const int64_t begin = at;
            for (int32_t k = 0; k < LW[t].n_words; ++k) {
                const size_t             w = (size_t)LW[t].first_word + (size_t)k;
                const str_er_word_split &W = (*o.word_splits)[w];
                if (W.first_part != at || W.n_parts < 0 || (size_t)at + (size_t)W.n_parts > n_lrows)
                    return fail(c, STR_ER_EHIP, "line decode: the parts of a line's words do not lie back to back (internal error)");
                for (int32_t j = 0; j < W.n_parts; ++j) { row_map[(size_t)at + (size_t)j] = slot[w] + j; row_run[(size_t)at + (size_t)j] = (*o.parts)[(size_t)at + (size_t)j].run; }
                at += W.n_parts;
            }
            first[t] = win[2 * t] = (int32_t)begin; n_of[t] = win[2 * t + 1] = (int32_t)(at - begin); colmax[t] = LW[t].colmax;
        }
        o.line_chars->assign(3 * n_lrows, 0xFF); o.line_src->assign(3 * n_lrows, 0xFFFF); o.line_word_of_row->assign(n_lrows, -1); o.line_gaps->assign(2 * n_lrows, 0);
        if (p.lnmargin) {
            o.line_row_margins->assign(n_lrows, -1); o.line_gap_margins->assign(n_lrows, -1);
            o.line_row_reads->assign(n_lrows, 0xFF); o.line_row_alts->assign(n_lrows, 0xFF); o.line_gap_moves->assign(n_lrows, 0xFF);
        }
        if (!str_er_ld::gap_costs(runs_of->data(), (int64_t)n_run, row_run.data(), (int64_t)n_lrows, first.data(), n_of.data(), colmax.data(), (int64_t)LW.size(), c->word_num,
                                  c->word_den, c->ln_weight, o.line_gaps->data()))
            return fail(c, STR_ER_EHIP, "line decode: a part outside the glyph runs (internal error)");
        if (LW.empty()) return STR_ER_OK;
        if (const int rc = line_enqueue(parts[p.decode_set], n_lrows, row_map.data()); rc != STR_ER_OK) return rc;
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(c->ln_tab.h() + NH.o_dec, c->ln_tab.d() + NH.o_dec, NH.down_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, wait_stream(c, s));
        line_collect(n_lrows);
        return STR_ER_OK;
    }

    // the window of a word in a row set: with split its parts' rows from its slot on, else its runs' rows
    struct Window { const uint8_t *rows; const int32_t *first, *n; };
    Window window(int set) const { return p.split ? Window{parts[set], TD.slot, SD.n_parts} : Window{rows[set], TD.first, TD.n_of}; }

    // a row set: k_run_costs on n_rows rows (the pieces' behind the runs'), and where the plan says so k_split_words into its part rows
    void make_set(int set, bool fold)
    {
        if (p.rows[set]) launch_run_costs(s, buf.prob, (int)n_rows, m->k, m->label, fold, rows[set]);
        if (p.parts[set])
            launch_split_words(s, TD.splits, rows[set], rows[set] + 65 * n_run, TD.first, TD.n_of, TD.slot, (int)n_words, c->rs_split, SD.word_out, SD.parts, parts[set], SD.n_parts);
    }

    // phase 3: the tables up in one copy, the scorer's chain, and behind it the plan's launches in the plan's order
    int enqueue()
    {
        std::memcpy(TH.tiles, tiles.data(), sizeof(RunTile) * n);
        std::memcpy(TH.boxes, boxes.data(), 16 * n);
        std::memcpy(TH.rot, rot.data(), sizeof(RotGeom) * n);
        if (p.split && n_words > 0) std::memcpy(TH.slot, slot.data(), 4 * n_words);
        if (p.split) std::memcpy(TH.splits, o.splits->data(), sizeof(str_er_run_split) * n_run);
        HIP_TRY(c, hipMemcpyAsync(c->run_tab.d(), c->run_tab.h(), TH.bytes, hipMemcpyHostToDevice, s));
        launch_run_tiles(s, TD.tiles, (int)n, c->foot_bits.d<uint64_t>(), c->run_atlas.d(), A.width);
        OcrSrc src{};
        src.plane = c->run_atlas.d(); src.stride = (int32_t)A.width; src.inv = 0; src.boxes = TD.boxes; src.rot = TD.rot;
        launch_ocr_features(s, src, (int)n, buf, m);
        if (m) launch_svm_score(s, (int)n, buf, *m, true);
        make_set(SET_A, p.fold_a);
        if (p.match) {
            const Window W = window(p.match_set);
            launch_word_match(s, c->lex, c->wm_prm, W.rows, W.first, W.n, (int)n_words, WD.partial, WD.matches);
            if (p.track && !tfirst.empty())
                if (const int rc = track_match_enqueue(c, s, W.rows, W.first, W.n, tfirst.data(), tcount.data(), o.track_members->data(), o.track_members->size(), tfirst.size(), KD);
                    rc != STR_ER_OK)
                    return rc;
        }
        if (p.lmatch && n_words > 0)          // the matcher's rows of the runs and, behind them, the pieces: folded when they are staged
            launch_lattice_match(s, c->lex, c->wm_prm, c->rs_split, TD.splits, rows[p.lattice_match_set], rows[p.lattice_match_set] + 65 * n_run, TD.first, TD.n_of, TD.slot,
                                 (int)n_words, MD.partial, reinterpret_cast<int32_t *>(MD.matches), MD.src, reinterpret_cast<int32_t *>(MD.parts));
        if (p.ltrack && !tfirst.empty())          // the same rows and records, and the tracks the track match took
            if (const int rc = lattice_track_enqueue(c, s, 0, TD.splits, rows[p.lattice_track_set], rows[p.lattice_track_set] + 65 * n_run, TD.first, TD.n_of, o.splits->data(),
                                                     TH.first, TH.n_of, n_words, tfirst.data(), tcount.data(), o.track_members->data(), o.track_members->size(),
                                                     tfirst.size(), pslot, &n_pslots, GH, GD);
                rc != STR_ER_OK)
                return rc;
        make_set(SET_U, false);
        if (p.decode) {
            const Window W = window(p.decode_set);
            launch_word_decode(s, c->bigram.d(), c->wd_ins, c->wd_del, W.rows, W.first, W.n, (int)n_words, DD.dec, DD.chars, DD.src);
            if (p.margin)          // the decoder's window, its records, labels and sources where it left them
                launch_word_margin(s, c->bigram.d(), c->wd_ins, c->wd_del, W.rows, W.first, W.n, (int)n_words, DD.dec, DD.chars, DD.src, GM.margins, GM.row_margin, GM.row_read,
                                   GM.row_alt, nullptr);
            if (p.ldecode && !p.split)          // the runs' rows of the decoder's set, a window a line (and with lnmargin k_line_margin behind it)
                if (const int rc = line_enqueue(rows[p.decode_set], n_run, nullptr); rc != STR_ER_OK) return rc;
            if (p.tdecode && !tfirst.empty())          // the decoder's window, its records and labels where it left them
                if (const int rc = track_decode_enqueue(c, s, 0, W.rows, W.first, W.n, DD.dec, DD.chars, tfirst.data(), tcount.data(), o.track_members->data(),
                                                        o.track_members->size(), tfirst.size(), EH, ED);
                    rc != STR_ER_OK)
                    return rc;
        }
        if (p.lattice && n_words > 0) {          // unfolded rows of the runs and, behind them, the pieces
            launch_lattice_decode(s, c->bigram.d(), c->wd_ins, c->wd_del, c->rs_split, TD.splits, rows[p.lattice_set], rows[p.lattice_set] + 65 * n_run, TD.first, TD.n_of, TD.slot,
                                  (int)n_words, reinterpret_cast<int32_t *>(LD.dec), LD.chars, LD.src, reinterpret_cast<int32_t *>(LD.parts));
            if (p.lmargin)          // the same rows and words, the decoder's records, labels, sources and parts where it left them
                launch_lattice_margin(s, c->bigram.d(), c->wd_ins, c->wd_del, c->rs_split, TD.splits, rows[p.lattice_set], rows[p.lattice_set] + 65 * n_run, TD.first, TD.n_of,
                                      TD.slot, (int)n_words, reinterpret_cast<const int32_t *>(LD.dec), LD.chars, LD.src, reinterpret_cast<const int32_t *>(LD.parts), LG.margins,
                                      LG.read_margin, LG.cut_margin, LG.read, LG.alt, LG.cut_alt, nullptr, nullptr);
            if (p.ltdecode && !tfirst.empty())          // the same rows and records, the decoder's records and labels where it left them, the track decode's tracks
                if (const int rc = lattice_track_decode_enqueue(c, s, 0, TD.splits, rows[p.lattice_set], rows[p.lattice_set] + 65 * n_run, TD.first, TD.n_of, LD.dec, LD.chars,
                                                                o.splits->data(), TH.first, TH.n_of, n_words, tfirst.data(), tcount.data(), o.track_members->data(),
                                                                o.track_members->size(), tfirst.size(), qslot, &n_qslots, QH, QD);
                    rc != STR_ER_OK)
                    return rc;
            if (p.lldecode && !ll_first.empty())          // the same rows and records, a window a line: nothing of it waits for the device
                if (const int rc = line_lattice_enqueue(c, s, 0, TD.splits, rows[p.lattice_set], rows[p.lattice_set] + 65 * n_run, n_run, o.ll_gaps->data(), ll_first.data(),
                                                        ll_n_of.data(), ll_slot.data(), ll_first.size(), ll_atoms, YH, YD);
                    rc != STR_ER_OK)
                    return rc;
        }
        HIP_TRY(c, hipGetLastError());
        return STR_ER_OK;
    }

    // phase 4: the wait, the copies back into the caller's tables (pageable memory, as the line scoring does), the parts compacted
    int collect(std::vector<str_er_run_read> *reads, std::vector<uint8_t> &q, const RunPieces *pieces)
    {
        std::vector<int32_t> label(reads ? n : 0);
        std::vector<double>  prob(reads ? n : 0);
        const auto           down = [&](void *to, const void *from, size_t bytes) { return bytes ? hipMemcpyAsync(to, from, bytes, hipMemcpyDeviceToHost, s) : hipSuccess; };
        HIP_TRY(c, wait_stream(c, s));
        HIP_TRY(c, down(q.data(), buf.q, 1800 * n_run));
        if (n_pc > 0) HIP_TRY(c, down(pieces->q->data(), buf.q + 1800 * n_run, 1800 * n_pc));
        if (reads) { HIP_TRY(c, down(label.data(), buf.label, 4 * n)); HIP_TRY(c, down(prob.data(), buf.pbest, 8 * n)); }
        if (p.result_set != SET_NONE) {
            HIP_TRY(c, down(o.run_costs->data(), rows[p.result_set], 65 * n_run));
            if (p.split) HIP_TRY(c, down(o.piece_costs->data(), rows[p.result_set] + 65 * n_run, 65 * n_pc));
        }
        if (p.run_probs) HIP_TRY(c, down(o.run_probs->data(), buf.prob, 8 * (size_t)m->k * n_run));
        if (p.match) HIP_TRY(c, down(o.matches->data(), WD.matches, sizeof(str_er_word_match) * n_words));
        if (p.track && !tfirst.empty()) {
            HIP_TRY(c, down(o.track_matches->data(), KD.matches, sizeof(str_er_track_match) * tfirst.size()));
            HIP_TRY(c, down(o.track_member_costs->data(), KD.member_cost, 4 * o.track_members->size()));
        }
        if (p.decode) {
            HIP_TRY(c, down(o.decodes->data(), DD.dec, sizeof(str_er_word_decode) * n_words));
            HIP_TRY(c, down(o.decode_chars->data(), DD.chars, 64 * n_words));
            HIP_TRY(c, down(o.decode_src->data(), DD.src, 64 * n_words));
        }
        if (p.margin) {
            HIP_TRY(c, down(o.margins->data(), GM.margins, sizeof(str_er_word_margin) * n_words));
            HIP_TRY(c, down(o.row_margins->data(), GM.row_margin, 4 * 32 * n_words));
            HIP_TRY(c, down(o.row_reads->data(), GM.row_read, 32 * n_words));
            HIP_TRY(c, down(o.row_alts->data(), GM.row_alt, 32 * n_words));
        }
        if (p.tdecode && !tfirst.empty()) HIP_TRY(c, down(c->td_tab.h() + EH.o_out, c->td_tab.d() + EH.o_out, EH.down_bytes));
        const bool ld_ran = p.ldecode && !p.split && !o.line_decodes->empty();
        if (ld_ran) HIP_TRY(c, down(c->ln_tab.h() + NH.o_dec, c->ln_tab.d() + NH.o_dec, NH.down_bytes));
        if (p.split && n_words > 0) HIP_TRY(c, down(c->rs_tab.h() + SH.o_out, c->rs_tab.d() + SH.o_out, SH.down_tables));          // (into page-locked memory: compacted below)
        if (p.lmargin && n_words > 0) {
            HIP_TRY(c, down(o.lattice_margins->data(), LG.margins, sizeof(str_er_lattice_margin) * n_words));
            HIP_TRY(c, down(o.lattice_read_margins->data(), LG.read_margin, 4 * 32 * n_words));
            HIP_TRY(c, down(o.lattice_cut_margins->data(), LG.cut_margin, 4 * 32 * n_words));
            HIP_TRY(c, down(o.lattice_part_reads->data(), LG.read, 32 * n_words));
            HIP_TRY(c, down(o.lattice_part_alts->data(), LG.alt, 32 * n_words));
            HIP_TRY(c, down(o.lattice_cut_alts->data(), LG.cut_alt, 32 * n_words));
        }
        if (p.lattice && n_words > 0) HIP_TRY(c, down(c->ld_tab.h() + LH.o_dec, c->ld_tab.d() + LH.o_dec, LH.down_bytes));
        const bool ll_ran = p.lldecode && n_words > 0 && !ll_first.empty();
        if (ll_ran) HIP_TRY(c, down(c->ll_tab.h() + YH.o_dec, c->ll_tab.d() + YH.o_dec, YH.down_bytes));
        if (p.lmatch && n_words > 0) HIP_TRY(c, down(c->lm_tab.h() + MH.o_matches, c->lm_tab.d() + MH.o_matches, MH.down_bytes));
        if (p.ltrack && !tfirst.empty()) HIP_TRY(c, down(c->lt_tab.h() + GH.o_matches, c->lt_tab.d() + GH.o_matches, GH.down_bytes));
        const bool ltd_ran = p.ltdecode && !tfirst.empty() && n_words > 0;
        if (ltd_ran) HIP_TRY(c, down(c->ltd_tab.h() + QH.o_out, c->ltd_tab.d() + QH.o_out, QH.down_bytes));
        HIP_TRY(c, wait_stream(c, s));
        if (ld_ran) line_collect(n_run);
        if (ll_ran) {          // the records with their first parts, the parts and their words compacted, labels and sources as they are
            uint64_t total = 0;
            if (!ll_compact(YH.dec, YH.parts, YH.word_of_part, ll_slot.data(), ll_slot_end.data(), ll_first.size(), nullptr, nullptr, nullptr, &total))
                return fail(c, STR_ER_EHIP, "line lattice decode: a line's parts outside its slots (internal error)");
            o.ll_parts->assign((size_t)total, str_er_split_part{0, 0}); o.ll_word_of_part->assign((size_t)total, -1);
            ll_compact(YH.dec, YH.parts, YH.word_of_part, ll_slot.data(), ll_slot_end.data(), ll_first.size(), o.ll_decodes->data(), o.ll_parts->data(), o.ll_word_of_part->data(), &total);
            if (ll_atoms > 0) { std::memcpy(o.ll_chars->data(), YH.chars, str_er_ld::LL_PER_NODE * ll_atoms); std::memcpy(o.ll_src->data(), YH.src, 2 * str_er_ld::LL_PER_NODE * ll_atoms); }
        }
        if (ltd_ran) {          // the member records with their first parts, the parts compacted, the records, labels and sources as they are
            uint64_t total = 0;
            if (!ltd_compact(QH, qslot, n_qslots, nullptr, nullptr, &total)) return fail(c, STR_ER_EHIP, "lattice track decode: a member's parts outside its slots (internal error)");
            o.lattice_track_decode_parts->assign((size_t)total, str_er_split_part{0, 0});
            ltd_compact(QH, qslot, n_qslots, o.lattice_track_decode_members->data(), o.lattice_track_decode_parts->data(), &total);
            std::memcpy(o.lattice_track_decodes->data(), QH.out, sizeof(str_er_track_decode) * tfirst.size());
            std::memcpy(o.lattice_track_decode_chars->data(), QH.chars, 32 * tfirst.size());
            std::memcpy(o.lattice_track_decode_src->data(), QH.src, 32 * o.track_members->size());
        }
        if (p.lmatch && n_words > 0) {          // the records with their first parts, the parts compacted, the sources as they are
            uint64_t total = 0;
            if (!lm_compact(MH, slot, n_slots, nullptr, nullptr, &total)) return fail(c, STR_ER_EHIP, "lattice match: a word's parts outside its slots (internal error)");
            o.lattice_match_parts->assign((size_t)total, str_er_split_part{0, 0});
            lm_compact(MH, slot, n_slots, o.lattice_matches->data(), o.lattice_match_parts->data(), &total);
            std::memcpy(o.lattice_match_src->data(), MH.src, 32 * n_words);
        }
        if (p.ltrack && !tfirst.empty()) {          // the member records with their first parts, the parts compacted, the records and sources as they are
            uint64_t total = 0;
            if (!lt_compact(GH, pslot, n_pslots, nullptr, nullptr, &total)) return fail(c, STR_ER_EHIP, "lattice track: a member's parts outside its slots (internal error)");
            o.lattice_track_parts->assign((size_t)total, str_er_split_part{0, 0});
            lt_compact(GH, pslot, n_pslots, o.lattice_track_members->data(), o.lattice_track_parts->data(), &total);
            std::memcpy(o.lattice_track_matches->data(), GH.matches, sizeof(str_er_track_match) * tfirst.size());
            std::memcpy(o.lattice_track_src->data(), GH.src, 32 * o.track_members->size());
        }
        if (p.tdecode && !tfirst.empty()) {
            std::memcpy(o.track_decodes->data(), EH.out, sizeof(str_er_track_decode) * tfirst.size());
            std::memcpy(o.track_decode_chars->data(), EH.chars, 32 * tfirst.size());
            if (!o.track_members->empty()) std::memcpy(o.track_decode_member_costs->data(), EH.member_cost, 4 * o.track_members->size());
        }
        if (p.lattice && n_words > 0) {          // the records with their first parts, the parts compacted, the strings as they are
            uint64_t total = 0;
            if (!ld_compact(LH, slot, n_slots, nullptr, nullptr, &total)) return fail(c, STR_ER_EHIP, "lattice decode: a word's parts outside its slots (internal error)");
            o.lattice_parts->assign((size_t)total, str_er_split_part{0, 0});
            ld_compact(LH, slot, n_slots, o.lattice_decodes->data(), o.lattice_parts->data(), &total);
            std::memcpy(o.lattice_chars->data(), LH.chars, 64 * n_words);
            std::memcpy(o.lattice_src->data(), LH.src, 64 * n_words);
        }
        if (p.split) {          // the parts compacted, and every run's share of them
            uint64_t total = 0;
            if (!rs_compact(SH, slot, n_slots, nullptr, nullptr, nullptr, &total)) return fail(c, STR_ER_EHIP, "run split: a word's parts outside its slots (internal error)");
            o.parts->assign((size_t)total, str_er_split_part{0, 0});
            rs_compact(SH, slot, n_slots, o.word_splits->data(), o.parts->data(), nullptr, &total);
            for (const str_er_split_part &P : *o.parts)
                if (P.run >= 0 && (size_t)P.run < n_run) ++(*o.splits)[(size_t)P.run].n_parts;
            if (p.ldecode)
                if (const int rc = line_pass_split(); rc != STR_ER_OK) return rc;
        }
        for (size_t i = 0; reads && i < n_run; ++i) (*reads)[i] = str_er_run_read{label[i], str_er_ocr_char(label[i]), prob[i]};
        for (size_t i = 0; reads && pieces && pieces->reads && i < n_pc; ++i)
            (*pieces->reads)[i] = str_er_run_read{label[n_run + i], str_er_ocr_char(label[n_run + i]), prob[n_run + i]};
        return STR_ER_OK;
    }
};

} // namespace

int run_read_stage(str_er_ctx *c, hipStream_t s, const std::vector<FootLine> &lines, const std::vector<str_er_line_words> &line_words,
                   const std::vector<str_er_line_run> &runs, const double *slopes, std::vector<str_er_run_read> *reads, std::vector<uint8_t> &q,
                   const RunPieces *pieces, const ReadChainOut *chain)
{
    // n_run runs and behind them n_pc pieces (str_er_run_split): n tiles, and whatever is per run takes the first n_run of them
    static const ReadChainOut none{};
    const ReadChainOut       &o = chain && reads ? *chain : none;
    const size_t              n_run = runs.size(), n_pc = pieces ? pieces->pieces->size() : 0;
    const ReadPlan p = read_plan(o.matches != nullptr, o.decodes != nullptr, o.splits != nullptr && pieces != nullptr, o.lattice_decodes != nullptr, o.track_matches != nullptr, c->lex.fold != 0,
                                   o.lattice_matches != nullptr, o.lattice_track_matches != nullptr, o.track_decodes != nullptr, o.margins != nullptr, o.lattice_margins != nullptr,
                                   o.lattice_track_decodes != nullptr, o.line_decodes != nullptr, o.line_margins != nullptr, o.ll_decodes != nullptr);
    if (reads) reads->assign(n_run, str_er_run_read{});
    q.assign(1800 * n_run, 0);
    if (pieces) {
        if (pieces->reads) pieces->reads->assign(n_pc, str_er_run_read{});
        pieces->q->assign(1800 * n_pc, 0);
    }
    o.preset(p, n_run, n_pc, (size_t)c->svm.k);
    if (n_run == 0) return STR_ER_OK;
    ReadCall R{c, s, p, o, reads ? &c->svm : nullptr, n_run, n_pc, n_run + n_pc, p.split ? n_run + n_pc : n_run, p.any() ? o.words->size() : 0};
    int      rc = R.geometry(lines, line_words, runs, slopes, pieces);
    if (rc != STR_ER_OK || (rc = R.buffers()) != STR_ER_OK || (rc = R.enqueue()) != STR_ER_OK || (rc = R.collect(reads, q, pieces)) != STR_ER_OK) return rc;
    if (c->dbg_stats)        // developer aid
        std::fprintf(stderr, "[str_er] run read: %zu tiles, atlas %u x %u (%zu bytes, %zu bytes of tiles)\n", R.n, R.A.width, R.A.height, R.atlas_bytes,
                     [&] { size_t b = 0; for (const RunTile &T : R.tiles) b += (size_t)(T.w + 3u) / 4u * 4u * T.h; return b; }());
    return STR_ER_OK;
}

} // namespace str_er_host

extern "C" {

int str_er_feet_read(str_er_ctx *c, int32_t W, int32_t H, const str_er_line_foot *feet, const uint32_t *bits, const double *slopes, int32_t n,
                     str_er_line_words *line_words, str_er_line_run *runs, int32_t cap_runs, int32_t *n_runs, str_er_line_word *words, int32_t cap_words,
                     int32_t *n_words, str_er_run_read *reads, uint8_t *q_out)
try {
    if (!c) return STR_ER_EINVAL;
    return feet_words_read(c, W, H, feet, bits, n, line_words, runs, cap_runs, n_runs, words, cap_words, n_words, true, slopes, reads, q_out);
} ABI_GUARD(c)

int str_er_run_atlas_stats(const str_er_ctx *c, uint64_t *bytes, uint64_t *grown)
{
    if (!c) return STR_ER_EINVAL;
    if (bytes) *bytes = c->run_atlas.size();
    if (grown) *grown = c->n_atlas_grown;
    return STR_ER_OK;
}

} // extern "C"
