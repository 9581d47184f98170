// api_run_read.cpp -- the C ABI, part 8c: the reading of the glyph runs of text lines (STR_ER_WANT_RUN_READ behind the line stage of
// api_frame_lines.cpp, str_er_feet_read on uploaded footprints; the contract is at str_er_run_read in str_er.h).  Only the host knows
// the compacted runs, so after the line stage's wait it lays their tiles out in an atlas (pack_run_tiles, words_host.cpp), k_run_tiles
// expands the footprint words still in c->foot_bits into it, and the scorer's launch chain reads the atlas as a device plane
// (run_read_stage: a second enqueue and wait).  With STR_ER_WANT_WORD_MATCH the scorer also leaves its class probabilities, and k_run_costs and
// the matcher (word_match_kernels.h) follow it on the same stream; their tables come down with the same wait.  With STR_ER_WANT_WORD_DECODE
// the decoder (word_decode_kernels.h) follows in the same way, on unfolded cost rows: the matcher's where its lexicon does not fold, else
// those of a second k_run_costs into the decoder's own buffer.  With STR_ER_WANT_RUN_SPLIT (str_er_feet_split: the tiles alone) the pieces of
// the cut runs (api_run_split.cpp) are tiles behind the runs' in the same atlas and rows behind the runs' in the same cost buffer, and
// k_split_words (run_split_kernels.h) goes between k_run_costs and the matcher / decoder, which then read the parts' rows.  With
// STR_ER_WANT_TRACK_READ the track match (api_track_read.cpp) follows the matcher on the same rows, for the word tracks the host made before.
// With STR_ER_WANT_LATTICE_DECODE k_lattice_decode (lattice_decode_kernels.h, api_lattice_decode.cpp) follows the scorer as well: it reads
// what k_split_words reads, on unfolded rows, and its tables come down with the same wait.
#include "str_er_ctx.h"
#include "lattice_decode_kernels.h"
#include "run_split_kernels.h"

namespace str_er_host {

int run_read_stage(str_er_ctx *c, hipStream_t s, const std::vector<FootLine> &lines, const std::vector<str_er_line_words> &line_words,
                   const std::vector<str_er_line_run> &runs, const double *slopes, std::vector<str_er_run_read> *reads, std::vector<uint8_t> &q,
                   const WordMatchOut *match, const WordDecodeOut *decode, const RunPieces *pieces, const TrackReadOut *track, const LatticeOut *lattice)
{
    // n_run runs and behind them n_pc pieces (str_er_run_split): n tiles, and whatever is per run below takes the first n_run of them
    const size_t n_run = runs.size(), n_pc = pieces ? pieces->pieces->size() : 0, n = n_run + n_pc;
    if (reads) reads->assign(n_run, str_er_run_read{});
    q.assign(1800 * n_run, 0);
    if (pieces) {
        if (pieces->reads) pieces->reads->assign(n_pc, str_er_run_read{});
        pieces->q->assign(1800 * n_pc, 0);
    }
    const bool   wmatch = match && reads;
    const size_t n_words = wmatch ? match->words->size() : 0;
    if (wmatch) {
        match->matches->assign(n_words, str_er_word_match{-1, -1, -1, -1, 0, 0});
        match->costs->assign(65 * n_run, 0);
        match->probs->assign((size_t)c->svm.k * n_run, 0.0);
    }
    // STR_ER_WANT_TRACK_READ: the track match behind the matcher, on the rows and the (first, n) arrays it read
    const bool   wtrack = track && wmatch;
    const size_t n_tracks = wtrack ? track->tracks->size() : 0, n_members = wtrack ? track->members->size() : 0;
    if (wtrack) {
        track->matches->assign(n_tracks, str_er_track_match{-1, -1, -1, -1, 0, 0, 0, -1});
        track->member_costs->assign(n_members, -1);
    }
    const bool   wdecode = decode && reads;
    const size_t n_dwords = wdecode ? decode->words->size() : 0;
    if (wdecode) {
        decode->decodes->assign(n_dwords, str_er_word_decode{});
        decode->chars->assign(64 * n_dwords, 0xFF);
        decode->src->assign(64 * n_dwords, 0xFF);
        if (!wmatch) {
            decode->costs->assign(65 * n_run, 0);
            decode->probs->assign((size_t)c->svm.k * n_run, 0.0);
        }
    }
    // STR_ER_WANT_RUN_SPLIT: k_split_words behind k_run_costs, the matcher and the decoder on the parts' rows
    const bool   wsplit = pieces && pieces->splits && reads;
    const size_t n_swords = wsplit ? pieces->words->size() : 0, n_rows = wsplit ? n : n_run;          // (cost rows: the pieces' behind the runs')
    if (wsplit) {
        pieces->costs->assign(65 * n_pc, 0);
        pieces->parts->clear();
        pieces->word_splits->assign(n_swords, str_er_word_split{0, 0, 0, 0});
    }
    // STR_ER_WANT_LATTICE_DECODE: k_lattice_decode on the split records, words and slots of k_split_words
    const bool wlattice = lattice && wsplit;
    if (wlattice) {
        lattice->decodes->assign(n_swords, str_er_lattice_decode{});
        lattice->chars->assign(64 * n_swords, 0xFF);
        lattice->src->assign(64 * n_swords, 0xFF);
        lattice->parts->clear();
    }
    if (n_run == 0) return STR_ER_OK;
    if (n > 0x7FFFFFFFull / 1800) return fail(c, STR_ER_ECAPACITY, "run read: too many glyph runs");
    std::vector<RunTile> tiles(n);
    std::vector<RotGeom> rot(n);
    std::vector<int32_t> line_of(n_pc ? n_run : 0);
    for (size_t t = 0; t < lines.size(); ++t) {
        const FootLine &L = lines[t];
        const double    sl = slopes && std::isfinite(slopes[t]) ? slopes[t] : 0.0;
        for (int32_t k = 0; k < line_words[t].n_runs; ++k) {
            const size_t           i = (size_t)line_words[t].first_run + (size_t)k;
            const str_er_line_run &R = runs[i];
            // (the kernel reads the rows and columns of the run in its line's words: they must lie inside the foot box)
            if (i >= n_run || R.x0 < L.x || R.x1 <= R.x0 || R.x1 > L.x + L.w || R.y0 < L.y || R.y1 <= R.y0 || R.y1 > L.y + L.h)
                return fail(c, STR_ER_EHIP, "run read: a glyph run outside its line's footprint (internal error)");
            RunTile &T = tiles[i];
            T.bit_off = L.word_off + (uint64_t)(R.y0 - L.y) * L.pitch; T.pitch = L.pitch; T.c0 = (uint32_t)(R.x0 - L.x);
            T.w = (uint32_t)(R.x1 - R.x0); T.h = (uint32_t)(R.y1 - R.y0);
            rot[i] = make_rot_geom((int)T.w, (int)T.h, sl);
            if (n_pc) line_of[i] = (int32_t)t;
        }
    }
    for (size_t p = 0; p < n_pc; ++p) {          // a piece: a box inside its run's, in the same line's words, with the line's slope
        const str_er_run_piece &Q = (*pieces->pieces)[p];
        if (Q.run < 0 || (size_t)Q.run >= n_run) return fail(c, STR_ER_EHIP, "run split: a piece outside the glyph runs (internal error)");
        const str_er_line_run &R = runs[(size_t)Q.run];
        const size_t           t = (size_t)line_of[(size_t)Q.run];
        const FootLine        &L = lines[t];
        if (Q.x0 < R.x0 || Q.x1 <= Q.x0 || Q.x1 > R.x1 || Q.y0 < R.y0 || Q.y1 <= Q.y0 || Q.y1 > R.y1)
            return fail(c, STR_ER_EHIP, "run split: a piece outside its glyph run (internal error)");
        RunTile &T = tiles[n_run + p];
        T.bit_off = L.word_off + (uint64_t)(Q.y0 - L.y) * L.pitch; T.pitch = L.pitch; T.c0 = (uint32_t)(Q.x0 - L.x);
        T.w = (uint32_t)(Q.x1 - Q.x0); T.h = (uint32_t)(Q.y1 - Q.y0);
        rot[n_run + p] = make_rot_geom((int)T.w, (int)T.h, slopes && std::isfinite(slopes[t]) ? slopes[t] : 0.0);
    }
    RunAtlas A;
    if (!pack_run_tiles(tiles.data(), n, RUN_SHELF_W, A)) return fail(c, STR_ER_ECAPACITY, "run read: the tiles of the glyph runs do not fit an atlas");
    std::vector<int32_t> boxes(4 * n);
    for (size_t i = 0; i < n; ++i) {
        const RunTile &T = tiles[i];
        if ((uint64_t)T.ax + (T.w + 3u) / 4u * 4u > A.width || (uint64_t)T.ay + T.h > A.height)
            return fail(c, STR_ER_EHIP, "run read: a tile outside the atlas (internal error)");
        boxes[4 * i] = (int32_t)T.ax; boxes[4 * i + 1] = (int32_t)T.ay; boxes[4 * i + 2] = (int32_t)T.w; boxes[4 * i + 3] = (int32_t)T.h;
    }
    const size_t atlas_bytes = (size_t)A.width * A.height;
    const size_t o_box = align_up(sizeof(RunTile) * n, 256), o_rot = align_up(o_box + 16 * n, 256), tab_bytes = o_rot + sizeof(RotGeom) * n;
    const SvmDev *m = reads ? &c->svm : nullptr;
    int rc = STR_ER_OK;
    if (atlas_bytes > c->run_atlas.size()) {
        if ((rc = c->run_atlas.ensure(c, atlas_bytes, "run tile atlas")) != STR_ER_OK) return rc;
        ++c->n_atlas_grown;
    }
    if ((rc = c->run_tab.ensure(c, tab_bytes, "run tile tables")) != STR_ER_OK ||
        (rc = ensure_scratch(c, ocr_layout(nullptr, n, m, true, false, wmatch || wdecode || wsplit).bytes)) != STR_ER_OK)
        return rc;
    const OcrBuf buf = ocr_layout(c->scratch.d(), n, m, true, false, wmatch || wdecode || wsplit);
    WmTab WH{}, WD{};
    if (wmatch) {
        if (n_run > 0x7FFFFFFFull / 65 || n_words > 0x7FFFFFFFull) return fail(c, STR_ER_ECAPACITY, "word match: too many glyph runs");
        for (const str_er_line_word &w : *match->words)
            if (w.first_run < 0 || w.n_runs < 0 || (size_t)w.first_run + (size_t)w.n_runs > n_run)
                return fail(c, STR_ER_EHIP, "word match: a word outside the glyph runs (internal error)");
        const int n_chunks = wm_chunks(c->lex);
        if ((rc = c->wm_tab.ensure(c, wm_layout(nullptr, n_rows, n_words, n_chunks).bytes, "word match tables")) != STR_ER_OK) return rc;
        WH = wm_layout(c->wm_tab.h(), n_rows, n_words, n_chunks); WD = wm_layout(c->wm_tab.d(), n_rows, n_words, n_chunks);
    }
    WdTab DH{}, DD{};
    if (wdecode) {
        if (n_run > 0x7FFFFFFFull / 65 || n_dwords > 0x7FFFFFFFull / 64) return fail(c, STR_ER_ECAPACITY, "word decode: too many glyph runs");
        for (const str_er_line_word &w : *decode->words)
            if (w.first_run < 0 || w.n_runs < 0 || (size_t)w.first_run + (size_t)w.n_runs > n_run)
                return fail(c, STR_ER_EHIP, "word decode: a word outside the glyph runs (internal error)");
        if ((rc = c->wd_tab.ensure(c, wd_layout(nullptr, n_rows, n_dwords).bytes, "word decode tables")) != STR_ER_OK) return rc;
        DH = wd_layout(c->wd_tab.h(), n_rows, n_dwords); DD = wd_layout(c->wd_tab.d(), n_rows, n_dwords);
    }
    RsTab                SH{}, SD{};
    std::vector<int32_t> slot;
    uint64_t             n_slots = 0;
    const bool           rows2 = wsplit && wmatch && wdecode && c->lex.fold != 0;          // (the decoder's parts: unfolded rows of their own)
    if (wsplit) {
        if (n > 0x7FFFFFFFull / 65 || n_swords > 0x7FFFFFFFull) return fail(c, STR_ER_ECAPACITY, "run split: too many glyph runs");
        if (pieces->splits->size() != n_run || (wmatch && match->words != pieces->words) || (wdecode && decode->words != pieces->words))
            return fail(c, STR_ER_EHIP, "run split: the split records are not the runs' (internal error)");
        std::vector<int32_t> first(n_swords), n_of(n_swords);
        for (size_t w = 0; w < n_swords; ++w) {
            const str_er_line_word &L = (*pieces->words)[w];
            if (L.first_run < 0 || L.n_runs < 0 || (size_t)L.first_run + (size_t)L.n_runs > n_run)
                return fail(c, STR_ER_EHIP, "run split: a word outside the glyph runs (internal error)");
            first[w] = L.first_run; n_of[w] = L.n_runs;
        }
        for (const str_er_run_split &S : *pieces->splits)
            if (S.n_cuts < 0 || S.n_cuts > 3 || (S.n_pieces > 0 && (S.first_piece < 0 || (size_t)S.first_piece + (size_t)S.n_pieces > n_pc)))
                return fail(c, STR_ER_EHIP, "run split: a run's pieces outside the piece table (internal error)");
        if (!rs_word_slots(pieces->splits->data(), first.data(), n_of.data(), n_swords, slot, &n_slots))
            return fail(c, STR_ER_ECAPACITY, "run split: more than 2^31 parts to reserve");
        const size_t own_rows = wmatch || wdecode ? 0 : n;          // (the rows are the matcher's or the decoder's where either runs)
        if ((rc = c->rs_tab.ensure(c, rs_layout(nullptr, n_run, own_rows, n_swords, (size_t)n_slots, rows2).bytes, "run split tables")) != STR_ER_OK) return rc;
        SH = rs_layout(c->rs_tab.h(), n_run, own_rows, n_swords, (size_t)n_slots, rows2);
        SD = rs_layout(c->rs_tab.d(), n_run, own_rows, n_swords, (size_t)n_slots, rows2);
        std::memcpy(SH.splits, pieces->splits->data(), sizeof(str_er_run_split) * n_run);
        if (n_swords > 0) {
            std::memcpy(SH.first, first.data(), 4 * n_swords); std::memcpy(SH.n_of, n_of.data(), 4 * n_swords); std::memcpy(SH.slot, slot.data(), 4 * n_swords);
        }
    }
    LdTab      LH{}, LD{};
    const bool lrows = wlattice && !wdecode && wmatch && c->lex.fold != 0;          // (no unfolded rows in this call yet: the lattice's own)
    if (wlattice) {
        if (n_swords > 0x7FFFFFFFull / 64) return fail(c, STR_ER_ECAPACITY, "lattice decode: too many words");
        if ((rc = c->ld_tab.ensure(c, ld_layout(nullptr, 0, lrows ? n : 0, n_swords, (size_t)n_slots, false).bytes, "lattice decode tables")) != STR_ER_OK) return rc;
        LH = ld_layout(c->ld_tab.h(), 0, lrows ? n : 0, n_swords, (size_t)n_slots, false);
        LD = ld_layout(c->ld_tab.d(), 0, lrows ? n : 0, n_swords, (size_t)n_slots, false);
    }
    uint8_t *h = c->run_tab.h(), *d = c->run_tab.d();
    std::memcpy(h, tiles.data(), sizeof(RunTile) * n);
    std::memcpy(h + o_box, boxes.data(), 16 * n);
    std::memcpy(h + o_rot, rot.data(), sizeof(RotGeom) * n);
    HIP_TRY(c, hipMemcpyAsync(d, h, tab_bytes, hipMemcpyHostToDevice, s));
    launch_run_tiles(s, reinterpret_cast<const RunTile *>(d), (int)n, c->foot_bits.d<uint64_t>(), c->run_atlas.d(), A.width);
    OcrSrc src{};
    src.plane = c->run_atlas.d(); src.stride = (int32_t)A.width; src.inv = 0; src.boxes = reinterpret_cast<const int32_t *>(d + o_box);
    src.rot = reinterpret_cast<const RotGeom *>(d + o_rot);
    launch_ocr_features(s, src, (int)n, buf, m);
    if (m) launch_svm_score(s, (int)n, buf, *m, true);
    // k_split_words on n_rows cost rows (the pieces' behind the runs') into one of the sets of part rows
    const auto split_on = [&](const uint8_t *rows, uint8_t *part_rows) {
        launch_split_words(s, SD.splits, rows, rows + 65 * n_run, SD.first, SD.n_of, SD.slot, (int)n_swords, c->rs_split, SD.word_out, SD.parts, part_rows, SD.n_parts);
    };
    if (wsplit) {
        HIP_TRY(c, hipMemcpyAsync(c->rs_tab.d(), c->rs_tab.h(), sizeof(str_er_run_split) * n_run, hipMemcpyHostToDevice, s));
        if (n_swords > 0) HIP_TRY(c, hipMemcpyAsync(c->rs_tab.d() + SH.o_first, c->rs_tab.h() + SH.o_first, SH.up_bytes - SH.o_first, hipMemcpyHostToDevice, s));
    }
    if (wmatch) {
        for (size_t w = 0; w < n_words; ++w) { WH.first[w] = (*match->words)[w].first_run; WH.n_of[w] = (*match->words)[w].n_runs; }
        const size_t o_first = (size_t)(reinterpret_cast<uint8_t *>(WH.first) - c->wm_tab.h());
        if (n_words > 0 && !wsplit) HIP_TRY(c, hipMemcpyAsync(c->wm_tab.d() + o_first, c->wm_tab.h() + o_first, WH.up_bytes - o_first, hipMemcpyHostToDevice, s));
        launch_run_costs(s, buf.prob, (int)n_rows, m->k, m->label, c->lex.fold != 0, WD.costs);
        if (wsplit) {          // (the word's window: its slot and the part count k_split_words leaves on the device)
            split_on(WD.costs, SD.part_costs);
            launch_word_match(s, c->lex, c->wm_prm, SD.part_costs, SD.slot, SD.n_parts, (int)n_words, WD.partial, WD.matches);
        } else
            launch_word_match(s, c->lex, c->wm_prm, WD.costs, WD.first, WD.n_of, (int)n_words, WD.partial, WD.matches);
    }
    TmTab TD{};
    if (wtrack && n_tracks > 0) {
        std::vector<int32_t> tfirst(n_tracks), tcount(n_tracks);
        for (size_t g = 0; g < n_tracks; ++g) {
            const str_er_word_track &G = (*track->tracks)[g];
            if (G.first < 0 || G.count < 0 || (size_t)G.first + (size_t)G.count > n_members)
                return fail(c, STR_ER_EHIP, "track read: a track outside the member array (internal error)");
            tfirst[g] = G.first; tcount[g] = G.count;
        }
        for (const int32_t w : *track->members)
            if (w < 0 || (size_t)w >= n_words) return fail(c, STR_ER_EHIP, "track read: a member outside the words (internal error)");
        if ((rc = track_match_enqueue(c, s, wsplit ? SD.part_costs : WD.costs, wsplit ? SD.slot : WD.first, wsplit ? SD.n_parts : WD.n_of, tfirst.data(),
                                      tcount.data(), track->members->data(), n_members, n_tracks, TD)) != STR_ER_OK)
            return rc;
    }
    const uint8_t *dcosts = wmatch && !c->lex.fold ? WD.costs : DD.costs;          // (the decoder's rows are never folded)
    if (wdecode) {
        for (size_t w = 0; w < n_dwords; ++w) { DH.first[w] = (*decode->words)[w].first_run; DH.n_of[w] = (*decode->words)[w].n_runs; }
        const size_t o_first = (size_t)(reinterpret_cast<uint8_t *>(DH.first) - c->wd_tab.h());
        if (n_dwords > 0 && !wsplit) HIP_TRY(c, hipMemcpyAsync(c->wd_tab.d() + o_first, c->wd_tab.h() + o_first, DH.up_bytes - o_first, hipMemcpyHostToDevice, s));
        if (dcosts == DD.costs) launch_run_costs(s, buf.prob, (int)n_rows, m->k, m->label, false, DD.costs);
        if (wsplit) {
            // (the matcher's parts serve where its rows are not folded; else the same segmentation again -- a fold moves no minimum -- on the unfolded rows)
            uint8_t *part_rows = rows2 ? SD.part_costs2 : SD.part_costs;
            if (dcosts == DD.costs) split_on(dcosts, part_rows);
            launch_word_decode(s, c->bigram.d(), c->wd_ins, c->wd_del, part_rows, SD.slot, SD.n_parts, (int)n_dwords, DD.dec, DD.chars, DD.src);
        } else
            launch_word_decode(s, c->bigram.d(), c->wd_ins, c->wd_del, dcosts, DD.first, DD.n_of, (int)n_dwords, DD.dec, DD.chars, DD.src);
    }
    const uint8_t *scosts = wmatch ? WD.costs : wdecode ? dcosts : SD.costs;          // (the rows the result's piece costs come from)
    if (wsplit && !wmatch && !wdecode) {
        launch_run_costs(s, buf.prob, (int)n_rows, m->k, m->label, false, SD.costs);
        split_on(SD.costs, SD.part_costs);
    }
    if (wlattice && n_swords > 0) {          // unfolded rows of the runs and, behind them, the pieces
        const uint8_t *lcosts = wdecode ? dcosts : wmatch ? (lrows ? LD.costs : WD.costs) : SD.costs;
        if (lrows) launch_run_costs(s, buf.prob, (int)n_rows, m->k, m->label, false, LD.costs);
        launch_lattice_decode(s, c->bigram.d(), c->wd_ins, c->wd_del, c->rs_split, SD.splits, lcosts, lcosts + 65 * n_run, SD.first, SD.n_of, SD.slot, (int)n_swords,
                              reinterpret_cast<int32_t *>(LD.dec), LD.chars, LD.src, reinterpret_cast<int32_t *>(LD.parts));
    }
    HIP_TRY(c, hipGetLastError());
    std::vector<int32_t> label(reads ? n : 0);
    std::vector<double>  prob(reads ? n : 0);
    HIP_TRY(c, wait_stream(c, s));          // (wait, then copy into pageable memory, as the line scoring does)
    HIP_TRY(c, hipMemcpyAsync(q.data(), buf.q, 1800 * n_run, hipMemcpyDeviceToHost, s));
    if (n_pc > 0) HIP_TRY(c, hipMemcpyAsync(pieces->q->data(), buf.q + 1800 * n_run, 1800 * n_pc, hipMemcpyDeviceToHost, s));
    if (reads) {
        HIP_TRY(c, hipMemcpyAsync(label.data(), buf.label, 4 * n, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(prob.data(), buf.pbest, 8 * n, hipMemcpyDeviceToHost, s));
    }
    if (wmatch) {
        if (n_words > 0) HIP_TRY(c, hipMemcpyAsync(match->matches->data(), WD.matches, sizeof(str_er_word_match) * n_words, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(match->costs->data(), WD.costs, 65 * n_run, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(match->probs->data(), buf.prob, 8 * (size_t)m->k * n_run, hipMemcpyDeviceToHost, s));
    }
    if (wtrack && n_tracks > 0) {
        HIP_TRY(c, hipMemcpyAsync(track->matches->data(), TD.matches, sizeof(str_er_track_match) * n_tracks, hipMemcpyDeviceToHost, s));
        if (n_members > 0) HIP_TRY(c, hipMemcpyAsync(track->member_costs->data(), TD.member_cost, 4 * n_members, hipMemcpyDeviceToHost, s));
    }
    if (wdecode) {
        if (n_dwords > 0) {
            HIP_TRY(c, hipMemcpyAsync(decode->decodes->data(), DD.dec, sizeof(str_er_word_decode) * n_dwords, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipMemcpyAsync(decode->chars->data(), DD.chars, 64 * n_dwords, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipMemcpyAsync(decode->src->data(), DD.src, 64 * n_dwords, hipMemcpyDeviceToHost, s));
        }
        if (!wmatch) {
            HIP_TRY(c, hipMemcpyAsync(decode->costs->data(), dcosts, 65 * n_run, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipMemcpyAsync(decode->probs->data(), buf.prob, 8 * (size_t)m->k * n_run, hipMemcpyDeviceToHost, s));
        }
    }
    if (wsplit) {
        if (n_pc > 0) HIP_TRY(c, hipMemcpyAsync(pieces->costs->data(), scosts + 65 * n_run, 65 * n_pc, hipMemcpyDeviceToHost, s));
        if (n_swords > 0) HIP_TRY(c, hipMemcpyAsync(c->rs_tab.h() + SH.o_out, c->rs_tab.d() + SH.o_out, SH.down_tables, hipMemcpyDeviceToHost, s));          // (the parts' rows stay on the device)
        if (!wmatch && !wdecode && pieces->run_costs) {
            pieces->run_costs->assign(65 * n_run, 0);
            HIP_TRY(c, hipMemcpyAsync(pieces->run_costs->data(), scosts, 65 * n_run, hipMemcpyDeviceToHost, s));
        }
    }
    if (wlattice && n_swords > 0) HIP_TRY(c, hipMemcpyAsync(c->ld_tab.h() + LH.o_dec, c->ld_tab.d() + LH.o_dec, LH.down_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(c, s));
    if (wlattice && n_swords > 0) {          // the records with their first parts, the parts compacted, the strings as they are
        uint64_t total = 0;
        if (!ld_compact(LH, slot, n_slots, nullptr, nullptr, &total)) return fail(c, STR_ER_EHIP, "lattice decode: a word's parts outside its slots (internal error)");
        lattice->parts->assign((size_t)total, str_er_split_part{0, 0});
        ld_compact(LH, slot, n_slots, lattice->decodes->data(), lattice->parts->data(), &total);
        std::memcpy(lattice->chars->data(), LH.chars, 64 * n_swords);
        std::memcpy(lattice->src->data(), LH.src, 64 * n_swords);
    }
    if (wsplit) {          // the parts compacted, and every run's share of them
        uint64_t total = 0;
        if (!rs_compact(SH, slot, n_slots, nullptr, nullptr, nullptr, &total)) return fail(c, STR_ER_EHIP, "run split: a word's parts outside its slots (internal error)");
        pieces->parts->assign((size_t)total, str_er_split_part{0, 0});
        rs_compact(SH, slot, n_slots, pieces->word_splits->data(), pieces->parts->data(), nullptr, &total);
        for (const str_er_split_part &P : *pieces->parts)
            if (P.run >= 0 && (size_t)P.run < n_run) ++(*pieces->splits)[(size_t)P.run].n_parts;
    }
    if (reads)
        for (size_t i = 0; i < n_run; ++i) (*reads)[i] = str_er_run_read{label[i], str_er_ocr_char(label[i]), prob[i]};
    if (reads && pieces && pieces->reads)
        for (size_t i = 0; i < n_pc; ++i) (*pieces->reads)[i] = str_er_run_read{label[n_run + i], str_er_ocr_char(label[n_run + i]), prob[n_run + i]};
    if (c->dbg_stats)        // developer aid
        std::fprintf(stderr, "[str_er] run read: %zu tiles, atlas %u x %u (%zu bytes, %zu bytes of tiles)\n", n, A.width, A.height, atlas_bytes,
                     [&] { size_t b = 0; for (const RunTile &T : tiles) b += (size_t)(T.w + 3u) / 4u * 4u * T.h; return b; }());
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
