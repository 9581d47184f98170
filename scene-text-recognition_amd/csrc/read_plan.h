// read_plan.h -- INTERNAL: what the reading chain behind the glyph-run scorer (run_read_stage, api_run_read.cpp) makes and who reads it,
// for every combination of the consumers' flags, in one place.  HIP-free (tests/cpp/read_plan_check.cpp holds it against the conditions
// run_read_stage used to spell out one by one).
// The plan as a table is at the head of api_run_read.cpp.  In short: at most two sets of cost rows, A (the matcher's: folded iff its
// lexicon folds) and U (unfolded; it IS A where the matcher runs and does not fold), with split a set of part rows (k_split_words) per
// row set whose parts a consumer reads, and every consumer and returned table on one of the sets.
#pragma once
#include <stdint.h>

namespace str_er_host {

enum { SET_A = 0, SET_U = 1, SET_NONE = -1 };

struct ReadPlan {
    bool match, decode, split, lattice, track;        // the flags as they count: track only with match, lattice only with split (tdecode, below, only with decode)
    bool lmatch;           // ... and the lattice match only with split and match
    bool ltrack;           // ... and the lattice track match only with the lattice match and the track match
    bool rows[2];          // a k_run_costs launch into the set ([SET_U]: only where U is a set of its own)
    bool fold_a;           // A's launch folds
    bool parts[2];         // a k_split_words launch on the set, into its part rows
    int  match_set, decode_set, lattice_set;        // the set each consumer reads (SET_NONE: it does not run); the track match reads the matcher's
    int  lattice_match_set;                         // ... and the lattice match: A, the matcher's rows (folded when they are read where A is not)
    int  lattice_track_set;                         // ... and the lattice track match: A as well, the runs' rows with the pieces behind them
    int  result_set;       // the set run_costs and piece_costs come from (SET_NONE: the call returns no rows)
    int  split_down;       // the set of the last k_split_words (SET_NONE: none)
    bool run_probs;
    bool tdecode;          // the track decode: only with decode; it reads the decoder's window (decode_set, with split its part rows)
    bool margin;           // the decoder's margins (str_er_set_word_margin): only with decode; the decoder's window, records, labels and sources
    bool lmargin;          // the lattice decoder's margins (str_er_set_lattice_margin): only with lattice; the decoder's window, records, labels, sources and parts
    bool ltdecode;         // the track decode over the members' lattices (str_er_set_lattice_track_decode): only with tdecode and lattice; it reads lattice_set, the lattice decoder's records and labels
    bool ldecode;          // the line decode (str_er_set_line_decode): only with decode; it reads the runs' rows of decode_set, every line one window
    bool lnmargin;         // the line decode's margins (str_er_set_line_margin): only with ldecode; behind it on its rows, gaps, windows, records, labels and sources
    bool lldecode;         // the line decode over the runs' piece lattices (str_er_set_line_lattice_decode): only with lattice; it reads what the lattice decode reads and a gap pair per run
    bool any() const { return match || decode || split; }      // some consumer reads the words and the class probabilities
};

inline ReadPlan read_plan(bool match, bool decode, bool split, bool lattice, bool track, bool fold, bool lmatch = false, bool ltrack = false, bool tdecode = false,
                          bool margin = false, bool lmargin = false, bool ltdecode = false, bool ldecode = false, bool lnmargin = false, bool lldecode = false)
{
    ReadPlan p{};
    p.match = match; p.decode = decode; p.split = split; p.lattice = lattice && split; p.track = track && match;
    p.lmatch = lmatch && split && match;
    p.ltrack = ltrack && p.lmatch && p.track;
    const bool need_u = p.decode || p.lattice || (p.split && !p.match), u_is_a = p.match && !fold;
    const int  u = !need_u ? SET_NONE : u_is_a ? SET_A : SET_U;
    p.rows[SET_A] = p.match; p.rows[SET_U] = u == SET_U;
    p.fold_a = p.match && fold;
    p.parts[SET_A] = p.match && p.split; p.parts[SET_U] = p.split && (p.decode || !p.match) && u == SET_U;
    p.match_set = p.match ? SET_A : SET_NONE;
    p.decode_set = p.decode ? u : SET_NONE;
    p.lattice_set = p.lattice ? u : SET_NONE;
    p.lattice_match_set = p.lmatch ? SET_A : SET_NONE;
    p.lattice_track_set = p.ltrack ? SET_A : SET_NONE;
    p.result_set = p.match ? SET_A : u;
    p.split_down = p.parts[SET_U] ? SET_U : p.parts[SET_A] ? SET_A : SET_NONE;
    p.run_probs = p.match || p.decode;
    p.tdecode = tdecode && p.decode;
    p.margin = margin && p.decode;
    p.lmargin = lmargin && p.lattice;
    p.ltdecode = ltdecode && p.tdecode && p.lattice;
    p.ldecode = ldecode && p.decode;
    p.lnmargin = lnmargin && p.ldecode;
    p.lldecode = lldecode && p.lattice;
    return p;
}

// the words' windows (first_run[w], n_of[w]) lie inside n_rows rows
inline bool words_in_rows(int64_t n_rows, const int32_t *first, const int32_t *n_of, int64_t n_words)
{
    for (int64_t w = 0; w < n_words; ++w)
        if (first[w] < 0 || n_of[w] < 0 || (int64_t)first[w] + n_of[w] > n_rows) return false;
    return true;
}

} // namespace str_er_host
