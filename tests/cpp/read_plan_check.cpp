// Host-only check of csrc/read_plan.h (compiled and run by tests/test_host_cpp.py): read_plan against the conditions run_read_stage spelled
// out one by one before they were gathered there -- transcribed below as they stood, buffer names included -- for all 64 inputs
// (match, decode, split, lattice, track, fold).  Both sides are played as a trace: every k_run_costs / k_split_words / consumer launch in
// stream order, each naming the launch that wrote what it reads, and the launch every returned table comes from.  The traces must be equal.
#include <stdio.h>

#include <string>
#include <vector>

#include "read_plan.h"

using namespace str_er_host;

namespace {

struct Trace {
    std::vector<std::string> launches;
    std::string              results;
    int add(const std::string &s) { launches.push_back(s); return (int)launches.size() - 1; }
};
std::string at(int launch) { return launch < 0 ? std::string("#none") : "#" + std::to_string(launch); }

// run_read_stage as it stood: wm_tab's, wd_tab's, rs_tab's and ld_tab's cost rows, rs_tab's two sets of part rows
Trace ref_trace(bool match, bool decode, bool split, bool lattice, bool track, bool lex_fold)
{
    enum { WD_costs, DD_costs, SD_costs, LD_costs, SD_part_costs, SD_part_costs2, N_BUF };
    int   wr[N_BUF] = {-1, -1, -1, -1, -1, -1};          // the launch that wrote the buffer
    Trace t;
    const bool wmatch = match, wtrack = track && wmatch, wdecode = decode, wsplit = split, wlattice = lattice && wsplit;
    const bool rows2 = wsplit && wmatch && wdecode && lex_fold;
    const bool lrows = wlattice && !wdecode && wmatch && lex_fold;
    int        last_split = -1;
    const auto run_costs = [&](bool fold, int into) { wr[into] = t.add(std::string("k_run_costs fold=") + (fold ? "1" : "0")); };
    const auto split_on = [&](int rows, int part_rows) { wr[part_rows] = last_split = t.add("k_split_words rows=" + at(wr[rows])); };
    const auto window = [&](const char *who, int rows, bool parts) { t.add(std::string(who) + " rows=" + at(wr[rows]) + (parts ? " (slot, n_parts)" : " (first, n_of)")); };
    if (wmatch) {
        run_costs(lex_fold, WD_costs);
        if (wsplit) {
            split_on(WD_costs, SD_part_costs);
            window("k_word_match", SD_part_costs, true);
        } else
            window("k_word_match", WD_costs, false);
    }
    if (wtrack) window("k_track_match", wsplit ? SD_part_costs : WD_costs, wsplit);
    const int dcosts = wmatch && !lex_fold ? WD_costs : DD_costs;
    if (wdecode) {
        if (dcosts == DD_costs) run_costs(false, DD_costs);
        if (wsplit) {
            const int part_rows = rows2 ? SD_part_costs2 : SD_part_costs;
            if (dcosts == DD_costs) split_on(dcosts, part_rows);
            window("k_word_decode", part_rows, true);
        } else
            window("k_word_decode", dcosts, false);
    }
    const int scosts = wmatch ? WD_costs : wdecode ? dcosts : SD_costs;
    if (wsplit && !wmatch && !wdecode) {
        run_costs(false, SD_costs);
        split_on(SD_costs, SD_part_costs);
    }
    if (wlattice) {
        const int lcosts = wdecode ? dcosts : wmatch ? (lrows ? LD_costs : WD_costs) : SD_costs;
        if (lrows) run_costs(false, LD_costs);
        t.add("k_lattice_decode rows=" + at(wr[lcosts]) + " (first, n_of, slot)");
    }
    // the copies back
    const int run_costs_from = wmatch ? WD_costs : wdecode ? dcosts : wsplit ? scosts : -1;
    t.results = "run_costs=" + at(run_costs_from < 0 ? -1 : wr[run_costs_from]) + " piece_costs=" + at(wsplit ? wr[scosts] : -1) +
                " run_probs=" + (wmatch || wdecode ? "1" : "0") + " word_splits=" + at(last_split);
    return t;
}

// the same trace, played from the plan alone
Trace plan_trace(const ReadPlan &p)
{
    int   rows[2] = {-1, -1}, parts[2] = {-1, -1};
    Trace t;
    const auto costs = [&](int set, bool fold) { if (p.rows[set]) rows[set] = t.add(std::string("k_run_costs fold=") + (fold ? "1" : "0")); };
    const auto split = [&](int set) { if (p.parts[set]) parts[set] = t.add("k_split_words rows=" + at(rows[set])); };
    const auto window = [&](const char *who, int set) {
        if (set != SET_NONE) t.add(std::string(who) + " rows=" + at(p.split ? parts[set] : rows[set]) + (p.split ? " (slot, n_parts)" : " (first, n_of)"));
    };
    costs(SET_A, p.fold_a);
    split(SET_A);
    window("k_word_match", p.match_set);
    if (p.track) window("k_track_match", p.match_set);
    costs(SET_U, false);
    split(SET_U);
    window("k_word_decode", p.decode_set);
    if (p.lattice_set != SET_NONE) t.add("k_lattice_decode rows=" + at(rows[p.lattice_set]) + " (first, n_of, slot)");
    const int from = p.result_set == SET_NONE ? -1 : rows[p.result_set];
    t.results = "run_costs=" + at(from) + " piece_costs=" + at(p.split ? from : -1) + " run_probs=" + (p.run_probs ? "1" : "0") + " word_splits=" +
                at(p.split_down == SET_NONE ? -1 : parts[p.split_down]);
    return t;
}

} // namespace

int main()
{
    int bad = 0;
    for (int i = 0; i < 64; ++i) {
        const bool match = i & 1, decode = i & 2, split = i & 4, lattice = i & 8, track = i & 16, fold = i & 32;
        const ReadPlan p = read_plan(match, decode, split, lattice, track, fold);
        const Trace    a = ref_trace(match, decode, split, lattice, track, fold), b = plan_trace(p);
        bool           ok = a.launches == b.launches && a.results == b.results;
        // the normalised flags, and a reader never without a writer
        ok = ok && p.match == match && p.decode == decode && p.split == split && p.lattice == (lattice && split) && p.track == (track && match);
        for (const std::string &s : b.launches) ok = ok && s.find("#none") == std::string::npos;
        ok = ok && p.any() == (match || decode || split);
        if (!ok) {
            ++bad;
            printf("match %d decode %d split %d lattice %d track %d fold %d:\n  was:", match, decode, split, lattice, track, fold);
            for (const std::string &s : a.launches) printf(" [%s]", s.c_str());
            printf(" %s\n  plan:", a.results.c_str());
            for (const std::string &s : b.launches) printf(" [%s]", s.c_str());
            printf(" %s\n", b.results.c_str());
        }
    }
    // words_in_rows: the window rule of every entry point
    const int32_t first[3] = {0, 2, 5}, n_of[3] = {2, 3, 0}, neg[1] = {-1}, one[1] = {1}, big[1] = {0x7FFFFFFF};
    if (!words_in_rows(5, first, n_of, 3) || words_in_rows(4, first, n_of, 3) || !words_in_rows(0, first, n_of, 0) || words_in_rows(5, neg, one, 1) ||
        words_in_rows(5, one, neg, 1) || words_in_rows(0x7FFFFFFF, big, big, 1)) {
        ++bad;
        printf("words_in_rows is wrong\n");
    }
    if (bad) { printf("read plan: %d inputs differ\n", bad); return 1; }
    printf("read plan ok: 64 inputs\n");
    return 0;
}
