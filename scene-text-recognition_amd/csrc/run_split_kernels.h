// run_split_kernels.h -- the launchers of the splitting of touching glyphs (run_split_kernels.hip; the rules are in run_split_rules.h,
// the contract at str_er_run_split in str_er.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/str_er.h"
#include "er_types.h"

namespace str_er {

constexpr int RS_MAX_W = 1024;         // RUN_SPLIT_MAX_W: the profile of a run of up to so many columns lies in LDS; a wider run is not split
constexpr int RS_WAVES = 4;            // runs / words of a workgroup: a wave each

// What k_run_cuts leaves per run slot of k_foot_words: the kept cuts (frame columns, ascending, -1 unused), the threshold and per atom
// the pixels and the row extent in frame rows (the atoms past n_cuts are 0).  The host forms the pieces from the atoms.
struct RunCutRec {
    int32_t  n_cuts, cut[3];
    uint32_t thr;
    uint32_t px[4];
    int32_t  y0[4], y1[4];
    uint32_t pad;
};
static_assert(sizeof(RunCutRec) == 72, "RunCutRec layout (host and device)");

// lines, slots, recs and runs as k_foot_words read and left them (recs and runs: on the device, behind it on the same stream); out has a
// record per run slot.  num / den: the valley threshold.
void launch_run_cuts(hipStream_t s, const FootLine *lines, int n_lines, const WordsSlot *slots, const WordsRec *recs, const WordsRun *runs,
                     const uint64_t *feet, int num, int den, RunCutRec *out);

// splits [n_runs] (n_cuts and first_piece are read), run_costs [n_runs x 65], piece_costs [n_pieces x 65],
// first_run / n_of / slot [n_words] (slot: the word's first part slot = the atoms of the words before it) -> word_out [n_words x 4]
// (n_parts, cost, read_cost, 0), parts [slots x 2] (run, piece) and part_costs [slots x 65], both at the word's slot.  The words must lie
// inside the runs and the pieces inside their rows: the caller checks.  n_parts_out (optional) [n_words]: n_parts again, as the run
// count of the window (slot, n_parts) into part_costs that the matcher and the decoder take.
void launch_split_words(hipStream_t s, const str_er_run_split *splits, const uint8_t *run_costs, const uint8_t *piece_costs, const int32_t *first_run, const int32_t *n_of,
                        const int32_t *slot, int n_words, int split, int32_t *word_out, int32_t *parts, uint8_t *part_costs, int32_t *n_parts_out = nullptr);

} // namespace str_er
