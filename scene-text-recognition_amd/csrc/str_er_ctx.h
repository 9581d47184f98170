// str_er_ctx.h -- INTERNAL: the context / result structs and the small host helpers shared by the translation units of the C ABI
// (str_er_api.cpp: contexts, batches, the detect entry points, results; api_models.cpp: cascade / libsvm models and the OCR entry points;
//  api_strips.cpp: one plane in strips over several GPUs; api_stages.cpp: the single-stage entry points; api_text_map.cpp / api_frame_lines.cpp: the
//  frame maps and the frame lines; api_run_read.cpp: the reading of the glyph runs; api_word_match.cpp: the lexicon matcher; api_word_decode.cpp: the bigram decoder; lines_host.cpp / words_host.cpp: the host side of the
//  line stage that touches no device).  Not installed, not part of the ABI.
// The helpers in the unnamed namespace are small and private to each translation unit; what one unit defines for the others is declared in str_er_host.
#pragma once
#include "../../include/str_er.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "er_kernels.h"
#include "ocr_kernels.h"
#include "track_kernels.h"
#include "word_match_kernels.h"
#include "track_match_kernels.h"
#include "word_decode_kernels.h"
#include "word_margin_kernels.h"
#include "line_decode_kernels.h"
#include "line_margin_kernels.h"
#include "lattice_margin_kernels.h"
#include "er_group.h"
#include "flood_order.h"
#include "stage_rules.h"
#include "read_plan.h"
#include <functional>
#include <map>
#include <thread>

using namespace str_er;

extern thread_local std::string g_create_error;      // the error text of a failed str_er_create (defined in str_er_api.cpp)

namespace str_er_host {

constexpr int TIE_SLOTS = 16;      // at most so many planes per batch the device hands to the host for the flood order walk without a round trip
                                   // (a context has as many slots as fit 64 MB of page-locked memory, at least 4: str_er_ctx::n_tie_slots)

struct HostCascade {
    bool loaded = false;
    bool real = true;
    std::vector<int32_t> stage_n, stage_thresh;
    std::vector<uint16_t> dim;
    std::vector<double> thr, dir, vp, vn;
    void *d_blob = nullptr;
    CascadeDev dev{};
};

static_assert(sizeof(str_er_node) == 24, "node layout");
static_assert(sizeof(CandRec) == sizeof(str_er_cand), "cand layout");

struct PlaneGeom { int w, h, stride; size_t off; }; // physical planes of one pyramid level

// An on-demand buffer of a context: created by the first call that needs it, grown when a call needs more, never shrunk, freed with
// the context.  Device memory (d), page-locked host memory (h, allocated with the hipHostMalloc flags given) or a pair of both of
// equal size.  It does no accounting: these buffers are not part of the fixed workspace and never were in str_er_workspace_bytes
// (ws_bytes), which bench.py reports.
template <bool DEV, bool HOST> class OnDemand {
public:
    explicit OnDemand(unsigned host_flags = hipHostMallocDefault) : host_flags_(host_flags) {}
    OnDemand(OnDemand &&o) noexcept : host_flags_(o.host_flags_) { *this = std::move(o); }
    OnDemand &operator=(OnDemand &&o) noexcept { std::swap(d_, o.d_); std::swap(h_, o.h_); std::swap(bytes_, o.bytes_); return *this; }
    ~OnDemand() { release(); }
    size_t size() const { return bytes_; }
    template <typename T = uint8_t> T *d() const { static_assert(DEV, "no device side"); return static_cast<T *>(d_); }
    template <typename T = uint8_t> T *h() const { static_assert(HOST, "no page-locked side"); return static_cast<T *>(h_); }
    // room for `need` bytes.  Growing frees first (the contents are lost) and allocates max(need, 2 * size()): hipFree / hipMalloc wait
    // for the whole device, every other context's kernels included.  On failure the buffer is empty.
    int ensure(str_er_ctx *c, size_t need, const char *what);

private:
    void release()
    {
        if (d_) (void)hipFree(d_);
        if (h_) (void)hipHostFree(h_);
        d_ = h_ = nullptr; bytes_ = 0;
    }
    void *d_ = nullptr, *h_ = nullptr;
    size_t bytes_ = 0;
    unsigned host_flags_;
};
using DevBuf = OnDemand<true, false>;
using HostBuf = OnDemand<false, true>;
using PairBuf = OnDemand<true, true>;

} // namespace str_er_host
using namespace str_er_host;

struct str_er_result {
    std::vector<str_er_plane_info> planes;
    std::vector<str_er_cand> cands;
    std::vector<uint32_t> cand_off;          // n_planes + 1
    std::vector<std::vector<str_er_node>> nodes;
    bool have_nodes = false;
    std::vector<int32_t> ocr_label;
    std::vector<double> ocr_prob;
    bool have_ocr = false;
    std::vector<str_er_track> tracks;
    bool have_tracks = false;
    std::vector<str_er_text> texts;
    std::vector<int32_t> text_ers;
    std::vector<str_er_gbound> gbounds;
    std::vector<int32_t> group_all;
    std::vector<int32_t> line_label;
    std::vector<double> line_prob;
    std::vector<uint8_t> line_kept, text_alive;
    bool have_line_ocr = false;
    bool have_texts = false;
    std::vector<str_er_mask> masks;          // STR_ER_WANT_MASKS: per candidate
    std::vector<uint32_t> mask_bits;
    bool have_masks = false;
    std::vector<str_er_shape> shapes;        // STR_ER_WANT_SHAPES: per candidate
    bool have_shapes = false;
    std::vector<str_er_stroke> strokes;      // STR_ER_WANT_STROKES: per candidate
    bool have_strokes = false;
    std::vector<str_er_line_crop> line_crops;     // STR_ER_WANT_LINE_CROPS: per line, and the bytes they index
    std::vector<uint8_t> crop_pixels, glyph_pixels;
    bool have_line_crops = false, have_line_glyphs = false;
    std::vector<str_er_frame_map> frame_maps;    // STR_ER_WANT_TEXT_MAP / _LINE_MAP: per frame, and the maps they index
    std::vector<uint8_t> text_map;
    std::vector<int32_t> line_map;
    bool have_text_map = false, have_line_map = false;
    std::vector<str_er_line_foot> line_feet;     // STR_ER_WANT_FRAME_LINES: per line, the pairs with common pixels, the frame lines and their members
    std::vector<str_er_line_pair> line_pairs;
    std::vector<str_er_frame_line> frame_lines;
    std::vector<int32_t> frame_line_members;
    bool have_frame_lines = false;
    std::vector<str_er_line_link> line_links;    // STR_ER_WANT_LINE_LINKS: the overlaps across adjacent frames, the track of every line, the tracks and their members
    std::vector<int32_t> line_tracks;
    std::vector<str_er_text_track> text_tracks;
    std::vector<int32_t> text_track_members;
    struct EdgeFeet {                            // ... and the footprints of the lines of the first ([0]) and of the last frame ([1])
        int32_t w = 0, h = 0;
        std::vector<str_er_line_foot> feet;
        std::vector<int32_t> lines;
        std::vector<uint32_t> bits;
    } edge_feet[2];
    bool have_line_links = false;
    std::vector<str_er_line_geom> line_geoms;    // STR_ER_WANT_LINE_GEOM: the geometry of every line and of every frame line, and the hull vertices of both
    std::vector<str_er_line_geom> frame_line_geoms;
    std::vector<int32_t> geom_points;
    bool have_line_geom = false;
    std::vector<str_er_line_words> line_words;   // STR_ER_WANT_LINE_WORDS: per line, and the glyph runs and words they index
    std::vector<str_er_line_run> line_runs;
    std::vector<str_er_line_word> words;
    bool have_line_words = false;
    std::vector<str_er_run_read> run_reads;      // STR_ER_WANT_RUN_READ: per run of line_runs, and their 1800 feature bytes each
    std::vector<uint8_t> run_features;
    bool have_run_reads = false;
    std::vector<str_er_word_match> word_matches; // STR_ER_WANT_WORD_MATCH: per word of words, and the cost rows and class probabilities of the runs
    std::vector<uint8_t> run_costs;
    std::vector<double> run_probs;
    bool have_word_matches = false;
    std::vector<str_er_word_decode> word_decodes; // STR_ER_WANT_WORD_DECODE: per word of words, and 64 label and 64 source bytes per word (run_costs / run_probs too)
    std::vector<uint8_t> word_decode_chars, word_decode_src;
    bool have_word_decodes = false;
    std::vector<str_er_word_margin> word_margins; // str_er_set_word_margin beside STR_ER_WANT_WORD_DECODE: per word of words, and 32 row margins, readings and alternatives per word
    std::vector<int32_t> word_row_margins;
    std::vector<uint8_t> word_row_reads, word_row_alts;
    bool have_word_margins = false;
    std::vector<str_er_run_split> run_splits;    // STR_ER_WANT_RUN_SPLIT: per run of line_runs; the pieces they index with a reading and a cost row each;
    std::vector<str_er_run_piece> run_pieces;    // the parts of the words; per word of words
    std::vector<str_er_run_read> piece_reads;
    std::vector<uint8_t> piece_costs;
    std::vector<str_er_split_part> split_parts;
    std::vector<str_er_word_split> word_splits;
    bool have_run_splits = false;
    std::vector<str_er_lattice_decode> lattice_decodes; // STR_ER_WANT_LATTICE_DECODE: per word of words, 64 label and 64 source bytes per word, and the lattice parts
    std::vector<uint8_t> lattice_decode_chars, lattice_decode_src;
    std::vector<str_er_split_part> lattice_parts;
    bool have_lattice_decodes = false;
    std::vector<str_er_lattice_margin> lattice_margins; // str_er_set_lattice_margin beside STR_ER_WANT_LATTICE_DECODE: per word of words, and per word 32 reading and cut margins, readings, alternatives and cut alternatives
    std::vector<int32_t> lattice_read_margins, lattice_cut_margins;
    std::vector<uint8_t> lattice_part_reads, lattice_part_alts, lattice_cut_alts;
    bool have_lattice_margins = false;
    std::vector<str_er_lattice_match> lattice_matches;  // STR_ER_WANT_LATTICE_MATCH: per word of words, 32 source bytes per word, and the parts of the winning entries
    std::vector<uint8_t> lattice_match_src;
    std::vector<str_er_split_part> lattice_match_parts;
    bool have_lattice_matches = false;
    std::vector<str_er_word_link> word_links;    // STR_ER_WANT_TRACK_READ: the word links, the word tracks, their members, the track of every word of words,
    std::vector<str_er_word_track> word_tracks;  // one match per word track and one cost per slot of the member array
    std::vector<int32_t> word_track_members, word_track_of_words;
    std::vector<str_er_track_match> track_matches;
    std::vector<int32_t> track_member_costs;
    bool have_track_read = false;
    std::vector<str_er_track_match> lattice_track_matches;          // STR_ER_WANT_LATTICE_TRACK: one match per word track, one record and 32 source bytes per slot of
    std::vector<str_er_lattice_track_member> lattice_track_members; // the member array, and the members' parts
    std::vector<uint8_t> lattice_track_src;
    std::vector<str_er_split_part> lattice_track_parts;
    bool have_lattice_track = false;
    bool have_word_tracks = false;                // the word links and word tracks above are made: STR_ER_WANT_TRACK_READ or STR_ER_WANT_TRACK_DECODE
    std::vector<str_er_track_decode> track_decodes; // STR_ER_WANT_TRACK_DECODE: one record and 32 label bytes per word track, one cost per slot of the member array
    std::vector<uint8_t> track_decode_chars;
    std::vector<int32_t> track_decode_member_costs;
    bool have_track_decodes = false;
    std::vector<str_er_track_decode> lattice_track_decodes; // str_er_set_lattice_track_decode beside STR_ER_WANT_TRACK_DECODE and STR_ER_WANT_LATTICE_DECODE: one record and 32 label
    std::vector<uint8_t> lattice_track_decode_chars;        // bytes per word track, one record and 32 source bytes per slot of the member array, and the members' parts
    std::vector<str_er_lattice_track_member> lattice_track_decode_members;
    std::vector<uint8_t> lattice_track_decode_src;
    std::vector<str_er_split_part> lattice_track_decode_parts;
    bool have_lattice_track_decodes = false;
    double times[7] = {0, 0, 0, 0, 0, 0, 0};
    std::vector<str_er_line_decode> line_decodes; // str_er_set_line_decode beside STR_ER_WANT_WORD_DECODE: per line of texts; 3 labels and 3 sources per run of line_runs, a word
    std::vector<uint8_t> line_decode_chars;       // per run, the gap costs used (2 bytes per run) and the lines' windows into the runs (first row, row count)
    std::vector<uint16_t> line_decode_src;
    std::vector<int32_t> line_decode_word_of_row, line_decode_windows;
    std::vector<uint8_t> line_gap_costs;
    bool have_line_decodes = false;
    std::vector<str_er_line_margin> line_margins; // str_er_set_line_margin beside the line decode: per line of texts, and per row of the line decode's rows a row margin, a reading,
    std::vector<int32_t> line_row_margins, line_gap_margins;      // an alternative, a gap margin and a gap move
    std::vector<uint8_t> line_row_reads, line_row_alts, line_gap_moves;
    bool have_line_margins = false;
    std::vector<str_er_line_lattice_decode> line_lattice_decodes; // str_er_set_line_lattice_decode beside STR_ER_WANT_LATTICE_DECODE: per line of texts; 3 labels and 3 sources per atom
    std::vector<uint8_t> line_lattice_chars, line_lattice_gap_costs;      // of line_runs, the lines' parts and the word of every part, the gap costs used (2 bytes per run) and the
    std::vector<uint16_t> line_lattice_src;                               // lines' windows into the runs (first run, run count)
    std::vector<str_er_split_part> line_lattice_parts;
    std::vector<int32_t> line_lattice_word_of_part, line_lattice_windows;
    bool have_line_lattice_decodes = false;
};

// A table of a result, as the str_er_result_* accessors hand it out: null (and *n = 0) when its stage did not run, and when it ran but made no
// rows a pointer to `empty` -- never null.  N: the count's type.
template <typename T> inline const T result_empty{};
template <typename T, typename N>
const T *result_table(const str_er_result *r, bool ran, std::vector<T> str_er_result::*table, N *n, const T &empty = result_empty<T>)
{
    if (!r || !ran) { if (n) *n = 0; return nullptr; }
    const std::vector<T> &v = r->*table;
    if (n) *n = (N)v.size();
    return v.empty() ? &empty : v.data();
}

struct str_er_ctx {
    str_er_params prm{};
    std::string err;
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;          // the opposite-rule NMS pass runs here, beside classify
    hipStream_t prio = nullptr;          // high priority: the few small operations that settle an NMS tie (they would queue behind other contexts' big kernels)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool own_stream = false;
    int ppf = 0;                     // logical planes per frame
    std::vector<int> chans;          // channel indices selected by the mask
    size_t slots = 0;                // node slots (== plane pixels) the workspace can hold
    int max_planes = 0;
    static constexpr size_t NB_PLANE_SHARE = 64;     // entries of the workgroup -> plane table (d_nb_plane) per plane of the capacity

    int kept_cap = 0, pool_cap = 0;   // per plane: the most a plane may get
    bool auto_caps = true;            // (neither was given: every plane gets a share of the tables by its pixel count)
    double kept_share = 1.0 / 64, pool_share = 1.0 / 256;   // ... kept nodes / pooled ERs per padded pixel; grown -- and the batch repeated -- on overflow
    size_t kept_total = 0, pool_total = 0;      // entries of the kept-node / pool arrays
    int64_t table_bytes = 0;
    double min_ocr_prob = 0.15;       // MIN_OCR_PROBABILITY (inc/utils.h), the ERFilter constructor's last argument
    bool   tile_sparse = true;        // which size of k_tile_tree the next batch uses (er_kernels.hip: FOLD_CAP_SPARSE / _DENSE)
    uint64_t last_tree_records = 0, last_tree_pairs = 0, last_tree_tiles = 0;     // of the last batch (str_er_last_tree_stats)
    bool   spin_wait = false;          // STR_ER_SPIN_WAIT=1: always hipStreamSynchronize (busy-waits on a core), see wait_stream
    int    wait_spin_us = 300;         // how long wait_stream polls before it sleeps between polls (run_batch: 2 ms for a call of a frame or two)
    bool   dbg_tile_only = false, dbg_stats = false;   // developer aids (STR_ER_DEBUG_TILE_ONLY / _STATS), read once at create
    int    tile_mode = 0;             // 0 auto (from the node density of the previous batch), 1 sparse, 2 dense (STR_ER_TILE_KERNEL)
    int64_t ws_bytes = 0;

    // device workspace
    uint8_t *d_in = nullptr;  size_t in_bytes = 0;    // staging for host inputs
    uint8_t *d_pix = nullptr; size_t pix_bytes = 0;   // physical planes (Y,Cr,Cb per level)
    PlaneDesc *d_planes = nullptr;
    PlaneCtr *d_ctr = nullptr;
    uint8_t *d_zero = nullptr, *h_zero = nullptr; size_t zero_gd_off = 0;      // the block a batch zeroes: d_total | d_ctr | d_group_done (and its page-locked mirror: h_total | h_ctr)
    size_t zero_clean_bytes = 0;      // so many bytes of d_zero are zero already: filled behind the last call's results (run_batch), off the next call's critical path
    int planes_on_device = 0;         // plane descriptors in d_planes = the first so many of h_planes (0: none)
    NodeArrays na{};
    KeptArrays ka{};
    uint16_t *d_seam = nullptr; size_t seam_slots = 0;
    size_t node_slots = 0;            // node records allocated (NodeArrays::rec / aux)
    uint32_t node_blocks_cap = 0;     // workgroups per plane in k_resolve / k_reduce; 0 = by the frames' content (STR_ER_NODE_BLOCKS sets it)
    uint32_t node_blocks = 12;        // workgroups per plane of the per-record kernels: from the record counts of the previous batch
    double node_share = 0.06;         // records per padded plane pixel (S-text needs 0.006, S-noise 0.09); grown -- and the batch repeated -- when a plane runs out
    uint16_t *d_tile_plane = nullptr, *d_sb_plane = nullptr; uint32_t *d_sb_first = nullptr; size_t sb_slots = 0;
    std::vector<uint16_t> h_tile_plane, h_sb_plane; std::vector<uint32_t> h_sb_first;
    std::vector<uint32_t> layout_key;   // (w,h,...) of the batch whose tables are on the device
    uint32_t *d_tile_nbase = nullptr; size_t tile_slots = 0;
    // the batch's tiles split between the two tile kernels (launch_tile_trees): the planes k_tile_tree2 takes (chroma: few levels per tile) as
    // pairs of tiles, the others as a list for k_tile_tree, and the tiles k_tile_tree2 hands back (their count: d_total[1])
    int       t2_mode = 1;                            // STR_ER_TILE2: 0 off, 1 the chroma planes (ch % 3 != 0), 2 every plane
    int       t2_backoff = 0;                         // batches for which the chroma planes stay with k_tile_tree (the last batch handed too many tiles back)
    uint32_t *d_t1_list = nullptr, *d_t2_pairs = nullptr, *d_fb_list = nullptr;
    std::vector<uint32_t> h_t1_list, h_t2_pairs, t2_key;
    uint32_t  n_t2_tiles = 0;                         // tiles of the planes k_tile_tree2 takes in the current lists
    uint64_t  t2_tiles_total = 0, t2_fb_total = 0;    // statistics (str_er_tile2_stats)
    uint32_t *d_pool = nullptr, *d_pool_tmp = nullptr;
    CandRec *d_cands = nullptr, *d_cands2 = nullptr;      // (second set: the layout after an NMS tie pass changed pools, then swapped)
    uint32_t *d_redo = nullptr;                          // candidates to classify again + their count (last word)
    TrackRec *d_track = nullptr; uint32_t *d_track_list = nullptr, *d_ranges = nullptr;   // STR_ER_STAGE_TRACK
    DevBuf group, group_pairs;                        // STR_ER_STAGE_GROUP: the grouping workspace and the pair list, both of 32-bit words
    uint32_t *d_total = nullptr;
    uint32_t *d_wparent = nullptr;
    // tie planes exported by the device itself (k_export_tie_planes): TIE_SLOTS x tie_slot_bytes of page-locked, device-addressable memory,
    // then the slot -> plane table and the slot counter
    uint8_t *h_tie = nullptr; size_t tie_slot_bytes = 0; int n_tie_slots = 0; uint32_t *h_tie_plane = nullptr, *h_tie_count = nullptr;
    HostBuf replay_host{hipHostMallocMapped};         // the planes (and watch lists) the flood order walk reads
    uint32_t *d_watch = nullptr, *d_wstamp = nullptr; // NMS: watched key pixels per plane (k_nms -> flood order walk) and their stamps (-> k_nms)
    ReplayItem *d_replay_items = nullptr;
    uint32_t *d_alt_list = nullptr;                   // planes of the opposite-rule NMS pass (k_alt_list)
    uint32_t *d_tie_slot_plane = nullptr;             // plane of every tie slot of the batch (k_tie_slots -> k_export_tie_planes)
    DevBuf replay;                                    // flood-replay scratch, of the first batch in which a plane has sibling ties
    uint32_t last_total = 0; bool last_valid = false;   // candidates of the last detect call, still in d_cands (str_er_gather_last)
    uint64_t n_replayed = 0;                          // planes whose NMS ties were decided by a flood replay (statistics)
    double   walk_ms_total = 0;                       // host time those walks took, summed over planes (statistics)
    uint64_t n_batches = 0;
    int  pyr_kernel = 1;                              // STR_ER_PYR_KERNEL: 0 every level of a uniform batch's pyramid by k_resize instead of k_pyr_level; 8 / 16 / 32: that tile height on every level (developer switch)
    bool replay_on_gpu = false;                       // STR_ER_REPLAY=gpu: walk the flood with k_flood_order instead of a host core
    uint16_t *d_cand_plane = nullptr, *d_cand_plane2 = nullptr;
    // the on-demand buffers of the stages (OnDemand)
    DevBuf   scratch;                 // whatever a stage lays out in it (ensure_scratch)
    // STR_ER_WANT_MASKS / str_er_er_masks
    PairBuf  mask;                    // jobs | popcounts | words
    DevBuf   mask_scratch;            // 64-bit words: rows of the boxes too large for LDS
    // STR_ER_WANT_LINE_CROPS / str_er_line_crops (str_er_set_line_crop)
    int32_t  crop_height = 32, crop_max_width = 1024; double crop_pad = 0.125;
    PairBuf  crop;                    // jobs | members | grey | glyph bytes
    // STR_ER_WANT_TEXT_MAP / _LINE_MAP / str_er_text_map_regions
    PairBuf  tmap;                    // the maps (bytes | ids), sized before a call enqueues anything
    PairBuf  tmap_tab;                // tiles | list | regions | xs / ys
    // STR_ER_WANT_FRAME_LINES / str_er_line_feet_regions (str_er_set_frame_merge)
    int32_t  merge_num = 1, merge_den = 2;
    PairBuf  foot_tab;                // lines | jobs | list | members | xs / ys
    PairBuf  foot_out;                // counters | per-line statistics | pairs
    DevBuf   foot_bits;               // 64-bit words: the footprints
    // STR_ER_WANT_LINE_LINKS / str_er_link_feet (str_er_set_line_link)
    int32_t  link_num = 1, link_den = 2;
    PairBuf  link_out;                // counters | pairs | on the page-locked side the edge frames' footprint words
    // STR_ER_WANT_LINE_GEOM / str_er_feet_geom
    PairBuf  geom_out;                // slots | records | hull vertices of k_foot_geom
    DevBuf   geom_x;                  // 64-bit words: the scratch rows of lines taller than its LDS
    // STR_ER_WANT_LINE_WORDS / str_er_feet_words (str_er_set_word_gap)
    int32_t  word_num = 1, word_den = 3;
    PairBuf  words_out;               // slots | records | run slots of k_foot_words
    // STR_ER_WANT_RUN_READ / str_er_feet_read
    DevBuf   run_atlas;               // the byte tiles of the runs of a call (k_run_tiles), in shelves (pack_run_tiles)
    PairBuf  run_tab;                 // tiles | boxes | rotations of the runs | first run, run count, part slot per word and the split records of the reading chain
    DevBuf   read_rows;               // the cost rows of a detect call's reading chain (read_plan.h): A | U | parts of A | parts of U, an absent set taking no bytes
    uint64_t n_atlas_grown = 0;       // statistics: how often run_atlas was allocated or grown (str_er_run_atlas_stats)
    // STR_ER_WANT_WORD_MATCH / str_er_set_lexicon / str_er_match_words / str_er_run_costs
    DevBuf   lexicon;                 // length tables | goff | index | chars of the padded lexicon (lex.n_groups > 0: one is set)
    WmLexDev lex{};
    int32_t  lex_n = 0; uint32_t lex_flags = 0;
    WmParams wm_prm{64, 64, 2};
    PairBuf  wm_tab;                  // (str_er_match_words / _match_tracks: cost rows | first run, run count per word) | chunk keys | matches
    // STR_ER_WANT_TRACK_READ / str_er_match_tracks (str_er_set_word_link)
    int32_t  wlink_num = 1, wlink_den = 2;
    PairBuf  tm_tab;                  // first member, member count per track | members | chunk keys | matches | member costs
    // STR_ER_WANT_WORD_DECODE / str_er_set_bigram / str_er_decode_words
    DevBuf   bigram;                  // the 66 x 66 table (bigram_set: one is set)
    bool     bigram_set = false;
    int32_t  wd_ins = 0, wd_del = 0;
    PairBuf  wd_tab;                  // (str_er_decode_words: cost rows | first run, run count per word) | records | labels | sources
    bool     wd_margin = false;       // str_er_set_word_margin: a detect call with STR_ER_WANT_WORD_DECODE also makes the margins
    PairBuf  wg_tab;                  // (str_er_word_margins: cost rows | first run, run count per word | the decoder's records, labels, sources) | records | row margins | row readings | row alternatives | (marginals)
    // STR_ER_WANT_TRACK_DECODE / str_er_decode_tracks (str_er_set_track_decode)
    int32_t  td_ins = 64, td_del = 64, td_rounds = 8;
    PairBuf  td_tab;                  // (str_er_decode_tracks: cost rows | first run, run count per word | the decoder's records, labels, sources) | first member, member count per track | members | records | labels | member costs
    bool     ltd_on = false;          // str_er_set_lattice_track_decode: a detect call with STR_ER_WANT_TRACK_DECODE and STR_ER_WANT_LATTICE_DECODE also decodes the tracks over their members' lattices
    PairBuf  ltd_tab;                 // (str_er_lattice_decode_tracks: splits | rows of the runs and pieces | first run, run count, slot per word | the lattice decoder's records, labels, sources, parts) | tracks, members and their slots | words' structure | records | labels | member records | sources | parts
    // str_er_feet_split / str_er_split_words (str_er_set_run_split)
    int32_t  rs_num = 1, rs_den = 4, rs_split = 8;
    PairBuf  rs_out;                  // a record per run slot of k_run_cuts
    PairBuf  rs_tab;                  // (str_er_split_words: splits | rows of the runs and pieces | first run, run count, slot per word) | records | parts | (its part rows) | part counts
    // STR_ER_WANT_LATTICE_DECODE / str_er_lattice_decode_words
    bool     ld_margin = false;       // str_er_set_lattice_margin: a detect call with STR_ER_WANT_LATTICE_DECODE also makes the margins
    PairBuf  lg_tab;                  // (str_er_lattice_margins: splits | rows | first run, run count, slot per word | the decoder's records, labels, sources, parts) | records | reading margins | cut margins | readings | alternatives | cut alternatives | (edge minima) | (marginals)
    PairBuf  ld_tab;                  // (str_er_lattice_decode_words: splits | rows of the runs and pieces | first run, run count, slot per word) | records | labels | sources | parts
    // STR_ER_WANT_LATTICE_MATCH / str_er_lattice_match_words
    PairBuf  lm_tab;                  // (str_er_lattice_match_words: splits | rows of the runs and pieces | first run, run count, slot per word) | chunk keys | records | sources | parts
    // STR_ER_WANT_LATTICE_TRACK / str_er_lattice_match_tracks
    PairBuf  lt_tab;                  // (str_er_lattice_match_tracks: splits | rows of the runs and pieces | first run, run count per word) | tracks, members and their slots | words' structure | chunk keys | records | member records | sources | parts | free costs
    // str_er_track_pool_*: what a track pool is bound to (the lexicon, INS / DEL / band, SPLIT) has this generation; their setters bump it
    // (a decode pool has a generation of its own, decode_pool_gen, at the end of the context)
    uint64_t pool_gen = 0;
    DevBuf   strip_out, strip_in;     // strip blobs: made here / uploaded for a merge
    uint32_t *d_strip_flag = nullptr;                 // a strip blob named a node outside its records
    uint16_t *d_nb_plane = nullptr; std::vector<uint16_t> h_nb_plane; uint32_t n_node_blocks = 0;      // plane of every workgroup of the per-record kernels
    uint16_t *d_tile_nrec = nullptr;                  // records per tile (k_tile_tree -> k_group_merge)
    uint16_t *d_group_plane = nullptr; std::vector<uint16_t> h_group_plane;      // plane of every group of tiles
    uint32_t *d_group_list = nullptr; std::vector<uint32_t> h_group_list; uint32_t n_groups_small = 0;      // the groups by class of plane: first those of the chroma planes (few records a tile: k_group_merge with a small table), then the others
    uint32_t *d_undone = nullptr;                     // the groups k_group_merge left alone, listed on the device (their number: d_total[2]) for k_seam_undone
    // k_group_bins (large text-like batches): the groups listed on the device by the table that holds their records -- four lists of tile_slots words, their
    // lengths in d_total[GROUP_BIN_WORD + 0..3], the one-tile groups counted in [GROUP_BIN_WORD + 4]
    static constexpr int GROUP_BIN_WORD = 8;
    uint32_t *d_bin_list = nullptr;
    int       group_bins = 1;                         // STR_ER_GROUP_BINS: 0 the launches per class of PLANE; else by record count: three tables (512 / 1024 / 2528 records), 4: four (+ 2048), 2: two (512 / 2528)
    int       dbg_group_grid = 0;                     // STR_ER_GROUP_GRID: so many workgroups per table, whatever its list holds (developer knob: the kernel's loop)
    int       dbg_cls_grid = 0;                       // STR_ER_CLASSIFY_GRID: so many workgroups of k_classify / k_cand_records, whatever the batch pools (developer knob: the kernels' loops)
    int       dbg_cls_form = 0;                       // STR_ER_CLASSIFY_FORM: another batch build of k_classify (developer knob, for measuring the forms that lost): 8 = 32 candidates on 8 waves, 64 = 64 on 8 waves
    uint32_t  bin_hint[4] = {0, 0, 0, 0}, bin_hint_groups = 0; bool bin_hint_valid = false;      // the lists' lengths in the context's last binned batch (of so many groups): the grids of the next one like it
    uint32_t  last_group_stats[6] = {0, 0, 0, 0, 0, 0};                     // str_er_last_group_stats: groups per table, listed for k_seam_undone, of one tile
    uint8_t  *d_group_done = nullptr;                 // per group of tiles: joined in LDS (k_group_merge -> k_seam)
    int       dbg_group[3] = {0, 0, -1};              // developer knobs STR_ER_GROUP_X / _Y / _KERNEL
    int       group_mode = -1;                        // STR_ER_GROUPS: -1 automatic (4 x 4 tiles with the small tile kernel, 2 x 5 with the big one), 0 off
    std::vector<void *> allocs;

    // pinned host mirrors
    PlaneDesc *h_planes = nullptr;
    PlaneCtr *h_ctr = nullptr;
    uint32_t *h_total = nullptr;
    CandRec  *h_cands_spec = nullptr;                 // small calls: the first SPEC_CANDS candidate records come back WITH the counters (run_batch)
    // STR_ER_STAGE_OCR behind classify, before the host has read a counter (run_batch): the launches are sized for a little more than the last batch's number of
    // strong / weak ERs and work on the device's own count; the results come back with the counters in one page-locked block
    // (count | list | labels | probabilities).  A batch with more ERs than guessed, or whose candidates an NMS tie pass re-made, is scored again the slow way.
    bool      ocr_spec = true;                        // STR_ER_OCR_SPEC=0 turns it off (developer switch)
    size_t    ocr_last_n = 0;                         // strong + weak ERs of the last batch scored
    HostBuf   ocr_host;                               // the results: two regions of 64 + 16 bytes per ER
    size_t    ocr_cap() const { return ocr_host.size() ? (ocr_host.size() / 2 - 64) / 16 : 0; }      // ... for up to so many ERs
    uint64_t  n_ocr_spec = 0, n_ocr_redo = 0;         // statistics: batches scored behind classify / scored again

    // list calls (str_er_detect_*_list): frames of different sizes make a new layout every call, and its tables -- tile / seam-block / group
    // lookups, the list kernels' job tables -- reach the device through one page-locked buffer instead of pageable vectors and a wait.  One
    // buffer does: a list call has waited for its stream by the time it returns.  Allocated by the first list call, for the largest layout.
    bool      stage_tables = false;                   // set during a list call (table_copy)
    uint8_t  *h_stage = nullptr; size_t stage_cap = 0, stage_used = 0;
    uint8_t  *d_list_tab = nullptr; size_t list_tab_bytes = 0;      // the list kernels' job tables (device)

    HostCascade casc[2];
    bool svm_loaded = false;
    SvmDev svm{};
    void *d_svm_blob = nullptr;
    static constexpr int MAX_EV = 32;
    hipEvent_t ev[MAX_EV]{};
    int n_ev = 0;
    bool profiling = false;
    std::vector<std::pair<const char *, double>> profile;
    // pool_gen's sibling: what a decode pool is bound to (the bigram table, the decoder's INS / DEL, the track decode's INS / DEL / rounds)
    // has this generation; their setters bump it.  It stands here, behind everything else, so that no member a detect call touches moves.
    uint64_t decode_pool_gen = 0;
    // str_er_set_line_decode / str_er_decode_lines (behind everything else for the same reason)
    bool     ln_on = false;           // a detect call with STR_ER_WANT_WORD_DECODE also decodes every line
    int32_t  ln_weight = 16;          // the weight of its gap costs
    PairBuf  ln_tab;                  // (str_er_decode_lines: cost rows | first row, row count per line) | gap costs | records | labels | sources | word of every row
    DevBuf   ln_bp;                   // the back pointers of k_line_decode: 68 uint16 per row, scratch
    bool     ln_margin = false;       // str_er_set_line_margin: a detect call that decodes its lines also makes their margins
    DevBuf   ln_fw;                   // the forward values of k_line_margin: 136 uint32 per row, scratch
    int32_t  bigram_ee = 0;           // B[E][E] of the table that is set: what a line without rows costs
    // str_er_set_line_lattice_decode / str_er_lattice_decode_lines (behind everything else for the same reason)
    bool     ll_on = false;           // a detect call with STR_ER_WANT_LATTICE_DECODE also decodes every line over its runs' piece lattices
    int32_t  ll_weight = 16;          // the weight of its gap costs
    PairBuf  ll_tab;                  // splits | rows of the runs and pieces | first run, run count, node slot per line | gap costs | records | labels | sources | parts | word of every part
    DevBuf   ll_bp;                   // the back pointers of k_line_lattice_decode: 68 uint32 per node, scratch
};

namespace {

int fail(str_er_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

// the flags of a detect call against its shape and the context's state (stage_rules.h): before the call stages or enqueues anything
int check_call(str_er_ctx *c, uint32_t stages, const CallShape &k)
{
    const StageVerdict v = check_stages(stages, k, c->casc[0].loaded && c->casc[1].loaded, c->svm_loaded && c->svm.dim == 1800, c->lex_n > 0, c->bigram_set);
    return v.code == STR_ER_OK ? STR_ER_OK : fail(c, v.code, v.msg);
}

// Waiting for a stream.  hipStreamSynchronize busy-waits (so does hipEventSynchronize on a hipEventBlockingSync event, measured): with a batch in
// flight on each of six contexts that is six host cores spinning -- and the GPU boxes grant a process 16 (cgroup quota), which the flood order walks
// of the NMS ties need (round 4: the S-ties bench leg, 86 ms of walks per batch on 16 pool threads + 6 spinning waiters = throttled).  So: poll for
// ~300 us, then sleep between polls.  A latency call (<= SPEC_PLANES planes: a frame or two, under a millisecond of GPU work, one wait at its end) polls
// for 2 ms instead: the 100 us naps added 0.14 ms to most one-frame calls (0.80 ms when the wait happened to end inside the polling, 0.94 otherwise).
// A call of a frame or two (<= SPEC_PLANES planes) is a latency call: its candidate records -- a thousand per 1920 x 1080 frame -- are copied to page-locked
// memory right behind the counters, before the host knows how many there are; if they all fit (and no NMS tie pass re-made them) the second trip to the
// device -- counters, THEN as many records as they say, into pageable memory -- is saved: about 0.1 of a 0.9 ms call.
constexpr uint32_t SPEC_CANDS = 8192;
constexpr int      SPEC_PLANES = 96;

static hipError_t wait_stream(str_er_ctx *c, hipStream_t s)
{
    if (!c || c->spin_wait) return hipStreamSynchronize(s);
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(s);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(c->wait_spin_us)) std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
}

// A host table to the device on c->stream.  In a list call through the page-locked staging buffer: nothing to wait for before the kernels that
// read it.  Otherwise straight from `src` (pageable): the caller waits before `src` changes.
static hipError_t table_copy(str_er_ctx *c, void *dst, const void *src, size_t n)
{
    if (!c->stage_tables) return hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, c->stream);
    size_t at = (c->stage_used + 255) / 256 * 256;
    if (at + n > c->stage_cap) {        // (a batch repeated inside the same call: what was staged before has been read once the stream is idle)
        const hipError_t e = wait_stream(c, c->stream);
        if (e != hipSuccess) return e;
        at = 0;
        if (n > c->stage_cap) return hipErrorInvalidValue;
    }
    std::memcpy(c->h_stage + at, src, n);
    c->stage_used = at + n;
    return hipMemcpyAsync(dst, c->h_stage + at, n, hipMemcpyHostToDevice, c->stream);
}

#define HIP_TRY(ctx, expr)                                                                         \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail((ctx), (e_ == hipErrorOutOfMemory) ? STR_ER_ENOMEM : STR_ER_EHIP,          \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                        \
    } while (0)

template <typename T> int dev_alloc(str_er_ctx *c, T *&p, size_t n)
{
    void *v = nullptr;
    const size_t bytes = std::max<size_t>(n * sizeof(T), 256);
    hipError_t e = hipMalloc(&v, bytes);
    if (e != hipSuccess) return fail(c, STR_ER_ENOMEM, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
    c->allocs.push_back(v);
    c->ws_bytes += (int64_t)bytes;
    p = static_cast<T *>(v);
    return STR_ER_OK;
}

// The node records (32 B + 2 x 4 B per record) are the one part of the workspace whose need depends on the frames' content: they
// are allocated for `node_share` records per pixel and re-allocated larger when a batch overflows them (run_batch).
int alloc_node_records(str_er_ctx *c, size_t n)
{
    if (c->na.rec) { (void)hipFree(c->na.rec); c->ws_bytes -= (int64_t)(c->node_slots * sizeof(NodeRec)); c->na.rec = nullptr; }
    if (c->na.aux) { (void)hipFree(c->na.aux); c->ws_bytes -= (int64_t)(c->node_slots * 8); c->na.aux = nullptr; c->na.arr = nullptr; }
    c->node_slots = 0;
    if (hipMalloc(reinterpret_cast<void **>(&c->na.rec), n * sizeof(NodeRec)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&c->na.aux), n * 8) != hipSuccess)
        return fail(c, STR_ER_ENOMEM, "hipMalloc (node records, " + std::to_string(n * 40) + " bytes)");
    c->na.arr = c->na.aux + n;
    c->node_slots = n;
    c->ws_bytes += (int64_t)(n * 40);
    return STR_ER_OK;
}

// Where the need follows a batch's content (how many ERs are scored, how many lines have members, how many candidates are grouped,
// how large a strip's blob is) a buffer asks for a quarter more than the call needs, so that the next, slightly larger batch does not
// allocate again.  (The scratch used to ask for at least 1.5 x what there was as well: OnDemand::ensure never gives less than 2 x.)
int ensure_quarter_more(str_er_ctx *c, DevBuf &b, size_t need, const char *what)
{
    return need <= b.size() ? STR_ER_OK : b.ensure(c, need + need / 4, what);
}
int ensure_scratch(str_er_ctx *c, size_t bytes) { return ensure_quarter_more(c, c->scratch, bytes, "scratch"); }

void pyr_dims(int w0, int h0, int level, int &w, int &h)
{
    const double s = std::pow(2.0, -0.5 * level);
    w = std::max(1, (int)std::floor(w0 * s + 0.5));
    h = std::max(1, (int)std::floor(h0 * s + 0.5));
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

DetectParams make_dp(const str_er_ctx *c)
{
    DetectParams d{};
    d.thresh_step = c->prm.thresh_step; d.min_area = c->prm.min_area; d.max_area = c->prm.max_area;
    d.stability_t = c->prm.stability_t; d.overlap_coef = c->prm.overlap_coef;
    d.hi = 255 / c->prm.thresh_step + 1;
    d.qscale = (float)(1.0 / (double)c->prm.thresh_step);
    d.kept_cap = c->kept_cap; d.pool_cap = c->pool_cap; d.sibling_order = c->prm.sibling_order;
    return d;
}

} // namespace

template <bool DEV, bool HOST> int str_er_host::OnDemand<DEV, HOST>::ensure(str_er_ctx *c, size_t need, const char *what)
{
    if (need <= bytes_) return STR_ER_OK;
    const size_t get = std::max(need, 2 * bytes_);
    const auto   failed = [&](const char *call) {
        release();
        return fail(c, STR_ER_ENOMEM, std::string(call) + " (" + what + ", " + std::to_string(get) + " bytes)");
    };
    release();
    if (DEV && hipMalloc(&d_, get) != hipSuccess) { d_ = nullptr; return failed("hipMalloc"); }
    if (HOST && hipHostMalloc(&h_, get, host_flags_) != hipSuccess) { h_ = nullptr; return failed("hipHostMalloc"); }
    bytes_ = get;
    return STR_ER_OK;
}

namespace str_er_host {
// ---- batch layout -------------------------------------------------------------------------------
struct Batch {
    std::vector<PlaneDesc> planes;
    uint32_t n_tiles = 0, n_pairs = 0;
    size_t slots = 0, seam = 0, nodes = 0;      // padded pixels, seam entries, node records
    size_t kept = 0, pool = 0;                  // entries of the kept-node / pool arrays handed to the planes
    uint32_t kept_floor = 0, pool_floor = 0;    // str_er_nms_tree: the plane's tables must hold the imported tree
    int planes_per_image = 0;       // BGR frames: planes of one (frame, pyramid level), consecutive in `planes`; 0 = no colour image
    std::vector<int32_t> frame_wh;  // frames: (w, h) at level 0 of every frame of the call, for the text maps; empty = no frames (per-plane calls)
    uint32_t n_groups = 0; int group_x = 0, group_y = 0;       // k_group_merge: groups of group_x x group_y tiles (0: none); assign_groups()
};

inline void add_plane(Batch &b, const uint8_t *pix, int w, int h, int stride, int invert, uint32_t frame, int ch, int pyr)
{
    PlaneDesc d{};
    d.pix = pix; d.w = w; d.h = h; d.stride = stride; d.invert = invert ? 0xFF : 0;
    d.tiles_x = (w + TILE_W - 1) / TILE_W; d.tiles_y = (h + TILE_H - 1) / TILE_H;
    d.tile_base = b.n_tiles; b.n_tiles += (uint32_t)d.tiles_x * d.tiles_y;
    d.n_hpairs = (uint32_t)w * (d.tiles_y - 1);
    d.n_pairs = d.n_hpairs + (uint32_t)h * (d.tiles_x - 1);
    d.pair_base = b.n_pairs; b.n_pairs += d.n_pairs;
    b.slots += (size_t)d.tiles_x * d.tiles_y * TILE_PX;      // (node records are laid out by assign_node_records)
    d.seam_base = (uint32_t)b.seam; b.seam += 2 * (size_t)d.n_pairs;
    d.frame = frame; d.ch = (uint8_t)ch; d.pyr = (uint8_t)pyr;
    b.planes.push_back(d);
}

// ---- defined in str_er_api.cpp, used by the other translation units ------------------------------------------------------------------
using ImportHook = std::function<int(const Batch &, const BatchDev &)>;
void assign_node_records(Batch &b, double share);
void assign_tables(Batch &b, const str_er_ctx *c);
int alloc_tables(str_er_ctx *c, size_t KP, size_t PP);
BatchDev make_batchdev(str_er_ctx *c, const Batch &b);
// an event behind what was enqueued so far.  `always`: one of the few a call needs for str_er_result_times (begin, end of extraction, NMS, classify, track);
// the others -- one per kernel group -- are recorded only while str_er_set_profiling is on: an event between two kernels costs ~7 us of stream time
// (1-frame calls: a dozen of them were a tenth of the call)
void rec(str_er_ctx *c, const char *name, hipStream_t on = nullptr, bool always = false);
RotGeom make_rot_geom(int w, int h, double slope);
int group_phase(str_er_ctx *c, const CandRec *d_cands, const TrackRec *d_track, const std::vector<uint32_t> &img, bool inner_sup, str_er_result *r,
                bool presorted = false);
int resolve_sibling_ties(str_er_ctx *c, const Batch &b, const BatchDev &bd, const DetectParams &dp, bool &replayed, bool from_tree = false);
int group_phase_overlap(str_er_ctx *c, const std::vector<uint32_t> &img, bool inner_sup, str_er_result *r);
int upload_layout(str_er_ctx *c, Batch &b);
int run_batch(str_er_ctx *c, const Batch &b_in, uint32_t stages, str_er_result **out, std::chrono::steady_clock::time_point t_start, bool pre_recorded,
              const ImportHook *import_trees = nullptr);
int stage_input(str_er_ctx *c, const uint8_t *src, size_t bytes, int mem_kind, const uint8_t **dev);
// ---- defined in api_stages.cpp
// the pixel masks of `jobs` (out_off / idx set by the caller, n_words words in all): launched on s, waited for, copied to pixels[idx] and
// bits (bits == null: the words are not copied back) (d_bits, optional: where the words stay on the device, as for mask_launch);
// shapes != null: the SHAPES kernels, shapes[idx] receives the str_er_shape of every mask; strokes != null: the STROKES kernels,
// strokes[idx] receives its str_er_stroke
int mask_stage(str_er_ctx *c, hipStream_t s, std::vector<MaskJob> &jobs, uint64_t n_words, float qscale, uint32_t *pixels, uint32_t *bits,
               const uint32_t **d_bits = nullptr, str_er_shape *shapes = nullptr, str_er_stroke *strokes = nullptr);
// the launches of mask_stage alone: the words stay on the device, at *d_bits (in c->mask, valid until the context's next mask launch)
int mask_launch(str_er_ctx *c, hipStream_t s, std::vector<MaskJob> &jobs, uint64_t n_words, float qscale, const uint32_t **d_bits, bool shapes = false,
                bool strokes = false);
// ---- defined in api_line_crops.cpp
// the str_er_line_crop geometry of one line (STR_ER_EINVAL when it leaves 16.16 fixed point)
int line_crop_geometry(const int32_t *boxes_xywh, int32_t n_boxes, double slope, int32_t height, int32_t max_width, double pad, str_er_line_crop &out);
// STR_ER_WANT_LINE_CROPS / _GLYPHS in run_batch: the crops of the lines of r, from the Y planes of b (planes_per_image > 0)
// (d_mask_bits: the words of this call's STR_ER_WANT_MASKS on the device, or null: then the glyphs' masks are made here)
int line_crop_phase(str_er_ctx *c, hipStream_t s, const Batch &b, float qscale, bool glyphs, const uint32_t *d_mask_bits, str_er_result *r);
// the validated jobs of n regions of one host plane (str_er_er_masks and the other single stages on regions) and the words their masks take;
// region_upload puts the plane in the context's workspace and points the jobs at it
int region_jobs(str_er_ctx *c, const uint8_t *plane, int32_t w, int32_t h, int64_t stride, const str_er_cand *regions, int32_t n,
                const DetectParams &dp, std::vector<MaskJob> &jobs, uint64_t &words);
int region_upload(str_er_ctx *c, const uint8_t *plane, int32_t w, int32_t h, int64_t stride, std::vector<MaskJob> &jobs);
// ---- defined in api_text_map.cpp
// STR_ER_WANT_TEXT_MAP / _LINE_MAP: the output maps of frames (w, h pairs) sized -- before a call enqueues anything
int text_map_reserve(str_er_ctx *c, uint32_t stages, const std::vector<int32_t> &frame_wh);
// ... in run_batch: the maps of the frames of b (b.frame_wh) from the final candidates and lines of r (d_mask_bits: this call's mask words
// on the device, indexed by r->masks, or null: then the masks are made here)
// (d_made_bits / made_word_off, optional: where the masks made here stay on the device and the first word of every candidate's,
// UINT64_MAX for a candidate without one -- left alone when the masks came in through d_mask_bits)
int text_map_phase(str_er_ctx *c, hipStream_t s, const Batch &b, uint32_t stages, float qscale, const uint32_t *d_mask_bits, str_er_result *r,
                   const uint32_t **d_made_bits = nullptr, std::vector<uint64_t> *made_word_off = nullptr);
// the first frame coordinate x in [0, W] whose sample ((2x + 1) * wp) / (2W) is >= a: the pre-image of a level box is
// [first_sample_at(x), first_sample_at(x + w)), the exact inverse of the pixel rule of str_er_frame_map
int32_t first_sample_at(int64_t a, int64_t W, int64_t wp);
// the uint16 tables xs(x) = ((2x + 1) * np) / (2n), x in [0, n), of the pixel rule, one per (frame size, level size) pair asked for
struct SampleTabs {
    std::vector<uint16_t> tabs;
    std::map<std::pair<int32_t, int32_t>, uint32_t> at;
    uint32_t table(int32_t n, int32_t np);       // where the table of (n, np) starts in tabs
};
// ---- defined in api_frame_lines.cpp
// STR_ER_WANT_FRAME_LINES in run_batch: the feet, pairs and frame lines of the lines of r.  d_mask_bits / word_off: mask words of this
// call still on the device and the first word of every candidate's (UINT64_MAX: none), or null: then the members' masks are made here
// want: what rides on the same stage
struct LineStageWants {
    bool links = false;       // STR_ER_WANT_LINE_LINKS: the links, tracks and edge feet of r (k_foot_links)
    bool geom = false;        // STR_ER_WANT_LINE_GEOM: the geometry of the lines and frame lines of r (k_foot_geom)
    bool words = false;       // STR_ER_WANT_LINE_WORDS: the glyph runs and words of the lines of r (k_foot_words)
    bool read = false;        // STR_ER_WANT_RUN_READ: the reading of every run (k_run_tiles and the scorer behind the stage's wait, with a wait of their own)
    bool match = false;       // STR_ER_WANT_WORD_MATCH: every word against the lexicon (k_run_costs and the matcher behind the scorer)
    bool decode = false;      // STR_ER_WANT_WORD_DECODE: every word under the bigram table (k_run_costs and the decoder behind the scorer)
    bool track = false;       // STR_ER_WANT_TRACK_READ: the word links and word tracks on the host before the reading, k_track_match behind the matcher
    bool lattice = false;     // STR_ER_WANT_LATTICE_DECODE: every word over its piece lattice under the bigram table (k_lattice_decode behind the scorer, on what k_split_words reads)
    bool lmatch = false;      // STR_ER_WANT_LATTICE_MATCH: every word against the lexicon over its piece lattice (k_lattice_match behind k_split_words on the matcher's rows)
    bool ltrack = false;      // STR_ER_WANT_LATTICE_TRACK: every word track against the lexicon over its members' piece lattices (k_lattice_track_match behind k_lattice_match)
    bool tdecode = false;     // STR_ER_WANT_TRACK_DECODE: the word links and word tracks on the host before the reading (as for track), k_track_decode behind the decoder
    bool ltdecode = false;    // str_er_set_lattice_track_decode with tdecode and lattice: k_lattice_track_decode behind k_lattice_decode
    bool split = false;       // STR_ER_WANT_RUN_SPLIT: the cuts of every run (k_run_cuts behind k_foot_words, down with the stage's wait), the pieces read with the runs, k_split_words behind the scorer
};
int frame_lines_phase(str_er_ctx *c, hipStream_t s, const Batch &b, float qscale, const uint32_t *d_mask_bits, const std::vector<uint64_t> *word_off,
                      str_er_result *r, const LineStageWants &want);
// the caller's footprints of str_er_feet_words / str_er_feet_read (api_run_read.cpp) cut into runs and words, and with read_runs read
// (slopes, reads, q_out: str_er_feet_read's arguments)
// split (optional): str_er_feet_split's further arguments -- the cuts and pieces of every run, and the pieces read with the runs
struct FeetSplitOut {
    str_er_run_split *splits;
    str_er_run_piece *pieces;
    int32_t           cap_pieces, *n_pieces;
    str_er_run_read  *piece_reads;
    uint8_t          *piece_q;
};
int feet_words_read(str_er_ctx *c, int32_t W, int32_t H, const str_er_line_foot *feet, const uint32_t *bits, int32_t n, str_er_line_words *line_words,
                    str_er_line_run *runs, int32_t cap_runs, int32_t *n_runs, str_er_line_word *words, int32_t cap_words, int32_t *n_words, bool read_runs,
                    const double *slopes, str_er_run_read *reads, uint8_t *q_out, const FeetSplitOut *split = nullptr);
// ---- defined in api_run_split.cpp
// k_run_cuts over the run slots k_foot_words leaves in `words` (the device side of its LinePass buffer: records at o_rec, n_slots run
// slots at o_elem), behind it on s, and the copy back of its records into c->rs_out; run_cuts_collect after the wait: the records
// of the compacted runs (slot_of: the slot of every run) as str_er_run_split, and the pieces formed from the atoms
int run_cuts_enqueue(str_er_ctx *c, hipStream_t s, const FootLine *d_lines, int32_t n_lines, const uint8_t *words, size_t o_rec, size_t o_elem, size_t n_slots);
int run_cuts_collect(str_er_ctx *c, const std::vector<str_er_line_run> &runs, const std::vector<uint32_t> &slot_of, std::vector<str_er_run_split> &splits,
                     std::vector<str_er_run_piece> &pieces);
// ---- defined in api_run_read.cpp
// The reading of the compacted runs of a launch whose footprints are still in c->foot_bits (lines: the table k_foot_words read):
// the tiles laid out and expanded into the atlas, then the scorer's launch chain on the atlas as a device plane with one box a run and
// the slope of the run's line (slopes: one per line, or null: all 0; a slope that is not finite counts as 0).  One upload, the
// launches, the copies back and a wait of its own on s.  reads == null: the features only (no model needed).
// pieces (optional): the pieces of the runs (str_er_run_split) read with them -- their tiles behind the runs' in the one atlas, one
// launch chain over both; reads (null: no labels) and q receive the pieces' results, the runs' are what they are without pieces
struct RunPieces {
    const std::vector<str_er_run_piece> *pieces;
    std::vector<str_er_run_read> *reads;
    std::vector<uint8_t> *q;
};
// chain (optional, with reads): the consumers behind the scorer on s, their tables back with the same wait.  A consumer runs where its
// first table is given; read_plan.h says which cost rows and part rows the call then makes and what every consumer and table reads.
struct ReadChainOut {
    const std::vector<str_er_line_word> *words = nullptr;      // the words every consumer works on
    std::vector<uint8_t> *run_costs = nullptr;                  // the runs' cost rows (match, decode or split) ...
    std::vector<double>  *run_probs = nullptr;                  // ... and class probabilities (match or decode)
    std::vector<str_er_word_match> *matches = nullptr;          // STR_ER_WANT_WORD_MATCH: the words against the context's lexicon
    std::vector<str_er_word_decode> *decodes = nullptr;         // STR_ER_WANT_WORD_DECODE: the words under the context's bigram table
    std::vector<uint8_t> *decode_chars = nullptr, *decode_src = nullptr;
    // str_er_set_word_margin (with decode): the margins of the decoder's strings, behind it on the decoder's window
    std::vector<str_er_word_margin> *margins = nullptr; std::vector<int32_t> *row_margins = nullptr;
    std::vector<uint8_t> *row_reads = nullptr, *row_alts = nullptr;
    // STR_ER_WANT_RUN_SPLIT (with pieces): the segmentation of the words' runs (splits: their records; n_parts is filled in), the pieces'
    // cost rows, the parts and word records; the matcher and the decoder then work on the parts' rows
    std::vector<str_er_run_split> *splits = nullptr; std::vector<uint8_t> *piece_costs = nullptr;
    std::vector<str_er_split_part> *parts = nullptr; std::vector<str_er_word_split> *word_splits = nullptr;
    // STR_ER_WANT_TRACK_READ (with match): the track match of the word tracks the host made before the call
    const std::vector<str_er_word_track> *tracks = nullptr; const std::vector<int32_t> *track_members = nullptr;
    std::vector<str_er_track_match> *track_matches = nullptr; std::vector<int32_t> *track_member_costs = nullptr;
    // STR_ER_WANT_LATTICE_DECODE (with split): the words over their piece lattices under the bigram table
    std::vector<str_er_lattice_decode> *lattice_decodes = nullptr; std::vector<str_er_split_part> *lattice_parts = nullptr;
    std::vector<uint8_t> *lattice_chars = nullptr, *lattice_src = nullptr;
    // str_er_set_lattice_margin (with the lattice decode): the margins of its paths, behind it on what it read and left
    std::vector<str_er_lattice_margin> *lattice_margins = nullptr; std::vector<int32_t> *lattice_read_margins = nullptr, *lattice_cut_margins = nullptr;
    std::vector<uint8_t> *lattice_part_reads = nullptr, *lattice_part_alts = nullptr, *lattice_cut_alts = nullptr;
    // STR_ER_WANT_LATTICE_MATCH (with split and match): the words against the context's lexicon over their piece lattices
    std::vector<str_er_lattice_match> *lattice_matches = nullptr; std::vector<uint8_t> *lattice_match_src = nullptr;
    std::vector<str_er_split_part> *lattice_match_parts = nullptr;
    // STR_ER_WANT_LATTICE_TRACK (with the lattice match and the track match): the word tracks over their members' piece lattices
    std::vector<str_er_track_match> *lattice_track_matches = nullptr; std::vector<str_er_lattice_track_member> *lattice_track_members = nullptr;
    std::vector<uint8_t> *lattice_track_src = nullptr; std::vector<str_er_split_part> *lattice_track_parts = nullptr;
    // STR_ER_WANT_TRACK_DECODE (with decode): the track decode of the word tracks the host made before the call (tracks, track_members: above)
    std::vector<str_er_track_decode> *track_decodes = nullptr; std::vector<uint8_t> *track_decode_chars = nullptr;
    std::vector<int32_t> *track_decode_member_costs = nullptr;
    // str_er_set_lattice_track_decode (with the track decode and the lattice decode): the word tracks decoded over their members' piece lattices
    std::vector<str_er_track_decode> *lattice_track_decodes = nullptr; std::vector<uint8_t> *lattice_track_decode_chars = nullptr, *lattice_track_decode_src = nullptr;
    std::vector<str_er_lattice_track_member> *lattice_track_decode_members = nullptr; std::vector<str_er_split_part> *lattice_track_decode_parts = nullptr;
    // str_er_set_line_decode (with decode): every line decoded jointly with its word breaks, behind the decoder on the runs' rows of its set
    // (line_bee: B[E][E], the cost of a line without rows)
    std::vector<str_er_line_decode> *line_decodes = nullptr; std::vector<uint8_t> *line_chars = nullptr, *line_gaps = nullptr;
    std::vector<uint16_t> *line_src = nullptr; std::vector<int32_t> *line_word_of_row = nullptr, *line_windows = nullptr;
    size_t n_lines = 0; int32_t line_bee = 0;
    // str_er_set_line_margin (with the line decode): the margins of the lines' strings, behind the line decode on its rows
    std::vector<str_er_line_margin> *line_margins = nullptr; std::vector<int32_t> *line_row_margins = nullptr, *line_gap_margins = nullptr;
    std::vector<uint8_t> *line_row_reads = nullptr, *line_row_alts = nullptr, *line_gap_moves = nullptr;
    // str_er_set_line_lattice_decode (with the lattice decode): every line decoded over the piece lattices of its runs, behind the lattice decode on what it
    // read (n_lines and line_bee as for the line decode)
    std::vector<str_er_line_lattice_decode> *ll_decodes = nullptr; std::vector<uint8_t> *ll_chars = nullptr, *ll_gaps = nullptr; std::vector<uint16_t> *ll_src = nullptr;
    std::vector<str_er_split_part> *ll_parts = nullptr; std::vector<int32_t> *ll_word_of_part = nullptr, *ll_windows = nullptr;
    void preset(const ReadPlan &p, size_t n_run, size_t n_pc, size_t k) const;      // every table of the plan as a call without runs leaves it (k: the model's classes)
};
// carving a table buffer: take(bytes) is the offset of the next piece, and the one after it starts at the next multiple of 256
struct Carve {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; }
};
// what a caller-rows entry point (str_er_match_words, _decode_words, _split_words, _lattice_decode_words, _lattice_match_words, _match_tracks, _lattice_match_tracks) puts up at the
// front of its table buffer (base: either side of the pair, or null for the size alone): n_splits split records, n_rows cost rows, the
// words' first run and run count, and with slots their part slot.  The detect calls keep their rows elsewhere (str_er_ctx::read_rows).
struct RowsIn {
    str_er_run_split *splits;
    uint8_t *costs;
    int32_t *first, *n_of, *slot;
    size_t   bytes;
};
RowsIn rows_in_layout(uint8_t *base, size_t n_splits, size_t n_rows, size_t n_words, bool slots);
// the caller's arrays into the front of buf (sized before) and up on s: splits (null: none) of the n_runs runs, the runs' rows and
// behind them the pieces', the words' (first, n) and slot (null: none); D receives the device side of the layout
int rows_in_upload(str_er_ctx *c, hipStream_t s, PairBuf &buf, const str_er_run_split *splits, const uint8_t *run_costs, size_t n_runs, const uint8_t *piece_costs,
                   size_t n_pieces, const int32_t *first, const int32_t *n_of, const int32_t *slot, size_t n_words, RowsIn &D);
// the layout of what k_split_words leaves in c->rs_tab from byte `at` on (the inputs' bytes): n_words word records and part counts,
// n_slots part slots, and with part_rows the parts' rows
struct RsTab {
    int32_t *word_out, *parts, *n_parts;
    uint8_t *part_costs;
    size_t   o_out, bytes;
    size_t   down_tables, down_bytes;        // from o_out: the word records and the parts; ... and the parts' rows behind them
};
RsTab rs_layout(uint8_t *base, size_t at, size_t n_words, size_t n_slots, bool part_rows);
// the part slot of every word: the atoms of the words before it; the total in *n_slots; false above 2^31 - 1
bool rs_word_slots(const str_er_run_split *splits, const int32_t *first_run, const int32_t *n_of, size_t n_words, std::vector<int32_t> &slot, uint64_t *n_slots);
// after the wait: the word records and the compacted parts from the host side of the layout (null parts / part_costs: not copied);
// false where a word's parts lie outside its slots
bool rs_compact(const RsTab &H, const std::vector<int32_t> &slot, uint64_t n_slots, str_er_word_split *word_splits, str_er_split_part *parts, uint8_t *part_costs,
                uint64_t *n_parts);
int run_read_stage(str_er_ctx *c, hipStream_t s, const std::vector<FootLine> &lines, const std::vector<str_er_line_words> &line_words,
                   const std::vector<str_er_line_run> &runs, const double *slopes, std::vector<str_er_run_read> *reads, std::vector<uint8_t> &q,
                   const RunPieces *pieces = nullptr, const ReadChainOut *chain = nullptr);
// ---- defined in api_lattice_decode.cpp
// the layout of what k_lattice_decode leaves in c->ld_tab from byte `at` on (the inputs' bytes), all of which comes down: n_words
// records, labels and sources and n_slots part slots
struct LdTab {
    str_er_lattice_decode *dec; uint8_t *chars, *src; str_er_split_part *parts;
    size_t o_dec, down_bytes, bytes;      // dec | chars | src | parts lie back to back (each aligned): one copy down
};
LdTab ld_layout(uint8_t *base, size_t at, size_t n_words, size_t n_slots);
// after the wait: the records with first_part set and the compacted parts from the host side of the layout (null: not copied); false
// where a word's parts lie outside its slots
bool ld_compact(const LdTab &H, const std::vector<int32_t> &slot, uint64_t n_slots, str_er_lattice_decode *dec, str_er_split_part *parts, uint64_t *n_parts);
// ---- defined in api_line_lattice.cpp
// the layout of c->ll_tab from byte `at` on (the inputs' bytes) for n_lines lines over n_runs runs of n_slots atoms: what goes up (the
// gap costs and the lines' first run, run count and node slot) and what k_line_lattice_decode leaves, all of which comes down
struct LlTab {
    uint8_t *gaps; int32_t *first, *n_of, *slot; str_er_line_lattice_decode *dec; uint8_t *chars; uint16_t *src; str_er_split_part *parts; int32_t *word_of_part;
    size_t o_up, up_bytes;                // gaps | first | n_of | slot lie back to back: one copy up
    size_t o_dec, down_bytes, bytes;      // dec | chars | src | parts | word_of_part lie back to back (each aligned): one copy down
};
LlTab ll_layout(uint8_t *base, size_t at, size_t n_runs, size_t n_lines, size_t n_slots);
// k_line_lattice_decode behind what is on s: the gap costs and the windows (host arrays) into c->ll_tab from byte `at` on and up, the
// back-pointer table sized, the outputs preset with bytes of 0xFF, the launch on the device's split records and rows; H and D receive
// the two sides of the layout (what comes down: H.o_dec, H.down_bytes)
int line_lattice_enqueue(str_er_ctx *c, hipStream_t s, size_t at, const str_er_run_split *d_splits, const uint8_t *d_run_costs, const uint8_t *d_piece_costs, size_t n_runs,
                         const uint8_t *gaps, const int32_t *first, const int32_t *n_of, const int32_t *slot, size_t n_lines, size_t n_slots, LlTab &H, LlTab &D);
// after the wait: the records with first_part set, the parts and their words compacted from the lines' slots (null: not copied); false
// where a line's parts lie outside its slots
bool ll_compact(const str_er_line_lattice_decode *from, const str_er_split_part *from_parts, const int32_t *from_wop, const int32_t *slot, const int32_t *slot_end, size_t n_lines,
                str_er_line_lattice_decode *dec, str_er_split_part *parts, int32_t *word_of_part, uint64_t *n_parts);
// ---- defined in api_lattice_match.cpp
// the layout of what k_lattice_match and k_lattice_match_final leave in c->lm_tab from byte `at` on (the inputs' bytes): the chunk keys
// of n_words words, and what comes down: their records and sources and n_slots part slots
struct LmTab {
    uint64_t *partial; str_er_lattice_match *matches; uint8_t *src; str_er_split_part *parts;
    size_t o_matches, down_bytes, bytes;      // matches | src | parts lie back to back (each aligned): one copy down
};
LmTab lm_layout(uint8_t *base, size_t at, size_t n_words, size_t n_slots, int n_chunks);
// after the wait: the records with first_part set and the compacted parts from the host side of the layout (null: not copied); false
// where a word's parts lie outside its slots
bool lm_compact(const LmTab &H, const std::vector<int32_t> &slot, uint64_t n_slots, str_er_lattice_match *matches, str_er_split_part *parts, uint64_t *n_parts);
// ---- defined in api_lattice_track.cpp
// the layout of c->lt_tab from byte `at` on (the inputs' bytes) for n_tracks tracks over a member array of n_members with n_pslots part
// slots: what goes up (the tracks, the members, the track and the part slot of every member slot), the structure of the n_words words
// and the chunk keys, and what comes down: the records, the member records, the sources and the parts; the free costs stay on the device
struct LtTab {
    int32_t *first, *count, *members, *slot_track, *pslot, *tab; uint64_t *partial; str_er_track_match *matches; str_er_lattice_track_member *mrec;
    uint8_t *src; str_er_split_part *parts; int32_t *mfree;
    size_t o_up, up_bytes;                    // first | count | members | slot_track | pslot lie back to back: one copy up
    size_t o_matches, down_bytes, bytes;      // matches | mrec | src | parts lie back to back (each aligned): one copy down
};
LtTab lt_layout(uint8_t *base, size_t at, size_t n_words, size_t n_tracks, size_t n_members, size_t n_pslots, int n_chunks);
// The track tables into c->lt_tab (from byte `at` on) and up on s, the kernels behind what is on s.  d_*: on the device; splits,
// first_run, n_of: the same on the host, checked by the caller as the tracks are.  pslot receives the part slot of every member slot
// and *n_pslots their sum; H and D the two sides of the layout (what comes down: H.o_matches, H.down_bytes)
int lattice_track_enqueue(str_er_ctx *c, hipStream_t s, size_t at, const str_er_run_split *d_splits, const uint8_t *d_run_costs, const uint8_t *d_piece_costs,
                          const int32_t *d_first, const int32_t *d_n_of, const str_er_run_split *splits, const int32_t *first_run, const int32_t *n_of, size_t n_words,
                          const int32_t *track_first, const int32_t *track_count, const int32_t *members, size_t n_members, size_t n_tracks, std::vector<int32_t> &pslot,
                          uint64_t *n_pslots, LtTab &H, LtTab &D);
// after the wait: the member records with first_part set and the compacted parts from the host side of the layout (null: not copied);
// false where a slot's parts lie outside its part slots
bool lt_compact(const LtTab &H, const std::vector<int32_t> &pslot, uint64_t n_pslots, str_er_lattice_track_member *mrec, str_er_split_part *parts, uint64_t *n_parts);
// ---- defined in api_track_read.cpp
// the layout of c->tm_tab for n_tracks tracks over a member array of n_members (base: either side of the pair, or null for the size alone)
struct TmTab {
    int32_t *first, *count, *members; uint64_t *partial; str_er_track_match *matches; int32_t *member_cost;
    size_t up_bytes;        // first | count | members lie at the front: what goes up
    size_t o_matches, o_mcost, bytes;
};
TmTab tm_layout(uint8_t *base, size_t n_tracks, size_t n_members, int n_chunks);
// the track tables into c->tm_tab and up on s, the two kernels behind what is on s (rows, first, n_of: on the device), the member costs
// preset to -1; D receives the device side of the layout (matches and member_cost come down from there)
int track_match_enqueue(str_er_ctx *c, hipStream_t s, const uint8_t *d_rows, const int32_t *d_first, const int32_t *d_n_of, const int32_t *track_first,
                        const int32_t *track_count, const int32_t *members, size_t n_members, size_t n_tracks, TmTab &D);
// ---- defined in api_track_decode.cpp
// the layout of c->td_tab from byte `at` on (the inputs' bytes) for n_tracks tracks over a member array of n_members
struct TdTab {
    int32_t *first, *count, *members; str_er_track_decode *out; uint8_t *chars; int32_t *member_cost;
    size_t o_up, up_bytes;                // first | count | members lie back to back: one copy up
    size_t o_out, down_bytes, bytes;      // out | chars | member_cost lie back to back (each aligned): one copy down
};
TdTab td_layout(uint8_t *base, size_t at, size_t n_tracks, size_t n_members);
// the track tables into c->td_tab (from byte `at` on) and up on s, k_track_decode behind what is on s (rows, first, n_of and the
// decoder's records and labels for these rows: on the device), the member costs preset to -1; H and D receive the two sides of the
// layout (what comes down: H.o_out, H.down_bytes)
int track_decode_enqueue(str_er_ctx *c, hipStream_t s, size_t at, const uint8_t *d_rows, const int32_t *d_first, const int32_t *d_n_of, const void *d_dec,
                         const uint8_t *d_dchars, const int32_t *track_first, const int32_t *track_count, const int32_t *members, size_t n_members, size_t n_tracks,
                         TdTab &H, TdTab &D);
// ---- defined in api_lattice_track_decode.cpp
// the layout of c->ltd_tab from byte `at` on (the inputs' bytes) for n_tracks tracks over a member array of n_members with n_pslots part
// slots: what goes up (the tracks, the members, the track and the part slot of every member slot), the structure of the n_words words,
// and what comes down: the records, the labels, the member records, the sources and the parts
struct LtdTab {
    int32_t *first, *count, *members, *slot_track, *pslot, *tab; str_er_track_decode *out; uint8_t *chars; str_er_lattice_track_member *mrec;
    uint8_t *src; str_er_split_part *parts;
    size_t o_up, up_bytes;                // first | count | members | slot_track | pslot lie back to back: one copy up
    size_t o_out, down_bytes, bytes;      // out | chars | mrec | src | parts lie back to back (each aligned): one copy down
};
LtdTab ltd_layout(uint8_t *base, size_t at, size_t n_words, size_t n_tracks, size_t n_members, size_t n_pslots);
// The track tables into c->ltd_tab (from byte `at` on) and up on s, the kernels behind what is on s.  d_*: on the device (d_dec, d_dchars:
// the lattice decoder's records and labels for these rows); splits, first_run, n_of: the same on the host, checked by the caller as the
// tracks are (no track of more than 1024 members).  pslot receives the part slot of every member slot and *n_pslots their sum; H and D
// the two sides of the layout (what comes down: H.o_out, H.down_bytes)
int lattice_track_decode_enqueue(str_er_ctx *c, hipStream_t s, size_t at, const str_er_run_split *d_splits, const uint8_t *d_run_costs, const uint8_t *d_piece_costs,
                                 const int32_t *d_first, const int32_t *d_n_of, const void *d_dec, const uint8_t *d_dchars, const str_er_run_split *splits,
                                 const int32_t *first_run, const int32_t *n_of, size_t n_words, const int32_t *track_first, const int32_t *track_count,
                                 const int32_t *members, size_t n_members, size_t n_tracks, std::vector<int32_t> &pslot, uint64_t *n_pslots, LtdTab &H, LtdTab &D);
// after the wait: the member records with first_part set and the compacted parts from the host side of the layout (null: not copied);
// false where a slot's parts lie outside its part slots
bool ltd_compact(const LtdTab &H, const std::vector<int32_t> &pslot, uint64_t n_pslots, str_er_lattice_track_member *mrec, str_er_split_part *parts, uint64_t *n_parts);
// ---- defined in api_word_match.cpp
// the layout of what the matcher leaves in c->wm_tab from byte `at` on (the inputs' bytes) for n_words words: chunk keys | matches
struct WmTab {
    uint64_t *partial; str_er_word_match *matches;
    size_t o_matches, bytes;
};
WmTab wm_layout(uint8_t *base, size_t at, size_t n_words, int n_chunks);
// a lexicon's entries as labels (checked before: wm::lexicon_check)
std::vector<uint8_t> lexicon_labels(const char *bytes, const int32_t *offsets, int32_t n);
// ---- defined in api_word_decode.cpp
// the layout of what the decoder leaves in c->wd_tab in the same way, all of which comes down
struct WdTab {
    str_er_word_decode *dec; uint8_t *chars, *src;
    size_t o_dec, down_bytes, bytes;      // dec | chars | src lie back to back (each aligned): one copy down
};
WdTab wd_layout(uint8_t *base, size_t at, size_t n_words);
// ---- defined in api_line_decode.cpp
// the layout of c->ln_tab from byte `at` on (the inputs' bytes) for n_lines lines over n_rows rows: what goes up (the gap costs, and with
// windows the lines' first row and row count) and what k_line_decode leaves, all of which comes down
struct LnTab {
    uint8_t *gaps; int32_t *first, *n_of, *row_map; str_er_line_decode *dec; uint8_t *chars; uint16_t *src; int32_t *word_of_row;
    // with margin, what k_line_margin leaves behind them (marginals: null where they are not made)
    str_er_line_margin *margins; int32_t *row_margin, *gap_margin; uint8_t *row_read, *row_alt, *gap_move; int32_t *marginals;
    size_t o_up, up_bytes;                // gaps | first | n_of | row_map lie back to back: one copy up
    size_t o_dec, down_bytes, bytes;      // dec | chars | src | word_of_row | the margins' tables lie back to back (each aligned): one copy down
};
LnTab ln_layout(uint8_t *base, size_t at, size_t n_rows, size_t n_lines, bool windows, bool map, bool margin = false, bool marginals = false);
// k_line_decode behind what is on s: the gap costs (and with first / n_of the windows, else d_first / d_n_of are on the device already;
// with row_map the cost row of every row, else row r is cost row r) into c->ln_tab from byte `at` on and up, the back-pointer table sized, the outputs preset for the rows of no line, the launch; H and D
// receive the two sides of the layout (what comes down: H.o_dec, H.down_bytes)
int line_decode_enqueue(str_er_ctx *c, hipStream_t s, size_t at, const uint8_t *d_rows, size_t n_rows, const uint8_t *gaps, const int32_t *first, const int32_t *n_of,
                        const int32_t *d_first, const int32_t *d_n_of, size_t n_lines, const int32_t *row_map, LnTab &H, LnTab &D, bool margin = false, bool marginals = false);
// (margin: k_line_margin behind it on the same rows, its forward table sized and its tables behind the decoder's in the same layout)
// ---- defined in api_lattice_margin.cpp
// the layout of what k_lattice_margin leaves in c->lg_tab from byte `at` on (the inputs' bytes), all of which comes down
struct LgTab {
    str_er_lattice_margin *margins; int32_t *read_margin, *cut_margin; uint8_t *read, *alt, *cut_alt; int32_t *edge_min, *marginals;      // the last two: null where they are not made
    size_t o_out, down_bytes, bytes;      // the tables lie back to back in that order (each aligned): one copy down
};
LgTab lg_layout(uint8_t *base, size_t at, size_t n_words, bool edge_min, bool marginals);
// ---- defined in api_word_margin.cpp
// the layout of what k_word_margin leaves in c->wg_tab from byte `at` on (the inputs' bytes), all of which comes down
struct WgTab {
    str_er_word_margin *margins; int32_t *row_margin; uint8_t *row_read, *row_alt; int32_t *marginals;      // marginals: null where they are not made
    size_t o_out, down_bytes, bytes;      // margins | row_margin | row_read | row_alt | marginals lie back to back (each aligned): one copy down
};
WgTab wg_layout(uint8_t *base, size_t at, size_t n_words, bool marginals);
// ---- defined in words_host.cpp and lines_host.cpp (HIP-free)
bool word_gap_ok(int32_t num, int32_t den);       // what str_er_set_word_gap takes
// inter * den >= num * (pa + pb - inter): footprints of pa and pb pixels, inter of them common, are duplicates (links) at num / den
bool overlap_passes(uint32_t inter, uint32_t pa, uint32_t pb, int32_t num, int32_t den);
// the geometry of frame lines: the hull of the union of the members' hull vertices (appended to points), the moments of the representative
int frame_line_geoms(const str_er_frame_line *frame_lines, size_t n_frame_lines, const int32_t *members, const str_er_line_geom *line_geoms,
                     std::vector<int32_t> &points, std::vector<str_er_line_geom> &out);
constexpr int MASK_MAX_WIDTH = 16384;       // widest box the mask kernels take (er_masks.inl: MASK_MAX_WPL words of 64 pixels per lane)
// ---- defined in api_models.cpp
int parse_cascade(str_er_ctx *c, HostCascade &hc, const char *text, size_t len);
} // namespace str_er_host

// =================================================================================================
// C ABI
// =================================================================================================
// Nothing is thrown across the C ABI: every entry point that takes a context is a function-try-block (the std::vector / std::string work behind
// them -- parsers of untrusted bytes, per-batch tables -- can run out of memory).
static int abi_caught(str_er_ctx *c, int code, const char *what)
{
    if (!c) return code;
    try { c->err = what; } catch (...) { }
    return code;
}
#define ABI_GUARD(ctx)                                                                                   \
    catch (const std::bad_alloc &) { return abi_caught((ctx), STR_ER_ENOMEM, "out of host memory"); }      \
    catch (const std::length_error &) { return abi_caught((ctx), STR_ER_ENOMEM, "out of host memory (container size)"); } \
    catch (...) { return abi_caught((ctx), STR_ER_EHIP, "internal error (exception)"); }
