/*
 * str_er.h -- C ABI of libstr_er_hip.so: the MI355X (gfx950) implementation of the
 * extremal-region scene-text detection hot path of HsiehYiChia/Scene-text-recognition.
 *
 * The boundary is the public surface of the reference's `class ERFilter`
 * (inc/ER.h:110-136) for the per-plane hot loop of ERFilter::text_detect
 * (src/ER.cpp:42-60):
 *
 *     compute_channels -> er_tree_extract -> non_maximum_supression -> classify
 *
 * and, behind further stage flags, what text_detect does with the classified ERs (src/ER.cpp:62-72): calc_color + er_track,
 * er_grouping, the chain-code / SVM scoring of er_ocr; plus a frame-ingest stream (str_er_stream_*).
 *
 * Plain pointers and sizes only; no C++/torch types cross this header.  Every entry
 * point returns 0 (STR_ER_OK) or a negative STR_ER_E* code and never throws.  All
 * per-pixel work runs in hand-written HIP kernels; there is no CPU fallback -- if no
 * gfx950 device is usable, str_er_create fails with STR_ER_EHIP.
 *
 * Paths below are relative to the reference checkout (/root/reference).
 */
#ifndef STR_ER_H
#define STR_ER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: str_er_params::sibling_order 0 means the reference's exact flood order (it was the largest-key rule, now 2);
 *    the library no longer edits the process environment when it is loaded (str_er_runtime_hint).                  */
#define STR_ER_ABI_VERSION 2

/* ---- error codes (reference: loaders print+return false, src/adaboost.cpp:877-881;
 *      CV_Assert throws on non-8UC1, src/ER.cpp:242) ------------------------------ */
#define STR_ER_OK          0
#define STR_ER_EINVAL     (-1)  /* bad argument (NULL, non-positive size, bad mask ...)    */
#define STR_ER_ENOMEM     (-2)  /* host or device allocation failed                         */
#define STR_ER_EHIP       (-3)  /* HIP runtime error / no usable device / kernel failure    */
#define STR_ER_EIO        (-4)  /* classifier file could not be opened                      */
#define STR_ER_EFORMAT    (-5)  /* classifier text could not be parsed                      */
#define STR_ER_ESTATE     (-6)  /* call needs cascades that are not loaded                  */
#define STR_ER_ECAPACITY  (-7)  /* input exceeds the capacity the context was created with  */

/* which cascade: ERFilter::stc / ERFilter::wtc (inc/ER.h:117-118) */
#define STR_ER_CASCADE_STRONG 0
#define STR_ER_CASCADE_WEAK   1

/* where an input buffer lives */
#define STR_ER_MEM_HOST   0
#define STR_ER_MEM_DEVICE 1     /* pointer is HIP device memory on params.device */

/* stage mask for str_er_detect_* (each stage needs the previous ones) */
#define STR_ER_STAGE_EXTRACT  1u   /* er_tree_extract          src/ER.cpp:240-374 */
#define STR_ER_STAGE_NMS      2u   /* non_maximum_supression   src/ER.cpp:416-505 */
#define STR_ER_STAGE_CLASSIFY 4u   /* classify                 src/ER.cpp:507-528 */
#define STR_ER_STAGE_ALL      7u
#define STR_ER_STAGE_OCR      8u   /* config 3: OCR::chain_run (slope 0) on every strong/weak ER; needs an SVM model */
/* output option */
#define STR_ER_WANT_NODES     16u  /* also return the kept-node table of every plane */
/* the rest of text_detect (src/ER.cpp:62-72), BGR frames only */
#define STR_ER_STAGE_TRACK    32u  /* calc_color + ERFilter::er_track on the strong/weak ERs of every image (src/ER.cpp:530-590) */
#define STR_ER_STAGE_GROUP    64u  /* ERFilter::er_grouping(tracked, text, false, false) (src/ER.cpp:612-692); needs STR_ER_STAGE_TRACK */
#define STR_ER_GROUP_INNER_SUP 128u /* ... with inner_sup = true, as text_detect calls it when DO_OCR is defined (src/ER.cpp:69) */
#define STR_ER_GROUP_OVERLAP_SUP 512u /* ... with overlap_sup = true, as video_mode calls it (er_grouping(tracked, text, true, true), src/utils.cpp:196) */
#define STR_ER_STAGE_OCR_LINES 256u /* er_ocr's per-line scoring (src/ER.cpp:695-747): chain_run with the line's slope on every member;
                                      needs STR_ER_STAGE_GROUP + an SVM model */
/* output option: also return the pixel mask of every candidate (str_er_result_masks / str_er_result_mask_bits).  Every
 * str_er_detect_* entry point and every str_er_stream_submit* call honours it; str_er_strip_merge[_ex] rejects it (STR_ER_EINVAL). */
#define STR_ER_WANT_MASKS     1024u
/* output options: a recogniser-ready image of every text line of str_er_result_texts() (str_er_result_line_crops): a grey crop
 * (_CROPS) and, with _GLYPHS as well, a glyph crop made from the member masks.  Both need STR_ER_STAGE_GROUP, _GLYPHS needs _CROPS
 * (STR_ER_EINVAL otherwise); str_er_strip_merge[_ex] rejects both.  Every str_er_detect_* entry point and str_er_stream_submit* call
 * that can group honours them; the geometry and the sampling rules are at str_er_line_crop.                                       */
#define STR_ER_WANT_LINE_CROPS  2048u
#define STR_ER_WANT_LINE_GLYPHS 4096u
/* output option: also return the shape and intensity descriptors of every candidate (str_er_result_shapes, str_er_shape), made on
 * the device from the candidate's mask; the mask words are returned only with STR_ER_WANT_MASKS as well (the masks are made once).
 * Every str_er_detect_* entry point and every str_er_stream_submit* call honours it; str_er_strip_merge[_ex] rejects it (STR_ER_EINVAL);
 * a candidate wider than 16384 pixels gives STR_ER_ECAPACITY.                                                                      */
#define STR_ER_WANT_SHAPES    (8192u)
/* output option: also return the stroke-width descriptor of every candidate (str_er_result_strokes, str_er_stroke), made on the device
 * from the candidate's mask like STR_ER_WANT_SHAPES: the mask words are returned only with STR_ER_WANT_MASKS as well, and the masks are
 * made once per call whatever combination of masks, shapes, strokes, glyphs and maps is asked for.  Every str_er_detect_* entry point
 * and every str_er_stream_submit* call honours it; str_er_strip_merge[_ex] rejects it (STR_ER_EINVAL); a candidate wider than 16384
 * pixels gives STR_ER_ECAPACITY.  It changes no other output of the call.                                                           */
#define STR_ER_WANT_STROKES   (65536u)
/* output options: frame-resolution maps of where the detected text is (str_er_result_frame_maps, str_er_frame_map).
 * _TEXT_MAP: one uint8 map per frame, at the frame's own (level-0) size, bits STR_ER_TEXT_MAP_* of every region that covers the
 * pixel; needs STR_ER_STAGE_CLASSIFY.  _LINE_MAP: one int32 map per frame, the smallest index into str_er_result_texts() of a line
 * with a member that covers the pixel, -1 where none does; needs STR_ER_STAGE_GROUP.  STR_ER_EINVAL otherwise, the context usable.
 * The two are independent of each other and of the other output options.  str_er_detect_bgr, _nv12, _bgr_list, _nv12_list,
 * _bgr_planes (the selected planes contribute) and every str_er_stream_submit* call honour them; str_er_detect_planes[_list] and
 * str_er_strip_merge[_ex] have no frames and reject them (STR_ER_EINVAL).  A contributing candidate wider than 16384 pixels gives
 * STR_ER_ECAPACITY.  The pixel rule and the layout are at str_er_frame_map.                                                      */
#define STR_ER_WANT_TEXT_MAP  (16384u)   /* one uint8 map per frame, at the frame's own size          */
#define STR_ER_WANT_LINE_MAP  (32768u)   /* one int32 map per frame: the text line of every pixel     */
/* output option: one list of text lines per frame, in frame pixels, the lines of different pyramid levels that are the same text
 * joined (str_er_result_line_feet / _line_pairs / _frame_lines / _frame_line_members; the contract is at str_er_line_foot).  Needs
 * STR_ER_STAGE_GROUP and frames: STR_ER_EINVAL without the stage, on str_er_detect_planes[_list] and on str_er_strip_merge[_ex], the
 * context usable afterwards.  str_er_detect_bgr, _nv12, _bgr_list, _nv12_list and every str_er_stream_submit* call honour it.  A
 * contributing candidate wider than 16384 pixels gives STR_ER_ECAPACITY.  It changes no other output of the call and combines with
 * every other STR_ER_WANT_* flag; the masks are still made once per call.                                                        */
#define STR_ER_WANT_FRAME_LINES (131072u)
/* output option: link the text lines of consecutive frames of the call into text tracks (str_er_result_line_links / _line_tracks /
 * _text_tracks / _text_track_members / _edge_feet; the contract is at str_er_line_link).  Needs STR_ER_WANT_FRAME_LINES (which needs
 * STR_ER_STAGE_GROUP and frames): STR_ER_EINVAL without it, and wherever _FRAME_LINES is refused (str_er_detect_planes[_list],
 * str_er_strip_merge[_ex]), the context usable afterwards.  str_er_detect_bgr, _nv12, _bgr_list, _nv12_list and every
 * str_er_stream_submit* call honour it.  It changes no other output of the call.                                                  */
#define STR_ER_WANT_LINE_LINKS (262144u)
/* output option: the convex hull, the moments and the oriented box of every text line and of every frame line, from the footprints
 * (str_er_result_line_geoms / _frame_line_geoms / _geom_points; the contract is at str_er_line_geom).  Needs STR_ER_WANT_FRAME_LINES
 * (which needs STR_ER_STAGE_GROUP and frames): STR_ER_EINVAL without it, and wherever _FRAME_LINES is refused
 * (str_er_detect_planes[_list], str_er_strip_merge[_ex]), the context usable afterwards.  str_er_detect_bgr, _nv12, _bgr_list,
 * _nv12_list and every str_er_stream_submit* call honour it.  A foot box wider or taller than 16384 pixels gives STR_ER_ECAPACITY.
 * It changes no other output of the call and combines with every other STR_ER_WANT_* flag.                                      */
#define STR_ER_WANT_LINE_GEOM (524288u)
/* output option: every text line split into glyph runs and words, from the footprints (str_er_result_line_words / _line_runs / _words;
 * the contract is at str_er_line_run; the gap that breaks a word: str_er_set_word_gap).  Needs STR_ER_WANT_FRAME_LINES (which needs
 * STR_ER_STAGE_GROUP and frames): STR_ER_EINVAL without it, and wherever _FRAME_LINES is refused (str_er_detect_planes[_list],
 * str_er_strip_merge[_ex]), the context usable afterwards.  str_er_detect_bgr, _nv12, _bgr_list, _nv12_list and every
 * str_er_stream_submit* call honour it.  A footprint wider or taller than 16384 pixels gives STR_ER_ECAPACITY.  It changes no other
 * output of the call and combines with every other STR_ER_WANT_* flag.                                                             */
#define STR_ER_WANT_LINE_WORDS (1048576u)
/* output option: every glyph run of STR_ER_WANT_LINE_WORDS read by the OCR scorer: a label, a character and a probability per run
 * (str_er_result_run_reads / _run_features; the contract is at str_er_run_read).  Needs STR_ER_WANT_LINE_WORDS: STR_ER_EINVAL without it
 * and wherever that flag is refused, and an SVM model of dim 1800 (str_er_load_svm_model): STR_ER_ESTATE without one; the context is
 * usable afterwards.  It does not need STR_ER_STAGE_OCR_LINES.  Every call that honours _LINE_WORDS honours it.  It changes no other
 * output of the call and combines with every other STR_ER_WANT_* flag.                                                             */
#define STR_ER_WANT_RUN_READ (2097152u)
/* output option: every word of STR_ER_WANT_RUN_READ matched against the lexicon of str_er_set_lexicon: the best and the second-best
 * entry per word (str_er_result_word_matches), the cost row of every run (str_er_result_run_costs) and its class probabilities
 * (str_er_result_run_probs); the contract is at str_er_word_match.  Needs STR_ER_WANT_RUN_READ: STR_ER_EINVAL without it and wherever
 * that flag is refused, and a lexicon: STR_ER_ESTATE without one; the context is usable afterwards.  Every call that honours
 * _RUN_READ honours it.  It changes no other output of the call and combines with every other STR_ER_WANT_* flag.                  */
#define STR_ER_WANT_WORD_MATCH (4194304u)
/* output option: every word of STR_ER_WANT_RUN_READ decoded under the bigram table of str_er_set_bigram: the cheapest character string
 * per word with the run every character came from (str_er_result_word_decodes / _word_decode_chars / _word_decode_src); the cost rows
 * and class probabilities of the runs come with it (str_er_result_run_costs / _run_probs); the contract is at str_er_word_decode.
 * Needs STR_ER_WANT_RUN_READ: STR_ER_EINVAL without it and wherever that flag is refused, and a table: STR_ER_ESTATE without one; the
 * context is usable afterwards.  It needs no lexicon.  Every call that honours _RUN_READ honours it.  It changes no other output of
 * the call and combines with every other STR_ER_WANT_* flag; beside STR_ER_WANT_WORD_MATCH the run costs stay the matcher's.        */
#define STR_ER_WANT_WORD_DECODE (8388608u)
/* output option: every glyph run of STR_ER_WANT_RUN_READ cut at the valleys of its column profile, every piece read, and per run the
 * segmentation the scorer likes best (str_er_result_run_splits / _run_pieces / _piece_reads / _piece_costs / _split_parts /
 * _word_splits; the contract is at str_er_run_split, the parameters: str_er_set_run_split).  Needs STR_ER_WANT_RUN_READ: STR_ER_EINVAL
 * without it and wherever that flag is refused; its parameters have defaults, so it needs no further state.  Every call that honours
 * _RUN_READ honours it.  Beside STR_ER_WANT_WORD_MATCH / _WORD_DECODE both work on the split sequence of a word instead of its runs.
 * It changes no other output of the call -- the runs' own reads are byte for byte those of a call without it -- and combines with
 * every other STR_ER_WANT_* flag.                                                                                                   */
#define STR_ER_WANT_RUN_SPLIT (16777216u)
/* output option: the words of adjacent frames linked into word tracks, and per word track one lexicon match over the cost rows of
 * all its members (str_er_result_word_links / _word_tracks / _word_track_members / _word_track_of_words / _track_matches /
 * _track_member_costs; the contract is at str_er_word_link).  Needs STR_ER_WANT_LINE_LINKS and STR_ER_WANT_WORD_MATCH: STR_ER_EINVAL
 * without either and wherever either is refused (the strip path, the per-plane calls), and through them a model and a lexicon:
 * STR_ER_ESTATE without; the context is usable afterwards.  Beside STR_ER_WANT_RUN_SPLIT the members' rows are those of their parts.
 * It changes no other output of the call and combines with every other STR_ER_WANT_* flag.                                          */
#define STR_ER_WANT_TRACK_READ (33554432u)
/* output option: every word of STR_ER_WANT_RUN_SPLIT decoded jointly over the lattice of all pieces of all its runs under the bigram table
 * of str_er_set_bigram: segmentation and string come out together (str_er_result_lattice_decodes / _lattice_decode_chars /
 * _lattice_decode_src / _lattice_parts; the contract is at str_er_lattice_decode).  Needs STR_ER_WANT_RUN_SPLIT (and through it
 * STR_ER_WANT_RUN_READ): STR_ER_EINVAL without it and wherever that flag is refused (the strip path, the per-plane calls), and a table:
 * STR_ER_ESTATE without one; the context is usable afterwards.  It needs no lexicon and is independent of STR_ER_WANT_WORD_DECODE and
 * _WORD_MATCH.  Every call that honours _RUN_SPLIT honours it.  It changes no other output of the call and combines with every other
 * STR_ER_WANT_* flag.                                                                                                               */
#define STR_ER_WANT_LATTICE_DECODE (67108864u)
/* output option: every word of STR_ER_WANT_RUN_SPLIT matched against the lexicon of str_er_set_lexicon with the segmentation of its runs
 * free: the best and the second-best entry over the lattice of all pieces of all its runs, and for the best its segmentation and its
 * alignment (str_er_result_lattice_matches / _lattice_match_src / _lattice_match_parts; the contract is at str_er_lattice_match).  Needs
 * STR_ER_WANT_RUN_SPLIT and STR_ER_WANT_WORD_MATCH (and through them STR_ER_WANT_RUN_READ): STR_ER_EINVAL without either and wherever
 * they are refused (the strip path, the per-plane calls), and a lexicon: STR_ER_ESTATE without one (the matcher's rule); the context
 * is usable afterwards.  It needs no bigram table.  It changes no other output of the call -- str_er_result_word_matches still reads the
 * split sequence -- and combines with every other STR_ER_WANT_* flag.                                                               */
#define STR_ER_WANT_LATTICE_MATCH (134217728u)
/* output option: every word track of STR_ER_WANT_TRACK_READ matched against the lexicon over the piece lattices of all its members: the
 * pooled evidence of the track chooses the entry, and for that entry every member gets its own segmentation and alignment
 * (str_er_result_lattice_track_matches / _lattice_track_members / _lattice_track_src / _lattice_track_parts; the contract is at
 * str_er_lattice_track_member).  Needs STR_ER_WANT_TRACK_READ and STR_ER_WANT_LATTICE_MATCH (and through them STR_ER_WANT_RUN_SPLIT,
 * _WORD_MATCH, _LINE_LINKS and _RUN_READ): STR_ER_EINVAL without either and wherever they are refused (the strip path, the per-plane
 * calls), and a lexicon: STR_ER_ESTATE without one (the matcher's rule); the context is usable afterwards.  It changes no other output
 * of the call -- str_er_result_track_matches still reads the split sequence -- and combines with every other STR_ER_WANT_* flag.     */
#define STR_ER_WANT_LATTICE_TRACK (268435456u)
/* output option: every word track decoded without a lexicon: the median string of its members under the bigram table of
 * str_er_set_bigram, found from the members' own decoder strings by single edits (str_er_result_track_decodes / _track_decode_chars /
 * _track_decode_member_costs, and the word links and word tracks of str_er_word_link: str_er_result_word_links / _word_tracks /
 * _word_track_members / _word_track_of_words; the contract is at str_er_track_decode, the parameters: str_er_set_track_decode).  Needs
 * STR_ER_WANT_LINE_LINKS and STR_ER_WANT_WORD_DECODE (and through the latter STR_ER_WANT_RUN_READ): STR_ER_EINVAL without either and
 * wherever either is refused (the strip path, the per-plane calls), and a table: STR_ER_ESTATE without one; the context is usable
 * afterwards.  It needs neither STR_ER_WANT_WORD_MATCH nor a lexicon.  Beside STR_ER_WANT_RUN_SPLIT the members' rows are those of
 * their parts.  It changes no other output of the call and combines with every other STR_ER_WANT_* flag.                            */
#define STR_ER_WANT_TRACK_DECODE (536870912u)
/* the bits of a STR_ER_WANT_TEXT_MAP pixel: the OR over every region that covers it */
#define STR_ER_TEXT_MAP_STRONG 1u   /* a strong candidate (cls == STR_ER_CLS_STRONG)                                              */
#define STR_ER_TEXT_MAP_WEAK   2u   /* a weak candidate                                                                            */
#define STR_ER_TEXT_MAP_LINE   4u   /* a member of a line of str_er_result_texts() (STR_ER_STAGE_GROUP; never set without it)      */
#define STR_ER_TEXT_MAP_OCR    8u   /* a member kept by STR_ER_STAGE_OCR_LINES (line_kept = 1) in a line with text_alive = 1,
                                       for any of its occurrences (never set without the stage)                                   */

/* candidate class: which list of text_detect() the ER landed in (src/ER.cpp:516-526) */
#define STR_ER_CLS_POOL   0   /* pooled by NMS, rejected by both cascades */
#define STR_ER_CLS_STRONG 1
#define STR_ER_CLS_WEAK   2

typedef struct str_er_ctx    str_er_ctx;
typedef struct str_er_result str_er_result;

/* Constructor arguments of ERFilter (inc/ER.h:113, src/main.cpp:22, macros
 * inc/utils.h:6-11) plus the build's own batching/pyramid/capacity knobs.          */
typedef struct str_er_params {
    int32_t  thresh_step;     /* THRESH_STEP   default 8                              */
    int32_t  min_area;        /* MIN_AREA      default 120                            */
    int32_t  max_area;        /* MAX_AREA      default 900000                         */
    int32_t  stability_t;     /* STABILITY_T   default 2                              */
    double   overlap_coef;    /* OVERLAP_COEF  default 0.7                            */
    int32_t  n_pyr_levels;    /* 1 = native resolution only (the reference);
                                 level k>=1 of Y/Cr/Cb is resize_linear(level k-1)
                                 to (lround(w*2^(-k/2)), lround(h*2^(-k/2)));
                                 inverted channels are 255 - that level               */
    uint32_t channel_mask;    /* bit i = plane i of [Y,Cr,Cb,255-Y,255-Cr,255-Cb]
                                 (src/ER.cpp:122-127); 0x3F = the reference           */
    int32_t  device;          /* HIP device ordinal                                   */
    int32_t  max_width;       /* capacity: largest frame / plane width                */
    int32_t  max_height;      /* capacity: largest frame / plane height               */
    int32_t  max_frames;      /* capacity: frames per str_er_detect_bgr call; the
                                 per-plane entry points accept up to
                                 max_frames * popcount(channel_mask) * n_pyr_levels   */
    int32_t  kept_cap;        /* per-plane capacity of the kept-node table.  0 (both
                                 this and pool_cap) = by the plane's size: padded
                                 pixels / 64 + 512, at most max(4096, w*h/64)         */
    int32_t  pool_cap;        /* per-plane capacity of the NMS pool, 0 = kept_cap/4
                                 (at least 256); a plane that needs more fails with
                                 STR_ER_ECAPACITY, the message names the plane        */
    int32_t  sibling_order;   /* what decides NMS where two or more child chains
                                 compete for a parent:
                                 0 = the reference's own order -- the child whose
                                     basin its flood entered last, src/ER.cpp:183-185,
                                     416-462; found by replaying the flood on the GPU
                                     for the planes that have such a tie (exact);
                                 1 = child with the smallest key, 2 = largest key
                                     (canonical rules, no replay; the plane is only
                                     flagged through str_er_plane_info::ambiguous)    */
    void    *stream;          /* hipStream_t to enqueue on; NULL = private stream     */
} str_er_params;

/* One kept node of a plane's component tree: flat form of struct ER (inc/ER.h:42-80). */
typedef struct str_er_node {
    uint32_t key;        /* canonical id: min linear pixel index (y*w+x) over the pixels
                            of level == `level` inside the component                   */
    int32_t  parent;     /* index in this plane's node table; the root points to itself
                            (non_maximum_supression sets root->parent=root, :424)      */
    int32_t  area;       /* ER::area as the reference computes it: pixel count +
                            number of tree nodes in the subtree (ctor starts at 1)     */
    uint16_t x, y, w, h; /* ER::bound                                                  */
    uint8_t  level;      /* ER::level (quantised grey level)                           */
    uint8_t  flags;      /* bit0: root                                                 */
    uint16_t reserved;
} str_er_node;           /* 24 bytes */

/* One NMS survivor (member of `pool`, and of `strong`/`weak` if cls says so). */
typedef struct str_er_cand {
    uint32_t frame;      /* frame index inside the call (0 for the per-plane calls)    */
    uint8_t  ch;         /* plane index 0..5 as in src/ER.cpp:122-127 (ER::ch)         */
    uint8_t  pyr;        /* pyramid level                                              */
    uint8_t  level;      /* ER::level                                                  */
    uint8_t  cls;        /* STR_ER_CLS_*                                               */
    uint16_t x, y, w, h; /* ER::bound in the plane's own coordinates                   */
    uint32_t area;       /* ER::area (reference semantics)                             */
    uint32_t key;        /* canonical id, see str_er_node                              */
    int32_t  node;       /* index in the plane's kept-node table                       */
    uint32_t plane;      /* plane index inside the result                              */
    double   score_strong; /* stc->predict(fv): last stage score or -DBL_MAX           */
    double   score_weak;   /* wtc->predict(fv) if the strong cascade rejected, else 0  */
} str_er_cand;           /* 48 bytes */

/* The pixel mask of one region (STR_ER_WANT_MASKS, str_er_er_masks).  With L(p) = rint_half_even(P'(p) / thresh_step), P' the plane
 * XOR its invert mask (the quantiser of the tile trees), the mask of a region c is the set of pixels reachable from pixel `key`
 * (x = key % plane width, y = key / plane width) through 4-neighbours with L <= c.level, without leaving the box (c.x, c.y, c.w, c.h).
 * For a candidate the box is the region's bounding box, so the mask is the whole node (t, C) of SURVEY A.3: its bounding box is
 * the candidate's box and its popcount is |C| (the own pixels of the node and of all its descendants).
 * Layout: h rows of pitch_words = (w + 31) / 32 32-bit words, from word word_off of str_er_result_mask_bits() on; pixel x of a row
 * is bit (x & 31) of word (x >> 5); padding bits are 0.  pixels = popcount.                                                        */
typedef struct str_er_mask {
    uint64_t word_off;
    uint32_t pixels;
    uint32_t pitch_words;
} str_er_mask;           /* 16 bytes */

/* The descriptors of one region (STR_ER_WANT_SHAPES, str_er_er_shapes): the Neumann-Matas features of cv::text::ERStat, all exact
 * integers, defined on the region's mask M (str_er_mask) over its box of w x h pixels; pixels outside the box count as outside M.
 * P' is the plane the mask was built on: the plane XOR its invert mask, at the candidate's pyramid level (for str_er_er_shapes the
 * host plane as given).  Layout: pixels 0, perimeter 4, euler 8, hole_pixels 12, crossings 16, hull_area2 24, grey_sum 32,
 * grey_sum2 40.  How each is computed, one wave per mask, in the epilogue of the mask kernels:
 *   perimeter    4|M| - 2 (horizontal + vertical pairs of 4-adjacent pixels of M), from popcounts of the bit rows;
 *   euler        |M| - pairs + 2x2 blocks of M (vertices - edges + faces of the 4-adjacency graph: Gray's bit-quad count
 *                (Q1 - Q3 + 2 QD) / 4 over the 2x2 windows of the box padded by one ring of zeros);
 *   hole_pixels  the complement of M in the box, flooded to a fixpoint through 8-neighbours from its pixels on the box border
 *                (no iteration cap): what the flood does not reach;
 *   crossings    2 x the runs of the row;
 *   hull_area2   monotone chains over the leftmost and rightmost pixel of every row (they determine the hull);
 *   grey_sum(2)  a second read of P' under M.                                                                                   */
typedef struct str_er_shape {
    uint32_t pixels;        /* |M| (== str_er_mask.pixels == the node's |C|)                                                        */
    uint32_t perimeter;     /* unit edges between a pixel of M and a 4-neighbour not in M (hole borders included)                     */
    int32_t  euler;         /* 4-connected components of M minus holes; a hole = an 8-connected component of the complement
                               that does not reach outside the box.  M is one 4-component, so holes = 1 - euler                       */
    uint32_t hole_pixels;   /* pixels of the box not in M with no 8-connected path of non-M pixels to outside the box                  */
    uint16_t crossings[4];  /* [k] for rows y = floor(j*h/6), j = 1, 3, 5: x in [0, w] with M(x-1, y) != M(x, y)
                               (= 2 x the runs of the row); [3] = the median of [0..2]                                                   */
    uint64_t hull_area2;    /* twice the area of the convex hull of the corners of M's pixel squares (an integer)                      */
    uint64_t grey_sum;      /* sum of P' over M                                                                                        */
    uint64_t grey_sum2;     /* sum of P'^2 over M                                                                                      */
} str_er_shape;             /* 48 bytes */

/* The stroke-width descriptor of one region (STR_ER_WANT_STROKES, str_er_er_strokes), exact integers, defined by this library (the
 * reference's StrokeWidth::SWT is compiled out): an octagonal erosion depth over the region's mask M (str_er_mask) in its box of w x h
 * pixels; pixels outside the box are in no set below.
 *   E_0 = M; E_k = { p in E_{k-1} : every neighbour of p in N_k lies in E_{k-1} }, N_k the 4-neighbourhood for odd k and the
 *   8-neighbourhood for even k.  K = the smallest k with E_k empty (K >= 1: M holds the key pixel).
 *   Depth D(p) = k for p in E_{k-1} \ E_k: 1 <= D(p) <= K on M (D = 0 off M).
 *   Ridge = the p in M whose 8 neighbours all have D <= D(p): the local maxima of D, plateaus included.  As bit rows, the ridge at
 *   depth k is (E_{k-1} & ~E_k) & ~dilate8(E_k).
 * The mean ridge depth m = ridge_depth_sum / ridge_pixels estimates the stroke width: a stroke t pixels wide has depth ceil(t/2), so
 * t = 2m - 1 for odd widths and 2m for even ones; ridge_depth_sum2 / ridge_pixels - m^2 is its spread (0 for a stroke of one width).
 * Closed forms: an axis-parallel bar of t x L pixels that fills its box has ridge depth ceil(t/2) along its whole ridge -- for odd t
 * a ridge one pixel wide that stops (t - 1)/2 pixels short of each end, for even t two pixels wide, t/2 - 1 short of each end; an
 * n x n square has K = ceil(n/2), depth_sum = sum over k >= 0 with n - 2k > 0 of (n - 2k)^2, and a ridge of 1 pixel (odd n) or 4
 * (even n); a single pixel gives {1, 1, 1, 1, 1}.
 * How it is computed, one wave per mask in the epilogue of the mask kernels: one pass over the rows a step, E_{k-1} and E_k as bit
 * rows, the step counting |E_k| and the ridge at depth k and making E_{k+1}; a step visits only the rows where E_{k-1} is
 * non-empty, and the last step is the first whose E_{k+1} is empty (no cap).  Layout: depth_max 0, ridge_pixels 4, depth_sum 8,
 * ridge_depth_sum 16, ridge_depth_sum2 24.                                                                                          */
typedef struct str_er_stroke {
    uint32_t depth_max;        /* K                                                                                                */
    uint32_t ridge_pixels;     /* |ridge|                                                                                          */
    uint64_t depth_sum;        /* sum of D over M = sum over k < K of |E_k|                                                        */
    uint64_t ridge_depth_sum;  /* sum of D over the ridge                                                                          */
    uint64_t ridge_depth_sum2; /* sum of D^2 over the ridge                                                                        */
} str_er_stroke;               /* 32 bytes */

/* The crop of one text line (STR_ER_WANT_LINE_CROPS, str_er_line_crops, str_er_line_crop_geometry).
 * Geometry, all f64 on the host in this order: s = the line's slope (non-finite counts as 0); r = sqrt(1 + s*s); d = (1, s) / r,
 * n = (-s, 1) / r.  The four corners of every box of the line (the members' str_er_result_group_bounds) project to u = c.d, v = c.n,
 * giving u0, u1, v0, v1.  p = pad * (v1 - v0); U0 = u0 - p, U1 = u1 + p, V0 = v0 - p, V1 = v1 + p; kv = (V1 - V0) / height;
 * width = min(max_width, max(1, ceil((U1 - U0) / kv))); ku = (U1 - U0) / width; a = U0*d + V0*n + 0.5*ku*d + 0.5*kv*n - (0.5, 0.5);
 * u = ku*d, v = kv*n.  ax .. vy = llround(65536 * value): 16.16 fixed point.
 * Grey pixel (i, j), int64: sx = ax + i*ux + j*vx, sy = ay + i*uy + j*vy; x0 = sx >> 16, fx = (sx >> 8) & 255 (y0, fy the same from
 * sy); the taps (x0 | x0+1, y0 | y0+1) clamped into the plane; top = P[ya][xa]*(256-fx) + P[ya][xb]*fx, bot the same on the lower row;
 * out = (top*(256-fy) + bot*fy + 32768) >> 16.  The plane is the Y plane of frame text.frame at pyramid level text.pyr (for NV12
 * input the luma plane, resized for pyr >= 1).
 * Glyph pixel (i, j): xn = (sx + 32768) >> 16, yn likewise; 255 if (xn, yn) lies in the plane and in the mask (STR_ER_WANT_MASKS,
 * over the candidate's own box) of at least one member of the line, else 0.
 * Layout: width x height bytes, row-major, pitch = width; crops back to back in line order, each from a multiple of 4 bytes on
 * (pix_off; the 0..3 bytes between two crops are 0).  The glyph crop of a line sits at the same pix_off of the glyph bytes.       */
typedef struct str_er_line_crop {
    uint64_t pix_off;
    int32_t  width, height;
    int32_t  ax, ay;
    int32_t  ux, uy, vx, vy;
} str_er_line_crop;      /* 40 bytes */

/* The maps of one frame (STR_ER_WANT_TEXT_MAP / _LINE_MAP, str_er_result_frame_maps).
 * Pixel rule, exact integers: a region lies on a plane of level size (w_p, h_p) of a frame of level-0 size (W, H); frame pixel
 * (x, y) samples level pixel xs = ((2x + 1) * w_p) / (2W), ys = ((2y + 1) * h_p) / (2H), both rounded down (the nearest sample of
 * the pixel centre; the identity at level 0).  The region covers (x, y) if (xs, ys) lies in its box and in its mask (str_er_mask:
 * the same quantiser, the same 4-flood from key over the candidate's own box).  Every plane of the frame contributes (all channels,
 * inversions and pyramid levels; only the selected ones for str_er_detect_bgr_planes); pool-only candidates (cls 0) never do.
 * Layout: frame f's map is height x width elements, row-major, pitch = width, from element `off` of the byte map and of the id map
 * (the same off for both, counted in elements); frames follow one another, each from a multiple of 4 elements on; the 0..3
 * elements between two frames are 0 in the byte map and -1 in the id map.                                                        */
typedef struct str_er_frame_map {
    uint64_t off;            /* first element of this frame's map in the arrays below; a multiple of 4 */
    int32_t  width, height;  /* the frame's level-0 size                                            */
} str_er_frame_map;          /* 16 bytes */

/* The text lines of a frame, merged across pyramid levels (STR_ER_WANT_FRAME_LINES, str_er_line_feet_regions,
 * str_er_frame_lines_from_pairs).  All exact integers, on top of the pixel rule of str_er_frame_map.
 *   Footprint F(t) of line t of str_er_result_texts(): the set of pixels of frame texts[t].frame (level-0 size W x H) covered, by
 *     that rule, by the mask (str_er_mask) of at least one member text_ers[first .. first + count).  A member listed twice counts
 *     once.  The masks are over the candidates' own boxes, as for STR_ER_TEXT_MAP_LINE: the box and centre rewrites of
 *     overlap_suppression play no part.
 *   Foot box: the bounding box of F(t) in frame pixels; pixels = |F(t)|.  In a detect call (levels never larger than the frame) it
 *     is the union of the members' pre-image boxes.  An empty footprint (only possible in str_er_line_feet_regions with a plane
 *     larger than the output) has box 0, 0, 0, 0 and pixels = 0.
 *   Overlap of two lines a < b of one frame: inter(a, b) = |F(a) & F(b)|.
 *   Duplicates: a and b are duplicates iff inter > 0 and inter * den >= num * (|F(a)| + |F(b)| - inter) (Jaccard index >= num / den,
 *     in 64-bit integers).  num / den: str_er_set_frame_merge, default 1 / 2 -- a definition of this library, like the pyramid; it
 *     is not tuned on labelled data.
 *   Frame line: a connected component of the duplicate relation among the lines of one frame (its transitive closure, so no order
 *     of merging is involved).  Its representative is the member with the most pixels, ties to the smallest line index.  Frame lines
 *     are ordered by frame, then by their smallest member line index.  Lines of different frames never meet.                       */
typedef struct str_er_line_foot {
    int32_t  x, y, w, h;     /*  0: the foot box, frame pixels                                          */
    uint32_t pixels;         /* 16: |F(t)|                                                              */
    int32_t  frame_line;     /* 20: index into str_er_result_frame_lines()                              */
} str_er_line_foot;          /* 24 bytes; one per line of str_er_result_texts(), same order */
typedef struct str_er_line_pair {
    int32_t  a, b;           /*  0: two lines of one frame, a < b                                       */
    uint32_t inter;          /*  8: |F(a) & F(b)|, > 0                                                  */
    uint32_t dup;            /* 12: 1 if the two are duplicates at the call's num / den, else 0         */
} str_er_line_pair;          /* 16 bytes; every pair with inter > 0, sorted by (a, b) */
typedef struct str_er_frame_line {
    uint32_t frame;          /*  0                                                                      */
    int32_t  rep;            /*  4: the representative: a line index                                    */
    int32_t  first, count;   /*  8: its members: str_er_result_frame_line_members()[first .. first + count), line indices, ascending */
    int32_t  x, y, w, h;     /* 16: the union of the members' foot boxes                                */
    uint32_t pixels;         /* 32: the representative's                                                */
    uint32_t levels;         /* 36: bit k set if a member has pyr == k (k < 32)                         */
} str_er_frame_line;         /* 40 bytes */

/* The text lines of consecutive frames linked into text tracks (STR_ER_WANT_LINE_LINKS, str_er_link_feet,
 * str_er_text_tracks_from_links).  All exact integers, on top of the footprints of str_er_line_foot.
 *   Time order: the frames of a call are in time order, frame f + 1 follows frame f.  Frames f and f + 1 are adjacent iff their
 *     level-0 sizes are equal; across a change of size (list calls) there are no links.
 *   Overlap of a line a of frame f and a line b of an adjacent frame f + 1: inter(a, b) = |F(a) & F(b)|, the two footprints read at the
 *     same pixel coordinates.  Every such pair with inter > 0 is a record; the table is sorted by (a, b).
 *   Link: link = 1 iff inter * den >= num * (|F(a)| + |F(b)| - inter), in 64-bit integers.  num / den: str_er_set_line_link, default
 *     1 / 2 -- a definition of this library, like the duplicate threshold of str_er_line_foot; it is not tuned on labelled data.
 *   Text track: a connected component of (duplicates within a frame, str_er_line_pair::dup) u (links across adjacent frames) over all
 *     lines of the call: the transitive closure, so no order of joining is involved.  Its representative is the member with the most
 *     footprint pixels, ties to the smallest line index.  Tracks are ordered by first_frame, then by their smallest member.
 *   Across calls and stream submissions nothing is remembered: a result made with the flag keeps the footprints of the lines of its
 *     first and of its last frame on the host (str_er_result_edge_feet), and str_er_link_feet overlaps two such sets.  The word
 *     tracks' readings are pooled across calls by a track pool (str_er_pool_match).                                               */
typedef struct str_er_line_link {
    int32_t  a, b;           /*  0: a line of frame f and a line of the adjacent frame f + 1            */
    uint32_t inter;          /*  8: |F(a) & F(b)|, > 0                                                  */
    uint32_t link;           /* 12: 1 if the two are linked at the call's num / den, else 0             */
} str_er_line_link;          /* 16 bytes; every such pair with inter > 0, sorted by (a, b) */
typedef struct str_er_text_track {
    uint32_t first_frame, last_frame;  /*  0: the smallest and the largest frame of a member            */
    int32_t  first, count;   /*  8: its members: str_er_result_text_track_members()[first .. first + count), line indices, ascending */
    int32_t  rep;            /* 16: the representative: a line index                                    */
    uint32_t pixels;         /* 20: the representative's                                                */
} str_er_text_track;         /* 24 bytes */

/* The geometry of a text line from its footprint (STR_ER_WANT_LINE_GEOM, str_er_feet_geom, str_er_hull_of_points,
 * str_er_quad_from_hull).  All exact, on top of the footprints F(t) of str_er_line_foot.  Screen coordinates: x to the right, y down;
 * pixel (x, y) is the unit square with the corners (x, y) .. (x + 1, y + 1).
 *   Hull of a line t: the convex hull of the corners of the pixel squares of F(t) (the construction of str_er_shape::hull_area2 for a
 *     mask).  Its vertices are integer corners in [0, W] x [0, H]; the hull is strictly convex (collinear points are dropped); the
 *     order is clockwise on screen, from the vertex with the smallest (y, then x): the pixel (0, 0) alone gives (0,0), (1,0), (1,1),
 *     (0,1).  hull_area2 is twice its area.
 *   Moments of F(t), over its pixels in absolute frame pixel coordinates: pixels = |F|, m10 = sum x, m01 = sum y, m20 = sum x^2,
 *     m11 = sum x y, m02 = sum y^2, uint64.  With a foot box of at most 16384 x 16384 and x, y < 65536 nothing overflows; a larger
 *     foot box gives STR_ER_ECAPACITY.
 *   Oriented box: for the hull edge i (vertex i -> vertex (i + 1) mod count) with the integer vector e = (ex, ey) and the normal
 *     (-ey, ex), d(p) = p.x ex + p.y ey and c(p) = -p.x ey + p.y ex; dmin, dmax, cmin, cmax are the extremes of d and c over the hull
 *     vertices and A_i = (dmax - dmin)(cmax - cmin) / (ex^2 + ey^2).  The box is that of the edge with the smallest A_i, the A_i
 *     compared as exact fractions (128-bit products), ties to the smallest i; edge = i.  Corner k takes (d, c) = (dmin, cmin),
 *     (dmax, cmin), (dmax, cmax), (dmin, cmax): qx[k] = (double)(d ex - c ey) / (double)(ex^2 + ey^2), qy[k] = (double)(d ey + c ex) /
 *     (double)(ex^2 + ey^2) -- the numerators stay below 2^53, so every corner is one correctly rounded division.
 *   Frame line: its hull is the hull of the union of its member lines' hull vertices (that is the hull of the union of their
 *     footprints), its box is made from that hull, its moments and pixels are those of its representative.
 *   Empty footprint: count = 0, edge = -1, everything else 0.
 *   The vertex array (str_er_result_geom_points): the hulls of the lines in line order, then those of the frame lines in their order. */
typedef struct str_er_line_geom {
    uint32_t first, count;              /*   0: vertices: xy[2*first .. 2*(first+count)) as int32 x, y pairs */
    uint64_t hull_area2;                /*   8 */
    uint64_t m10, m01, m20, m11, m02;   /*  16 .. 48 */
    uint32_t pixels;                    /*  56 */
    int32_t  edge;                      /*  60 */
    int32_t  ex, ey;                    /*  64, 68 */
    int64_t  dmin, dmax, cmin, cmax;    /*  72 .. 96 */
    double   qx[4], qy[4];              /* 104, 136 */
} str_er_line_geom;                     /* 168 bytes */

/* The glyph runs and words of a text line from its footprint (STR_ER_WANT_LINE_WORDS, str_er_feet_words, str_er_words_from_runs).  All
 * exact integers, on top of the footprint F(t) and the foot box (x, y, w, h) of str_er_line_foot.
 *   Column count n(c), 0 <= c < w: the number of pixels of F(t) in the frame column x + c.  colmax = max over c of n(c).
 *   Glyph run: a maximal interval [c0, c1) of columns with n(c) > 0 throughout.  The runs of a line are ordered by c0; the foot box
 *     is tight, so the first run of a footprint that is not empty starts at column 0 and its last ends at w.  A run carries, over
 *     the pixels of F(t) in its columns, their number (pixels) and their row extent [y0, y1).  The record holds frame columns and
 *     rows: x0 = x + c0, x1 = x + c1.
 *   Gap between consecutive runs p, q of one line: g = q.x0 - p.x1 (>= 1).  It is a word break iff g * den >= num * colmax in 64-bit
 *     integers; num / den is set with str_er_set_word_gap and is 1 / 3 by default.  That default is a definition of this library,
 *     like the duplicate and the link thresholds: it is not tuned on labelled data.  (1, 65535) makes every gap a break, (65535, 1)
 *     makes none a break (colmax <= 16384).
 *   Word: a maximal sequence of consecutive runs of one line without a break between them.  Its box is the bounding box of its
 *     runs' pixels, its pixels their sum.
 *   Empty footprint: no runs, no words, colmax 0.
 *   Frame line: its words and runs are those of its representative line (str_er_frame_line::rep), the rule its moments follow;
 *     there is no separate table.
 *   The columns are those of the upright frame: a sloped baseline does not change the gaps between upright glyphs, rotated glyphs
 *     smear them.  Nothing is deskewed, and the runs are not mapped into the columns of a line crop.
 *   Runs and words lie back to back in line order.                                                                                 */
typedef struct str_er_line_run {
    int32_t  x0, x1;         /*  0,  4: frame columns, half open                     */
    int32_t  y0, y1;         /*  8, 12: frame rows, half open                        */
    uint32_t pixels;         /* 16                                                    */
    int32_t  word;           /* 20: index into the word table                         */
} str_er_line_run;           /* 24 bytes */
typedef struct str_er_line_word {
    int32_t  line;           /*  0: index into str_er_result_texts() / the feet given */
    int32_t  first_run, n_runs;      /*  4,  8: into the run table                    */
    int32_t  x, y, w, h;     /* 12 .. 24: the bounding box of its runs' pixels        */
    uint32_t pixels;         /* 28                                                    */
} str_er_line_word;          /* 32 bytes */
typedef struct str_er_line_words {
    int32_t  first_word, n_words, first_run, n_runs;      /* 0 .. 12                  */
    uint32_t colmax, reserved;       /* 16, 20                                        */
} str_er_line_words;         /* 24 bytes; one per line of str_er_result_texts() */

/* The reading of a glyph run (STR_ER_WANT_RUN_READ, str_er_feet_read): one character per run and one string per word.  A definition of
 * this library, like the word gap, on top of the footprint F(t) and OCR::chain_run (str_er_ocr_chain_run_slope).
 *   Tile of a run r = (x0, x1, y0, y1) of line t: T_r has (x1 - x0) x (y1 - y0) bytes, T_r(i, j) = 0 if the frame pixel
 *     (x0 + i, y0 + j) is in F(t), else 255.  Only line t's own footprint counts: another line's pixels inside the box do not.  A glyph
 *     is dark on light, so chain_run's 255 - roi makes it bright, as for a region of a plane that is not inverted.
 *   Reading of a run: what OCR::chain_run gives for the whole tile as its box with the slope s of the line: the 1800 feature bytes q,
 *     label and prob = pv[label].  s = str_er_text::slope of line t (str_er_feet_read: slopes[t]); a slope that is not finite counts
 *     as 0, as for the line crops.  The slope is in the coordinates of the line's pyramid level and the tile is in frame pixels: the
 *     pyramid scales both axes alike up to the rounding of the level sizes, so the slope is used as it is.
 *   Character of a run: str_er_ocr_char(label).  No run is dropped for a low probability: prob is returned and the caller filters.
 *   String of a word: the characters of runs[first_run .. first_run + n_runs).  Text of a frame line: the words of its representative
 *     joined by one blank.
 *   Limits: the string of a word is the arg max of its runs: in it there is no spelling correction and no language model (the
 *     reference's word graph and corrector are not rebuilt), and a run of touching glyphs reads as one character here: runs
 *     are split in the image by a separate output, str_er_run_split (STR_ER_WANT_RUN_SPLIT).  The match of a word against a lexicon, which may spend a character without a run of its own or a
 *     run without a character, is a separate output: str_er_word_match (STR_ER_WANT_WORD_MATCH); so is the cheapest string of a word
 *     under a character bigram table, with the same two moves: str_er_word_decode (STR_ER_WANT_WORD_DECODE).                        */
typedef struct str_er_run_read {
    int32_t  label;          /*  0: the scorer's label                                */
    int32_t  ch;             /*  4: str_er_ocr_char(label)                            */
    double   prob;           /*  8: pv[label]                                         */
} str_er_run_read;           /* 16 bytes; one per run of str_er_result_line_runs()    */

/* The match of a word against a lexicon (STR_ER_WANT_WORD_MATCH, str_er_match_words): a weighted edit distance, in integers, between
 * the glyph runs of the word and every entry of the caller's lexicon, with the best and the second-best entry.  A definition of this
 * library, like the word gap and the reading of a run; it is exact, and the host states the same rules (str_er_prob_costs,
 * str_er_match_words_host).
 *   Alphabet: the 65 characters of str_er_ocr_char; the index a of a character is its label 0 .. 64.
 *   Cost of a probability: T[c] = ldexp(M[c % 8], -(c / 8)) for c = 0 .. 254, M the eight doubles nearest to 2^(-j/8)
 *     (str_er_cost_thresholds).  cost(p) is the smallest c in 0 .. 254 with p >= T[c], otherwise 255; NaN and negative values give
 *     255.  The unit is 1/8 bit.  Only comparisons of doubles are involved: the host and the device agree exactly.
 *   Cost row of a run: 65 bytes, C[a] = cost(prob[j]) for the class j of the model whose label is a (the first such class), 255 where
 *     the model has no such class; classes with a label outside 0 .. 64 are ignored.  With the lexicon's fold-case flag both letters
 *     of a case pair get the minimum of the two.
 *   Lexicon: n entries, 0 <= n <= 2^20, each of 1 .. 32 bytes over the alphabet; duplicates are allowed.  With
 *     STR_ER_LEXICON_FOLD_CASE the entries are compared without regard to case -- the matcher reads min(C[a], C[a']) for a letter a
 *     and its other case a' -- and reported as given.
 *   Cost of entry e (length l) for a word with the runs 1 .. m: D[0][0] = 0, D[i][0] = i * DEL, D[0][j] = j * INS,
 *     D[i][j] = min(D[i-1][j-1] + C_i[e_j], D[i-1][j] + DEL, D[i][j-1] + INS); the cost is D[m][l].  DEL is a run with no character
 *     of its own (a speck, a broken piece), INS a character with no run of its own (touching glyphs); both are in 1 .. 255 and 64 by
 *     default (str_er_set_word_match).
 *   Band: an entry is tried iff |l - m| <= band; the band is in 0 .. 31 and 2 by default.  A word with m > 32 tries nothing.
 *   Result: (cost, entry) is the minimum over the tried entries of (cost, index); second_* the same minimum over the tried entries
 *     other than `entry`; free_cost the sum over the runs of min_a C_i[a], the cost of the word's own reading (of every run, also
 *     for m > 32); n_tried the number of entries tried.  entry and second_entry are -1, with their costs -1, where nothing qualifies. */
typedef struct str_er_word_match {
    int32_t  entry, cost;                 /*  0,  4                                   */
    int32_t  second_entry, second_cost;   /*  8, 12                                   */
    int32_t  free_cost, n_tried;          /* 16, 20                                   */
} str_er_word_match;         /* 24 bytes; one per word of str_er_result_words()       */
#define STR_ER_LEXICON_FOLD_CASE 1u

/* The words of consecutive frames linked into word tracks, and one lexicon match per word track over the cost rows of all its
 * members (STR_ER_WANT_TRACK_READ, str_er_word_links, str_er_word_tracks_from_links, str_er_match_tracks).  All exact integers and
 * a definition of this library, on top of the text tracks of str_er_line_link, the words of str_er_line_word and the matcher of
 * str_er_word_match; nothing is tuned on labelled data.
 *   Reading line: for a text track k and a frame f that holds members of k, R(k, f) is the member line of frame f with the most
 *     footprint pixels, ties to the smallest line index (the representative's rule).  A word is eligible iff its line is a reading
 *     line: of the duplicate lines of several pyramid levels only one is read.
 *   Word link: frames f and f + 1 are adjacent as for str_er_line_link (equal level-0 sizes).  For every track k with reading lines
 *     in both, every word u of R(k, f) and every word v of R(k, f + 1): inter(u, v) is the area of the intersection of the two
 *     boxes (x, y, w, h) of str_er_line_word, as uint32.  Every such pair with inter > 0 is a record; the table is sorted by (a, b).
 *     link = 1 iff inter * den >= num * (area(u) + area(v) - inter) in 64-bit integers; num / den: str_er_set_word_link, each in
 *     1 .. 65535, 1 / 2 by default.  Words of different tracks, of frames that are not adjacent and of lines that are not reading
 *     lines never meet.  Boxes are linked, not footprints.
 *   Word track: a connected component of the links with link = 1 over the eligible words: the transitive closure, so two words of
 *     one frame can land in one track.  Its members are word indices, ascending; rep is the member with the most pixels
 *     (str_er_line_word::pixels), ties to the smallest index.  Tracks are ordered by first_frame, then by their smallest member.  An
 *     eligible word without a link is a track of one.  One int32 per word gives its track, -1 for a word that is not eligible.
 *   Track match of a track with the members w_1 .. w_n: member i has m_i cost rows, the rows the matcher read for that word (with
 *     STR_ER_WANT_RUN_SPLIT those of its parts).  The fold, INS, DEL and the band are those of str_er_word_match.  A member is usable
 *     iff m_i <= 32.  For an entry e of length l, cost(e) is the sum over the usable members of D_i[m_i][l], the recurrence of
 *     str_er_word_match, whatever |l - m_i| is.  e is tried iff |l - m_i| <= band for at least one usable member: the lengths tried
 *     are a union of bands and may have gaps.  (cost, entry) is the minimum of (cost, index) over the tried entries, second_* the
 *     same over the tried entries other than `entry`; both are -1 with their costs where nothing qualifies.  free_cost is the sum of
 *     the free costs of all members (also the unusable ones), n_tried the number of entries tried, n_used the number of usable
 *     members.  Per slot of the member array, member_cost is D_i[m_i][l] for the winning entry, -1 for an unusable member or where
 *     entry is -1: their sum is cost.  best_member is the word with the smallest member_cost, ties to the earliest slot, or -1.  A
 *     track has at most 65536 members (STR_ER_ECAPACITY above): with at most 64 * 255 a member the sum stays inside int32.
 *     A track of one usable member has the six fields of that word's str_er_word_match; a track of unusable members tries nothing.
 *   Limits: across calls and stream submissions a detect call remembers nothing -- str_er_word_links and
 *     str_er_word_tracks_from_links link words over submissions, and a track pool (str_er_pool_match) keeps the summed costs of a
 *     track on the device from call to call.  The open-vocabulary reading of a track, a median string over members with different
 *     run counts, is a separate output, str_er_track_decode (STR_ER_WANT_TRACK_DECODE).  The members enter with the rows the
 *     matcher read; the track match in which every member's segmentation is free is a separate output,
 *     str_er_lattice_track_member (STR_ER_WANT_LATTICE_TRACK).                                                                    */
typedef struct str_er_word_link {
    int32_t  a, b;           /*  0: a word of frame f and a word of the adjacent frame f + 1            */
    uint32_t inter;          /*  8: the area of the intersection of their boxes, > 0                    */
    uint32_t link;           /* 12: 1 if the two are linked at the call's num / den, else 0             */
} str_er_word_link;          /* 16 bytes; every such pair with inter > 0, sorted by (a, b) */
typedef struct str_er_word_track {
    uint32_t first_frame, last_frame;  /*  0: the smallest and the largest frame of a member            */
    int32_t  first, count;   /*  8: its members: str_er_result_word_track_members()[first .. first + count), word indices, ascending */
    int32_t  rep;            /* 16: the representative: a word index                                    */
    int32_t  text_track;     /* 20: the text track of its members' lines                                */
} str_er_word_track;         /* 24 bytes */
typedef struct str_er_track_match {
    int32_t  entry, cost;                 /*  0,  4                                   */
    int32_t  second_entry, second_cost;   /*  8, 12                                   */
    int32_t  free_cost, n_tried;          /* 16, 20                                   */
    int32_t  n_used, best_member;         /* 24, 28                                   */
} str_er_track_match;        /* 32 bytes; one per word track                          */

/* The track pool: the track match of str_er_track_match pooled across calls (str_er_track_pool_create, _add, _add_lattice, _join,
 * _clear, _read).  A pool belongs to one context and has cap_tracks slots; a slot is one pooled word track.  At creation (and at
 * every _reset) the pool is bound to the context's lexicon and its INS / DEL / band, and in lattice mode (STR_ER_POOL_LATTICE) to the
 * SPLIT of str_er_set_run_split as well: str_er_set_lexicon, str_er_set_word_match and str_er_set_run_split make every pool of the
 * context stale, and a stale pool answers STR_ER_ESTATE to everything except _reset and _destroy.
 *   State of a slot, on the device: for every entry of the lexicon the int32 sum, over the usable members added so far, of
 *     D_i[m_i][l] (in lattice mode L_i of str_er_lattice_track_member), whatever |l - m_i| is -- a member added later may widen the
 *     lengths tried, and the entries of the new lengths then carry the earlier members' distances already; the 32-bit mask of the
 *     lengths tried so far; free_cost, n_used and the number of members.
 *   Defining property: the first seven fields of a slot's record equal the first seven fields of the str_er_track_match that
 *     str_er_match_tracks_host (in lattice mode str_er_lattice_match_tracks_host) gives, with the pool's lexicon, flags and
 *     parameters, for one track whose member list is the concatenation, in any order, of everything added to the slot; n_members
 *     is the length of that list.  Costs are exact integers and a sum does not depend on its order: the record is the same bytes
 *     whatever the order and the grouping of the additions.  An empty slot reads as a track of no members: -1, -1, -1, -1, 0, 0, 0, 0.
 *   A slot holds at most 65536 members (STR_ER_ECAPACITY above), the bound under which the int32 sums are safe.
 *   Limits: member_cost, best_member and the members' segmentations are not pooled -- the winning entry can change with every
 *     addition, and the members' rows are not kept; str_er_match_tracks / str_er_lattice_match_tracks give them for the members of
 *     one call.  There is no pooled open-vocabulary decode across calls in a pool of this kind: str_er_track_decode
 *     (STR_ER_WANT_TRACK_DECODE) decodes the word tracks of one call, and a pool of another kind, the decode pool
 *     (str_er_pool_decode, below), keeps the newest members of a track on the device and decodes them.  The pool must be destroyed
 *     before its context.                                                                                                          */
#define STR_ER_POOL_LATTICE 1u
typedef struct str_er_track_pool str_er_track_pool;
typedef struct str_er_pool_match {
    int32_t  entry, cost;                 /*  0,  4                                   */
    int32_t  second_entry, second_cost;   /*  8, 12                                   */
    int32_t  free_cost, n_tried;          /* 16, 20                                   */
    int32_t  n_used, n_members;           /* 24, 28                                   */
} str_er_pool_match;         /* 32 bytes; one per slot read                           */

/* The decode pool: the track decode of str_er_track_decode pooled across calls.  It is a str_er_track_pool of another kind, made by
 * str_er_track_pool_create_decode with cap_tracks slots and a per-slot limit keep, 1 .. 1024 (the member bound of the track decode);
 * _info reports the flag STR_ER_POOL_DECODE and n_entries = 0.  The score J(s) = lm(s) + the sum of A_i(s) has to be evaluable for
 * strings nobody has seen yet, so there is no sum to keep: the members' cost rows themselves stay on the device.
 *   Binding: at creation and at every _reset the pool is bound to the context's bigram table, to the INS / DEL of
 *     str_er_set_word_decode (they make the seeds' strings when a member is added) and to the INS / DEL / rounds of
 *     str_er_set_track_decode (a read uses them).  str_er_set_bigram, str_er_set_word_decode and str_er_set_track_decode make every
 *     decode pool of the context stale -- and no lexicon pool; str_er_set_lexicon, str_er_set_word_match and str_er_set_run_split
 *     make every lexicon pool stale -- and no decode pool.  A stale pool answers STR_ER_ESTATE to everything except _reset, _info
 *     and _destroy.  A decode pool needs no lexicon and no SVM model; without a bigram table its creation answers STR_ER_ESTATE.
 *   Keys: every successful _add with n_tracks > 0 takes the next serial of the pool, 1, 2, ... (uint32, back to 0 at _reset).  The
 *     key of a member is serial << 32 | its index in that call's member array.  Keys are unique in a pool: "newer" is a total order.
 *   State of a slot: n_members counts everything ever added to the slot or joined into it, the unusable members (more than 32 rows)
 *     included, under the pool's bound of 65536 (STR_ER_ECAPACITY).  The kept list is the `keep` largest keys among all usable
 *     members ever added to the slot or to slots joined into it; per kept member the slot stores its key, its run count, its up to
 *     32 rows of 65 bytes (unfolded, the rows of str_er_word_decode), its str_er_word_decode record and its 64 string bytes as the
 *     decoder made them on those rows.  An unusable member is counted and not kept.  The top-keep of a union is the top-keep of the
 *     union of top-keeps: the kept list does not depend on how joins were grouped.
 *   Defining property: _read_decode of a slot gives a record, 32 label bytes and member costs in age order that equal what
 *     str_er_decode_tracks_host gives for one track whose member list is the kept list in ascending key order, the words numbered
 *     0 .. n_kept - 1 in that order, under the table and parameters the pool is bound to.  seed_member is therefore an age rank.
 *     Age order matters: the seeds are the first 32 in order, and ties go to the seed rank.  n_members and n_kept follow the eight
 *     fields of str_er_track_decode.  An empty slot reads as a track of no members: -1, -1, 0, 0, 0, 0, -1, -1, n_members = n_kept
 *     = 0, labels 0xFF, no member costs.
 *   Limits: a slot's reading uses at most keep members, the newest; evicted evidence is gone -- this is not a sum over all members
 *     ever seen.  There is no lattice mode of a pool of this kind: a pool of a third kind, the lattice decode pool (below), keeps the
 *     members' piece lattices and decodes them jointly.  A read decodes what it is asked for every time: there is no cache of clean
 *     slots.                                                                                                                          */
#define STR_ER_POOL_DECODE 2u
typedef struct str_er_pool_decode {
    int32_t  cost, seed_cost;             /*  0,  4                                   */
    int32_t  n_chars, n_edits;            /*  8, 12                                   */
    int32_t  converged, n_used;           /* 16, 20                                   */
    int32_t  seed_member, lm_cost;        /* 24, 28: seed_member is an age rank       */
    int32_t  n_members, n_kept;           /* 32, 36                                   */
} str_er_pool_decode;        /* 40 bytes; one per slot read                           */

/* The lattice decode pool: the track decode over the members' piece lattices (str_er_lattice_track_decode) pooled across calls -- the
 * cell bigram table x piece lattice of the pools.  It is a str_er_track_pool of a third kind, made by
 * str_er_track_pool_create_lattice_decode with cap_tracks slots and a per-slot limit keep, 1 .. 1024; _info reports the flags
 * STR_ER_POOL_DECODE | STR_ER_POOL_LATTICE (3) and n_entries = 0.  str_er_track_pool_create with the flags 2 or 3 stays STR_ER_EINVAL.
 *   Members: _add_lattice takes the arguments and checks of str_er_lattice_decode_tracks, plus slots, on the unfolded rows.  A member
 *     is usable iff N_i <= 32, and N_i = 0 is usable: the rule of str_er_lattice_track_decode.  An unusable member is counted in
 *     n_members and not kept.
 *   Keys, keep and joins are the decode pool's, word for word: the key of a member is serial << 32 | its index in that call's member
 *     array, keep is 1 .. 1024, the kept list is the `keep` largest keys among all usable members ever added to the slot or to slots
 *     joined into it, the top-keep of a union is the top-keep of the union of top-keeps, and a slot counts at most 65536 members.
 *     One bound is tighter: cap_tracks * keep is at most 13 421 772 (2^30 / 80), not 2^24 -- a kept member owns 80 piece rows and the
 *     track decode tells a piece's row from a run's by bit 30 of its index, so every piece row of the store lies below 2^30.
 *   Kept per member, on the device: its key and its run count; the str_er_run_split records of its runs; the rows of its runs (up to 32)
 *     and of all its pieces (up to 72: 8 runs of 4 atoms with 9 pieces each); its str_er_lattice_decode record and the 64 label bytes
 *     that the lattice decoder made on these rows under the bound table, INS / DEL and SPLIT.  A kept member takes 9072 bytes on the
 *     device: 2080 of run rows, 5200 of piece rows (80 rows, so that every member's block starts at a multiple of 65 and of 16 bytes),
 *     1024 of split records, 656 of lattice structure and 112 of key, counts, record and labels.
 *   Binding: the pool is bound to what a decode pool is bound to -- the bigram table, str_er_set_word_decode and
 *     str_er_set_track_decode -- and to the SPLIT of str_er_set_run_split.  It is stale after any setter that makes a decode pool
 *     stale, and while the context's SPLIT differs from the bound one: the values are compared, so setting the same SPLIT again, or
 *     another num / den only, leaves it usable (the pool never makes cuts).  A decode pool of rows does not go stale on
 *     str_er_set_run_split.  _reset binds the pool to the context as it is then.
 *   Defining property: take one track whose member list is the slot's kept list in ascending key order, the words numbered
 *     0 .. n_kept - 1 in that order, word i with its runs at 32 * i and its pieces at 80 * i + its piece rows back to back in run
 *     order, under the bound table and parameters.  _read_lattice_decode of the slot equals what str_er_lattice_decode_tracks_host
 *     gives for that track: the record and the 32 label bytes; in age order, per kept member, its str_er_lattice_track_member, its 32
 *     source bytes and its parts.  seed_member is an age rank, and the member records' word is the age rank too.  The record is
 *     str_er_pool_decode.  An empty slot reads exactly as an empty slot of a decode pool.
 *   It follows: (1) a lattice decode pool whose members have no cut reads, byte for byte, what a decode pool of rows fed the same
 *     words reads (property (5) of str_er_lattice_track_decode); (2) one addition into empty slots with keep >= the track's usable
 *     members equals str_er_lattice_decode_tracks of that call, up to seed_member and word being ranks and the parts' indices being
 *     the store's.
 *   Limits: those of the decode pool -- at most keep members, the newest, are read; evicted evidence is gone; a read decodes what it is
 *     asked for every time -- and those of str_er_lattice_track_decode: a local optimum of single edits.                             */

/* The decoding of a word under a character bigram table (STR_ER_WANT_WORD_DECODE, str_er_decode_words): the cheapest character string
 * of a word under the cost rows of its glyph runs plus a table of costs of one character after another, which may drop a run (a speck)
 * or spend a character that has no run of its own (touching glyphs), the two moves of str_er_word_match.  A definition of this
 * library; integers only, exact, and the host states the same rules (str_er_decode_words_host).
 *   Symbols: the 65 characters of str_er_ocr_char with their labels 0 .. 64, and 65 = E, the word boundary ("no character yet", "end
 *     of word").
 *   Table: B, 66 x 66 bytes, row-major, in the unit of the cost rows (1/8 bit): B[a][b] the cost of b directly after a, B[E][b] of
 *     beginning with b, B[a][E] of ending on a, B[E][E] of the empty word (str_er_set_bigram; str_er_bigram_from_probs makes one).
 *   Cost rows: the 65-byte rows of str_er_word_match, never folded: case matters to a bigram table.
 *   Moves: INS and DEL in 0 .. 255, 0 switches a move off; both are 0 by default (str_er_set_word_decode): a plain Viterbi pass, one
 *     character per run.
 *   Recurrence, for a word with the runs 1 .. m, m <= 32, in int32 with INF = 2^20: V_0[E] = 0, V_0[a] = INF for a < 65.  For
 *     i = 1 .. m: SUB, for b < 65: S[b] = min over a in 0 .. 65 of (V_{i-1}[a] + B[a][b]) + C_i[b], the predecessor the smallest a
 *     that attains the minimum; U[b] = S[b], U[E] = INF.  DEL, if DEL > 0, for a in 0 .. 65: D = V_{i-1}[a] + DEL; if D < U[a] then
 *     U[a] = D and the move is DEL (on a tie SUB stays).  INS, if INS > 0, for c < 65: I = min over b in 0 .. 64 of (U[b] + B[b][c])
 *     + INS, with the smallest b; if I < U[c] then V_i[c] = I and the move is INS, else V_i[c] = U[c]; always V_i[E] = U[E].  So at
 *     most one character is inserted after a run, and only after some character.  cost = min over a in 0 .. 65 of V_m[a] + B[a][E],
 *     with the smallest a; for m = 0 that is B[E][E].  INF is never the minimum.
 *   String: the backtrack from the end state by the recorded moves.  At (i, c) an INS move emits c with the source (i-1) | 0x80 and
 *     goes to the U-level state b; a SUB move emits b with the source i-1 and goes to (i-1, predecessor); a DEL move emits nothing
 *     and goes to (i-1, a).  Reversed: at most 2m <= 64 labels, each with the word-relative index of the run it came from, bit 7 set
 *     on an inserted character.  Per word 64 bytes of labels and 64 bytes of sources, padded with 0xFF past n_chars.
 *   Record: read_cost is the cost under B of the plain reading -- the first arg min of every row, all SUB, with the boundary terms --
 *     and is made for every m.  Hence cost <= read_cost, n_sub + n_ins = n_chars and n_sub + n_del = m.  A word with m > 32 is not
 *     decoded: cost = -1 and the four counts are 0.
 *   Limits: runs are split in the image only with STR_ER_WANT_RUN_SPLIT (str_er_run_split), then the rows are those of the word's
 *     parts, a segmentation fixed ahead of the table; segmentation and string chosen together over all pieces are a separate output,
 *     str_er_lattice_decode (STR_ER_WANT_LATTICE_DECODE); one path per word -- how far the next reading of every run lies from it is a
 *     separate output, str_er_word_margin (str_er_set_word_margin); the table is the caller's.  The bridge from a table of
 *     transition probabilities (str_er_bigram_from_probs) takes 65 x 65 doubles as P(b after a); whether the floats of the
 *     reference's dictionary/tp_table.txt are such probabilities has not been checked, and nothing beyond that reading is promised. */
typedef struct str_er_word_decode {
    int32_t  cost, read_cost;             /*  0,  4                                   */
    int32_t  n_chars, n_sub;              /*  8, 12                                   */
    int32_t  n_del, n_ins;                /* 16, 20                                   */
} str_er_word_decode;        /* 24 bytes; one per word of str_er_result_words()       */

/* The margins of a decoded word (str_er_set_word_margin beside STR_ER_WANT_WORD_DECODE, str_er_word_margins): the min-marginals of
 * the recurrence of str_er_word_decode -- for every run of the word and every reading of it the cost of the cheapest whole path that
 * reads the run that way -- and from them how much more the cheapest path costs that reads some run differently from the decoded
 * string.  A definition of this library; integers only, exact, and the host states the same rules (str_er_word_margins_host).
 *   Take a word with the rows C_1 .. C_m, 1 <= m <= 32.  B, INS, DEL, E = 65, INF and the forward values V_i[a], U_i[a] are those of
 *     str_er_word_decode; S_i[b] is its SUB value before DEL is compared: min over a of (V_{i-1}[a] + B[a][b]) + C_i[b], for b < 65.
 *   Backward values, in int32: G_m[a] = B[a][E] for a in 0 .. 65.  For i = m .. 1: GU_i[a] = G_i[a]; if INS > 0, for b < 65:
 *     GU_i[b] = min(G_i[b], min over c < 65 of (B[b][c] + G_i[c]) + INS).  Then G_{i-1}[a] = min over b < 65 of (B[a][b] + C_i[b] +
 *     GU_i[b]), and if DEL > 0 that value is also min-ed with DEL + GU_i[a].  min over a of (V_i[a] + G_i[a]) = cost for every i, and
 *     G_0[E] = cost.
 *   Marginals, 66 per row: M_i[b] = S_i[b] + GU_i[b] for b < 65, run i read as b; M_i[65] = min over a in 0 .. 65 of (V_{i-1}[a] + DEL
 *     + GU_i[a]) if DEL > 0, else -1: run i dropped.  Every path does exactly one of these at run i, so the minimum of M_i[x] over the
 *     entries >= 0 is cost.  Every marginal that exists is at most 16575 (the all-SUB path); INF never wins.
 *   Reading of a row: x_i is the label of the character of the word's decoded string whose source is i-1 with bit 7 clear, or 65 if
 *     there is none.  M_i[x_i] = cost.
 *   Margin of a row: margin_i is the minimum of M_i[x] over x != x_i with M_i[x] >= 0, minus cost: >= 0, and 0 on a tie; alt_i is the
 *     smallest such x that attains it (there are 65 labels: it always exists).
 *   Record: margin = min over i of margin_i, row the smallest word-relative i-1 that attains it, read and alt those of that row.  So
 *     margin is the extra cost of the cheapest path that reads some run differently.  All four fields are -1 for m = 0 and for m > 32
 *     (not decoded).
 *   Per word, beside the record: 32 int32 row margins, -1 past m; 32 bytes of row readings and 32 of row alternatives, 0xFF past m;
 *     on request (str_er_word_margins) the marginals, 32 x 66 int32, -1 past m and where no path exists.  The layout is fixed per
 *     word, as for the decoder's labels and sources.
 *   Limits: an inserted character has no row, so it has no margin of its own, and paths that differ only in insertions are not told
 *     apart.  This covers the word decoder only: no lattice decode, no tracks, no pool (the lattice decoder has margins of its own,
 *     str_er_lattice_margin).  Nothing is calibrated against labelled text: a margin is a cost difference in the unit of the cost
 *     rows, not a probability.                                                                                                     */
typedef struct str_er_word_margin {
    int32_t  margin, row;                 /*  0,  4                                   */
    int32_t  read, alt;                   /*  8, 12                                   */
} str_er_word_margin;        /* 16 bytes; one per word of str_er_result_words()       */

/* The decoding of a whole text line under the bigram table (str_er_set_line_decode beside STR_ER_WANT_WORD_DECODE, str_er_decode_lines):
 * one Viterbi pass over all rows of a line in which every gap between two rows either joins them into one word or breaks the line into
 * two words, so that the word breaks are chosen together with the string.  The cheapest string of the line, blanks included, and the
 * word segmentation that goes with it.  A definition of this library; integers only, exact, and the host states the same rules
 * (str_er_decode_lines_host).  The word gap of str_er_line_run stays what it is: it is one path this decoder is never worse than.
 *   Symbols and moves: the symbols, the table B (66 x 66, E = 65), INS, DEL (str_er_set_word_decode), INF = 2^20 and the unfolded
 *     65-byte cost rows are those of str_er_word_decode.
 *   Gap costs: one pair of bytes (J_i, K_i) per row, for the gap in front of row i: J_i the cost of joining row i to the word of row
 *     i-1, K_i of breaking in front of it.  The pair of a line's first row is ignored.  255 means the move is off; a pair with both
 *     entries off is an argument error (STR_ER_EINVAL).
 *   Recurrence, for a line with the rows 1 .. n, n <= 1024, in int32: V_0[E] = 0, V_0[a] = INF for a < 65.  For i = 1 .. n:
 *     Gap step, for i >= 2, on V = V_{i-1}: W[a] = V[a] + J_i for all a in 0 .. 65; if J_i is off, W[a] = INF exactly.  If K_i is not
 *     off: X = min over a in 0 .. 65 of (V[a] + B[a][E]) + K_i, attained at the smallest such a; if X < W[E] then W[E] = X and the gap is
 *     a BREAK from a; on a tie the join stays.  A break from a = E is allowed: that is an empty word and it costs B[E][E].  For i = 1,
 *     W = V_0.
 *     Run step on W: exactly the step of str_er_word_decode (SUB with the smallest predecessor in 0 .. 65, U[E] = INF, DEL on a strict
 *     <, INS over b < 65 on a strict <).  It gives V_i.
 *     cost = min over a of V_n[a] + B[a][E], attained at the smallest a.  For n = 0 it is B[E][E].
 *   Why 1024: the all-SUB path that takes at every gap a move that is on costs at most 255 + 255 for the first row, for every further
 *     row the row byte 255 plus the larger of a join, B[a][b] + J <= 255 + 254, and a break, B[a][E] + K + B[E][b] <= 255 + 254 + 255,
 *     that is 1019, and 255 at the end: cost <= 510 + 1019 * 1023 + 255 = 1 043 202 < 2^20 for n = 1024, so INF never wins, and every
 *     value stays below 2^25.  A line with n > 1024 is not decoded: cost = -1, the counts are 0, the labels are 0xFF, the sources
 *     0xFFFF and word_of_row is -1.
 *   Backtrack, from the end state, for i = n .. 1: undo the run step as str_er_word_decode does (INS emits c and goes to the U-level
 *     state, SUB emits b, DEL emits nothing).  If the state is now E and gap i recorded a BREAK, emit the label 65 and go to the
 *     recorded a.  Reversed, the labels are the line's string: 0 .. 64 for characters, 65 for a blank.
 *   Sources (uint16, the line-relative row index): i-1 for SUB, (i-1) | 0x8000 for INS, (i-1) | 0x4000 for the break in front of row
 *     i-1.
 *   Per line: the record below, with n_chars counting the breaks too: n_sub + n_ins + n_breaks = n_chars and n_sub + n_del = n.
 *     Labels (uint8) and sources (uint16): the line's slice begins at entry 3 * first_row of a table of 3 * n_rows entries (3n - 1 is
 *     the most a line can emit) and is padded with 0xFF / 0xFFFF past n_chars.  One int32 per row, word_of_row: the number of breaks
 *     emitted before the row's character, or -1 for a dropped row.  So the line has n_breaks + 1 words, empty ones included.
 *   It follows: (1) with (J, K) = (0, off) at every gap and n <= 32, cost, labels and sources equal str_er_word_decode's on the same
 *     rows (bit 7 of its source is 0x8000 here).  (2) With (0, off) inside the words of some segmentation and (off, 0) at its word
 *     gaps, every word of <= 32 rows: cost is the sum of the words' str_er_word_decode costs, and the labels are the words' labels
 *     joined by one 65, for any table, B[E][E] != 0 included.  (3) For any gap costs with both moves on, cost <= that same sum plus
 *     the J / K the segmentation pays at its gaps.
 *   Gap costs from the geometry (str_er_line_gap_costs; a definition of this library, like the word gap itself, not tuned): for
 *     consecutive rows of one line that belong to different runs p, q: g = q.x0 - p.x1 (below 0 counts as 0),
 *     x = min(16, (8 * g * den) / (num * colmax)) in 64-bit integers with num / den the word gap, so x = 8 is exactly the threshold
 *     of str_er_line_run; with the weight w in 0 .. 127: J = (w * x) / 8, K = (w * (16 - x)) / 8.  Both are <= 254 and never off, they
 *     tie at the old threshold, and w = 0 leaves the decision to the table alone.  Rows of the same run (the parts of
 *     STR_ER_WANT_RUN_SPLIT) get (0, 255): a cut inside a run is never a blank.  The first row of a line, and a row of no line, gets
 *     (0, 255) as well.
 *   Limits: one path per line, no margins in this record: how firmly its readings and breaks hold is str_er_line_margin's to say.
 *     The segmentation of the runs themselves is the fixed one of the decoder's window: joint decoding over the piece lattice is not
 *     part of this.  The cuts of touching glyphs chosen together with the word breaks over the runs' piece lattices are a separate
 *     output, str_er_line_lattice_decode (str_er_lattice_decode_lines).  No tracks, no pool.  Nothing is calibrated: the weight is
 *     the caller's.
 *   In a detect call the rows are the decoder's: the runs of the line, and with STR_ER_WANT_RUN_SPLIT the parts of its words in word
 *     order (the rows of str_er_result_split_parts(); the windows then index that table, and the line is decoded behind a second wait,
 *     once the parts are known).  A line's window runs from the first row of its first word to the last row of its last word.       */
typedef struct str_er_line_decode {
    int32_t  cost, n_chars;               /*  0,  4                                   */
    int32_t  n_breaks, n_sub;             /*  8, 12                                   */
    int32_t  n_del, n_ins;                /* 16, 20                                   */
} str_er_line_decode;        /* 24 bytes; one per line of str_er_result_texts()       */

/* The margins of a decoded line (str_er_set_line_margin beside str_er_set_line_decode, str_er_line_margins): the min-marginals of the
 * recurrence of str_er_line_decode -- for every row and every reading of it, and for every gap and either move at it, the cost of the
 * cheapest whole path that does just that -- and from them how much more the cheapest path costs that reads some row differently or
 * decides some gap differently from the decoded string.  A definition of this library; integers only, exact, and the host states the
 * same rules (str_er_line_margins_host).
 *   Symbols, B, E = 65, INS, DEL, INF = 2^20, the cost rows C_i, the gap pairs (J_i, K_i) with 255 = off and the forward values are
 *     those of str_er_line_decode.  Take a line with the rows 1 .. n, 1 <= n <= 1024.
 *   Forward values: V_{i-1} is the state vector before gap i, W_i the one behind the gap step (W_1 = V_0);
 *     X_i = min over a of (V_{i-1}[a] + B[a][E]) + K_i where K_i is on; S_i[b] = min over a in 0 .. 65 of (W_i[a] + B[a][b]) + C_i[b]
 *     for b < 65, the SUB value before DEL is compared.
 *   Backward values, in int32: G_n[a] = B[a][E] for a in 0 .. 65.  For i = n .. 1, in this order: GU_i = G_i; if INS > 0, for b < 65:
 *     GU_i[b] = min(G_i[b], min over c < 65 of (B[b][c] + G_i[c]) + INS).  H_i[a] = min over b < 65 of (B[a][b] + C_i[b] + GU_i[b]),
 *     and if DEL > 0 also min-ed with DEL + GU_i[a].  For i >= 2: G_{i-1}[a] = the smaller of J_i + H_i[a] (if J_i is on) and
 *     B[a][E] + K_i + H_i[E] (if K_i is on).  For i = 1: G_0 = H_1, and G_0[E] = cost.
 *   Row marginals, 66 per row: M_i[b] = S_i[b] + GU_i[b] for b < 65, row i read as b; M_i[65] = min over a of (W_i[a] + DEL + GU_i[a])
 *     if DEL > 0, else none: row i dropped.
 *   Gap marginals, 2 per row i >= 2: the join MJ_i = min over a of (V_{i-1}[a] + J_i + H_i[a]) if J_i is on; the break
 *     MK_i = X_i + H_i[E] if K_i is on.
 *   A value >= INF means "no path" and is reported as -1.  Every marginal that exists is at most 1 043 202, the bound of
 *     str_er_line_decode, and every unreachable forward value is >= INF.  Every path does exactly one thing at a row and one at a gap:
 *     the minimum over the entries of M_i that exist is cost, and so is the minimum of MJ_i and MK_i over those that exist.
 *   Readings: x_i is the label of the character of the decoded string whose source is exactly i-1 (no flag bit), or 65 if there is
 *     none; d_i = 1 if the string has the source (i-1) | 0x4000, else 0.  M_i[x_i] = cost, and the marginal of the move d_i at gap i is
 *     cost.
 *   Margins: row_margin_i = min over x != x_i with M_i[x] >= 0 of M_i[x] - cost, >= 0; alt_i is the smallest x that attains it.  For
 *     i >= 2, gap_margin_i = (the marginal of the move 1 - d_i) - cost if that move is on, else -1: no alternative.  The first row of a
 *     line has no gap: its gap_margin is -1 and its gap_move 0xFF.
 *   Record: read_margin, row, read, alt: the smallest row margin, at the smallest line-relative row.  gap_margin, gap, gap_move: the
 *     smallest gap margin that exists, at the smallest line-relative row i-1, with d of that gap; all three -1 if no gap has an
 *     alternative.  margin: the smaller of read_margin and gap_margin where both exist, else read_margin.  All eight fields are -1 for
 *     n = 0 and for n > 1024 (not decoded).
 *   Per row, indexed like word_of_row (the row of the line's window, not the cost row behind a row map): row_margin (int32, -1 where
 *     nothing is written), row_read and row_alt (uint8, 0xFF), gap_margin (int32, -1), gap_move (uint8: 0 join, 1 break, 0xFF).  On
 *     request, from str_er_line_margins only: the marginals, 68 int32 per row: [0 .. 64] the row read as b, [65] dropped, [66] the join
 *     and [67] the break in front of it; -1 where there is none.
 *   It follows: (1) with (0, off) at every gap and n <= 32, row_margin, row_read, row_alt and the marginals [0 .. 65] equal
 *     str_er_word_margin's on the same rows, and every gap_margin is -1.  (2) With (0, off) inside the words of a segmentation and
 *     (off, 0) at its word gaps, every word of <= 32 rows: the row outputs of a row equal the word margin's row outputs of its word,
 *     and its marginals are the word's plus the other words' costs.  (3) For a gap whose margin g >= 0: the same line decoded again
 *     with only the decided move of that gap set to 255 costs exactly cost + g.  So, all else fixed, the decision flips exactly when
 *     the byte of the decided move rises by more than g.
 *   Limits: an inserted character has no row, so it has no margin of its own, and paths that differ only in insertions are not told
 *     apart.  One gap or one row is varied at a time.  This covers the line decoder only: no lattice, no tracks, no pool.  Nothing is
 *     calibrated: a margin is a cost difference in the unit of the cost rows and the gap bytes, not a probability.                  */
typedef struct str_er_line_margin {
    int32_t  margin, read_margin;         /*  0,  4                                   */
    int32_t  row, read;                   /*  8, 12                                   */
    int32_t  alt, gap_margin;             /* 16, 20                                   */
    int32_t  gap, gap_move;               /* 24, 28                                   */
} str_er_line_margin;        /* 32 bytes; one per line of str_er_result_texts()       */

/* The decoding of a word track without a lexicon (STR_ER_WANT_TRACK_DECODE, str_er_decode_tracks): one string for all members of a
 * word track of str_er_word_link, a median string of the members under their cost rows and the bigram table, reached from the members'
 * own decoder strings by single edits.  A definition of this library; integers only, exact, and the host states the same rules
 * (str_er_decode_tracks_host).
 *   Members: a track with the members w_1 .. w_n is given as for str_er_match_tracks.  Member i has m_i cost rows C_i, the rows the
 *     decoder read for that word: the unfolded 65-byte rows of str_er_word_decode, with STR_ER_WANT_RUN_SPLIT those of its parts; they
 *     are never folded.  A member is usable iff m_i <= 32.  A track has at most 1024 members (STR_ER_ECAPACITY above): the loop over
 *     the members runs inside one workgroup, so the track match's bound of 65536 does not carry over; the int32 sums are safe far
 *     beyond this bound.
 *   Parameters: INS and DEL in 1 .. 255, 64 each by default, and rounds in 0 .. 64, 8 by default (str_er_set_track_decode).  The
 *     table B is the context's (str_er_set_bigram).
 *   Score of a string s of length l, 1 <= l <= 32, over the labels 0 .. 64, with E = 65: lm(s) = B[E][s_1] + the sum over j of
 *     B[s_j][s_{j+1}] + B[s_l][E].  A_i(s) = D[m_i][l] of the recurrence of str_er_word_match on C_i with this output's INS and DEL,
 *     no band and no fold.  J(s) = lm(s) + the sum of A_i(s) over the usable members.  Every term is at most 32 * 255 * 2: with 1024
 *     members J stays far inside int32.
 *   Seeds: the first 32 usable members, in slot order, whose str_er_word_decode string -- made on these rows with the INS / DEL of
 *     str_er_set_word_decode -- has 1 .. 32 characters; duplicates count as they come.  s^0 is the seed with the smallest (J, seed
 *     rank), the set median; seed_cost = J(s^0), seed_member that member's word index.  A track without a seed is not decoded: cost,
 *     seed_cost and lm_cost are -1, n_chars = n_edits = converged = 0, seed_member = -1 and every member cost is -1; n_used is still
 *     made.
 *   Polish: for round r = 1 .. rounds, the neighbours of the current s of length l, positions j from 0: SUB(j, a), s_j replaced by a
 *     (j < l, a in 0 .. 64), has the index j * 65 + a; DEL(j), s_j removed (j < l, only if l > 1), the index 2080 + j; INS(j, a), a
 *     inserted before position j (j <= l, only if l < 32), the index 2112 + j * 65 + a.  The step is the neighbour with the smallest
 *     (J, index).  If its J is strictly below J(s) it becomes s and n_edits grows by one; otherwise the search stops with
 *     converged = 1.  After `rounds` rounds without that stop converged = 0; rounds = 0 leaves the set median with converged = 0.  (A
 *     neighbour equal to s is never taken.)
 *   Record: cost = J(s), lm_cost = lm(s), n_chars = l, n_used the number of usable members.  Per slot of the member array
 *     member_cost = A_i(s), -1 for an unusable member, in a slot of no track and where nothing was decoded.  Per track 32 bytes of
 *     labels, padded with 0xFF.  Hence cost = lm_cost + the sum of the member costs >= 0; cost <= seed_cost <= J(every seed);
 *     converged = 1 implies that no neighbour scores below cost; rounds = 0 gives the winning seed's decoder string byte for byte;
 *     and for a track of one usable member decoded with the decoder's INS = DEL = 0, seed_cost <= that word's str_er_word_decode
 *     cost (the diagonal alignment is one of the alignments).
 *   Limits: this is a local optimum of single edits from the set median, not the global median string.  The members enter with the
 *     rows the decoder read; a joint search over the members' piece lattices is not part of it: it is a separate output, str_er_lattice_track_decode.  Nothing is pooled across calls by this output: a decode
 *     pool (str_er_pool_decode) keeps the newest members of a track on the device and decodes them, call after call.
 *     Whether the polish helps on real text has not been measured, and nothing here is tuned on labelled data.                      */
typedef struct str_er_track_decode {
    int32_t  cost, seed_cost;             /*  0,  4                                   */
    int32_t  n_chars, n_edits;            /*  8, 12                                   */
    int32_t  converged, n_used;           /* 16, 20                                   */
    int32_t  seed_member, lm_cost;        /* 24, 28                                   */
} str_er_track_decode;       /* 32 bytes; one per word track                          */

/* The splitting of touching glyphs (str_er_feet_split, str_er_split_words): candidate cut columns inside a glyph run, the pieces they
 * make, the reading of every piece, and per run the segmentation the scorer likes best (STR_ER_WANT_RUN_SPLIT).  A definition of this library, like the word
 * gap and the reading of a run: exact integers, not tuned on labelled data; the host states the same rules (str_er_cuts_from_counts,
 * str_er_split_words_host).
 *   Column profile of a run r of line t with the frame columns [x0, x1) and rows [y0, y1): W = x1 - x0, H = y1 - y0, and n(c),
 *     0 <= c < W, the number of pixels of F(t) in the frame column x0 + c (>= 1 by the definition of a run).  Only line t's own
 *     footprint counts.
 *   Threshold: thr = floor(H * num / den) in 64-bit integers; num / den is set with str_er_set_run_split, 1 <= num, den <= 65535,
 *     1 / 4 by default.
 *   Valley: a maximal interval [a, b) of columns with n(c) <= thr throughout, with a > 0 and b < W: an interval that touches either
 *     end of the run is no valley.  Its depth d = min n(c) over the interval; its cut column p = floor((cf + cl) / 2), cf and cl the
 *     first and the last column of the interval that attain d.  p lies in the valley and need not attain d itself.
 *   Cuts: the valleys' cut columns; of more than 3 valleys the 3 with the smallest (d, p) are kept.  The kept cuts p_1 < .. < p_k
 *     (k <= 3) split the run into A = k + 1 atoms [0, p_1), [p_1, p_2), .., [p_k, W).  A run with W > 1024 is not split (k = 0);
 *     thr = 0 gives no valley.
 *   Pieces: the nodes are 0 .. A, the piece (i, j), i < j, is the union of the atoms i .. j - 1.  (0, A) is the run itself and is not
 *     listed again, so a cut run has A (A + 1) / 2 - 1 pieces: 2, 5 or 9, ordered by (i, j).  A piece carries its frame columns, its
 *     pixel count and its own tight row extent over the pixels of F(t) in its columns.  The pieces of all runs lie back to back in
 *     run order.
 *   Reading of a piece: the definition of str_er_run_read with the piece's box as the tile: the same T(i, j) rule (0 in F(t), else
 *     255), the line's slope, the same scorer.  The cost row of a piece is that of str_er_word_match, never folded.
 *   Segmentation of a run: m(i, j) is the minimum of the 65 bytes of the cost row of piece (i, j), for (0, A) of the run's own row.
 *     D[0] = 0, D[j] = min over 0 <= i < j of D[i] + m(i, j) + (i > 0 ? SPLIT : 0), the predecessor the smallest i that attains the
 *     minimum; the parts of the run are the pieces on the backtrack from A.  SPLIT is in 0 .. 255 and 8 by default (one bit: a split
 *     must double the product of the parts' best probabilities).  The minimum of a folded row equals that of the unfolded row, so a
 *     lexicon's fold flag does not enter.
 *   Split word: the parts of a word's runs in run order are its split sequence, each part (run, piece) with piece = -1 for a whole
 *     run.  Per word: first_part and n_parts, cost = the sum of the parts' m plus the SPLIT terms, read_cost = the sum of the runs'
 *     own minima (the matcher's free_cost).  Hence cost <= read_cost and n_parts >= n_runs.  The string of a split word is the first
 *     arg min of the row of each part.
 *   Limits: at most 3 cuts a run; the cut follows the upright column profile, no slanted or curved cuts; the segmentation is chosen
 *     per run from the scorer alone, ahead of any lexicon or bigram table: this output makes no joint decode over the piece lattice.
 *     That is a separate output, str_er_lattice_decode (STR_ER_WANT_LATTICE_DECODE): one pass per word over all pieces under the table;
 *     and, against the lexicon, str_er_lattice_match (STR_ER_WANT_LATTICE_MATCH): every entry over all pieces of the word.
 *   Beside the matcher and the decoder: with STR_ER_WANT_RUN_SPLIT next to STR_ER_WANT_WORD_MATCH or _WORD_DECODE both run on the split
 *     sequence instead of the runs: m in their contracts is n_parts, with the same limit of 32, and src of the decoder indexes the
 *     word's parts.  run_costs and run_probs stay per run; the rows of the pieces (str_er_result_piece_costs) are folded where the
 *     runs' are (a lexicon with the fold-case flag), which moves no minimum.  Without STR_ER_WANT_RUN_SPLIT nothing of theirs changes.  */
typedef struct str_er_run_split {
    int32_t  n_cuts;                      /*  0: 0 .. 3                               */
    int32_t  cut[3];                      /*  4: frame columns, ascending, -1 unused  */
    uint32_t thr;                         /* 16                                       */
    int32_t  first_piece, n_pieces;       /* 20, 24: into the piece table             */
    int32_t  n_parts;                     /* 28: parts of its segmentation (0 where no model ran) */
} str_er_run_split;          /* 32 bytes; one per run                                 */
typedef struct str_er_run_piece {
    int32_t  run;                         /*  0: index into the run table             */
    int32_t  from, to;                    /*  4,  8: the nodes i < j                  */
    int32_t  x0, x1;                      /* 12, 16: frame columns, half open         */
    int32_t  y0, y1;                      /* 20, 24: frame rows, half open            */
    uint32_t pixels;                      /* 28                                       */
} str_er_run_piece;          /* 32 bytes */
typedef struct str_er_split_part {
    int32_t  run, piece;                  /*  0,  4: piece -1: the whole run          */
} str_er_split_part;         /*  8 bytes */
typedef struct str_er_word_split {
    int32_t  first_part, n_parts;         /*  0,  4: into the part table              */
    int32_t  cost, read_cost;             /*  8, 12                                   */
} str_er_word_split;         /* 16 bytes; one per word                                */
#define STR_ER_RUN_SPLIT_MAX_W 1024

/* The joint decode of a word over its piece lattice and the bigram table (STR_ER_WANT_LATTICE_DECODE, str_er_lattice_decode_words): one
 * Viterbi pass per word over the lattice of all pieces of all its runs, under the table of str_er_word_decode; the segmentation of the
 * runs and the string come out together.  A definition of this library; integers only, exact, and the host states the same rules
 * (str_er_lattice_decode_words_host).
 *   Lattice of a word with the runs r = 0 .. R-1: run r has k_r kept cuts (str_er_run_split.n_cuts), A_r = k_r + 1 atoms and the local
 *     nodes 0 .. A_r.  The word's nodes are 0 .. N, N = sum of A_r, off_r = sum of A_r' over r' < r: local node i of run r is the
 *     word's node off_r + i, and local node A_r of run r is local node 0 of run r + 1.  The edges are the pieces (i, j),
 *     0 <= i < j <= A_r, of every run, from node off_r + i to node off_r + j; no edge crosses a run boundary.  The row C_{r,i,j} of an
 *     edge is the unfolded 65-byte cost row of that piece, for (0, A_r) the run's own row.  The penalty of an edge is s = SPLIT if
 *     i > 0, else 0: the term of str_er_run_split, with the SPLIT of str_er_set_run_split.
 *   Symbols, the table B (66 x 66, E = 65), INS, DEL and INF = 2^20 are those of str_er_word_decode; INS and DEL come from
 *     str_er_set_word_decode.
 *   Recurrence, in int32: V_0[E] = 0, V_0[a] = INF for a < 65.  For n = 1 .. N, in run r with the local index j = n - off_r:
 *     U_n[x] = INF for all x in 0 .. 65; then for i = 0 .. j - 1 in ascending order, with f = off_r + i: SUB, for b < 65:
 *     S = min over a in 0 .. 65 of (V_f[a] + B[a][b]) + C_{r,i,j}[b] + s, the predecessor the smallest a that attains the minimum;
 *     if S < U_n[b] then U_n[b] = S with the move (SUB, i, a).  DEL, if DEL > 0, for a in 0 .. 65: D = V_f[a] + DEL + s; if
 *     D < U_n[a] then U_n[a] = D with the move (DEL, i).  The comparisons are strict: on equal values the smaller i wins, then SUB
 *     before DEL, then the smaller a.  INS on U_n gives V_n exactly as in str_er_word_decode: if INS > 0, for c < 65:
 *     I = min over b in 0 .. 64 of (U_n[b] + B[b][c]) + INS, with the smallest b; if I < U_n[c] then V_n[c] = I and the move is INS,
 *     else V_n[c] = U_n[c]; always V_n[E] = U_n[E]: at most one inserted character per node.  cost = min over a in 0 .. 65 of
 *     V_N[a] + B[a][E], with the smallest a; for N = 0 that is B[E][E].  INF is never the minimum, and every value is below 2^21.
 *   Backtrack from the end state by the recorded moves, as in str_er_word_decode; a SUB or DEL step at node n also goes to the node
 *     off_r + i.  The edges on the path, in word order, are the word's lattice parts, each (run, piece) as str_er_split_part with
 *     piece = -1 for a whole run and the indices of str_er_result_split_parts.  The string has at most 2N <= 64 labels; the source
 *     byte of a label is the word-relative index of the part it came from, bit 7 set on an inserted character (the part that ends at
 *     the node it was inserted at).  Per word 64 bytes of labels and 64 bytes of sources, padded with 0xFF past n_chars.
 *   Record: read_cost is str_er_word_decode's read_cost on the word's unsplit runs and is made for every word.  Hence
 *     cost <= read_cost, n_sub + n_ins = n_chars, n_sub + n_del = n_parts and n_runs <= n_parts <= N.  A word with N > 32 is not
 *     decoded: cost = -1, the four counts and n_parts are 0.
 *   It follows: (1) if no run of the word has a cut, record, labels and sources equal str_er_word_decode's on the runs byte for
 *     byte, and the parts are the runs; (2) cost <= the str_er_word_decode cost of the word on its runs; (3) cost <= the
 *     str_er_word_decode cost on the split sequence of str_er_run_split plus SPLIT * (n_parts of that sequence - n_runs) -- both are
 *     paths of the lattice (where those words are decoded at all).
 *   Limits: the lattice is that of str_er_run_split (at most 3 upright cuts a run); one path per word -- how far the next reading
 *     and the next cut of every part lie from it is a separate output, str_er_lattice_margin (str_er_set_lattice_margin); no lexicon
 *     enters here: the lexicon over the same lattice is a separate output, str_er_lattice_match (STR_ER_WANT_LATTICE_MATCH), while
 *     str_er_word_match still reads the split sequence of str_er_run_split.  A word is what the word gap made of the line before any
 *     table was asked: the cuts chosen together with the word breaks of the line are a separate output, str_er_line_lattice_decode
 *     (str_er_lattice_decode_lines).                                                                                                   */
typedef struct str_er_lattice_decode {
    int32_t  cost, read_cost;             /*  0,  4                                   */
    int32_t  n_chars, n_sub;              /*  8, 12                                   */
    int32_t  n_del, n_ins;                /* 16, 20                                   */
    int32_t  first_part, n_parts;         /* 24, 28: into the lattice part table      */
} str_er_lattice_decode;     /* 32 bytes; one per word                                */

/* The joint decode of a text line over the piece lattices of its runs (str_er_lattice_decode_lines), here called
 * str_er_line_lattice_decode: one Viterbi pass per line over the atoms' ends of all its runs, under the table of str_er_word_decode.
 * The cuts of touching glyphs, the word breaks and the string come out together: inside a run it takes the edges of
 * str_er_lattice_decode, between two runs the gap step of str_er_line_decode.  A definition of this library; integers only, exact, and
 * the host states the same rules (str_er_lattice_decode_lines_host).
 *   Inputs: symbols, the table B (66 x 66, E = 65), INS, DEL, INF = 2^20, the unfolded 65-byte rows of runs and pieces and SPLIT are
 *     those of str_er_lattice_decode.  The gap pairs (J, K), 255 meaning the move is off, are those of str_er_line_decode, but here
 *     there is one pair per run, for the gap in front of it: the pair of a line's first run is ignored, and a pair of a later run of a
 *     line with both moves off is STR_ER_EINVAL.
 *   Nodes: the atoms' ends of the runs of the line, in order.  Run r has A_r = n_cuts + 1 <= 4 atoms and the local nodes 0 .. A_r; the
 *     line's nodes are 0 .. N, N = sum of A_r, off_r = sum of A_r' over the line's runs r' < r.  A line of more than 1024 runs is not
 *     decoded: cost = -1, the counts 0, labels 0xFF, sources 0xFFFF, no parts.  So a decoded line has at most 4096 nodes.
 *   Recurrence, in int32: V_0 is that of str_er_line_decode (V_0[E] = 0, INF elsewhere).  For every run of the line in turn:
 *     Gap step, for every run but the first, on V at the run's local node 0 (node off_r): exactly the gap step of str_er_line_decode.
 *     W[a] = V[a] + J for all a, or INF exactly if J is off; if K is on, X = min over a in 0 .. 65 of (V[a] + B[a][E]) + K at the
 *     smallest a, and if X < W[E] then W[E] = X and the gap breaks: the comparison is strict, on a tie the join stays; a break from
 *     a = E is allowed.  W replaces V at that node: no edge crosses a run boundary, so V before the gap has no other reader.
 *     Node step, for the local nodes j = 1 .. A_r: exactly the step of str_er_lattice_decode at n = off_r + j, with the edges (i, j),
 *     i < j, from the gapped local node 0 and the later local nodes; the row of an edge is that of the piece (i, j) in the order of
 *     str_er_run_split, the run's own row for (0, A_r); SPLIT is added where i > 0; SUB over the predecessors 0 .. 65 with U[E] = INF,
 *     DEL costs V_i[a] + DEL + s; on equal values the smaller i wins, then SUB before DEL, then the smallest a; then INS over b < 65
 *     on a strict comparison.  cost = min over a of V_N[a] + B[a][E] at the smallest a; a line without runs costs B[E][E].
 *   Bounds: the path that takes every run whole and reads it is a path of str_er_line_decode on 1024 rows, 510 + 1019 * 1023 + 255 =
 *     1 043 202 < 2^20 at the most, so INF is never the minimum; every value stays below 2^20 + 4096 * (509 + 510 + 255 + 510) + 255 =
 *     8 356 095 < 2^25.
 *   Backtrack from the end state by the recorded moves as in str_er_lattice_decode, per node, a SUB or DEL step from the local node i
 *     going to the node off_r + i; where that is local node 0 of a run but the line's first, the state is E and the gap broke, a blank
 *     is emitted and the state becomes the break's predecessor (the check of str_er_line_decode).
 *   Outputs: one record per line; n_sub + n_ins + n_breaks = n_chars and n_sub + n_del = n_parts, runs of the line <= n_parts <= N.
 *     Labels (uint8, 65 = blank) and sources (uint16) lie in a slice of 3 entries per node at the line's node slot -- the number of
 *     atoms of all runs before the line's first run, so the slice begins at entry 3 * slot -- padded with 0xFF / 0xFFFF; a line emits
 *     at most 2 * n_parts + runs - 1 <= 3N - 1 entries.  A source is the line-relative index p of a part: p for the character read
 *     from it, p | 0x8000 for a character inserted behind it, p | 0x4000 for the blank in front of it.  The parts are
 *     str_er_split_part {run, piece} in line order, the lines' back to back (first_part, n_parts); with them one int32 per part,
 *     word_of_part: the number of breaks before it, or -1 for a dropped part.
 *   It follows: (1) if no run has a cut, cost, labels, sources and word indices equal str_er_line_decode's on the runs' rows and the
 *     same pairs, byte for byte; (2) with the pair (0, off) at every gap and at most 32 atoms, cost, labels, parts and counts equal
 *     str_er_lattice_decode's on the same word; (3) with (0, off) inside the words of a segmentation into words of at most 32 atoms
 *     and (off, k) at its word gaps, cost = the sum of those words' str_er_lattice_decode costs + the sum of k, the labels are the
 *     words' joined by one 65 and the parts their concatenation, for any table, B[E][E] != 0 included; (4) for any gap costs with
 *     both moves on, cost <= the str_er_line_decode cost on the runs' rows; (5) cost <= the str_er_line_decode cost over the parts of
 *     str_er_run_split on the same rows (gaps inside a run (0, 255)) + SPLIT * (those parts - runs): both are paths of this decoder.
 *   Limits: one path per line; no margins, tracks, pool or lexicon for it; the weight of the gap costs is not calibrated; the lattice
 *     is that of str_er_run_split (at most 3 upright cuts a run).                                                                     */
typedef struct str_er_line_lattice_decode {
    int32_t  cost, n_chars;               /*  0,  4                                   */
    int32_t  n_breaks, n_sub;             /*  8, 12                                   */
    int32_t  n_del, n_ins;                /* 16, 20                                   */
    int32_t  first_part, n_parts;         /* 24, 28: into the line lattice part table */
} str_er_line_lattice_decode; /* 32 bytes; one per line                               */

/* The margins of a word decoded over its lattice (str_er_set_lattice_margin beside STR_ER_WANT_LATTICE_DECODE, str_er_lattice_margins):
 * the min-marginals of the recurrence of str_er_lattice_decode -- for every edge of the word's lattice and every reading of it the cost
 * of the cheapest whole path that takes the edge and reads it that way -- and from them, for every part of the decoded path, how much
 * more the cheapest path costs that reads the part differently (is this character right?) and that cuts the part's atoms differently
 * (is this cut right?).  A definition of this library; integers only, exact, and the host states the same rules
 * (str_er_lattice_margins_host).
 *   Take a word with 1 <= N <= 32 nodes.  The lattice, B, E = 65, INF, INS, DEL, SPLIT, off_r, A_r, the rows C_{r,i,j}, the penalty
 *     s(i) = (i > 0 ? SPLIT : 0) and the forward values V_n, U_n are exactly those of str_er_lattice_decode.  P_f[b] = min over a in
 *     0 .. 65 of (V_f[a] + B[a][b]).
 *   Backward values, in int32: G_N[a] = B[a][E] for a in 0 .. 65.  For n = N .. 1: GU_n[a] = G_n[a]; if INS > 0, for b < 65:
 *     GU_n[b] = min(G_n[b], min over c < 65 of (B[b][c] + G_n[c]) + INS).  A node f < N is local node i of the run r whose edges leave
 *     it (a run boundary off_r is local node 0 of run r): H_f[b] = min over j in i+1 .. A_r of (C_{r,i,j}[b] + GU_{off_r+j}[b]) for
 *     b < 65; G_f[a] = min over b < 65 of (B[a][b] + H_f[b]) + s(i); if DEL > 0, G_f[a] is also min-ed with DEL + s(i) + min over j of
 *     GU_{off_r+j}[a].  It follows that G_0[E] = cost, and min over a of (V_n[a] + G_n[a]) is the cheapest path through node n: >= cost
 *     for every node, and cost at every run boundary.
 *   Edge marginals, 66 per edge e = (r, i, j), with f = off_r + i and n = off_r + j: M_e[b] = P_f[b] + C_e[b] + s(i) + GU_n[b] for
 *     b < 65, the edge taken and read as b; M_e[65] = min over a in 0 .. 65 of (V_f[a] + DEL + s(i) + GU_n[a]) if DEL > 0, else -1: the
 *     edge taken and dropped.  An entry that is not below INF is -1.  m_e is the minimum of the entries >= 0: the cost of the cheapest
 *     whole path that uses edge e.  Every path covers every atom with exactly one edge, so for every atom the minimum of m_e over the
 *     edges covering it is cost.  Every marginal that exists is at most 32 * 5 * 255 + 255 = 41055; INF never wins.
 *   Parts: the decoded path has the parts k = 0 .. n_parts - 1, part k on the edge e_k = (r_k, i_k, j_k).  x_k is the label of the
 *     decoded character whose source byte is k with bit 7 clear, or 65 if there is none.  M_{e_k}[x_k] = cost.
 *   Reading margin: read_margin_k = min over x != x_k with M_{e_k}[x] >= 0 of M_{e_k}[x] - cost: >= 0, and 0 on a tie; alt_k is the
 *     smallest such x that attains it (there are 65 labels: it always exists).
 *   Cut margin: cut_margin_k = min of m_e' - cost over the edges e' = (r_k, i', j') != e_k with i' < j_k and j' > i_k, the other edges
 *     over the part's atoms -- none of them is on the path; -1 if there is none, which happens exactly when A_r = 1.
 *     cut_alt_k = i' | j' << 4 of the smallest (i', j') that attains it, 0xFF if none.
 *   Record: read_margin is the smallest reading margin, read_part the smallest part that attains it, read and alt those of that part.
 *     cut_margin is the smallest cut margin >= 0, cut_part the smallest part that attains it and cut_alt that part's; all three -1 if
 *     no run of the word is cut.  n_edges is the number of edges of the lattice.  cut_margin + cost is the cost of the cheapest path
 *     whose part sequence differs from the decoded one: such a path uses an edge that is not on the path, and every such edge lies over
 *     the atoms of some part.  All fields are -1 (and n_edges is 0) for N = 0 and for N > 32 (not decoded).
 *   Per word, beside the record, in a layout fixed per word: 32 int32 reading margins and 32 int32 cut margins, -1 past n_parts; 32
 *     bytes each of readings, alternatives and cut alternatives, 0xFF past n_parts.  On request, from str_er_lattice_margins only:
 *     edge_min, int32 [32][4], entry [n-1][i] the m_e of the edge from the local node i into the word's node n, -1 where there is no
 *     such edge; marginals, int32 [32][4][66], with the same index.
 *   It follows: if no run of the word is cut, the reading margins, readings and alternatives equal str_er_word_margin's row outputs on
 *     the runs byte for byte, and every cut field is -1 / 0xFF.
 *   Limits: an inserted character has no part, so it has no margin of its own, and paths that differ only in insertions are not told
 *     apart.  This covers the lattice decoder only: no tracks, no pool, no lattice match.  Nothing is calibrated against labelled text:
 *     a margin is a cost difference in the unit of the cost rows, not a probability.                                                */
typedef struct str_er_lattice_margin {
    int32_t  read_margin, read_part;      /*  0,  4                                   */
    int32_t  read, alt;                   /*  8, 12                                   */
    int32_t  cut_margin, cut_part;        /* 16, 20                                   */
    int32_t  cut_alt, n_edges;            /* 24, 28                                   */
} str_er_lattice_margin;     /* 32 bytes; one per word                                */

/* The lexicon match of a word over its piece lattice (STR_ER_WANT_LATTICE_MATCH, str_er_lattice_match_words): for every word the best
 * and the second-best entry of the lexicon when the segmentation of its runs is free, and for the best its segmentation and its
 * alignment.  A definition of this library; integers only, exact, and the host states the same rules
 * (str_er_lattice_match_words_host).
 *   Lattice: that of str_er_lattice_decode.  Run r has A_r = n_cuts + 1 atoms; the word's nodes are 0 .. N, N = sum of A_r, off_r as
 *     there.  The edges are the pieces (i, j) of every run with the row C_{r,i,j}: the run's own row for (0, A_r), else the piece's
 *     row.  The penalty of an edge is s = SPLIT if i > 0, else 0; no edge crosses a run boundary.  SPLIT comes from
 *     str_er_set_run_split; INS, DEL, the band and the fold from str_er_set_word_match and the lexicon.  With the fold a row is read as
 *     min(C[a], C[a']) for the two letters a, a' of a case pair, as in str_er_word_match.
 *   Cost of the entry e of the length l, in int32: D[0][0] = 0 and D[0][j] = j * INS.  For the node n >= 1 in run r with the local
 *     index jl = n - off_r, D[n][j] is the minimum of these candidates, in this order: for i = 0 .. jl - 1 ascending, with
 *     f = off_r + i: SUB(i) = D[f][j - 1] + C_{r,i,jl}[e_j] + s, only for j >= 1; then DEL(i) = D[f][j] + DEL + s; last
 *     INS = D[n][j - 1] + INS, only for j >= 1.  cost(e) = D[N][l].  Equivalently cost(e) is the minimum over all segmentations P of
 *     the word of the str_er_word_match cost of e on the rows of P's parts plus SPLIT * (|P| - n_runs).
 *   Band: an entry is tried iff max(1, R - band) <= l <= min(32, N + band), with R the word's run count: every part count from R to N
 *     is reachable, so this is the union of the matcher's bands over all segmentations.  A word with N > 32 tries nothing; N = 0 (a
 *     word without runs) behaves as the matcher does for m = 0.
 *   Record: (cost, entry) and (second_cost, second_entry) are the two smallest (cost, index) of the entries tried, as in
 *     str_er_word_match, -1 where nothing qualifies; n_tried is the number of entries tried.  free_cost is the word's
 *     str_er_word_split cost, the cheapest segmentation with free characters; it is made for every word, also for N > 32.  The parts of
 *     the winning entry come from a backtrack from (N, l): at every cell the first candidate in the order above that attains D[n][j]
 *     is the move taken.  The edges taken, in word order, are the word's parts: str_er_split_part records with piece = -1 for a whole
 *     run and the indices of str_er_result_split_parts, in a part table of their own, back to back in word order.  n_parts, n_del and
 *     n_ins are 0 where entry is -1; n_parts - n_del characters are substituted, and n_parts - n_del + n_ins = l.
 *   Sources: 32 bytes per word, padded with 0xFF.  The byte for character j of the winning entry is the word-relative index of the part
 *     it was read from; for an inserted character it is 0x80 | (the number of parts that end at or before the node it was inserted at).
 *   It follows: (1) if no run of the word has a cut, the first six fields equal str_er_word_match's on the runs, field for field, and
 *     the parts are the runs; (2) cost <= the str_er_word_match cost on the unsplit runs, wherever that matcher tried anything;
 *     (3) cost <= the str_er_word_match cost on the split sequence of str_er_run_split + SPLIT * (n_parts of that sequence - n_runs):
 *     both are paths of the lattice, and their bands lie inside this one.
 *   Limits: one path per word, for the best entry only; per word and per frame: pooling lattices over a word track is not part of this
 *     output but a separate one, str_er_lattice_track_member (STR_ER_WANT_LATTICE_TRACK); no bigram table enters.                     */
typedef struct str_er_lattice_match {
    int32_t  entry, cost;                 /*  0,  4                                   */
    int32_t  second_entry, second_cost;   /*  8, 12                                   */
    int32_t  free_cost, n_tried;          /* 16, 20                                   */
    int32_t  first_part, n_parts;         /* 24, 28: into the lattice match part table */
    int32_t  n_del, n_ins;                /* 32, 36                                   */
} str_er_lattice_match;      /* 40 bytes; one per word                                */

/* The lexicon match of a word track over the piece lattices of its members (STR_ER_WANT_LATTICE_TRACK, str_er_lattice_match_tracks): one
 * entry per track, chosen by the sum over the members of each member's cheapest segmentation for that entry, and for that entry every
 * member's own parts and alignment.  A definition of this library; integers only, exact, and the host states the same rules
 * (str_er_lattice_match_tracks_host).
 *   Members: a word track with the members w_1 .. w_n is given as for str_er_match_tracks.  Member i has R_i runs; its lattice is that
 *     of str_er_lattice_decode, with N_i nodes; the rows, the fold, INS, DEL, the band and SPLIT are exactly those of
 *     str_er_lattice_match.  A member is usable iff N_i <= 32.
 *   Cost: for an entry e of the length l, L_i(e) is D_i[N_i][l] of the recurrence of str_er_lattice_match, whatever l is, and cost(e)
 *     is the sum of L_i(e) over the usable members.  Equivalently every usable member adds the minimum over its segmentations P of the
 *     str_er_word_match cost of e on the rows of P's parts plus SPLIT * (|P| - R_i).
 *   Tried: e is tried iff max(1, R_i - band) <= l <= min(32, N_i + band) for at least one usable member: a union of the bands of
 *     str_er_lattice_match, which may have gaps.  A member with N_i = 0 behaves as str_er_lattice_match says for N = 0.
 *   Record per track, a str_er_track_match: (cost, entry) and (second_cost, second_entry) are the two smallest (cost, index) over the
 *     tried entries, -1 where nothing qualifies; free_cost is the sum of the str_er_word_split costs of all members, the unusable ones
 *     included; n_tried the number of entries tried; n_used the number of usable members; best_member the word with the smallest member
 *     cost, ties to the earliest slot, -1 where there is none.  A track has at most 65536 members (STR_ER_ECAPACITY above): L_i is at
 *     most the cost of the unsplit path, at most 64 * 255, so the sum stays inside int32.
 *   Record per slot of the member array, a str_er_lattice_track_member: for the winning entry of the slot's track, cost = L_i, and
 *     the parts, n_del and n_ins of member i's own backtrack from (N_i, l) with the first-candidate rule of str_er_lattice_match
 *     (SUB(i) and DEL(i) for i ascending, then INS); word is the member.  For an unusable member or where entry is -1, cost = -1 and
 *     the counts are 0; in a slot of no track word is -1 as well.  The parts are str_er_split_part records in a table of their own,
 *     back to back in slot order; every slot has 32 source bytes with the meaning and the 0xFF padding of str_er_lattice_match.
 *   It follows: (1) a track of one usable member has the first six fields of that word's str_er_lattice_match, and that word's parts,
 *     sources, n_del and n_ins; (2) if no member has a cut, the record and every member cost equal str_er_track_match's on the runs'
 *     rows field for field, and every member's parts are its runs; (3) where every member has N_i <= 32, cost <= the
 *     str_er_track_match cost on the unsplit runs wherever that one tried anything: per entry every term is smaller or equal, and the
 *     entries tried are a superset.
 *   Limits: only the winning entry gets segmentations; a call remembers nothing across calls or stream submissions (a track pool in
 *     lattice mode, str_er_pool_match, pools the summed costs across them); no bigram table enters.                                     */
typedef struct str_er_lattice_track_member {
    int32_t  cost;                        /*  0: L_i of the track's entry, -1 without  */
    int32_t  first_part, n_parts;         /*  4,  8: into the lattice track part table */
    int32_t  n_del, n_ins;                /* 12, 16                                   */
    int32_t  word;                        /* 20: the member (a word index), -1 in a slot of no track */
} str_er_lattice_track_member; /* 24 bytes; one per slot of the member array          */

/* The decoding of a word track over the piece lattices of its members (str_er_set_lattice_track_decode beside STR_ER_WANT_TRACK_DECODE
 * and STR_ER_WANT_LATTICE_DECODE, str_er_lattice_decode_tracks), here called str_er_lattice_track_decode: one string per word track, a
 * local median under the bigram table with every member's segmentation free, and for that string every member's own cuts and
 * alignment -- the consensus string says how each frame's touching glyphs split.  It is the cell track x bigram x lattice of the
 * reading chain.  A definition of this library; integers only, exact, and the host states the same rules
 * (str_er_lattice_decode_tracks_host).
 *   Members: a track with the members w_1 .. w_n is given as for str_er_lattice_match_tracks.  Member i has the lattice of
 *     str_er_lattice_decode on the unfolded 65-byte rows: N_i nodes, the edges (r, i, j) with the rows C_{r,i,j} and the penalty
 *     s = SPLIT for i > 0, else 0.  A member is usable iff N_i <= 32; N_i = 0 is usable.  A track has at most 1024 members
 *     (STR_ER_ECAPACITY above), as in str_er_track_decode.
 *   Parameters: INS, DEL and rounds come from str_er_set_track_decode, SPLIT from str_er_set_run_split, the table B from
 *     str_er_set_bigram.  The seeds' strings are the str_er_lattice_decode strings of the members, made with the INS / DEL of
 *     str_er_set_word_decode.
 *   Score of a string s of length l, 1 <= l <= 32: lm(s) is as in str_er_track_decode.  L_i(s) = D_i[N_i][l] of the recurrence of
 *     str_er_lattice_match on member i's unfolded rows, with this output's INS / DEL, no band and no fold.  J(s) = lm(s) + the sum of
 *     L_i(s) over the usable members.  L_i(s) is at most the cost of inserting every label and deleting every node over its shortest
 *     edges, 32 * 255 + 32 * (255 + 255) = 24480, and lm(s) at most 33 * 255: with 1024 members J <= 25075935 < 2^31, inside int32.
 *   Seeds: the first 32 usable members in slot order whose str_er_lattice_decode string has 1 .. 32 labels (those strings can have up
 *     to 64 labels; longer or empty ones are no seed); duplicates count as they come.  s^0 is the seed with the smallest (J, seed
 *     rank); seed_cost = J(s^0), seed_member that member's word index.  A track without a seed is not decoded, with exactly the "not
 *     decoded" values of str_er_track_decode: cost, seed_cost and lm_cost are -1, n_chars = n_edits = converged = 0, seed_member = -1;
 *     n_used is still made.
 *   Polish: word for word that of str_er_track_decode, with J as above: the same neighbour indices (SUB j * 65 + a, DEL 2080 + j, INS
 *     2112 + j * 65 + a), the smallest (J, index), a strict improvement or stop, converged and n_edits as there.
 *   Record per track: a str_er_track_decode with cost = J(s), lm_cost = lm(s), n_chars = l, n_used the number of usable members, and 32
 *     label bytes padded with 0xFF.
 *   Record per slot of the member array, a str_er_lattice_track_member, for the final string s: cost = L_i(s), and the parts, n_del and
 *     n_ins of member i's backtrack from (N_i, l) with the first-candidate rule of str_er_lattice_match; 32 source bytes with that
 *     contract's meaning and padding; the parts as str_er_split_part in a table of their own, back to back in slot order.  For an
 *     unusable member or an undecoded track, cost = -1 and the counts are 0.  In a slot of no track, word = -1.
 *   It follows: (1) cost = lm_cost + the sum of the member costs; (2) cost <= seed_cost <= J(every seed); (3) n_parts - n_del + n_ins
 *     = n_chars for every usable member of a decoded track; (4) rounds = 0 gives the winning seed's str_er_lattice_decode string byte
 *     for byte; (5) if no member has a cut, the record, the labels and every member cost equal str_er_decode_tracks on the runs' rows
 *     byte for byte, and every member's parts are its runs; (6) a track of one usable member decoded with the decoder's INS = DEL = 0
 *     has seed_cost <= that word's str_er_lattice_decode cost: the decoded path is one alignment; (7) for the final string s taken as
 *     a one-entry lexicon without fold, member i's cost, parts, n_del, n_ins and sources equal str_er_lattice_match_words' on that
 *     word, wherever the band admits l.
 *   Limits: the result is a local optimum of single edits, not the global median string.  Nothing is pooled across calls by this entry
 *     point: the decode pool of rows (str_er_pool_decode) still has no lattice mode, and pooling this decode across calls is a pool of
 *     its own kind, the lattice decode pool (str_er_track_pool_create_lattice_decode).  Nothing here is tuned on labelled text, and
 *     whether the joint search helps on real video has not been measured.                                                            */

typedef struct str_er_plane_info {
    uint32_t frame;
    uint8_t  ch, pyr, reserved0, reserved1;
    int32_t  width, height;
    int32_t  n_created;   /* tree nodes before pruning (all (t,C) pairs)              */
    int32_t  n_kept;      /* nodes with area > MIN_AREA, plus the root                */
    int32_t  n_pool, n_strong, n_weak;
    int32_t  ambiguous;   /* informational: #nodes where >=2 child chains competed
                             in the first NMS pass (the reference's answer depends on
                             its flood's sibling order there).  With
                             sibling_order = 0 those ties were decided exactly by a
                             replay of the reference's flood; 0 = no tie at all       */
    int32_t  root;        /* index of the root in the kept-node table                 */
} str_er_plane_info;

/* STR_ER_STAGE_TRACK / STR_ER_STAGE_GROUP records (described at str_er_result_tracks / str_er_result_texts) */
typedef struct str_er_track {
    double   color1, color2, color3;     /* NaN where the Otsu mask is empty (0.0 / 0 in calc_color) */
    int32_t  cx, cy;
    uint32_t tracked;
    uint32_t reserved;
} str_er_track;
typedef struct str_er_text {
    uint32_t frame;
    uint8_t  pyr, reserved0, reserved1, reserved2;
    int32_t  first, count;
    double   slope;
    int32_t  x, y, w, h;
} str_er_text;
typedef struct str_er_gbound {
    int32_t x, y, w, h, cx, cy;
} str_er_gbound;

/* ---- lifetime --------------------------------------------------------------------- */
/* Fills the reference's own defaults (src/main.cpp:22): 8,120,900000,2,0.7; six
 * planes, one level; capacity 1920x1080x8 frames.                                     */
void str_er_default_params(str_er_params *p);
int  str_er_create(const str_er_params *p, str_er_ctx **out);
void str_er_destroy(str_er_ctx *ctx);
/* Text of the last error on this context ("" if none). ctx may be NULL for create errors. */
const char *str_er_last_error(const str_er_ctx *ctx);
const char *str_er_strerror(int code);
int  str_er_abi_version(void);
/* Settings of the HIP runtime this library works best with, as "NAME=value" (space separated if several): a context uses
 * two HIP streams (three until round 6, and with STR_ER_PRIO_STREAM) and hosts keep several contexts in flight, which the runtime's default of 4 hardware queues serialises
 * (about 8 % in bench.py).  The runtime reads them when it initialises, so they must be in the environment before the
 * process's first HIP call.  The library never sets them by itself; str_er_apply_runtime_hint() does, for a host that
 * opts in: returns 1 if it set something, 0 if the host's environment already decides, < 0 on error.                  */
/* Exact NMS sibling ties (sibling_order = 0): how many planes of this context's calls so far needed the reference's flood order
 * walked on a host core, the host time those walks took in all (ms, summed over planes), and how many host threads the
 * library's process-wide pool for them has at most (the CPUs the process may use -- hardware threads cut down to a container's cgroup CPU quota --, at least 1,
 * at most 64; STR_ER_WALK_THREADS overrides).  Any pointer may be NULL. */
/* (The pool's threads are detached and live as long as the process: do not dlclose() the library once a tie has been walked.) */
int  str_er_tie_stats(const str_er_ctx *ctx, uint64_t *planes_walked, double *walk_ms_total, int32_t *host_threads);
/* What the component-tree passes of this context's last detect call worked on: node records the tile kernel exported (32 bytes each; what
 * k_group_merge / k_resolve / k_reduce read and write), pixel pairs across tile borders (k_seam: two 16-bit seam entries each) and tiles.
 * Measurement aid (bench.py prices the passes against the HBM roofline with it); the reference has no counterpart.  Any pointer may be NULL. */
int  str_er_last_tree_stats(const str_er_ctx *ctx, uint64_t *records, uint64_t *seam_pairs, uint64_t *tiles);
/* The tile trees of the chroma planes (few levels per tile) are built by a second tile kernel, k_tile_tree2 (level by level on bit masks); a tile with
 * more levels / nodes than it takes is handed back to k_tile_tree.  Since the context was created: tiles given to k_tile_tree2, tiles it handed
 * back.  Measurement aid; results do not depend on which kernel built a tile's tree.  Any pointer may be NULL. */
int  str_er_tile2_stats(const str_er_ctx *ctx, uint64_t *tiles, uint64_t *handed_back);
/* Where the groups of tiles of this context's last detect call went.  A large text-like batch (more than 96 planes) sorts its groups by their record count
 * on the device (k_group_bins): per_table[0..3] = the groups k_group_merge joined in its tables of 512 / 1024 / 2048 / 2528 records, one_tile = the groups
 * of a single tile (no inner seam: nobody's); by default the 2048-record list stays empty, its groups are the 2528-record table's.  listed = the groups whose inner seams k_seam_undone joined on the global records instead -- more records than
 * the largest table, or a plane that ran out of node records.  Any other call joins its groups with one table for all (or one per class of plane) and fills
 * `listed` only, the rest is 0.  Measurement aid; results do not depend on where a group went.  Any pointer may be NULL. */
int  str_er_last_group_stats(const str_er_ctx *ctx, uint32_t per_table[4], uint32_t *listed, uint32_t *one_tile);
/* STR_ER_STAGE_OCR is enqueued right behind classify, sized from the previous batch of the context and working on the device's own count of strong / weak
 * ERs (the reference's call site, src/ER.cpp:728-735, has no barrier between the two either); a batch with more ERs than guessed, or whose candidates an NMS
 * tie pass re-made, is scored again after the counters were read.  Since the context was created: batches whose early scores were used, batches scored again.
 * Measurement aid; results do not depend on it.  Any pointer may be NULL. */
int  str_er_ocr_stage_stats(const str_er_ctx *ctx, uint64_t *scored_early, uint64_t *scored_again);
const char *str_er_runtime_hint(void);
int  str_er_apply_runtime_hint(void);
/* Several contexts of a process keep batches in flight on one GPU (bench.py: six).  The GPU shares itself evenly among their kernels, so equal batches
 * that started together finish together -- and then all wait together for whatever their host side does next (the flood order walk of an NMS sibling tie,
 * about 5 ms for a 1080p plane: src/ER.cpp:416-505 depends on the flood's order), with the GPU idle meanwhile: a trace of six 48-frame batches in flight
 * showed no kernel running for 14 % of the time.  With n > 0, at most n detect calls of the process have their batch's kernels on the GPU at a time: a
 * call takes a slot before it enqueues and gives it back when its kernels are done, BEFORE the host-side work that follows, so the waiting calls' kernels
 * run during that work.  Calls of a frame or two (<= 96 planes) do not take part.  n = 0 (the default): no limit.  Process-wide; returns the old value.
 * A scheduling aid only: results do not depend on it.  (No reference counterpart: text_detect is one frame at a time.) */
int  str_er_set_batch_slots(int n);

/* ERFilter::set_thresh_step / set_min_area (src/ER.cpp:21-30) */
int str_er_set_thresh_step(str_er_ctx *ctx, int32_t t);
/* MIN_OCR_PROB, the last constructor argument of ERFilter (inc/ER.h:113; src/main.cpp:22 passes 0.15, the default here) */
int str_er_set_min_ocr_prob(str_er_ctx *ctx, double min_ocr_prob);
int str_er_set_min_area(str_er_ctx *ctx, int32_t m);

/* ---- models: CascadeBoost::load_classifier (src/adaboost.cpp:873-951) --------------- */
int str_er_load_cascade(str_er_ctx *ctx, int which, const char *path);
int str_er_load_cascade_mem(str_er_ctx *ctx, int which, const char *text, size_t len);
/* n_stages / n_stumps of a loaded cascade (0 if not loaded) */
int str_er_cascade_info(const str_er_ctx *ctx, int which, int32_t *n_stages, int32_t *n_stumps);

/* ---- the hot path ------------------------------------------------------------------ */
/* Whole loop of ERFilter::text_detect up to and including classify
 * (src/ER.cpp:39-60) for n_frames interleaved-BGR 8UC3 frames of w*h pixels
 * (stride = bytes per row, frame_pitch = bytes between frames): compute_channels,
 * optional pyramid, then per plane extract -> NMS -> classify.                        */
int str_er_detect_bgr(str_er_ctx *ctx, const uint8_t *bgr, int32_t w, int32_t h,
                      int64_t stride, int64_t frame_pitch, int32_t n_frames,
                      int mem_kind, uint32_t stages, str_er_result **out);

/* The same for NV12 frames -- what a video decoder delivers: a luma plane of h rows, then one interleaved chroma plane
 * (Cb, Cr, Cb, Cr ...) of h / 2 rows, `stride` bytes per row both; w and h even.  The reference has no such input (it decodes to
 * BGR: cv::imread / `cap >> frame`, src/utils.cpp:31, 109); the conversion is BUILD-DEFINED like the pyramid: Y = the luma byte,
 * Cr(x, y) = V(x/2, y/2), Cb(x, y) = U(x/2, y/2) -- the decoder's samples are the channel values, chroma replicated over its 2 x 2
 * block (oracle: ero_nv12_to_ycrcb).  Everything after the three planes is the path of str_er_detect_bgr.  Half the bytes of a BGR
 * frame cross the host link.                                                                                                     */
int str_er_detect_nv12(str_er_ctx *ctx, const uint8_t *nv12, int32_t w, int32_t h,
                       int64_t stride, int64_t frame_pitch, int32_t n_frames,
                       int mem_kind, uint32_t stages, str_er_result **out);

/* The same for a SUBSET of the logical planes of every frame: plane_select[level * n_channels + k] != 0 selects the
 * k-th channel of the context's channel_mask at that pyramid level (n_select = n_pyr_levels * popcount(channel_mask)).
 * Channels and the pyramid are built on the device as far as the deepest selected level; the result holds the selected
 * planes only, in the usual order.  This is how one large frame is split over GPUs plane by plane without a
 * host copy of any plane.  Not with STR_ER_STAGE_TRACK / _GROUP (they read every plane of an image).                        */
int str_er_detect_bgr_planes(str_er_ctx *ctx, const uint8_t *bgr, int32_t w, int32_t h, int64_t stride, int64_t frame_pitch,
                             int32_t n_frames, int mem_kind, uint32_t stages, const uint8_t *plane_select,
                             int32_t n_select, str_er_result **out);

/* The loop body (src/ER.cpp:52-59) for n_planes independent 8UC1 planes of w*h
 * pixels (plane_pitch = bytes between planes).  This is what the reference's direct
 * callers use (src/utils.cpp:680-684, 716-720, 763-769, 940-947, 1386-1388).        */
int str_er_detect_planes(str_er_ctx *ctx, const uint8_t *planes, int32_t w, int32_t h,
                         int64_t stride, int64_t plane_pitch, int32_t n_planes,
                         int mem_kind, uint32_t stages, str_er_result **out);

/* ---- lists of frames of different sizes --------------------------------------------- */
/* One frame (or plane) of a list: `data` = its top-left pixel, in host or device memory as the call's mem_kind says (one kind for
 * the whole list); `stride` = bytes per row, >= 3*w for a BGR frame, >= w for a plane.                                           */
typedef struct str_er_image_ref {
    const uint8_t *data;
    int32_t  w, h;
    int64_t  stride;
} str_er_image_ref;      /* 24 bytes */

/* str_er_detect_bgr for n_frames interleaved-BGR 8UC3 frames that need not share a size -- the reference's image mode works on
 * photographs as they come (src/main.cpp: one cv::imread per file).  The result for frame i is exactly what str_er_detect_bgr gives
 * for that frame alone, with frame = i in the candidates and plane infos: same planes in the same order, same nodes, candidates,
 * scores and records of every stage (all stages allowed).  One launch converts all frames, one launch per further pyramid level
 * resizes them all.  Capacity is the context's: every frame w <= max_width and h <= max_height, n_frames <= max_frames; a
 * violation returns STR_ER_ECAPACITY (STR_ER_EINVAL for bad arguments) with a message naming the frame, and the context stays usable. */
int str_er_detect_bgr_list(str_er_ctx *ctx, const str_er_image_ref *frames, int32_t n_frames,
                           int mem_kind, uint32_t stages, str_er_result **out);

/* str_er_detect_nv12 for n_frames NV12 frames that need not share a size (several cameras, or photographs through a hardware
 * decoder): frames[i].data = the top-left pixel of its luma plane, the interleaved chroma plane follows h rows later (h / 2 rows),
 * stride >= w bytes per row both; w and h even.  The result for frame i is exactly what str_er_detect_nv12 gives for that frame
 * alone, with frame = i.  Capacity rules, error codes and the context after an error: those of str_er_detect_bgr_list.          */
int str_er_detect_nv12_list(str_er_ctx *ctx, const str_er_image_ref *frames, int32_t n,
                            int mem_kind, uint32_t stages, str_er_result **out);

/* str_er_detect_planes for n_planes independent 8UC1 planes of assorted sizes (n_planes <= the context's planes per call:
 * max_frames x channels x levels).  Plane i's result is what str_er_detect_planes gives for it alone, with ch = i & 255 in its plane
 * info and candidates (as for plane i of a str_er_detect_planes call).                                                           */
int str_er_detect_planes_list(str_er_ctx *ctx, const str_er_image_ref *planes, int32_t n_planes,
                              int mem_kind, uint32_t stages, str_er_result **out);

/* ---- single stages, one per remaining ERFilter method ------------------------------ */
/* ERFilter::compute_channels (src/ER.cpp:114-128): planes6 receives the six w*h
 * planes [Y,Cr,Cb,255-Y,255-Cr,255-Cb], each tightly packed (host memory).           */
int str_er_compute_channels(str_er_ctx *ctx, const uint8_t *bgr, int32_t w, int32_t h,
                            int64_t stride, uint8_t *planes6);

/* ERFilter::classify (src/ER.cpp:507-528) on caller-supplied boxes of one host plane:
 * boxes_xywh[4*i..4*i+3] = ER::bound.  cls/score arrays receive n entries.           */
int str_er_classify_boxes(str_er_ctx *ctx, const uint8_t *plane, int32_t w, int32_t h,
                          int64_t stride, const int32_t *boxes_xywh, int32_t n,
                          uint8_t *cls, double *score_strong, double *score_weak);

/* The pixel masks (str_er_mask) of n regions of one host plane, at the context's current thresh_step; the plane is taken as it
 * is (no invert mask).  Of every region only x, y, w, h, level and key are read.  The masks are written back to back in region order:
 * region i's h rows of (w + 31) / 32 words, then region i + 1's; pixels (optional, may be NULL) receives the n popcounts.
 * bits == NULL only reports *n_words.  cap_words too small -> STR_ER_ECAPACITY, *n_words still set.  STR_ER_EINVAL, with a message
 * naming the region, if a box leaves the plane, key lies outside its box, L(key) > level, or level >= highest_level (255 / step + 1).
 * Boxes of any size up to the whole plane (within the context's capacity).                                                   */
int str_er_er_masks(str_er_ctx *ctx, const uint8_t *plane, int32_t w, int32_t h, int64_t stride, const str_er_cand *regions,
                    int32_t n, uint32_t *bits, uint64_t cap_words, uint64_t *n_words, uint32_t *pixels);

/* The descriptors (str_er_shape) of n regions of one host plane, at the context's current thresh_step, into out[0 .. n - 1]: the
 * masks of str_er_er_masks (same regions, same validation and error codes), the plane taken as it is.                          */
int str_er_er_shapes(str_er_ctx *ctx, const uint8_t *plane, int32_t w, int32_t h, int64_t stride, const str_er_cand *regions,
                     int32_t n, str_er_shape *out);

/* The stroke-width descriptors (str_er_stroke) of n regions of one host plane, at the context's current thresh_step, into
 * out[0 .. n - 1]: the masks of str_er_er_masks (same regions, same validation and error codes), the plane taken as it is.          */
int str_er_er_strokes(str_er_ctx *ctx, const uint8_t *plane, int32_t w, int32_t h, int64_t stride, const str_er_cand *regions,
                      int32_t n, str_er_stroke *out);

/* The text map of n regions of one host plane of w x h pixels (the level size) onto an out_w x out_h frame (out_map, out_w * out_h
 * bytes, pitch out_w), by the pixel rule of str_er_frame_map: every output pixel is the OR of values[i] over the regions that cover
 * it, and with ids (then out_ids != NULL, out_w * out_h int32) out_ids the smallest ids[i] of them, -1 if none.  Of every region only
 * x, y, w, h, level and key are read; the masks are those of str_er_er_masks (same validation and error codes), at the context's
 * current thresh_step, the plane taken as it is.                                                                               */
int str_er_text_map_regions(str_er_ctx *ctx, const uint8_t *plane, int32_t w, int32_t h, int64_t stride,
                            const str_er_cand *regions, const uint8_t *values, const int32_t *ids /* or NULL */, int32_t n,
                            int32_t out_w, int32_t out_h, uint8_t *out_map, int32_t *out_ids /* NULL iff ids is NULL */);

/* The duplicate threshold num / den of STR_ER_WANT_FRAME_LINES and str_er_line_feet_regions (str_er_line_foot): 1 <= num <= den <=
 * 65535, default 1 / 2.  Anything else -> STR_ER_EINVAL, the context unchanged.  A stream's contexts: str_er_stream_context.        */
int str_er_set_frame_merge(str_er_ctx *ctx, int32_t num, int32_t den);
/* The footprints and overlaps (str_er_line_foot) of n_lines lines made of n regions of one host plane of w x h pixels (the level
 * size): region i belongs to line line_of[i] in [0, n_lines); all lines count as one frame of out_w x out_h pixels.  Of every region
 * only x, y, w, h, level and key are read; the masks are those of str_er_er_masks (same validation and error codes), at the context's
 * current thresh_step, the plane taken as it is.  feet receives the n_lines records (frame_line as str_er_frame_lines_from_pairs
 * sets it at the context's num / den).  bits receives the footprints themselves: line t's h rows of (w + 31) / 32 32-bit words over
 * its foot box (bit i of word k of row r: frame pixel (x + 32 k + i, y + r); the layout of str_er_mask), back to back in line order;
 * bits == NULL only reports *n_words.  pairs receives the pairs with inter > 0, sorted by (a, b), dup set; pairs == NULL only
 * reports *n_pairs.  cap_words / cap_pairs too small -> STR_ER_ECAPACITY, both counts and feet still set.                          */
int str_er_line_feet_regions(str_er_ctx *ctx, const uint8_t *plane, int32_t w, int32_t h, int64_t stride, const str_er_cand *regions,
                             const int32_t *line_of, int32_t n, int32_t n_lines, int32_t out_w, int32_t out_h, str_er_line_foot *feet,
                             uint32_t *bits, uint64_t cap_words, uint64_t *n_words, str_er_line_pair *pairs, int32_t cap_pairs,
                             int32_t *n_pairs);
/* The frame lines of n_lines lines from their feet and pairs (str_er_line_foot).  Pure host, no context, no GPU; the detect calls use
 * this same function.  frames_of_lines[t], pyr_of_lines[t]: the frame and pyramid level of line t (str_er_text::frame / pyr).  Reads
 * feet[t].x, y, w, h, pixels and pairs[k].a, b, inter; sets pairs[k].dup and feet[t].frame_line, fills frame_lines (at most n_lines
 * of them: cap_frame_lines too small -> STR_ER_ECAPACITY, *n_frame_lines still set; frame_lines == NULL only counts and sets dup)
 * and members (n_lines line indices).  STR_ER_EINVAL: bad arguments, a pair with a >= b or an index outside [0, n_lines), a pair
 * of lines of different frames, inter == 0 or inter larger than either footprint.                                                */
int str_er_frame_lines_from_pairs(str_er_line_foot *feet, const uint32_t *frames_of_lines, const uint8_t *pyr_of_lines, int32_t n_lines,
                                  str_er_line_pair *pairs, int32_t n_pairs, int32_t num, int32_t den, str_er_frame_line *frame_lines,
                                  int32_t cap_frame_lines, int32_t *n_frame_lines, int32_t *members);

/* The link threshold num / den of STR_ER_WANT_LINE_LINKS and str_er_link_feet (str_er_line_link): 1 <= num <= den <= 65535, default
 * 1 / 2.  Anything else -> STR_ER_EINVAL, the context unchanged.  A stream's contexts: str_er_stream_context.                     */
int str_er_set_line_link(str_er_ctx *ctx, int32_t num, int32_t den);
/* The overlaps (str_er_line_link) of every line of set a with every line of set b, two sets of footprints in the pixels of one frame
 * size W x H (1..65535): feet_x[i] is the foot box and pixel count of line i of the set, bits_x its rows of (w + 31) / 32 32-bit words
 * over the box, back to back in set order -- the layout str_er_line_feet_regions and str_er_result_edge_feet return.  pairs receives
 * the records with inter > 0, a an index into set a and b into set b, sorted by (a, b), link set at the context's num / den;
 * pairs == NULL only reports *n_pairs; cap_pairs too small -> STR_ER_ECAPACITY, *n_pairs still set.  STR_ER_EINVAL: bad arguments, a
 * box that leaves the frame, a set bit past a row's width, pixels that are not the number of set bits.  Either set may be empty.  */
int str_er_link_feet(str_er_ctx *ctx, int32_t W, int32_t H, const str_er_line_foot *feet_a, const uint32_t *bits_a, int32_t n_a,
                     const str_er_line_foot *feet_b, const uint32_t *bits_b, int32_t n_b, str_er_line_link *pairs, int32_t cap_pairs,
                     int32_t *n_pairs);
/* The text tracks of n_lines lines from their feet, pairs and links (str_er_line_link).  Pure host, no context, no GPU; the detect
 * calls use this same function.  Reads feet[t].pixels, frames_of_lines[t], pairs[k].a, b, inter, dup and links[k].a, b, inter; sets
 * links[k].link and line_tracks[t] (n_lines track indices), fills tracks (at most n_lines: cap_tracks too small -> STR_ER_ECAPACITY,
 * *n_tracks still set; tracks == NULL only counts, sets link and line_tracks) and members (n_lines line indices).  STR_ER_EINVAL: bad
 * arguments, an index outside [0, n_lines), a pair with a >= b or of two frames, a link whose b is not of the frame after a's,
 * inter == 0 or inter larger than either footprint.                                                                             */
int str_er_text_tracks_from_links(const str_er_line_foot *feet, const uint32_t *frames_of_lines, int32_t n_lines,
                                  const str_er_line_pair *pairs, int32_t n_pairs, str_er_line_link *links, int32_t n_links, int32_t num,
                                  int32_t den, int32_t *line_tracks, str_er_text_track *tracks, int32_t cap_tracks, int32_t *n_tracks,
                                  int32_t *members);

/* The geometry (str_er_line_geom) of n footprints in the pixels of one frame size W x H (1..65535), made on the GPU: feet[i] is the
 * foot box and pixel count of line i, bits its rows of (w + 31) / 32 32-bit words over the box, back to back in line order -- the
 * layout str_er_line_feet_regions and str_er_result_edge_feet return and str_er_link_feet takes; validation and error codes are
 * those of str_er_link_feet, and a foot box wider or taller than 16384 gives STR_ER_ECAPACITY.  geoms receives n records, xy the
 * vertices (x, y pairs) they index, *n_points their number; xy == NULL only counts (geoms is still filled); cap_points too small ->
 * STR_ER_ECAPACITY, *n_points still set.                                                                                          */
int str_er_feet_geom(str_er_ctx *ctx, int32_t W, int32_t H, const str_er_line_foot *feet, const uint32_t *bits, int32_t n,
                     str_er_line_geom *geoms, int32_t *xy, int32_t cap_points, int32_t *n_points);
/* The strictly convex hull of n points (x, y pairs, any int32), in the vertex order of str_er_line_geom.  Pure host, no context, no
 * GPU; the detect calls merge the hulls of a frame line with this same function.  out_xy == NULL only counts; cap too small ->
 * STR_ER_ECAPACITY, *n_out still set.  One point gives one vertex, collinear points their two ends.  STR_ER_EINVAL: bad arguments. */
int str_er_hull_of_points(const int32_t *xy, int32_t n, int32_t *out_xy, int32_t cap, int32_t *n_out);
/* hull_area2, edge, ex, ey, dmin .. cmax, qx and qy of *out (str_er_line_geom) from a hull of n vertices; the other fields of *out are
 * left as they are.  Pure host, no context, no GPU; the detect calls use this same function.  STR_ER_EINVAL: fewer than 3 vertices,
 * a hull that is not strictly convex in the order of str_er_line_geom, coordinates outside 0..65535.                               */
int str_er_quad_from_hull(const int32_t *xy, int32_t n, str_er_line_geom *out);

/* The gap that breaks a word (str_er_line_run): num / den of the line's colmax, 1 <= num, den <= 65535.  Default 1 / 3.  Anything else
 * -> STR_ER_EINVAL, the context unchanged.  A stream's contexts: str_er_stream_context.                                            */
int str_er_set_word_gap(str_er_ctx *ctx, int32_t num, int32_t den);
/* The glyph runs and words (str_er_line_run) of n footprints in the pixels of one frame size W x H (1..65535), the runs made on the
 * GPU: feet and bits as str_er_feet_geom and str_er_link_feet take them, with their validation and error codes; a foot box wider or
 * taller than 16384 gives STR_ER_ECAPACITY.  line_words receives n records, runs and words the tables they index, *n_runs and
 * *n_words their sizes; runs == NULL or words == NULL only counts (line_words is still filled); cap_runs or cap_words too small ->
 * STR_ER_ECAPACITY, both counts still set.  The words are those of str_er_words_from_runs with the context's word gap.             */
int str_er_feet_words(str_er_ctx *ctx, int32_t W, int32_t H, const str_er_line_foot *feet, const uint32_t *bits, int32_t n,
                      str_er_line_words *line_words, str_er_line_run *runs, int32_t cap_runs, int32_t *n_runs, str_er_line_word *words,
                      int32_t cap_words, int32_t *n_words);
/* The words of n_lines lines from their runs.  Pure host, no context, no GPU; the detect calls use this same function.  In:
 * line_words[t].first_run, .n_runs and .colmax (the lines' runs back to back in line order: first_run is the sum of the earlier
 * n_runs, and they add up to n_runs) and x0 .. pixels of every run.  Out: the word of every run, first_word and n_words of every line
 * (reserved = 0), and the word records; words == NULL only counts (the runs and line_words are still filled); cap_words too small ->
 * STR_ER_ECAPACITY, *n_words still set.  STR_ER_EINVAL: bad arguments, num or den outside 1..65535, run lists that do not lie back to
 * back, a line with runs and colmax 0, a run with x0 >= x1, y0 >= y1 or pixels == 0, runs of a line out of order, overlapping or
 * touching (every gap is >= 1).                                                                                                    */
int str_er_words_from_runs(str_er_line_run *runs, int32_t n_runs, str_er_line_words *line_words, int32_t n_lines, int32_t num, int32_t den,
                           str_er_line_word *words, int32_t cap_words, int32_t *n_words);
/* The character of a label of the OCR scorer (str_er_run_read): table[label] for 0 <= label < 65 with the reference's table
 * "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz&()" (src/OCR.cpp:10), else '?'.  Pure: no context, no GPU.          */
int32_t str_er_ocr_char(int32_t label);
/* str_er_feet_words and the reading of every run (str_er_run_read): slopes receives one slope per footprint (NULL: all 0; a slope that
 * is not finite -> STR_ER_EINVAL, as in str_er_ocr_chain_run_slope).  reads receives one record per run and q_out (optional) the
 * 1800 feature bytes of every run, both in the order of runs; reads == NULL gives the features only, and no SVM model is needed then
 * (with reads: STR_ER_ESTATE without a model of dim 1800).  Arguments, validation and capacity codes are those of str_er_feet_words:
 * reads and q_out hold cap_runs records / 1800 * cap_runs bytes, and a counting call (runs == NULL or words == NULL) reads nothing. */
int str_er_feet_read(str_er_ctx *ctx, int32_t W, int32_t H, const str_er_line_foot *feet, const uint32_t *bits, const double *slopes, int32_t n,
                     str_er_line_words *line_words, str_er_line_run *runs, int32_t cap_runs, int32_t *n_runs, str_er_line_word *words,
                     int32_t cap_words, int32_t *n_words, str_er_run_read *reads, uint8_t *q_out);
/* Statistics of the tile atlas of STR_ER_WANT_RUN_READ / str_er_feet_read: its size in bytes (0: never made) and how often it was
 * allocated or grown since the context was created.  Either pointer may be NULL.                                                  */
int str_er_run_atlas_stats(const str_er_ctx *ctx, uint64_t *bytes, uint64_t *grown);

/* The lexicon of the context (str_er_word_match): n entries, entry i the bytes [offsets[i], offsets[i + 1]) of `bytes`, the
 * characters themselves ('0' .. '9', 'A' .. 'Z', 'a' .. 'z', '&', '(', ')'); offsets has n + 1 values and starts at 0.  n = 0 clears
 * the lexicon (bytes and offsets may be NULL).  flags: 0 or STR_ER_LEXICON_FOLD_CASE.  STR_ER_EINVAL on a byte outside the alphabet,
 * on a length of 0 or above 32, on offsets that do not lie back to back from 0 and on other flags; STR_ER_ECAPACITY above 2^20
 * entries; the context is unchanged then.  The call waits for the context's work.  A stream's contexts: str_er_stream_context.      */
int str_er_set_lexicon(str_er_ctx *ctx, const char *bytes, const int32_t *offsets, int32_t n, uint32_t flags);
/* The lexicon that is set: its entries, its flags, the chunk size in entries (a workgroup of the matcher takes so many slots of the
 * padded lexicon) and the bytes it takes on the device (0 without one).  Any pointer may be NULL.                                  */
int str_er_lexicon_info(const str_er_ctx *ctx, int32_t *n, uint32_t *flags, int32_t *chunk_entries, uint64_t *device_bytes);
/* INS, DEL (1 .. 255) and the band (0 .. 31) of str_er_word_match; defaults 64, 64, 2.  Anything else -> STR_ER_EINVAL, the context
 * unchanged.  A stream's contexts: str_er_stream_context.                                                                          */
int str_er_set_word_match(str_er_ctx *ctx, int32_t ins, int32_t del, int32_t band);
/* The table T of str_er_word_match.  Pure: no context, no GPU.                                                                     */
void str_er_cost_thresholds(double out[255]);
/* The cost rows (65 bytes each, into cost_out) of n runs from their k class probabilities (prob: n x k) of a model with the given k
 * labels; fold: the fold-case rule.  Pure: no context, no GPU.  STR_ER_EINVAL on NULL or negative arguments.                        */
int str_er_prob_costs(const double *prob, int32_t n, int32_t k, const int32_t *labels, int32_t fold, uint8_t *cost_out);
/* The same on the GPU with the labels of the loaded SVM model (prob: n x nr_class) and the fold-case flag of the lexicon (none: not
 * folded).  STR_ER_ESTATE without a model.                                                                                         */
int str_er_run_costs(str_er_ctx *ctx, const double *prob, int32_t n, uint8_t *cost_out);
/* The matcher on the caller's cost rows: costs holds n_runs rows of 65 bytes, word w has the rows first_run[w] .. first_run[w] +
 * n_runs_of_word[w]; matches receives n_words records.  STR_ER_ESTATE without a lexicon; STR_ER_EINVAL on a word outside the rows.
 * It needs no SVM model.                                                                                                           */
int str_er_match_words(str_er_ctx *ctx, const uint8_t *costs, int32_t n_runs, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words,
                       str_er_word_match *matches);
/* The same rules on one host thread, with the lexicon and the parameters as arguments (as for str_er_set_lexicon and
 * str_er_set_word_match, with their checks).  Pure: no context, no GPU.                                                            */
int str_er_match_words_host(const uint8_t *costs, int32_t n_runs, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, const char *bytes,
                            const int32_t *offsets, int32_t n, uint32_t flags, int32_t ins, int32_t del, int32_t band, str_er_word_match *matches);

/* The link threshold num / den of STR_ER_WANT_TRACK_READ (str_er_word_link): 1 <= num, den <= 65535, default 1 / 2.  Anything else
 * -> STR_ER_EINVAL, the context unchanged.  A stream's contexts: str_er_stream_context.                                            */
int str_er_set_word_link(str_er_ctx *ctx, int32_t num, int32_t den);
/* The reading lines and the word links (str_er_word_link) of n_words words of n_lines lines of n_frames frames.  Pure host, no
 * context, no GPU; the detect calls run the same rules.  Reads feet[t].pixels, frames_of_lines[t] (< n_frames), line_tracks[t]
 * (>= 0: the text track of line t), frame_wh (w, h of every frame at level 0) and words[w].line, x, y, w, h.  reading receives one
 * byte per line, 1 for a reading line; links the records with inter > 0 sorted by (a, b), link set at num / den; links == NULL only
 * reports *n_links; cap_links too small -> STR_ER_ECAPACITY, *n_links still set.  STR_ER_EINVAL: bad arguments, num or den outside
 * 1 .. 65535, a frame, a track or a word's line out of range, a word box with w or h outside 0 .. 65535.                          */
int str_er_word_links(const str_er_line_foot *feet, const uint32_t *frames_of_lines, const int32_t *line_tracks, int32_t n_lines, const int32_t *frame_wh,
                      int32_t n_frames, const str_er_line_word *words, int32_t n_words, int32_t num, int32_t den, uint8_t *reading, str_er_word_link *links,
                      int32_t cap_links, int32_t *n_links);
/* The word tracks (str_er_word_track) from the reading flags and the links of str_er_word_links.  Pure host, no context, no GPU; the
 * detect calls run the same rules.  Reads links[k].a, b, link.  track_of_words receives one track index per word, -1 for a word
 * that is not eligible; tracks at most n_words records (cap_tracks too small -> STR_ER_ECAPACITY, *n_tracks still set; tracks == NULL
 * only counts and sets track_of_words); members the eligible words, at most n_words.  STR_ER_EINVAL: bad arguments, an index out of
 * range, a link between words that are not eligible.                                                                              */
int str_er_word_tracks_from_links(const uint32_t *frames_of_lines, const int32_t *line_tracks, const uint8_t *reading, int32_t n_lines,
                                  const str_er_line_word *words, int32_t n_words, const str_er_word_link *links, int32_t n_links, int32_t *track_of_words,
                                  str_er_word_track *tracks, int32_t cap_tracks, int32_t *n_tracks, int32_t *members);
/* The track match (str_er_track_match) on the caller's cost rows, on the GPU: costs holds n_rows rows of 65 bytes, word w has the
 * rows first_run[w] .. first_run[w] + n_runs_of_word[w] as for str_er_match_words; track g has the members members[track_first[g] ..
 * track_first[g] + track_count[g]) of the member array of n_members word indices; the tracks lie in it in ascending order without
 * overlap.  Any word may appear in any member list, also twice, in which case it counts twice.  out receives n_tracks records,
 * member_cost n_members values (-1 in a slot of no track).  STR_ER_ESTATE without a lexicon; STR_ER_EINVAL on a word outside the rows,
 * a member outside the words, a track outside the member array; STR_ER_ECAPACITY on a track of more than 65536 members.             */
int str_er_match_tracks(str_er_ctx *ctx, const uint8_t *costs, int32_t n_rows, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words,
                        const int32_t *track_first, const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks,
                        str_er_track_match *out, int32_t *member_cost);
/* The same rules on one host thread, with the lexicon and the parameters as arguments (as for str_er_match_words_host).  Pure: no
 * context, no GPU.                                                                                                                */
int str_er_match_tracks_host(const uint8_t *costs, int32_t n_rows, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words,
                             const int32_t *track_first, const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks,
                             const char *bytes, const int32_t *offsets, int32_t n, uint32_t flags, int32_t ins, int32_t del, int32_t band,
                             str_er_track_match *out, int32_t *member_cost);

/* The bigram table of the context (str_er_word_decode): 66 * 66 bytes, copied.  NULL removes the table.  The call waits for the
 * context's work.  A stream's contexts: str_er_stream_context.                                                                     */
int str_er_set_bigram(str_er_ctx *ctx, const uint8_t *cost);
/* Whether a table is set (1 / 0) and the bytes it takes on the device (0 without one).  Either pointer may be NULL.                 */
int str_er_bigram_info(const str_er_ctx *ctx, int32_t *set, uint64_t *device_bytes);
/* INS and DEL (0 .. 255, 0: the move is off) of str_er_word_decode; defaults 0, 0.  Anything else -> STR_ER_EINVAL, the context
 * unchanged.  A stream's contexts: str_er_stream_context.                                                                          */
int str_er_set_word_decode(str_er_ctx *ctx, int32_t ins, int32_t del);
/* A table from probabilities: out[a][b] = cost(tp[a * 65 + b]) with the cost() of str_er_word_match, tp taken as P(b after a);
 * out[E][b] = cost(start[b]) and out[a][E] = cost(end[a]), 0 where start / end is NULL; out[E][E] = 0.  Pure: no context, no GPU.
 * STR_ER_EINVAL on a NULL tp or out.  (See the limits at str_er_word_decode for what is known of the reference's tp_table.txt.)      */
int str_er_bigram_from_probs(const double *tp, const double *start, const double *end, uint8_t out[4356]);
/* The decoder on the caller's cost rows: costs holds n_runs rows of 65 bytes, word w has the rows first_run[w] .. first_run[w] +
 * n_runs_of_word[w]; dec receives n_words records, chars and src 64 bytes per word each.  STR_ER_ESTATE without a table;
 * STR_ER_EINVAL on a word outside the rows.  n_words = 0 is fine.  It needs no SVM model and no lexicon.                             */
int str_er_decode_words(str_er_ctx *ctx, const uint8_t *costs, int32_t n_runs, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words,
                        str_er_word_decode *dec, uint8_t *chars, uint8_t *src);
/* The same rules on one host thread, with the table and INS / DEL as arguments (with the checks of str_er_set_word_decode).  Pure:
 * no context, no GPU.                                                                                                              */
int str_er_decode_words_host(const uint8_t *costs, int32_t n_runs, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words,
                             const uint8_t *bigram, int32_t ins, int32_t del, str_er_word_decode *dec, uint8_t *chars, uint8_t *src);
/* Whether a detect call with STR_ER_WANT_WORD_DECODE also makes the margins of its words (str_er_word_margin): on != 0 switches them
 * on; off by default.  A context setting, not a stage flag: without STR_ER_WANT_WORD_DECODE it does nothing, and while it is off no
 * call does anything more than before.  A stream's contexts: str_er_stream_context.                                                */
int str_er_set_word_margin(str_er_ctx *ctx, int32_t on);
/* The margins (str_er_word_margin) on the caller's cost rows, on the GPU, under the context's table and the INS / DEL of
 * str_er_set_word_decode: the arguments up to n_words and their checks are those of str_er_decode_words, and the decoder runs on
 * these rows first.  margins receives n_words records, row_margin 32 int32 per word, row_read and row_alt 32 bytes per word each,
 * marginals (NULL: not wanted) 32 x 66 int32 per word.  Words may share rows.  STR_ER_ESTATE without a table; STR_ER_EINVAL on a
 * word outside the rows.  n_words = 0 is fine.                                                                                    */
int str_er_word_margins(str_er_ctx *ctx, const uint8_t *costs, int32_t n_runs, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words,
                        str_er_word_margin *margins, int32_t *row_margin, uint8_t *row_read, uint8_t *row_alt, int32_t *marginals);
/* The same rules on one host thread, with the table and INS / DEL as arguments (with the checks of str_er_set_word_decode).  Pure:
 * no context, no GPU.                                                                                                              */
int str_er_word_margins_host(const uint8_t *costs, int32_t n_runs, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words,
                             const uint8_t *bigram, int32_t ins, int32_t del, str_er_word_margin *margins, int32_t *row_margin, uint8_t *row_read,
                             uint8_t *row_alt, int32_t *marginals);
/* Whether a detect call with STR_ER_WANT_WORD_DECODE also decodes every line of str_er_result_texts() (str_er_line_decode), and the
 * weight (0 .. 127) of its gap costs: on != 0 switches it on; off by default, the weight 16.  A weight outside 0 .. 127 ->
 * STR_ER_EINVAL, the context unchanged.  A context setting, not a stage flag: without STR_ER_WANT_WORD_DECODE it does nothing, and while
 * it is off no call does anything more than before.  A stream's contexts: str_er_stream_context.                                  */
int str_er_set_line_decode(str_er_ctx *ctx, int32_t on, int32_t weight);
/* The gap costs of str_er_line_decode from the geometry.  Line t has the rows first_row[t] .. first_row[t] + n_rows_of_line[t] of
 * n_rows rows and the colmax colmax[t] of str_er_line_words; row r belongs to the run row_run[r] of runs (row_run == NULL: row r is
 * run r); num / den is the word gap (1 .. 65535 each), weight is in 0 .. 127.  gaps receives 2 * n_rows bytes, (J, K) per row.  Pure:
 * no context, no GPU.  STR_ER_EINVAL on NULL arguments, a window outside the rows, a row outside the runs, num, den or weight out of
 * range, or a line of more than one run with colmax 0.                                                                           */
int str_er_line_gap_costs(const str_er_line_run *runs, int32_t n_runs, const int32_t *row_run, int32_t n_rows, const int32_t *first_row,
                          const int32_t *n_rows_of_line, const uint32_t *colmax, int32_t n_lines, int32_t num, int32_t den, int32_t weight, uint8_t *gaps);
/* The line decoder (str_er_line_decode) on the caller's cost rows, on the GPU, under the context's table and the INS / DEL of
 * str_er_set_word_decode: costs holds n_rows rows of 65 bytes and gaps 2 * n_rows bytes, line t has the rows first_row[t] ..
 * first_row[t] + n_rows_of_line[t]; the windows lie in ascending order and do not overlap (every line writes its own slice).  dec
 * receives n_lines records, chars 3 * n_rows bytes, src 3 * n_rows uint16 and word_of_row n_rows int32; what lies in no line is
 * 0xFF / 0xFFFF / -1.  STR_ER_ESTATE without a table; STR_ER_EINVAL on NULL arguments, a window outside the rows or out of order, or a
 * gap of a line with both moves off; the context stays usable.  n_lines = 0 is fine.                                               */
int str_er_decode_lines(str_er_ctx *ctx, const uint8_t *costs, int32_t n_rows, const uint8_t *gaps, const int32_t *first_row, const int32_t *n_rows_of_line,
                        int32_t n_lines, str_er_line_decode *dec, uint8_t *chars, uint16_t *src, int32_t *word_of_row);
/* The same rules on one host thread, with the table and INS / DEL as arguments (with the checks of str_er_set_word_decode).  Pure:
 * no context, no GPU.                                                                                                              */
int str_er_decode_lines_host(const uint8_t *costs, int32_t n_rows, const uint8_t *gaps, const int32_t *first_row, const int32_t *n_rows_of_line, int32_t n_lines,
                             const uint8_t *bigram, int32_t ins, int32_t del, str_er_line_decode *dec, uint8_t *chars, uint16_t *src, int32_t *word_of_row);
/* The bytes of the line decoder's back-pointer table on the device (68 uint16 per row of the largest call so far; 0 before the first).  */
int str_er_line_decode_stats(const str_er_ctx *ctx, uint64_t *table_bytes);
/* Whether a detect call that decodes its lines (STR_ER_WANT_WORD_DECODE on a context whose str_er_set_line_decode is on) also makes
 * their margins (str_er_line_margin): on != 0 switches it on; off by default.  A context setting, not a stage flag: without the line
 * decode it does nothing, and while it is off no call enqueues or allocates anything more than before.  A stream's contexts:
 * str_er_stream_context.                                                                                                          */
int str_er_set_line_margin(str_er_ctx *ctx, int32_t on);
/* The line decoder and its margins (str_er_line_margin) on the caller's cost rows, on the GPU, in one enqueue with one wait: the
 * arguments, checks and error codes of str_er_decode_lines.  margins receives n_lines records; row_margin and gap_margin n_rows int32,
 * row_read, row_alt and gap_move n_rows bytes; marginals (NULL: not wanted) 68 * n_rows int32.  What lies in no line is -1 / 0xFF.
 * STR_ER_ECAPACITY where the forward table of the rows would pass 2^31 bytes.                                                     */
int str_er_line_margins(str_er_ctx *ctx, const uint8_t *costs, int32_t n_rows, const uint8_t *gaps, const int32_t *first_row, const int32_t *n_rows_of_line,
                        int32_t n_lines, str_er_line_margin *margins, int32_t *row_margin, uint8_t *row_read, uint8_t *row_alt, int32_t *gap_margin,
                        uint8_t *gap_move, int32_t *marginals);
/* The same rules on one host thread, with the table and INS / DEL as arguments.  Pure: no context, no GPU.                          */
int str_er_line_margins_host(const uint8_t *costs, int32_t n_rows, const uint8_t *gaps, const int32_t *first_row, const int32_t *n_rows_of_line, int32_t n_lines,
                             const uint8_t *bigram, int32_t ins, int32_t del, str_er_line_margin *margins, int32_t *row_margin, uint8_t *row_read,
                             uint8_t *row_alt, int32_t *gap_margin, uint8_t *gap_move, int32_t *marginals);
/* The bytes of the margins' forward table on the device (136 uint32 per row of the largest call so far; 0 before the first).          */
int str_er_line_margin_stats(const str_er_ctx *ctx, uint64_t *table_bytes);
/* INS and DEL (1 .. 255) and the number of polish rounds (0 .. 64) of str_er_track_decode; defaults 64, 64 and 8.  Anything else ->
 * STR_ER_EINVAL, the context unchanged.  A stream's contexts: str_er_stream_context.                                               */
int str_er_set_track_decode(str_er_ctx *ctx, int32_t ins, int32_t del, int32_t rounds);
/* The track decode (str_er_track_decode) on the caller's cost rows, on the GPU, under the context's table, its str_er_set_word_decode
 * (the seeds' strings: the decoder runs on these rows first) and its str_er_set_track_decode: the rows, the words and the tracks are
 * given as for str_er_match_tracks.  out receives n_tracks records, chars 32 bytes per track, member_cost n_members values (-1 in a
 * slot of no track).  STR_ER_ESTATE without a table; STR_ER_EINVAL on a word outside the rows, a member outside the words, a track
 * outside the member array; STR_ER_ECAPACITY on a track of more than 1024 members.  It needs no SVM model and no lexicon.           */
int str_er_decode_tracks(str_er_ctx *ctx, const uint8_t *costs, int32_t n_rows, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words,
                         const int32_t *track_first, const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks,
                         str_er_track_decode *out, uint8_t *chars, int32_t *member_cost);
/* The same rules on one host thread, with the table, the decoder's INS / DEL (dec_ins, dec_del: the checks of str_er_set_word_decode)
 * and this output's parameters (the checks of str_er_set_track_decode) as arguments.  Pure: no context, no GPU.                     */
int str_er_decode_tracks_host(const uint8_t *costs, int32_t n_rows, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words,
                              const int32_t *track_first, const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks,
                              const uint8_t *bigram, int32_t dec_ins, int32_t dec_del, int32_t ins, int32_t del, int32_t rounds,
                              str_er_track_decode *out, uint8_t *chars, int32_t *member_cost);

/* num / den of the valley threshold (1 .. 65535 each) and SPLIT (0 .. 255) of str_er_run_split; defaults 1 / 4 and 8.  Anything else
 * -> STR_ER_EINVAL, the context unchanged.                                                                                          */
int str_er_set_run_split(str_er_ctx *ctx, int32_t num, int32_t den, int32_t split_cost);
/* Statistics of the buffers of STR_ER_WANT_RUN_SPLIT / str_er_feet_split / str_er_split_words: the bytes of the cut records and of the
 * segmentation tables on the device (0: never made).  Either pointer may be NULL.                                                   */
int str_er_run_split_stats(const str_er_ctx *ctx, uint64_t *cut_bytes, uint64_t *table_bytes);
/* The kept cuts of one run from its column counts n[0 .. W) and its height H (str_er_run_split): cut receives the columns relative
 * to the run, ascending, -1 unused; *n_cuts their number; *thr (optional) the threshold.  Pure: no context, no GPU.  STR_ER_EINVAL on
 * NULL arguments, W < 1, H < 1 or num / den outside 1 .. 65535.                                                                     */
int str_er_cuts_from_counts(const uint32_t *n, int32_t W, int32_t H, int32_t num, int32_t den, int32_t cut[3], int32_t *n_cuts, uint32_t *thr);
/* str_er_feet_read and the cuts and pieces of every run (str_er_run_split), made on the GPU from the run slots and the footprint
 * words: splits receives one record per run (cap_runs of them; n_parts is left 0), pieces the piece table and *n_pieces its size
 * (pieces == NULL only counts; cap_pieces too small -> STR_ER_ECAPACITY, *n_pieces still set).  piece_reads (optional) receives the
 * reading of every piece and piece_q (optional) its 1800 feature bytes, both for cap_pieces pieces; piece_reads needs an SVM model of
 * dim 1800 (STR_ER_ESTATE without), cuts, pieces and piece_q need none.  splits == NULL or n_pieces == NULL -> STR_ER_EINVAL.  The
 * other arguments, their validation and capacity codes are those of str_er_feet_read; a counting call (runs == NULL or words ==
 * NULL) makes no cuts.  The runs' own results are those of str_er_feet_read, byte for byte.                                        */
int str_er_feet_split(str_er_ctx *ctx, int32_t W, int32_t H, const str_er_line_foot *feet, const uint32_t *bits, const double *slopes, int32_t n,
                      str_er_line_words *line_words, str_er_line_run *runs, int32_t cap_runs, int32_t *n_runs, str_er_line_word *words,
                      int32_t cap_words, int32_t *n_words, str_er_run_read *reads, uint8_t *q_out, str_er_run_split *splits,
                      str_er_run_piece *pieces, int32_t cap_pieces, int32_t *n_pieces, str_er_run_read *piece_reads, uint8_t *piece_q);
/* The segmentation (str_er_run_split) of the runs of n_words words on the caller's cost rows, on the GPU: splits holds n_runs records
 * (n_cuts, first_piece and n_pieces are read), run_costs n_runs rows of 65 bytes, piece_costs n_pieces rows; word w has the runs
 * first_run[w] .. first_run[w] + n_runs_of_word[w].  word_splits receives n_words records, parts the split sequences of the words back
 * to back in word order and *n_parts their number; part_costs (optional) the 65-byte rows of the parts in the same order, which
 * str_er_match_words and str_er_decode_words take with (first_part, n_parts) as the windows.  cap_parts too small -> STR_ER_ECAPACITY,
 * *n_parts still set (it is at most the sum over the words' runs of n_cuts + 1).  STR_ER_EINVAL on a word outside the runs, a record
 * whose n_cuts is outside 0 .. 3, whose n_pieces does not follow from n_cuts or whose pieces lie outside the rows.  It needs no model. */
int str_er_split_words(str_er_ctx *ctx, const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs,
                       int32_t n_pieces, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, str_er_word_split *word_splits,
                       str_er_split_part *parts, int32_t cap_parts, int32_t *n_parts, uint8_t *part_costs);
/* The same rules on one host thread, with SPLIT as an argument (0 .. 255).  Pure: no context, no GPU.                               */
int str_er_split_words_host(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                            const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, int32_t split_cost,
                            str_er_word_split *word_splits, str_er_split_part *parts, int32_t cap_parts, int32_t *n_parts, uint8_t *part_costs);

/* The joint decode (str_er_lattice_decode) of n_words words on the caller's rows, on the GPU, with the context's table, INS / DEL
 * (str_er_set_word_decode) and SPLIT (str_er_set_run_split): the arguments up to n_words are those of str_er_split_words (the rows
 * unfolded).  dec receives n_words records, chars and src 64 bytes per word each, parts the lattice parts of the words back to back in
 * word order and *n_parts their number.  cap_parts too small -> STR_ER_ECAPACITY, *n_parts still set (it is at most the sum over
 * the words' runs of n_cuts + 1).  STR_ER_ESTATE without a table; the validation is that of str_er_split_words.  It needs no model.   */
int str_er_lattice_decode_words(str_er_ctx *ctx, const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs,
                                int32_t n_pieces, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, str_er_lattice_decode *dec,
                                uint8_t *chars, uint8_t *src, str_er_split_part *parts, int32_t cap_parts, int32_t *n_parts);
/* The same rules on one host thread, with SPLIT, the table and INS / DEL as arguments (with the checks of str_er_set_run_split and
 * str_er_set_word_decode).  Pure: no context, no GPU.                                                                              */
int str_er_lattice_decode_words_host(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                                     const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, int32_t split_cost, const uint8_t *bigram,
                                     int32_t ins, int32_t del, str_er_lattice_decode *dec, uint8_t *chars, uint8_t *src, str_er_split_part *parts,
                                     int32_t cap_parts, int32_t *n_parts);
/* Whether a detect call with STR_ER_WANT_LATTICE_DECODE also makes the margins of its words (str_er_lattice_margin): on != 0 switches
 * them on; off by default.  A context setting, not a stage flag: without STR_ER_WANT_LATTICE_DECODE it does nothing, and while it is
 * off no call enqueues, uploads or allocates anything more than before.  A stream's contexts: str_er_stream_context.               */
int str_er_set_lattice_margin(str_er_ctx *ctx, int32_t on);
/* The margins (str_er_lattice_margin) on the caller's rows, on the GPU, under the context's table, INS / DEL and SPLIT: the arguments
 * up to n_words and their checks are those of str_er_lattice_decode_words, and the decoder runs on these rows first.  margins receives
 * n_words records, read_margin and cut_margin 32 int32 per word each, read, alt and cut_alt 32 bytes per word each, edge_min (NULL: not
 * wanted) 32 x 4 int32 per word, marginals (NULL: not wanted) 32 x 4 x 66 int32 per word.  Words may share runs.  STR_ER_ESTATE without
 * a table; STR_ER_EINVAL on a word outside the runs or a record with cuts or pieces that are none.  n_words = 0 is fine.           */
int str_er_lattice_margins(str_er_ctx *ctx, const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs,
                           int32_t n_pieces, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, str_er_lattice_margin *margins,
                           int32_t *read_margin, int32_t *cut_margin, uint8_t *read, uint8_t *alt, uint8_t *cut_alt, int32_t *edge_min, int32_t *marginals);
/* The same rules on one host thread, with SPLIT, the table and INS / DEL as arguments (with the checks of
 * str_er_lattice_decode_words_host).  Pure: no context, no GPU.                                                                     */
int str_er_lattice_margins_host(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                                const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, int32_t split_cost, const uint8_t *bigram,
                                int32_t ins, int32_t del, str_er_lattice_margin *margins, int32_t *read_margin, int32_t *cut_margin, uint8_t *read,
                                uint8_t *alt, uint8_t *cut_alt, int32_t *edge_min, int32_t *marginals);
/* Statistics of the buffer of STR_ER_WANT_LATTICE_DECODE / str_er_lattice_decode_words: the bytes of its tables on the device (0: never
 * made).  The pointer may be NULL.                                                                                                  */
int str_er_lattice_decode_stats(const str_er_ctx *ctx, uint64_t *table_bytes);
/* Whether a detect call with STR_ER_WANT_LATTICE_DECODE also decodes every line of str_er_result_texts() over the piece lattices of
 * its runs (str_er_line_lattice_decode), and the weight (0 .. 127) of its gap costs: on != 0 switches it on; off by default, the
 * weight 16.  A weight outside 0 .. 127 -> STR_ER_EINVAL, the context unchanged.  A context setting, not a stage flag: without
 * STR_ER_WANT_LATTICE_DECODE (and STR_ER_WANT_RUN_SPLIT, which it needs) it does nothing, and while it is off no call enqueues,
 * uploads or allocates anything more than before.  A stream's contexts: str_er_stream_context.                                       */
int str_er_set_line_lattice_decode(str_er_ctx *ctx, int32_t on, int32_t weight);
/* The joint decode of lines over their runs' piece lattices (str_er_line_lattice_decode) on the caller's rows, on the GPU, with the
 * context's table, INS / DEL (str_er_set_word_decode) and SPLIT (str_er_set_run_split): splits, the rows and n_pieces are those of
 * str_er_lattice_decode_words; gaps holds 2 * n_runs bytes, (J, K) per run; line t has the runs first_run[t] .. first_run[t] +
 * n_runs_of_line[t], the windows in ascending order and none over another (every line writes its own slices).  With S the sum of
 * n_cuts + 1 over all n_runs runs: dec receives n_lines records, chars 3 * S bytes and src 3 * S uint16 (0xFF / 0xFFFF in no line's
 * slice), parts and word_of_part the parts of the lines back to back in line order and *n_parts their number.  cap_parts too small
 * -> STR_ER_ECAPACITY, *n_parts still set (it is at most the sum over the lines' runs of n_cuts + 1) and nothing else written.
 * STR_ER_ESTATE without a table; STR_ER_EINVAL on NULL arguments, a record with cuts or pieces that are none, a window outside the
 * runs or out of order, or a gap of a line with both moves off; the context stays usable.  n_lines = 0 is fine.  It needs no model. */
int str_er_lattice_decode_lines(str_er_ctx *ctx, const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs,
                                int32_t n_pieces, const uint8_t *gaps, const int32_t *first_run, const int32_t *n_runs_of_line, int32_t n_lines,
                                str_er_line_lattice_decode *dec, uint8_t *chars, uint16_t *src, str_er_split_part *parts, int32_t cap_parts,
                                int32_t *n_parts, int32_t *word_of_part);
/* The same rules on one host thread, with SPLIT, the table and INS / DEL as arguments (with the checks of str_er_set_run_split and
 * str_er_set_word_decode).  Pure: no context, no GPU.                                                                              */
int str_er_lattice_decode_lines_host(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                                     const uint8_t *gaps, const int32_t *first_run, const int32_t *n_runs_of_line, int32_t n_lines, int32_t split_cost,
                                     const uint8_t *bigram, int32_t ins, int32_t del, str_er_line_lattice_decode *dec, uint8_t *chars, uint16_t *src,
                                     str_er_split_part *parts, int32_t cap_parts, int32_t *n_parts, int32_t *word_of_part);
/* The bytes of the line lattice decoder's back-pointer table on the device (68 uint32 per node of the largest call so far; 0 before
 * the first).  The pointer may be NULL.                                                                                            */
int str_er_line_lattice_decode_stats(const str_er_ctx *ctx, uint64_t *table_bytes);

/* The lexicon match over the piece lattice (str_er_lattice_match) of n_words words on the caller's rows, on the GPU, with the context's
 * lexicon (str_er_set_lexicon), INS / DEL / band (str_er_set_word_match) and SPLIT (str_er_set_run_split): the arguments up to n_words,
 * the validation and the capacity rule are those of str_er_lattice_decode_words.  The rows are taken as given; the fold of the lexicon
 * is applied when they are read.  matches receives n_words records, src 32 bytes per word, parts the parts of the winning entries back
 * to back in word order and *n_parts their number.  cap_parts too small -> STR_ER_ECAPACITY, *n_parts still set (it is at most the sum
 * over the words' runs of n_cuts + 1).  STR_ER_ESTATE without a lexicon.  It needs no model.                                        */
int str_er_lattice_match_words(str_er_ctx *ctx, const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs,
                               int32_t n_pieces, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, str_er_lattice_match *matches,
                               uint8_t *src, str_er_split_part *parts, int32_t cap_parts, int32_t *n_parts);
/* The same rules on one host thread, with the lexicon (as str_er_set_lexicon takes it), INS / DEL / band and SPLIT as arguments (with
 * the checks of str_er_set_lexicon, str_er_set_word_match and str_er_set_run_split).  Pure: no context, no GPU.                       */
int str_er_lattice_match_words_host(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                                    const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, const char *bytes, const int32_t *offsets,
                                    int32_t n, uint32_t flags, int32_t ins, int32_t del, int32_t band, int32_t split_cost, str_er_lattice_match *matches,
                                    uint8_t *src, str_er_split_part *parts, int32_t cap_parts, int32_t *n_parts);
/* Statistics of the buffer of STR_ER_WANT_LATTICE_MATCH / str_er_lattice_match_words: the bytes of its tables on the device (0: never
 * made).  The pointer may be NULL.                                                                                                  */
int str_er_lattice_match_stats(const str_er_ctx *ctx, uint64_t *table_bytes);

/* The track match over the members' piece lattices (str_er_lattice_track_member) on the caller's rows, on the GPU, with the context's
 * lexicon, INS / DEL / band and SPLIT: the arguments up to n_words are those of str_er_lattice_match_words, the tracks those of
 * str_er_match_tracks, each with its validation.  out receives n_tracks records, members_out n_members records, src 32 bytes per slot
 * of the member array, parts the members' parts back to back in slot order and *n_parts their number.  cap_parts too small ->
 * STR_ER_ECAPACITY, *n_parts still set (it is at most the sum over the slots of the member's N).  STR_ER_ESTATE without a lexicon;
 * STR_ER_ECAPACITY on a track of more than 65536 members.  It needs no model.                                                        */
int str_er_lattice_match_tracks(str_er_ctx *ctx, const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs,
                                int32_t n_pieces, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, const int32_t *track_first,
                                const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks, str_er_track_match *out,
                                str_er_lattice_track_member *members_out, uint8_t *src, str_er_split_part *parts, int32_t cap_parts, int32_t *n_parts);
/* The same rules on one host thread, with the lexicon, INS / DEL / band and SPLIT as arguments (as for
 * str_er_lattice_match_words_host).  Pure: no context, no GPU.                                                                       */
int str_er_lattice_match_tracks_host(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                                     const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, const int32_t *track_first,
                                     const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks, const char *bytes,
                                     const int32_t *offsets, int32_t n, uint32_t flags, int32_t ins, int32_t del, int32_t band, int32_t split_cost,
                                     str_er_track_match *out, str_er_lattice_track_member *members_out, uint8_t *src, str_er_split_part *parts,
                                     int32_t cap_parts, int32_t *n_parts);
/* Statistics of the buffer of STR_ER_WANT_LATTICE_TRACK / str_er_lattice_match_tracks: the bytes of its tables on the device (0: never
 * made).  The pointer may be NULL.                                                                                                  */
int str_er_lattice_track_stats(const str_er_ctx *ctx, uint64_t *table_bytes);

/* Whether a detect call that carries both STR_ER_WANT_TRACK_DECODE and STR_ER_WANT_LATTICE_DECODE also decodes every word track over
 * its members' piece lattices (str_er_lattice_track_decode; the tables: str_er_result_lattice_track_decodes and its neighbours).  Off
 * by default; on is 0 or 1, anything else -> STR_ER_EINVAL.  It is a setting of the context and no stage flag: with either flag missing
 * it does nothing, and while it is off every output of every call is byte for byte what it is without it.                          */
int str_er_set_lattice_track_decode(str_er_ctx *ctx, int32_t on);
/* The track decode over the members' piece lattices (str_er_lattice_track_decode) on the caller's rows, on the GPU, under the context's
 * table, its str_er_set_word_decode INS / DEL for the seeds, its str_er_set_track_decode parameters and its SPLIT: the inputs are those
 * of str_er_lattice_match_tracks, each with its validation; k_lattice_decode runs on the words first (the seeds), as
 * str_er_decode_tracks runs the word decoder.  out receives n_tracks records, chars 32 label bytes per track, members_out n_members
 * records, src 32 bytes per slot of the member array, parts the members' parts back to back in slot order and *n_parts their number.
 * cap_parts too small -> STR_ER_ECAPACITY, *n_parts still set (it is at most the sum over the slots of the member's N).  STR_ER_ESTATE
 * without a table; STR_ER_ECAPACITY on a track of more than 1024 members.  It needs no lexicon and no SVM model.                     */
int str_er_lattice_decode_tracks(str_er_ctx *ctx, const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs,
                                 int32_t n_pieces, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, const int32_t *track_first,
                                 const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks, str_er_track_decode *out,
                                 uint8_t *chars, str_er_lattice_track_member *members_out, uint8_t *src, str_er_split_part *parts, int32_t cap_parts,
                                 int32_t *n_parts);
/* The same rules on one host thread, with the table (66 x 66), the seeds' INS / DEL (dec_ins, dec_del: 0 .. 255), this output's INS /
 * DEL (1 .. 255) and rounds (0 .. 64) and SPLIT (0 .. 255) as arguments.  Pure: no context, no GPU.                                  */
int str_er_lattice_decode_tracks_host(const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs, const uint8_t *piece_costs, int32_t n_pieces,
                                      const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words, const int32_t *track_first,
                                      const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks, const uint8_t *bigram,
                                      int32_t dec_ins, int32_t dec_del, int32_t ins, int32_t del, int32_t rounds, int32_t split_cost,
                                      str_er_track_decode *out, uint8_t *chars, str_er_lattice_track_member *members_out, uint8_t *src,
                                      str_er_split_part *parts, int32_t cap_parts, int32_t *n_parts);
/* Statistics of the buffer of str_er_lattice_decode_tracks and of the setting in a detect call: the bytes of its tables on the device
 * (0: never made).  The pointer may be NULL.                                                                                          */
int str_er_lattice_track_decode_stats(const str_er_ctx *ctx, uint64_t *table_bytes);

/* The track pool (str_er_pool_match).  Every entry point returns the library's codes and leaves the pool unchanged on any error; the
 * error text is the context's (str_er_last_error).  The calls run on the context's stream and wait for it.
 * _create: a pool of cap_tracks >= 1 empty slots in *pool; flags: 0 (the members' rows, as str_er_match_tracks) or
 * STR_ER_POOL_LATTICE (the members' piece lattices, as str_er_lattice_match_tracks).  STR_ER_ESTATE without a lexicon;
 * STR_ER_ECAPACITY where cap_tracks * groups * 256 bytes (groups: the 64-entry groups of the padded device lexicon) pass 2^40,
 * STR_ER_ENOMEM where the device does not have them.                                                                              */
int str_er_track_pool_create(str_er_ctx *ctx, int32_t cap_tracks, uint32_t flags, str_er_track_pool **pool);
void str_er_track_pool_destroy(str_er_track_pool *pool);
/* Every slot empty, and the pool bound to the context's lexicon and parameters as they are now (the accumulators are allocated again
 * if the lexicon's size changed).  STR_ER_ESTATE without a lexicon: the pool then stays stale.                                      */
int str_er_track_pool_reset(str_er_track_pool *pool);
/* The slots, the flags, the entries of the lexicon the pool is bound to, its bytes on the device, the slots with a member, and
 * whether it is stale (1 / 0).  Any pointer may be NULL.  This one call works on a stale pool.                                      */
int str_er_track_pool_info(const str_er_track_pool *pool, int32_t *cap_tracks, uint32_t *flags, int32_t *n_entries, uint64_t *device_bytes,
                           int32_t *n_in_use, int32_t *stale);
/* Track g of the call, given as for str_er_match_tracks with that call's checks, is added to the slot slots[g].  STR_ER_EINVAL on a
 * slot outside 0 .. cap_tracks - 1 or named twice in one call (distinct slots: the kernel owns its rows without atomics);
 * STR_ER_ECAPACITY where a slot would pass 65536 members; STR_ER_ESTATE on a lattice pool.                                          */
int str_er_track_pool_add(str_er_track_pool *pool, const uint8_t *costs, int32_t n_rows, const int32_t *first_run, const int32_t *n_runs_of_word,
                          int32_t n_words, const int32_t *track_first, const int32_t *track_count, const int32_t *members, int32_t n_members,
                          int32_t n_tracks, const int32_t *slots);
/* The same for a lattice pool, with the arguments and checks of str_er_lattice_match_tracks.  STR_ER_ESTATE on a rows pool.         */
int str_er_track_pool_add_lattice(str_er_track_pool *pool, const str_er_run_split *splits, int32_t n_runs, const uint8_t *run_costs,
                                  const uint8_t *piece_costs, int32_t n_pieces, const int32_t *first_run, const int32_t *n_runs_of_word, int32_t n_words,
                                  const int32_t *track_first, const int32_t *track_count, const int32_t *members, int32_t n_members, int32_t n_tracks,
                                  const int32_t *slots);
/* Slot dst becomes the pooled track of its own and all srcs' members (sums added, masks or-ed, counts and free costs summed); the
 * srcs become empty.  STR_ER_EINVAL on a slot out of range, a repeated slot or dst among the srcs; STR_ER_ECAPACITY where the
 * members pass 65536.  n_srcs = 0 is fine.                                                                                          */
int str_er_track_pool_join(str_er_track_pool *pool, int32_t dst, const int32_t *srcs, int32_t n_srcs);
/* Those slots become empty (a slot may be named more than once).                                                                    */
int str_er_track_pool_clear(str_er_track_pool *pool, const int32_t *slots, int32_t n);
/* out receives n records, out[i] of the slot slots[i]; a slot may be named more than once.                                          */
int str_er_track_pool_read(str_er_track_pool *pool, const int32_t *slots, int32_t n, str_er_pool_match *out);

/* The decode pool (str_er_pool_decode).  _destroy, _reset, _info, _add, _join and _clear above work on it as on a lexicon pool: _add
 * takes the unfolded 65-byte rows of str_er_word_decode with the arguments and checks it has, a join leaves in dst the keep newest
 * of the union and the srcs empty.  _add_lattice and _read on a decode pool and _read_decode and _members on a lexicon pool answer
 * STR_ER_ESTATE; the pool that takes _add_lattice without a lexicon is the lattice decode pool (below).
 * _create_decode: cap_tracks >= 1 empty slots of 1 <= keep <= 1024 kept members each (else STR_ER_EINVAL); STR_ER_ESTATE without a
 * bigram table; STR_ER_ECAPACITY where cap_tracks * keep passes 2^24 (a kept member takes about 2.2 KB on the device),
 * STR_ER_ENOMEM where the device does not have the memory.                                                                          */
int str_er_track_pool_create_decode(str_er_ctx *ctx, int32_t cap_tracks, int32_t keep, str_er_track_pool **pool);
/* The per-slot limit of a decode pool (0 for a lexicon pool).  Works on a stale pool.                                                */
int str_er_track_pool_keep(const str_er_track_pool *pool, int32_t *keep);
/* out receives n records, out[i] of the slot slots[i], chars 32 label bytes a slot and member_cost keep values a slot: the kept
 * members' costs in age order, -1 past n_kept.  A slot may be named more than once.                                                 */
int str_er_track_pool_read_decode(str_er_track_pool *pool, const int32_t *slots, int32_t n, str_er_pool_decode *out, uint8_t *chars, int32_t *member_cost);
/* The kept list of one slot in age order: *n_kept members with their keys, run counts and rows (keep * 32 * 65 bytes, 32 rows a
 * member, of which the first n_runs are the member's).  Any of keys, n_runs and rows may be NULL.  For callers who want the evidence
 * back, e.g. to read it again over lattices.                                                                                        */
int str_er_track_pool_members(str_er_track_pool *pool, int32_t slot, uint64_t *keys, int32_t *n_runs, uint8_t *rows, int32_t *n_kept);

/* The lattice decode pool (see "The lattice decode pool" at str_er_pool_decode).  _destroy, _reset, _info, _keep, _join and _clear
 * work on it as on a decode pool; _add_lattice adds to it; _read_decode gives the decode pool's record, labels and member costs, the
 * same shapes.  _add, _read and _members on it answer STR_ER_ESTATE, as _read_lattice_decode and _lattice_members do on every other
 * kind of pool.
 * _create_lattice_decode: cap_tracks >= 1 empty slots of 1 <= keep <= 1024 kept members each (else STR_ER_EINVAL); STR_ER_ESTATE
 * without a bigram table; STR_ER_ECAPACITY where cap_tracks * keep passes 13 421 772 (2^30 / 80: the piece rows of the store stay
 * below the bit that marks a piece's row) or the store (9072 bytes a kept member and 4 a slot: about 122 GB at that bound) passes 2^40
 * bytes, STR_ER_ENOMEM where the device does not have the memory.                                                       */
int str_er_track_pool_create_lattice_decode(str_er_ctx *ctx, int32_t cap_tracks, int32_t keep, str_er_track_pool **pool);
/* out, chars and member_cost as str_er_track_pool_read_decode.  members_out receives keep records a slot, the kept members' in age
 * order with word = the age rank, behind them records with cost = -1 and word = -1; src 32 bytes per such record; parts the kept
 * members' parts of all slots read back to back in that order, first_part indexing that table, *n_parts their number.  A part's run
 * is 32 * rank + the member's run and its piece 80 * rank + the member's piece row (-1: the whole run): the indices of
 * str_er_track_pool_lattice_members' arrays for that slot.  members_out, src and parts may be NULL, each on its own; with parts
 * cap_parts too small -> STR_ER_ECAPACITY, *n_parts still set (it is at most 32 * the kept members).  A slot may be named more than
 * once.                                                                                                                              */
int str_er_track_pool_read_lattice_decode(str_er_track_pool *pool, const int32_t *slots, int32_t n, str_er_pool_decode *out, uint8_t *chars, int32_t *member_cost,
                                          str_er_lattice_track_member *members_out, uint8_t *src, str_er_split_part *parts, int32_t cap_parts, int32_t *n_parts);
/* The kept list of one slot in age order, with fixed strides per member: *n_kept members with their keys [keep], run counts [keep],
 * split records [keep x 32], run rows [keep x 32 x 65 bytes] and piece rows [keep x 80 x 65 bytes].  Of a member's 32 records and run
 * rows the first n_runs are its own, of its 80 piece rows the first sum of its runs' n_pieces (at most 72); what lies behind them is
 * zero.  The first_piece of a returned split record indexes that member's own piece rows.  Any of keys, n_runs, splits, run_rows and
 * piece_rows may be NULL.                                                                                                            */
int str_er_track_pool_lattice_members(str_er_track_pool *pool, int32_t slot, uint64_t *keys, int32_t *n_runs, str_er_run_split *splits, uint8_t *run_rows,
                                      uint8_t *piece_rows, int32_t *n_kept);

/* The crops of STR_ER_WANT_LINE_CROPS: height (8..256), max_width (1..8192) and pad (0..1, a fraction of the line's height on every
 * side).  Defaults 32, 1024, 0.125.  Anything else -> STR_ER_EINVAL, the context unchanged.  A stream's contexts:
 * str_er_stream_context.                                                                                                          */
int str_er_set_line_crop(str_er_ctx *ctx, int32_t height, int32_t max_width, double pad);
/* The geometry of one line (str_er_line_crop; pix_off = 0) from its n_boxes boxes (x, y, w, h; w, h >= 1) and slope.  Pure host, no
 * context.  STR_ER_EINVAL on bad arguments (out of the ranges of str_er_set_line_crop) or a geometry outside 16.16 fixed point. */
int str_er_line_crop_geometry(const int32_t *boxes_xywh, int32_t n_boxes, double slope, int32_t height, int32_t max_width, double pad,
                              str_er_line_crop *out);
/* Grey crops of n_lines lines of one host plane at the context's crop settings: line k has the boxes
 * boxes_xywh[first[k] .. first[k] + count[k]) (count >= 1) and slope slopes[k].  recs receives the n_lines records, pixels the crops
 * (laid out as in a result).  pixels == NULL only fills recs and *n_bytes; cap too small -> STR_ER_ECAPACITY, *n_bytes still set. */
int str_er_line_crops(str_er_ctx *ctx, const uint8_t *plane, int32_t w, int32_t h, int64_t stride, const int32_t *boxes_xywh,
                      const int32_t *first, const int32_t *count, const double *slopes, int32_t n_lines, uint8_t *pixels, uint64_t cap,
                      uint64_t *n_bytes, str_er_line_crop *recs);

/* ERFilter::make_LBP_hist(input, 2, 24) (src/ER.cpp:789-816) for n boxes of one host
 * plane: hist receives n*1024 doubles; tiles26 (optional, may be NULL) receives the
 * n ARAN(26) tiles (src/OCR.cpp:394-430), 676 bytes each.                            */
int str_er_lbp_hist(str_er_ctx *ctx, const uint8_t *plane, int32_t w, int32_t h,
                    int64_t stride, const int32_t *boxes_xywh, int32_t n,
                    double *hist, uint8_t *tiles26);

/* ERFilter::calc_LBP(input, 24) (inc/ER.h:134, src/ER.cpp:819-845; caller OCR::lbp_run,
 * src/OCR.cpp:37-39) for n boxes of one host plane: lbp24 receives the n 24x24 Mean-LBP
 * code maps, 576 bytes each, row-major -- the Mat the reference returns, stride-24-on-26
 * addressing included.                                                                */
int str_er_calc_lbp(str_er_ctx *ctx, const uint8_t *plane, int32_t w, int32_t h,
                    int64_t stride, const int32_t *boxes_xywh, int32_t n, uint8_t *lbp24);

/* AdaBoost::predict(vector<double> fv) (inc/adaboost.h:131; CascadeBoost::predict,
 * src/adaboost.cpp:507-542) for n caller-supplied 1024-element feature vectors:
 * out[i] = last stage score, or -DBL_MAX if a stage rejected.                       */
int str_er_cascade_predict(str_er_ctx *ctx, int which, const double *fv, int32_t n, double *out);

/* ---- OCR scorer, SVM half (config 3) --------------------------------------
 * svm_load_model (src/svm.cpp:2767-2982; OCR::OCR, src/OCR.cpp:19-22): a libsvm C-SVC / RBF text model
 * with probability information (probA/probB).  dim = feature dimension (1800 = 8 x 15 x 15 for the
 * reference's chain-code features, src/OCR.cpp:203-216); must exceed the largest SV index.  2 <= nr_class <= 125
 * (the reference's model has 65): STR_ER_EFORMAT otherwise.                                                     */
int str_er_load_svm_model(str_er_ctx *ctx, const char *path, int32_t dim);
int str_er_load_svm_model_mem(str_er_ctx *ctx, const char *text, size_t len, int32_t dim);
int str_er_svm_info(const str_er_ctx *ctx, int32_t *nr_class, int32_t *total_sv, int32_t *dim);
/* How the loaded model's kernel matrix is computed for vectors that come from boxes (chain_run, STR_ER_STAGE_OCR / _OCR_LINES; measurement aid, any pointer
 * may be NULL): *bytes = 1 if the support vectors are 8-bit numerators over 255 -- as the reference's are, being feature vectors of its training set
 * (src/OCR.cpp:211) -- and |x - sv|^2 is an exact integer from 8-bit matrix instructions, 0 if each f32 value goes as three bf16 pieces; *class_sums = 1 if
 * the decision values are summed per class as dense f64 products (models with more than 8 support vectors a class), 0 if per vector. */
int str_er_svm_forms(const str_er_ctx *ctx, int32_t *bytes, int32_t *class_sums);
/* svm_predict_probability (inc/svm.h:88, src/svm.cpp:2592-2629) for n dense feature vectors x[n][dim]
 * (zeros = absent svm_nodes): label[i] = model->label[argmax], prob[i][nr_class]; dec (optional, may
 * be NULL) receives the nr_class*(nr_class-1)/2 decision values of svm_predict_values.              */
int str_er_svm_predict_probability(str_er_ctx *ctx, const double *x, int32_t n, int32_t dim, int32_t *label, double *prob,
                                   double *dec);
/* The same for n vectors given as 8-bit numerators over 255, q[n][dim] (feature j = q[i][j] / 255.0: the vectors OCR::chain_run makes from its
 * boxes, src/OCR.cpp:211), scored by the kernels that score the boxes of chain_run and of STR_ER_STAGE_OCR / _OCR_LINES (str_er_svm_forms says which):
 * for dim = 1800, a box's label and pv[label] are those of its q_out row here, bit for bit.  label[i], prob[i][nr_class], dec (optional) as above. */
int str_er_svm_predict_probability_q8(str_er_ctx *ctx, const uint8_t *q, int32_t n, int32_t dim, int32_t *label, double *prob, double *dec);

/* OCR::chain_run(Mat src, int thresh, double slope) (src/OCR.cpp:67-140) for n boxes (ER::bound) of one host
 * plane (the channel the ER came from), with slope == 0: Otsu-binarise 255-roi, ARAN(30), chain-code
 * features (src/OCR.cpp:144-218), then
 * svm_predict_probability.  label[i] = class label, prob[i] = pv[label] (chain_run returns
 * table[label] + prob); q_out (optional) receives the 1800 feature bytes of every box (value = q/255);
 * label/prob may be NULL to get the features only (no SVM model needed then).                        */
int str_er_ocr_chain_run(str_er_ctx *ctx, const uint8_t *plane, int32_t w, int32_t h, int64_t stride, const int32_t *boxes_xywh,
                         int32_t n, int32_t *label, double *prob, uint8_t *q_out);

/* calc_color(ER*, Mat mask_channel, Mat color_img) (src/ER.cpp:1391-1419) for n boxes (ER::bound) of one host
 * mask plane and one host 3-byte interleaved colour image (the Ycrcb Mat): colors[i][0..2] = ER::color1..3.
 * The colour image is read from its own row 0 / column 0 for every box, as the reference does (:1404).
 * It must be at least as large as the largest box.                                                    */
int str_er_calc_color(str_er_ctx *ctx, const uint8_t *mask_plane, int32_t w, int32_t h, int64_t stride, const uint8_t *color_img,
                      int32_t cw, int32_t ch, int64_t cstride, const int32_t *boxes_xywh, int32_t n, double *colors);

/* ERFilter::er_track (src/ER.cpp:530-590) on caller-supplied ERs of ONE image: cands[i].{x,y,w,h,area,cls}
 * (cls 1 = from strong[], 2 = from weak[], others ignored) and colors[i][3] (from str_er_calc_color);
 * tracked[i] = 1 for the members of all_er, cx/cy (optional) receive ER::center.                     */
int str_er_er_track(str_er_ctx *ctx, const str_er_cand *cands, const double *colors, int32_t n, uint8_t *tracked, int32_t *cx,
                    int32_t *cy);

/* ERFilter::er_grouping(all_er, text, false, inner_sup) (src/ER.cpp:612-692) on caller-supplied ERs of ONE image:
 * cands[i].{x,y,w,h,area} and tracks[i].{color1-3, cx, cy, tracked} (all_er = the ones with tracked != 0).  The
 * result holds copies of cands and tracks plus the lines (str_er_result_texts / _text_ers / _group_bounds);
 * free it with str_er_result_free.  overlap_sup = true (video_mode without DO_OCR asks for it,
 * src/utils.cpp:196): sort + overlap_suppression (src/ER.cpp:614-617, sequential -- a merge rewrites the survivor's box) run
 * on the host, the survivors then take the same GPU stages; the merged boxes are in str_er_result_gbounds, the surviving
 * list (all_er as the reference leaves it) in str_er_result_group_all.                                    */
int str_er_er_grouping(str_er_ctx *ctx, const str_er_cand *cands, const str_er_track *tracks, int32_t n, int overlap_sup,
                       int inner_sup, str_er_result **out);

/* The same with the text line's slope per box (Text::slope, src/ER.cpp:731): where |slope[i]| > 0.01 the
 * binarised ROI goes through OCR::rotate_mat(atan2(slope, 1), crop = true) (src/OCR.cpp:73-78, 254-357)
 * before ARAN.  slope == NULL means all zero.  A non-finite slope is STR_ER_EINVAL.                   */
int str_er_ocr_chain_run_slope(str_er_ctx *ctx, const uint8_t *plane, int32_t w, int32_t h, int64_t stride,
                               const int32_t *boxes_xywh, const double *slope, int32_t n, int32_t *label, double *prob,
                               uint8_t *q_out);

/* ERFilter::non_maximum_supression (src/ER.cpp:416-505) on a caller-supplied kept tree
 * (parent indices; root points to itself or -1).  pool_idx receives up to cap node
 * indices in ascending key order; *n_pool the count; *ambiguous as in plane_info.
 * Sibling ties with sibling_order = 0: the TABLE ORDER is the child-list order -- of
 * the children of one parent the one listed first is the first of ER::child / ER::next
 * (src/ER.cpp:183-185), i.e. the one the reference's post-order walk visits first.     */
int str_er_nms_tree(str_er_ctx *ctx, const str_er_node *nodes, int32_t n_nodes,
                    int32_t rows, int32_t cols, int32_t *pool_idx, int32_t cap,
                    int32_t *n_pool, int32_t *ambiguous);

/* The same for a table that came from str_er_detect_planes / er_tree_extract (ordered
 * by key, which says nothing about the flood): the plane itself is passed -- as the
 * reference's signature does (`Mat input`, src/ER.cpp:416) -- and sibling ties are
 * decided by replaying the reference's flood on it (sibling_order = 0).  node.key
 * must be the canonical key (min pixel index of the node's own level).                */
int str_er_nms_tree_plane(str_er_ctx *ctx, const str_er_node *nodes, int32_t n_nodes,
                          const uint8_t *plane, int32_t cols, int32_t rows, int64_t stride,
                          int32_t *pool_idx, int32_t cap, int32_t *n_pool, int32_t *ambiguous);

/* The order in which the reference's flood (er_tree_extract, src/ER.cpp:240-374) first reaches the pixels
 * of a host plane: stamp[y*w+x] = 1-based position, 0 = never reached (sealed off by sentinel-level
 * pixels).  This is the walk that decides NMS sibling ties (sibling_order = 0); it runs on the calling
 * thread, needs no context and no GPU, and is exported so that the tie-break can be checked on its own. */
int str_er_flood_order(const uint8_t *plane, int32_t w, int32_t h, int64_t stride, int32_t thresh_step, uint32_t *stamp);

/* Build-defined pyramid primitive (no reference counterpart): fixed-point bilinear
 * resize of one host plane, same arithmetic as cv::resize INTER_LINEAR 8UC1.         */
int str_er_resize_plane(str_er_ctx *ctx, const uint8_t *src, int32_t sw, int32_t sh,
                        int64_t sstride, uint8_t *dst, int32_t dw, int32_t dh);

/* One pyramid level of one host plane through the dispatch the uniform-batch ingest uses for every level:
 * k_pyr_level where the shape qualifies (a linear reduction with 1 < scale <= 1.5 in both directions, strides
 * that are multiples of 4), k_resize otherwise.  The planes keep the given strides on the device.  rows: the
 * output rows a wave walks, 8 / 16 / 32, or 0 for the library's choice.  *kernel_used: 1 k_pyr_level ran,
 * 0 k_resize did.  Same bytes as str_er_resize_plane either way.                                              */
int str_er_pyr_level_plane(str_er_ctx *ctx, const uint8_t *src, int32_t sw, int32_t sh, int64_t sstride,
                           uint8_t *dst, int32_t dw, int32_t dh, int64_t dstride, int32_t rows,
                           int32_t *kernel_used);

/* ---- results (owned by the library until str_er_result_free) ----------------------- */
int32_t str_er_result_n_planes(const str_er_result *r);
int     str_er_result_plane_info(const str_er_result *r, int32_t plane, str_er_plane_info *info);
/* All plane records of the call as one array (n = str_er_result_n_planes). */
const str_er_plane_info *str_er_result_plane_infos(const str_er_result *r, int32_t *n);
/* All candidates of the call, ordered by (plane, key). */
const str_er_cand *str_er_result_cands(const str_er_result *r, int32_t *n);
/* Candidates of one plane (a slice of the array above). */
const str_er_cand *str_er_result_plane_cands(const str_er_result *r, int32_t plane, int32_t *n);
/* With STR_ER_STAGE_OCR: per candidate of str_er_result_cands(), the class label chosen by
 * svm_predict_probability and its probability (what OCR::chain_run returns as table[label] + prob,
 * src/OCR.cpp:139); label -1 / prob 0 for candidates that are neither strong nor weak.  NULL otherwise. */
const int32_t *str_er_result_ocr_labels(const str_er_result *r, int32_t *n);
const double  *str_er_result_ocr_probs(const str_er_result *r, int32_t *n);
/* With STR_ER_STAGE_TRACK: per candidate of str_er_result_cands(), what er_track leaves on the ER
 * (ER::color1-3, ER::center) and whether it is in `tracked` (all_er of src/ER.cpp:530).  An image is
 * one frame at one pyramid level (the reference has only level 0): its strong ERs and every weak ER the
 * rule at :575-587 ties, directly or through other tracked ERs, to one of them.  all_er's ORDER (strong
 * lists, then weak ones as found) is not reproduced -- er_grouping sorts it first thing (:614).
 * Records of pool-only candidates (cls 0) are all zero.  NULL without the stage.                   */
const str_er_track *str_er_result_tracks(const str_er_result *r, int32_t *n);
/* With STR_ER_STAGE_GROUP: the text lines (`vector<Text>` of src/ER.cpp:612) of every image, images in plane
 * order.  A line's members are str_er_result_text_ers()[first .. first+count): indices into
 * str_er_result_cands(), in the line's order (sorted by center.x); as in the reference an ER can sit in more
 * than one line, and more than once in a line (:650-661 never merges two lines).  slope = fitline_avgslope of
 * the members that survive overlap_ and inner_suppression; box = union of the members' bounds
 * (the reference fills Text::box here only without DO_OCR, :684-690).
 * Where the reference calls std::sort on center.x (:614, :668) this library sorts STABLY, ties in candidate
 * order / current line order: the reference's order among equal center.x is unspecified (unstable sort over a
 * traversal-dependent input order), so lines that hinge on such ties may legitimately differ from it.
 * overlap_suppression rewrites bound and center of the ERs it merges into (:945-955, shared by all lines):
 * str_er_result_group_bounds() has every candidate's bound and center as er_grouping leaves them.        */
const str_er_text   *str_er_result_texts(const str_er_result *r, int32_t *n);
const int32_t       *str_er_result_text_ers(const str_er_result *r, int32_t *n);
const str_er_gbound *str_er_result_group_bounds(const str_er_result *r, int32_t *n);
/* all_er as er_grouping leaves it (sorted by center.x, minus inner_suppression's victims): candidate indices, images concatenated */
const int32_t       *str_er_result_group_all(const str_er_result *r, int32_t *n);
/* With STR_ER_STAGE_OCR_LINES: the first half of ERFilter::er_ocr (src/ER.cpp:695-747) on the lines of
 * str_er_result_texts().  Parallel to str_er_result_text_ers(): label / prob = what OCR::chain_run(channel[er->ch](er->bound),
 * level * THRESH_STEP, text.slope) returns for that member (bound as er_grouping left it), kept = 1 if the member survives the
 * 0.95-overlap deletion (:700-721) and prob >= MIN_OCR_PROB (:737-741).  Per line: alive = at least 2 members kept (:743-747).
 * The word graph, feedback verification and spelling correction that follow in er_ocr are not part of this library.        */
const int32_t *str_er_result_line_labels(const str_er_result *r, int32_t *n);
const double  *str_er_result_line_probs(const str_er_result *r, int32_t *n);
const uint8_t *str_er_result_line_kept(const str_er_result *r, int32_t *n);
const uint8_t *str_er_result_text_alive(const str_er_result *r, int32_t *n);
/* With STR_ER_WANT_MASKS: one mask record per candidate of str_er_result_cands() (same order), and the words they index
 * (n_words in total).  NULL unless the flag was given.                                                                    */
const str_er_mask *str_er_result_masks(const str_er_result *r, int32_t *n);
const uint32_t    *str_er_result_mask_bits(const str_er_result *r, uint64_t *n_words);
/* With STR_ER_WANT_SHAPES: one descriptor record per candidate of str_er_result_cands() (same order); NULL and 0 without the flag. */
const str_er_shape *str_er_result_shapes(const str_er_result *r, int32_t *n);
/* With STR_ER_WANT_STROKES: one stroke-width record per candidate of str_er_result_cands() (same order); NULL and 0 without the flag. */
const str_er_stroke *str_er_result_strokes(const str_er_result *r, int32_t *n);
/* With STR_ER_WANT_LINE_CROPS: one record per line of str_er_result_texts() (same order), the grey crop bytes they index and, with
 * STR_ER_WANT_LINE_GLYPHS, the glyph crop bytes (same offsets, same size).  NULL without the flag(s).                              */
const str_er_line_crop *str_er_result_line_crops(const str_er_result *r, int32_t *n);
const uint8_t          *str_er_result_line_crop_pixels(const str_er_result *r, uint64_t *n_bytes);
const uint8_t          *str_er_result_line_glyph_pixels(const str_er_result *r, uint64_t *n_bytes);
/* With STR_ER_WANT_TEXT_MAP and / or _LINE_MAP: one record per frame of the call (frame order), and the maps they index (n_bytes
 * bytes / n int32 in total, padding included; layout at str_er_frame_map).  Each accessor returns NULL and 0 without its flag;
 * str_er_result_frame_maps returns the records with either flag.                                                                 */
const str_er_frame_map *str_er_result_frame_maps(const str_er_result *r, int32_t *n);
const uint8_t          *str_er_result_text_map_pixels(const str_er_result *r, uint64_t *n_bytes);
const int32_t          *str_er_result_line_map_ids(const str_er_result *r, uint64_t *n);
/* With STR_ER_WANT_FRAME_LINES (str_er_line_foot): one foot per line of str_er_result_texts() (same order), the pairs of lines with
 * common pixels sorted by (a, b), the frame lines and the line indices their first / count index.  Each returns NULL and 0 without
 * the flag; a grouped call without lines returns empty arrays (not NULL).                                                         */
const str_er_line_foot  *str_er_result_line_feet(const str_er_result *r, int32_t *n);
const str_er_line_pair  *str_er_result_line_pairs(const str_er_result *r, int32_t *n);
const str_er_frame_line *str_er_result_frame_lines(const str_er_result *r, int32_t *n);
const int32_t           *str_er_result_frame_line_members(const str_er_result *r, int32_t *n);
/* With STR_ER_WANT_LINE_LINKS (str_er_line_link): the overlaps of lines of adjacent frames sorted by (a, b), one track index per line
 * of str_er_result_texts(), the text tracks and the line indices their first / count index.  Each returns NULL and 0 without the
 * flag; a call without lines returns empty arrays (not NULL).                                                                      */
const str_er_line_link  *str_er_result_line_links(const str_er_result *r, int32_t *n);
const int32_t           *str_er_result_line_tracks(const str_er_result *r, int32_t *n);
const str_er_text_track *str_er_result_text_tracks(const str_er_result *r, int32_t *n);
const int32_t           *str_er_result_text_track_members(const str_er_result *r, int32_t *n);
/* With STR_ER_WANT_LINE_LINKS: the edge feet of the result, which = 0: of the lines of its first frame, 1: of its last frame (the
 * same frame in a call of one frame).  *n lines; lines[i] is the index into str_er_result_texts(), feet[i] its foot, bits its rows
 * of (w + 31) / 32 words over the foot box, back to back (*n_words in all): what str_er_link_feet takes.  *frame_w, *frame_h: the
 * frame's level-0 size.  STR_ER_EINVAL without the flag or with another `which`; any output pointer may be NULL.                 */
int str_er_result_edge_feet(const str_er_result *r, int32_t which, int32_t *frame_w, int32_t *frame_h, const str_er_line_foot **feet,
                            const int32_t **lines, int32_t *n, const uint32_t **bits, uint64_t *n_words);
/* With STR_ER_WANT_LINE_GEOM (str_er_line_geom): one record per line of str_er_result_texts(), one per frame line of
 * str_er_result_frame_lines(), and the vertex array (x, y pairs, *n_points of them) both sets of records index.  Each returns NULL
 * and 0 without the flag; a call without lines returns empty arrays (not NULL).                                                    */
const str_er_line_geom  *str_er_result_line_geoms(const str_er_result *r, int32_t *n);
const str_er_line_geom  *str_er_result_frame_line_geoms(const str_er_result *r, int32_t *n);
const int32_t           *str_er_result_geom_points(const str_er_result *r, int32_t *n_points);
/* With STR_ER_WANT_LINE_WORDS (str_er_line_run): one str_er_line_words per line of str_er_result_texts(), the runs and the words they
 * index.  Each returns NULL and 0 without the flag; a call without lines returns empty arrays (not NULL).                          */
const str_er_line_words *str_er_result_line_words(const str_er_result *r, int32_t *n);
const str_er_line_run   *str_er_result_line_runs(const str_er_result *r, int32_t *n);
const str_er_line_word  *str_er_result_words(const str_er_result *r, int32_t *n);
/* With STR_ER_WANT_RUN_READ (str_er_run_read): one record per run of str_er_result_line_runs(), in the same order, and the 1800 * n
 * feature bytes of the runs.  Each returns NULL and 0 without the flag; a call without runs returns empty arrays (not NULL).       */
const str_er_run_read   *str_er_result_run_reads(const str_er_result *r, int32_t *n);
const uint8_t           *str_er_result_run_features(const str_er_result *r, uint64_t *n_bytes);
/* With STR_ER_WANT_WORD_MATCH (str_er_word_match): one record per word of str_er_result_words(), the 65 * n cost bytes of the runs
 * and their k * n class probabilities (k: nr_class of str_er_svm_info, in the model's class order), the runs in the order of
 * str_er_result_line_runs().  Each returns NULL and 0 without the flag; a call without runs returns empty arrays (not NULL).  The
 * cost bytes also come with STR_ER_WANT_WORD_DECODE and with STR_ER_WANT_RUN_SPLIT (unfolded where there is no matcher).             */
const str_er_word_match *str_er_result_word_matches(const str_er_result *r, int32_t *n);
const uint8_t           *str_er_result_run_costs(const str_er_result *r, uint64_t *n_bytes);
const double            *str_er_result_run_probs(const str_er_result *r, uint64_t *n_values);
/* With STR_ER_WANT_WORD_DECODE (str_er_word_decode): one record per word of str_er_result_words() and 64 label bytes and 64 source
 * bytes per word; str_er_result_run_costs and _run_probs are filled with this flag too: the unfolded rows, unless
 * STR_ER_WANT_WORD_MATCH is set as well, when they stay the matcher's (folded as its lexicon says).  Each returns NULL and 0 without
 * the flag; a call without words returns empty arrays (not NULL).                                                                  */
const str_er_word_decode *str_er_result_word_decodes(const str_er_result *r, int32_t *n);
const uint8_t            *str_er_result_word_decode_chars(const str_er_result *r, uint64_t *n_bytes);
const uint8_t            *str_er_result_word_decode_src(const str_er_result *r, uint64_t *n_bytes);
/* With STR_ER_WANT_WORD_DECODE on a context whose str_er_set_word_margin is on (str_er_word_margin): one record per word of
 * str_er_result_words(), 32 int32 row margins per word (n_bytes: 128 per word) and 32 bytes of row readings and of row alternatives
 * per word; with STR_ER_WANT_RUN_SPLIT the rows are the word's parts, as for the decoder.  Each returns NULL and 0 when the call made
 * none; a call without words returns empty arrays (not NULL).                                                                      */
const str_er_word_margin *str_er_result_word_margins(const str_er_result *r, int32_t *n);
const int32_t            *str_er_result_word_row_margins(const str_er_result *r, uint64_t *n_bytes);
const uint8_t            *str_er_result_word_row_reads(const str_er_result *r, uint64_t *n_bytes);
const uint8_t            *str_er_result_word_row_alts(const str_er_result *r, uint64_t *n_bytes);
/* With STR_ER_WANT_WORD_DECODE on a context whose str_er_set_line_decode is on (str_er_line_decode): one record per line of
 * str_er_result_texts(); the labels (3 bytes per row: a row is a run of str_er_result_line_runs(), with STR_ER_WANT_RUN_SPLIT a part
 * of str_er_result_split_parts()), the sources (uint16, n: their number) and word_of_row (one per row); the gap costs used (2 bytes
 * per row) and the lines' windows into the rows (2 int32 per line: first row, row count).  Each returns NULL and 0 when the call made none; a call without lines returns empty arrays (not NULL).             */
const str_er_line_decode *str_er_result_line_decodes(const str_er_result *r, int32_t *n);
const uint8_t            *str_er_result_line_decode_chars(const str_er_result *r, uint64_t *n_bytes);
const uint16_t           *str_er_result_line_decode_src(const str_er_result *r, uint64_t *n);
const int32_t            *str_er_result_line_decode_word_of_row(const str_er_result *r, uint64_t *n);
const uint8_t            *str_er_result_line_gap_costs(const str_er_result *r, uint64_t *n_bytes);
const int32_t            *str_er_result_line_decode_windows(const str_er_result *r, uint64_t *n);
/* With the line decode on a context whose str_er_set_line_margin is on (str_er_line_margin): one record per line of
 * str_er_result_texts(), and per row of the line decode's rows a row margin and a gap margin (int32, n_bytes: their bytes), a reading,
 * an alternative and a gap move (one byte each).  Each returns NULL and 0 when the call made none; a call without lines returns empty
 * arrays (not NULL).                                                                                                              */
const str_er_line_margin *str_er_result_line_margins(const str_er_result *r, int32_t *n);
const int32_t            *str_er_result_line_row_margins(const str_er_result *r, uint64_t *n_bytes);
const uint8_t            *str_er_result_line_row_reads(const str_er_result *r, uint64_t *n_bytes);
const uint8_t            *str_er_result_line_row_alts(const str_er_result *r, uint64_t *n_bytes);
const int32_t            *str_er_result_line_gap_margins(const str_er_result *r, uint64_t *n_bytes);
const uint8_t            *str_er_result_line_gap_moves(const str_er_result *r, uint64_t *n_bytes);
/* With STR_ER_WANT_RUN_SPLIT (str_er_run_split): one split record per run of str_er_result_line_runs(); the pieces they index, with
 * one reading and one 65-byte cost row per piece; the parts of the words back to back in word order; one record per word of
 * str_er_result_words().  NULL (and *n = 0) without the flag.                                                                       */
const str_er_run_split   *str_er_result_run_splits(const str_er_result *r, int32_t *n);
const str_er_run_piece   *str_er_result_run_pieces(const str_er_result *r, int32_t *n);
const str_er_run_read    *str_er_result_piece_reads(const str_er_result *r, int32_t *n);
const uint8_t            *str_er_result_piece_costs(const str_er_result *r, uint64_t *n_bytes);
const str_er_split_part  *str_er_result_split_parts(const str_er_result *r, int32_t *n);
const str_er_word_split  *str_er_result_word_splits(const str_er_result *r, int32_t *n);
/* With STR_ER_WANT_LATTICE_DECODE (str_er_lattice_decode): one record per word of str_er_result_words(), 64 label bytes and 64 source
 * bytes per word, and the lattice parts of the words back to back in word order.  Each returns NULL and 0 without the flag; a call
 * without words returns empty arrays (not NULL).                                                                                   */
const str_er_lattice_decode *str_er_result_lattice_decodes(const str_er_result *r, int32_t *n);
/* With STR_ER_WANT_LATTICE_DECODE on a context whose str_er_set_line_lattice_decode is on (str_er_line_lattice_decode): one record per
 * line of str_er_result_texts(); with S the sum of n_cuts + 1 over str_er_result_run_splits(), 3 * S label bytes and 3 * S uint16
 * sources, a line's slice at 3 * (the atoms of all runs before its first run); the lines' parts back to back (first_part, n_parts)
 * with the indices of str_er_result_split_parts() and one int32 per part, the number of breaks before it (-1: dropped); the gap
 * costs used, 2 bytes per run of str_er_result_line_runs() (str_er_line_gap_costs on the runs, row_run == NULL, at the setting's
 * weight); and the lines' windows into the runs, (first run, run count) per line.  In a detect call a line's window runs from the
 * first run of its first word to the last run of its last word; the kernel follows the lattice decode on the same stream and its
 * tables come down with the stage's one wait.  NULL (and 0) without the flag or the setting.                                         */
const str_er_line_lattice_decode *str_er_result_line_lattice_decodes(const str_er_result *r, int32_t *n);
const uint8_t *str_er_result_line_lattice_chars(const str_er_result *r, uint64_t *n_bytes);
const uint16_t *str_er_result_line_lattice_src(const str_er_result *r, uint64_t *n);
const str_er_split_part *str_er_result_line_lattice_parts(const str_er_result *r, int32_t *n);
const int32_t *str_er_result_line_lattice_word_of_part(const str_er_result *r, uint64_t *n);
const uint8_t *str_er_result_line_lattice_gap_costs(const str_er_result *r, uint64_t *n_bytes);
const int32_t *str_er_result_line_lattice_windows(const str_er_result *r, uint64_t *n);
const uint8_t               *str_er_result_lattice_decode_chars(const str_er_result *r, uint64_t *n_bytes);
const uint8_t               *str_er_result_lattice_decode_src(const str_er_result *r, uint64_t *n_bytes);
const str_er_split_part     *str_er_result_lattice_parts(const str_er_result *r, int32_t *n);
/* With STR_ER_WANT_LATTICE_DECODE on a context whose str_er_set_lattice_margin is on (str_er_lattice_margin): one record per word of
 * str_er_result_words(); per word 32 int32 reading margins and 32 int32 cut margins (n_bytes: 128 per word each) and 32 bytes each of
 * readings, alternatives and cut alternatives, indexed by the word-relative part of str_er_result_lattice_parts().  Each returns NULL
 * and 0 when the call made none; a call without words returns empty arrays (not NULL).                                              */
const str_er_lattice_margin *str_er_result_lattice_margins(const str_er_result *r, int32_t *n);
const int32_t               *str_er_result_lattice_read_margins(const str_er_result *r, uint64_t *n_bytes);
const int32_t               *str_er_result_lattice_cut_margins(const str_er_result *r, uint64_t *n_bytes);
const uint8_t               *str_er_result_lattice_part_reads(const str_er_result *r, uint64_t *n_bytes);
const uint8_t               *str_er_result_lattice_part_alts(const str_er_result *r, uint64_t *n_bytes);
const uint8_t               *str_er_result_lattice_cut_alts(const str_er_result *r, uint64_t *n_bytes);
/* With STR_ER_WANT_LATTICE_MATCH (str_er_lattice_match): one record per word of str_er_result_words(), 32 source bytes per word, and the
 * parts of the winning entries back to back in word order.  Each returns NULL and 0 without the flag; a call without words returns
 * empty arrays (not NULL).                                                                                                          */
const str_er_lattice_match  *str_er_result_lattice_matches(const str_er_result *r, int32_t *n);
const uint8_t               *str_er_result_lattice_match_src(const str_er_result *r, uint64_t *n_bytes);
const str_er_split_part     *str_er_result_lattice_match_parts(const str_er_result *r, int32_t *n);
/* With STR_ER_WANT_TRACK_READ (str_er_word_link): the word links sorted by (a, b); the word tracks; their members (word indices); one
 * track index per word of str_er_result_words() (-1: not eligible); one match per word track; one cost per slot of the member array.
 * Each returns NULL and 0 without the flag; a call without words returns empty arrays (not NULL).  The first four answer for
 * STR_ER_WANT_TRACK_DECODE as well; the matches and their member costs are STR_ER_WANT_TRACK_READ's alone.                          */
const str_er_word_link   *str_er_result_word_links(const str_er_result *r, int32_t *n);
const str_er_word_track  *str_er_result_word_tracks(const str_er_result *r, int32_t *n);
const int32_t            *str_er_result_word_track_members(const str_er_result *r, int32_t *n);
const int32_t            *str_er_result_word_track_of_words(const str_er_result *r, int32_t *n);
const str_er_track_match *str_er_result_track_matches(const str_er_result *r, int32_t *n);
const int32_t            *str_er_result_track_member_costs(const str_er_result *r, int32_t *n);
/* With STR_ER_WANT_TRACK_DECODE (str_er_track_decode): one record and 32 label bytes per word track of str_er_result_word_tracks(), and
 * one cost per slot of str_er_result_word_track_members().  Each returns NULL and 0 without the flag; a call without words returns
 * empty arrays (not NULL).                                                                                                          */
const str_er_track_decode *str_er_result_track_decodes(const str_er_result *r, int32_t *n);
const uint8_t             *str_er_result_track_decode_chars(const str_er_result *r, uint64_t *n_bytes);
const int32_t             *str_er_result_track_decode_member_costs(const str_er_result *r, int32_t *n);
/* With STR_ER_WANT_LATTICE_TRACK (str_er_lattice_track_member): one match per word track of str_er_result_word_tracks(), one record and
 * 32 source bytes per slot of str_er_result_word_track_members(), and the members' parts back to back in slot order.  Each returns NULL
 * and 0 without the flag; a call without words returns empty arrays (not NULL).                                                      */
const str_er_track_match          *str_er_result_lattice_track_matches(const str_er_result *r, int32_t *n);
const str_er_lattice_track_member *str_er_result_lattice_track_members(const str_er_result *r, int32_t *n);
const uint8_t                     *str_er_result_lattice_track_src(const str_er_result *r, uint64_t *n_bytes);
const str_er_split_part           *str_er_result_lattice_track_parts(const str_er_result *r, int32_t *n);
/* With str_er_set_lattice_track_decode on and both STR_ER_WANT_TRACK_DECODE and STR_ER_WANT_LATTICE_DECODE (str_er_lattice_track_decode):
 * one record and 32 label bytes per word track of str_er_result_word_tracks(), one record and 32 source bytes per slot of
 * str_er_result_word_track_members(), and the members' parts back to back in slot order.  Each returns NULL and 0 otherwise; a call
 * without words returns empty arrays (not NULL).                                                                                   */
const str_er_track_decode         *str_er_result_lattice_track_decodes(const str_er_result *r, int32_t *n);
const uint8_t                     *str_er_result_lattice_track_decode_chars(const str_er_result *r, uint64_t *n_bytes);
const str_er_lattice_track_member *str_er_result_lattice_track_decode_members(const str_er_result *r, int32_t *n);
const uint8_t                     *str_er_result_lattice_track_decode_src(const str_er_result *r, uint64_t *n_bytes);
const str_er_split_part           *str_er_result_lattice_track_decode_parts(const str_er_result *r, int32_t *n);
/* Kept-node table of one plane, ascending (key, level); NULL unless STR_ER_WANT_NODES. */
const str_er_node *str_er_result_plane_nodes(const str_er_result *r, int32_t plane, int32_t *n);
/* times[7] = {extract, nms, classify, track, group, ocr, total} seconds, the contract of
 * ERFilter::text_detect's return value (src/ER.cpp:99-110); track, group and ocr are filled by their stages.
 * extract/nms/classify are GPU stage times for the whole batch (HIP events).          */
const double *str_er_result_times(const str_er_result *r);
/* Device copy of the candidate array (for an RCCL gather without a host round trip):
 * copies min(n, cap) records to dst_dev on the context's stream and synchronises.     */
int  str_er_result_cands_to_device(str_er_ctx *ctx, const str_er_result *r, void *dst_dev,
                                   int32_t cap, int32_t *n);
void str_er_result_free(str_er_result *r);

/* ---- one plane in strips over several GPUs (no reference counterpart) -----------------------
 * The level-0 planes of ONE frame cut into n_strips bands of tile rows.  Every participant calls str_er_strip_extract with the
 * frame and its strip number: compute_channels, the tile trees of the strip and the seams inside it, for every channel of the
 * context; the blob holds the strip's node records and the node of every pixel of its first and last row -- plain bytes, to be
 * brought to the plane's owner by any transport.  The owner calls str_er_strip_merge with the frame and all n_strips blobs (in
 * strip order): records behind one another, seams across the cuts joined, then the usual passes; the result is the one
 * str_er_detect_bgr gives for the level-0 planes of the frame (same planes, same records).  Equal parameters on all participants;
 * a context with a pyramid strips its level-0 planes only (the smaller planes are dealt out whole: str_er_detect_bgr_planes).
 * A blob is checked before it is used (sizes against the headers, rows against the cut, every node id against its strip's record
 * count): a damaged or foreign one gives STR_ER_EFORMAT, never an out-of-range device access.
 *   _extract      *blob is malloc'ed host memory (str_er_strip_free)
 *   _extract_dev  *d_blob is a device buffer of the context, valid until its next strip call: with str_er_comm_allgather_bytes
 *                 (STR_ER_MEM_DEVICE in and out) over an RCCL communicator a blob goes from GPU to GPU without touching a host
 *   _merge        host blobs, all channels;  _merge_ex: blobs in host or device memory (blob_kind), and plane_select (one byte per
 *                 channel of the context, or NULL = all): the channels THIS owner puts together -- different planes of one frame
 *                 can have different owners                                                                                     */
int  str_er_strip_extract(str_er_ctx *ctx, const uint8_t *bgr, int32_t w, int32_t h, int64_t stride, int mem_kind,
                          int32_t strip, int32_t n_strips, void **blob, int64_t *blob_bytes);
int  str_er_strip_extract_dev(str_er_ctx *ctx, const uint8_t *bgr, int32_t w, int32_t h, int64_t stride, int mem_kind,
                              int32_t strip, int32_t n_strips, const void **d_blob, int64_t *blob_bytes);
void str_er_strip_free(void *blob);
int  str_er_strip_merge(str_er_ctx *ctx, const uint8_t *bgr, int32_t w, int32_t h, int64_t stride, int mem_kind,
                        const void *const *blobs, const int64_t *blob_bytes, int32_t n_strips, uint32_t stages,
                        str_er_result **out);
int  str_er_strip_merge_ex(str_er_ctx *ctx, const uint8_t *bgr, int32_t w, int32_t h, int64_t stride, int mem_kind,
                           const void *const *blobs, const int64_t *blob_bytes, int blob_kind, int32_t n_strips,
                           const uint8_t *plane_select, uint32_t stages, str_er_result **out);

/* ---- multi-GPU: the one exchange of the path ------------------------------------------
 * One process per GPU; frames (or planes) are dealt out to the ranks and only the candidate records travel, where the
 * reference's er_track reads the strong / weak lists of every plane (src/ER.cpp:63):
 *     all_gather(my count) -> all_gather(records padded to the largest count) -> padding dropped, frame offsets added.
 * A communicator is an RCCL communicator (librccl.so is loaded on first use; ncclAllGather over xGMI on a stream of its own)
 * or a member of an in-process group that exchanges through host memory (tests without a GPU; one thread per rank).     */
typedef struct str_er_comm str_er_comm;
typedef struct str_er_comm_group str_er_comm_group;
/* RCCL: rank 0 makes the 128-byte id (ncclGetUniqueId) and hands it to the others by any means; all ranks then create. */
int  str_er_comm_unique_id(void *id128);
int  str_er_comm_create(int32_t device, int32_t rank, int32_t world, const void *id128, str_er_comm **out);
/* in-process group of `world` ranks */
int  str_er_comm_local_group(int32_t world, str_er_comm_group **out);
int  str_er_comm_create_local(str_er_comm_group *g, int32_t rank, str_er_comm **out);
void str_er_comm_local_group_free(str_er_comm_group *g);
void str_er_comm_destroy(str_er_comm *c);
int32_t str_er_comm_rank(const str_er_comm *c);
int32_t str_er_comm_world(const str_er_comm *c);
const char *str_er_comm_last_error(const str_er_comm *c);
/* Collective: every rank passes its records (host memory) and the number to add to their `frame` field; every rank receives
 * all records ordered by rank (*all, free with str_er_gather_free) and, if counts != NULL, the per-rank counts.            */
int  str_er_gather_cands(str_er_comm *c, const str_er_cand *local, int32_t n_local, uint32_t frame_offset,
                         str_er_cand **all, int32_t *n_all, int32_t *counts);
/* The same for the candidates of ctx's last detect call, taken from the device array they are still in: no host hop on
 * the sending side (RCCL communicators only).                                                                             */
int  str_er_gather_last(str_er_comm *c, str_er_ctx *ctx, uint32_t frame_offset, str_er_cand **all, int32_t *n_all,
                        int32_t *counts);
void str_er_gather_free(str_er_cand *p);
/* Collective: a variable-length all-gather of plain bytes (the strip blobs of str_er_strip_extract).  `local` is host or device memory
 * (in_kind).  out_kind STR_ER_MEM_HOST: *all is malloc'ed (str_er_comm_free) and holds the contributions back to back; STR_ER_MEM_DEVICE:
 * *all points into a device buffer of the communicator, valid until its next collective -- with an RCCL communicator and device input
 * the bytes never touch the host.  starts[k] / sizes[k] (world entries each): where rank k's bytes are in *all.
 * A rank whose arguments are bad still joins the exchange of the sizes: every rank then returns an error, none is left waiting.      */
int  str_er_comm_allgather_bytes(str_er_comm *c, const void *local, int64_t n_local, int in_kind, int out_kind,
                                 void **all, int64_t *starts, int64_t *sizes);
void str_er_comm_free(void *p);

/* ---- introspection / measurement --------------------------------------------------- */
/* Per-kernel-group GPU time of the LAST detect call, measured with HIP events on the
 * context's stream.  names[i] are static strings.  Returns the number of groups.      */
int str_er_last_profile(const str_er_ctx *ctx, const char **names, double *ms, int32_t cap);
/* Enable (1) / disable (0) the per-group events above (default 0: two events per call). */
int str_er_set_profiling(str_er_ctx *ctx, int enable);
/* Bytes of device workspace held by the context. */
int64_t str_er_workspace_bytes(const str_er_ctx *ctx);

/* ---- frame ingest ------------------------------------------------------------------
 * The reference takes its frames from the host (cv::imread / `cap >> frame`, src/utils.cpp:31, 59-82, 109) and calls
 * text_detect on each.  A str_er_stream keeps `depth` batches in flight: it owns `depth` contexts (same parameters,
 * each with its own HIP stream and workspace), one page-locked staging buffer per context and a worker thread per
 * context, so the upload of one batch overlaps the kernels of the others.  Producer loop:
 *
 *     str_er_stream_acquire(s, &slot, &buf, &cap);     // a pinned buffer of max_frames * max_width * max_height * 3 bytes
 *     ... decode / copy up to max_frames BGR frames into buf ...
 *     str_er_stream_submit(s, slot, w, h, stride, frame_pitch, n_frames, stages, &ticket);
 *     if (str_er_stream_pending(s) == depth) str_er_stream_next(s, &result, &ticket);   // oldest first; blocks until it is done
 *
 * Photographs of assorted sizes: decode each into the buffer at an offset of your choosing and submit the list of them with
 * str_er_stream_submit_list (NV12: str_er_stream_submit_nv12_list) instead.
 *
 * acquire never blocks: with every buffer in flight it returns STR_ER_ESTATE (collect a result first).  Results come
 * back in submission order and are freed with str_er_result_free.  Models are loaded into every context with
 * str_er_stream_load_cascade (other per-context calls: str_er_stream_context).  One producer/consumer thread at a time. */
typedef struct str_er_stream str_er_stream;
int         str_er_stream_create(const str_er_params *p, int32_t depth, str_er_stream **out);
void        str_er_stream_destroy(str_er_stream *s);
int32_t     str_er_stream_depth(const str_er_stream *s);
str_er_ctx *str_er_stream_context(str_er_stream *s, int32_t i);
const char *str_er_stream_last_error(const str_er_stream *s);
int         str_er_stream_load_cascade(str_er_stream *s, int which, const char *path);
int         str_er_stream_acquire(str_er_stream *s, int32_t *slot, uint8_t **buffer, int64_t *capacity);
int         str_er_stream_submit(str_er_stream *s, int32_t slot, int32_t w, int32_t h, int64_t stride, int64_t frame_pitch,
                                 int32_t n_frames, uint32_t stages, uint64_t *ticket);
/* ... the staging buffer holds NV12 frames (str_er_detect_nv12): stride >= w, a frame is h + h/2 rows */
int         str_er_stream_submit_nv12(str_er_stream *s, int32_t slot, int32_t w, int32_t h, int64_t stride, int64_t frame_pitch,
                                      int32_t n_frames, uint32_t stages, uint64_t *ticket);
/* convenience: acquire + copy the frames in (one extra host copy) + submit */
int         str_er_stream_submit_copy(str_er_stream *s, const uint8_t *bgr, int32_t w, int32_t h, int64_t stride, int64_t frame_pitch,
                                      int32_t n_frames, uint32_t stages, uint64_t *ticket);
/* A list of BGR frames of assorted sizes in the slot's staging buffer (str_er_detect_bgr_list): every frames[i].data points into
 * the buffer str_er_stream_acquire returned for `slot`, at any offset and stride; the refs array is copied here.  The worker
 * uploads the byte span from the lowest frame start to the highest frame end and detects on the copy in device memory; frame i
 * of the result is what str_er_detect_bgr gives for that frame alone, with frame = i.  Checked here: a frame not wholly inside
 * the buffer, a stride below a row, a NULL data or an empty frame -> STR_ER_EINVAL; a frame over max_width x max_height or
 * n > max_frames -> STR_ER_ECAPACITY; the message names the frame and the slot stays acquired.  Uniform and list submissions
 * may alternate on one stream; results come back in ticket order.                                                          */
int         str_er_stream_submit_list(str_er_stream *s, int32_t slot, const str_er_image_ref *frames, int32_t n, uint32_t stages,
                                      uint64_t *ticket);
/* ... the same for NV12 frames (str_er_detect_nv12_list): a frame is h + h/2 rows of `stride` bytes; odd w or h -> STR_ER_EINVAL */
int         str_er_stream_submit_nv12_list(str_er_stream *s, int32_t slot, const str_er_image_ref *frames, int32_t n, uint32_t stages,
                                           uint64_t *ticket);
/* convenience, BGR: acquire + pack the frames (host memory) into the buffer + str_er_stream_submit_list.  Frames start at 4-byte
 * boundaries when the padded total fits the buffer, otherwise back to back.  On an error no slot stays acquired.           */
int         str_er_stream_submit_copy_list(str_er_stream *s, const str_er_image_ref *frames, int32_t n, uint32_t stages, uint64_t *ticket);
int         str_er_stream_next(str_er_stream *s, str_er_result **out, uint64_t *ticket);
int32_t     str_er_stream_pending(str_er_stream *s);

#ifdef __cplusplus
}
#endif
#endif /* STR_ER_H */
