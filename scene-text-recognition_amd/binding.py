"""ctypes binding of include/str_er.h.

`ERFilter` mirrors the reference's `class ERFilter` (inc/ER.h:110-169) for the hot path:
same constructor arguments and method names (`text_detect`, `compute_channels`,
`er_tree_extract`, `non_maximum_supression`, `classify`, `make_LBP_hist`,
`set_thresh_step`, `set_min_area`), results as numpy structured arrays instead of
heap `ER*` trees.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

STAGE_EXTRACT, STAGE_NMS, STAGE_CLASSIFY, STAGE_ALL, STAGE_OCR, WANT_NODES, STAGE_TRACK = 1, 2, 4, 7, 8, 16, 32
STAGE_GROUP, GROUP_INNER_SUP, STAGE_OCR_LINES, GROUP_OVERLAP_SUP = 64, 128, 256, 512
WANT_MASKS = 1024       # output option: the pixel mask of every candidate (Result.mask)
# str_er_mask: mask i = pitch_words 32-bit words per row, h rows, from word word_off of the call's mask words; pixels = popcount
MASK_DTYPE = np.dtype([("word_off", "<u8"), ("pixels", "<u4"), ("pitch_words", "<u4")])
# output options (need STAGE_GROUP): a rectified grey crop of every text line, and with WANT_LINE_GLYPHS too its glyph crop (Result.line_crop)
WANT_LINE_CROPS, WANT_LINE_GLYPHS = 2048, 4096
WANT_SHAPES = 8192      # output option: the shape and intensity descriptors of every candidate (Result.shapes)
# str_er_shape: exact integers over the candidate's mask M (include/str_er.h); ERStat's hole_area_ratio = hole_pixels / pixels,
# convex_hull_ratio = hull_area2 / (2 * pixels), med_crossings = crossings[3]
SHAPE_DTYPE = np.dtype([("pixels", "<u4"), ("perimeter", "<u4"), ("euler", "<i4"), ("hole_pixels", "<u4"), ("crossings", "<u2", (4,)),
                        ("hull_area2", "<u8"), ("grey_sum", "<u8"), ("grey_sum2", "<u8")])
WANT_STROKES = 65536    # output option: the stroke-width descriptor of every candidate (Result.strokes)
# str_er_stroke: exact integers over the candidate's mask M (include/str_er.h): K erosions (4- and 8-neighbourhoods in turn) empty M;
# the mean ridge depth m = ridge_depth_sum / ridge_pixels gives the stroke width 2m - 1 (odd) or 2m (even), and
# ridge_depth_sum2 / ridge_pixels - m * m its spread
STROKE_DTYPE = np.dtype([("depth_max", "<u4"), ("ridge_pixels", "<u4"), ("depth_sum", "<u8"), ("ridge_depth_sum", "<u8"),
                         ("ridge_depth_sum2", "<u8")])
# output options: frame-resolution maps (Result.text_map / Result.line_map).  WANT_TEXT_MAP (needs STAGE_CLASSIFY): one uint8 map per
# frame at its own size, the OR of the TEXT_MAP_* bits of every region covering the pixel; WANT_LINE_MAP (needs STAGE_GROUP): one
# int32 map per frame, the smallest index into texts of a line with a member covering the pixel, -1 where none does
WANT_TEXT_MAP, WANT_LINE_MAP = 16384, 32768
TEXT_MAP_STRONG, TEXT_MAP_WEAK, TEXT_MAP_LINE, TEXT_MAP_OCR = 1, 2, 4, 8
# str_er_frame_map: frame f's maps = height x width elements (pitch width) from element off of the byte map and of the id map
FRAME_MAP_DTYPE = np.dtype([("off", "<u8"), ("width", "<i4"), ("height", "<i4")])
# output option: one list of text lines per frame, the lines of different pyramid levels that are the same text joined (needs
# STAGE_GROUP; Result.line_feet / line_pairs / frame_lines / frame_line_members; the contract is at str_er_line_foot in include/str_er.h)
WANT_FRAME_LINES = 131072
# str_er_line_foot: per line of texts, its footprint's box and pixel count in frame pixels and its frame line
LINE_FOOT_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"), ("pixels", "<u4"), ("frame_line", "<i4")])
# str_er_line_pair: two lines a < b of one frame with inter > 0 common pixels; dup: duplicates at the call's threshold
LINE_PAIR_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("inter", "<u4"), ("dup", "<u4")])
# str_er_frame_line: members = frame_line_members[first:first + count] (line indices, ascending), rep the one with the most pixels
FRAME_LINE_DTYPE = np.dtype([("frame", "<u4"), ("rep", "<i4"), ("first", "<i4"), ("count", "<i4"), ("x", "<i4"), ("y", "<i4"), ("w", "<i4"),
                             ("h", "<i4"), ("pixels", "<u4"), ("levels", "<u4")])
# output option: the lines of consecutive frames linked into text tracks (needs WANT_FRAME_LINES; Result.line_links / line_tracks /
# text_tracks / text_track_members / edge_feet(which); the contract is at str_er_line_link in include/str_er.h)
WANT_LINE_LINKS = 262144
# str_er_line_link: a line a of frame f and a line b of the adjacent frame f + 1 with inter > 0 common pixels; link: linked at the call's threshold
LINE_LINK_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("inter", "<u4"), ("link", "<u4")])
# str_er_text_track: members = text_track_members[first:first + count] (line indices, ascending), rep the one with the most pixels
TEXT_TRACK_DTYPE = np.dtype([("first_frame", "<u4"), ("last_frame", "<u4"), ("first", "<i4"), ("count", "<i4"), ("rep", "<i4"), ("pixels", "<u4")])
# output option: the convex hull, the moments and the oriented box of every text line and frame line (needs WANT_FRAME_LINES;
# Result.line_geoms / frame_line_geoms / geom_points / line_hull / line_quad; the contract is at str_er_line_geom in include/str_er.h)
WANT_LINE_GEOM = 524288
# str_er_line_geom: the hull vertices are geom_points[first:first + count]; the box is that of hull edge `edge`, corners (qx[k], qy[k])
LINE_GEOM_DTYPE = np.dtype([("first", "<u4"), ("count", "<u4"), ("hull_area2", "<u8"), ("m10", "<u8"), ("m01", "<u8"), ("m20", "<u8"), ("m11", "<u8"),
                            ("m02", "<u8"), ("pixels", "<u4"), ("edge", "<i4"), ("ex", "<i4"), ("ey", "<i4"), ("dmin", "<i8"), ("dmax", "<i8"),
                            ("cmin", "<i8"), ("cmax", "<i8"), ("qx", "<f8", (4,)), ("qy", "<f8", (4,))])
# output option: every text line split into glyph runs and words (needs WANT_FRAME_LINES; Result.line_words / line_runs / words /
# words_of_line / runs_of_line / frame_line_words; the contract is at str_er_line_run in include/str_er.h)
WANT_LINE_WORDS = 1048576
# output option: every glyph run read by the OCR scorer (needs WANT_LINE_WORDS and an SVM model of dim 1800; Result.run_reads /
# run_features / word_text / words_text_of_line / frame_line_text; the contract is at str_er_run_read in include/str_er.h)
WANT_RUN_READ = 2097152
# output option: every word matched against the lexicon of set_lexicon (needs WANT_RUN_READ and a lexicon; Result.word_matches /
# run_costs / run_probs / word_match_text / words_match_text_of_line / frame_line_match_text; the contract is at str_er_word_match)
WANT_WORD_MATCH = 4194304
LEXICON_FOLD_CASE = 1
# output option: every word decoded under the bigram table of set_bigram (needs WANT_RUN_READ and a table, no lexicon;
# Result.word_decodes / word_decode_chars / word_decode_src / word_decode_text / word_decode_runs / words_decode_text_of_line /
# frame_line_decode_text, and run_costs / run_probs; the contract is at str_er_word_decode)
WANT_WORD_DECODE = 8388608
# output option: every glyph run cut at the valleys of its column profile, every piece read, per run the segmentation the scorer likes
# best (needs WANT_RUN_READ; Result.run_splits / run_pieces / piece_reads / piece_costs / split_parts / word_splits / word_split_text /
# words_split_text_of_line / frame_line_split_text; the contract is at str_er_run_split).  Beside WANT_WORD_MATCH / WANT_WORD_DECODE both
# work on the split sequence of a word: word_decode_src then indexes the word's parts
WANT_RUN_SPLIT = 16777216
# output option: the words of adjacent frames linked into word tracks and one lexicon match per word track over the cost rows of all
# its members (needs WANT_LINE_LINKS and WANT_WORD_MATCH; Result.word_links / word_tracks / word_track_members / word_track_of_words /
# track_matches / track_member_costs / word_track_text / text_track_match_text; the contract is at str_er_word_link)
WANT_TRACK_READ = 33554432
WANT_LATTICE_DECODE = 67108864
# every word of WANT_RUN_SPLIT against the lexicon with the segmentation of its runs free: the best and second entry over the lattice of all
# pieces of all its runs, the winner's parts and sources (needs WANT_RUN_SPLIT and WANT_WORD_MATCH; Result.lattice_matches /
# lattice_match_src / lattice_match_parts / word_lattice_match_text; the contract is at str_er_lattice_match)
WANT_LATTICE_MATCH = 134217728
# every word track of WANT_TRACK_READ against the lexicon over the piece lattices of all its members: the pooled evidence chooses the entry,
# and for it every member gets its own parts and sources (needs WANT_TRACK_READ and WANT_LATTICE_MATCH; Result.lattice_track_matches /
# lattice_track_members / lattice_track_src / lattice_track_parts / word_track_lattice_text; the contract is at str_er_lattice_track_member)
WANT_LATTICE_TRACK = 268435456
# every word track decoded without a lexicon: the median string of its members under the bigram table, from the members' own decoder
# strings by single edits (needs WANT_LINE_LINKS and WANT_WORD_DECODE, no lexicon; Result.track_decodes / track_decode_chars /
# track_decode_member_costs / word_track_decode_text / text_track_decode_text, and word_links / word_tracks / word_track_members /
# word_track_of_words; the contract is at str_er_track_decode)
WANT_TRACK_DECODE = 536870912
# str_er_track_decode: per word track, J of the string and of the set median it started from (-1: no seed, not decoded), its length,
# the edits taken, whether no single edit improves it, the usable members, the word whose decoder string was the seed, and lm of the string
TRACK_DECODE_DTYPE = np.dtype([("cost", "<i4"), ("seed_cost", "<i4"), ("n_chars", "<i4"), ("n_edits", "<i4"), ("converged", "<i4"), ("n_used", "<i4"),
                               ("seed_member", "<i4"), ("lm_cost", "<i4")])
assert TRACK_DECODE_DTYPE.itemsize == 32
# str_er_lattice_track_member: per slot of the member array, the member's own cost for its track's entry (-1: none), its parts in the
# lattice track part table, the parts dropped and the characters inserted, and the member (a word index; -1 in a slot of no track)
LATTICE_TRACK_MEMBER_DTYPE = np.dtype([("cost", "<i4"), ("first_part", "<i4"), ("n_parts", "<i4"), ("n_del", "<i4"), ("n_ins", "<i4"), ("word", "<i4")])
assert LATTICE_TRACK_MEMBER_DTYPE.itemsize == 24
# str_er_word_link: a word a of frame f and a word b of the adjacent frame f + 1 whose boxes share inter > 0 pixels; link: linked at the call's threshold
WORD_LINK_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("inter", "<u4"), ("link", "<u4")])
# str_er_word_track: members = word_track_members[first:first + count] (word indices, ascending), rep the one with the most pixels
WORD_TRACK_DTYPE = np.dtype([("first_frame", "<u4"), ("last_frame", "<u4"), ("first", "<i4"), ("count", "<i4"), ("rep", "<i4"), ("text_track", "<i4")])
# str_er_track_match: str_er_word_match over the summed costs of the usable members, their number and the word with the smallest own cost
TRACK_MATCH_DTYPE = np.dtype([("entry", "<i4"), ("cost", "<i4"), ("second_entry", "<i4"), ("second_cost", "<i4"), ("free_cost", "<i4"), ("n_tried", "<i4"),
                              ("n_used", "<i4"), ("best_member", "<i4")])
assert WORD_LINK_DTYPE.itemsize == 16 and WORD_TRACK_DTYPE.itemsize == 24 and TRACK_MATCH_DTYPE.itemsize == 32
# str_er_pool_match: the first seven fields of str_er_track_match for everything a slot of a track pool was given, and how many members that is
POOL_MATCH_DTYPE = np.dtype([("entry", "<i4"), ("cost", "<i4"), ("second_entry", "<i4"), ("second_cost", "<i4"), ("free_cost", "<i4"), ("n_tried", "<i4"),
                             ("n_used", "<i4"), ("n_members", "<i4")])
POOL_LATTICE = 1
assert POOL_MATCH_DTYPE.itemsize == 32
# str_er_pool_decode: the fields of TRACK_DECODE_DTYPE (seed_member: an age rank), then the members ever added and the members kept
POOL_DECODE_DTYPE = np.dtype([("cost", "<i4"), ("seed_cost", "<i4"), ("n_chars", "<i4"), ("n_edits", "<i4"), ("converged", "<i4"), ("n_used", "<i4"),
                              ("seed_member", "<i4"), ("lm_cost", "<i4"), ("n_members", "<i4"), ("n_kept", "<i4")])
POOL_DECODE = 2
assert POOL_DECODE_DTYPE.itemsize == 40
# str_er_word_decode: per word, the cost of the cheapest string (-1: more than 32 runs, not decoded) and of the plain reading, the
# characters of the string and the runs read, dropped and the characters inserted
WORD_DECODE_DTYPE = np.dtype([("cost", "<i4"), ("read_cost", "<i4"), ("n_chars", "<i4"), ("n_sub", "<i4"), ("n_del", "<i4"), ("n_ins", "<i4")])
LINE_DECODE_DTYPE = np.dtype([("cost", "<i4"), ("n_chars", "<i4"), ("n_breaks", "<i4"), ("n_sub", "<i4"), ("n_del", "<i4"), ("n_ins", "<i4")])
assert WORD_DECODE_DTYPE.itemsize == 24 and LINE_DECODE_DTYPE.itemsize == 24
# str_er_line_margin: per line, the smaller of its smallest row margin and its smallest gap margin; the smallest row margin, the
# line-relative row, its decoded reading and the alternative (65: the row dropped); the smallest gap margin, the line-relative row the
# gap lies in front of and its decided move (0 join, 1 break), all three -1 where no gap has an alternative; all -1: not decoded
LINE_MARGIN_DTYPE = np.dtype([("margin", "<i4"), ("read_margin", "<i4"), ("row", "<i4"), ("read", "<i4"), ("alt", "<i4"), ("gap_margin", "<i4"), ("gap", "<i4"),
                              ("gap_move", "<i4")])
assert LINE_MARGIN_DTYPE.itemsize == 32
# str_er_word_margin: per word, the extra cost of the cheapest path that reads some run differently from the decoded string, the
# word-relative row where it does, the decoded reading of that row and the alternative (65: the row dropped); all -1: not decoded
WORD_MARGIN_DTYPE = np.dtype([("margin", "<i4"), ("row", "<i4"), ("read", "<i4"), ("alt", "<i4")])
assert WORD_MARGIN_DTYPE.itemsize == 16
# str_er_word_match: per word, the best and the second-best lexicon entry with their costs (-1: none), the cost of the word's own
# reading and the number of entries tried
WORD_MATCH_DTYPE = np.dtype([("entry", "<i4"), ("cost", "<i4"), ("second_entry", "<i4"), ("second_cost", "<i4"), ("free_cost", "<i4"), ("n_tried", "<i4")])
assert WORD_MATCH_DTYPE.itemsize == 24
# str_er_run_read: per glyph run, the scorer's label, its character (str_er_ocr_char) and pv[label]
RUN_READ_DTYPE = np.dtype([("label", "<i4"), ("ch", "<i4"), ("prob", "<f8")])
assert RUN_READ_DTYPE.itemsize == 16
# str_er_run_split (ERFilter.feet_split / split_words, cuts_from_counts, split_words_host): per run its kept cut columns (frame columns,
# -1 unused), the valley threshold and its pieces in the piece table; per piece its run, nodes, box and pixels; per part of a split
# word (run, piece or -1 for the whole run); per word its parts in the part table, the cost of its split sequence and of its runs' own reading
RUN_SPLIT_DTYPE = np.dtype([("n_cuts", "<i4"), ("cut", "<i4", (3,)), ("thr", "<u4"), ("first_piece", "<i4"), ("n_pieces", "<i4"), ("n_parts", "<i4")])
RUN_PIECE_DTYPE = np.dtype([("run", "<i4"), ("from", "<i4"), ("to", "<i4"), ("x0", "<i4"), ("x1", "<i4"), ("y0", "<i4"), ("y1", "<i4"), ("pixels", "<u4")])
SPLIT_PART_DTYPE = np.dtype([("run", "<i4"), ("piece", "<i4")])
WORD_SPLIT_DTYPE = np.dtype([("first_part", "<i4"), ("n_parts", "<i4"), ("cost", "<i4"), ("read_cost", "<i4")])
assert RUN_SPLIT_DTYPE.itemsize == 32 and RUN_PIECE_DTYPE.itemsize == 32 and SPLIT_PART_DTYPE.itemsize == 8 and WORD_SPLIT_DTYPE.itemsize == 16
LATTICE_DECODE_DTYPE = np.dtype([("cost", "<i4"), ("read_cost", "<i4"), ("n_chars", "<i4"), ("n_sub", "<i4"), ("n_del", "<i4"), ("n_ins", "<i4"),
                                 ("first_part", "<i4"), ("n_parts", "<i4")])
assert LATTICE_DECODE_DTYPE.itemsize == 32
LINE_LATTICE_DECODE_DTYPE = np.dtype([("cost", "<i4"), ("n_chars", "<i4"), ("n_breaks", "<i4"), ("n_sub", "<i4"), ("n_del", "<i4"), ("n_ins", "<i4"),
                                      ("first_part", "<i4"), ("n_parts", "<i4")])
assert LINE_LATTICE_DECODE_DTYPE.itemsize == 32
# str_er_lattice_margin: per word, the smallest reading margin of its lattice parts with the part, its decoded reading and the
# alternative (65: the part dropped); the smallest cut margin with the part and the other edge (i | j << 4) -- all three -1 where no
# run of the word is cut; the edges of the lattice.  All -1 (n_edges 0): not decoded or no runs
LATTICE_MARGIN_DTYPE = np.dtype([("read_margin", "<i4"), ("read_part", "<i4"), ("read", "<i4"), ("alt", "<i4"), ("cut_margin", "<i4"), ("cut_part", "<i4"),
                                 ("cut_alt", "<i4"), ("n_edges", "<i4")])
assert LATTICE_MARGIN_DTYPE.itemsize == 32
LATTICE_MATCH_DTYPE = np.dtype([("entry", "<i4"), ("cost", "<i4"), ("second_entry", "<i4"), ("second_cost", "<i4"), ("free_cost", "<i4"), ("n_tried", "<i4"),
                                ("first_part", "<i4"), ("n_parts", "<i4"), ("n_del", "<i4"), ("n_ins", "<i4")])
assert LATTICE_MATCH_DTYPE.itemsize == 40
# str_er_line_run: frame columns [x0, x1) and rows [y0, y1), half open; word: its row of the word table
LINE_RUN_DTYPE = np.dtype([("x0", "<i4"), ("x1", "<i4"), ("y0", "<i4"), ("y1", "<i4"), ("pixels", "<u4"), ("word", "<i4")])
# str_er_line_word: the runs line_runs[first_run:first_run + n_runs] of line `line`, their bounding box and pixels
LINE_WORD_DTYPE = np.dtype([("line", "<i4"), ("first_run", "<i4"), ("n_runs", "<i4"), ("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"), ("pixels", "<u4")])
# str_er_line_words: per line, its rows of the word and run tables and the largest column count of its footprint
LINE_WORDS_DTYPE = np.dtype([("first_word", "<i4"), ("n_words", "<i4"), ("first_run", "<i4"), ("n_runs", "<i4"), ("colmax", "<u4"), ("reserved", "<u4")])
# str_er_line_crop: crop t = width x height bytes (pitch width) from byte pix_off of the crop bytes (and of the glyph bytes);
# ax .. vy: the 16.16 sampling geometry (include/str_er.h)
LINE_CROP_DTYPE = np.dtype([("pix_off", "<u8"), ("width", "<i4"), ("height", "<i4"), ("ax", "<i4"), ("ay", "<i4"),
                            ("ux", "<i4"), ("uy", "<i4"), ("vx", "<i4"), ("vy", "<i4")])
TEXT_DTYPE = np.dtype([("frame", "<u4"), ("pyr", "u1"), ("r0", "u1"), ("r1", "u1"), ("r2", "u1"), ("first", "<i4"), ("count", "<i4"),
                       ("slope", "<f8"), ("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4")])
GBOUND_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"), ("cx", "<i4"), ("cy", "<i4")])
TRACK_DTYPE = np.dtype([("color1", "<f8"), ("color2", "<f8"), ("color3", "<f8"), ("cx", "<i4"), ("cy", "<i4"),
                        ("tracked", "<u4"), ("reserved", "<u4")])
CLS_POOL, CLS_STRONG, CLS_WEAK = 0, 1, 2
MEM_HOST, MEM_DEVICE = 0, 1

NODE_DTYPE = np.dtype([("key", "<u4"), ("parent", "<i4"), ("area", "<i4"), ("x", "<u2"), ("y", "<u2"),
                       ("w", "<u2"), ("h", "<u2"), ("level", "u1"), ("flags", "u1"), ("reserved", "<u2")])
CAND_DTYPE = np.dtype([("frame", "<u4"), ("ch", "u1"), ("pyr", "u1"), ("level", "u1"), ("cls", "u1"),
                       ("x", "<u2"), ("y", "<u2"), ("w", "<u2"), ("h", "<u2"), ("area", "<u4"), ("key", "<u4"),
                       ("node", "<i4"), ("plane", "<u4"), ("score_strong", "<f8"), ("score_weak", "<f8")])
PLANE_DTYPE = np.dtype([("frame", "<u4"), ("ch", "u1"), ("pyr", "u1"), ("r0", "u1"), ("r1", "u1"), ("width", "<i4"),
                        ("height", "<i4"), ("n_created", "<i4"), ("n_kept", "<i4"), ("n_pool", "<i4"), ("n_strong", "<i4"),
                        ("n_weak", "<i4"), ("ambiguous", "<i4"), ("root", "<i4")])
assert NODE_DTYPE.itemsize == 24 and CAND_DTYPE.itemsize == 48 and PLANE_DTYPE.itemsize == 44 and MASK_DTYPE.itemsize == 16
assert LINE_CROP_DTYPE.itemsize == 40
assert SHAPE_DTYPE.itemsize == 48
assert STROKE_DTYPE.itemsize == 32
assert FRAME_MAP_DTYPE.itemsize == 16
assert LINE_FOOT_DTYPE.itemsize == 24 and LINE_PAIR_DTYPE.itemsize == 16 and FRAME_LINE_DTYPE.itemsize == 40
assert LINE_LINK_DTYPE.itemsize == 16 and TEXT_TRACK_DTYPE.itemsize == 24
assert LINE_GEOM_DTYPE.itemsize == 168
assert LINE_RUN_DTYPE.itemsize == 24 and LINE_WORD_DTYPE.itemsize == 32 and LINE_WORDS_DTYPE.itemsize == 24


def unpack_mask(words: np.ndarray, word_off: int, w: int, h: int) -> np.ndarray:
    """One mask of a str_er_mask word array as a bool array (h, w): pixel x of a row is bit x & 31 of word x >> 5."""
    pitch = (w + 31) // 32
    rows = np.ascontiguousarray(words[word_off:word_off + pitch * h], dtype="<u4").reshape(h, pitch)
    return np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little")[:, :w].astype(bool)


class ImageRef(C.Structure):
    """str_er_image_ref: one frame / plane of a list call (top-left pixel, size, bytes per row)."""
    _fields_ = [("data", C.c_void_p), ("w", C.c_int32), ("h", C.c_int32), ("stride", C.c_int64)]


assert C.sizeof(ImageRef) == 24 and (ImageRef.data.offset, ImageRef.w.offset, ImageRef.h.offset, ImageRef.stride.offset) == (0, 8, 12, 16)


def _row_view(a, bpp: int) -> np.ndarray:
    """`a` as uint8 rows of bpp-byte pixels, contiguous within a row; a view with a row stride is kept as it is (no copy)."""
    a = np.asarray(a)
    if a.dtype != np.uint8:
        a = a.astype(np.uint8)
    if a.ndim != (3 if bpp == 3 else 2) or (bpp == 3 and a.shape[2] != 3):
        raise ValueError("expected (H,W,3) uint8 BGR frames" if bpp == 3 else "expected (H,W) uint8 planes")
    if a.strides[-1] != 1 or (bpp == 3 and a.strides[1] != 3) or a.strides[0] < bpp * a.shape[1]:
        a = np.ascontiguousarray(a)
    return a


class StrErError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"str_er error {code}: {msg}")
        self.code = code


class _Params(C.Structure):
    _fields_ = [("thresh_step", C.c_int32), ("min_area", C.c_int32), ("max_area", C.c_int32),
                ("stability_t", C.c_int32), ("overlap_coef", C.c_double), ("n_pyr_levels", C.c_int32),
                ("channel_mask", C.c_uint32), ("device", C.c_int32), ("max_width", C.c_int32),
                ("max_height", C.c_int32), ("max_frames", C.c_int32), ("kept_cap", C.c_int32),
                ("pool_cap", C.c_int32), ("sibling_order", C.c_int32), ("stream", C.c_void_p)]


class _PlaneInfo(C.Structure):
    _fields_ = [("frame", C.c_uint32), ("ch", C.c_uint8), ("pyr", C.c_uint8), ("r0", C.c_uint8), ("r1", C.c_uint8),
                ("width", C.c_int32), ("height", C.c_int32), ("n_created", C.c_int32), ("n_kept", C.c_int32),
                ("n_pool", C.c_int32), ("n_strong", C.c_int32), ("n_weak", C.c_int32), ("ambiguous", C.c_int32),
                ("root", C.c_int32)]


@dataclass
class Params:
    """Constructor arguments of ERFilter (inc/ER.h:113; src/main.cpp:22) + capacity."""
    thresh_step: int = 8
    min_area: int = 120
    max_area: int = 900000
    stability_t: int = 2
    overlap_coef: float = 0.7
    n_pyr_levels: int = 1
    channel_mask: int = 0x3F
    device: int = 0
    max_width: int = 1920
    max_height: int = 1080
    max_frames: int = 8
    kept_cap: int = 0
    pool_cap: int = 0
    sibling_order: int = 0
    stream: Optional[int] = None


_LIB = None


def lib_path() -> str:
    # STR_ER_LIB: developer switch, load another build of the same library (tools/dev_stop_all.sh)
    return os.environ.get("STR_ER_LIB") or os.path.join(HERE, "lib", "libstr_er_hip.so")


def load_library():
    """Load libstr_er_hip.so; raises if it has not been built (no fallback exists)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} is missing: run `python scene-text-recognition_amd/build.py` (hipcc, gfx950). "
            "There is no CPU implementation of this path.")
    L = C.CDLL(path)
    u8p, i32p, f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    vp = C.c_void_p
    L.str_er_abi_version.restype = C.c_int
    L.str_er_default_params.argtypes = [C.POINTER(_Params)]
    L.str_er_create.argtypes = [C.POINTER(_Params), C.POINTER(vp)]
    L.str_er_destroy.argtypes = [vp]
    L.str_er_last_error.argtypes = [vp]
    L.str_er_last_error.restype = C.c_char_p
    L.str_er_strerror.argtypes = [C.c_int]
    L.str_er_strerror.restype = C.c_char_p
    L.str_er_set_thresh_step.argtypes = [vp, C.c_int32]
    L.str_er_set_min_area.argtypes = [vp, C.c_int32]
    L.str_er_load_cascade.argtypes = [vp, C.c_int, C.c_char_p]
    L.str_er_load_cascade_mem.argtypes = [vp, C.c_int, C.c_char_p, C.c_size_t]
    L.str_er_cascade_info.argtypes = [vp, C.c_int, i32p, i32p]
    L.str_er_detect_bgr.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int,
                                    C.c_uint32, C.POINTER(vp)]
    L.str_er_detect_bgr_planes.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int,
                                           C.c_uint32, vp, C.c_int32, C.POINTER(vp)]
    L.str_er_strip_extract.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, C.c_int, C.c_int32, C.c_int32, C.POINTER(vp), C.POINTER(C.c_int64)]
    L.str_er_strip_free.argtypes = [vp]
    L.str_er_strip_free.restype = None
    L.str_er_strip_merge.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, C.c_int, vp, vp, C.c_int32, C.c_uint32, C.POINTER(vp)]
    L.str_er_strip_extract_dev.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, C.c_int, C.c_int32, C.c_int32, C.POINTER(vp), C.POINTER(C.c_int64)]
    L.str_er_strip_merge_ex.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, C.c_int, vp, vp, C.c_int, C.c_int32, vp, C.c_uint32, C.POINTER(vp)]
    L.str_er_comm_allgather_bytes.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.str_er_comm_free.argtypes = [vp]
    L.str_er_comm_free.restype = None
    L.str_er_detect_planes.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int,
                                       C.c_uint32, C.POINTER(vp)]
    L.str_er_detect_bgr_list.argtypes = [vp, vp, C.c_int32, C.c_int, C.c_uint32, C.POINTER(vp)]
    L.str_er_detect_planes_list.argtypes = [vp, vp, C.c_int32, C.c_int, C.c_uint32, C.POINTER(vp)]
    L.str_er_detect_nv12_list.argtypes = [vp, vp, C.c_int32, C.c_int, C.c_uint32, C.POINTER(vp)]
    L.str_er_compute_channels.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, vp]
    L.str_er_classify_boxes.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, vp, C.c_int32, vp, vp, vp]
    L.str_er_lbp_hist.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, vp, C.c_int32, vp, vp]
    L.str_er_calc_lbp.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, vp, C.c_int32, vp]
    L.str_er_cascade_predict.argtypes = [vp, C.c_int, vp, C.c_int32, vp]
    L.str_er_load_svm_model.argtypes = [vp, C.c_char_p, C.c_int32]
    L.str_er_load_svm_model_mem.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int32]
    L.str_er_svm_info.argtypes = [vp, i32p, i32p, i32p]
    L.str_er_svm_forms.argtypes = [vp, i32p, i32p]
    L.str_er_svm_predict_probability.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp, vp]
    L.str_er_svm_predict_probability_q8.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp, vp]
    L.str_er_ocr_chain_run.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, vp, C.c_int32, vp, vp, vp]
    L.str_er_ocr_chain_run_slope.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, vp, vp, C.c_int32, vp, vp, vp]
    L.str_er_nms_tree.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, i32p, i32p]
    L.str_er_nms_tree_plane.argtypes = [vp, vp, C.c_int32, vp, C.c_int32, C.c_int32, C.c_int64, vp, C.c_int32, i32p, i32p]
    L.str_er_flood_order.argtypes = [vp, C.c_int32, C.c_int32, C.c_int64, C.c_int32, vp]
    L.str_er_comm_unique_id.argtypes = [vp]
    L.str_er_comm_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp, C.POINTER(vp)]
    L.str_er_comm_local_group.argtypes = [C.c_int32, C.POINTER(vp)]
    L.str_er_comm_create_local.argtypes = [vp, C.c_int32, C.POINTER(vp)]
    L.str_er_comm_local_group_free.argtypes = [vp]
    L.str_er_comm_local_group_free.restype = None
    L.str_er_comm_destroy.argtypes = [vp]
    L.str_er_comm_destroy.restype = None
    L.str_er_comm_last_error.argtypes = [vp]
    L.str_er_comm_last_error.restype = C.c_char_p
    L.str_er_gather_cands.argtypes = [vp, vp, C.c_int32, C.c_uint32, C.POINTER(vp), i32p, i32p]
    L.str_er_gather_last.argtypes = [vp, vp, C.c_uint32, C.POINTER(vp), i32p, i32p]
    L.str_er_gather_free.argtypes = [vp]
    L.str_er_gather_free.restype = None
    L.str_er_resize_plane.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, vp, C.c_int32, C.c_int32]
    L.str_er_result_n_planes.argtypes = [vp]
    L.str_er_result_n_planes.restype = C.c_int32
    L.str_er_result_plane_info.argtypes = [vp, C.c_int32, C.POINTER(_PlaneInfo)]
    L.str_er_result_plane_infos.argtypes = [vp, i32p]
    L.str_er_result_plane_infos.restype = vp
    L.str_er_result_cands.argtypes = [vp, i32p]
    L.str_er_result_cands.restype = vp
    L.str_er_result_plane_cands.argtypes = [vp, C.c_int32, i32p]
    L.str_er_result_plane_cands.restype = vp
    L.str_er_result_plane_nodes.argtypes = [vp, C.c_int32, i32p]
    L.str_er_result_plane_nodes.restype = vp
    L.str_er_result_tracks.argtypes = [vp, i32p]
    L.str_er_result_tracks.restype = vp
    L.str_er_result_masks.argtypes = [vp, i32p]
    L.str_er_result_masks.restype = vp
    L.str_er_result_mask_bits.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.str_er_result_mask_bits.restype = vp
    L.str_er_er_masks.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, vp, C.c_int32, vp, C.c_uint64, C.POINTER(C.c_uint64), vp]
    L.str_er_result_shapes.argtypes = [vp, i32p]
    L.str_er_result_shapes.restype = vp
    L.str_er_er_shapes.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, vp, C.c_int32, vp]
    L.str_er_result_strokes.argtypes = [vp, i32p]
    L.str_er_result_strokes.restype = vp
    L.str_er_er_strokes.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, vp, C.c_int32, vp]
    L.str_er_set_min_ocr_prob.argtypes = [vp, C.c_double]
    L.str_er_result_line_crops.argtypes = [vp, i32p]
    L.str_er_result_line_crops.restype = vp
    for fn in (L.str_er_result_line_crop_pixels, L.str_er_result_line_glyph_pixels):
        fn.argtypes = [vp, C.POINTER(C.c_uint64)]
        fn.restype = vp
    L.str_er_set_line_crop.argtypes = [vp, C.c_int32, C.c_int32, C.c_double]
    L.str_er_result_frame_maps.argtypes = [vp, i32p]
    L.str_er_result_frame_maps.restype = vp
    for fn in (L.str_er_result_text_map_pixels, L.str_er_result_line_map_ids):
        fn.argtypes = [vp, C.POINTER(C.c_uint64)]
        fn.restype = vp
    L.str_er_text_map_regions.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, vp, vp]
    for fn in (L.str_er_result_line_feet, L.str_er_result_line_pairs, L.str_er_result_frame_lines, L.str_er_result_frame_line_members):
        fn.argtypes = [vp, i32p]
        fn.restype = vp
    L.str_er_set_frame_merge.argtypes = [vp, C.c_int32, C.c_int32]
    L.str_er_line_feet_regions.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp,
                                           C.c_uint64, C.POINTER(C.c_uint64), vp, C.c_int32, i32p]
    L.str_er_frame_lines_from_pairs.argtypes = [vp, vp, vp, C.c_int32, vp, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, i32p, vp]
    for fn in (L.str_er_result_line_links, L.str_er_result_line_tracks, L.str_er_result_text_tracks, L.str_er_result_text_track_members):
        fn.argtypes = [vp, i32p]
        fn.restype = vp
    L.str_er_result_edge_feet.argtypes = [vp, C.c_int32, i32p, i32p, C.POINTER(vp), C.POINTER(vp), i32p, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.str_er_set_line_link.argtypes = [vp, C.c_int32, C.c_int32]
    L.str_er_link_feet.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int32, vp, C.c_int32, i32p]
    L.str_er_text_tracks_from_links.argtypes = [vp, vp, C.c_int32, vp, C.c_int32, vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, C.c_int32, i32p, vp]
    for fn in (L.str_er_result_line_geoms, L.str_er_result_frame_line_geoms, L.str_er_result_geom_points):
        fn.argtypes = [vp, i32p]
        fn.restype = vp
    L.str_er_feet_geom.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int32, i32p]
    L.str_er_hull_of_points.argtypes = [vp, C.c_int32, vp, C.c_int32, i32p]
    L.str_er_quad_from_hull.argtypes = [vp, C.c_int32, vp]
    for fn in (L.str_er_result_line_words, L.str_er_result_line_runs, L.str_er_result_words):
        fn.argtypes = [vp, i32p]
        fn.restype = vp
    L.str_er_set_word_gap.argtypes = [vp, C.c_int32, C.c_int32]
    L.str_er_feet_words.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int32, i32p, vp, C.c_int32, i32p]
    L.str_er_words_from_runs.argtypes = [vp, C.c_int32, vp, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, i32p]
    L.str_er_result_run_reads.argtypes = [vp, i32p]
    L.str_er_result_run_reads.restype = vp
    L.str_er_result_run_features.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.str_er_result_run_features.restype = vp
    L.str_er_set_lexicon.argtypes = [vp, vp, vp, C.c_int32, C.c_uint32]
    L.str_er_lexicon_info.argtypes = [vp, i32p, C.POINTER(C.c_uint32), i32p, C.POINTER(C.c_uint64)]
    L.str_er_set_word_match.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32]
    L.str_er_cost_thresholds.argtypes = [vp]
    L.str_er_cost_thresholds.restype = None
    L.str_er_prob_costs.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_int32, vp]
    L.str_er_run_costs.argtypes = [vp, vp, C.c_int32, vp]
    L.str_er_match_words.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int32, vp]
    L.str_er_match_words_host.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, vp]
    L.str_er_result_word_matches.argtypes = [vp, i32p]
    L.str_er_result_word_matches.restype = vp
    L.str_er_set_word_link.argtypes = [vp, C.c_int32, C.c_int32]
    L.str_er_word_links.argtypes = [vp, vp, vp, C.c_int32, vp, C.c_int32, vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, C.c_int32, i32p]
    L.str_er_word_tracks_from_links.argtypes = [vp, vp, vp, C.c_int32, vp, C.c_int32, vp, C.c_int32, vp, vp, C.c_int32, i32p, vp]
    L.str_er_match_tracks.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, vp, vp]
    L.str_er_match_tracks_host.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, vp, vp, C.c_int32, C.c_uint32, C.c_int32,
                                           C.c_int32, C.c_int32, vp, vp]
    for fn in (L.str_er_result_word_links, L.str_er_result_word_tracks, L.str_er_result_word_track_members, L.str_er_result_word_track_of_words,
               L.str_er_result_track_matches, L.str_er_result_track_member_costs):
        fn.argtypes = [vp, i32p]
        fn.restype = vp
    L.str_er_set_track_decode.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32]
    L.str_er_decode_tracks.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, vp, vp, vp]
    L.str_er_decode_tracks_host.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_int32, vp, vp, vp]
    for name, cnt in (("track_decodes", i32p), ("track_decode_chars", C.POINTER(C.c_uint64)), ("track_decode_member_costs", i32p)):
        fn = getattr(L, "str_er_result_" + name)
        fn.argtypes, fn.restype = [vp, cnt], vp
    L.str_er_result_run_costs.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.str_er_result_run_costs.restype = vp
    L.str_er_result_run_probs.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.str_er_result_run_probs.restype = vp
    L.str_er_set_bigram.argtypes = [vp, vp]
    L.str_er_bigram_info.argtypes = [vp, i32p, C.POINTER(C.c_uint64)]
    L.str_er_set_word_decode.argtypes = [vp, C.c_int32, C.c_int32]
    L.str_er_bigram_from_probs.argtypes = [vp, vp, vp, vp]
    L.str_er_decode_words.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp]
    L.str_er_decode_words_host.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, C.c_int32, C.c_int32, vp, vp, vp]
    L.str_er_result_word_decodes.argtypes = [vp, i32p]
    L.str_er_result_word_decodes.restype = vp
    L.str_er_result_word_decode_chars.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.str_er_result_word_decode_chars.restype = vp
    L.str_er_result_word_decode_src.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.str_er_result_word_decode_src.restype = vp
    L.str_er_set_line_decode.argtypes = [vp, C.c_int32, C.c_int32]
    L.str_er_line_gap_costs.argtypes = [vp, C.c_int32, vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp]
    L.str_er_decode_lines.argtypes = [vp, vp, C.c_int32, vp, vp, vp, C.c_int32, vp, vp, vp, vp]
    L.str_er_decode_lines_host.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int32, vp, C.c_int32, C.c_int32, vp, vp, vp, vp]
    L.str_er_line_decode_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.str_er_result_line_decodes.argtypes = [vp, i32p]
    L.str_er_result_line_decodes.restype = vp
    for fn in (L.str_er_result_line_decode_chars, L.str_er_result_line_decode_src, L.str_er_result_line_decode_word_of_row, L.str_er_result_line_gap_costs,
               L.str_er_result_line_decode_windows):
        fn.argtypes = [vp, C.POINTER(C.c_uint64)]
        fn.restype = vp
    L.str_er_set_line_margin.argtypes = [vp, C.c_int32]
    L.str_er_line_margins.argtypes = [vp, vp, C.c_int32, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp]
    L.str_er_line_margins_host.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int32, vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, vp]
    L.str_er_line_margin_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.str_er_result_line_margins.argtypes = [vp, i32p]
    L.str_er_result_line_margins.restype = vp
    for fn in (L.str_er_result_line_row_margins, L.str_er_result_line_row_reads, L.str_er_result_line_row_alts, L.str_er_result_line_gap_margins,
               L.str_er_result_line_gap_moves):
        fn.argtypes = [vp, C.POINTER(C.c_uint64)]
        fn.restype = vp
    L.str_er_set_word_margin.argtypes = [vp, C.c_int32]
    L.str_er_word_margins.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, vp, vp]
    L.str_er_word_margins_host.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp]
    L.str_er_result_word_margins.argtypes = [vp, i32p]
    L.str_er_result_word_margins.restype = vp
    for fn in (L.str_er_result_word_row_margins, L.str_er_result_word_row_reads, L.str_er_result_word_row_alts):
        fn.argtypes = [vp, C.POINTER(C.c_uint64)]
        fn.restype = vp
    L.str_er_ocr_char.argtypes = [C.c_int32]
    L.str_er_ocr_char.restype = C.c_int32
    for name, cnt in (("run_splits", i32p), ("run_pieces", i32p), ("piece_reads", i32p), ("piece_costs", C.POINTER(C.c_uint64)), ("split_parts", i32p),
                      ("word_splits", i32p)):
        fn = getattr(L, "str_er_result_" + name)
        fn.argtypes, fn.restype = [vp, cnt], vp
    L.str_er_run_split_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    for name, cnt in (("lattice_decodes", i32p), ("lattice_decode_chars", C.POINTER(C.c_uint64)), ("lattice_decode_src", C.POINTER(C.c_uint64)), ("lattice_parts", i32p)):
        fn = getattr(L, "str_er_result_" + name)
        fn.argtypes, fn.restype = [vp, cnt], vp
    L.str_er_lattice_decode_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.str_er_set_lattice_margin.argtypes = [vp, C.c_int32]
    L.str_er_lattice_margins.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.str_er_lattice_margins_host.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int32, C.c_int32, vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.str_er_result_lattice_margins.argtypes = [vp, i32p]
    L.str_er_result_lattice_margins.restype = vp
    for fn in (L.str_er_result_lattice_read_margins, L.str_er_result_lattice_cut_margins, L.str_er_result_lattice_part_reads, L.str_er_result_lattice_part_alts,
               L.str_er_result_lattice_cut_alts):
        fn.argtypes = [vp, C.POINTER(C.c_uint64)]
        fn.restype = vp
    for name, cnt in (("lattice_matches", i32p), ("lattice_match_src", C.POINTER(C.c_uint64)), ("lattice_match_parts", i32p)):
        fn = getattr(L, "str_er_result_" + name)
        fn.argtypes, fn.restype = [vp, cnt], vp
    L.str_er_lattice_match_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    for name, cnt in (("lattice_track_matches", i32p), ("lattice_track_members", i32p), ("lattice_track_src", C.POINTER(C.c_uint64)), ("lattice_track_parts", i32p)):
        fn = getattr(L, "str_er_result_" + name)
        fn.argtypes, fn.restype = [vp, cnt], vp
    L.str_er_lattice_track_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.str_er_lattice_match_tracks.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_int32, i32p]
    L.str_er_lattice_match_tracks_host.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, vp, vp, C.c_int32, C.c_uint32,
                                                   C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_int32, i32p]
    for name, cnt in (("lattice_track_decodes", i32p), ("lattice_track_decode_chars", C.POINTER(C.c_uint64)), ("lattice_track_decode_members", i32p),
                      ("lattice_track_decode_src", C.POINTER(C.c_uint64)), ("lattice_track_decode_parts", i32p)):
        fn = getattr(L, "str_er_result_" + name)
        fn.argtypes, fn.restype = [vp, cnt], vp
    L.str_er_set_lattice_track_decode.argtypes = [vp, C.c_int32]
    L.str_er_lattice_track_decode_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.str_er_lattice_decode_tracks.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, C.c_int32, i32p]
    L.str_er_lattice_decode_tracks_host.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, vp, C.c_int32, C.c_int32,
                                                    C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, C.c_int32, i32p]
    L.str_er_track_pool_create.argtypes = [vp, C.c_int32, C.c_uint32, C.POINTER(vp)]
    L.str_er_track_pool_destroy.argtypes, L.str_er_track_pool_destroy.restype = [vp], None
    L.str_er_track_pool_reset.argtypes = [vp]
    L.str_er_track_pool_info.argtypes = [vp, i32p, C.POINTER(C.c_uint32), i32p, C.POINTER(C.c_uint64), i32p, i32p]
    L.str_er_track_pool_add.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, vp]
    L.str_er_track_pool_add_lattice.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, vp]
    L.str_er_track_pool_join.argtypes = [vp, C.c_int32, vp, C.c_int32]
    L.str_er_track_pool_clear.argtypes = [vp, vp, C.c_int32]
    L.str_er_track_pool_read.argtypes = [vp, vp, C.c_int32, vp]
    L.str_er_track_pool_create_decode.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.str_er_track_pool_keep.argtypes = [vp, i32p]
    L.str_er_track_pool_read_decode.argtypes = [vp, vp, C.c_int32, vp, vp, vp]
    L.str_er_track_pool_members.argtypes = [vp, C.c_int32, vp, vp, vp, i32p]
    L.str_er_track_pool_create_lattice_decode.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.str_er_track_pool_read_lattice_decode.argtypes = [vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp, C.c_int32, i32p]
    L.str_er_track_pool_lattice_members.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, i32p]
    L.str_er_lattice_match_words.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, C.c_int32, i32p]
    L.str_er_lattice_match_words_host.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32,
                                                  C.c_int32, vp, vp, vp, C.c_int32, i32p]
    L.str_er_lattice_decode_words.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, vp, C.c_int32, i32p]
    L.str_er_lattice_decode_lines.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, C.c_int32, vp, vp, vp, vp, C.c_int32, i32p, vp]
    L.str_er_lattice_decode_lines_host.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, vp, C.c_int32, C.c_int32, vp, vp, vp, vp,
                                                   C.c_int32, i32p, vp]
    L.str_er_line_lattice_decode_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.str_er_set_line_lattice_decode.argtypes = [vp, C.c_int32, C.c_int32]
    for fn in (L.str_er_result_line_lattice_decodes, L.str_er_result_line_lattice_parts):
        fn.argtypes = [vp, i32p]
        fn.restype = vp
    for fn in (L.str_er_result_line_lattice_chars, L.str_er_result_line_lattice_src, L.str_er_result_line_lattice_word_of_part, L.str_er_result_line_lattice_gap_costs,
               L.str_er_result_line_lattice_windows):
        fn.argtypes = [vp, C.POINTER(C.c_uint64)]
        fn.restype = vp
    L.str_er_lattice_decode_words_host.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int32, C.c_int32, vp, C.c_int32, C.c_int32, vp, vp, vp, vp,
                                                   C.c_int32, i32p]
    L.str_er_set_run_split.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32]
    L.str_er_cuts_from_counts.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, i32p, C.POINTER(C.c_uint32)]
    L.str_er_feet_split.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, C.c_int32, vp, vp, C.c_int32, i32p, vp, C.c_int32, i32p, vp, vp,
                                    vp, vp, C.c_int32, i32p, vp, vp]
    L.str_er_split_words.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int32, i32p, vp]
    L.str_er_split_words_host.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int32, C.c_int32, vp, vp, C.c_int32, i32p, vp]
    L.str_er_feet_read.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, C.c_int32, vp, vp, C.c_int32, i32p, vp, C.c_int32, i32p, vp, vp]
    L.str_er_run_atlas_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.str_er_line_crop_geometry.argtypes = [vp, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_double, vp]
    L.str_er_line_crops.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, vp, vp, vp, vp, C.c_int32, vp, C.c_uint64,
                                    C.POINTER(C.c_uint64), vp]
    for fn in (L.str_er_result_texts, L.str_er_result_text_ers, L.str_er_result_group_bounds, L.str_er_result_group_all,
               L.str_er_result_line_labels, L.str_er_result_line_probs, L.str_er_result_line_kept, L.str_er_result_text_alive):
        fn.argtypes = [vp, i32p]
        fn.restype = vp
    L.str_er_er_grouping.argtypes = [vp, vp, vp, C.c_int32, C.c_int, C.c_int, C.POINTER(vp)]
    L.str_er_stream_create.argtypes = [vp, C.c_int32, C.POINTER(vp)]
    L.str_er_stream_destroy.argtypes = [vp]
    L.str_er_stream_destroy.restype = None
    L.str_er_stream_depth.argtypes = [vp]
    L.str_er_stream_context.argtypes = [vp, C.c_int32]
    L.str_er_stream_context.restype = vp
    L.str_er_stream_last_error.argtypes = [vp]
    L.str_er_stream_last_error.restype = C.c_char_p
    L.str_er_stream_load_cascade.argtypes = [vp, C.c_int, C.c_char_p]
    L.str_er_stream_acquire.argtypes = [vp, i32p, C.POINTER(vp), C.POINTER(C.c_int64)]
    L.str_er_stream_submit.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.str_er_stream_submit_nv12.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.str_er_detect_nv12.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int, C.c_uint32, C.POINTER(vp)]
    L.str_er_stream_submit_copy.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.str_er_stream_submit_list.argtypes = [vp, C.c_int32, vp, C.c_int32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.str_er_stream_submit_nv12_list.argtypes = [vp, C.c_int32, vp, C.c_int32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.str_er_stream_submit_copy_list.argtypes = [vp, vp, C.c_int32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.str_er_stream_next.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.str_er_stream_pending.argtypes = [vp]
    L.str_er_calc_color.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, vp, C.c_int32, C.c_int32, C.c_int64, vp, C.c_int32, vp]
    L.str_er_er_track.argtypes = [vp, vp, vp, C.c_int32, vp, vp, vp]
    L.str_er_result_ocr_labels.argtypes = [vp, i32p]
    L.str_er_result_ocr_labels.restype = vp
    L.str_er_result_ocr_probs.argtypes = [vp, i32p]
    L.str_er_result_ocr_probs.restype = vp
    L.str_er_result_times.argtypes = [vp]
    L.str_er_result_times.restype = f64p
    L.str_er_result_cands_to_device.argtypes = [vp, vp, vp, C.c_int32, i32p]
    L.str_er_result_free.argtypes = [vp]
    L.str_er_last_tree_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.str_er_tile2_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.str_er_last_group_stats.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.str_er_ocr_stage_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.str_er_last_profile.argtypes = [vp, C.POINTER(C.c_char_p), f64p, C.c_int32]
    L.str_er_set_profiling.argtypes = [vp, C.c_int]
    L.str_er_workspace_bytes.argtypes = [vp]
    L.str_er_workspace_bytes.restype = C.c_int64
    L.str_er_runtime_hint.restype = C.c_char_p
    L.str_er_tie_stats.argtypes = [vp, C.POINTER(C.c_uint64), f64p, i32p]
    if L.str_er_abi_version() != 2:
        raise RuntimeError("libstr_er_hip.so ABI version mismatch")
    _LIB = L
    return L


def set_batch_slots(n: int) -> int:
    """At most n detect calls of the process have their batch's kernels on the GPU at a time (0: no limit); include/str_er.h."""
    return int(load_library().str_er_set_batch_slots(int(n)))


def apply_runtime_hint() -> int:
    """Opt in to the HIP runtime settings the library recommends (str_er_runtime_hint(): more hardware queues).  Only
    effective before the process's first HIP call (e.g. before torch.cuda is initialised); importing the package does
    not touch the environment."""
    return int(load_library().str_er_apply_runtime_hint())


@dataclass
class PlaneResult:
    frame: int
    ch: int
    pyr: int
    width: int
    height: int
    n_created: int
    n_kept: int
    n_pool: int
    n_strong: int
    n_weak: int
    ambiguous: int
    root: int
    cands: np.ndarray                      # CAND_DTYPE, ascending key
    nodes: Optional[np.ndarray] = None     # NODE_DTYPE, ascending (key, level)

    @property
    def pool(self) -> np.ndarray:
        return self.cands

    @property
    def strong(self) -> np.ndarray:
        return self.cands[self.cands["cls"] == CLS_STRONG]

    @property
    def weak(self) -> np.ndarray:
        return self.cands[self.cands["cls"] == CLS_WEAK]


class Result:
    """Outcome of one detect call.  `info` (PLANE_DTYPE) and `cands` (CAND_DTYPE) are flat arrays;
    `planes` builds one PlaneResult per plane on first use."""

    def __init__(self, info: np.ndarray, cands: np.ndarray, times: np.ndarray, profile: dict, nodes=None):
        self.info, self.cands, self.times, self.profile, self._nodes = info, cands, times, profile, nodes
        self.ocr_label = None      # with STAGE_OCR: per candidate, -1 for cls == 0
        self.ocr_prob = None
        self.tracks = None         # with STAGE_TRACK: TRACK_DTYPE per candidate (zeros for cls == 0)
        self.texts = None          # with STAGE_GROUP: TEXT_DTYPE per line; members = text_ers[first:first+count] (candidate indices)
        self.text_ers = None
        self.group_bounds = None   # GBOUND_DTYPE per candidate: bound / center as er_grouping leaves them
        self.group_all = None      # all_er after er_grouping's sort / inner_suppression (candidate indices, images concatenated)
        self.line_label = None     # with STAGE_OCR_LINES: per entry of text_ers, chain_run's label / prob with the line's slope,
        self.line_prob = None      # whether the member survives er_ocr's two deletions, and per line whether >= 2 members do
        self.line_kept = None
        self.text_alive = None
        self.masks = None          # with WANT_MASKS: MASK_DTYPE per candidate, and the words they index (uint32)
        self.mask_bits = None
        self.shapes = None         # with WANT_SHAPES: SHAPE_DTYPE per candidate
        self.strokes = None        # with WANT_STROKES: STROKE_DTYPE per candidate
        self.line_crops = None     # with WANT_LINE_CROPS: LINE_CROP_DTYPE per line of texts, the grey crop bytes and (WANT_LINE_GLYPHS) the glyph bytes
        self.line_crop_pixels = None
        self.line_glyph_pixels = None
        self.frame_maps = None     # with WANT_TEXT_MAP / WANT_LINE_MAP: FRAME_MAP_DTYPE per frame, and the maps they index (uint8 / int32)
        self.text_map_pixels = None
        self.line_map_ids = None
        self._line_feet = None     # with WANT_FRAME_LINES: the tables behind line_feet / line_pairs / frame_lines / frame_line_members
        self._line_pairs = None
        self._frame_lines = None
        self._frame_line_members = None
        self._line_links = None    # with WANT_LINE_LINKS: the tables behind line_links / line_tracks / text_tracks / text_track_members / edge_feet
        self._line_tracks = None
        self._text_tracks = None
        self._text_track_members = None
        self._edge_feet = None
        self._line_geoms = None    # with WANT_LINE_GEOM: the tables behind line_geoms / frame_line_geoms / geom_points
        self._frame_line_geoms = None
        self._geom_points = None
        self._line_words = None    # with WANT_LINE_WORDS: the tables behind line_words / line_runs / words
        self._line_runs = None
        self._words = None
        self._run_reads = None     # with WANT_RUN_READ: the tables behind run_reads / run_features
        self._run_features = None
        self._word_matches = None  # with WANT_WORD_MATCH: the tables behind word_matches / run_costs / run_probs, and the lexicon's words
        self._run_costs = None
        self._run_probs = None
        self._lexicon = ()
        self._word_decodes = None  # with WANT_WORD_DECODE: the tables behind word_decodes / word_decode_chars / word_decode_src (and run_costs / run_probs)
        self._word_decode_chars = None
        self._word_decode_src = None
        self._run_splits = None    # with WANT_RUN_SPLIT: the tables behind run_splits / run_pieces / piece_reads / piece_costs / split_parts / word_splits
        self._lattice_matches = None  # with WANT_LATTICE_MATCH: the tables behind lattice_matches / lattice_match_src / lattice_match_parts
        self._lattice_match_src = self._lattice_match_parts = None
        self._lattice_decodes = None  # with WANT_LATTICE_DECODE: the tables behind lattice_decodes / lattice_decode_chars / lattice_decode_src / lattice_parts
        self._word_links = None    # with WANT_TRACK_READ: the tables behind word_links / word_tracks / word_track_members / word_track_of_words / track_matches / track_member_costs
        self._word_tracks = self._word_track_members = self._word_track_of_words = self._track_matches = self._track_member_costs = None
        self._track_decodes = self._track_decode_chars = self._track_decode_member_costs = None  # with WANT_TRACK_DECODE: the tables behind track_decodes / track_decode_chars / track_decode_member_costs
        self._lattice_track_matches = None  # with WANT_LATTICE_TRACK: the tables behind lattice_track_matches / lattice_track_members / lattice_track_src / lattice_track_parts
        self._lattice_track_members = self._lattice_track_src = self._lattice_track_parts = None
        self._run_pieces = None
        self._piece_reads = None
        self._piece_costs = None
        self._split_parts = None
        self._word_splits = None
        self._planes = None

    def _line_words_table(self, table):
        if table is None:
            raise ValueError("the result has no line words (pass WANT_LINE_WORDS / want_line_words=True)")
        return table

    @property
    def line_words(self) -> np.ndarray:
        """With WANT_LINE_WORDS: LINE_WORDS_DTYPE per line of texts."""
        return self._line_words_table(self._line_words)

    @property
    def line_runs(self) -> np.ndarray:
        """With WANT_LINE_WORDS: LINE_RUN_DTYPE, the glyph runs of the lines back to back in line order."""
        return self._line_words_table(self._line_runs)

    @property
    def words(self) -> np.ndarray:
        """With WANT_LINE_WORDS: LINE_WORD_DTYPE, the words of the lines back to back in line order."""
        return self._line_words_table(self._words)

    def words_of_line(self, t: int) -> np.ndarray:
        """With WANT_LINE_WORDS: the words of line t (LINE_WORD_DTYPE), left to right."""
        lw = self.line_words[t]
        return self.words[int(lw["first_word"]):int(lw["first_word"]) + int(lw["n_words"])].copy()

    def runs_of_line(self, t: int) -> np.ndarray:
        """With WANT_LINE_WORDS: the glyph runs of line t (LINE_RUN_DTYPE), left to right."""
        lw = self.line_words[t]
        return self.line_runs[int(lw["first_run"]):int(lw["first_run"]) + int(lw["n_runs"])].copy()

    def frame_line_words(self, i: int) -> np.ndarray:
        """With WANT_LINE_WORDS: the words of frame line i: those of its representative line."""
        return self.words_of_line(int(self.frame_lines[i]["rep"]))

    def _run_read_table(self, table):
        if table is None:
            raise ValueError("the result has no run reads (pass WANT_RUN_READ / want_run_read=True)")
        return table

    @property
    def run_reads(self) -> np.ndarray:
        """With WANT_RUN_READ: RUN_READ_DTYPE per glyph run of line_runs, in the same order."""
        return self._run_read_table(self._run_reads)

    @property
    def run_features(self) -> np.ndarray:
        """With WANT_RUN_READ: (n runs, 1800) uint8, the feature bytes the scorer read from every run's tile."""
        return self._run_read_table(self._run_features)

    def word_text(self, w: int) -> str:
        """With WANT_RUN_READ: the string of word w (an index into words): the characters of its runs."""
        wd = self.words[w]
        return "".join(chr(int(c)) for c in self.run_reads["ch"][int(wd["first_run"]):int(wd["first_run"]) + int(wd["n_runs"])])

    def words_text_of_line(self, t: int) -> list:
        """With WANT_RUN_READ: the strings of the words of line t, left to right."""
        lw = self.line_words[t]
        return [self.word_text(w) for w in range(int(lw["first_word"]), int(lw["first_word"]) + int(lw["n_words"]))]

    def frame_line_text(self, i: int) -> str:
        """With WANT_RUN_READ: the text of frame line i: the words of its representative line joined by one blank."""
        return " ".join(self.words_text_of_line(int(self.frame_lines[i]["rep"])))

    def _word_match_table(self, table):
        if table is None:
            raise ValueError("the result has no word matches (pass WANT_WORD_MATCH / want_word_match=True)")
        return table

    def _word_decode_table(self, table):
        if table is None:
            raise ValueError("the result has no word decodes (pass WANT_WORD_DECODE / want_word_decode=True)")
        return table

    def _word_margin_table(self, table):
        if table is None:
            raise ValueError("the result has no word margins (ERFilter.set_word_margin(True) and WANT_WORD_DECODE / want_word_decode=True)")
        return table

    def _line_decode_table(self, table):
        if table is None:
            raise ValueError("the result has no line decodes (ERFilter.set_line_decode(True) and WANT_WORD_DECODE / want_word_decode=True)")
        return table

    def _line_lattice_table(self, table):
        if table is None:
            raise ValueError("the result has no line lattice decodes (ERFilter.set_line_lattice_decode(True) and WANT_LATTICE_DECODE / want_lattice_decode=True)")
        return table

    def _line_margin_table(self, table):
        if table is None:
            raise ValueError("the result has no line margins (ERFilter.set_line_margin(True) beside set_line_decode(True) and WANT_WORD_DECODE)")
        return table

    def _run_split_table(self, table):
        if table is None:
            raise ValueError("the result has no run splits (pass WANT_RUN_SPLIT / want_run_split=True)")
        return table

    @property
    def run_splits(self) -> np.ndarray:
        """With WANT_RUN_SPLIT: RUN_SPLIT_DTYPE per run of line_runs, in the same order."""
        return self._run_split_table(getattr(self, "_run_splits", None))

    @property
    def run_pieces(self) -> np.ndarray:
        """With WANT_RUN_SPLIT: RUN_PIECE_DTYPE, the pieces of the cut runs back to back in run order."""
        return self._run_split_table(getattr(self, "_run_pieces", None))

    @property
    def piece_reads(self) -> np.ndarray:
        """With WANT_RUN_SPLIT: RUN_READ_DTYPE per piece of run_pieces."""
        return self._run_split_table(getattr(self, "_piece_reads", None))

    @property
    def piece_costs(self) -> np.ndarray:
        """With WANT_RUN_SPLIT: (n pieces, 65) uint8, the cost row of every piece (folded where run_costs are)."""
        return self._run_split_table(getattr(self, "_piece_costs", None))

    @property
    def split_parts(self) -> np.ndarray:
        """With WANT_RUN_SPLIT: SPLIT_PART_DTYPE, the split sequences of the words back to back in word order."""
        return self._run_split_table(getattr(self, "_split_parts", None))

    @property
    def word_splits(self) -> np.ndarray:
        """With WANT_RUN_SPLIT: WORD_SPLIT_DTYPE per word of words, in the same order."""
        return self._run_split_table(getattr(self, "_word_splits", None))

    def word_split_text(self, w: int) -> str:
        """With WANT_RUN_SPLIT: the string of the split sequence of word w: per part -- a whole run or a piece -- the character of the
        first minimum of its cost row (run_costs / piece_costs; where a lexicon folds them, the first of a case pair)."""
        ws = self.word_splits[w]
        out = []
        for p in self.split_parts[int(ws["first_part"]):int(ws["first_part"]) + int(ws["n_parts"])]:
            row = self.run_costs[int(p["run"])] if int(p["piece"]) < 0 else self.piece_costs[int(p["piece"])]
            out.append(_OCR_ALPHABET[int(np.argmin(row))])
        return "".join(out)

    def words_split_text_of_line(self, t: int) -> list:
        """With WANT_RUN_SPLIT: word_split_text of the words of line t, left to right."""
        lw = self.line_words[t]
        return [self.word_split_text(w) for w in range(int(lw["first_word"]), int(lw["first_word"]) + int(lw["n_words"]))]

    def frame_line_split_text(self, i: int) -> str:
        """With WANT_RUN_SPLIT: the split text of frame line i: words_split_text_of_line of its representative joined by one blank."""
        return " ".join(self.words_split_text_of_line(int(self.frame_lines[i]["rep"])))

    def _lattice_decode_table(self, table):
        if table is None:
            raise ValueError("the result has no lattice decodes (pass WANT_LATTICE_DECODE / want_lattice_decode=True)")
        return table

    @property
    def lattice_decodes(self) -> np.ndarray:
        """With WANT_LATTICE_DECODE: LATTICE_DECODE_DTYPE per word of words, in the same order."""
        return self._lattice_decode_table(getattr(self, "_lattice_decodes", None))

    @property
    def lattice_decode_chars(self) -> np.ndarray:
        """With WANT_LATTICE_DECODE: (n words, 64) uint8, the labels of every word's string, 0xFF past n_chars."""
        return self._lattice_decode_table(getattr(self, "_lattice_decode_chars", None))

    @property
    def lattice_decode_src(self) -> np.ndarray:
        """With WANT_LATTICE_DECODE: (n words, 64) uint8, per character the word-relative index of the lattice part it came from, bit 7
        set on an inserted character; 0xFF past n_chars."""
        return self._lattice_decode_table(getattr(self, "_lattice_decode_src", None))

    @property
    def lattice_parts(self) -> np.ndarray:
        """With WANT_LATTICE_DECODE: SPLIT_PART_DTYPE, the lattice parts of the words back to back in word order (piece -1: a whole
        run; the indices are those of split_parts)."""
        return self._lattice_decode_table(getattr(self, "_lattice_parts", None))

    def _lattice_margin_table(self, table):
        if table is None:
            raise ValueError("the result has no lattice margins (ERFilter.set_lattice_margin(True) and WANT_LATTICE_DECODE / want_lattice_decode=True)")
        return table

    @property
    def lattice_margins(self) -> np.ndarray:
        """With set_lattice_margin(True) and WANT_LATTICE_DECODE: LATTICE_MARGIN_DTYPE per word of words, in the same order."""
        return self._lattice_margin_table(getattr(self, "_lattice_margins", None))

    @property
    def lattice_read_margins(self) -> np.ndarray:
        """With set_lattice_margin(True) and WANT_LATTICE_DECODE: (n words, 32) int32, the reading margin of every lattice part of every
        word, -1 past its parts."""
        return self._lattice_margin_table(getattr(self, "_lattice_read_margins", None))

    @property
    def lattice_cut_margins(self) -> np.ndarray:
        """With set_lattice_margin(True) and WANT_LATTICE_DECODE: (n words, 32) int32, the cut margin of every lattice part of every word,
        -1 past its parts and for a part of a run without cuts."""
        return self._lattice_margin_table(getattr(self, "_lattice_cut_margins", None))

    @property
    def lattice_part_reads(self) -> np.ndarray:
        """With set_lattice_margin(True) and WANT_LATTICE_DECODE: (n words, 32) uint8, how the decoded string reads every lattice part
        (65: dropped), 0xFF past the word's parts."""
        return self._lattice_margin_table(getattr(self, "_lattice_part_reads", None))

    @property
    def lattice_part_alts(self) -> np.ndarray:
        """With set_lattice_margin(True) and WANT_LATTICE_DECODE: (n words, 32) uint8, the cheapest other reading of every lattice part
        (65: dropped), 0xFF past the word's parts."""
        return self._lattice_margin_table(getattr(self, "_lattice_part_alts", None))

    @property
    def lattice_cut_alts(self) -> np.ndarray:
        """With set_lattice_margin(True) and WANT_LATTICE_DECODE: (n words, 32) uint8, the cheapest other edge over every lattice part's
        atoms as i | j << 4 (local nodes of the part's run), 0xFF past the word's parts and where there is none."""
        return self._lattice_margin_table(getattr(self, "_lattice_cut_alts", None))

    def word_lattice_margin(self, w: int) -> tuple:
        """With set_lattice_margin(True) and WANT_LATTICE_DECODE: (reading margin, cut margin) of word w: the extra cost of the cheapest
        path that reads some part differently from word_lattice_text(w), and of the cheapest path that cuts the word differently from
        word_lattice_parts(w) (-1: no run of the word is cut); (-1, -1) for a word that was not decoded or has no runs."""
        g = self.lattice_margins[w]
        return int(g["read_margin"]), int(g["cut_margin"])

    def word_lattice_part_margins(self, w: int) -> list:
        """With set_lattice_margin(True) and WANT_LATTICE_DECODE: per lattice part of word w (word_lattice_parts(w)) the pair (reading
        margin, cut margin), the cut margin -1 for a part of a run without cuts; none for a word that was not decoded."""
        n = int(self.lattice_decodes[w]["n_parts"]) if int(self.lattice_decodes[w]["cost"]) >= 0 else 0
        return [(int(a), int(b)) for a, b in zip(self.lattice_read_margins[w, :n], self.lattice_cut_margins[w, :n])]

    def word_lattice_text(self, w: int) -> str:
        """With WANT_LATTICE_DECODE: the jointly decoded string of word w; word_text(w) for a word that was not decoded (cost < 0)."""
        d = self.lattice_decodes[w]
        if int(d["cost"]) < 0:
            return self.word_text(w)
        return "".join(_OCR_ALPHABET[int(a)] for a in self.lattice_decode_chars[w, :int(d["n_chars"])])

    def word_lattice_parts(self, w: int) -> np.ndarray:
        """With WANT_LATTICE_DECODE: the lattice parts of word w (SPLIT_PART_DTYPE), the segmentation chosen with its string; none for
        a word that was not decoded."""
        d = self.lattice_decodes[w]
        return self.lattice_parts[int(d["first_part"]):int(d["first_part"]) + int(d["n_parts"])]

    def words_lattice_text_of_line(self, t: int) -> list:
        """With WANT_LATTICE_DECODE: word_lattice_text of the words of line t, left to right."""
        lw = self.line_words[t]
        return [self.word_lattice_text(w) for w in range(int(lw["first_word"]), int(lw["first_word"]) + int(lw["n_words"]))]

    def frame_line_lattice_text(self, i: int) -> str:
        """With WANT_LATTICE_DECODE: the jointly decoded text of frame line i: words_lattice_text_of_line of its representative joined by one blank."""
        return " ".join(self.words_lattice_text_of_line(int(self.frame_lines[i]["rep"])))

    def _lattice_match_table(self, table):
        if table is None:
            raise ValueError("the result has no lattice matches (pass WANT_LATTICE_MATCH / want_lattice_match=True)")
        return table

    @property
    def lattice_matches(self) -> np.ndarray:
        """With WANT_LATTICE_MATCH: LATTICE_MATCH_DTYPE per word of words, in the same order."""
        return self._lattice_match_table(getattr(self, "_lattice_matches", None))

    @property
    def lattice_match_src(self) -> np.ndarray:
        """With WANT_LATTICE_MATCH: (n words, 32) uint8, per character of the winning entry the word-relative index of the part it was
        read from; for an inserted character 0x80 | the number of parts that end at or before its node; 0xFF past the entry."""
        return self._lattice_match_table(getattr(self, "_lattice_match_src", None))

    @property
    def lattice_match_parts(self) -> np.ndarray:
        """With WANT_LATTICE_MATCH: SPLIT_PART_DTYPE, the parts of the winning entries of the words back to back in word order (piece
        -1: a whole run; the indices are those of split_parts)."""
        return self._lattice_match_table(getattr(self, "_lattice_match_parts", None))

    def word_lattice_match_text(self, w: int) -> str:
        """With WANT_LATTICE_MATCH: the lexicon entry that matches word w best over its piece lattice, as it was given to set_lexicon;
        word_text(w) for a word without a match."""
        e = int(self.lattice_matches[w]["entry"])
        lex = getattr(self, "_lexicon", ())
        return lex[e] if 0 <= e < len(lex) else self.word_text(w)

    def word_lattice_match_parts(self, w: int) -> np.ndarray:
        """With WANT_LATTICE_MATCH: the parts of word w (SPLIT_PART_DTYPE), the segmentation chosen with its best entry; none for a word
        without a match."""
        d = self.lattice_matches[w]
        return self.lattice_match_parts[int(d["first_part"]):int(d["first_part"]) + int(d["n_parts"])]

    def words_lattice_match_text_of_line(self, t: int) -> list:
        """With WANT_LATTICE_MATCH: word_lattice_match_text of the words of line t, left to right."""
        lw = self.line_words[t]
        return [self.word_lattice_match_text(w) for w in range(int(lw["first_word"]), int(lw["first_word"]) + int(lw["n_words"]))]

    def frame_line_lattice_match_text(self, i: int) -> str:
        """With WANT_LATTICE_MATCH: the text of frame line i matched over the piece lattices: words_lattice_match_text_of_line of its
        representative joined by one blank."""
        return " ".join(self.words_lattice_match_text_of_line(int(self.frame_lines[i]["rep"])))

    @property
    def word_decodes(self) -> np.ndarray:
        """With WANT_WORD_DECODE: WORD_DECODE_DTYPE per word of words, in the same order."""
        return self._word_decode_table(getattr(self, "_word_decodes", None))

    @property
    def word_decode_chars(self) -> np.ndarray:
        """With WANT_WORD_DECODE: (n words, 64) uint8, the labels of every word's string, 0xFF past n_chars."""
        return self._word_decode_table(getattr(self, "_word_decode_chars", None))

    @property
    def word_decode_src(self) -> np.ndarray:
        """With WANT_WORD_DECODE: (n words, 64) uint8, per character the word-relative index of the run it came from, bit 7 set on an
        inserted character; 0xFF past n_chars."""
        return self._word_decode_table(getattr(self, "_word_decode_src", None))

    def word_decode_text(self, w: int) -> str:
        """With WANT_WORD_DECODE: the decoded string of word w; word_text(w) for a word that was not decoded (cost < 0)."""
        d = self.word_decodes[w]
        if int(d["cost"]) < 0:
            return self.word_text(w)
        return "".join(_OCR_ALPHABET[int(a)] for a in self.word_decode_chars[w, :int(d["n_chars"])])

    def word_decode_runs(self, w: int) -> list:
        """With WANT_WORD_DECODE: per character of word_decode_text(w), (index into line_runs of the run it came from, whether it
        was inserted behind that run); for a word that was not decoded its runs, none inserted."""
        d, first = self.word_decodes[w], int(self.words[w]["first_run"])
        if int(d["cost"]) < 0:
            return [(first + k, False) for k in range(int(self.words[w]["n_runs"]))]
        return [(first + (int(v) & 0x7F), bool(int(v) & 0x80)) for v in self.word_decode_src[w, :int(d["n_chars"])]]

    @property
    def line_decodes(self) -> np.ndarray:
        """With set_line_decode(True) and WANT_WORD_DECODE: LINE_DECODE_DTYPE per line of texts, in the same order."""
        return self._line_decode_table(getattr(self, "_line_decodes", None))

    @property
    def line_decode_chars(self) -> np.ndarray:
        """With set_line_decode(True) and WANT_WORD_DECODE: (3 x n rows) uint8, the labels of every line's string (65: a blank) from entry
        3 * first row of its window on, 0xFF past n_chars.  A row is a run of line_runs, with WANT_RUN_SPLIT a part of split_parts."""
        return self._line_decode_table(getattr(self, "_line_decode_chars", None))

    @property
    def line_decode_src(self) -> np.ndarray:
        """With set_line_decode(True) and WANT_WORD_DECODE: (3 x n rows) uint16, per label the line-relative row it came from, 0x8000 set
        on an inserted character and 0x4000 on the break in front of that row; 0xFFFF past n_chars."""
        return self._line_decode_table(getattr(self, "_line_decode_src", None))

    @property
    def line_decode_word_of_row(self) -> np.ndarray:
        """With set_line_decode(True) and WANT_WORD_DECODE: int32 per row, the decoded word of its line it is read in, -1 for a dropped
        row."""
        return self._line_decode_table(getattr(self, "_line_decode_word_of_row", None))

    @property
    def line_gap_costs(self) -> np.ndarray:
        """With set_line_decode(True) and WANT_WORD_DECODE: (n rows, 2) uint8, the (join, break) costs of the gap in front of every row."""
        return self._line_decode_table(getattr(self, "_line_gap_costs", None))

    @property
    def line_decode_windows(self) -> np.ndarray:
        """With set_line_decode(True) and WANT_WORD_DECODE: (n lines, 2) int32, the first row and the row count of every line."""
        return self._line_decode_table(getattr(self, "_line_decode_windows", None))

    @property
    def line_margins(self) -> np.ndarray:
        """With set_line_margin(True) beside the line decode: LINE_MARGIN_DTYPE per line of texts, in the same order."""
        return self._line_margin_table(getattr(self, "_line_margins", None))

    @property
    def line_row_margins(self) -> np.ndarray:
        """With set_line_margin(True): int32 per row of the line decode's rows, how much more the cheapest path costs that reads the row
        differently; -1 for a row of a line that was not decoded."""
        return self._line_margin_table(getattr(self, "_line_row_margins", None))

    @property
    def line_row_reads(self) -> np.ndarray:
        """With set_line_margin(True): uint8 per row, the label the decoded string reads it as (65: dropped), 0xFF where there is none."""
        return self._line_margin_table(getattr(self, "_line_row_reads", None))

    @property
    def line_row_alts(self) -> np.ndarray:
        """With set_line_margin(True): uint8 per row, the reading of the cheapest path that reads it differently (65: dropped)."""
        return self._line_margin_table(getattr(self, "_line_row_alts", None))

    @property
    def line_gap_margins(self) -> np.ndarray:
        """With set_line_margin(True): int32 per row, how much more the cheapest path costs that takes the other move at the gap in
        front of it; -1 for the first row of a line and where the other move is off."""
        return self._line_margin_table(getattr(self, "_line_gap_margins", None))

    @property
    def line_gap_moves(self) -> np.ndarray:
        """With set_line_margin(True): uint8 per row, the decided move of the gap in front of it: 0 join, 1 break, 0xFF for the first
        row of a line."""
        return self._line_margin_table(getattr(self, "_line_gap_moves", None))

    def line_decode_margin(self, t: int) -> int:
        """With set_line_margin(True): the margin of line t (the smaller of its smallest row margin and its smallest gap margin), -1
        for a line without rows or one that was not decoded."""
        return int(self.line_margins[t]["margin"])

    def line_break_margins(self, t: int) -> list:
        """With set_line_margin(True): per gap of line t (line-relative row it lies in front of, move: 0 join / 1 break, margin: -1
        where the other move is off)."""
        first, n = (int(v) for v in self.line_decode_windows[t])
        if int(self.line_margins[t]["margin"]) < 0:
            return []
        return [(k, int(self.line_gap_moves[first + k]), int(self.line_gap_margins[first + k])) for k in range(1, n)]

    def _line_decode_slice(self, t: int):
        d, first = self.line_decodes[t], int(self.line_decode_windows[t, 0])
        n = max(0, int(d["n_chars"]))
        return d, first, self.line_decode_chars[3 * first:3 * first + n], self.line_decode_src[3 * first:3 * first + n]

    def line_decode_text(self, t: int) -> str:
        """With set_line_decode(True): the decoded string of line t, a blank per break (consecutive blanks are kept); for a line that
        was not decoded (cost < 0) its words' decoded strings joined by one blank."""
        d, first, lab, src = self._line_decode_slice(t)
        if int(d["cost"]) < 0:
            return " ".join(self.words_decode_text_of_line(t))
        return "".join(" " if int(a) == 65 else _OCR_ALPHABET[int(a)] for a in lab)

    def frame_line_line_decode_text(self, i: int) -> str:
        """With set_line_decode(True): line_decode_text of the representative line of frame line i."""
        return self.line_decode_text(int(self.frame_lines[i]["rep"]))

    def line_decode_words(self, t: int) -> list:
        """With set_line_decode(True): the words of line t under the decoded segmentation, empty ones included: per word (text,
        (x, y, w, h) the bounding box of the runs of its rows that are read, None for a word without one)."""
        d, first, lab, src = self._line_decode_slice(t)
        if int(d["cost"]) < 0:
            lw = self.line_words[t]
            return [(self.word_decode_text(w), tuple(int(self.words[w][k]) for k in ("x", "y", "w", "h")))
                    for w in range(int(lw["first_word"]), int(lw["first_word"]) + int(lw["n_words"]))]
        texts, boxes = [""], [None]
        for a, v in zip(lab, src):
            if int(a) == 65:
                texts.append(""); boxes.append(None)
                continue
            texts[-1] += _OCR_ALPHABET[int(a)]
            if not int(v) & 0x8000:
                row = first + (int(v) & 0x3FFF)          # (a run, or with WANT_RUN_SPLIT a part: its run's box)
                parts = getattr(self, "_split_parts", None)
                q = self.line_runs[row if parts is None else int(parts[row]["run"])]
                b = boxes[-1]
                x0, y0, x1, y1 = int(q["x0"]), int(q["y0"]), int(q["x1"]), int(q["y1"])
                boxes[-1] = (x0, y0, x1, y1) if b is None else (min(b[0], x0), min(b[1], y0), max(b[2], x1), max(b[3], y1))
        return [(s, None if b is None else (b[0], b[1], b[2] - b[0], b[3] - b[1])) for s, b in zip(texts, boxes)]

    @property
    def line_lattice_decodes(self) -> np.ndarray:
        """With set_line_lattice_decode(True) and WANT_LATTICE_DECODE: LINE_LATTICE_DECODE_DTYPE per line of texts, in the same order."""
        return self._line_lattice_table(getattr(self, "_line_lattice_decodes", None))

    @property
    def line_lattice_chars(self) -> np.ndarray:
        """With set_line_lattice_decode(True): (3 x atoms of run_splits) uint8, the labels of every line's string (65: a blank) from entry
        3 * (the atoms of the runs before the first run of its window) on, 0xFF past n_chars."""
        return self._line_lattice_table(getattr(self, "_line_lattice_chars", None))

    @property
    def line_lattice_src(self) -> np.ndarray:
        """With set_line_lattice_decode(True): (3 x atoms) uint16, per label the line-relative part it came from, 0x8000 set on an
        inserted character and 0x4000 on the break in front of that part; 0xFFFF past n_chars."""
        return self._line_lattice_table(getattr(self, "_line_lattice_src", None))

    @property
    def line_lattice_parts(self) -> np.ndarray:
        """With set_line_lattice_decode(True): SPLIT_PART_DTYPE, the parts of the lines' paths back to back (first_part, n_parts of the
        records), with the indices of run_pieces."""
        return self._line_lattice_table(getattr(self, "_line_lattice_parts", None))

    @property
    def line_lattice_word_of_part(self) -> np.ndarray:
        """With set_line_lattice_decode(True): int32 per part, the decoded word of its line it is read in, -1 for a dropped part."""
        return self._line_lattice_table(getattr(self, "_line_lattice_word_of_part", None))

    @property
    def line_lattice_gap_costs(self) -> np.ndarray:
        """With set_line_lattice_decode(True): (n runs, 2) uint8, the (join, break) costs of the gap in front of every run of line_runs."""
        return self._line_lattice_table(getattr(self, "_line_lattice_gap_costs", None))

    @property
    def line_lattice_windows(self) -> np.ndarray:
        """With set_line_lattice_decode(True): (n lines, 2) int32, the first run and the run count of every line."""
        return self._line_lattice_table(getattr(self, "_line_lattice_windows", None))

    def _line_lattice_slice(self, t: int):
        d, first = self.line_lattice_decodes[t], int(self.line_lattice_windows[t, 0])
        at = 3 * int(line_lattice_node_slots(self.run_splits, [first])[0]) if len(self.run_splits) else 0
        n = max(0, int(d["n_chars"]))
        return d, self.line_lattice_chars[at:at + n], self.line_lattice_src[at:at + n]

    def line_lattice_text(self, t: int) -> str:
        """With set_line_lattice_decode(True): the decoded string of line t, a blank per break (consecutive blanks are kept); for a
        line that was not decoded (cost < 0) its words' lattice strings joined by one blank."""
        d, lab, src = self._line_lattice_slice(t)
        if int(d["cost"]) < 0:
            return " ".join(self.words_lattice_text_of_line(t))
        return "".join(" " if int(a) == 65 else _OCR_ALPHABET[int(a)] for a in lab)

    def frame_line_line_lattice_text(self, i: int) -> str:
        """With set_line_lattice_decode(True): line_lattice_text of the representative line of frame line i."""
        return self.line_lattice_text(int(self.frame_lines[i]["rep"]))

    def line_lattice_words(self, t: int) -> list:
        """With set_line_lattice_decode(True): the words of line t under the decoded cuts and breaks, empty ones included: per word
        (text, its parts as SPLIT_PART_DTYPE, (x, y, w, h) the union of the boxes of its parts that are read -- a piece's box, a whole
        run's -- or None for a word without one).  A line that was not decoded has no words here."""
        d, lab, src = self._line_lattice_slice(t)
        if int(d["cost"]) < 0:
            return []
        parts = self.line_lattice_parts[int(d["first_part"]):int(d["first_part"]) + int(d["n_parts"])]
        texts, boxes, own = [""], [None], [[]]
        for a, v in zip(lab, src):
            if int(a) == 65:
                texts.append(""); boxes.append(None); own.append([])
                continue
            texts[-1] += _OCR_ALPHABET[int(a)]
            if not int(v) & 0x8000:
                k = int(v) & 0x3FFF
                own[-1].append(k)
                q = self.line_runs[int(parts[k]["run"])] if int(parts[k]["piece"]) < 0 else self.run_pieces[int(parts[k]["piece"])]
                b = boxes[-1]
                x0, y0, x1, y1 = int(q["x0"]), int(q["y0"]), int(q["x1"]), int(q["y1"])
                boxes[-1] = (x0, y0, x1, y1) if b is None else (min(b[0], x0), min(b[1], y0), max(b[2], x1), max(b[3], y1))
        return [(s, parts[np.asarray(ks, np.int64)], None if b is None else (b[0], b[1], b[2] - b[0], b[3] - b[1])) for s, ks, b in zip(texts, own, boxes)]

    @property
    def word_margins(self) -> np.ndarray:
        """With set_word_margin(True) and WANT_WORD_DECODE: WORD_MARGIN_DTYPE per word of words, in the same order."""
        return self._word_margin_table(getattr(self, "_word_margins", None))

    @property
    def word_row_margins(self) -> np.ndarray:
        """With set_word_margin(True) and WANT_WORD_DECODE: (n words, 32) int32, the margin of every row of every word, -1 past its rows."""
        return self._word_margin_table(getattr(self, "_word_row_margins", None))

    @property
    def word_row_reads(self) -> np.ndarray:
        """With set_word_margin(True) and WANT_WORD_DECODE: (n words, 32) uint8, how the decoded string reads every row (65: dropped),
        0xFF past the word's rows."""
        return self._word_margin_table(getattr(self, "_word_row_reads", None))

    @property
    def word_row_alts(self) -> np.ndarray:
        """With set_word_margin(True) and WANT_WORD_DECODE: (n words, 32) uint8, the cheapest other reading of every row (65: dropped),
        0xFF past the word's rows."""
        return self._word_margin_table(getattr(self, "_word_row_alts", None))

    def word_decode_margin(self, w: int) -> int:
        """With set_word_margin(True) and WANT_WORD_DECODE: the margin of word w: the extra cost of the cheapest path that reads some
        run differently from word_decode_text(w); -1 for a word that was not decoded or has no runs."""
        return int(self.word_margins[w]["margin"])

    def word_decode_char_margins(self, w: int) -> list:
        """With set_word_margin(True) and WANT_WORD_DECODE: per character of word_decode_text(w), the margin of the row it came from,
        and -1 for an inserted character (it has no row); for a word that was not decoded -1 per run."""
        d, rows = self.word_decodes[w], self.word_row_margins[w]
        if int(d["cost"]) < 0:
            return [-1] * int(self.words[w]["n_runs"])
        return [-1 if int(v) & 0x80 else int(rows[int(v)]) for v in self.word_decode_src[w, :int(d["n_chars"])]]

    def words_decode_text_of_line(self, t: int) -> list:
        """With WANT_WORD_DECODE: word_decode_text of the words of line t, left to right."""
        lw = self.line_words[t]
        return [self.word_decode_text(w) for w in range(int(lw["first_word"]), int(lw["first_word"]) + int(lw["n_words"]))]

    def frame_line_decode_text(self, i: int) -> str:
        """With WANT_WORD_DECODE: the decoded text of frame line i: words_decode_text_of_line of its representative joined by one blank."""
        return " ".join(self.words_decode_text_of_line(int(self.frame_lines[i]["rep"])))

    @property
    def word_matches(self) -> np.ndarray:
        """With WANT_WORD_MATCH: WORD_MATCH_DTYPE per word of words, in the same order."""
        return self._word_match_table(self._word_matches)

    @property
    def run_costs(self) -> np.ndarray:
        """With WANT_WORD_MATCH, WANT_WORD_DECODE or WANT_RUN_SPLIT: (n runs, 65) uint8, the cost row of every glyph run of line_runs
        (folded as the lexicon says with WANT_WORD_MATCH, else unfolded)."""
        return self._word_match_table(self._run_costs)

    @property
    def run_probs(self) -> np.ndarray:
        """With WANT_WORD_MATCH or WANT_WORD_DECODE: (n runs, nr_class) float64, the class probabilities of every glyph run in the model's class order."""
        return self._word_match_table(self._run_probs)

    def word_match_text(self, w: int) -> str:
        """With WANT_WORD_MATCH: the lexicon entry that matches word w best, as it was given to set_lexicon; word_text(w) for a
        word without a match."""
        e = int(self.word_matches[w]["entry"])
        return self._lexicon[e] if 0 <= e < len(self._lexicon) else self.word_text(w)

    def words_match_text_of_line(self, t: int) -> list:
        """With WANT_WORD_MATCH: word_match_text of the words of line t, left to right."""
        lw = self.line_words[t]
        return [self.word_match_text(w) for w in range(int(lw["first_word"]), int(lw["first_word"]) + int(lw["n_words"]))]

    def frame_line_match_text(self, i: int) -> str:
        """With WANT_WORD_MATCH: the matched text of frame line i: words_match_text_of_line of its representative joined by one blank."""
        return " ".join(self.words_match_text_of_line(int(self.frame_lines[i]["rep"])))

    def _track_read_table(self, table):
        if table is None:
            raise ValueError("the result has no word tracks (pass WANT_TRACK_READ / want_track_read=True)")
        return table

    def _track_decode_table(self, table):
        if table is None:
            raise ValueError("the result has no track decodes (pass WANT_TRACK_DECODE / want_track_decode=True)")
        return table

    @property
    def track_decodes(self) -> np.ndarray:
        """With WANT_TRACK_DECODE: TRACK_DECODE_DTYPE per word track."""
        return self._track_decode_table(self._track_decodes)

    @property
    def track_decode_chars(self) -> np.ndarray:
        """With WANT_TRACK_DECODE: (n tracks, 32) uint8, the labels of every track's string, 0xFF past n_chars."""
        return self._track_decode_table(self._track_decode_chars)

    @property
    def track_decode_member_costs(self) -> np.ndarray:
        """With WANT_TRACK_DECODE: the own alignment cost of every member of word_track_members for its track's string (int32), -1 without one."""
        return self._track_decode_table(self._track_decode_member_costs)

    def word_track_decode_text(self, g: int) -> str:
        """With WANT_TRACK_DECODE: the string word track g was decoded to; the representative's own reading (word_text) where the track
        was not decoded."""
        d = self.track_decodes[g]
        if int(d["cost"]) < 0:
            return self.word_text(int(self.word_tracks[g]["rep"]))
        return "".join(_OCR_ALPHABET[int(a)] for a in self.track_decode_chars[g, :int(d["n_chars"])])

    def text_track_decode_text(self, k: int) -> str:
        """With WANT_TRACK_DECODE: the words of the representative line of text track k in order, each as its word track's decoded
        string (its own word_text where the line is no reading line), joined by one blank."""
        lw = self.line_words[int(self.text_tracks[k]["rep"])]
        of = self.word_track_of_words
        ws = range(int(lw["first_word"]), int(lw["first_word"]) + int(lw["n_words"]))
        return " ".join(self.word_track_decode_text(int(of[w])) if of[w] >= 0 else self.word_text(w) for w in ws)

    @property
    def word_links(self) -> np.ndarray:
        """With WANT_TRACK_READ: WORD_LINK_DTYPE, the pairs of words of adjacent frames whose boxes overlap, sorted by (a, b)."""
        return self._track_read_table(self._word_links)

    @property
    def word_tracks(self) -> np.ndarray:
        """With WANT_TRACK_READ: WORD_TRACK_DTYPE per word track, by first frame, then by smallest member."""
        return self._track_read_table(self._word_tracks)

    @property
    def word_track_members(self) -> np.ndarray:
        """With WANT_TRACK_READ: the word indices the word tracks index (int32)."""
        return self._track_read_table(self._word_track_members)

    @property
    def word_track_of_words(self) -> np.ndarray:
        """With WANT_TRACK_READ: the word track of every word of words (int32), -1 for a word that is not eligible."""
        return self._track_read_table(self._word_track_of_words)

    @property
    def track_matches(self) -> np.ndarray:
        """With WANT_TRACK_READ: TRACK_MATCH_DTYPE per word track."""
        return self._track_read_table(self._track_matches)

    @property
    def track_member_costs(self) -> np.ndarray:
        """With WANT_TRACK_READ: the own cost of every member of word_track_members for its track's entry (int32), -1 without one."""
        return self._track_read_table(self._track_member_costs)

    def word_track_text(self, g: int) -> str:
        """With WANT_TRACK_READ: the lexicon entry word track g takes, as it was given to set_lexicon; the representative's own
        reading (word_text) where the track has no entry."""
        e = int(self.track_matches[g]["entry"])
        return self._lexicon[e] if 0 <= e < len(self._lexicon) else self.word_text(int(self.word_tracks[g]["rep"]))

    def text_track_match_text(self, k: int) -> str:
        """With WANT_TRACK_READ: the words of the representative line of text track k in order, each as its word track's text
        (its own word_text where the line is no reading line), joined by one blank."""
        lw = self.line_words[int(self.text_tracks[k]["rep"])]
        of = self.word_track_of_words
        ws = range(int(lw["first_word"]), int(lw["first_word"]) + int(lw["n_words"]))
        return " ".join(self.word_track_text(int(of[w])) if of[w] >= 0 else self.word_text(w) for w in ws)

    def _lattice_track_table(self, table):
        if table is None:
            raise ValueError("the result has no lattice track matches (pass WANT_LATTICE_TRACK / want_lattice_track=True)")
        return table

    @property
    def lattice_track_matches(self) -> np.ndarray:
        """With WANT_LATTICE_TRACK: TRACK_MATCH_DTYPE per word track, over the members' piece lattices."""
        return self._lattice_track_table(getattr(self, "_lattice_track_matches", None))

    @property
    def lattice_track_members(self) -> np.ndarray:
        """With WANT_LATTICE_TRACK: LATTICE_TRACK_MEMBER_DTYPE per slot of word_track_members."""
        return self._lattice_track_table(getattr(self, "_lattice_track_members", None))

    @property
    def lattice_track_src(self) -> np.ndarray:
        """With WANT_LATTICE_TRACK: (slots of word_track_members, 32) uint8, per character of the track's entry the member's part it was
        read from, or 0x80 | the parts before the place it was inserted at; 0xFF behind the entry's end."""
        return self._lattice_track_table(getattr(self, "_lattice_track_src", None))

    @property
    def lattice_track_parts(self) -> np.ndarray:
        """With WANT_LATTICE_TRACK: SPLIT_PART_DTYPE, the members' parts back to back in slot order (piece: an index of run_pieces, or
        -1 for a whole run)."""
        return self._lattice_track_table(getattr(self, "_lattice_track_parts", None))

    def word_track_lattice_text(self, g: int) -> str:
        """With WANT_LATTICE_TRACK: the lexicon entry word track g takes over its members' piece lattices, as it was given to
        set_lexicon; the representative's own reading (word_text) where the track has no entry."""
        e = int(self.lattice_track_matches[g]["entry"])
        return self._lexicon[e] if 0 <= e < len(self._lexicon) else self.word_text(int(self.word_tracks[g]["rep"]))

    def text_track_lattice_match_text(self, k: int) -> str:
        """With WANT_LATTICE_TRACK: the words of the representative line of text track k in order, each as its word track's
        word_track_lattice_text (its own word_text where the line is no reading line), joined by one blank."""
        lw = self.line_words[int(self.text_tracks[k]["rep"])]
        of = self.word_track_of_words
        ws = range(int(lw["first_word"]), int(lw["first_word"]) + int(lw["n_words"]))
        return " ".join(self.word_track_lattice_text(int(of[w])) if of[w] >= 0 else self.word_text(w) for w in ws)

    def track_member_lattice_parts(self, slot: int) -> np.ndarray:
        """With WANT_LATTICE_TRACK: the parts of the member in `slot` of word_track_members for its track's entry (SPLIT_PART_DTYPE;
        none for an unusable member and without an entry)."""
        d = self.lattice_track_members[slot]
        return self.lattice_track_parts[int(d["first_part"]):int(d["first_part"]) + int(d["n_parts"])]

    def _lattice_track_decode_table(self, table):
        if table is None:
            raise ValueError("the result has no lattice track decodes (ERFilter.set_lattice_track_decode(True) and WANT_TRACK_DECODE with WANT_LATTICE_DECODE)")
        return table

    @property
    def lattice_track_decodes(self) -> np.ndarray:
        """With set_lattice_track_decode(True), WANT_TRACK_DECODE and WANT_LATTICE_DECODE: TRACK_DECODE_DTYPE per word track, decoded over
        the members' piece lattices (str_er_lattice_track_decode)."""
        return self._lattice_track_decode_table(getattr(self, "_lattice_track_decodes", None))

    @property
    def lattice_track_decode_chars(self) -> np.ndarray:
        """... (n tracks, 32) uint8, the labels of every track's string, 0xFF past n_chars."""
        return self._lattice_track_decode_table(getattr(self, "_lattice_track_decode_chars", None))

    @property
    def lattice_track_decode_members(self) -> np.ndarray:
        """... LATTICE_TRACK_MEMBER_DTYPE per slot of word_track_members: the member's cost, parts, n_del and n_ins for its track's string."""
        return self._lattice_track_decode_table(getattr(self, "_lattice_track_decode_members", None))

    @property
    def lattice_track_decode_src(self) -> np.ndarray:
        """... (slots of word_track_members, 32) uint8, per character of the track's string the member's part it was read from, or 0x80 |
        the parts before the place it was inserted at; 0xFF behind the string's end."""
        return self._lattice_track_decode_table(getattr(self, "_lattice_track_decode_src", None))

    @property
    def lattice_track_decode_parts(self) -> np.ndarray:
        """... SPLIT_PART_DTYPE, the members' parts back to back in slot order (piece: an index of run_pieces, or -1 for a whole run)."""
        return self._lattice_track_decode_table(getattr(self, "_lattice_track_decode_parts", None))

    def word_track_lattice_decode_text(self, g: int) -> str:
        """The string word track g was decoded to over its members' piece lattices; the representative's own reading (word_text) where
        the track was not decoded."""
        d = self.lattice_track_decodes[g]
        if int(d["cost"]) < 0:
            return self.word_text(int(self.word_tracks[g]["rep"]))
        return "".join(_OCR_ALPHABET[int(a)] for a in self.lattice_track_decode_chars[g, :int(d["n_chars"])])

    def text_track_lattice_decode_text(self, k: int) -> str:
        """The words of the representative line of text track k in order, each as its word track's word_track_lattice_decode_text (its own
        word_text where the line is no reading line), joined by one blank."""
        lw = self.line_words[int(self.text_tracks[k]["rep"])]
        of = self.word_track_of_words
        ws = range(int(lw["first_word"]), int(lw["first_word"]) + int(lw["n_words"]))
        return " ".join(self.word_track_lattice_decode_text(int(of[w])) if of[w] >= 0 else self.word_text(w) for w in ws)

    def track_member_lattice_decode_parts(self, slot: int) -> np.ndarray:
        """The parts of the member in `slot` of word_track_members for its track's decoded string (SPLIT_PART_DTYPE; none for an unusable
        member and an undecoded track): how the consensus string cuts that frame's touching glyphs."""
        d = self.lattice_track_decode_members[slot]
        return self.lattice_track_decode_parts[int(d["first_part"]):int(d["first_part"]) + int(d["n_parts"])]

    def _line_geom_table(self, table):
        if table is None:
            raise ValueError("the result has no line geometry (pass WANT_LINE_GEOM / want_line_geom=True)")
        return table

    @property
    def line_geoms(self) -> np.ndarray:
        """With WANT_LINE_GEOM: LINE_GEOM_DTYPE per line of texts."""
        return self._line_geom_table(self._line_geoms)

    @property
    def frame_line_geoms(self) -> np.ndarray:
        """With WANT_LINE_GEOM: LINE_GEOM_DTYPE per frame line."""
        return self._line_geom_table(self._frame_line_geoms)

    @property
    def geom_points(self) -> np.ndarray:
        """With WANT_LINE_GEOM: the hull vertices both sets of records index, (n_points, 2) int32 x, y."""
        return self._line_geom_table(self._geom_points)

    def line_hull(self, t: int) -> np.ndarray:
        """With WANT_LINE_GEOM: the hull of line t, (n, 2) int32 corners, clockwise on screen from the smallest (y, x)."""
        g = self.line_geoms[t]
        return self.geom_points[int(g["first"]):int(g["first"]) + int(g["count"])].copy()

    def line_quad(self, t: int) -> np.ndarray:
        """With WANT_LINE_GEOM: the oriented box of line t, (4, 2) float64 corners (x, y)."""
        g = self.line_geoms[t]
        return np.stack([g["qx"], g["qy"]], 1).astype(np.float64)

    def frame_line_hull(self, i: int) -> np.ndarray:
        """With WANT_LINE_GEOM: the hull of frame line i, (n, 2) int32."""
        g = self.frame_line_geoms[i]
        return self.geom_points[int(g["first"]):int(g["first"]) + int(g["count"])].copy()

    def frame_line_quad(self, i: int) -> np.ndarray:
        """With WANT_LINE_GEOM: the oriented box of frame line i, (4, 2) float64 corners (x, y)."""
        g = self.frame_line_geoms[i]
        return np.stack([g["qx"], g["qy"]], 1).astype(np.float64)

    def _line_links_table(self, table):
        if table is None:
            raise ValueError("the result has no line links (pass WANT_LINE_LINKS / want_line_links=True)")
        return table

    @property
    def line_links(self) -> np.ndarray:
        """With WANT_LINE_LINKS: LINE_LINK_DTYPE per pair of lines of adjacent frames with common pixels, sorted by (a, b)."""
        return self._line_links_table(self._line_links)

    @property
    def line_tracks(self) -> np.ndarray:
        """With WANT_LINE_LINKS: the index into text_tracks of every line of texts (int32)."""
        return self._line_links_table(self._line_tracks)

    @property
    def text_tracks(self) -> np.ndarray:
        """With WANT_LINE_LINKS: TEXT_TRACK_DTYPE per text track, ordered by first frame, then by smallest member."""
        return self._line_links_table(self._text_tracks)

    @property
    def text_track_members(self) -> np.ndarray:
        """With WANT_LINE_LINKS: the line indices the tracks' first / count index (int32)."""
        return self._line_links_table(self._text_track_members)

    def edge_feet(self, which: int) -> "EdgeFeet":
        """With WANT_LINE_LINKS: the footprints of the lines of the first (which = 0) or of the last frame (1) of the call, as
        ERFilter.link_feet takes them."""
        if which not in (0, 1):
            raise ValueError("which is 0 (the first frame) or 1 (the last frame)")
        return self._line_links_table(self._edge_feet)[which]

    def _frame_lines_table(self, table):
        if table is None:
            raise ValueError("the result has no frame lines (pass WANT_FRAME_LINES / want_frame_lines=True)")
        return table

    @property
    def line_feet(self) -> np.ndarray:
        """With WANT_FRAME_LINES: LINE_FOOT_DTYPE per line of texts."""
        return self._frame_lines_table(self._line_feet)

    @property
    def line_pairs(self) -> np.ndarray:
        """With WANT_FRAME_LINES: LINE_PAIR_DTYPE per pair of lines of one frame with common pixels, sorted by (a, b)."""
        return self._frame_lines_table(self._line_pairs)

    @property
    def frame_lines(self) -> np.ndarray:
        """With WANT_FRAME_LINES: FRAME_LINE_DTYPE per frame line, ordered by frame, then by smallest member."""
        return self._frame_lines_table(self._frame_lines)

    @property
    def frame_line_members(self) -> np.ndarray:
        """With WANT_FRAME_LINES: the line indices the frame lines' first / count index (int32)."""
        return self._frame_lines_table(self._frame_line_members)

    @property
    def mask_pixels(self) -> Optional[np.ndarray]:
        """With WANT_MASKS: the pixel count of every candidate's mask."""
        return None if self.masks is None else self.masks["pixels"]

    def mask(self, i: int) -> np.ndarray:
        """With WANT_MASKS: the mask of candidate i as a bool array (h, w) over its box."""
        if self.masks is None:
            raise ValueError("the result has no masks (pass WANT_MASKS / want_masks=True)")
        c = self.cands[i]
        return unpack_mask(self.mask_bits, int(self.masks[i]["word_off"]), int(c["w"]), int(c["h"]))

    def _crop_of(self, pixels, t: int) -> np.ndarray:
        if self.line_crops is None:
            raise ValueError("the result has no line crops (pass WANT_LINE_CROPS / want_line_crops=True)")
        g = self.line_crops[t]
        o, w, h = int(g["pix_off"]), int(g["width"]), int(g["height"])
        return pixels[o:o + w * h].reshape(h, w)

    def line_crop(self, t: int) -> np.ndarray:
        """With WANT_LINE_CROPS: the grey crop of line t as a (height, width) uint8 array."""
        return self._crop_of(self.line_crop_pixels, t)

    def line_glyph(self, t: int) -> np.ndarray:
        """With WANT_LINE_GLYPHS: the glyph crop of line t (255 on the member masks, else 0) as a (height, width) uint8 array."""
        if self.line_crops is not None and self.line_glyph_pixels is None:
            raise ValueError("the result has no glyph crops (pass WANT_LINE_GLYPHS / want_line_crops=\"glyphs\")")
        return self._crop_of(self.line_glyph_pixels, t)

    def _map_of(self, flat, f: int, flag: str) -> np.ndarray:
        if flat is None:
            raise ValueError(f"the result has no {flag.lower()[5:]} (pass {flag} / want_{flag.lower()[5:]}=True)")
        g = self.frame_maps[f]
        o, w, h = int(g["off"]), int(g["width"]), int(g["height"])
        return flat[o:o + w * h].reshape(h, w)

    def text_map(self, f: int) -> np.ndarray:
        """With WANT_TEXT_MAP: the text map of frame f as an (H, W) uint8 array of TEXT_MAP_* bits."""
        return self._map_of(self.text_map_pixels, f, "WANT_TEXT_MAP")

    def line_map(self, f: int) -> np.ndarray:
        """With WANT_LINE_MAP: the line-id map of frame f as an (H, W) int32 array (index into texts, -1 for no line)."""
        return self._map_of(self.line_map_ids, f, "WANT_LINE_MAP")

    def line_crop_batch(self, glyphs: bool = False):
        """With WANT_LINE_CROPS: every line's crop (or glyph crop) in one (n, height, max width) uint8 array, zero-padded on the
        right, and the widths (n,) -- the input of a recogniser that takes a batch."""
        if self.line_crops is None:
            raise ValueError("the result has no line crops (pass WANT_LINE_CROPS / want_line_crops=True)")
        n = len(self.line_crops)
        widths = self.line_crops["width"].astype(np.int32)
        h = int(self.line_crops["height"][0]) if n else 0
        out = np.zeros((n, h, int(widths.max()) if n else 0), np.uint8)
        for t in range(n):
            out[t, :, :widths[t]] = self.line_glyph(t) if glyphs else self.line_crop(t)
        return out, widths

    @property
    def planes(self) -> List[PlaneResult]:
        if self._planes is None:
            out, off = [], 0
            for i, pi in enumerate(self.info):
                n = int(pi["n_pool"])
                out.append(PlaneResult(int(pi["frame"]), int(pi["ch"]), int(pi["pyr"]), int(pi["width"]), int(pi["height"]),
                                       int(pi["n_created"]), int(pi["n_kept"]), n, int(pi["n_strong"]), int(pi["n_weak"]),
                                       int(pi["ambiguous"]), int(pi["root"]), self.cands[off:off + n],
                                       self._nodes[i] if self._nodes is not None else None))
                off += n
            self._planes = out
        return self._planes


def _np_ptr(a: np.ndarray) -> int:
    return a.ctypes.data


class ERFilter:
    """Drop-in for the hot-path surface of the reference's ERFilter (inc/ER.h:110-136)."""

    def __init__(self, thresh_step: int = 2, min_area: int = 100, max_area: int = 100000, stability_t: int = 2,
                 overlap_coef: float = 0.7, min_ocr_prob: float = 0.01, *, params: Optional[Params] = None, **cap):
        # positional defaults are the reference's (inc/ER.h:113); src/main.cpp:22 passes 8,120,900000,2,0.7,0.15
        self.L = load_library()
        p = params or Params(thresh_step=thresh_step, min_area=min_area, max_area=max_area, stability_t=stability_t,
                             overlap_coef=overlap_coef, **cap)
        self.params = p
        self.min_ocr_prob = min_ocr_prob
        cp = _Params(p.thresh_step, p.min_area, p.max_area, p.stability_t, p.overlap_coef, p.n_pyr_levels,
                     p.channel_mask, p.device, p.max_width, p.max_height, p.max_frames, p.kept_cap, p.pool_cap,
                     p.sibling_order, p.stream)
        h = C.c_void_p()
        rc = self.L.str_er_create(C.byref(cp), C.byref(h))
        if rc != 0:
            raise StrErError(rc, (self.L.str_er_last_error(None) or b"").decode())
        self.h = h
        self.stc = None  # names of the reference's public members (inc/ER.h:117-118)
        self.wtc = None

    # ---- lifetime -------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "h", None):
            self.L.str_er_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise StrErError(rc, (self.L.str_er_last_error(self.h) or b"").decode())

    # ---- models: stc / wtc = new CascadeBoost(file)  (src/main.cpp:23-24) ------------------
    def load_cascade(self, which: int, path: str) -> None:
        self._check(self.L.str_er_load_cascade(self.h, which, path.encode()))
        if which == 0:
            self.stc = path
        else:
            self.wtc = path

    def load_cascade_text(self, which: int, text: str) -> None:
        b = text.encode()
        self._check(self.L.str_er_load_cascade_mem(self.h, which, b, len(b)))

    def cascade_info(self, which: int):
        a, b = C.c_int32(), C.c_int32()
        self._check(self.L.str_er_cascade_info(self.h, which, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_thresh_step(self, t: int) -> None:      # src/ER.cpp:21-24
        self._check(self.L.str_er_set_thresh_step(self.h, t))
        self.params.thresh_step = t

    def set_min_area(self, m: int) -> None:         # src/ER.cpp:27-30
        self._check(self.L.str_er_set_min_area(self.h, m))
        self.params.min_area = m

    # ---- results ------------------------------------------------------------------------------
    def _collect(self, rh: C.c_void_p, profile: Optional[dict] = None) -> Result:
        L = self.L

        n32, n64 = C.c_int32(), C.c_uint64()        # (the counts: a table's length, a byte / word array's)

        def table(fn, dtype, n=n32):                 # a table a stage makes: None when the stage did not run
            ptr = fn(rh, C.byref(n))
            return _owned(ptr, n.value, dtype) if ptr else None

        try:
            n = C.c_int32()
            cands = _owned(L.str_er_result_cands(rh, C.byref(n)), n.value, CAND_DTYPE)
            info = _owned(L.str_er_result_plane_infos(rh, C.byref(n)), n.value, PLANE_DTYPE)
            nodes = None
            nn = C.c_int32()
            if n.value and L.str_er_result_plane_nodes(rh, 0, C.byref(nn)):
                nodes = []
                for i in range(n.value):
                    nptr = L.str_er_result_plane_nodes(rh, i, C.byref(nn))
                    nodes.append(_owned(nptr, nn.value, NODE_DTYPE))
            t = L.str_er_result_times(rh)
            times = np.array([t[i] for i in range(7)])
            res = Result(info, cands, times, self.last_profile() if profile is None else profile, nodes)
            # (a table that comes with another is asked for only when that one is there: one call less per absent table on the latency path)
            res.ocr_label = table(L.str_er_result_ocr_labels, np.int32)
            if res.ocr_label is not None:
                res.ocr_prob = table(L.str_er_result_ocr_probs, np.float64)
            res.tracks = table(L.str_er_result_tracks, TRACK_DTYPE)
            res.texts = table(L.str_er_result_texts, TEXT_DTYPE)
            if res.texts is not None:
                res.text_ers = table(L.str_er_result_text_ers, np.int32)
                res.group_all = table(L.str_er_result_group_all, np.int32)
                res.group_bounds = table(L.str_er_result_group_bounds, GBOUND_DTYPE)
            res.line_crops = table(L.str_er_result_line_crops, LINE_CROP_DTYPE)
            if res.line_crops is not None:
                res.line_crop_pixels = table(L.str_er_result_line_crop_pixels, np.uint8, n64)
                res.line_glyph_pixels = table(L.str_er_result_line_glyph_pixels, np.uint8, n64)
            res.frame_maps = table(L.str_er_result_frame_maps, FRAME_MAP_DTYPE)
            if res.frame_maps is not None:
                res.text_map_pixels = table(L.str_er_result_text_map_pixels, np.uint8, n64)
                res.line_map_ids = table(L.str_er_result_line_map_ids, np.int32, n64)
            if res.texts is not None:
                res._line_feet = table(L.str_er_result_line_feet, LINE_FOOT_DTYPE)
                if res._line_feet is not None:
                    res._line_pairs = table(L.str_er_result_line_pairs, LINE_PAIR_DTYPE)
                    res._frame_lines = table(L.str_er_result_frame_lines, FRAME_LINE_DTYPE)
                    res._frame_line_members = table(L.str_er_result_frame_line_members, np.int32)
                    res._line_geoms = table(L.str_er_result_line_geoms, LINE_GEOM_DTYPE)
                    if res._line_geoms is not None:
                        res._frame_line_geoms = table(L.str_er_result_frame_line_geoms, LINE_GEOM_DTYPE)
                        npts = C.c_int32()
                        ptr = L.str_er_result_geom_points(rh, C.byref(npts))
                        res._geom_points = _owned(ptr, 2 * npts.value, np.int32).reshape(-1, 2)
                    res._line_words = table(L.str_er_result_line_words, LINE_WORDS_DTYPE)
                    if res._line_words is not None:
                        res._line_runs = table(L.str_er_result_line_runs, LINE_RUN_DTYPE)
                        res._words = table(L.str_er_result_words, LINE_WORD_DTYPE)
                        res._run_reads = table(L.str_er_result_run_reads, RUN_READ_DTYPE)
                        if res._run_reads is not None:
                            res._run_features = table(L.str_er_result_run_features, np.uint8, n64).reshape(-1, 1800)
                            res._word_matches = table(L.str_er_result_word_matches, WORD_MATCH_DTYPE)
                            res._word_decodes = table(L.str_er_result_word_decodes, WORD_DECODE_DTYPE)
                            if res._word_decodes is not None:
                                res._word_decode_chars = table(L.str_er_result_word_decode_chars, np.uint8, n64).reshape(-1, 64)
                                res._word_decode_src = table(L.str_er_result_word_decode_src, np.uint8, n64).reshape(-1, 64)
                                res._word_margins = table(L.str_er_result_word_margins, WORD_MARGIN_DTYPE)
                                if res._word_margins is not None:
                                    res._word_row_margins = table(L.str_er_result_word_row_margins, np.uint8, n64).view(np.int32).reshape(-1, 32)
                                    res._word_row_reads = table(L.str_er_result_word_row_reads, np.uint8, n64).reshape(-1, 32)
                                    res._word_row_alts = table(L.str_er_result_word_row_alts, np.uint8, n64).reshape(-1, 32)
                                res._line_decodes = table(L.str_er_result_line_decodes, LINE_DECODE_DTYPE)
                                if res._line_decodes is not None:
                                    res._line_decode_chars = table(L.str_er_result_line_decode_chars, np.uint8, n64)
                                    res._line_decode_src = table(L.str_er_result_line_decode_src, np.uint16, n64)
                                    res._line_decode_word_of_row = table(L.str_er_result_line_decode_word_of_row, np.int32, n64)
                                    res._line_gap_costs = table(L.str_er_result_line_gap_costs, np.uint8, n64).reshape(-1, 2)
                                    res._line_decode_windows = table(L.str_er_result_line_decode_windows, np.int32, n64).reshape(-1, 2)
                                    res._line_margins = table(L.str_er_result_line_margins, LINE_MARGIN_DTYPE)
                                    if res._line_margins is not None:
                                        res._line_row_margins = table(L.str_er_result_line_row_margins, np.uint8, n64).view(np.int32)
                                        res._line_row_reads = table(L.str_er_result_line_row_reads, np.uint8, n64)
                                        res._line_row_alts = table(L.str_er_result_line_row_alts, np.uint8, n64)
                                        res._line_gap_margins = table(L.str_er_result_line_gap_margins, np.uint8, n64).view(np.int32)
                                        res._line_gap_moves = table(L.str_er_result_line_gap_moves, np.uint8, n64)
                            res._run_splits = table(L.str_er_result_run_splits, RUN_SPLIT_DTYPE)
                            if res._run_splits is not None:
                                res._run_pieces = table(L.str_er_result_run_pieces, RUN_PIECE_DTYPE)
                                res._piece_reads = table(L.str_er_result_piece_reads, RUN_READ_DTYPE)
                                res._piece_costs = table(L.str_er_result_piece_costs, np.uint8, n64).reshape(-1, 65)
                                res._split_parts = table(L.str_er_result_split_parts, SPLIT_PART_DTYPE)
                                res._word_splits = table(L.str_er_result_word_splits, WORD_SPLIT_DTYPE)
                                res._run_costs = table(L.str_er_result_run_costs, np.uint8, n64).reshape(len(res._run_reads), 65)
                                res._lattice_decodes = table(L.str_er_result_lattice_decodes, LATTICE_DECODE_DTYPE)
                                if res._lattice_decodes is not None:
                                    res._lattice_decode_chars = table(L.str_er_result_lattice_decode_chars, np.uint8, n64).reshape(-1, 64)
                                    res._lattice_decode_src = table(L.str_er_result_lattice_decode_src, np.uint8, n64).reshape(-1, 64)
                                    res._lattice_parts = table(L.str_er_result_lattice_parts, SPLIT_PART_DTYPE)
                                    res._line_lattice_decodes = table(L.str_er_result_line_lattice_decodes, LINE_LATTICE_DECODE_DTYPE)
                                    if res._line_lattice_decodes is not None:
                                        res._line_lattice_chars = table(L.str_er_result_line_lattice_chars, np.uint8, n64)
                                        res._line_lattice_src = table(L.str_er_result_line_lattice_src, np.uint16, n64)
                                        res._line_lattice_parts = table(L.str_er_result_line_lattice_parts, SPLIT_PART_DTYPE)
                                        res._line_lattice_word_of_part = table(L.str_er_result_line_lattice_word_of_part, np.int32, n64)
                                        res._line_lattice_gap_costs = table(L.str_er_result_line_lattice_gap_costs, np.uint8, n64).reshape(-1, 2)
                                        res._line_lattice_windows = table(L.str_er_result_line_lattice_windows, np.int32, n64).reshape(-1, 2)
                                    res._lattice_margins = table(L.str_er_result_lattice_margins, LATTICE_MARGIN_DTYPE)
                                    if res._lattice_margins is not None:
                                        res._lattice_read_margins = table(L.str_er_result_lattice_read_margins, np.uint8, n64).view(np.int32).reshape(-1, 32)
                                        res._lattice_cut_margins = table(L.str_er_result_lattice_cut_margins, np.uint8, n64).view(np.int32).reshape(-1, 32)
                                        res._lattice_part_reads = table(L.str_er_result_lattice_part_reads, np.uint8, n64).reshape(-1, 32)
                                        res._lattice_part_alts = table(L.str_er_result_lattice_part_alts, np.uint8, n64).reshape(-1, 32)
                                        res._lattice_cut_alts = table(L.str_er_result_lattice_cut_alts, np.uint8, n64).reshape(-1, 32)
                                res._lattice_matches = table(L.str_er_result_lattice_matches, LATTICE_MATCH_DTYPE)
                                if res._lattice_matches is not None:
                                    res._lattice_match_src = table(L.str_er_result_lattice_match_src, np.uint8, n64).reshape(-1, 32)
                                    res._lattice_match_parts = table(L.str_er_result_lattice_match_parts, SPLIT_PART_DTYPE)
                            if res._word_matches is not None or res._word_decodes is not None:
                                nr = len(res._run_reads)
                                res._run_costs = table(L.str_er_result_run_costs, np.uint8, n64).reshape(nr, 65)
                                pr = table(L.str_er_result_run_probs, np.float64, n64)
                                res._run_probs = pr.reshape(nr, len(pr) // nr if nr else 0)
                                res._lexicon = tuple(getattr(self, "_lexicon", ()))
                    res._line_links = table(L.str_er_result_line_links, LINE_LINK_DTYPE)
                    if res._line_links is not None:
                        res._line_tracks = table(L.str_er_result_line_tracks, np.int32)
                        res._text_tracks = table(L.str_er_result_text_tracks, TEXT_TRACK_DTYPE)
                        res._text_track_members = table(L.str_er_result_text_track_members, np.int32)
                        res._edge_feet = [self._edge_feet_of(rh, which) for which in (0, 1)]
                        res._word_links = table(L.str_er_result_word_links, WORD_LINK_DTYPE)
                        if res._word_links is not None:
                            res._word_tracks = table(L.str_er_result_word_tracks, WORD_TRACK_DTYPE)
                            res._word_track_members = table(L.str_er_result_word_track_members, np.int32)
                            res._word_track_of_words = table(L.str_er_result_word_track_of_words, np.int32)
                            res._track_matches = table(L.str_er_result_track_matches, TRACK_MATCH_DTYPE)
                            res._track_member_costs = table(L.str_er_result_track_member_costs, np.int32)
                            res._track_decodes = table(L.str_er_result_track_decodes, TRACK_DECODE_DTYPE)
                            if res._track_decodes is not None:
                                res._track_decode_chars = table(L.str_er_result_track_decode_chars, np.uint8, n64).reshape(-1, 32)
                                res._track_decode_member_costs = table(L.str_er_result_track_decode_member_costs, np.int32)
                            res._lattice_track_matches = table(L.str_er_result_lattice_track_matches, TRACK_MATCH_DTYPE)
                            if res._lattice_track_matches is not None:
                                res._lattice_track_members = table(L.str_er_result_lattice_track_members, LATTICE_TRACK_MEMBER_DTYPE)
                                res._lattice_track_src = table(L.str_er_result_lattice_track_src, np.uint8, n64).reshape(-1, 32)
                                res._lattice_track_parts = table(L.str_er_result_lattice_track_parts, SPLIT_PART_DTYPE)
                            res._lattice_track_decodes = table(L.str_er_result_lattice_track_decodes, TRACK_DECODE_DTYPE)
                            if res._lattice_track_decodes is not None:
                                res._lattice_track_decode_chars = table(L.str_er_result_lattice_track_decode_chars, np.uint8, n64).reshape(-1, 32)
                                res._lattice_track_decode_members = table(L.str_er_result_lattice_track_decode_members, LATTICE_TRACK_MEMBER_DTYPE)
                                res._lattice_track_decode_src = table(L.str_er_result_lattice_track_decode_src, np.uint8, n64).reshape(-1, 32)
                                res._lattice_track_decode_parts = table(L.str_er_result_lattice_track_decode_parts, SPLIT_PART_DTYPE)
            res.masks = table(L.str_er_result_masks, MASK_DTYPE)
            if res.masks is not None:
                res.mask_bits = table(L.str_er_result_mask_bits, np.uint32, n64)
            res.shapes = table(L.str_er_result_shapes, SHAPE_DTYPE)
            res.strokes = table(L.str_er_result_strokes, STROKE_DTYPE)
            res.line_label = table(L.str_er_result_line_labels, np.int32)
            if res.line_label is not None:
                res.line_prob = table(L.str_er_result_line_probs, np.float64)
                res.line_kept = table(L.str_er_result_line_kept, np.uint8).astype(bool)
                res.text_alive = table(L.str_er_result_text_alive, np.uint8).astype(bool)
            return res
        finally:
            L.str_er_result_free(rh)

    def _edge_feet_of(self, rh, which: int) -> "EdgeFeet":
        w, h, n, nw = C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint64()
        feet, lines, bits = C.c_void_p(), C.c_void_p(), C.c_void_p()
        rc = self.L.str_er_result_edge_feet(rh, which, C.byref(w), C.byref(h), C.byref(feet), C.byref(lines), C.byref(n), C.byref(bits), C.byref(nw))
        if rc != 0:
            raise StrErError(rc, "str_er_result_edge_feet")
        return EdgeFeet(w.value, h.value, _owned(lines.value, n.value, np.int32), _owned(feet.value, n.value, LINE_FOOT_DTYPE),
                        _owned(bits.value, nw.value, np.uint32))

    def last_tree_stats(self) -> dict:
        """Node records / border pixel pairs / tiles of the last detect call (str_er_last_tree_stats)."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.L.str_er_last_tree_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"records": int(a.value), "seam_pairs": int(b.value), "tiles": int(c.value)}

    def last_group_stats(self) -> dict:
        """Where the groups of tiles of the last detect call went: groups per k_group_merge table (512 / 1024 / 2048 / 2528 records; a large text-like
        batch only), groups listed for k_seam_undone, groups of one tile (str_er_last_group_stats)."""
        t, a, b = (C.c_uint32 * 4)(), C.c_uint32(), C.c_uint32()
        self._check(self.L.str_er_last_group_stats(self.h, t, C.byref(a), C.byref(b)))
        return {"per_table": {cap: int(v) for cap, v in zip((512, 1024, 2048, 2528), t)}, "listed": int(a.value), "one_tile": int(b.value)}

    def tile2_stats(self) -> dict:
        """Tiles given to the second tile kernel (k_tile_tree2) since the context was created, and how many it handed back (str_er_tile2_stats)."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self.L.str_er_tile2_stats(self.h, C.byref(a), C.byref(b)))
        return {"tiles": int(a.value), "handed_back": int(b.value)}

    def set_profiling(self, on: bool = True) -> None:
        """Per-kernel-group HIP events for the calls that follow (Result.profile / last_profile()); off by default: an event between two kernels costs
        stream time (str_er_set_profiling)."""
        self._check(self.L.str_er_set_profiling(self.h, 1 if on else 0))

    def ocr_stage_stats(self) -> dict:
        """Batches whose STAGE_OCR scores were computed right behind classify (sized from the previous batch), and batches scored again after the
        counters were read (str_er_ocr_stage_stats)."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self.L.str_er_ocr_stage_stats(self.h, C.byref(a), C.byref(b)))
        return {"scored_early": int(a.value), "scored_again": int(b.value)}

    def last_profile(self) -> dict:
        names = (C.c_char_p * 32)()
        ms = (C.c_double * 32)()
        k = self.L.str_er_last_profile(self.h, names, ms, 32)
        return {names[i].decode(): ms[i] for i in range(min(k, 32))}

    # ---- the hot path ---------------------------------------------------------------------------
    def text_detect(self, src: np.ndarray, stages: int = STAGE_ALL, want_nodes: bool = False, want_masks: bool = False,
                    want_line_crops=False, want_shapes: bool = False, want_text_map: bool = False, want_line_map: bool = False,
                    want_strokes: bool = False, want_frame_lines: bool = False,
                    want_line_links: bool = False, want_line_geom: bool = False, want_line_words: bool = False,
                    want_run_read: bool = False, want_word_match: bool = False, want_word_decode: bool = False, want_run_split: bool = False, want_track_read: bool = False, want_lattice_decode: bool = False, want_lattice_match: bool = False, want_lattice_track: bool = False, want_track_decode: bool = False) -> Result:
        """ERFilter::text_detect up to classify (src/ER.cpp:33-60) for one BGR frame (H,W,3)
        or a batch (F,H,W,3) of uint8."""
        a = np.ascontiguousarray(src, dtype=np.uint8)
        if a.ndim == 3:
            a = a[None]
        if a.ndim != 4 or a.shape[3] != 3:
            raise ValueError("expected (H,W,3) or (F,H,W,3) uint8 BGR")
        f, h, w, _ = a.shape
        rh = C.c_void_p()
        self._check(self.L.str_er_detect_bgr(self.h, _np_ptr(a), w, h, 3 * w, 3 * w * h, f, MEM_HOST,
                                             stages | _want_flags(nodes=want_nodes, masks=want_masks, line_crops=want_line_crops, shapes=want_shapes,
                                                                  text_map=want_text_map, line_map=want_line_map, strokes=want_strokes, frame_lines=want_frame_lines,
                                                                  line_links=want_line_links, line_geom=want_line_geom, line_words=want_line_words, run_read=want_run_read, word_match=want_word_match, word_decode=want_word_decode, run_split=want_run_split, track_read=want_track_read, lattice_decode=want_lattice_decode, lattice_match=want_lattice_match, lattice_track=want_lattice_track, track_decode=want_track_decode), C.byref(rh)))
        return self._collect(rh)

    def text_detect_nv12(self, nv12: np.ndarray, w: int, h: int, stages: int = STAGE_ALL, want_nodes: bool = False) -> Result:
        """str_er_detect_nv12: frames as a video decoder delivers them, (h * 3 // 2, w) or (F, h * 3 // 2, w) uint8 (luma plane,
        then interleaved Cb/Cr at half resolution); the NV12 -> Y/Cr/Cb step is build-defined (include/str_er.h)."""
        a = np.ascontiguousarray(nv12, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        f = a.shape[0]
        assert a.shape[1:] == (h + h // 2, w), a.shape
        rh = C.c_void_p()
        self._check(self.L.str_er_detect_nv12(self.h, _np_ptr(a), w, h, w, w * (h + h // 2), f, MEM_HOST,
                                              stages | (WANT_NODES if want_nodes else 0), C.byref(rh)))
        return self._collect(rh)

    def text_detect_planes(self, src: np.ndarray, select, stages: int = STAGE_ALL, want_nodes: bool = False) -> Result:
        """text_detect for a subset of the logical planes (str_er_detect_bgr_planes): select[level * n_channels + k] flags."""
        a = np.ascontiguousarray(src, dtype=np.uint8)
        if a.ndim == 3:
            a = a[None]
        f, h, w, _ = a.shape
        sel = np.ascontiguousarray(select, dtype=np.uint8)
        rh = C.c_void_p()
        self._check(self.L.str_er_detect_bgr_planes(self.h, _np_ptr(a), w, h, 3 * w, 3 * w * h, f, MEM_HOST,
                                                    stages | (WANT_NODES if want_nodes else 0), _np_ptr(sel), len(sel), C.byref(rh)))
        return self._collect(rh)

    # ---- the level-0 planes of one frame in strips over several GPUs ---------------------------
    def strip_extract(self, frame: np.ndarray, strip: int, n_strips: int) -> bytes:
        """Tile trees of strip `strip` of `n_strips` of every channel's level-0 plane: the bytes to send to the plane's owner."""
        a = np.ascontiguousarray(frame, dtype=np.uint8)
        h, w, _ = a.shape
        p, n = C.c_void_p(), C.c_int64()
        self._check(self.L.str_er_strip_extract(self.h, _np_ptr(a), w, h, 3 * w, MEM_HOST, strip, n_strips, C.byref(p), C.byref(n)))
        try:
            return C.string_at(p.value, n.value)
        finally:
            self.L.str_er_strip_free(p)

    def strip_merge(self, frame: np.ndarray, blobs, stages: int = STAGE_ALL, want_nodes: bool = False) -> Result:
        """The owner's half: all strips' blobs (in strip order) -> the result text_detect gives for the frame."""
        a = np.ascontiguousarray(frame, dtype=np.uint8)
        h, w, _ = a.shape
        k = len(blobs)
        bufs = [C.create_string_buffer(bytes(x), len(x)) for x in blobs]
        ptrs = (C.c_void_p * k)(*[C.cast(x, C.c_void_p) for x in bufs])
        sizes = (C.c_int64 * k)(*[len(x) for x in blobs])
        rh = C.c_void_p()
        self._check(self.L.str_er_strip_merge(self.h, _np_ptr(a), w, h, 3 * w, MEM_HOST, ptrs, sizes, k,
                                              stages | (WANT_NODES if want_nodes else 0), C.byref(rh)))
        return self._collect(rh)

    def strip_extract_dev(self, frame: np.ndarray, strip: int, n_strips: int):
        """The same, the blob left in a device buffer of this context (valid until its next strip call): (device address, bytes)."""
        a = np.ascontiguousarray(frame, dtype=np.uint8)
        h, w, _ = a.shape
        p, n = C.c_void_p(), C.c_int64()
        self._check(self.L.str_er_strip_extract_dev(self.h, _np_ptr(a), w, h, 3 * w, MEM_HOST, strip, n_strips, C.byref(p), C.byref(n)))
        return int(p.value), int(n.value)

    def strip_merge_ex(self, frame: np.ndarray, blobs, sizes=None, device_blobs: bool = False, plane_select=None, stages: int = STAGE_ALL,
                       want_nodes: bool = False) -> Result:
        """str_er_strip_merge_ex: blobs = bytes objects (host) or device addresses with `sizes` (device_blobs=True); plane_select =
        one flag per channel of the context: the channels this owner puts together (None: all)."""
        a = np.ascontiguousarray(frame, dtype=np.uint8)
        h, w, _ = a.shape
        k = len(blobs)
        if device_blobs:
            ptrs = (C.c_void_p * k)(*[C.c_void_p(int(x)) for x in blobs])
            szs = (C.c_int64 * k)(*[int(x) for x in sizes])
        else:
            bufs = [C.create_string_buffer(bytes(x), len(x)) for x in blobs]
            ptrs = (C.c_void_p * k)(*[C.cast(x, C.c_void_p) for x in bufs])
            szs = (C.c_int64 * k)(*[len(x) for x in blobs])
        sel = np.ascontiguousarray(plane_select, dtype=np.uint8) if plane_select is not None else None
        rh = C.c_void_p()
        self._check(self.L.str_er_strip_merge_ex(self.h, _np_ptr(a), w, h, 3 * w, MEM_HOST, ptrs, szs, MEM_DEVICE if device_blobs else MEM_HOST, k,
                                                 _np_ptr(sel) if sel is not None else None, stages | (WANT_NODES if want_nodes else 0), C.byref(rh)))
        return self._collect(rh)

    def detect_bgr_device(self, dptr: int, w: int, h: int, n_frames: int, stages: int = STAGE_ALL,
                          stride: Optional[int] = None, frame_pitch: Optional[int] = None) -> Result:
        """Same, for frames already resident in HBM (dptr = device address)."""
        stride = stride or 3 * w
        frame_pitch = frame_pitch or stride * h
        rh = C.c_void_p()
        self._check(self.L.str_er_detect_bgr(self.h, dptr, w, h, stride, frame_pitch, n_frames, MEM_DEVICE, stages,
                                             C.byref(rh)))
        return self._collect(rh)

    def detect_planes(self, planes: np.ndarray, stages: int = STAGE_ALL, want_nodes: bool = False) -> Result:
        """The loop body at src/ER.cpp:52-59 for (H,W) or (N,H,W) uint8 planes."""
        a = np.ascontiguousarray(planes, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        n, h, w = a.shape
        rh = C.c_void_p()
        self._check(self.L.str_er_detect_planes(self.h, _np_ptr(a), w, h, w, w * h, n, MEM_HOST,
                                                stages | (WANT_NODES if want_nodes else 0), C.byref(rh)))
        return self._collect(rh)

    def detect_planes_device(self, dptr: int, w: int, h: int, n_planes: int, stages: int = STAGE_ALL,
                             stride: Optional[int] = None, plane_pitch: Optional[int] = None) -> Result:
        stride = stride or w
        plane_pitch = plane_pitch or stride * h
        rh = C.c_void_p()
        self._check(self.L.str_er_detect_planes(self.h, dptr, w, h, stride, plane_pitch, n_planes, MEM_DEVICE, stages,
                                                C.byref(rh)))
        return self._collect(rh)

    # ---- lists of frames of different sizes -------------------------------------------------------
    def _detect_list(self, fn, refs, mem_kind: int, stages: int) -> Result:
        arr = (ImageRef * len(refs))(*refs)
        rh = C.c_void_p()
        self._check(fn(self.h, arr, len(refs), mem_kind, stages, C.byref(rh)))
        return self._collect(rh)

    def text_detect_list(self, frames, stages: int = STAGE_ALL, want_nodes: bool = False, want_masks: bool = False,
                         want_line_crops=False, want_shapes: bool = False, want_text_map: bool = False, want_line_map: bool = False,
                         want_strokes: bool = False, want_frame_lines: bool = False,
                         want_line_links: bool = False, want_line_geom: bool = False, want_line_words: bool = False,
                    want_run_read: bool = False, want_word_match: bool = False, want_word_decode: bool = False, want_run_split: bool = False, want_track_read: bool = False, want_lattice_decode: bool = False, want_lattice_match: bool = False, want_lattice_track: bool = False, want_track_decode: bool = False) -> Result:
        """text_detect for a sequence of (H,W,3) uint8 BGR frames of any sizes (each within the capacity) in one call.  Frame i's
        planes and candidates are those text_detect gives for it alone, with frame = i.  Views with a row stride are not copied."""
        keep = [_row_view(f, 3) for f in frames]
        refs = [ImageRef(_np_ptr(a), a.shape[1], a.shape[0], a.strides[0]) for a in keep]
        return self._detect_list(self.L.str_er_detect_bgr_list, refs, MEM_HOST,
                                 stages | _want_flags(nodes=want_nodes, masks=want_masks, line_crops=want_line_crops, shapes=want_shapes,
                                                      text_map=want_text_map, line_map=want_line_map, strokes=want_strokes, frame_lines=want_frame_lines,
                                                                  line_links=want_line_links, line_geom=want_line_geom, line_words=want_line_words, run_read=want_run_read, word_match=want_word_match, word_decode=want_word_decode, run_split=want_run_split, track_read=want_track_read, lattice_decode=want_lattice_decode, lattice_match=want_lattice_match, lattice_track=want_lattice_track, track_decode=want_track_decode))

    def detect_planes_list(self, planes, stages: int = STAGE_ALL, want_nodes: bool = False) -> Result:
        """detect_planes for a sequence of (H,W) uint8 planes of any sizes in one call: plane i gets ch = i & 255."""
        keep = [_row_view(p, 1) for p in planes]
        refs = [ImageRef(_np_ptr(a), a.shape[1], a.shape[0], a.strides[0]) for a in keep]
        return self._detect_list(self.L.str_er_detect_planes_list, refs, MEM_HOST, stages | (WANT_NODES if want_nodes else 0))

    def detect_bgr_list_device(self, ptrs_dims, stages: int = STAGE_ALL, want_nodes: bool = False) -> Result:
        """text_detect_list for frames resident in HBM: ptrs_dims = [(device address, w, h[, stride]), ...] (stride default 3 w)."""
        refs = [ImageRef(int(t[0]), int(t[1]), int(t[2]), int(t[3]) if len(t) > 3 else 3 * int(t[1])) for t in ptrs_dims]
        return self._detect_list(self.L.str_er_detect_bgr_list, refs, MEM_DEVICE, stages | (WANT_NODES if want_nodes else 0))

    def text_detect_nv12_list(self, frames, stages: int = STAGE_ALL, want_nodes: bool = False) -> Result:
        """text_detect_nv12 for a sequence of NV12 frames of any (even) sizes in one call: each a (h + h/2, w) uint8 array (luma rows,
        then interleaved Cb/Cr rows) or a view of one with a row stride (not copied).  Frame i's result is text_detect_nv12's on it alone."""
        keep = [_row_view(f, 1) for f in frames]
        refs = []
        for a in keep:
            if a.shape[0] % 3:
                raise ValueError("an NV12 frame has h + h/2 rows (h even)")
            refs.append(ImageRef(_np_ptr(a), a.shape[1], a.shape[0] // 3 * 2, a.strides[0]))
        return self._detect_list(self.L.str_er_detect_nv12_list, refs, MEM_HOST, stages | (WANT_NODES if want_nodes else 0))

    def detect_nv12_list_device(self, ptrs_dims, stages: int = STAGE_ALL, want_nodes: bool = False) -> Result:
        """text_detect_nv12_list for frames resident in HBM: ptrs_dims = [(device address of the luma plane, w, h[, stride]), ...]
        (stride default w; chroma h rows after the luma plane)."""
        refs = [ImageRef(int(t[0]), int(t[1]), int(t[2]), int(t[3]) if len(t) > 3 else int(t[1])) for t in ptrs_dims]
        return self._detect_list(self.L.str_er_detect_nv12_list, refs, MEM_DEVICE, stages | (WANT_NODES if want_nodes else 0))

    def detect_planes_list_device(self, ptrs_dims, stages: int = STAGE_ALL, want_nodes: bool = False) -> Result:
        """detect_planes_list for planes resident in HBM: ptrs_dims = [(device address, w, h[, stride]), ...] (stride default w)."""
        refs = [ImageRef(int(t[0]), int(t[1]), int(t[2]), int(t[3]) if len(t) > 3 else int(t[1])) for t in ptrs_dims]
        return self._detect_list(self.L.str_er_detect_planes_list, refs, MEM_DEVICE, stages | (WANT_NODES if want_nodes else 0))

    # ---- single stages ---------------------------------------------------------------------------
    def compute_channels(self, src: np.ndarray) -> np.ndarray:
        """ERFilter::compute_channels (src/ER.cpp:114-128) -> (6,H,W) uint8."""
        a = np.ascontiguousarray(src, dtype=np.uint8)
        h, w, _ = a.shape
        out = np.empty((6, h, w), np.uint8)
        self._check(self.L.str_er_compute_channels(self.h, _np_ptr(a), w, h, 3 * w, _np_ptr(out)))
        return out

    def er_tree_extract(self, plane: np.ndarray) -> PlaneResult:
        """ERFilter::er_tree_extract (src/ER.cpp:240-374): the kept tree as a node table."""
        return self.detect_planes(plane, STAGE_EXTRACT, want_nodes=True).planes[0]

    def non_maximum_supression(self, nodes: np.ndarray, rows: int, cols: int, plane: Optional[np.ndarray] = None):
        """ERFilter::non_maximum_supression (src/ER.cpp:416-505) on a node table.
        Returns (pool indices in ascending key order, ambiguous count).  Sibling ties (sibling_order = 0): without `plane` the
        table order is the child-list order; with the (rows, cols) uint8 plane they are decided by replaying the reference's flood."""
        nd = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
        cap = max(1, len(nd))
        pool = np.zeros(cap, np.int32)
        n, amb = C.c_int32(), C.c_int32()
        if plane is None:
            self._check(self.L.str_er_nms_tree(self.h, _np_ptr(nd), len(nd), rows, cols, _np_ptr(pool), cap, C.byref(n),
                                               C.byref(amb)))
        else:
            a = np.ascontiguousarray(plane, dtype=np.uint8)
            if a.shape != (rows, cols):
                raise ValueError("plane must be (rows, cols)")
            self._check(self.L.str_er_nms_tree_plane(self.h, _np_ptr(nd), len(nd), _np_ptr(a), cols, rows, cols, _np_ptr(pool), cap,
                                                     C.byref(n), C.byref(amb)))
        return pool[:n.value].copy(), amb.value

    def classify(self, plane: np.ndarray, boxes_xywh: np.ndarray):
        """ERFilter::classify (src/ER.cpp:507-528): (cls, score_strong, score_weak) per box."""
        a = np.ascontiguousarray(plane, dtype=np.uint8)
        b = np.ascontiguousarray(boxes_xywh, dtype=np.int32).reshape(-1, 4)
        n = len(b)
        cls = np.zeros(n, np.uint8)
        ss = np.zeros(n, np.float64)
        sw = np.zeros(n, np.float64)
        self._check(self.L.str_er_classify_boxes(self.h, _np_ptr(a), a.shape[1], a.shape[0], a.shape[1], _np_ptr(b), n,
                                                 _np_ptr(cls), _np_ptr(ss), _np_ptr(sw)))
        return cls, ss, sw

    def er_masks(self, plane: np.ndarray, regions: np.ndarray):
        """str_er_er_masks: the pixel masks of `regions` (CAND_DTYPE records; x, y, w, h, level and key are read) on one (H, W) uint8
        plane at the context's thresh_step.  Returns (words, pixels): the masks back to back in region order (region i: h rows of
        (w + 31) // 32 uint32 words) and their popcounts.  unpack_mask(words, off, w, h) gives one as a bool array."""
        a = np.ascontiguousarray(plane, dtype=np.uint8)
        r = np.ascontiguousarray(regions, dtype=CAND_DTYPE).reshape(-1)
        n = len(r)
        nw = C.c_uint64()
        self._check(self.L.str_er_er_masks(self.h, _np_ptr(a), a.shape[1], a.shape[0], a.shape[1], _np_ptr(r) if n else None, n,
                                           None, 0, C.byref(nw), None))
        words = np.zeros(max(1, nw.value), np.uint32)
        pixels = np.zeros(max(1, n), np.uint32)
        if n:
            self._check(self.L.str_er_er_masks(self.h, _np_ptr(a), a.shape[1], a.shape[0], a.shape[1], _np_ptr(r), n,
                                               _np_ptr(words), nw.value, C.byref(nw), _np_ptr(pixels)))
        return words[:nw.value], pixels[:n]

    def er_shapes(self, plane: np.ndarray, regions: np.ndarray) -> np.ndarray:
        """str_er_er_shapes: the descriptors (SHAPE_DTYPE) of the masks er_masks gives for `regions` on one (H, W) uint8 plane."""
        a = np.ascontiguousarray(plane, dtype=np.uint8)
        r = np.ascontiguousarray(regions, dtype=CAND_DTYPE).reshape(-1)
        n = len(r)
        out = np.zeros(max(1, n), SHAPE_DTYPE)
        self._check(self.L.str_er_er_shapes(self.h, _np_ptr(a), a.shape[1], a.shape[0], a.shape[1], _np_ptr(r) if n else None, n,
                                            _np_ptr(out)))
        return out[:n]

    def er_strokes(self, plane: np.ndarray, regions: np.ndarray) -> np.ndarray:
        """str_er_er_strokes: the stroke-width descriptors (STROKE_DTYPE) of the masks er_masks gives for `regions` on one (H, W) uint8 plane."""
        a = np.ascontiguousarray(plane, dtype=np.uint8)
        r = np.ascontiguousarray(regions, dtype=CAND_DTYPE).reshape(-1)
        n = len(r)
        out = np.zeros(max(1, n), STROKE_DTYPE)
        self._check(self.L.str_er_er_strokes(self.h, _np_ptr(a), a.shape[1], a.shape[0], a.shape[1], _np_ptr(r) if n else None, n,
                                             _np_ptr(out)))
        return out[:n]

    def text_map_regions(self, plane: np.ndarray, regions: np.ndarray, values, out_w: int, out_h: int, ids=None):
        """str_er_text_map_regions: the text map of `regions` (CAND_DTYPE; x, y, w, h, level and key are read) of one (h, w) uint8
        plane onto an (out_h, out_w) frame by the pixel rule of str_er_frame_map: each pixel the OR of values[i] over the regions whose
        mask (that of er_masks) holds its sample.  Returns the (out_h, out_w) uint8 map, and with ids (int32, >= 0) also the
        (out_h, out_w) int32 map of the smallest id covering each pixel (-1 for none): (map, id_map)."""
        a = np.ascontiguousarray(plane, dtype=np.uint8)
        r = np.ascontiguousarray(regions, dtype=CAND_DTYPE).reshape(-1)
        n = len(r)
        v = np.ascontiguousarray(values, dtype=np.uint8).reshape(-1)
        if len(v) != n:
            raise ValueError("values needs one entry per region")
        d = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        if d is not None and len(d) != n:
            raise ValueError("ids needs one entry per region")
        out = np.zeros((int(out_h), int(out_w)), np.uint8)
        out_ids = None if d is None else np.zeros((int(out_h), int(out_w)), np.int32)
        self._check(self.L.str_er_text_map_regions(self.h, _np_ptr(a), a.shape[1], a.shape[0], a.shape[1], _np_ptr(r) if n else None,
                                                   _np_ptr(v) if n else None, (_np_ptr(d) if n else _np_ptr(np.zeros(1, np.int32))) if d is not None else None,
                                                   n, int(out_w), int(out_h), _np_ptr(out), None if out_ids is None else _np_ptr(out_ids)))
        return out if d is None else (out, out_ids)

    def set_frame_merge(self, num: int = 1, den: int = 2) -> None:
        """str_er_set_frame_merge: two lines of a frame are duplicates from a Jaccard index of num / den of their footprints on
        (1 <= num <= den <= 65535; WANT_FRAME_LINES and line_feet_regions)."""
        self._check(self.L.str_er_set_frame_merge(self.h, int(num), int(den)))

    def line_feet_regions(self, plane: np.ndarray, regions: np.ndarray, line_of, n_lines: int, out_w: int, out_h: int):
        """str_er_line_feet_regions: the footprints of n_lines lines made of `regions` (CAND_DTYPE; x, y, w, h, level and key are
        read; region i belongs to line line_of[i]) of one (h, w) uint8 plane on an (out_h, out_w) frame, by the pixel rule of
        str_er_frame_map.  Returns (feet LINE_FOOT_DTYPE, bits uint32, pairs LINE_PAIR_DTYPE): line t's footprint is its h rows of
        (w + 31) // 32 words over its foot box, back to back in line order (unpack_mask reads one)."""
        a = np.ascontiguousarray(plane, dtype=np.uint8)
        r = np.ascontiguousarray(regions, dtype=CAND_DTYPE).reshape(-1)
        n = len(r)
        lo = np.ascontiguousarray(line_of, dtype=np.int32).reshape(-1)
        if len(lo) != n:
            raise ValueError("line_of needs one entry per region")
        feet = np.zeros(max(1, int(n_lines)), LINE_FOOT_DTYPE)
        nw, npairs = C.c_uint64(), C.c_int32()
        args = (self.h, _np_ptr(a), a.shape[1], a.shape[0], a.shape[1], _np_ptr(r) if n else None, _np_ptr(lo) if n else None, n, int(n_lines),
                int(out_w), int(out_h), _np_ptr(feet))
        self._check(self.L.str_er_line_feet_regions(*args, None, 0, C.byref(nw), None, 0, C.byref(npairs)))
        bits = np.zeros(max(1, nw.value), np.uint32)
        pairs = np.zeros(max(1, npairs.value), LINE_PAIR_DTYPE)
        self._check(self.L.str_er_line_feet_regions(*args, _np_ptr(bits), len(bits), C.byref(nw), _np_ptr(pairs), len(pairs), C.byref(npairs)))
        return feet[:int(n_lines)], bits[:nw.value], pairs[:npairs.value]

    def set_line_link(self, num: int = 1, den: int = 2) -> None:
        """str_er_set_line_link: two lines of adjacent frames are linked from a Jaccard index of num / den of their footprints on
        (1 <= num <= den <= 65535; WANT_LINE_LINKS and link_feet)."""
        self._check(self.L.str_er_set_line_link(self.h, int(num), int(den)))

    def link_feet(self, W: int, H: int, feet_a: np.ndarray, bits_a: np.ndarray, feet_b: np.ndarray, bits_b: np.ndarray) -> np.ndarray:
        """str_er_link_feet: the overlaps of every line of set a with every line of set b, two sets of footprints in the pixels of one
        (H, W) frame: feet LINE_FOOT_DTYPE (box and pixels are read), bits the rows of (w + 31) // 32 words over each foot box, back to
        back -- what line_feet_regions and Result.edge_feet return.  Returns LINE_LINK_DTYPE records with inter > 0, a / b indices into
        the two sets, sorted by (a, b), link set at the context's threshold."""
        fa = np.ascontiguousarray(feet_a, dtype=LINE_FOOT_DTYPE).reshape(-1)
        fb = np.ascontiguousarray(feet_b, dtype=LINE_FOOT_DTYPE).reshape(-1)
        ba = np.ascontiguousarray(bits_a, dtype=np.uint32).reshape(-1)
        bb = np.ascontiguousarray(bits_b, dtype=np.uint32).reshape(-1)
        for ft, bt in ((fa, ba), (fb, bb)):
            if int((ft["h"].astype(np.int64).clip(0) * ((ft["w"].astype(np.int64).clip(0) + 31) // 32)).sum()) != len(bt):
                raise ValueError("bits needs h rows of (w + 31) // 32 words per foot, back to back")
        n = C.c_int32()
        args = (self.h, int(W), int(H), _np_ptr(fa) if len(fa) else None, _np_ptr(ba) if len(ba) else None, len(fa),
                _np_ptr(fb) if len(fb) else None, _np_ptr(bb) if len(bb) else None, len(fb))
        self._check(self.L.str_er_link_feet(*args, None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value), LINE_LINK_DTYPE)
        if n.value:
            self._check(self.L.str_er_link_feet(*args, _np_ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    def feet_geom(self, W: int, H: int, feet: np.ndarray, bits: np.ndarray):
        """str_er_feet_geom: the geometry (str_er_line_geom) of footprints in the pixels of one (H, W) frame, on the GPU: feet
        LINE_FOOT_DTYPE (box and pixels are read), bits the rows of (w + 31) // 32 words over each foot box, back to back -- what
        line_feet_regions and Result.edge_feet return.  Returns (LINE_GEOM_DTYPE per footprint, (n_points, 2) int32 hull vertices)."""
        ft = np.ascontiguousarray(feet, dtype=LINE_FOOT_DTYPE).reshape(-1)
        bt = np.ascontiguousarray(bits, dtype=np.uint32).reshape(-1)
        if int((ft["h"].astype(np.int64).clip(0) * ((ft["w"].astype(np.int64).clip(0) + 31) // 32)).sum()) != len(bt):
            raise ValueError("bits needs h rows of (w + 31) // 32 words per foot, back to back")
        geoms = np.zeros(max(1, len(ft)), LINE_GEOM_DTYPE)
        n = C.c_int32()
        cap = int((2 * (ft["h"].astype(np.int64).clip(0) + 1)).sum())        # (a hull has at most two vertices per height 0 .. h: one call)
        xy = np.zeros((max(1, cap), 2), np.int32)
        self._check(self.L.str_er_feet_geom(self.h, int(W), int(H), _np_ptr(ft) if len(ft) else None, _np_ptr(bt) if len(bt) else None, len(ft),
                                            _np_ptr(geoms), _np_ptr(xy), min(len(xy), 2 ** 31 - 1), C.byref(n)))
        return geoms[:len(ft)], xy[:n.value].copy()

    def set_word_gap(self, num: int = 1, den: int = 3) -> None:
        """str_er_set_word_gap: a gap between glyph runs breaks a word when gap * den >= num * colmax (1 <= num, den <= 65535)."""
        self._check(self.L.str_er_set_word_gap(self.h, int(num), int(den)))

    def set_lexicon(self, words, fold_case: bool = True) -> None:
        """str_er_set_lexicon: the lexicon of the word matcher (str_er_word_match): strings (or bytes) of 1 .. 32 characters of the
        alphabet of ocr_char, at most 2^20 of them; an empty sequence clears it.  fold_case: compared without regard to case."""
        self._check(_set_lexicon(self.L, self.h, words, fold_case))
        self._lexicon = _lexicon_strings(words)

    def lexicon_info(self) -> dict:
        """str_er_lexicon_info: the entries and flags of the lexicon, the matcher's chunk size in entries, its bytes on the device."""
        n, fl, ch, by = C.c_int32(), C.c_uint32(), C.c_int32(), C.c_uint64()
        self._check(self.L.str_er_lexicon_info(self.h, C.byref(n), C.byref(fl), C.byref(ch), C.byref(by)))
        return {"n": int(n.value), "flags": int(fl.value), "chunk_entries": int(ch.value), "device_bytes": int(by.value)}

    def set_word_match(self, ins: int = 64, dele: int = 64, band: int = 2) -> None:
        """str_er_set_word_match: INS, DEL (1 .. 255) and the band (0 .. 31) of the word matcher."""
        self._check(self.L.str_er_set_word_match(self.h, int(ins), int(dele), int(band)))

    def run_costs(self, prob: np.ndarray) -> np.ndarray:
        """str_er_run_costs: the cost rows (n, 65) uint8 of (n, nr_class) class probabilities, on the GPU, with the labels of the
        loaded SVM model and the fold-case flag of the lexicon."""
        p = np.ascontiguousarray(prob, dtype=np.float64)
        k = self.svm_info()[0]
        if p.ndim != 2 or (k and p.shape[1] != k):
            raise ValueError("prob must be (n, nr_class)")
        out = np.zeros((len(p), 65), np.uint8)
        self._check(self.L.str_er_run_costs(self.h, _np_ptr(p) if p.size else None, len(p), _np_ptr(out) if len(p) else None))
        return out

    def match_words(self, costs: np.ndarray, first_run, n_runs_of_word) -> np.ndarray:
        """str_er_match_words: the words [first_run[w], first_run[w] + n_runs_of_word[w]) of the cost rows (n runs, 65) uint8
        against the lexicon; WORD_MATCH_DTYPE per word."""
        cs = np.ascontiguousarray(costs, dtype=np.uint8).reshape(-1, 65)
        fr = np.ascontiguousarray(first_run, dtype=np.int32).reshape(-1)
        no = np.ascontiguousarray(n_runs_of_word, dtype=np.int32).reshape(-1)
        if len(fr) != len(no):
            raise ValueError("first_run and n_runs_of_word: one value per word each")
        out = np.zeros(max(1, len(fr)), WORD_MATCH_DTYPE)
        self._check(self.L.str_er_match_words(self.h, _np_ptr(cs) if len(cs) else None, len(cs), _np_ptr(fr) if len(fr) else None,
                                              _np_ptr(no) if len(no) else None, len(fr), _np_ptr(out)))
        return out[:len(fr)]

    def set_word_link(self, num: int = 1, den: int = 2) -> None:
        """str_er_set_word_link: two words of adjacent frames are linked from a Jaccard index of num / den of their boxes on
        (str_er_word_link); each in 1 .. 65535."""
        self._check(self.L.str_er_set_word_link(self.h, int(num), int(den)))
        self._word_link = (int(num), int(den))

    def word_links(self, feet, frames_of_lines, line_tracks, frame_wh, words):
        """word_links (pure host) at the threshold of set_word_link."""
        return word_links(feet, frames_of_lines, line_tracks, frame_wh, words, *getattr(self, "_word_link", (1, 2)))

    def word_tracks_from_links(self, frames_of_lines, line_tracks, reading, words, links):
        """word_tracks_from_links (pure host)."""
        return word_tracks_from_links(frames_of_lines, line_tracks, reading, words, links)

    def match_tracks(self, costs: np.ndarray, first_run, n_runs_of_word, track_first, track_count, members):
        """str_er_match_tracks: the tracks members[track_first[g]:track_first[g] + track_count[g]] of the words [first_run[w],
        first_run[w] + n_runs_of_word[w]) of the cost rows (n rows, 65) uint8 against the lexicon; returns (TRACK_MATCH_DTYPE per
        track, int32 member costs per slot of members)."""
        cs, fr, no, tf, tc, mem = _track_args(costs, first_run, n_runs_of_word, track_first, track_count, members)
        out = np.zeros(max(1, len(tf)), TRACK_MATCH_DTYPE)
        mc = np.zeros(max(1, len(mem)), np.int32)
        opt = lambda a: _np_ptr(a) if len(a) else None
        self._check(self.L.str_er_match_tracks(self.h, opt(cs), len(cs), opt(fr), opt(no), len(fr), opt(tf), opt(tc), opt(mem), len(mem), len(tf),
                                               _np_ptr(out), _np_ptr(mc)))
        return out[:len(tf)], mc[:len(mem)]

    def set_track_decode(self, ins: int = 64, dele: int = 64, rounds: int = 8) -> None:
        """str_er_set_track_decode: INS and DEL (1 .. 255) and the polish rounds (0 .. 64) of the track decode."""
        self._check(self.L.str_er_set_track_decode(self.h, int(ins), int(dele), int(rounds)))

    def decode_tracks(self, costs: np.ndarray, first_run, n_runs_of_word, track_first, track_count, members):
        """str_er_decode_tracks: the tracks members[track_first[g]:track_first[g] + track_count[g]] of the words [first_run[w],
        first_run[w] + n_runs_of_word[w]) of the cost rows (n rows, 65) uint8 under the table, set_word_decode (the seeds) and
        set_track_decode; returns (TRACK_DECODE_DTYPE per track, (n tracks, 32) uint8 labels, int32 member costs per slot of members)."""
        cs, fr, no, tf, tc, mem = _track_args(costs, first_run, n_runs_of_word, track_first, track_count, members)
        out = np.zeros(max(1, len(tf)), TRACK_DECODE_DTYPE)
        ch = np.full((max(1, len(tf)), 32), 0xFF, np.uint8)
        mc = np.zeros(max(1, len(mem)), np.int32)
        opt = lambda a: _np_ptr(a) if len(a) else None
        self._check(self.L.str_er_decode_tracks(self.h, opt(cs), len(cs), opt(fr), opt(no), len(fr), opt(tf), opt(tc), opt(mem), len(mem), len(tf),
                                                _np_ptr(out), _np_ptr(ch), _np_ptr(mc)))
        return out[:len(tf)], ch[:len(tf)], mc[:len(mem)]

    def set_bigram(self, table) -> None:
        """str_er_set_bigram: the (66, 66) uint8 table of the word decoder (str_er_word_decode; bigram_from_probs / bigram_from_words
        make one); None removes it."""
        self._check(self.L.str_er_set_bigram(self.h, None if table is None else _np_ptr(_bigram_table(table))))

    def bigram_info(self) -> dict:
        """str_er_bigram_info: whether a table is set and its bytes on the device."""
        st, by = C.c_int32(), C.c_uint64()
        self._check(self.L.str_er_bigram_info(self.h, C.byref(st), C.byref(by)))
        return {"set": bool(st.value), "device_bytes": int(by.value)}

    def set_word_decode(self, ins: int = 0, dele: int = 0) -> None:
        """str_er_set_word_decode: INS and DEL (0 .. 255, 0: off) of the word decoder."""
        self._check(self.L.str_er_set_word_decode(self.h, int(ins), int(dele)))

    def decode_words(self, costs: np.ndarray, first_run, n_runs_of_word):
        """str_er_decode_words: the words [first_run[w], first_run[w] + n_runs_of_word[w]) of the cost rows (n runs, 65) uint8 under
        the table; (WORD_DECODE_DTYPE per word, (n, 64) uint8 labels, (n, 64) uint8 sources)."""
        cs, fr, no, out, ch, sr = _decode_args(costs, first_run, n_runs_of_word)
        self._check(self.L.str_er_decode_words(self.h, _np_ptr(cs) if len(cs) else None, len(cs), _np_ptr(fr) if len(fr) else None,
                                               _np_ptr(no) if len(no) else None, len(fr), _np_ptr(out), _np_ptr(ch), _np_ptr(sr)))
        return out[:len(fr)], ch[:len(fr)], sr[:len(fr)]

    def set_word_margin(self, on: bool = True) -> None:
        """str_er_set_word_margin: whether a detect call with WANT_WORD_DECODE also makes the margins of its words (off by default)."""
        self._check(self.L.str_er_set_word_margin(self.h, 1 if on else 0))

    def set_line_decode(self, on: bool = True, weight: int = 16) -> None:
        """str_er_set_line_decode: whether a detect call with WANT_WORD_DECODE also decodes every line jointly with its word breaks
        (str_er_line_decode; off by default), and the weight (0 .. 127) of the gap costs."""
        self._check(self.L.str_er_set_line_decode(self.h, 1 if on else 0, int(weight)))

    def decode_lines(self, costs: np.ndarray, gaps, first_row, n_rows):
        """str_er_decode_lines: the lines [first_row[t], first_row[t] + n_rows[t]) of the cost rows (n, 65) uint8 with the gap costs
        (n, 2) uint8 under the table and set_word_decode; (LINE_DECODE_DTYPE per line, (3n,) uint8 labels, (3n,) uint16 sources, (n,)
        int32 word of every row)."""
        cs, gp, fr, no, out, ch, sr, wr = _line_decode_args(costs, gaps, first_row, n_rows)
        opt = lambda a: _np_ptr(a) if len(a) else None
        self._check(self.L.str_er_decode_lines(self.h, opt(cs), len(cs), opt(gp), opt(fr), opt(no), len(fr), _np_ptr(out), _np_ptr(ch), _np_ptr(sr), _np_ptr(wr)))
        return out[:len(fr)], ch[:3 * len(cs)], sr[:3 * len(cs)], wr[:len(cs)]

    def set_line_margin(self, on: bool = True) -> None:
        """str_er_set_line_margin: whether a detect call that decodes its lines (set_line_decode(True) and WANT_WORD_DECODE) also makes
        their margins (str_er_line_margin; off by default)."""
        self._check(self.L.str_er_set_line_margin(self.h, 1 if on else 0))

    def line_margins(self, costs: np.ndarray, gaps, first_row, n_rows, want_marginals: bool = False):
        """str_er_line_margins: the margins (str_er_line_margin) of the lines decode_lines takes, under the table and set_word_decode;
        (LINE_MARGIN_DTYPE per line, (n,) int32 row margins, (n,) uint8 row readings, (n,) uint8 row alternatives, (n,) int32 gap
        margins, (n,) uint8 gap moves[, (n, 68) int32 marginals])."""
        cs, gp, fr, no, out, rm, rr, ra, gm, gv, mg = _line_margin_args(costs, gaps, first_row, n_rows, want_marginals)
        opt = lambda a: _np_ptr(a) if len(a) else None
        self._check(self.L.str_er_line_margins(self.h, opt(cs), len(cs), opt(gp), opt(fr), opt(no), len(fr), _np_ptr(out), _np_ptr(rm), _np_ptr(rr), _np_ptr(ra),
                                               _np_ptr(gm), _np_ptr(gv), _np_ptr(mg) if want_marginals else None))
        return _line_margin_out(len(cs), len(fr), out, rm, rr, ra, gm, gv, mg, want_marginals)

    def line_margin_stats(self) -> dict:
        """str_er_line_margin_stats: the bytes of the margins' forward table on the device."""
        by = C.c_uint64()
        self._check(self.L.str_er_line_margin_stats(self.h, C.byref(by)))
        return {"table_bytes": int(by.value)}

    def line_decode_stats(self) -> dict:
        """str_er_line_decode_stats: the bytes of the line decoder's back-pointer table on the device."""
        by = C.c_uint64()
        self._check(self.L.str_er_line_decode_stats(self.h, C.byref(by)))
        return {"table_bytes": int(by.value)}

    def word_margins(self, costs: np.ndarray, first_run, n_runs_of_word, want_marginals: bool = False):
        """str_er_word_margins: the margins (str_er_word_margin) of the words [first_run[w], first_run[w] + n_runs_of_word[w]) of the
        cost rows (n runs, 65) uint8 under the table and set_word_decode; (WORD_MARGIN_DTYPE per word, (n, 32) int32 row margins,
        (n, 32) uint8 row readings, (n, 32) uint8 row alternatives, and with want_marginals (n, 32, 66) int32 marginals, else None)."""
        cs, fr, no, out, rm, rr, ra, mg = _margin_args(costs, first_run, n_runs_of_word, want_marginals)
        self._check(self.L.str_er_word_margins(self.h, _np_ptr(cs) if len(cs) else None, len(cs), _np_ptr(fr) if len(fr) else None,
                                               _np_ptr(no) if len(no) else None, len(fr), _np_ptr(out), _np_ptr(rm), _np_ptr(rr), _np_ptr(ra),
                                               None if mg is None else _np_ptr(mg)))
        return out[:len(fr)], rm[:len(fr)], rr[:len(fr)], ra[:len(fr)], None if mg is None else mg[:len(fr)]

    def feet_words(self, W: int, H: int, feet: np.ndarray, bits: np.ndarray):
        """str_er_feet_words: the glyph runs and words (str_er_line_run) of footprints in the pixels of one (H, W) frame, the runs made
        on the GPU: feet and bits as feet_geom takes them.  Returns (LINE_WORDS_DTYPE per footprint, LINE_RUN_DTYPE runs, LINE_WORD_DTYPE
        words), the words at the gap of set_word_gap."""
        ft = np.ascontiguousarray(feet, dtype=LINE_FOOT_DTYPE).reshape(-1)
        bt = np.ascontiguousarray(bits, dtype=np.uint32).reshape(-1)
        if int((ft["h"].astype(np.int64).clip(0) * ((ft["w"].astype(np.int64).clip(0) + 31) // 32)).sum()) != len(bt):
            raise ValueError("bits needs h rows of (w + 31) // 32 words per foot, back to back")
        lw = np.zeros(max(1, len(ft)), LINE_WORDS_DTYPE)
        cap = int(((ft["w"].astype(np.int64).clip(0) + 1) // 2).sum())          # (a row of w columns holds at most (w + 1) // 2 runs: one call)
        runs = np.zeros(max(1, cap), LINE_RUN_DTYPE)
        words = np.zeros(max(1, cap), LINE_WORD_DTYPE)
        nr, nw = C.c_int32(), C.c_int32()
        self._check(self.L.str_er_feet_words(self.h, int(W), int(H), _np_ptr(ft) if len(ft) else None, _np_ptr(bt) if len(bt) else None, len(ft),
                                             _np_ptr(lw), _np_ptr(runs), min(len(runs), 2 ** 31 - 1), C.byref(nr), _np_ptr(words),
                                             min(len(words), 2 ** 31 - 1), C.byref(nw)))
        return lw[:len(ft)], runs[:nr.value].copy(), words[:nw.value].copy()

    def feet_read(self, W: int, H: int, feet: np.ndarray, bits: np.ndarray, slopes=None, want_reads: bool = True):
        """str_er_feet_read: feet_words and the reading of every glyph run (str_er_run_read): slopes one per footprint (None: all 0).
        Returns (line_words, runs, words, reads RUN_READ_DTYPE or None without want_reads, features (n runs, 1800) uint8); without
        want_reads no SVM model is needed."""
        ft = np.ascontiguousarray(feet, dtype=LINE_FOOT_DTYPE).reshape(-1)
        bt = np.ascontiguousarray(bits, dtype=np.uint32).reshape(-1)
        if int((ft["h"].astype(np.int64).clip(0) * ((ft["w"].astype(np.int64).clip(0) + 31) // 32)).sum()) != len(bt):
            raise ValueError("bits needs h rows of (w + 31) // 32 words per foot, back to back")
        sl = None
        if slopes is not None:
            sl = np.ascontiguousarray(slopes, dtype=np.float64).reshape(-1)
            if len(sl) != len(ft):
                raise ValueError("slopes needs one entry per foot")
        lw = np.zeros(max(1, len(ft)), LINE_WORDS_DTYPE)
        nr, nw = C.c_int32(), C.c_int32()
        args = (self.h, int(W), int(H), _np_ptr(ft) if len(ft) else None, _np_ptr(bt) if len(bt) else None,
                _np_ptr(sl) if sl is not None and len(sl) else None, len(ft), _np_ptr(lw))
        self._check(self.L.str_er_feet_read(*args, None, 0, C.byref(nr), None, 0, C.byref(nw), None, None))         # (the counting call)
        runs = np.zeros(max(1, nr.value), LINE_RUN_DTYPE)
        words = np.zeros(max(1, nw.value), LINE_WORD_DTYPE)
        reads = np.zeros(max(1, nr.value), RUN_READ_DTYPE) if want_reads else None
        q = np.zeros((max(1, nr.value), 1800), np.uint8)
        self._check(self.L.str_er_feet_read(*args, _np_ptr(runs), len(runs), C.byref(nr), _np_ptr(words), len(words), C.byref(nw),
                                            _np_ptr(reads) if want_reads else None, _np_ptr(q)))
        return lw[:len(ft)], runs[:nr.value].copy(), words[:nw.value].copy(), reads[:nr.value].copy() if want_reads else None, q[:nr.value].copy()

    def set_run_split(self, num: int = 1, den: int = 4, split_cost: int = 8) -> None:
        """str_er_set_run_split: the valley threshold num / den of a run's height (1 .. 65535 each) and SPLIT (0 .. 255) of
        feet_split and split_words (str_er_run_split)."""
        self._check(self.L.str_er_set_run_split(self.h, int(num), int(den), int(split_cost)))

    def run_split_stats(self):
        """str_er_run_split_stats: (bytes of the cut records, bytes of the segmentation tables) on the device; 0: never made."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self.L.str_er_run_split_stats(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def feet_split(self, W: int, H: int, feet: np.ndarray, bits: np.ndarray, slopes=None, want_reads: bool = True, want_q: bool = True):
        """str_er_feet_split: feet_read and the cuts and pieces of every glyph run (str_er_run_split), made on the GPU.  Returns a dict:
        line_words, runs, words, reads (None without want_reads), q, splits (RUN_SPLIT_DTYPE per run), pieces (RUN_PIECE_DTYPE),
        piece_reads (None without want_reads) and piece_q ((n pieces, 1800) uint8, None without want_q).  Without want_reads no SVM
        model is needed."""
        ft = np.ascontiguousarray(feet, dtype=LINE_FOOT_DTYPE).reshape(-1)
        bt = np.ascontiguousarray(bits, dtype=np.uint32).reshape(-1)
        if int((ft["h"].astype(np.int64).clip(0) * ((ft["w"].astype(np.int64).clip(0) + 31) // 32)).sum()) != len(bt):
            raise ValueError("bits needs h rows of (w + 31) // 32 words per foot, back to back")
        sl = None
        if slopes is not None:
            sl = np.ascontiguousarray(slopes, dtype=np.float64).reshape(-1)
            if len(sl) != len(ft):
                raise ValueError("slopes needs one entry per foot")
        lw = np.zeros(max(1, len(ft)), LINE_WORDS_DTYPE)
        nr, nw, npc = C.c_int32(), C.c_int32(), C.c_int32()
        args = (self.h, int(W), int(H), _np_ptr(ft) if len(ft) else None, _np_ptr(bt) if len(bt) else None,
                _np_ptr(sl) if sl is not None and len(sl) else None, len(ft), _np_ptr(lw))
        self._check(self.L.str_er_feet_read(*args, None, 0, C.byref(nr), None, 0, C.byref(nw), None, None))         # (the counting call)
        n = nr.value
        runs = np.zeros(max(1, n), LINE_RUN_DTYPE)
        words = np.zeros(max(1, nw.value), LINE_WORD_DTYPE)
        reads = np.zeros(max(1, n), RUN_READ_DTYPE) if want_reads else None
        q = np.zeros((max(1, n), 1800), np.uint8)
        splits = np.zeros(max(1, n), RUN_SPLIT_DTYPE)
        cap = 9 * n                                                    # (a run has at most 9 pieces: one call)
        pieces = np.zeros(max(1, cap), RUN_PIECE_DTYPE)
        preads = np.zeros(max(1, cap), RUN_READ_DTYPE) if want_reads else None
        pq = np.zeros((max(1, cap), 1800), np.uint8) if want_q else None
        self._check(self.L.str_er_feet_split(*args, _np_ptr(runs), len(runs), C.byref(nr), _np_ptr(words), len(words), C.byref(nw),
                                             _np_ptr(reads) if want_reads else None, _np_ptr(q), _np_ptr(splits), _np_ptr(pieces), cap, C.byref(npc),
                                             _np_ptr(preads) if want_reads else None, _np_ptr(pq) if want_q else None))
        k = npc.value
        return {"line_words": lw[:len(ft)], "runs": runs[:nr.value].copy(), "words": words[:nw.value].copy(),
                "reads": reads[:nr.value].copy() if want_reads else None, "q": q[:nr.value].copy(), "splits": splits[:nr.value].copy(),
                "pieces": pieces[:k].copy(), "piece_reads": preads[:k].copy() if want_reads else None, "piece_q": pq[:k].copy() if want_q else None}

    def split_words(self, splits, run_costs, piece_costs, first_run, n_runs_of_word):
        """str_er_split_words: the segmentation (str_er_run_split) of the runs of the words [first_run[w], first_run[w] +
        n_runs_of_word[w]) from the cost rows of the runs (n runs, 65) and of their pieces (n pieces, 65), at the SPLIT of
        set_run_split.  Returns (WORD_SPLIT_DTYPE per word, SPLIT_PART_DTYPE parts, (n parts, 65) uint8 rows of the parts)."""
        a = _split_args(splits, run_costs, piece_costs, first_run, n_runs_of_word)
        self._check(self.L.str_er_split_words(self.h, *a[0], *a[1]))
        return _split_out(a)

    def lattice_decode_stats(self) -> int:
        """str_er_lattice_decode_stats: the bytes of the lattice decode tables on the device; 0: never made."""
        a = C.c_uint64()
        self._check(self.L.str_er_lattice_decode_stats(self.h, C.byref(a)))
        return int(a.value)

    def lattice_decode_words(self, splits, run_costs, piece_costs, first_run, n_runs_of_word):
        """str_er_lattice_decode_words: the joint decode (str_er_lattice_decode) of the words [first_run[w], first_run[w] +
        n_runs_of_word[w]) over the pieces of their runs, from the unfolded cost rows of the runs (n runs, 65) and of their pieces
        (n pieces, 65), under the table of set_bigram with INS / DEL of set_word_decode and SPLIT of set_run_split.  Returns
        (LATTICE_DECODE_DTYPE per word, (n, 64) uint8 labels, (n, 64) uint8 sources, SPLIT_PART_DTYPE lattice parts)."""
        a = _lattice_args(splits, run_costs, piece_costs, first_run, n_runs_of_word)
        self._check(self.L.str_er_lattice_decode_words(self.h, *a[0], *a[1]))
        return _lattice_out(a)

    def set_line_lattice_decode(self, on: bool = True, weight: int = 16) -> None:
        """str_er_set_line_lattice_decode: whether a detect call with WANT_LATTICE_DECODE also decodes every line over the piece lattices
        of its runs, cuts, word breaks and string together (str_er_line_lattice_decode; off by default), and the weight (0 .. 127) of
        the gap costs."""
        self._check(self.L.str_er_set_line_lattice_decode(self.h, 1 if on else 0, int(weight)))

    def lattice_decode_lines(self, splits, run_costs, piece_costs, gaps, first_run, n_runs_of_line):
        """str_er_lattice_decode_lines: the joint decode (str_er_line_lattice_decode) of the lines [first_run[t], first_run[t] +
        n_runs_of_line[t]) over the pieces of their runs, from the unfolded cost rows of the runs (n runs, 65) and of their pieces
        (n pieces, 65) and the gap costs (n runs, 2) uint8, under the table of set_bigram with INS / DEL of set_word_decode and SPLIT
        of set_run_split.  With S the atoms of all runs, returns (LINE_LATTICE_DECODE_DTYPE per line, (3S,) uint8 labels, (3S,) uint16
        sources, SPLIT_PART_DTYPE parts, int32 word of every part)."""
        a = _line_lattice_args(splits, run_costs, piece_costs, gaps, first_run, n_runs_of_line)
        self._check(self.L.str_er_lattice_decode_lines(self.h, *a[0], *a[1]))
        return _line_lattice_out(a)

    def line_lattice_decode_stats(self) -> dict:
        """str_er_line_lattice_decode_stats: the bytes of the line lattice decoder's back-pointer table on the device."""
        by = C.c_uint64()
        self._check(self.L.str_er_line_lattice_decode_stats(self.h, C.byref(by)))
        return {"table_bytes": int(by.value)}

    def set_lattice_margin(self, on: bool = True) -> None:
        """str_er_set_lattice_margin: whether a detect call with WANT_LATTICE_DECODE also makes the margins of its words (off by default)."""
        self._check(self.L.str_er_set_lattice_margin(self.h, 1 if on else 0))

    def lattice_margins(self, splits, run_costs, piece_costs, first_run, n_runs_of_word, want_edges: bool = False, want_marginals: bool = False):
        """str_er_lattice_margins: the margins (str_er_lattice_margin) of the words lattice_decode_words takes, under the same table and
        settings; (LATTICE_MARGIN_DTYPE per word, (n, 32) int32 reading margins, (n, 32) int32 cut margins, (n, 32) uint8 readings,
        (n, 32) uint8 alternatives, (n, 32) uint8 cut alternatives, with want_edges (n, 32, 4) int32 edge minima, else None, with
        want_marginals (n, 32, 4, 66) int32 marginals, else None)."""
        a, out = _lattice_margin_args(splits, run_costs, piece_costs, first_run, n_runs_of_word, want_edges, want_marginals)
        self._check(self.L.str_er_lattice_margins(self.h, *a[0], *[None if v is None else _np_ptr(v) for v in out]))
        return tuple(None if v is None else v[:len(a[2][3])] for v in out)

    def lattice_track_stats(self) -> int:
        """str_er_lattice_track_stats: the bytes of the lattice track tables on the device; 0: never made."""
        a = C.c_uint64()
        self._check(self.L.str_er_lattice_track_stats(self.h, C.byref(a)))
        return int(a.value)

    def lattice_match_tracks(self, splits, run_costs, piece_costs, first_run, n_runs_of_word, track_first, track_count, members):
        """str_er_lattice_match_tracks: the track match over the members' piece lattices (str_er_lattice_track_member) of the tracks
        members[track_first[g]:track_first[g] + track_count[g]] of the words [first_run[w], first_run[w] + n_runs_of_word[w]) of the runs
        (splits: RUN_SPLIT_DTYPE, run_costs (n runs, 65), piece_costs (n pieces, 65)) against the lexicon; returns (TRACK_MATCH_DTYPE
        per track, LATTICE_TRACK_MEMBER_DTYPE per slot of members, (slots, 32) uint8 sources, SPLIT_PART_DTYPE parts)."""
        a = _lattice_track_args(splits, run_costs, piece_costs, first_run, n_runs_of_word, track_first, track_count, members)
        self._check(self.L.str_er_lattice_match_tracks(self.h, *a[0], *a[1]))
        return _lattice_track_out(a)

    def set_lattice_track_decode(self, on: bool = True) -> None:
        """str_er_set_lattice_track_decode: whether a detect call with WANT_TRACK_DECODE and WANT_LATTICE_DECODE also decodes every word
        track over its members' piece lattices (off by default)."""
        self._check(self.L.str_er_set_lattice_track_decode(self.h, 1 if on else 0))

    def lattice_track_decode_stats(self) -> int:
        """str_er_lattice_track_decode_stats: the bytes of the lattice track decode tables on the device; 0: never made."""
        a = C.c_uint64()
        self._check(self.L.str_er_lattice_track_decode_stats(self.h, C.byref(a)))
        return int(a.value)

    def lattice_decode_tracks(self, splits, run_costs, piece_costs, first_run, n_runs_of_word, track_first, track_count, members):
        """str_er_lattice_decode_tracks: the track decode over the members' piece lattices (str_er_lattice_track_decode) of the tracks
        members[track_first[g]:track_first[g] + track_count[g]] of the words lattice_match_tracks takes, under the context's table, its
        set_word_decode INS / DEL for the seeds, its set_track_decode parameters and its SPLIT; returns (TRACK_DECODE_DTYPE per track,
        (n tracks, 32) uint8 labels, LATTICE_TRACK_MEMBER_DTYPE per slot of members, (slots, 32) uint8 sources, SPLIT_PART_DTYPE parts)."""
        a, out, ch = _lattice_track_decode_args(splits, run_costs, piece_costs, first_run, n_runs_of_word, track_first, track_count, members)
        self._check(self.L.str_er_lattice_decode_tracks(self.h, *a[0], _np_ptr(out), _np_ptr(ch), *a[1][1:]))
        return _lattice_track_decode_out(a, out, ch)

    def lattice_match_stats(self) -> int:
        """str_er_lattice_match_stats: the bytes of the lattice match tables on the device; 0: never made."""
        a = C.c_uint64()
        self._check(self.L.str_er_lattice_match_stats(self.h, C.byref(a)))
        return int(a.value)

    def lattice_match_words(self, splits, run_costs, piece_costs, first_run, n_runs_of_word):
        """str_er_lattice_match_words: the lexicon match over the piece lattice (str_er_lattice_match) of the words [first_run[w],
        first_run[w] + n_runs_of_word[w]), from the cost rows of the runs (n runs, 65) and of their pieces (n pieces, 65) as they are (the
        fold is applied when they are read), with the lexicon of set_lexicon, INS / DEL / band of set_word_match and SPLIT of
        set_run_split.  Returns (LATTICE_MATCH_DTYPE per word, (n, 32) uint8 sources, SPLIT_PART_DTYPE parts)."""
        a = _lattice_match_args(splits, run_costs, piece_costs, first_run, n_runs_of_word)
        self._check(self.L.str_er_lattice_match_words(self.h, *a[0], *a[1]))
        return _lattice_match_out(a)

    def run_atlas_stats(self):
        """str_er_run_atlas_stats: (bytes of the run tile atlas, how often it was allocated or grown)."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self.L.str_er_run_atlas_stats(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def set_line_crop(self, height: int = 32, max_width: int = 1024, pad: float = 0.125) -> None:
        """str_er_set_line_crop: the crop height (8..256), the widest crop (1..8192) and the pad (0..1, of the line's height) of
        WANT_LINE_CROPS and line_crops."""
        self._check(self.L.str_er_set_line_crop(self.h, int(height), int(max_width), float(pad)))

    def line_crops(self, plane: np.ndarray, boxes_xywh: np.ndarray, first, count, slopes):
        """str_er_line_crops: grey crops of lines of one (H, W) uint8 plane at the context's crop settings.  Line k has the boxes
        boxes_xywh[first[k]:first[k] + count[k]] and slope slopes[k].  Returns (records LINE_CROP_DTYPE, crop bytes)."""
        a = np.ascontiguousarray(plane, dtype=np.uint8)
        bx = np.ascontiguousarray(boxes_xywh, dtype=np.int32).reshape(-1, 4)
        fi = np.ascontiguousarray(first, dtype=np.int32).reshape(-1)
        co = np.ascontiguousarray(count, dtype=np.int32).reshape(-1)
        sl = np.ascontiguousarray(slopes, dtype=np.float64).reshape(-1)
        n = len(fi)
        if len(co) != n or len(sl) != n or (n and int((fi + co).max()) > len(bx)):
            raise ValueError("first / count / slopes must have one entry per line, and the boxes they name must exist")
        recs = np.zeros(max(1, n), LINE_CROP_DTYPE)
        nb = C.c_uint64()
        args = (self.h, _np_ptr(a), a.shape[1], a.shape[0], a.shape[1], _np_ptr(bx) if len(bx) else None, _np_ptr(fi) if n else None,
                _np_ptr(co) if n else None, _np_ptr(sl) if n else None, n)
        self._check(self.L.str_er_line_crops(*args, None, 0, C.byref(nb), _np_ptr(recs)))
        pixels = np.zeros(max(1, nb.value), np.uint8)
        if n:
            self._check(self.L.str_er_line_crops(*args, _np_ptr(pixels), nb.value, C.byref(nb), _np_ptr(recs)))
        return recs[:n], pixels[:nb.value]

    def predict(self, which: int, fv: np.ndarray) -> np.ndarray:
        """stc->predict(fv) / wtc->predict(fv) (inc/adaboost.h:131) for (n,1024) feature vectors."""
        a = np.ascontiguousarray(fv, dtype=np.float64).reshape(-1, 1024)
        out = np.zeros(len(a), np.float64)
        self._check(self.L.str_er_cascade_predict(self.h, which, _np_ptr(a), len(a), _np_ptr(out)))
        return out

    # ---- OCR scorer, SVM half (config 3): OCR::OCR loads the model, chain_run calls svm_predict_probability ----
    def load_svm_model(self, path: str, dim: int = 1800) -> None:
        self._check(self.L.str_er_load_svm_model(self.h, path.encode(), dim))

    def load_svm_model_text(self, text: bytes, dim: int = 1800) -> None:
        self._check(self.L.str_er_load_svm_model_mem(self.h, text, len(text), dim))

    def svm_info(self):
        a, b, d = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.L.str_er_svm_info(self.h, C.byref(a), C.byref(b), C.byref(d)))
        return a.value, b.value, d.value

    def svm_forms(self) -> dict:
        """How the loaded model is evaluated (str_er_svm_forms): support vectors as bytes (exact 8-bit kernel matrix) or as three bf16 pieces; decision values
        summed per class (f64 matrix products) or per vector."""
        a, b = C.c_int32(), C.c_int32()
        self._check(self.L.str_er_svm_forms(self.h, C.byref(a), C.byref(b)))
        return {"bytes": bool(a.value), "class_sums": bool(b.value)}

    def svm_predict_probability(self, x: np.ndarray, want_dec: bool = False):
        """svm_predict_probability (src/svm.cpp:2592-2629) for dense (n, dim) features -> (label, prob[, dec])."""
        a = np.ascontiguousarray(x, dtype=np.float64)
        if a.ndim == 1:
            a = a[None]
        n, dim = a.shape
        k = self.svm_info()[0]
        label = np.zeros(n, np.int32)
        prob = np.zeros((n, k), np.float64)
        dec = np.zeros((n, k * (k - 1) // 2), np.float64) if want_dec else None
        self._check(self.L.str_er_svm_predict_probability(self.h, _np_ptr(a), n, dim, _np_ptr(label), _np_ptr(prob),
                                                          _np_ptr(dec) if want_dec else None))
        return (label, prob, dec) if want_dec else (label, prob)

    def svm_predict_q8(self, q: np.ndarray, want_dec: bool = False):
        """svm_predict_probability for (n, dim) 8-bit numerators over 255 (chain_run's q rows), by the kernels that score boxes -> (label, prob[, dec])."""
        a = np.ascontiguousarray(q, dtype=np.uint8)
        if a.ndim == 1:
            a = a[None]
        n, dim = a.shape
        k = self.svm_info()[0]
        label = np.zeros(n, np.int32)
        prob = np.zeros((n, k), np.float64)
        dec = np.zeros((n, k * (k - 1) // 2), np.float64) if want_dec else None
        self._check(self.L.str_er_svm_predict_probability_q8(self.h, _np_ptr(a), n, dim, _np_ptr(label), _np_ptr(prob),
                                                             _np_ptr(dec) if want_dec else None))
        return (label, prob, dec) if want_dec else (label, prob)

    def chain_run(self, plane: np.ndarray, boxes_xywh: np.ndarray, classify: bool = True, slope=None):
        """OCR::chain_run (src/OCR.cpp:67-140) for every box: (q[n,1800] uint8, label, prob) or q only.
        slope: None (all 0), one number (the Text line's slope, src/ER.cpp:731) or one per box."""
        a = np.ascontiguousarray(plane, dtype=np.uint8)
        b = np.ascontiguousarray(boxes_xywh, dtype=np.int32).reshape(-1, 4)
        n = len(b)
        q = np.zeros((n, 1800), np.uint8)
        label = np.zeros(n, np.int32)
        prob = np.zeros(n, np.float64)
        sl = None
        if slope is not None:
            sl = np.ascontiguousarray(np.broadcast_to(np.asarray(slope, np.float64), (n,)))
        self._check(self.L.str_er_ocr_chain_run_slope(self.h, _np_ptr(a), a.shape[1], a.shape[0], a.shape[1], _np_ptr(b),
                                                      _np_ptr(sl) if sl is not None else None, n,
                                                      _np_ptr(label) if classify else None, _np_ptr(prob) if classify else None, _np_ptr(q)))
        return (q, label, prob) if classify else q

    def set_min_ocr_prob(self, p: float) -> None:
        """MIN_OCR_PROB, ERFilter's last constructor argument (inc/ER.h:113)."""
        self._check(self.L.str_er_set_min_ocr_prob(self.h, float(p)))
        self.min_ocr_prob = float(p)

    # ---- the first consumers of the classified ERs --------------------------------
    def calc_color(self, mask_plane: np.ndarray, color_img: np.ndarray, boxes_xywh: np.ndarray) -> np.ndarray:
        """calc_color (src/ER.cpp:1391-1419) for every box: [n,3] = ER::color1..3 (color_img: H x W x 3 uint8, the Ycrcb Mat)."""
        a = np.ascontiguousarray(mask_plane, dtype=np.uint8)
        ci = np.ascontiguousarray(color_img, dtype=np.uint8)
        if ci.ndim != 3 or ci.shape[2] != 3:
            raise ValueError("color_img must be H x W x 3")
        b = np.ascontiguousarray(boxes_xywh, dtype=np.int32).reshape(-1, 4)
        out = np.zeros((len(b), 3), np.float64)
        self._check(self.L.str_er_calc_color(self.h, _np_ptr(a), a.shape[1], a.shape[0], a.shape[1], _np_ptr(ci), ci.shape[1], ci.shape[0],
                                             ci.shape[1] * 3, _np_ptr(b), len(b), _np_ptr(out)))
        return out

    def er_track(self, cands: np.ndarray, colors: np.ndarray):
        """ERFilter::er_track (src/ER.cpp:530-590) on the ERs of one image: cands (CAND_DTYPE; cls 1 = strong[], 2 = weak[]) and
        their colours [n,3] -> (tracked[n] bool, cx[n], cy[n])."""
        cd = np.ascontiguousarray(cands, dtype=CAND_DTYPE)
        col = np.ascontiguousarray(colors, dtype=np.float64).reshape(-1, 3)
        n = len(cd)
        if len(col) != n:
            raise ValueError("one colour triple per candidate")
        tr = np.zeros(n, np.uint8)
        cx = np.zeros(n, np.int32)
        cy = np.zeros(n, np.int32)
        self._check(self.L.str_er_er_track(self.h, _np_ptr(cd), _np_ptr(col), n, _np_ptr(tr), _np_ptr(cx), _np_ptr(cy)))
        return tr.astype(bool), cx, cy

    def er_grouping(self, cands: np.ndarray, tracks: np.ndarray, overlap_sup: bool = False, inner_sup: bool = False) -> Result:
        """ERFilter::er_grouping(all_er, text, overlap_sup, inner_sup) (src/ER.cpp:612-692) on the ERs of one image
        (cands CAND_DTYPE, tracks TRACK_DTYPE with color1-3 / cx / cy / tracked): Result with .texts / .text_ers / .group_bounds."""
        cd = np.ascontiguousarray(cands, dtype=CAND_DTYPE)
        tr = np.ascontiguousarray(tracks, dtype=TRACK_DTYPE)
        if len(cd) != len(tr):
            raise ValueError("one track record per candidate")
        rh = C.c_void_p()
        self._check(self.L.str_er_er_grouping(self.h, _np_ptr(cd), _np_ptr(tr), len(cd), int(overlap_sup), int(inner_sup), C.byref(rh)))
        return self._collect(rh)

    def make_LBP_hist(self, plane: np.ndarray, boxes_xywh: Optional[np.ndarray] = None, return_tiles: bool = False):
        """ERFilter::make_LBP_hist(input, 2, 24) (src/ER.cpp:789-816).  With no boxes the whole
        plane is the ROI (what the reference's get_lbp_data does, src/utils.cpp:1451-1470)."""
        a = np.ascontiguousarray(plane, dtype=np.uint8)
        if boxes_xywh is None:
            boxes_xywh = np.array([[0, 0, a.shape[1], a.shape[0]]], np.int32)
        b = np.ascontiguousarray(boxes_xywh, dtype=np.int32).reshape(-1, 4)
        n = len(b)
        hist = np.zeros((n, 1024), np.float64)
        tiles = np.zeros((n, 26, 26), np.uint8) if return_tiles else None
        self._check(self.L.str_er_lbp_hist(self.h, _np_ptr(a), a.shape[1], a.shape[0], a.shape[1], _np_ptr(b), n,
                                           _np_ptr(hist), _np_ptr(tiles) if return_tiles else None))
        return (hist, tiles) if return_tiles else hist

    def calc_LBP(self, plane: np.ndarray, boxes_xywh: Optional[np.ndarray] = None) -> np.ndarray:
        """ERFilter::calc_LBP(input, 24) (inc/ER.h:134, src/ER.cpp:819-845): the 24x24 Mean-LBP code map of every box
        (of the whole plane with no boxes, which is how OCR::lbp_run calls it, src/OCR.cpp:37-39)."""
        a = np.ascontiguousarray(plane, dtype=np.uint8)
        if boxes_xywh is None:
            boxes_xywh = np.array([[0, 0, a.shape[1], a.shape[0]]], np.int32)
        b = np.ascontiguousarray(boxes_xywh, dtype=np.int32).reshape(-1, 4)
        out = np.zeros((len(b), 24, 24), np.uint8)
        self._check(self.L.str_er_calc_lbp(self.h, _np_ptr(a), a.shape[1], a.shape[0], a.shape[1], _np_ptr(b), len(b), _np_ptr(out)))
        return out

    def resize_plane(self, src: np.ndarray, dw: int, dh: int) -> np.ndarray:
        a = np.ascontiguousarray(src, dtype=np.uint8)
        out = np.empty((dh, dw), np.uint8)
        self._check(self.L.str_er_resize_plane(self.h, _np_ptr(a), a.shape[1], a.shape[0], a.shape[1], _np_ptr(out), dw, dh))
        return out

    def pyr_level_plane(self, src: np.ndarray, dw: int, dh: int, rows: int = 0, sstride: Optional[int] = None, dstride: Optional[int] = None):
        """One pyramid level of a plane through launch_pyr_level's dispatch: (plane, True when k_pyr_level ran / False when k_resize did).
        rows: 0 the library's choice, else 8 / 16 / 32.  sstride / dstride: the row strides of the planes on the device (default: the widths)."""
        sh, sw = src.shape
        sstride, dstride = sstride or sw, dstride or dw
        a = np.zeros((sh, sstride), np.uint8)
        a[:, :sw] = src
        out = np.zeros((dh, dstride), np.uint8)
        used = C.c_int32(-1)
        fn = self.L.str_er_pyr_level_plane        # (bound here: STR_ER_LIB may name a build from before this entry point)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_int32)]
        self._check(fn(self.h, _np_ptr(a), sw, sh, sstride, _np_ptr(out), dw, dh, dstride, rows, C.byref(used)))
        return np.ascontiguousarray(out[:, :dw]), bool(used.value)

    def tie_stats(self) -> dict:
        """Exact NMS ties: planes whose flood order had to be walked on a host core so far, the host time that took, pool size."""
        n, ms, th = C.c_uint64(), C.c_double(), C.c_int32()
        self._check(self.L.str_er_tie_stats(self.h, C.byref(n), C.byref(ms), C.byref(th)))
        return {"planes_walked": int(n.value), "walk_ms_total": float(ms.value), "host_threads": int(th.value)}

    def workspace_bytes(self) -> int:
        return int(self.L.str_er_workspace_bytes(self.h))


def _owned(ptr, n: int, dtype) -> np.ndarray:
    """n records of dtype at ptr (a table of a result), copied into an array of its own; an empty array when n = 0."""
    dtype = np.dtype(dtype)
    if not n:
        return np.zeros(0, dtype)
    return np.frombuffer((C.c_char * (dtype.itemsize * n)).from_address(ptr), dtype=dtype).copy()


def _lexicon_bytes(words):
    """(bytes back to back, int32 offsets of n + 1 values) of a sequence of strings or bytes."""
    enc = [w.encode("latin-1", "replace") if isinstance(w, str) else bytes(w) for w in words]
    off = np.zeros(len(enc) + 1, np.int64)
    np.cumsum([len(e) for e in enc], out=off[1:])
    if len(off) and off[-1] > 2 ** 31 - 1:
        raise ValueError("lexicon too large")
    return b"".join(enc), off.astype(np.int32)


def _lexicon_strings(words) -> tuple:
    return tuple(w if isinstance(w, str) else bytes(w).decode("latin-1") for w in words)


def _set_lexicon(L, ctx, words, fold_case: bool) -> int:
    words = list(words)
    raw, off = _lexicon_bytes(words)
    buf = np.frombuffer(raw, np.uint8) if raw else np.zeros(1, np.uint8)
    return L.str_er_set_lexicon(ctx, _np_ptr(buf), _np_ptr(off), len(words), LEXICON_FOLD_CASE if fold_case else 0)


def cost_thresholds() -> np.ndarray:
    """str_er_cost_thresholds (pure host): the 255 thresholds T of str_er_word_match."""
    out = np.zeros(255, np.float64)
    load_library().str_er_cost_thresholds(_np_ptr(out))
    return out


def prob_costs(prob: np.ndarray, labels, fold: bool = False) -> np.ndarray:
    """str_er_prob_costs (pure host): the cost rows (n, 65) uint8 of (n, k) class probabilities of a model with the k labels."""
    p = np.ascontiguousarray(prob, dtype=np.float64)
    lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
    if p.ndim != 2 or p.shape[1] != len(lab):
        raise ValueError("prob must be (n, k) with k labels")
    out = np.zeros((len(p), 65), np.uint8)
    rc = load_library().str_er_prob_costs(_np_ptr(p) if p.size else None, len(p), len(lab), _np_ptr(lab) if len(lab) else None, 1 if fold else 0,
                                          _np_ptr(out) if len(p) else None)
    if rc != 0:
        raise StrErError(rc, "str_er_prob_costs")
    return out


def match_words_host(costs: np.ndarray, first_run, n_runs_of_word, words, fold_case: bool = True, ins: int = 64, dele: int = 64, band: int = 2) -> np.ndarray:
    """str_er_match_words_host (pure host, one thread): ERFilter.match_words with the lexicon and the parameters as arguments."""
    cs = np.ascontiguousarray(costs, dtype=np.uint8).reshape(-1, 65)
    fr = np.ascontiguousarray(first_run, dtype=np.int32).reshape(-1)
    no = np.ascontiguousarray(n_runs_of_word, dtype=np.int32).reshape(-1)
    words = list(words)
    raw, off = _lexicon_bytes(words)
    buf = np.frombuffer(raw, np.uint8) if raw else np.zeros(1, np.uint8)
    out = np.zeros(max(1, len(fr)), WORD_MATCH_DTYPE)
    rc = load_library().str_er_match_words_host(_np_ptr(cs) if len(cs) else None, len(cs), _np_ptr(fr) if len(fr) else None, _np_ptr(no) if len(no) else None,
                                                len(fr), _np_ptr(buf), _np_ptr(off), len(words), LEXICON_FOLD_CASE if fold_case else 0, int(ins), int(dele),
                                                int(band), _np_ptr(out))
    if rc != 0:
        raise StrErError(rc, "str_er_match_words_host")
    return out[:len(fr)]


def _bigram_table(table) -> np.ndarray:
    t = np.ascontiguousarray(table, dtype=np.uint8)
    if t.size != 66 * 66:
        raise ValueError("a bigram table is (66, 66) uint8")
    return t.reshape(66, 66)


def _decode_args(costs, first_run, n_runs_of_word):
    cs = np.ascontiguousarray(costs, dtype=np.uint8).reshape(-1, 65)
    fr = np.ascontiguousarray(first_run, dtype=np.int32).reshape(-1)
    no = np.ascontiguousarray(n_runs_of_word, dtype=np.int32).reshape(-1)
    if len(fr) != len(no):
        raise ValueError("first_run and n_runs_of_word: one value per word each")
    n = max(1, len(fr))
    return cs, fr, no, np.zeros(n, WORD_DECODE_DTYPE), np.full((n, 64), 0xFF, np.uint8), np.full((n, 64), 0xFF, np.uint8)


def _line_decode_args(costs, gaps, first_row, n_rows):
    cs = np.ascontiguousarray(costs, dtype=np.uint8).reshape(-1, 65)
    gp = np.ascontiguousarray(gaps, dtype=np.uint8).reshape(-1, 2)
    fr = np.ascontiguousarray(first_row, dtype=np.int32).reshape(-1)
    no = np.ascontiguousarray(n_rows, dtype=np.int32).reshape(-1)
    if len(fr) != len(no):
        raise ValueError("first_row and n_rows: one value per line each")
    if len(gp) != len(cs):
        raise ValueError("gaps: one (join, break) pair per cost row")
    n = max(1, len(cs))
    return (cs, gp, fr, no, np.zeros(max(1, len(fr)), LINE_DECODE_DTYPE), np.full(3 * n, 0xFF, np.uint8), np.full(3 * n, 0xFFFF, np.uint16),
            np.full(n, -1, np.int32))


def _line_margin_args(costs, gaps, first_row, n_rows, want_marginals):
    cs, gp, fr, no = _line_decode_args(costs, gaps, first_row, n_rows)[:4]
    n = max(1, len(cs))
    return (cs, gp, fr, no, np.full(max(1, len(fr)), -1, LINE_MARGIN_DTYPE), np.full(n, -1, np.int32), np.full(n, 0xFF, np.uint8), np.full(n, 0xFF, np.uint8),
            np.full(n, -1, np.int32), np.full(n, 0xFF, np.uint8), np.full((n if want_marginals else 1, 68), -1, np.int32))


def _line_margin_out(n, n_lines, out, rm, rr, ra, gm, gv, mg, want_marginals):
    res = (out[:n_lines], rm[:n], rr[:n], ra[:n], gm[:n], gv[:n])
    return res + (mg[:n],) if want_marginals else res


def line_margins_host(costs: np.ndarray, gaps, first_row, n_rows, table, ins: int = 0, dele: int = 0, want_marginals: bool = False):
    """str_er_line_margins_host (pure host, one thread): ERFilter.line_margins with the table and the parameters as arguments."""
    cs, gp, fr, no, out, rm, rr, ra, gm, gv, mg = _line_margin_args(costs, gaps, first_row, n_rows, want_marginals)
    opt = lambda a: _np_ptr(a) if len(a) else None
    rc = load_library().str_er_line_margins_host(opt(cs), len(cs), opt(gp), opt(fr), opt(no), len(fr), _np_ptr(_bigram_table(table)), int(ins), int(dele),
                                                 _np_ptr(out), _np_ptr(rm), _np_ptr(rr), _np_ptr(ra), _np_ptr(gm), _np_ptr(gv), _np_ptr(mg) if want_marginals else None)
    if rc != 0:
        raise StrErError(rc, "str_er_line_margins_host")
    return _line_margin_out(len(cs), len(fr), out, rm, rr, ra, gm, gv, mg, want_marginals)


def decode_lines_host(costs: np.ndarray, gaps, first_row, n_rows, table, ins: int = 0, dele: int = 0):
    """str_er_decode_lines_host (pure host, one thread): ERFilter.decode_lines with the table and the parameters as arguments."""
    cs, gp, fr, no, out, ch, sr, wr = _line_decode_args(costs, gaps, first_row, n_rows)
    opt = lambda a: _np_ptr(a) if len(a) else None
    rc = load_library().str_er_decode_lines_host(opt(cs), len(cs), opt(gp), opt(fr), opt(no), len(fr), _np_ptr(_bigram_table(table)), int(ins), int(dele),
                                                 _np_ptr(out), _np_ptr(ch), _np_ptr(sr), _np_ptr(wr))
    if rc != 0:
        raise StrErError(rc, "str_er_decode_lines_host")
    return out[:len(fr)], ch[:3 * len(cs)], sr[:3 * len(cs)], wr[:len(cs)]


def line_gap_costs(runs, first_row, n_rows_of_line, colmax, num: int = 1, den: int = 3, weight: int = 16, row_run=None, n_rows=None) -> np.ndarray:
    """str_er_line_gap_costs (pure host): the (join, break) costs of str_er_line_decode from the geometry, (n_rows, 2) uint8.  Line t has
    the rows [first_row[t], first_row[t] + n_rows_of_line[t]) and the colmax colmax[t]; row r is the run row_run[r] of runs
    (LINE_RUN_DTYPE; x0 and x1 are read), or run r where row_run is None; n_rows: the rows there are (default: one per run, or per
    entry of row_run)."""
    rs = np.ascontiguousarray(runs, dtype=LINE_RUN_DTYPE).reshape(-1)
    fr = np.ascontiguousarray(first_row, dtype=np.int32).reshape(-1)
    no = np.ascontiguousarray(n_rows_of_line, dtype=np.int32).reshape(-1)
    cm = np.ascontiguousarray(colmax, dtype=np.uint32).reshape(-1)
    rr = None if row_run is None else np.ascontiguousarray(row_run, dtype=np.int32).reshape(-1)
    if not len(fr) == len(no) == len(cm):
        raise ValueError("first_row, n_rows_of_line and colmax: one value per line each")
    n = int(n_rows) if n_rows is not None else len(rs) if rr is None else len(rr)
    if rr is not None and len(rr) != n:
        raise ValueError("row_run: one run per row")
    out = np.zeros((max(1, n), 2), np.uint8)
    opt = lambda a: _np_ptr(a) if a is not None and len(a) else None
    rc = load_library().str_er_line_gap_costs(opt(rs), len(rs), opt(rr), n, opt(fr), opt(no), opt(cm), len(fr), int(num), int(den), int(weight), _np_ptr(out))
    if rc != 0:
        raise StrErError(rc, "str_er_line_gap_costs")
    return out[:n]


def _margin_args(costs, first_run, n_runs_of_word, want_marginals):
    cs, fr, no = _decode_args(costs, first_run, n_runs_of_word)[:3]
    n = max(1, len(fr))
    return (cs, fr, no, np.full(n, -1, np.int32).repeat(4).view(WORD_MARGIN_DTYPE), np.full((n, 32), -1, np.int32), np.full((n, 32), 0xFF, np.uint8),
            np.full((n, 32), 0xFF, np.uint8), np.full((n, 32, 66), -1, np.int32) if want_marginals else None)


def bigram_from_probs(tp, start=None, end=None) -> np.ndarray:
    """str_er_bigram_from_probs (pure host): the (66, 66) uint8 table of (65, 65) probabilities tp[a][b] = P(b after a), with the
    boundary row from start (65) and the boundary column from end (65), 0 where they are None."""
    t = np.ascontiguousarray(tp, dtype=np.float64)
    if t.size != 65 * 65:
        raise ValueError("tp must be (65, 65)")
    st = None if start is None else np.ascontiguousarray(start, dtype=np.float64).reshape(65)
    en = None if end is None else np.ascontiguousarray(end, dtype=np.float64).reshape(65)
    out = np.zeros((66, 66), np.uint8)
    rc = load_library().str_er_bigram_from_probs(_np_ptr(t), None if st is None else _np_ptr(st), None if en is None else _np_ptr(en), _np_ptr(out))
    if rc != 0:
        raise StrErError(rc, "str_er_bigram_from_probs")
    return out


_OCR_ALPHABET = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz&()"


def bigram_from_words(words, alpha: float = 1.0) -> np.ndarray:
    """A (66, 66) uint8 table from a word list: the counts of every character pair of the words, with the word boundary as the
    66th symbol (before the first and after the last character), plus alpha everywhere, every row normalised to probabilities, then
    cost() of str_er_word_match.  The entry [65][65] (the empty word) is 0.  Characters outside the alphabet of ocr_char raise."""
    label = {ch: a for a, ch in enumerate(_OCR_ALPHABET)}
    cnt = np.full((66, 66), float(alpha), np.float64)
    for w in words:
        w = w if isinstance(w, str) else bytes(w).decode("latin-1")
        prev = 65
        for ch in w:
            if ch not in label:
                raise ValueError(f"bigram_from_words: {ch!r} is outside the alphabet")
            cnt[prev, label[ch]] += 1
            prev = label[ch]
        if w:
            cnt[prev, 65] += 1
    tot = cnt.sum(axis=1, keepdims=True)
    p = np.divide(cnt, tot, out=np.zeros_like(cnt), where=tot > 0)
    return bigram_from_probs(p[:65, :65], p[65, :65], p[:65, 65])


def load_tp_table(path: str) -> np.ndarray:
    """The (66, 66) uint8 table of a text file of 65 x 65 numbers in row order (the layout of the reference's
    dictionary/tp_table.txt), taken as P(b after a); the boundary row and column are 0.  Whether the reference's file holds such
    probabilities has not been checked (str_er_word_decode, Limits)."""
    with open(path) as fh:
        v = np.array(fh.read().split(), dtype=np.float64)
    if v.size != 65 * 65:
        raise ValueError(f"{path}: expected 65 x 65 numbers, found {v.size}")
    return bigram_from_probs(v.reshape(65, 65))


def cuts_from_counts(counts, H: int, num: int = 1, den: int = 4):
    """str_er_cuts_from_counts (pure host): the kept cut columns of one run of height H with the column counts `counts`, relative to the
    run and ascending, and the threshold: (list of cuts, thr)."""
    n = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
    cut = np.zeros(3, np.int32)
    k, thr = C.c_int32(), C.c_uint32()
    rc = load_library().str_er_cuts_from_counts(_np_ptr(n) if len(n) else None, len(n), int(H), int(num), int(den), _np_ptr(cut), C.byref(k), C.byref(thr))
    if rc != 0:
        raise StrErError(rc, "str_er_cuts_from_counts")
    return [int(v) for v in cut[:k.value]], int(thr.value)


def _split_args(splits, run_costs, piece_costs, first_run, n_runs_of_word):
    sp = np.ascontiguousarray(splits, dtype=RUN_SPLIT_DTYPE).reshape(-1)
    rc = np.ascontiguousarray(run_costs, dtype=np.uint8).reshape(-1, 65)
    pc = np.ascontiguousarray(piece_costs, dtype=np.uint8).reshape(-1, 65)
    fr = np.ascontiguousarray(first_run, dtype=np.int32).reshape(-1)
    no = np.ascontiguousarray(n_runs_of_word, dtype=np.int32).reshape(-1)
    if len(sp) != len(rc) or len(fr) != len(no):
        raise ValueError("splits and run_costs need one row per run, first_run and n_runs_of_word one entry per word")
    cap = int(min(4 * int(no.astype(np.int64).clip(0).sum()), 2 ** 31 - 1))          # (a run has at most 4 parts)
    ws = np.zeros(max(1, len(fr)), WORD_SPLIT_DTYPE)
    parts = np.zeros(max(1, cap), SPLIT_PART_DTYPE)
    rows = np.zeros((max(1, cap), 65), np.uint8)
    n = C.c_int32()
    p = lambda a: _np_ptr(a) if len(a) else None
    return ((p(sp), len(sp), p(rc), p(pc), len(pc), p(fr), p(no), len(fr)), (_np_ptr(ws), _np_ptr(parts), cap, C.byref(n), _np_ptr(rows)),
            (sp, rc, pc, fr, no), ws, parts, rows, n)


def _split_out(a):
    ws, parts, rows, n = a[3], a[4], a[5], a[6]
    return ws[:len(a[2][3])], parts[:n.value].copy(), rows[:n.value].copy()


def split_words_host(splits, run_costs, piece_costs, first_run, n_runs_of_word, split_cost: int = 8):
    """str_er_split_words_host (pure host, one thread): ERFilter.split_words with SPLIT as an argument."""
    a = _split_args(splits, run_costs, piece_costs, first_run, n_runs_of_word)
    rc = load_library().str_er_split_words_host(*a[0], int(split_cost), *a[1])
    if rc != 0:
        raise StrErError(rc, "str_er_split_words_host")
    return _split_out(a)


def _lattice_args(splits, run_costs, piece_costs, first_run, n_runs_of_word):
    sp = np.ascontiguousarray(splits, dtype=RUN_SPLIT_DTYPE).reshape(-1)
    rc = np.ascontiguousarray(run_costs, dtype=np.uint8).reshape(-1, 65)
    pc = np.ascontiguousarray(piece_costs, dtype=np.uint8).reshape(-1, 65)
    fr = np.ascontiguousarray(first_run, dtype=np.int32).reshape(-1)
    no = np.ascontiguousarray(n_runs_of_word, dtype=np.int32).reshape(-1)
    if len(sp) != len(rc) or len(fr) != len(no):
        raise ValueError("splits and run_costs need one row per run, first_run and n_runs_of_word one entry per word")
    cap = int(min(4 * int(no.astype(np.int64).clip(0).sum()), 2 ** 31 - 1))          # (a run has at most 4 parts)
    dec = np.zeros(max(1, len(fr)), LATTICE_DECODE_DTYPE)
    ch = np.full((max(1, len(fr)), 64), 0xFF, np.uint8)
    sr = np.full((max(1, len(fr)), 64), 0xFF, np.uint8)
    parts = np.zeros(max(1, cap), SPLIT_PART_DTYPE)
    n = C.c_int32()
    p = lambda a: _np_ptr(a) if len(a) else None
    return ((p(sp), len(sp), p(rc), p(pc), len(pc), p(fr), p(no), len(fr)), (_np_ptr(dec), _np_ptr(ch), _np_ptr(sr), _np_ptr(parts), cap, C.byref(n)),
            (sp, rc, pc, fr, no), dec, ch, sr, parts, n)


def _lattice_out(a):
    nw = len(a[2][3])
    return a[3][:nw], a[4][:nw], a[5][:nw], a[6][:a[7].value].copy()


def _lattice_margin_args(splits, run_costs, piece_costs, first_run, n_runs_of_word, want_edges, want_marginals):
    a = _lattice_args(splits, run_costs, piece_costs, first_run, n_runs_of_word)
    n = max(1, len(a[2][3]))
    rec = np.full(n, -1, np.int32).repeat(8).view(LATTICE_MARGIN_DTYPE)
    rec["n_edges"] = 0
    return a, (rec, np.full((n, 32), -1, np.int32), np.full((n, 32), -1, np.int32), np.full((n, 32), 0xFF, np.uint8), np.full((n, 32), 0xFF, np.uint8),
               np.full((n, 32), 0xFF, np.uint8), np.full((n, 32, 4), -1, np.int32) if want_edges else None,
               np.full((n, 32, 4, 66), -1, np.int32) if want_marginals else None)


def lattice_margins_host(splits, run_costs, piece_costs, first_run, n_runs_of_word, table, ins: int = 0, dele: int = 0, split_cost: int = 8,
                         want_edges: bool = False, want_marginals: bool = False):
    """str_er_lattice_margins_host (pure host, one thread): ERFilter.lattice_margins with the table and the parameters as arguments."""
    a, out = _lattice_margin_args(splits, run_costs, piece_costs, first_run, n_runs_of_word, want_edges, want_marginals)
    tb = _bigram_table(table)
    rc = load_library().str_er_lattice_margins_host(*a[0], int(split_cost), _np_ptr(tb), int(ins), int(dele), *[None if v is None else _np_ptr(v) for v in out])
    if rc != 0:
        raise StrErError(rc, "str_er_lattice_margins_host")
    return tuple(None if v is None else v[:len(a[2][3])] for v in out)


def lattice_decode_words_host(splits, run_costs, piece_costs, first_run, n_runs_of_word, table, ins: int = 0, dele: int = 0, split_cost: int = 8):
    """str_er_lattice_decode_words_host (pure host, one thread): ERFilter.lattice_decode_words with the table and the parameters as arguments."""
    a = _lattice_args(splits, run_costs, piece_costs, first_run, n_runs_of_word)
    tb = _bigram_table(table)
    rc = load_library().str_er_lattice_decode_words_host(*a[0], int(split_cost), _np_ptr(tb), int(ins), int(dele), *a[1])
    if rc != 0:
        raise StrErError(rc, "str_er_lattice_decode_words_host")
    return _lattice_out(a)


def _line_lattice_args(splits, run_costs, piece_costs, gaps, first_run, n_runs_of_line):
    sp = np.ascontiguousarray(splits, dtype=RUN_SPLIT_DTYPE).reshape(-1)
    rc = np.ascontiguousarray(run_costs, dtype=np.uint8).reshape(-1, 65)
    pc = np.ascontiguousarray(piece_costs, dtype=np.uint8).reshape(-1, 65)
    gp = np.ascontiguousarray(gaps, dtype=np.uint8).reshape(-1, 2)
    fr = np.ascontiguousarray(first_run, dtype=np.int32).reshape(-1)
    no = np.ascontiguousarray(n_runs_of_line, dtype=np.int32).reshape(-1)
    if len(sp) != len(rc) or len(gp) != len(rc) or len(fr) != len(no):
        raise ValueError("splits, run_costs and gaps need one row per run, first_run and n_runs_of_line one entry per line")
    atoms = int((sp["n_cuts"].astype(np.int64).clip(0, 3) + 1).sum())          # (the slices of all runs; a line has at most as many parts)
    cap = int(min(atoms, 2 ** 31 - 1))
    dec = np.zeros(max(1, len(fr)), LINE_LATTICE_DECODE_DTYPE)
    ch = np.full(max(1, 3 * atoms), 0xFF, np.uint8)
    sr = np.full(max(1, 3 * atoms), 0xFFFF, np.uint16)
    parts = np.zeros(max(1, cap), SPLIT_PART_DTYPE)
    wop = np.full(max(1, cap), -1, np.int32)
    n = C.c_int32()
    p = lambda a: _np_ptr(a) if len(a) else None
    return ((p(sp), len(sp), p(rc), p(pc), len(pc), p(gp), p(fr), p(no), len(fr)), (_np_ptr(dec), _np_ptr(ch), _np_ptr(sr), _np_ptr(parts), cap, C.byref(n), _np_ptr(wop)),
            (sp, rc, pc, gp, fr, no), dec, ch, sr, parts, wop, n, atoms)


def _line_lattice_out(a):
    nl, atoms, n = len(a[2][4]), a[9], a[8].value
    return a[3][:nl], a[4][:3 * atoms], a[5][:3 * atoms], a[6][:n].copy(), a[7][:n].copy()


def lattice_decode_lines_host(splits, run_costs, piece_costs, gaps, first_run, n_runs_of_line, table, ins: int = 0, dele: int = 0, split_cost: int = 8):
    """str_er_lattice_decode_lines_host (pure host, one thread): ERFilter.lattice_decode_lines with the table and the parameters as arguments."""
    a = _line_lattice_args(splits, run_costs, piece_costs, gaps, first_run, n_runs_of_line)
    tb = _bigram_table(table)
    rc = load_library().str_er_lattice_decode_lines_host(*a[0], int(split_cost), _np_ptr(tb), int(ins), int(dele), *a[1])
    if rc != 0:
        raise StrErError(rc, "str_er_lattice_decode_lines_host")
    return _line_lattice_out(a)


def line_lattice_node_slots(splits, first_run):
    """The node slot of every line of lattice_decode_lines: the atoms of all runs before its first run (its labels begin at 3 * slot)."""
    sp = np.ascontiguousarray(splits, dtype=RUN_SPLIT_DTYPE).reshape(-1)
    at = np.concatenate([[0], np.cumsum(sp["n_cuts"].astype(np.int64).clip(0, 3) + 1)])
    return at[np.asarray(first_run, np.int64).reshape(-1)]


def _lattice_match_args(splits, run_costs, piece_costs, first_run, n_runs_of_word):
    sp = np.ascontiguousarray(splits, dtype=RUN_SPLIT_DTYPE).reshape(-1)
    rc = np.ascontiguousarray(run_costs, dtype=np.uint8).reshape(-1, 65)
    pc = np.ascontiguousarray(piece_costs, dtype=np.uint8).reshape(-1, 65)
    fr = np.ascontiguousarray(first_run, dtype=np.int32).reshape(-1)
    no = np.ascontiguousarray(n_runs_of_word, dtype=np.int32).reshape(-1)
    if len(sp) != len(rc) or len(fr) != len(no):
        raise ValueError("splits and run_costs need one row per run, first_run and n_runs_of_word one entry per word")
    cap = int(min(4 * int(no.astype(np.int64).clip(0).sum()), 2 ** 31 - 1))          # (a run has at most 4 parts)
    rec = np.zeros(max(1, len(fr)), LATTICE_MATCH_DTYPE)
    sr = np.full((max(1, len(fr)), 32), 0xFF, np.uint8)
    parts = np.zeros(max(1, cap), SPLIT_PART_DTYPE)
    n = C.c_int32()
    p = lambda a: _np_ptr(a) if len(a) else None
    return ((p(sp), len(sp), p(rc), p(pc), len(pc), p(fr), p(no), len(fr)), (_np_ptr(rec), _np_ptr(sr), _np_ptr(parts), cap, C.byref(n)),
            (sp, rc, pc, fr, no), rec, sr, parts, n)


def _lattice_match_out(a):
    nw = len(a[2][3])
    return a[3][:nw], a[4][:nw], a[5][:a[6].value].copy()


def lattice_match_words_host(splits, run_costs, piece_costs, first_run, n_runs_of_word, words, fold_case: bool = True, ins: int = 64, dele: int = 64,
                             band: int = 2, split_cost: int = 8):
    """str_er_lattice_match_words_host (pure host, one thread): ERFilter.lattice_match_words with the lexicon and the parameters as arguments."""
    a = _lattice_match_args(splits, run_costs, piece_costs, first_run, n_runs_of_word)
    words = list(words)
    raw, off = _lexicon_bytes(words)
    buf = np.frombuffer(raw, np.uint8) if raw else np.zeros(1, np.uint8)
    rc = load_library().str_er_lattice_match_words_host(*a[0], _np_ptr(buf), _np_ptr(off), len(words), LEXICON_FOLD_CASE if fold_case else 0, int(ins), int(dele),
                                                        int(band), int(split_cost), *a[1])
    if rc != 0:
        raise StrErError(rc, "str_er_lattice_match_words_host")
    return _lattice_match_out(a)


def _lattice_track_args(splits, run_costs, piece_costs, first_run, n_runs_of_word, track_first, track_count, members):
    sp = np.ascontiguousarray(splits, dtype=RUN_SPLIT_DTYPE).reshape(-1)
    rc = np.ascontiguousarray(run_costs, dtype=np.uint8).reshape(-1, 65)
    pc = np.ascontiguousarray(piece_costs, dtype=np.uint8).reshape(-1, 65)
    fr = np.ascontiguousarray(first_run, dtype=np.int32).reshape(-1)
    no = np.ascontiguousarray(n_runs_of_word, dtype=np.int32).reshape(-1)
    tf = np.ascontiguousarray(track_first, dtype=np.int32).reshape(-1)
    tc = np.ascontiguousarray(track_count, dtype=np.int32).reshape(-1)
    mem = np.ascontiguousarray(members, dtype=np.int32).reshape(-1)
    if len(sp) != len(rc) or len(fr) != len(no) or len(tf) != len(tc):
        raise ValueError("splits and run_costs need one row per run, first_run and n_runs_of_word one entry per word, track_first and track_count one per track")
    cap = int(min(32 * len(mem), 2 ** 31 - 1))          # (a usable member has at most 32 parts)
    out = np.zeros(max(1, len(tf)), TRACK_MATCH_DTYPE)
    mrec = np.zeros(max(1, len(mem)), LATTICE_TRACK_MEMBER_DTYPE)
    sr = np.full((max(1, len(mem)), 32), 0xFF, np.uint8)
    parts = np.zeros(max(1, cap), SPLIT_PART_DTYPE)
    n = C.c_int32()
    p = lambda a: _np_ptr(a) if len(a) else None
    return ((p(sp), len(sp), p(rc), p(pc), len(pc), p(fr), p(no), len(fr), p(tf), p(tc), p(mem), len(mem), len(tf)),
            (_np_ptr(out), _np_ptr(mrec), _np_ptr(sr), _np_ptr(parts), cap, C.byref(n)), (sp, rc, pc, fr, no, tf, tc, mem), out, mrec, sr, parts, n)


def _lattice_track_out(a):
    nt, nm = len(a[2][5]), len(a[2][7])
    return a[3][:nt], a[4][:nm], a[5][:nm], a[6][:a[7].value].copy()


def _lattice_track_decode_args(splits, run_costs, piece_costs, first_run, n_runs_of_word, track_first, track_count, members):
    a = _lattice_track_args(splits, run_costs, piece_costs, first_run, n_runs_of_word, track_first, track_count, members)
    nt = len(a[2][5])
    return a, np.zeros(max(1, nt), TRACK_DECODE_DTYPE), np.full((max(1, nt), 32), 0xFF, np.uint8)


def _lattice_track_decode_out(a, out, ch):
    nt, nm = len(a[2][5]), len(a[2][7])
    return out[:nt], ch[:nt], a[4][:nm], a[5][:nm], a[6][:a[7].value].copy()


def lattice_decode_tracks_host(splits, run_costs, piece_costs, first_run, n_runs_of_word, track_first, track_count, members, table, dec_ins: int = 0,
                               dec_dele: int = 0, ins: int = 64, dele: int = 64, rounds: int = 8, split_cost: int = 8):
    """str_er_lattice_decode_tracks_host (pure host, one thread): ERFilter.lattice_decode_tracks with the table, the lattice decoder's INS /
    DEL, the track decode's parameters and SPLIT as arguments."""
    a, out, ch = _lattice_track_decode_args(splits, run_costs, piece_costs, first_run, n_runs_of_word, track_first, track_count, members)
    rc = load_library().str_er_lattice_decode_tracks_host(*a[0], _np_ptr(_bigram_table(table)), int(dec_ins), int(dec_dele), int(ins), int(dele), int(rounds),
                                                          int(split_cost), _np_ptr(out), _np_ptr(ch), *a[1][1:])
    if rc != 0:
        raise StrErError(rc, "str_er_lattice_decode_tracks_host")
    return _lattice_track_decode_out(a, out, ch)


def lattice_match_tracks_host(splits, run_costs, piece_costs, first_run, n_runs_of_word, track_first, track_count, members, words, fold_case: bool = True,
                              ins: int = 64, dele: int = 64, band: int = 2, split_cost: int = 8):
    """str_er_lattice_match_tracks_host (pure host, one thread): ERFilter.lattice_match_tracks with the lexicon and the parameters as arguments."""
    a = _lattice_track_args(splits, run_costs, piece_costs, first_run, n_runs_of_word, track_first, track_count, members)
    words = list(words)
    raw, off = _lexicon_bytes(words)
    buf = np.frombuffer(raw, np.uint8) if raw else np.zeros(1, np.uint8)
    rc = load_library().str_er_lattice_match_tracks_host(*a[0], _np_ptr(buf), _np_ptr(off), len(words), LEXICON_FOLD_CASE if fold_case else 0, int(ins), int(dele),
                                                         int(band), int(split_cost), *a[1])
    if rc != 0:
        raise StrErError(rc, "str_er_lattice_match_tracks_host")
    return _lattice_track_out(a)


def decode_tracks_host(costs: np.ndarray, first_run, n_runs_of_word, track_first, track_count, members, table, dec_ins: int = 0, dec_dele: int = 0,
                       ins: int = 64, dele: int = 64, rounds: int = 8):
    """str_er_decode_tracks_host (pure host, one thread): ERFilter.decode_tracks with the table, the decoder's INS / DEL and the
    parameters as arguments."""
    cs, fr, no, tf, tc, mem = _track_args(costs, first_run, n_runs_of_word, track_first, track_count, members)
    out = np.zeros(max(1, len(tf)), TRACK_DECODE_DTYPE)
    ch = np.full((max(1, len(tf)), 32), 0xFF, np.uint8)
    mc = np.zeros(max(1, len(mem)), np.int32)
    opt = lambda a: _np_ptr(a) if len(a) else None
    rc = load_library().str_er_decode_tracks_host(opt(cs), len(cs), opt(fr), opt(no), len(fr), opt(tf), opt(tc), opt(mem), len(mem), len(tf),
                                                  _np_ptr(_bigram_table(table)), int(dec_ins), int(dec_dele), int(ins), int(dele), int(rounds),
                                                  _np_ptr(out), _np_ptr(ch), _np_ptr(mc))
    if rc != 0:
        raise StrErError(rc, "str_er_decode_tracks_host")
    return out[:len(tf)], ch[:len(tf)], mc[:len(mem)]


def decode_words_host(costs: np.ndarray, first_run, n_runs_of_word, table, ins: int = 0, dele: int = 0):
    """str_er_decode_words_host (pure host, one thread): ERFilter.decode_words with the table and the parameters as arguments."""
    cs, fr, no, out, ch, sr = _decode_args(costs, first_run, n_runs_of_word)
    rc = load_library().str_er_decode_words_host(_np_ptr(cs) if len(cs) else None, len(cs), _np_ptr(fr) if len(fr) else None, _np_ptr(no) if len(no) else None,
                                                 len(fr), _np_ptr(_bigram_table(table)), int(ins), int(dele), _np_ptr(out), _np_ptr(ch), _np_ptr(sr))
    if rc != 0:
        raise StrErError(rc, "str_er_decode_words_host")
    return out[:len(fr)], ch[:len(fr)], sr[:len(fr)]


def word_margins_host(costs: np.ndarray, first_run, n_runs_of_word, table, ins: int = 0, dele: int = 0, want_marginals: bool = False):
    """str_er_word_margins_host (pure host, one thread): ERFilter.word_margins with the table and the parameters as arguments."""
    cs, fr, no, out, rm, rr, ra, mg = _margin_args(costs, first_run, n_runs_of_word, want_marginals)
    rc = load_library().str_er_word_margins_host(_np_ptr(cs) if len(cs) else None, len(cs), _np_ptr(fr) if len(fr) else None, _np_ptr(no) if len(no) else None,
                                                 len(fr), _np_ptr(_bigram_table(table)), int(ins), int(dele), _np_ptr(out), _np_ptr(rm), _np_ptr(rr), _np_ptr(ra),
                                                 None if mg is None else _np_ptr(mg))
    if rc != 0:
        raise StrErError(rc, "str_er_word_margins_host")
    return out[:len(fr)], rm[:len(fr)], rr[:len(fr)], ra[:len(fr)], None if mg is None else mg[:len(fr)]


def _want_flags(*, nodes=False, masks=False, line_crops=False, shapes=False, text_map=False, line_map=False, strokes=False,
                frame_lines=False, line_links=False, line_geom=False, line_words=False, run_read=False, word_match=False, word_decode=False, run_split=False, track_read=False, lattice_decode=False, lattice_match=False, lattice_track=False, track_decode=False) -> int:
    """The WANT_* bits of the want_* arguments of a detect call (line_crops: False, True (grey crops) or "glyphs" (grey and glyph crops))."""
    bits = [(nodes, WANT_NODES), (masks, WANT_MASKS), (shapes, WANT_SHAPES), (strokes, WANT_STROKES), (text_map, WANT_TEXT_MAP),
            (line_map, WANT_LINE_MAP), (frame_lines, WANT_FRAME_LINES), (line_links, WANT_LINE_LINKS), (line_geom, WANT_LINE_GEOM), (line_words, WANT_LINE_WORDS), (run_read, WANT_RUN_READ), (word_match, WANT_WORD_MATCH), (word_decode, WANT_WORD_DECODE), (run_split, WANT_RUN_SPLIT), (track_read, WANT_TRACK_READ), (lattice_decode, WANT_LATTICE_DECODE), (lattice_match, WANT_LATTICE_MATCH), (lattice_track, WANT_LATTICE_TRACK), (track_decode, WANT_TRACK_DECODE), (line_crops, WANT_LINE_CROPS), (line_crops == "glyphs", WANT_LINE_GLYPHS)]
    return sum(bit for want, bit in bits if want)


def frame_lines_from_pairs(feet: np.ndarray, frames_of_lines, pyr_of_lines, pairs: np.ndarray, num: int = 1, den: int = 2):
    """str_er_frame_lines_from_pairs (pure host): the frame lines of the lines with these feet (LINE_FOOT_DTYPE; box and pixels are
    read), frames and pyramid levels from the pairs with common pixels (LINE_PAIR_DTYPE; a, b, inter are read).  Returns copies
    (feet with frame_line set, pairs with dup set, frame lines FRAME_LINE_DTYPE, members int32)."""
    ft = np.array(feet, dtype=LINE_FOOT_DTYPE).reshape(-1)
    pr = np.array(pairs, dtype=LINE_PAIR_DTYPE).reshape(-1)
    fr = np.ascontiguousarray(frames_of_lines, dtype=np.uint32).reshape(-1)
    py = np.ascontiguousarray(pyr_of_lines, dtype=np.uint8).reshape(-1)
    n = len(ft)
    if len(fr) != n or len(py) != n:
        raise ValueError("frames_of_lines and pyr_of_lines need one entry per line")
    fl = np.zeros(max(1, n), FRAME_LINE_DTYPE)
    mem = np.zeros(max(1, n), np.int32)
    nfl = C.c_int32()
    rc = load_library().str_er_frame_lines_from_pairs(_np_ptr(ft) if n else None, _np_ptr(fr) if n else None, _np_ptr(py) if n else None, n,
                                                      _np_ptr(pr) if len(pr) else None, len(pr), int(num), int(den), _np_ptr(fl), len(fl),
                                                      C.byref(nfl), _np_ptr(mem))
    if rc != 0:
        raise StrErError(rc, "str_er_frame_lines_from_pairs")
    return ft, pr, fl[:nfl.value], mem[:n]


def ocr_char(label: int) -> str:
    """str_er_ocr_char (pure host): the character of a label of the OCR scorer, '?' outside 0 .. 64."""
    return chr(load_library().str_er_ocr_char(int(label)))


def words_from_runs(line_words: np.ndarray, runs: np.ndarray, num: int = 1, den: int = 3):
    """str_er_words_from_runs (pure host): the words of lines from their glyph runs: line_words (LINE_WORDS_DTYPE; first_run, n_runs and
    colmax are read) and runs (LINE_RUN_DTYPE; x0 .. pixels are read), the runs of the lines back to back.  A gap g between two runs
    breaks a word when g * den >= num * colmax.  Returns copies (line_words, runs, words) with first_word / n_words, word and the
    LINE_WORD_DTYPE records filled."""
    lw = np.array(line_words, dtype=LINE_WORDS_DTYPE).reshape(-1)
    rn = np.array(runs, dtype=LINE_RUN_DTYPE).reshape(-1)
    words = np.zeros(max(1, len(rn)), LINE_WORD_DTYPE)
    n = C.c_int32()
    rc = load_library().str_er_words_from_runs(_np_ptr(rn) if len(rn) else None, len(rn), _np_ptr(lw) if len(lw) else None, len(lw), int(num), int(den),
                                               _np_ptr(words), len(words), C.byref(n))
    if rc != 0:
        raise StrErError(rc, "str_er_words_from_runs")
    return lw, rn, words[:n.value].copy()


def hull_of_points(points) -> np.ndarray:
    """str_er_hull_of_points (pure host): the strictly convex hull of (n, 2) integer points, (m, 2) int32, clockwise on screen (x to
    the right, y down) from the vertex with the smallest (y, x)."""
    pts = np.ascontiguousarray(points, dtype=np.int32).reshape(-1, 2)
    out = np.zeros((max(1, len(pts)), 2), np.int32)
    n = C.c_int32()
    rc = load_library().str_er_hull_of_points(_np_ptr(pts) if len(pts) else None, len(pts), _np_ptr(out), len(out), C.byref(n))
    if rc != 0:
        raise StrErError(rc, "str_er_hull_of_points")
    return out[:n.value]


def quad_from_hull(hull) -> np.ndarray:
    """str_er_quad_from_hull (pure host): one LINE_GEOM_DTYPE record with hull_area2, edge, ex .. cmax, qx and qy of a hull of (n, 2)
    vertices in the order of hull_of_points (first = 0, count = n; the moments stay 0)."""
    pts = np.ascontiguousarray(hull, dtype=np.int32).reshape(-1, 2)
    g = np.zeros(1, LINE_GEOM_DTYPE)
    rc = load_library().str_er_quad_from_hull(_np_ptr(pts) if len(pts) else None, len(pts), _np_ptr(g))
    if rc != 0:
        raise StrErError(rc, "str_er_quad_from_hull")
    g["count"] = len(pts)
    return g[0]


def _track_args(costs, first_run, n_runs_of_word, track_first, track_count, members):
    cs = np.ascontiguousarray(costs, dtype=np.uint8).reshape(-1, 65)
    fr = np.ascontiguousarray(first_run, dtype=np.int32).reshape(-1)
    no = np.ascontiguousarray(n_runs_of_word, dtype=np.int32).reshape(-1)
    tf = np.ascontiguousarray(track_first, dtype=np.int32).reshape(-1)
    tc = np.ascontiguousarray(track_count, dtype=np.int32).reshape(-1)
    mem = np.ascontiguousarray(members, dtype=np.int32).reshape(-1)
    if len(fr) != len(no) or len(tf) != len(tc):
        raise ValueError("first_run and n_runs_of_word: one value per word each; track_first and track_count: one per track each")
    return cs, fr, no, tf, tc, mem


def match_tracks_host(costs: np.ndarray, first_run, n_runs_of_word, track_first, track_count, members, words, fold_case: bool = True, ins: int = 64,
                      dele: int = 64, band: int = 2):
    """str_er_match_tracks_host (pure host, one thread): ERFilter.match_tracks with the lexicon and the parameters as arguments."""
    cs, fr, no, tf, tc, mem = _track_args(costs, first_run, n_runs_of_word, track_first, track_count, members)
    words = list(words)
    raw, off = _lexicon_bytes(words)
    buf = np.frombuffer(raw, np.uint8) if raw else np.zeros(1, np.uint8)
    out = np.zeros(max(1, len(tf)), TRACK_MATCH_DTYPE)
    mc = np.zeros(max(1, len(mem)), np.int32)
    opt = lambda a: _np_ptr(a) if len(a) else None
    rc = load_library().str_er_match_tracks_host(opt(cs), len(cs), opt(fr), opt(no), len(fr), opt(tf), opt(tc), opt(mem), len(mem), len(tf), _np_ptr(buf),
                                                 _np_ptr(off), len(words), LEXICON_FOLD_CASE if fold_case else 0, int(ins), int(dele), int(band),
                                                 _np_ptr(out), _np_ptr(mc))
    if rc != 0:
        raise StrErError(rc, "str_er_match_tracks_host")
    return out[:len(tf)], mc[:len(mem)]


def word_links(feet, frames_of_lines, line_tracks, frame_wh, words, num: int = 1, den: int = 2):
    """str_er_word_links (pure host): the reading lines and the word links of the words (LINE_WORD_DTYPE; line and the box are read)
    of the lines with these feet (LINE_FOOT_DTYPE; pixels are read), frames and text tracks; frame_wh: (n frames, 2) level-0 sizes.
    Returns (reading uint8 per line, links WORD_LINK_DTYPE)."""
    ft = np.ascontiguousarray(feet, dtype=LINE_FOOT_DTYPE).reshape(-1)
    fr = np.ascontiguousarray(frames_of_lines, dtype=np.uint32).reshape(-1)
    lt = np.ascontiguousarray(line_tracks, dtype=np.int32).reshape(-1)
    wh = np.ascontiguousarray(frame_wh, dtype=np.int32).reshape(-1, 2)
    ws = np.ascontiguousarray(words, dtype=LINE_WORD_DTYPE).reshape(-1)
    n = len(ft)
    if len(fr) != n or len(lt) != n:
        raise ValueError("frames_of_lines and line_tracks need one entry per line")
    reading = np.zeros(max(1, n), np.uint8)
    opt = lambda a: _np_ptr(a) if len(a) else None
    L, nl = load_library(), C.c_int32()
    rc = L.str_er_word_links(opt(ft), opt(fr), opt(lt), n, opt(wh), len(wh), opt(ws), len(ws), int(num), int(den), _np_ptr(reading), None, 0, C.byref(nl))
    if rc != 0:
        raise StrErError(rc, "str_er_word_links")
    links = np.zeros(max(1, nl.value), WORD_LINK_DTYPE)
    rc = L.str_er_word_links(opt(ft), opt(fr), opt(lt), n, opt(wh), len(wh), opt(ws), len(ws), int(num), int(den), _np_ptr(reading), _np_ptr(links), len(links),
                             C.byref(nl))
    if rc != 0:
        raise StrErError(rc, "str_er_word_links")
    return reading[:n], links[:nl.value]


def word_tracks_from_links(frames_of_lines, line_tracks, reading, words, links):
    """str_er_word_tracks_from_links (pure host): the word tracks from the reading flags and the links of word_links.  Returns
    (track_of_words int32, tracks WORD_TRACK_DTYPE, members int32)."""
    fr = np.ascontiguousarray(frames_of_lines, dtype=np.uint32).reshape(-1)
    lt = np.ascontiguousarray(line_tracks, dtype=np.int32).reshape(-1)
    rd = np.ascontiguousarray(reading, dtype=np.uint8).reshape(-1)
    ws = np.ascontiguousarray(words, dtype=LINE_WORD_DTYPE).reshape(-1)
    lk = np.ascontiguousarray(links, dtype=WORD_LINK_DTYPE).reshape(-1)
    n, nw = len(fr), len(ws)
    if len(lt) != n or len(rd) != n:
        raise ValueError("line_tracks and reading need one entry per line")
    of = np.zeros(max(1, nw), np.int32)
    tr = np.zeros(max(1, nw), WORD_TRACK_DTYPE)
    mem = np.zeros(max(1, nw), np.int32)
    opt = lambda a: _np_ptr(a) if len(a) else None
    ntr = C.c_int32()
    rc = load_library().str_er_word_tracks_from_links(opt(fr), opt(lt), opt(rd), n, opt(ws), nw, opt(lk), len(lk), _np_ptr(of), _np_ptr(tr), len(tr), C.byref(ntr),
                                                      _np_ptr(mem))
    if rc != 0:
        raise StrErError(rc, "str_er_word_tracks_from_links")
    tr = tr[:ntr.value]
    return of[:nw], tr, mem[:int(tr["count"].sum()) if len(tr) else 0]


def text_tracks_from_links(feet: np.ndarray, frames_of_lines, pairs: np.ndarray, links: np.ndarray, num: int = 1, den: int = 2):
    """str_er_text_tracks_from_links (pure host): the text tracks of the lines with these feet (LINE_FOOT_DTYPE; pixels are read) and
    frames from the pairs within a frame (LINE_PAIR_DTYPE; a, b, inter, dup are read) and the overlaps across adjacent frames
    (LINE_LINK_DTYPE; a, b, inter are read).  Returns (links with link set, line_tracks int32, tracks TEXT_TRACK_DTYPE, members int32)."""
    ft = np.ascontiguousarray(feet, dtype=LINE_FOOT_DTYPE).reshape(-1)
    pr = np.ascontiguousarray(pairs, dtype=LINE_PAIR_DTYPE).reshape(-1)
    lk = np.array(links, dtype=LINE_LINK_DTYPE).reshape(-1)
    fr = np.ascontiguousarray(frames_of_lines, dtype=np.uint32).reshape(-1)
    n = len(ft)
    if len(fr) != n:
        raise ValueError("frames_of_lines needs one entry per line")
    lt = np.zeros(max(1, n), np.int32)
    tr = np.zeros(max(1, n), TEXT_TRACK_DTYPE)
    mem = np.zeros(max(1, n), np.int32)
    ntr = C.c_int32()
    rc = load_library().str_er_text_tracks_from_links(_np_ptr(ft) if n else None, _np_ptr(fr) if n else None, n, _np_ptr(pr) if len(pr) else None, len(pr),
                                                      _np_ptr(lk) if len(lk) else None, len(lk), int(num), int(den), _np_ptr(lt), _np_ptr(tr), len(tr),
                                                      C.byref(ntr), _np_ptr(mem))
    if rc != 0:
        raise StrErError(rc, "str_er_text_tracks_from_links")
    return lk, lt[:n], tr[:ntr.value], mem[:n]


@dataclass
class EdgeFeet:
    """The footprints of the lines of one frame of a result (Result.edge_feet): the frame's size, the lines' indices into texts,
    their feet (LINE_FOOT_DTYPE) and their rows of (w + 31) // 32 words over the foot boxes, back to back."""
    width: int
    height: int
    lines: np.ndarray
    feet: np.ndarray
    bits: np.ndarray


class TextTracker:
    """Persistent text track ids over successive results (host only).  Feed it the results of consecutive calls or stream
    submissions in time (ticket) order, each made with WANT_FRAME_LINES | WANT_LINE_LINKS: update() overlaps the last frame's
    footprints of the previous result with the first frame's of the new one (ERFilter.link_feet on `linker`, at its
    set_line_link threshold) and returns one id per line of the result.  A track that continues keeps its id; two tracks that a
    later result joins keep the smaller id: resolve() maps ids handed out earlier to their current ones."""

    def __init__(self, linker: "ERFilter"):
        self.linker = linker
        self._parent = []            # union-find over the ids handed out; the root is the smallest
        self._prev = None            # (EdgeFeet of the last frame, id of each of its lines)

    def _find(self, i: int) -> int:
        while self._parent[i] != i:
            self._parent[i] = self._parent[self._parent[i]]
            i = self._parent[i]
        return i

    def _join(self, i: int, j: int) -> None:
        i, j = self._find(i), self._find(j)
        if i != j:
            self._parent[max(i, j)] = min(i, j)

    def reset(self) -> None:
        """Forget the previous result (a cut the caller knows of); the ids handed out stay valid."""
        self._prev = None

    def resolve(self, ids) -> np.ndarray:
        return np.array([self._find(int(i)) for i in np.asarray(ids).reshape(-1)], np.int64)

    def update(self, res: "Result") -> np.ndarray:
        lt = res.line_tracks
        first, last = res.edge_feet(0), res.edge_feet(1)
        base = len(self._parent)
        self._parent.extend(range(base, base + len(res.text_tracks)))      # a new id per track of the result, joined with older ones below
        if self._prev is not None:
            pe, pid = self._prev
            if (pe.width, pe.height) == (first.width, first.height) and len(pe.lines) and len(first.lines):
                for k in self.linker.link_feet(first.width, first.height, pe.feet, pe.bits, first.feet, first.bits):
                    if k["link"]:
                        self._join(int(pid[k["a"]]), base + int(lt[first.lines[k["b"]]]))
        ids = self.resolve(base + lt.astype(np.int64)) if len(lt) else np.zeros(0, np.int64)
        self._prev = (last, ids[last.lines] if len(last.lines) else np.zeros(0, np.int64))
        return ids


class TrackPool:
    """str_er_track_pool_*: cap_tracks pooled word tracks on the device of the ERFilter f (str_er_pool_match): per slot the summed
    costs of everything added to it against every entry of f's lexicon, kept from call to call.  Bound to f's lexicon, set_word_match
    and (lattice=True) set_run_split as they are at creation: after one of those setters every call raises STR_ER_ESTATE until
    reset().  Close it before f."""

    def __init__(self, f: "ERFilter", cap_tracks: int, lattice: bool = False):
        self.f, self.L, self.lattice = f, f.L, bool(lattice)
        h = C.c_void_p()
        f._check(self.L.str_er_track_pool_create(f.h, int(cap_tracks), POOL_LATTICE if lattice else 0, C.byref(h)))
        self.h = h
        self.cap_tracks = int(cap_tracks)

    def close(self) -> None:
        if getattr(self, "h", None):
            if getattr(self.f, "h", None):          # (the context frees nothing of the pool: without it only the handle is dropped)
                self.L.str_er_track_pool_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> None:
        self.f._check(rc)

    @staticmethod
    def _slots(slots) -> np.ndarray:
        return np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)

    def add(self, costs, first_run, n_runs_of_word, track_first, track_count, members, slots) -> None:
        """str_er_track_pool_add: the tracks, given as for ERFilter.match_tracks, are added to the slots slots[g] (distinct)."""
        cs, fr, no, tf, tc, mem = _track_args(costs, first_run, n_runs_of_word, track_first, track_count, members)
        sl = self._slots(slots)
        if len(sl) != len(tf):
            raise ValueError("slots: one per track")
        opt = lambda a: _np_ptr(a) if len(a) else None
        self._check(self.L.str_er_track_pool_add(self.h, opt(cs), len(cs), opt(fr), opt(no), len(fr), opt(tf), opt(tc), opt(mem), len(mem), len(tf), opt(sl)))

    def add_lattice(self, splits, run_costs, piece_costs, first_run, n_runs_of_word, track_first, track_count, members, slots) -> None:
        """str_er_track_pool_add_lattice: the same for a lattice pool, the tracks given as for ERFilter.lattice_match_tracks."""
        a = _lattice_track_args(splits, run_costs, piece_costs, first_run, n_runs_of_word, track_first, track_count, members)
        sl = self._slots(slots)
        if len(sl) != a[0][-1]:
            raise ValueError("slots: one per track")
        self._check(self.L.str_er_track_pool_add_lattice(self.h, *a[0], _np_ptr(sl) if len(sl) else None))

    def join(self, dst: int, srcs) -> None:
        """str_er_track_pool_join: slot dst takes the members of the slots srcs, which become empty."""
        sl = self._slots(srcs)
        self._check(self.L.str_er_track_pool_join(self.h, int(dst), _np_ptr(sl) if len(sl) else None, len(sl)))

    def clear(self, slots) -> None:
        """str_er_track_pool_clear: those slots become empty."""
        sl = self._slots(slots)
        self._check(self.L.str_er_track_pool_clear(self.h, _np_ptr(sl) if len(sl) else None, len(sl)))

    def read(self, slots) -> np.ndarray:
        """str_er_track_pool_read: POOL_MATCH_DTYPE per slot named (a slot may be named more than once)."""
        sl = self._slots(slots)
        out = np.zeros(max(1, len(sl)), POOL_MATCH_DTYPE)
        self._check(self.L.str_er_track_pool_read(self.h, _np_ptr(sl) if len(sl) else None, len(sl), _np_ptr(out)))
        return out[:len(sl)]

    def reset(self) -> None:
        """str_er_track_pool_reset: every slot empty, the pool bound to f's lexicon and parameters as they are now."""
        self._check(self.L.str_er_track_pool_reset(self.h))

    def info(self) -> dict:
        """str_er_track_pool_info: the slots, the mode, the entries of the lexicon it is bound to, its bytes on the device, the
        slots in use and whether it is stale."""
        cap, fl, n, by, use, st = C.c_int32(), C.c_uint32(), C.c_int32(), C.c_uint64(), C.c_int32(), C.c_int32()
        self._check(self.L.str_er_track_pool_info(self.h, C.byref(cap), C.byref(fl), C.byref(n), C.byref(by), C.byref(use), C.byref(st)))
        return {"cap_tracks": int(cap.value), "lattice": bool(fl.value & POOL_LATTICE), "decode": bool(fl.value & POOL_DECODE), "n_entries": int(n.value), "device_bytes": int(by.value),
                "in_use": int(use.value), "stale": bool(st.value)}


class DecodePool(TrackPool):
    """str_er_track_pool_create_decode: cap_tracks pooled word tracks on the device of the ERFilter f without a lexicon
    (str_er_pool_decode): per slot the newest `keep` usable members added to it, their cost rows and decoder strings, kept from call
    to call; read() decodes a slot as ERFilter.decode_tracks decodes the track of its kept members in age order.  Bound to f's
    set_bigram, set_word_decode and set_track_decode as they are at creation: after one of those setters every call raises
    STR_ER_ESTATE until reset().  add, join, clear, reset and close are TrackPool's.  Close it before f."""

    def __init__(self, f: "ERFilter", cap_tracks: int, keep: int = 32):
        self.f, self.L, self.lattice = f, f.L, False
        h = C.c_void_p()
        f._check(self.L.str_er_track_pool_create_decode(f.h, int(cap_tracks), int(keep), C.byref(h)))
        self.h = h
        self.cap_tracks, self.keep = int(cap_tracks), int(keep)

    def add_lattice(self, *args, **kw) -> None:
        raise StrErError(-3, "a decode pool has no lattice mode")

    def read(self, slots):
        """str_er_track_pool_read_decode: (POOL_DECODE_DTYPE per slot named, (n, 32) uint8 labels, (n, keep) int32 member costs in
        age order, -1 past n_kept); a slot may be named more than once."""
        sl = self._slots(slots)
        n = len(sl)
        out = np.zeros(max(1, n), POOL_DECODE_DTYPE)
        ch = np.full((max(1, n), 32), 0xFF, np.uint8)
        mc = np.full((max(1, n), self.keep), -1, np.int32)
        self._check(self.L.str_er_track_pool_read_decode(self.h, _np_ptr(sl) if n else None, n, _np_ptr(out), _np_ptr(ch), _np_ptr(mc)))
        return out[:n], ch[:n], mc[:n]

    def members(self, slot: int):
        """str_er_track_pool_members: the kept list of a slot in age order: (uint64 keys, int32 run counts, (n_kept, 32, 65) uint8
        rows, of which the first n_runs of a member are its own)."""
        keys, nr, rows, n = np.zeros(self.keep, np.uint64), np.zeros(self.keep, np.int32), np.zeros((self.keep, 32, 65), np.uint8), C.c_int32()
        self._check(self.L.str_er_track_pool_members(self.h, int(slot), _np_ptr(keys), _np_ptr(nr), _np_ptr(rows), C.byref(n)))
        return keys[:n.value], nr[:n.value], rows[:n.value]

    def text(self, slot: int):
        """The string of the slot's pooled decode, None where nothing was decoded."""
        rec, ch, _ = self.read([slot])
        return _decode_text(rec[0], ch[0])

    def info(self) -> dict:
        """str_er_track_pool_info and _keep: the slots, keep, its bytes on the device, the slots in use and whether it is stale."""
        d = TrackPool.info(self)
        k = C.c_int32()
        self._check(self.L.str_er_track_pool_keep(self.h, C.byref(k)))
        d.update(decode=True, keep=int(k.value))
        return d


class LatticeDecodePool(DecodePool):
    """str_er_track_pool_create_lattice_decode: a DecodePool over the members' piece lattices (the lattice decode pool of str_er.h):
    per slot the newest `keep` usable members (N <= 32 nodes) added to it -- their split records, run rows, piece rows and lattice
    decoder strings -- kept from call to call; a read decodes a slot as ERFilter.lattice_decode_tracks decodes the track of its kept
    members in age order, every member's segmentation free.  Bound to what a DecodePool is bound to and to the SPLIT of
    set_run_split: after set_bigram, set_word_decode, set_track_decode or a set_run_split with another split_cost every call raises
    STR_ER_ESTATE until reset().  add_lattice feeds it and add raises; join, clear, reset, text and close are DecodePool's."""

    def __init__(self, f: "ERFilter", cap_tracks: int, keep: int = 32):
        self.f, self.L, self.lattice = f, f.L, True
        h = C.c_void_p()
        f._check(self.L.str_er_track_pool_create_lattice_decode(f.h, int(cap_tracks), int(keep), C.byref(h)))
        self.h = h
        self.cap_tracks, self.keep = int(cap_tracks), int(keep)

    def add(self, *args, **kw) -> None:
        raise StrErError(-6, "a lattice decode pool takes add_lattice")

    def add_lattice(self, splits, run_costs, piece_costs, first_run, n_runs_of_word, track_first, track_count, members, slots) -> None:
        """str_er_track_pool_add_lattice: the tracks, given as for ERFilter.lattice_decode_tracks, are added to the slots slots[g]
        (distinct)."""
        TrackPool.add_lattice(self, splits, run_costs, piece_costs, first_run, n_runs_of_word, track_first, track_count, members, slots)

    def read_lattice(self, slots):
        """str_er_track_pool_read_lattice_decode: read()'s triple, then (n, keep) LATTICE_TRACK_MEMBER_DTYPE (the kept members in age
        order, word = the age rank; cost = word = -1 past n_kept), (n, keep, 32) uint8 sources and the SPLIT_PART_DTYPE parts of all
        slots back to back (run 32 * rank + the member's run, piece 80 * rank + the member's piece row)."""
        sl = self._slots(slots)
        n = len(sl)
        out = np.zeros(max(1, n), POOL_DECODE_DTYPE)
        ch = np.full((max(1, n), 32), 0xFF, np.uint8)
        mc = np.full((max(1, n), self.keep), -1, np.int32)
        mrec = np.zeros((max(1, n), self.keep), LATTICE_TRACK_MEMBER_DTYPE)
        sr = np.full((max(1, n), self.keep, 32), 0xFF, np.uint8)
        cap = int(min(32 * max(1, n) * self.keep, 2 ** 31 - 1))
        parts = np.zeros(cap, SPLIT_PART_DTYPE)
        k = C.c_int32()
        self._check(self.L.str_er_track_pool_read_lattice_decode(self.h, _np_ptr(sl) if n else None, n, _np_ptr(out), _np_ptr(ch), _np_ptr(mc), _np_ptr(mrec), _np_ptr(sr),
                                                                 _np_ptr(parts), cap, C.byref(k)))
        return out[:n], ch[:n], mc[:n], mrec[:n], sr[:n], parts[:k.value].copy()

    def members(self, slot: int):
        """str_er_track_pool_lattice_members: the kept list of a slot in age order: (uint64 keys, int32 run counts, (n_kept, 32)
        RUN_SPLIT_DTYPE whose first_piece indexes the member's own piece rows, (n_kept, 32, 65) uint8 run rows, (n_kept, 80, 65) uint8
        piece rows); what lies behind a member's own records and rows is zero."""
        kp = self.keep
        keys, nr, sp = np.zeros(kp, np.uint64), np.zeros(kp, np.int32), np.zeros((kp, 32), RUN_SPLIT_DTYPE)
        rr, pr, n = np.zeros((kp, 32, 65), np.uint8), np.zeros((kp, 80, 65), np.uint8), C.c_int32()
        self._check(self.L.str_er_track_pool_lattice_members(self.h, int(slot), _np_ptr(keys), _np_ptr(nr), _np_ptr(sp), _np_ptr(rr), _np_ptr(pr), C.byref(n)))
        return keys[:n.value], nr[:n.value], sp[:n.value], rr[:n.value], pr[:n.value]


def _decode_text(rec, chars):
    return "".join(_OCR_ALPHABET[int(a)] for a in chars[:int(rec["n_chars"])]) if int(rec["cost"]) >= 0 else None


class WordTracker:
    """Persistent word track ids and pooled readings over successive results: the word-level sibling of TextTracker, which it holds.
    Feed update() the results of consecutive calls or stream submissions in time order, each made with want_frame_lines,
    want_line_links, want_line_words, want_run_read, want_word_match and want_track_read (and want_run_split for a lattice pool).
    Every word track of a result gets a fresh id and a fresh slot of `pool` (a TrackPool on `linker`, whose lexicon and parameters
    are those of the calls), to which its members are added with the rows the call's own track match read: run_costs, the rows of
    split_parts where the result has them, or for a lattice pool run_splits / run_costs / piece_costs.  Where the previous result's
    last frame and this result's first frame have equal sizes, a word u of the one and a word v of the other, both eligible in their
    own call and on lines whose persistent text ids are the same after TextTracker.update, are linked iff their boxes share pixels and
    inter * den >= num * (area(u) + area(v) - inter), the rule of str_er_word_link at linker's set_word_link threshold.  Linked ids
    are joined, the smaller id stays, and their slots are joined.  A pooled track without a member in the result's last frame cannot
    be extended: its final record goes to `closed` as (id, record) and its slot is freed.
      Without a lexicon: decode_pool, a DecodePool on `linker`, takes the place of `pool` or stands beside it (at least one of the two;
    both get the same slot numbers, joins and clears, and the smaller capacity counts).  The results then need want_track_decode
    (with want_word_decode) instead of, or beside, want_word_match and want_track_read; the decode pool is fed the unfolded rows of
    the words, so a result whose run_costs a folding lexicon folded is refused with ValueError before either pool is touched.
    read_decode / decode_text give the pooled decode of an id, and a closed track's final one goes to `closed_decodes` as
    (id, record, chars).
      A LatticeDecodePool as decode_pool pools the joint decode over the members' piece lattices instead: it is fed run_splits,
    run_costs and piece_costs of the result, which then needs want_run_split and want_lattice_decode beside want_track_decode.  The
    refusal of folded rows applies unchanged, the pieces' rows being folded where the runs' are; read_decode, decode_text and
    closed_decodes work as with a DecodePool."""

    def __init__(self, linker: "ERFilter", pool: Optional[TrackPool] = None, decode_pool: Optional["DecodePool"] = None):
        if pool is None and decode_pool is None:
            raise ValueError("WordTracker: a TrackPool, a DecodePool or both")
        if isinstance(pool, DecodePool) or (decode_pool is not None and not isinstance(decode_pool, DecodePool)):
            raise ValueError("WordTracker: pool is a TrackPool and decode_pool a DecodePool")
        self.linker, self.pool, self.decode_pool = linker, pool, decode_pool
        self.lines = TextTracker(linker)
        self.closed = []
        self.closed_decodes = []
        self._parent = []            # union-find over the ids handed out; the root is the smallest
        self._slot = {}              # root id of a live track -> its slot
        cap = min(p.cap_tracks for p in (pool, decode_pool) if p is not None)
        self._free = list(range(cap - 1, -1, -1))      # (pop() hands out the smallest)
        self._final = {}             # id of a closed track -> its record
        self._final_decode = {}      # id of a closed track -> (its decode record, its labels)
        self._prev = None            # (w, h, boxes (n, 4) int64, text ids, word track ids) of the eligible words of the last frame

    def _find(self, i: int) -> int:
        while self._parent[i] != i:
            self._parent[i] = self._parent[self._parent[i]]
            i = self._parent[i]
        return i

    def reset(self) -> None:
        """Forget the previous frame (a cut the caller knows of): the live tracks are closed, the ids handed out stay valid."""
        self._close(list(self._slot))
        self._prev = None
        self.lines.reset()

    def resolve(self, ids) -> np.ndarray:
        return np.array([self._find(int(i)) if int(i) >= 0 else -1 for i in np.asarray(ids).reshape(-1)], np.int64)

    def read(self, ids) -> np.ndarray:
        """POOL_MATCH_DTYPE per id: the pooled record of a live track, the final record of a closed one."""
        if self.pool is None:
            raise ValueError("WordTracker.read: no lexicon pool (read_decode gives the pooled decode)")
        roots = self.resolve(ids)
        out = np.zeros(len(roots), POOL_MATCH_DTYPE)
        live = [k for k, r in enumerate(roots) if int(r) in self._slot]
        if live:
            out[live] = self.pool.read([self._slot[int(roots[k])] for k in live])
        for k, r in enumerate(roots):
            if int(r) not in self._slot:
                out[k] = self._final[int(r)]
        return out

    def text(self, i: int):
        """The lexicon entry of the track's pooled match, None where it has none."""
        e = int(self.read([i])[0]["entry"])
        return self.linker._lexicon[e] if e >= 0 else None

    def read_decode(self, ids):
        """(POOL_DECODE_DTYPE per id, (n, 32) uint8 labels): the pooled decode of a live track, the final one of a closed track."""
        if self.decode_pool is None:
            raise ValueError("WordTracker.read_decode: no decode pool")
        roots = self.resolve(ids)
        out, ch = np.zeros(len(roots), POOL_DECODE_DTYPE), np.full((len(roots), 32), 0xFF, np.uint8)
        live = [k for k, r in enumerate(roots) if int(r) in self._slot]
        if live:
            out[live], ch[live], _ = self.decode_pool.read([self._slot[int(roots[k])] for k in live])
        for k, r in enumerate(roots):
            if int(r) not in self._slot:
                out[k], ch[k] = self._final_decode[int(r)]
        return out, ch

    def decode_text(self, i: int):
        """The string of the track's pooled decode, None where nothing was decoded."""
        rec, ch = self.read_decode([i])
        return _decode_text(rec[0], ch[0])

    def _close(self, roots) -> None:
        roots = sorted(int(r) for r in roots)
        if not roots:
            return
        slots = [self._slot[r] for r in roots]
        if self.pool is not None:
            recs = self.pool.read(slots)
            self.pool.clear(slots)
            for r, rec in zip(roots, recs):
                self.closed.append((r, rec.copy()))
                self._final[r] = rec.copy()
        if self.decode_pool is not None:
            recs, chars, _ = self.decode_pool.read(slots)
            self.decode_pool.clear(slots)
            for r, rec, ch in zip(roots, recs, chars):
                self.closed_decodes.append((r, rec.copy(), ch.copy()))
                self._final_decode[r] = (rec.copy(), ch.copy())
        for r, s in zip(roots, slots):
            del self._slot[r]
            self._free.append(s)
        self._free.sort(reverse=True)

    def _rows(self, res: "Result"):
        try:
            parts = res.split_parts
        except ValueError:
            return res.run_costs, res.words["first_run"], res.words["n_runs"]
        rows = np.zeros((len(parts), 65), np.uint8)
        whole = parts["piece"] < 0
        rows[whole] = res.run_costs[parts["run"][whole]]
        rows[~whole] = res.piece_costs[parts["piece"][~whole]]
        return rows, res.word_splits["first_part"], res.word_splits["n_parts"]

    def update(self, res: "Result") -> np.ndarray:
        tow, tracks, members, words = res.word_track_of_words, res.word_tracks, res.word_track_members, res.words
        nt = len(tracks)
        if nt > len(self._free):
            raise StrErError(-7, "WordTracker: the pool has %d free slots, the result %d word tracks" % (len(self._free), nt))
        if self.decode_pool is not None and res._word_matches is not None and self.linker.lexicon_info()["flags"] & LEXICON_FOLD_CASE:
            raise ValueError("WordTracker: the result's run_costs are folded by the lexicon (want_word_match under fold_case); a decode pool "
                             "takes the unfolded rows of the word decoder: set the lexicon with fold_case=False, or keep the two pools on separate calls")
        first, last = res.edge_feet(0), res.edge_feet(1)
        slots = self._free[::-1][:nt]          # (the smallest free slots; an addition that is refused leaves the tracker as it was)
        if nt:
            if self.pool is not None:
                if self.pool.lattice:
                    self.pool.add_lattice(res.run_splits, res.run_costs, res.piece_costs, words["first_run"], words["n_runs"], tracks["first"], tracks["count"], members, slots)
                else:
                    self.pool.add(*self._rows(res), tracks["first"], tracks["count"], members, slots)
            if self.decode_pool is not None:
                try:
                    if isinstance(self.decode_pool, LatticeDecodePool):
                        self.decode_pool.add_lattice(res.run_splits, res.run_costs, res.piece_costs, words["first_run"], words["n_runs"], tracks["first"], tracks["count"],
                                                     members, slots)
                    else:
                        self.decode_pool.add(*self._rows(res), tracks["first"], tracks["count"], members, slots)
                except Exception:
                    if self.pool is not None:          # (the lexicon pool took the tracks already: it gives them back)
                        self.pool.clear(slots)
                    raise
            del self._free[-nt:]
        tids = self.lines.update(res)
        base = len(self._parent)
        self._parent.extend(range(base, base + nt))
        for g, s in enumerate(slots):
            self._slot[base + g] = s
        box = lambda ws: np.stack([words[k][ws].astype(np.int64) for k in ("x", "y", "w", "h")], 1) if len(ws) else np.zeros((0, 4), np.int64)
        eligible = lambda lines: np.flatnonzero((tow >= 0) & np.isin(words["line"], lines)).astype(np.int64) if len(words) else np.zeros(0, np.int64)
        # the boundary: the eligible words of the previous last frame against those of this first frame
        if self._prev is not None and (self._prev[0], self._prev[1]) == (first.width, first.height):
            num, den = getattr(self.linker, "_word_link", (1, 2))
            _, _, pbox, ptid, pwid = self._prev
            vs = eligible(first.lines)
            vbox = box(vs)
            for u in range(len(pbox)):
                tu = int(self.lines.resolve([ptid[u]])[0])
                for k, v in enumerate(vs):
                    if int(tids[int(words["line"][v])]) != tu:
                        continue
                    (ux, uy, uw, uh), (vx, vy, vw, vh) = (int(a) for a in pbox[u]), (int(a) for a in vbox[k])
                    iw, ih = min(ux + uw, vx + vw) - max(ux, vx), min(uy + uh, vy + vh) - max(uy, vy)
                    inter = iw * ih if iw > 0 and ih > 0 else 0
                    if inter > 0 and inter * den >= num * (uw * uh + vw * vh - inter):
                        i, j = self._find(int(pwid[u])), self._find(base + int(tow[v]))
                        if i != j:
                            self._parent[max(i, j)] = min(i, j)
        # one join per component of live tracks: the smallest id keeps its slot
        comp = {}
        for r in list(self._slot):
            comp.setdefault(self._find(r), []).append(r)
        for root, rs in comp.items():
            if len(rs) > 1:
                srcs = [self._slot[r] for r in sorted(rs) if r != root]
                for p in (self.pool, self.decode_pool):
                    if p is not None:
                        p.join(self._slot[root], srcs)
                for r in rs:
                    if r != root:
                        del self._slot[r]
                self._free.extend(srcs)
        self._free.sort(reverse=True)
        ids = np.array([self._find(base + int(t)) if t >= 0 else -1 for t in tow], np.int64)
        # what has no member in the last frame cannot be extended
        ends = eligible(last.lines)
        open_roots = set(int(ids[w]) for w in ends)
        self._close([r for r in self._slot if r not in open_roots])
        self._prev = (last.width, last.height, box(ends), np.array([tids[int(words["line"][w])] for w in ends], np.int64), ids[ends] if len(ends) else np.zeros(0, np.int64))
        return ids


def line_crop_geometry(boxes_xywh: np.ndarray, slope: float, height: int = 32, max_width: int = 1024, pad: float = 0.125) -> np.ndarray:
    """str_er_line_crop_geometry: the crop record (LINE_CROP_DTYPE, pix_off 0) of one line with these boxes and slope."""
    bx = np.ascontiguousarray(boxes_xywh, dtype=np.int32).reshape(-1, 4)
    out = np.zeros(1, LINE_CROP_DTYPE)
    rc = load_library().str_er_line_crop_geometry(_np_ptr(bx) if len(bx) else None, len(bx), float(slope), int(height), int(max_width),
                                                  float(pad), _np_ptr(out))
    if rc != 0:
        raise StrErError(rc, "str_er_line_crop_geometry")
    return out[0]


def flood_order(plane: np.ndarray, thresh_step: int = 8) -> np.ndarray:
    """str_er_flood_order: (h, w) uint32, 1-based order in which the reference's flood first reaches each pixel (0: never)."""
    a = np.ascontiguousarray(plane, dtype=np.uint8)
    h, w = a.shape
    out = np.zeros((h, w), np.uint32)
    rc = load_library().str_er_flood_order(_np_ptr(a), w, h, w, thresh_step, _np_ptr(out))
    if rc != 0:
        raise StrErError(rc, "str_er_flood_order")
    return out


class Comm:
    """One rank of the candidate gather (include/str_er.h, str_er_comm_* / str_er_gather_*): an RCCL communicator
    (`Comm.rccl`) or a member of an in-process group that exchanges through host memory (`Comm.local_group`)."""

    def __init__(self, handle, world: int, rank: int, group=None):
        self.L, self.h, self.world, self.rank, self._group = load_library(), handle, world, rank, group

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        rc = load_library().str_er_comm_unique_id(buf)
        if rc != 0:
            raise StrErError(rc, "str_er_comm_unique_id (is librccl.so there?)")
        return buf.raw

    @classmethod
    def rccl(cls, device: int, rank: int, world: int, uid: bytes) -> "Comm":
        h = C.c_void_p()
        L = load_library()
        rc = L.str_er_comm_create(device, rank, world, C.create_string_buffer(uid, 128), C.byref(h))
        if rc != 0:
            raise StrErError(rc, "str_er_comm_create: " + (L.str_er_comm_last_error(None) or b"").decode())
        return cls(h, world, rank)

    @classmethod
    def local_group(cls, world: int):
        """`world` communicators of one in-process group (use one per thread)."""
        L = load_library()
        g = C.c_void_p()
        rc = L.str_er_comm_local_group(world, C.byref(g))
        if rc != 0:
            raise StrErError(rc, "str_er_comm_local_group")
        out = []
        for r in range(world):
            h = C.c_void_p()
            rc = L.str_er_comm_create_local(g, r, C.byref(h))
            if rc != 0:
                raise StrErError(rc, "str_er_comm_create_local")
            out.append(cls(h, world, r, group=g))
        L.str_er_comm_local_group_free(g)        # the communicators keep the group alive
        return out

    def _take(self, rc, p, n, counts):
        if rc != 0:
            raise StrErError(rc, (self.L.str_er_comm_last_error(self.h) or b"").decode())
        try:
            out = (np.frombuffer((C.c_char * (48 * n.value)).from_address(p.value), dtype=CAND_DTYPE).copy()
                   if n.value else np.zeros(0, CAND_DTYPE))
        finally:
            self.L.str_er_gather_free(p)
        return out, np.array(counts[:], np.int32)

    def gather(self, cands: np.ndarray, frame_offset: int = 0, failed: bool = False):
        """Collective: (all ranks' records ordered by rank, per-rank counts); `frame_offset` is added to this rank's frames.
        failed=True: this rank has nothing valid to contribute -- it still takes part (a count of -1), and EVERY rank's call returns an
        error instead of one rank leaving the others waiting in the collective."""
        a = np.ascontiguousarray(cands, dtype=CAND_DTYPE)
        p, n = C.c_void_p(), C.c_int32()
        counts = (C.c_int32 * self.world)()
        rc = self.L.str_er_gather_cands(self.h, _np_ptr(a) if len(a) and not failed else None, -1 if failed else len(a), frame_offset,
                                        C.byref(p), C.byref(n), counts)
        return self._take(rc, p, n, counts)

    def gather_last(self, erf: "ERFilter", frame_offset: int = 0):
        """The same for the candidates of erf's last detect call, straight from the device array (RCCL only)."""
        p, n = C.c_void_p(), C.c_int32()
        counts = (C.c_int32 * self.world)()
        rc = self.L.str_er_gather_last(self.h, erf.h, frame_offset, C.byref(p), C.byref(n), counts)
        return self._take(rc, p, n, counts)

    def allgather_bytes(self, data, device_in: bool = False, device_out: bool = False):
        """Collective, variable length (str_er_comm_allgather_bytes).  data: bytes / uint8 array, or (device address, n) with
        device_in.  Host output: list of `world` bytes objects; device output: (base address, starts, sizes) -- the communicator's
        buffer, valid until its next collective."""
        if device_in:
            ptr, n = C.c_void_p(int(data[0])), int(data[1])
            keep = None
        else:
            keep = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8).reshape(-1)
            ptr, n = (_np_ptr(keep) if len(keep) else None), len(keep)
        out = C.c_void_p()
        starts, sizes = (C.c_int64 * self.world)(), (C.c_int64 * self.world)()
        rc = self.L.str_er_comm_allgather_bytes(self.h, ptr, n, MEM_DEVICE if device_in else MEM_HOST, MEM_DEVICE if device_out else MEM_HOST,
                                                C.byref(out), starts, sizes)
        if rc != 0:
            raise StrErError(rc, (self.L.str_er_comm_last_error(self.h) or b"").decode())
        if device_out:
            return int(out.value or 0), [int(v) for v in starts], [int(v) for v in sizes]
        try:
            return [C.string_at(out.value + starts[r], sizes[r]) if sizes[r] else b"" for r in range(self.world)]
        finally:
            self.L.str_er_comm_free(out)

    def close(self) -> None:
        if getattr(self, "h", None):
            self.L.str_er_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FrameStream:
    """Frame ingest (include/str_er.h, str_er_stream_*): `depth` batches of host frames in flight, uploads overlapping
    compute.  acquire() hands out a page-locked numpy buffer to decode into; results come back in submission order."""

    def __init__(self, params: Params, depth: int = 3):
        self.L = load_library()
        p = params
        cp = _Params(p.thresh_step, p.min_area, p.max_area, p.stability_t, p.overlap_coef, p.n_pyr_levels,
                     p.channel_mask, p.device, p.max_width, p.max_height, p.max_frames, p.kept_cap, p.pool_cap,
                     p.sibling_order, p.stream)
        h = C.c_void_p()
        rc = self.L.str_er_stream_create(C.byref(cp), depth, C.byref(h))
        if rc != 0:
            raise StrErError(rc, (self.L.str_er_last_error(None) or b"").decode())
        self.h = h
        self.params = p
        self._base = {}                     # slot -> address of its staging buffer (acquire)

    def close(self) -> None:
        if getattr(self, "h", None):
            self.L.str_er_stream_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise StrErError(rc, (self.L.str_er_stream_last_error(self.h) or b"").decode())

    @property
    def depth(self) -> int:
        return int(self.L.str_er_stream_depth(self.h))

    def load_cascade(self, which: int, path: str) -> None:
        self._check(self.L.str_er_stream_load_cascade(self.h, which, path.encode()))

    def load_svm_model(self, path: str, dim: int = 1800) -> None:
        """str_er_load_svm_model on every context of the stream (str_er_stream_context): what WANT_RUN_READ submissions need."""
        for i in range(int(self.L.str_er_stream_depth(self.h))):
            ctx = self.L.str_er_stream_context(self.h, i)
            if self.L.str_er_load_svm_model(ctx, path.encode(), dim) != 0:
                raise StrErError(-6, (self.L.str_er_last_error(ctx) or b"").decode())

    def set_lexicon(self, words, fold_case: bool = True) -> None:
        """str_er_set_lexicon on every context of the stream (str_er_stream_context): what WANT_WORD_MATCH submissions need."""
        for i in range(int(self.L.str_er_stream_depth(self.h))):
            ctx = self.L.str_er_stream_context(self.h, i)
            rc = _set_lexicon(self.L, ctx, words, fold_case)
            if rc != 0:
                raise StrErError(rc, (self.L.str_er_last_error(ctx) or b"").decode())
        self._lexicon = _lexicon_strings(words)

    def set_word_match(self, ins: int = 64, dele: int = 64, band: int = 2) -> None:
        """str_er_set_word_match on every context of the stream."""
        for i in range(int(self.L.str_er_stream_depth(self.h))):
            ctx = self.L.str_er_stream_context(self.h, i)
            rc = self.L.str_er_set_word_match(ctx, int(ins), int(dele), int(band))
            if rc != 0:
                raise StrErError(rc, (self.L.str_er_last_error(ctx) or b"").decode())

    def set_word_link(self, num: int = 1, den: int = 2) -> None:
        """str_er_set_word_link on every context of the stream."""
        for i in range(int(self.L.str_er_stream_depth(self.h))):
            ctx = self.L.str_er_stream_context(self.h, i)
            rc = self.L.str_er_set_word_link(ctx, int(num), int(den))
            if rc != 0:
                raise StrErError(rc, (self.L.str_er_last_error(ctx) or b"").decode())

    def set_bigram(self, table) -> None:
        """str_er_set_bigram on every context of the stream: what WANT_WORD_DECODE submissions need."""
        t = None if table is None else _bigram_table(table)
        for i in range(int(self.L.str_er_stream_depth(self.h))):
            ctx = self.L.str_er_stream_context(self.h, i)
            rc = self.L.str_er_set_bigram(ctx, None if t is None else _np_ptr(t))
            if rc != 0:
                raise StrErError(rc, (self.L.str_er_last_error(ctx) or b"").decode())

    def set_word_margin(self, on: bool = True) -> None:
        """str_er_set_word_margin on every context of the stream."""
        for i in range(int(self.L.str_er_stream_depth(self.h))):
            ctx = self.L.str_er_stream_context(self.h, i)
            rc = self.L.str_er_set_word_margin(ctx, 1 if on else 0)
            if rc != 0:
                raise StrErError(rc, (self.L.str_er_last_error(ctx) or b"").decode())

    def set_line_decode(self, on: bool = True, weight: int = 16) -> None:
        """str_er_set_line_decode on every context of the stream."""
        for i in range(int(self.L.str_er_stream_depth(self.h))):
            ctx = self.L.str_er_stream_context(self.h, i)
            rc = self.L.str_er_set_line_decode(ctx, 1 if on else 0, int(weight))
            if rc != 0:
                raise StrErError(rc, (self.L.str_er_last_error(ctx) or b"").decode())

    def set_line_lattice_decode(self, on: bool = True, weight: int = 16) -> None:
        """str_er_set_line_lattice_decode on every context of the stream."""
        for i in range(int(self.L.str_er_stream_depth(self.h))):
            ctx = self.L.str_er_stream_context(self.h, i)
            rc = self.L.str_er_set_line_lattice_decode(ctx, 1 if on else 0, int(weight))
            if rc != 0:
                raise StrErError(rc, (self.L.str_er_last_error(ctx) or b"").decode())

    def set_line_margin(self, on: bool = True) -> None:
        """str_er_set_line_margin on every context of the stream."""
        for i in range(int(self.L.str_er_stream_depth(self.h))):
            ctx = self.L.str_er_stream_context(self.h, i)
            rc = self.L.str_er_set_line_margin(ctx, 1 if on else 0)
            if rc != 0:
                raise StrErError(rc, (self.L.str_er_last_error(ctx) or b"").decode())

    def set_lattice_margin(self, on: bool = True) -> None:
        """str_er_set_lattice_margin on every context of the stream."""
        for i in range(int(self.L.str_er_stream_depth(self.h))):
            ctx = self.L.str_er_stream_context(self.h, i)
            rc = self.L.str_er_set_lattice_margin(ctx, 1 if on else 0)
            if rc != 0:
                raise StrErError(rc, (self.L.str_er_last_error(ctx) or b"").decode())

    def set_lattice_track_decode(self, on: bool = True) -> None:
        """str_er_set_lattice_track_decode on every context of the stream."""
        for i in range(int(self.L.str_er_stream_depth(self.h))):
            ctx = self.L.str_er_stream_context(self.h, i)
            rc = self.L.str_er_set_lattice_track_decode(ctx, 1 if on else 0)
            if rc != 0:
                raise StrErError(rc, (self.L.str_er_last_error(ctx) or b"").decode())

    def set_track_decode(self, ins: int = 64, dele: int = 64, rounds: int = 8) -> None:
        """str_er_set_track_decode on every context of the stream."""
        for i in range(int(self.L.str_er_stream_depth(self.h))):
            ctx = self.L.str_er_stream_context(self.h, i)
            rc = self.L.str_er_set_track_decode(ctx, int(ins), int(dele), int(rounds))
            if rc != 0:
                raise StrErError(rc, (self.L.str_er_last_error(ctx) or b"").decode())

    def set_word_decode(self, ins: int = 0, dele: int = 0) -> None:
        """str_er_set_word_decode on every context of the stream."""
        for i in range(int(self.L.str_er_stream_depth(self.h))):
            ctx = self.L.str_er_stream_context(self.h, i)
            rc = self.L.str_er_set_word_decode(ctx, int(ins), int(dele))
            if rc != 0:
                raise StrErError(rc, (self.L.str_er_last_error(ctx) or b"").decode())

    def set_run_split(self, num: int = 1, den: int = 4, split_cost: int = 8) -> None:
        """str_er_set_run_split on every context of the stream."""
        for i in range(int(self.L.str_er_stream_depth(self.h))):
            ctx = self.L.str_er_stream_context(self.h, i)
            rc = self.L.str_er_set_run_split(ctx, int(num), int(den), int(split_cost))
            if rc != 0:
                raise StrErError(rc, (self.L.str_er_last_error(ctx) or b"").decode())

    def acquire(self):
        """(slot, uint8 view of the pinned staging buffer)."""
        slot, buf, cap = C.c_int32(), C.c_void_p(), C.c_int64()
        self._check(self.L.str_er_stream_acquire(self.h, C.byref(slot), C.byref(buf), C.byref(cap)))
        self._base[slot.value] = buf.value
        arr = np.frombuffer((C.c_uint8 * cap.value).from_address(buf.value), dtype=np.uint8)
        return slot.value, arr

    def submit(self, slot: int, w: int, h: int, n_frames: int, stages: int = STAGE_ALL, want_line_words: bool = False, want_run_read: bool = False,
               want_word_match: bool = False, want_word_decode: bool = False, want_run_split: bool = False, want_track_read: bool = False, want_lattice_decode: bool = False, want_lattice_match: bool = False, want_lattice_track: bool = False, want_track_decode: bool = False) -> int:
        stages |= (WANT_LINE_WORDS if want_line_words else 0) | (WANT_RUN_READ if want_run_read else 0) | (WANT_WORD_MATCH if want_word_match else 0) | (WANT_WORD_DECODE if want_word_decode else 0) | (WANT_RUN_SPLIT if want_run_split else 0) | (WANT_TRACK_READ if want_track_read else 0) | (WANT_LATTICE_DECODE if want_lattice_decode else 0) | (WANT_LATTICE_MATCH if want_lattice_match else 0) | (WANT_LATTICE_TRACK if want_lattice_track else 0) | (WANT_TRACK_DECODE if want_track_decode else 0)
        t = C.c_uint64()
        self._check(self.L.str_er_stream_submit(self.h, slot, w, h, 3 * w, 3 * w * h, n_frames, stages, C.byref(t)))
        return int(t.value)

    def submit_nv12(self, slot: int, w: int, h: int, n_frames: int, stages: int = STAGE_ALL, want_line_words: bool = False, want_run_read: bool = False,
               want_word_match: bool = False, want_word_decode: bool = False, want_run_split: bool = False, want_track_read: bool = False, want_lattice_decode: bool = False, want_lattice_match: bool = False, want_lattice_track: bool = False, want_track_decode: bool = False) -> int:
        """The staging buffer holds n_frames tightly packed NV12 frames (w * h * 3 / 2 bytes each)."""
        stages |= (WANT_LINE_WORDS if want_line_words else 0) | (WANT_RUN_READ if want_run_read else 0) | (WANT_WORD_MATCH if want_word_match else 0) | (WANT_WORD_DECODE if want_word_decode else 0) | (WANT_RUN_SPLIT if want_run_split else 0) | (WANT_TRACK_READ if want_track_read else 0) | (WANT_LATTICE_DECODE if want_lattice_decode else 0) | (WANT_LATTICE_MATCH if want_lattice_match else 0) | (WANT_LATTICE_TRACK if want_lattice_track else 0) | (WANT_TRACK_DECODE if want_track_decode else 0)
        t = C.c_uint64()
        self._check(self.L.str_er_stream_submit_nv12(self.h, slot, w, h, w, w * (h + h // 2), n_frames, stages, C.byref(t)))
        return int(t.value)

    def submit_copy(self, frames: np.ndarray, stages: int = STAGE_ALL, want_line_words: bool = False, want_run_read: bool = False,
               want_word_match: bool = False, want_word_decode: bool = False, want_run_split: bool = False, want_track_read: bool = False, want_lattice_decode: bool = False, want_lattice_match: bool = False, want_lattice_track: bool = False, want_track_decode: bool = False) -> int:
        stages |= (WANT_LINE_WORDS if want_line_words else 0) | (WANT_RUN_READ if want_run_read else 0) | (WANT_WORD_MATCH if want_word_match else 0) | (WANT_WORD_DECODE if want_word_decode else 0) | (WANT_RUN_SPLIT if want_run_split else 0) | (WANT_TRACK_READ if want_track_read else 0) | (WANT_LATTICE_DECODE if want_lattice_decode else 0) | (WANT_LATTICE_MATCH if want_lattice_match else 0) | (WANT_LATTICE_TRACK if want_lattice_track else 0) | (WANT_TRACK_DECODE if want_track_decode else 0)
        a = np.ascontiguousarray(frames, dtype=np.uint8)
        if a.ndim == 3:
            a = a[None]
        n, h, w, _ = a.shape
        t = C.c_uint64()
        self._check(self.L.str_er_stream_submit_copy(self.h, _np_ptr(a), w, h, 3 * w, 3 * w * h, n, stages, C.byref(t)))
        return int(t.value)

    def _submit_list(self, fn, slot: int, layout, stages: int) -> int:
        base = self._base.get(slot, 0)
        refs = [ImageRef(base + int(o), int(w), int(h), int(st)) for o, w, h, st in layout]
        arr = (ImageRef * max(1, len(refs)))(*refs)
        t = C.c_uint64()
        self._check(fn(self.h, slot, arr, len(refs), stages, C.byref(t)))
        return int(t.value)

    def submit_list(self, slot: int, layout, stages: int = STAGE_ALL, want_line_words: bool = False, want_run_read: bool = False,
               want_word_match: bool = False, want_word_decode: bool = False, want_run_split: bool = False, want_track_read: bool = False, want_lattice_decode: bool = False, want_lattice_match: bool = False, want_lattice_track: bool = False, want_track_decode: bool = False) -> int:
        """BGR frames of assorted sizes in the acquired buffer: layout = [(byte offset, w, h, stride), ...] (str_er_stream_submit_list)."""
        stages |= (WANT_LINE_WORDS if want_line_words else 0) | (WANT_RUN_READ if want_run_read else 0) | (WANT_WORD_MATCH if want_word_match else 0) | (WANT_WORD_DECODE if want_word_decode else 0) | (WANT_RUN_SPLIT if want_run_split else 0) | (WANT_TRACK_READ if want_track_read else 0) | (WANT_LATTICE_DECODE if want_lattice_decode else 0) | (WANT_LATTICE_MATCH if want_lattice_match else 0) | (WANT_LATTICE_TRACK if want_lattice_track else 0) | (WANT_TRACK_DECODE if want_track_decode else 0)
        return self._submit_list(self.L.str_er_stream_submit_list, slot, layout, stages)

    def submit_nv12_list(self, slot: int, layout, stages: int = STAGE_ALL, want_line_words: bool = False, want_run_read: bool = False,
               want_word_match: bool = False, want_word_decode: bool = False, want_run_split: bool = False, want_track_read: bool = False, want_lattice_decode: bool = False, want_lattice_match: bool = False, want_lattice_track: bool = False, want_track_decode: bool = False) -> int:
        """The same for NV12 frames: at every offset h + h/2 rows of `stride` bytes (str_er_stream_submit_nv12_list)."""
        stages |= (WANT_LINE_WORDS if want_line_words else 0) | (WANT_RUN_READ if want_run_read else 0) | (WANT_WORD_MATCH if want_word_match else 0) | (WANT_WORD_DECODE if want_word_decode else 0) | (WANT_RUN_SPLIT if want_run_split else 0) | (WANT_TRACK_READ if want_track_read else 0) | (WANT_LATTICE_DECODE if want_lattice_decode else 0) | (WANT_LATTICE_MATCH if want_lattice_match else 0) | (WANT_LATTICE_TRACK if want_lattice_track else 0) | (WANT_TRACK_DECODE if want_track_decode else 0)
        return self._submit_list(self.L.str_er_stream_submit_nv12_list, slot, layout, stages)

    def submit_copy_list(self, frames, stages: int = STAGE_ALL, want_line_words: bool = False, want_run_read: bool = False,
               want_word_match: bool = False, want_word_decode: bool = False, want_run_split: bool = False, want_track_read: bool = False, want_lattice_decode: bool = False, want_lattice_match: bool = False, want_lattice_track: bool = False, want_track_decode: bool = False) -> int:
        """(H,W,3) uint8 BGR frames of any sizes, copied into a buffer and submitted as one list (str_er_stream_submit_copy_list)."""
        stages |= (WANT_LINE_WORDS if want_line_words else 0) | (WANT_RUN_READ if want_run_read else 0) | (WANT_WORD_MATCH if want_word_match else 0) | (WANT_WORD_DECODE if want_word_decode else 0) | (WANT_RUN_SPLIT if want_run_split else 0) | (WANT_TRACK_READ if want_track_read else 0) | (WANT_LATTICE_DECODE if want_lattice_decode else 0) | (WANT_LATTICE_MATCH if want_lattice_match else 0) | (WANT_LATTICE_TRACK if want_lattice_track else 0) | (WANT_TRACK_DECODE if want_track_decode else 0)
        keep = [_row_view(f, 3) for f in frames]
        refs = [ImageRef(_np_ptr(a), a.shape[1], a.shape[0], a.strides[0]) for a in keep]
        arr = (ImageRef * max(1, len(refs)))(*refs)
        t = C.c_uint64()
        self._check(self.L.str_er_stream_submit_copy_list(self.h, arr, len(refs), stages, C.byref(t)))
        return int(t.value)

    def pending(self) -> int:
        return int(self.L.str_er_stream_pending(self.h))

    def next(self):
        """(ticket, Result) of the oldest submitted batch; blocks until it is done."""
        rh, t = C.c_void_p(), C.c_uint64()
        rc = self.L.str_er_stream_next(self.h, C.byref(rh), C.byref(t))
        self._check(rc)
        shim = object.__new__(ERFilter)
        shim.L = self.L
        shim.h = None
        shim._lexicon = getattr(self, "_lexicon", ())
        return int(t.value), ERFilter._collect(shim, rh, profile={})
