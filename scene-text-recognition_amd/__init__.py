"""scene-text-recognition_amd -- MI355X (gfx950) extremal-region text-detection hot path.

Python binding (ctypes) of the C ABI in include/str_er.h.  The directory name carries a
hyphen (it follows the reference's repository name), so import it with

    import importlib; str_er = importlib.import_module("scene-text-recognition_amd")

or through the alias module `str_er_amd` at the repository root.

Everything here forwards to libstr_er_hip.so: there is no Python or CPU implementation
of the path, and loading fails loudly if the HIP library has not been built.
"""
from __future__ import annotations

from .binding import (  # noqa: F401
    CLS_POOL, CLS_STRONG, CLS_WEAK, STAGE_ALL, STAGE_CLASSIFY, STAGE_OCR, STAGE_EXTRACT, STAGE_NMS, STAGE_TRACK, STAGE_GROUP, GROUP_INNER_SUP, GROUP_OVERLAP_SUP, STAGE_OCR_LINES, TRACK_DTYPE, TEXT_DTYPE, GBOUND_DTYPE, WANT_NODES, WANT_MASKS, MASK_DTYPE, unpack_mask, WANT_SHAPES, SHAPE_DTYPE, WANT_STROKES, STROKE_DTYPE, WANT_LINE_CROPS, WANT_LINE_GLYPHS, LINE_CROP_DTYPE, line_crop_geometry,
    WANT_TEXT_MAP, WANT_LINE_MAP, TEXT_MAP_STRONG, TEXT_MAP_WEAK, TEXT_MAP_LINE, TEXT_MAP_OCR, FRAME_MAP_DTYPE,
    WANT_LINE_GEOM, LINE_GEOM_DTYPE, hull_of_points, quad_from_hull,
    WANT_LINE_WORDS, LINE_RUN_DTYPE, LINE_WORD_DTYPE, LINE_WORDS_DTYPE, words_from_runs, WANT_RUN_READ, RUN_READ_DTYPE, ocr_char,
    WANT_WORD_MATCH, LEXICON_FOLD_CASE, WORD_MATCH_DTYPE, cost_thresholds, prob_costs, match_words_host,
    WANT_WORD_DECODE, WORD_DECODE_DTYPE, bigram_from_probs, bigram_from_words, load_tp_table, decode_words_host,
    WORD_MARGIN_DTYPE, word_margins_host,
    LINE_DECODE_DTYPE, line_gap_costs, decode_lines_host, LINE_MARGIN_DTYPE, line_margins_host,
    WANT_RUN_SPLIT, RUN_SPLIT_DTYPE, RUN_PIECE_DTYPE, SPLIT_PART_DTYPE, WORD_SPLIT_DTYPE, cuts_from_counts, split_words_host,
    WANT_LATTICE_DECODE, LATTICE_DECODE_DTYPE, lattice_decode_words_host, LINE_LATTICE_DECODE_DTYPE, lattice_decode_lines_host, line_lattice_node_slots,
    LATTICE_MARGIN_DTYPE, lattice_margins_host,
    WANT_LATTICE_MATCH, LATTICE_MATCH_DTYPE, lattice_match_words_host,
    WANT_LATTICE_TRACK, LATTICE_TRACK_MEMBER_DTYPE, lattice_match_tracks_host,
    WANT_TRACK_READ, WORD_LINK_DTYPE, WORD_TRACK_DTYPE, TRACK_MATCH_DTYPE, word_links, word_tracks_from_links, match_tracks_host,
    WANT_TRACK_DECODE, TRACK_DECODE_DTYPE, decode_tracks_host, lattice_decode_tracks_host,
    POOL_MATCH_DTYPE, POOL_LATTICE, TrackPool, WordTracker, POOL_DECODE_DTYPE, POOL_DECODE, DecodePool, LatticeDecodePool,
    WANT_LINE_LINKS, LINE_LINK_DTYPE, TEXT_TRACK_DTYPE, text_tracks_from_links, EdgeFeet, TextTracker,
    WANT_FRAME_LINES, LINE_FOOT_DTYPE, LINE_PAIR_DTYPE, FRAME_LINE_DTYPE, frame_lines_from_pairs,
    CAND_DTYPE, NODE_DTYPE, PLANE_DTYPE, ERFilter, FrameStream, PlaneResult, Params, Result, StrErError, apply_runtime_hint, set_batch_slots, lib_path, load_library,
    flood_order, Comm, ImageRef,
)
from . import cascade_io, synth  # noqa: F401

__all__ = ["ERFilter", "Params", "Result", "StrErError", "load_library", "lib_path", "cascade_io", "synth",
           "CAND_DTYPE", "NODE_DTYPE"]


def __getattr__(name):
    # `dist` pulls in torch; load it only when somebody asks for it
    if name == "dist":
        import importlib
        return importlib.import_module(__name__ + ".dist")
    raise AttributeError(name)
