"""The numpy reference of the reading of glyph runs (STR_ER_WANT_RUN_READ, str_er_feet_read): the contract at str_er_run_read
(include/str_er.h).  Tiles come from boolean footprints, runs from line_words_ref.py and features from the oracle's chain_features
(OCR::chain_run up to the SVM input).  It shares no code with the library."""
import numpy as np

import line_words_ref as LW

TABLE = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz&()"        # src/OCR.cpp:10


def ocr_char(label):
    return TABLE[label] if 0 <= label < 65 else "?"


def tile_of(bits, x, y, run):
    """The tile of a run (x0, x1, y0, y1, ...) of the footprint `bits` (h, w) bool at (x, y): 0 where the line's own footprint has
    the pixel, else 255."""
    x0, x1, y0, y1 = run[:4]
    assert x <= x0 < x1 <= x + bits.shape[1] and y <= y0 < y1 <= y + bits.shape[0]
    return np.where(bits[y0 - y:y1 - y, x0 - x:x1 - x], 0, 255).astype(np.uint8)


def slope_of(s):
    return float(s) if np.isfinite(s) else 0.0


def tiles(feet, num=1, den=3):
    """(the three tables of line_words_ref.tables, the tile of every run in the order of the run table, the line of every run)."""
    tabs = LW.tables(feet, num, den)
    out, line_of = [], []
    for t, (x, y, bits) in enumerate(feet):
        lw = tabs[0][t]
        for r in tabs[1][lw[2]:lw[2] + lw[3]]:
            out.append(tile_of(np.asarray(bits, bool), x, y, r))
            line_of.append(t)
    return tabs, out, line_of


def features(oracle, feet, slopes=None, num=1, den=3):
    """(tables, (n runs, 1800) uint8 features, tiles): chain_features of every tile as its own box with its line's slope."""
    tabs, tl, line_of = tiles(feet, num, den)
    q = np.zeros((len(tl), 1800), np.uint8)
    for i, (tile, t) in enumerate(zip(tl, line_of)):
        q[i] = oracle.chain_features(tile, slope_of(slopes[t]) if slopes is not None else 0.0)
    return tabs, q, tl


def word_strings(tabs, chars):
    """The string of every word: the characters of its runs."""
    return ["".join(chars[w[1]:w[1] + w[2]]) for w in tabs[2]]
