"""The reference of the run reading (run_read_ref.py) on hand-drawn footprints: tiles, features and strings."""
import numpy as np

import run_read_ref as RR

GLYPH = ["..####..",
         ".#....#.",
         "#......#",
         "#......#",
         "########",
         "#......#",
         "#......#",
         "#......#"]


def _bits(rows):
    return np.array([[c == "#" for c in r] for r in rows], bool)


def test_tile_of_a_hand_drawn_glyph(oracle):
    g = _bits(GLYPH)
    foot = np.zeros((10, 20), bool)
    foot[1:9, 0:8] = g                       # the glyph, then a gap, then a bar lower down
    foot[0, 0] = True                        # (the box's first row; part of the first run)
    foot[4:10, 12:20] = True
    tabs, tl, line_of = RR.tiles([(30, 40, foot)])
    assert [r[:5] for r in tabs[1]] == [(30, 38, 40, 49, int(g.sum()) + 1), (42, 50, 44, 50, 48)] and line_of == [0, 0]
    exp = np.full((9, 8), 255, np.uint8)
    exp[1:9][g] = 0
    exp[0, 0] = 0
    assert (tl[0] == exp).all() and tl[0].dtype == np.uint8
    assert tl[1].shape == (6, 8) and (tl[1] == 0).all()                    # a solid rectangle: all 0
    _, q, _ = RR.features(oracle, [(30, 40, foot)])
    assert q.shape == (2, 1800) and (q[0] == oracle.chain_features(exp)).all() and q[0].any()
    _, qs, _ = RR.features(oracle, [(30, 40, foot)], [0.3])
    assert (qs[0] == oracle.chain_features(exp, 0.3)).all() and (qs[0] != q[0]).any()
    _, qn, _ = RR.features(oracle, [(30, 40, foot)], [float("nan")])
    assert (qn == q).all()                                                 # a slope that is not finite counts as 0


def test_only_the_lines_own_pixels():
    a = np.zeros((6, 6), bool)
    a[:, 0] = a[:, 5] = a[0, :] = True       # an open frame: its inside belongs to nobody
    b = np.ones((4, 4), bool)                # another line, solid, inside a's box
    tabs, tl, _ = RR.tiles([(10, 10, a), (11, 11, b)])
    assert len(tl) == 2 and tl[0].shape == (6, 6)
    assert (tl[0] == np.where(a, 0, 255)).all() and (tl[0][1:5, 1:5] == 255).all()
    assert (tl[1] == 0).all()


def test_chars_and_strings():
    assert [RR.ocr_char(k) for k in (0, 9, 10, 35, 36, 61, 62, 64, 65, -1)] == ["0", "9", "A", "Z", "a", "z", "&", ")", "?", "?"]
    foot = np.zeros((2, 12), bool)
    foot[:, [0, 2, 8, 11]] = True            # colmax 2: gaps of 1 break at 1 / 3
    tabs, tl, _ = RR.tiles([(0, 0, foot)], 65535, 1)
    assert RR.word_strings(tabs, list("abcd")) == ["abcd"]
    tabs, _, _ = RR.tiles([(0, 0, foot)], 3, 1)                            # a break at a gap of 6 and more
    assert RR.word_strings(tabs, list("abcd")) == ["abcd"]
    tabs, _, _ = RR.tiles([(0, 0, foot)], 2, 1)                            # ... of 4 and more: 2..8 has 5 columns between
    assert RR.word_strings(tabs, list("abcd")) == ["ab", "cd"]
