"""The numpy reference of the splitting of touching glyphs (run_split_ref.py, written from the definition at str_er_run_split): the
hand profiles of the contract are what they claim to be, footprints give the pieces the definition names, and the recurrence equals
the brute force over every composition of the atoms."""
import numpy as np
import pytest

import run_split_ref as RS

# (profile, H, the kept cuts)
HAND = (
    ([8, 8, 1, 8, 8], 8, [2]),
    ([1, 8, 8, 8, 1], 8, []),                                   # low columns at the ends are no valley
    ([8, 2, 8], 8, [1]),                                        # n == thr
    ([8, 3, 8], 8, []),                                         # n == thr + 1
    ([3, 1, 3], 3, []),                                         # thr 0
    ([9, 1, 1, 1, 1, 9], 12, [2]),
    ([9, 1, 2, 3, 2, 1, 9], 12, [3]),                           # the cut column is no minimum column
    ([9, 2, 9, 1, 9, 2, 9, 1, 9, 3, 9], 12, [1, 3, 7]),         # five valleys: depth 3 and the second of depth 2 lose
)


@pytest.mark.parametrize("profile,H,want", HAND)
def test_hand_profiles(profile, H, want):
    got, thr = RS.cuts(profile, H)
    assert got == want and thr == H // 4
    for p in got:
        assert 0 < p < len(profile) - 1 and profile[p] <= thr


def test_hand_profile_details():
    assert RS.threshold(8) == 2 and RS.threshold(3) == 0 and RS.threshold(12) == 3
    assert RS.valleys([9, 1, 2, 3, 2, 1, 9], 3) == [(1, 3, 1, 6)]
    v = RS.valleys([9, 2, 9, 1, 9, 2, 9, 1, 9, 3, 9], 3)
    assert [(d, p) for d, p, _, _ in v] == [(2, 1), (1, 3), (2, 5), (1, 7), (3, 9)]
    assert RS.cuts([8] * 500 + [1] + [8] * 524, 8)[0] == [] and RS.cuts([8] * 500 + [1] + [8] * 523, 8)[0] == [500]      # 1025 / 1024 columns
    assert RS.cuts([8, 8, 1, 8, 8], 8, 1, 65535)[0] == [] and RS.cuts([8, 8, 8, 8, 8], 8, 65535, 65535)[0] == []


def test_pieces_of_a_footprint():
    b = np.zeros((8, 9), bool)
    b[:, 0:3] = True
    b[2, 3] = True                                              # the valley: one pixel, row 2
    b[1:5, 4:6] = True                                          # an atom whose row extent is tighter than the run's
    b[0, 6] = True                                              # a second valley
    b[:, 7:9] = True
    tabs, splits, pieces, line_of = RS.tables([(10, 20, b)])
    assert tabs[1] == [(10, 19, 20, 28, 8 * 3 + 1 + 8 + 1 + 16, 0)] and line_of == [0]
    assert splits == [(2, 13, 16, -1, 2, 0, 5, 0)]
    assert [p[1:3] for p in pieces] == [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)] == RS.piece_nodes(3)
    assert pieces[0] == (0, 0, 1, 10, 13, 20, 28, 24) and pieces[2] == (0, 1, 2, 13, 16, 21, 25, 9) and pieces[4] == (0, 2, 3, 16, 19, 20, 28, 17)
    assert [len(RS.piece_nodes(A)) for A in (1, 2, 3, 4)] == [0, 2, 5, 9]
    tl = RS.piece_tiles([(10, 20, b)], pieces, line_of)
    assert tl[2].shape == (4, 3) and tl[2].tolist() == [[255, 0, 0], [0, 0, 0], [255, 0, 0], [255, 0, 0]]


def test_recurrence_equals_brute_force():
    rng = np.random.default_rng(77)
    n = 0
    for split in (0, 8, 255):
        for _ in range(700):
            A = int(rng.integers(1, 5))
            hi = int(rng.choice([3, 16, 256]))                 # small ranges tie often
            m = {(i, j): int(rng.integers(0, hi)) for i in range(A) for j in range(i + 1, A + 1)}
            assert RS.segment_dp(m, A, split) == RS.segment_brute(m, A, split), (m, A, split)
            n += 1
    assert n >= 2000 and [len(RS.compositions(A)) for A in (1, 2, 3, 4)] == [1, 2, 4, 8]
