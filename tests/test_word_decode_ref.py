"""The numpy reference of the word decoder (word_decode_ref.py, written from the definition at str_er_word_decode) against an
enumeration of every path on alphabets of 2 and 3 characters, and the fixed vectors of the contract.  The enumeration walks the paths
the recurrence allows: per run a drop, a reading, and behind either one inserted character that follows some character."""
import numpy as np
import pytest

import word_decode_ref as WD

PAIRS = ((0, 0), (5, 0), (0, 7), (3, 4), (1, 1), (255, 255))


@pytest.mark.parametrize("n", (2, 3))
def test_reference_equals_the_enumeration_of_every_path(n):
    rng = np.random.default_rng(100 + n)
    cases = 0
    for m in range(4):
        for ins, dele in PAIRS:
            for rep in range(30):
                hi = (4, 16, 256)[rep % 3]                      # small ranges tie often
                C = rng.integers(0, hi, (m, n))
                B = rng.integers(0, hi, (n + 1, n + 1))
                rec, lab, src = WD.decode_word(C, B, ins, dele, n)
                assert rec[0] == WD.enumerate_best(C, B, ins, dele, n), (m, ins, dele, C, B)
                assert rec[0] == WD.path_cost(C, B, lab, src, ins, dele, n)
                assert rec[0] <= rec[1] and rec[3] + rec[5] == rec[2] == len(lab) and rec[3] + rec[4] == m
                assert rec[1] == WD.read_cost(C, B, n)
                if ins == 0:
                    assert rec[5] == 0
                if dele == 0:
                    assert rec[4] == 0
                if ins == 0 and dele == 0:
                    assert src == list(range(m))
                cases += 1
    assert cases == 4 * 6 * 30


def test_five_zero_rows():
    rec, lab, src = WD.decode_word(np.zeros((5, 65)), np.zeros((66, 66)), 64, 64)
    assert rec == (0, 0, 5, 5, 0, 0) and lab == [0] * 5 and src == [0, 1, 2, 3, 4]


def insertion_vector():
    C = np.full((32, 65), 255, np.uint8)
    C[:, 63] = 0
    B = np.full((66, 66), 255, np.uint8)
    B[65, 63] = B[63, 64] = B[64, 63] = B[64, 65] = 0
    return C, B


def test_an_insertion_after_every_run():
    C, B = insertion_vector()
    rec, lab, src = WD.decode_word(C, B, 1, 0)
    assert rec[0] == 32 and rec[2:] == (64, 32, 0, 32)
    assert lab == [63, 64] * 32
    assert src == [v for i in range(32) for v in (i, 0x80 | i)]
    assert src[-2:] == [31, 0x9F]


def test_everything_at_255():
    C, B = np.full((33, 65), 255, np.uint8), np.full((66, 66), 255, np.uint8)
    rec, lab, src = WD.decode_word(C[:32], B, 255, 255)
    # a dropped run costs 255 and a read one 510: every run is dropped (on the tie of run 2 onwards SUB stays, but it is dearer in all)
    assert rec == (33 * 255, 65 * 255, 0, 0, 32, 0) and lab == [] and src == []
    rec, lab, src = WD.decode_word(C, B, 255, 255)
    assert rec == (-1, 67 * 255, 0, 0, 0, 0) and lab == []
    recs, chars, srcs = WD.decode_words(C, [0, 0], [32, 33], B, 255, 255)
    assert recs[1][0] == -1 and (chars == 0xFF).all() and (srcs == 0xFF).all()


def test_counts_and_bounds_on_the_full_alphabet():
    rng = np.random.default_rng(7)
    for ins, dele in PAIRS:
        for m in (0, 1, 5, 32):
            C = np.where(rng.random((m, 65)) < 0.1, rng.integers(0, 24, (m, 65)), rng.integers(60, 256, (m, 65)))
            B = rng.integers(0, 256, (66, 66))
            rec, lab, src = WD.decode_word(C, B, ins, dele)
            assert rec[0] == WD.path_cost(C, B, lab, src, ins, dele)
            assert rec[0] <= rec[1] and rec[3] + rec[5] == rec[2] <= 64 and rec[3] + rec[4] == m
            if m == 0:
                assert rec[0] == rec[1] == int(B[65, 65])
