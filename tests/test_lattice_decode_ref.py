"""The numpy reference of the joint decode over the piece lattice (lattice_decode_ref.py, written from the definition at
str_er_lattice_decode) against an enumeration of every path, string and choice of moves on an alphabet of 3 characters, against the
reference of the word decoder on lattices without cuts, and the three properties the contract states."""
import itertools

import numpy as np
import pytest

import lattice_decode_ref as LD
import run_split_ref as RS
import word_decode_ref as WD

MOVES = ((0, 0), (5, 0), (0, 7), (3, 4), (255, 255))          # off, each move alone, both


def random_word(rng, cuts, n, hi):
    """Rows of a word whose runs have the given cut counts: (first_piece, run rows, piece rows)."""
    first_piece, at = [], 0
    for k in cuts:
        first_piece.append(at)
        at += LD.n_pieces(k)
    return first_piece, rng.integers(0, hi, (len(cuts), n)), rng.integers(0, hi, (at, n))


SHAPES = [()] + [(a,) for a in range(3)] + list(itertools.product(range(3), repeat=2))          # <= 2 runs of <= 3 atoms


@pytest.mark.parametrize("ins,dele", MOVES)
def test_reference_equals_the_enumeration_of_every_path(ins, dele):
    n = 3
    rng = np.random.default_rng(300 + ins + dele)
    cases = 0
    for cuts in SHAPES:
        for rep in range(6):
            hi = (4, 16, 256)[rep % 3]                              # small ranges tie often
            split = (0, 8, 255)[rep // 2]
            fp, runs, pieces = random_word(rng, cuts, n, hi)
            B = rng.integers(0, hi, (n + 1, n + 1))
            rec, lab, src, parts = LD.decode_word(cuts, fp, runs, pieces, B, ins, dele, split, 0, n)
            assert rec[0] == LD.enumerate_best(cuts, fp, runs, pieces, B, ins, dele, split, n), (cuts, ins, dele, split, runs, pieces, B)
            assert rec[0] == LD.path_cost(LD.Word(cuts, fp, runs, pieces, 0, n), B, lab, src, parts, ins, dele, split, n)
            N = sum(k + 1 for k in cuts)
            assert rec[0] <= rec[1] and rec[3] + rec[5] == rec[2] == len(lab) and rec[3] + rec[4] == rec[6] == len(parts)
            assert len(cuts) <= rec[6] <= N
            if ins == 0:
                assert rec[5] == 0
            if dele == 0:
                assert rec[4] == 0
            cases += 1
    assert cases == 13 * 6


def test_without_cuts_it_is_the_word_decoder():
    rng = np.random.default_rng(11)
    for ins, dele in MOVES:
        for m in (0, 1, 2, 7, 32, 33):
            C = np.where(rng.random((m, 65)) < 0.1, rng.integers(0, 24, (m, 65)), rng.integers(60, 256, (m, 65)))
            B = rng.integers(0, 256, (66, 66))
            rec, lab, src, parts = LD.decode_word([0] * m, [0] * m, C, np.zeros((0, 65)), B, ins, dele, 8)
            wrec, wlab, wsrc = WD.decode_word(C, B, ins, dele)
            assert rec[:6] == wrec and lab == wlab and src == wsrc
            assert parts == ([(r, -1) for r in range(m)] if m <= 32 else []) and rec[6] == len(parts)


def split_sequence(cuts, fp, runs, pieces, split):
    """The rows of the split sequence of str_er_run_split on the same word (run_split_ref.py)."""
    splits = [(k, -1, -1, -1, 0, f, LD.n_pieces(k), 0) for k, f in zip(cuts, fp)]
    return RS.split_words(splits, runs, pieces, [0], [len(cuts)], split)[2].astype(np.int64)


def test_the_three_properties_on_random_words():
    rng = np.random.default_rng(5)
    seen_cut = 0
    for t in range(200):
        ins, dele = MOVES[t % 5]
        split = (0, 8, 255)[t % 3]
        R = int(rng.integers(0, 9))
        cuts = [int(k) for k in rng.integers(0, 4, R)] if t % 4 else [0] * R
        fp, runs, pieces = random_word(rng, cuts, 65, 256)
        runs = np.where(rng.random(runs.shape) < 0.1, runs // 8, runs)
        pieces = np.where(rng.random(pieces.shape) < 0.1, pieces // 8, pieces)
        B = rng.integers(0, 256, (66, 66))
        rec, lab, src, parts = LD.decode_word(cuts, fp, runs, pieces, B, ins, dele, split)
        assert rec[0] == LD.path_cost(LD.Word(cuts, fp, runs, pieces), B, lab, src, parts, ins, dele, split)
        wrec, wlab, wsrc = WD.decode_word(runs, B, ins, dele)
        if not any(cuts):                                             # (1) byte for byte the word decoder, the parts the runs
            assert rec[:6] == wrec and lab == wlab and src == wsrc and parts == [(r, -1) for r in range(R)]
        assert rec[0] <= wrec[0] and rec[1] == wrec[1]                # (2)
        rows = split_sequence(cuts, fp, runs, pieces, split)
        if len(rows) <= 32:                                           # (3)
            srec, _, _ = WD.decode_word(rows, B, ins, dele)
            assert rec[0] <= srec[0] + split * (len(rows) - R)
        seen_cut += any(cuts)
    assert seen_cut >= 100
