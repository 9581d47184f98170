"""The numpy reference of the word decoder's margins (word_margin_ref.py, written from the definition at str_er_word_margin): its
backward form against an enumeration of every path on alphabets of 2 and 3 characters and against forward passes with one row forced
to one reading at the library's 65; the identities of the contract; the host entry point (str_er_word_margins_host) against it with
==; and the C++ rules check under the host sanitizers, a program of its own.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import word_decode_ref as WD
import word_margin_ref as WG
from test_word_decode_ref import PAIRS, insertion_vector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(rng, m, n=65):
    return np.where(rng.random((m, n)) < 0.1, rng.integers(0, 24, (m, n)), rng.integers(60, 256, (m, n)))


@pytest.mark.parametrize("n", (2, 3))
def test_backward_form_equals_the_enumeration_of_every_path(n):
    rng = np.random.default_rng(200 + n)
    cases = 0
    for m in (1, 2, 3):
        for ins, dele in PAIRS:
            for rep in range(10):
                hi = (4, 16, 256)[rep % 3]                      # small ranges tie often
                C = rng.integers(0, hi, (m, n))
                B = rng.integers(0, hi, (n + 1, n + 1))
                cost, M = WG.marginals_backward(C, B, ins, dele, n)
                assert (M == WG.marginals_enumerated(C, B, ins, dele, n)).all(), (m, ins, dele, C, B)
                assert (M == WG.marginals_forced(C, B, ins, dele, n)).all()
                assert cost == WD.enumerate_best(C, B, ins, dele, n)
                cases += 1
    assert cases == 3 * 6 * 10


@pytest.mark.parametrize("m", (1, 2, 5))
def test_backward_form_equals_the_forced_forward_passes_at_65_labels(m):
    rng = np.random.default_rng(300 + m)
    for k, (ins, dele) in enumerate(PAIRS):
        C = _rows(rng, m)
        B = rng.integers(0, 6 if k % 2 else 256, (66, 66))
        cost, M = WG.marginals_backward(C, B, ins, dele)
        assert (M == WG.marginals_forced(C, B, ins, dele)).all()
        assert ((M[:, 65] >= 0) == (dele > 0)).all() and (M[:, :65] >= 0).all()


def test_the_identities_of_the_contract():
    rng = np.random.default_rng(8)
    for k, (ins, dele) in enumerate(PAIRS):
        for m in (1, 2, 9, 32):
            C = _rows(rng, m)
            B = rng.integers(0, 6 if (k + m) % 2 else 256, (66, 66))
            rec, row_margin, read, alt, M, cost = WG.margins_word(C, B, ins, dele)
            dec, labels, src = WD.decode_word(C, B, ins, dele)
            assert cost == dec[0] and M.shape == (m, 66) and M.max() <= 16575
            for i in range(m):
                assert M[i, read[i]] == cost                                   # the decoded path's own reading
                assert min(int(v) for v in M[i] if v >= 0) == cost             # every path does one of them at run i
                assert row_margin[i] >= 0 and alt[i] != read[i] and M[i, alt[i]] == cost + row_margin[i]
            assert sorted(i for i in range(m) if read[i] != 65) == [r for r in src if not r & 0x80]
            assert rec == (min(row_margin), row_margin.index(min(row_margin)), read[rec[1]], alt[rec[1]])
    assert WG.margins_word(np.zeros((0, 65)), np.zeros((66, 66)))[0] == (-1, -1, -1, -1)
    assert WG.margins_word(np.zeros((33, 65)), np.zeros((66, 66)))[0] == (-1, -1, -1, -1)
    # all zero: every reading ties, the string reads 0 everywhere and 1 is the smallest other label
    rec, row_margin, read, alt, M, cost = WG.margins_word(np.zeros((5, 65)), np.zeros((66, 66)), 64, 64)
    assert rec == (0, 0, 0, 1) and row_margin == [0] * 5 and read == [0] * 5 and alt == [1] * 5 and (M[:, :65] == 0).all() and (M[:, 65] == 64).all()
    # all 255 at 32 rows: the largest marginals there are
    full = np.full((32, 65), 255)
    rec, row_margin, read, alt, M, cost = WG.margins_word(full, np.full((66, 66), 255), 0, 0)
    assert cost == 65 * 255 == 16575 and (M[:, :65] == 16575).all() and (M[:, 65] == -1).all() and rec == (0, 0, 0, 1)
    rec, row_margin, read, alt, M, cost = WG.margins_word(full, np.full((66, 66), 255), 255, 255)
    assert cost == 33 * 255 and read == [65] * 32 and (M[:, 65] == cost).all() and alt == [0] * 32 and rec == (255, 0, 65, 0)
    # an insertion after every run: the inserted characters have no row, every row reads 63
    C, B = insertion_vector()
    rec, row_margin, read, alt, M, cost = WG.margins_word(C, B, 1, 0)
    assert cost == 32 and read == [63] * 32 and min(row_margin) > 0


def test_the_host_entry_point_equals_the_reference(S):
    rng = np.random.default_rng(9)
    n_of = np.array([0, 1, 2, 8, 9, 16, 17, 31, 32, 33], np.int32)
    first = np.concatenate([[0], np.cumsum(n_of)])[:len(n_of)].astype(np.int32)
    costs = _rows(rng, int(n_of.sum())).astype(np.uint8)
    for k, (ins, dele) in enumerate(PAIRS):
        B = rng.integers(0, 6 if k % 2 else 256, (66, 66)).astype(np.uint8)
        rec, rm, rr, ra, mg = S.word_margins_host(costs, first, n_of, B, ins, dele, want_marginals=True)
        want = WG.word_margins(costs, first, n_of, B, ins, dele)
        assert rec.dtype == S.WORD_MARGIN_DTYPE and WG.as_tuples(rec) == want[0]
        assert (rm == want[1]).all() and (rr == want[2]).all() and (ra == want[3]).all() and (mg == want[4]).all()
        again = S.word_margins_host(costs, first, n_of, B, ins, dele)
        assert again[4] is None and again[0].tobytes() == rec.tobytes() and again[1].tobytes() == rm.tobytes()
    # two words over the same rows, and the checks of the decoder's host entry point
    rec, rm, rr, ra, mg = S.word_margins_host(costs, [0, 0], [5, 5], B, 3, 4, want_marginals=True)
    assert rec[0].tobytes() == rec[1].tobytes() and mg[0].tobytes() == mg[1].tobytes()
    for bad in (([1], [len(costs)]), ([0], [-1]), ([-1], [1])):
        with pytest.raises(S.StrErError) as e:
            S.word_margins_host(costs, *bad, B, 0, 0)
        assert e.value.code == -1
    with pytest.raises(S.StrErError):
        S.word_margins_host(costs, [0], [1], B, 256, 0)
    rec, rm, rr, ra, mg = S.word_margins_host(np.zeros((0, 65), np.uint8), [], [], B)
    assert rec.shape == (0,) and rm.shape == (0, 32) and rr.shape == (0, 32) and ra.shape == (0, 32)


def test_word_margin_rules_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "word_margin_rules_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    "-Werror", os.path.join(ROOT, "tests", "cpp", "word_margin_rules_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.endswith(" 0 wrong") and int(last.split()[0]) > 1000, out.stdout
