"""The numpy reference of the lexicon match over the piece lattice (lattice_match_ref.py) against the definition's second form and its
consequences: the recurrence equals the enumeration over all segmentations of the plain matcher (word_match_ref) plus SPLIT per part
beyond the runs; without cuts it is the plain matcher; the three properties of the contract; the backtrack's parts and sources give the
cost back when they are priced again.  No library, no GPU."""
import itertools

import numpy as np
import pytest

import lattice_decode_ref as LD
import lattice_match_ref as LM
import run_split_ref as RS
import word_match_ref as WM

PARAMS = ((64, 64, 8), (1, 1, 0), (255, 255, 255), (3, 200, 8))          # INS, DEL, SPLIT


def make_word(rng, n_cuts, hi=256, cheap=True):
    """(first pieces, run rows, piece rows) of a word with the given cut counts."""
    npc = [LD.n_pieces(int(k)) for k in n_cuts]
    fp = np.concatenate([[0], np.cumsum(npc)[:-1]]).astype(int) if len(npc) else np.zeros(0, int)
    rows = lambda n: rng.integers(0, hi, (n, 65)).astype(np.uint8)
    rr, pr = rows(len(n_cuts)), rows(int(sum(npc)))
    if cheap:                                                            # a tenth of the bytes made cheap, so that paths differ by more than noise
        rr = np.where(rng.random(rr.shape) < 0.1, rr // 8, rr).astype(np.uint8)
        pr = np.where(rng.random(pr.shape) < 0.1, pr // 8, pr).astype(np.uint8)
    return fp, rr, pr


def random_entries(rng, n, l):
    return rng.integers(0, 65, (n, l))


@pytest.mark.parametrize("ins,dele,split", PARAMS)
def test_the_recurrence_equals_the_enumeration_over_all_segmentations(ins, dele, split):
    rng = np.random.default_rng(31)
    k = 0
    for R in (1, 2, 3):
        for cuts in itertools.product(range(4), repeat=R):               # every cut count of every run
            fp, rr, pr = make_word(rng, cuts)
            k += 1
            fold = bool(k & 1)                                           # (the fold and the shortest length in turn: 84 words a parameter set)
            L = LM.lattice(cuts, fp, rr, pr, 0, fold)
            for l in sorted({1 if k % 3 == 0 else max(1, R - 1), L.N, L.N + 2}):
                E = random_entries(rng, 3, l)
                assert LM.entry_costs(L, E, ins, dele, split).tolist() == LM.enumerate_costs(L, E, ins, dele, split).tolist(), (cuts, l, fold)


def test_without_cuts_it_is_the_plain_matcher():
    rng = np.random.default_rng(32)
    words = ["".join(WM.ALPHABET[a] for a in rng.integers(0, 65, int(l))) for l in rng.integers(1, 9, 300)] + ["a" * 32, "Zz9" * 10]
    for fold in (False, True):
        lex = WM.Lexicon(words, fold)
        for m in (0, 1, 2, 5, 7, 32, 33):
            fp, rr, pr = make_word(rng, [0] * m)
            for ins, dele, split in PARAMS:
                for band in (0, 2, 31):
                    rec, src, parts = LM.match_word([0] * m, fp, rr, pr, lex, ins, dele, band, split)
                    assert rec[:6] == WM.match_word(rr, lex, ins, dele, band), (m, band)
                    if rec[0] >= 0:
                        assert parts == [(r, -1) for r in range(m)] and rec[6] == m


def test_the_three_properties_on_random_words():
    rng = np.random.default_rng(33)
    words = ["".join(WM.ALPHABET[a] for a in rng.integers(0, 65, int(l))) for l in rng.integers(1, 12, 400)]
    lex = WM.Lexicon(words, True)
    cut_words = 0
    for _ in range(40):
        R = int(rng.integers(1, 6))
        cuts = rng.integers(0, 4, R)
        fp, rr, pr = make_word(rng, cuts)
        ins, dele, split = PARAMS[int(rng.integers(0, 4))]
        band = int(rng.integers(0, 4))
        rec, src, parts = LM.match_word(cuts, fp, rr, pr, lex, ins, dele, band, split)
        # (2) the plain matcher on the unsplit runs
        plain = WM.match_word(rr, lex, ins, dele, band)
        if plain[5] > 0:
            assert rec[5] >= plain[5] and 0 <= rec[1] <= plain[1]
        # (3) the plain matcher on the split sequence of str_er_run_split, plus SPLIT per part beyond the runs
        sp = [(int(k), -1, -1, -1, 0, int(f), LD.n_pieces(int(k)), 0) for k, f in zip(cuts, fp)]
        ws, pt, prow = RS.split_words(sp, rr, pr, [0], [R], split)
        seq = WM.match_word(prow, lex, ins, dele, band)
        if seq[5] > 0:
            assert rec[5] >= seq[5] and rec[1] <= seq[1] + split * (len(pt) - R)
        assert rec[4] == ws[0][2]                                        # free_cost is the word split's cost
        cut_words += int(cuts.max() > 0)
    assert cut_words >= 20


def test_the_backtrack_gives_the_cost_back_and_the_counts_add_up():
    rng = np.random.default_rng(34)
    for trial in range(60):
        R = int(rng.integers(0, 5))
        cuts = rng.integers(0, 4, R)
        fp, rr, pr = make_word(rng, cuts, hi=256 if trial % 3 else 4)    # (small values: many ties)
        ins, dele, split = PARAMS[trial % 4] if trial % 5 else (2, 2, 1)
        fold = bool(trial & 1)
        L = LM.lattice(cuts, fp, rr, pr, 0, fold)
        l = int(rng.integers(1, L.N + 4))
        e = rng.integers(0, 65, l).tolist()
        cost, parts, src, n_del, n_ins = LM.backtrack(L, e, ins, dele, split)
        assert cost == int(LM.entry_costs(L, [e], ins, dele, split)[0])
        assert LM.path_cost(L, e, src, parts, ins, dele, split) == cost
        assert len(parts) - n_del + n_ins == l and R <= len(parts) <= L.N
        assert sum(1 for t in src if t & 0x80) == n_ins


def test_the_tie_rules_of_the_backtrack_on_constant_rows():
    """Every row 3 everywhere, INS = DEL = 3, SPLIT = 0: every move costs the same, so the order of the candidates decides."""
    cuts = [3]
    fp, rr, pr = [0], np.full((1, 65), 3, np.uint8), np.full((9, 65), 3, np.uint8)
    L = LM.lattice(cuts, fp, rr, pr)
    # one character against four atoms: SUB(0) at the last node comes first -- the whole run is read
    cost, parts, src, n_del, n_ins = LM.backtrack(L, [5], 3, 3, 0)
    assert (cost, parts, src, n_del, n_ins) == (3, [(0, 0, 4)], [0], 0, 0)
    # two characters: at (4, 2) SUB(0) attains 6 (INS 3 at node 0, then the whole run): smaller i before a later split
    cost, parts, src, n_del, n_ins = LM.backtrack(L, [5, 6], 3, 3, 0)
    assert (cost, parts, src, n_del, n_ins) == (6, [(0, 0, 4)], [0x80, 0], 0, 1)
    # with a costly INS the two characters take two parts: the first split the order allows is (0, 1) + (1, 4)
    cost, parts, src, n_del, n_ins = LM.backtrack(L, [5, 6], 100, 3, 0)
    assert (cost, parts, src, n_del, n_ins) == (6, [(0, 0, 1), (0, 1, 4)], [0, 1], 0, 0)
