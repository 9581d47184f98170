"""The numpy reference of the track match over the members' piece lattices (lattice_track_ref.py) against the contract's second form and
the three identities the contract states: the cost of an entry is the sum over the usable members of the minimum over the member's
segmentations of the plain matcher's cost plus SPLIT per part beyond the runs (lattice_match_ref.enumerate_costs); a track of one usable
member is that word's lattice match; without cuts it is the track match on the runs' rows; where every member is usable it never costs
more than the track match on the unsplit runs.  No library, no GPU."""
import numpy as np
import pytest

import lattice_decode_ref as LD
import lattice_match_ref as LM
import lattice_track_ref as LT
import track_read_ref as TR
import word_match_ref as WM

SPLIT_DTYPE = np.dtype([("n_cuts", "<i4"), ("first_piece", "<i4")])
PARAMS = ((64, 64, 2, 8), (3, 200, 1, 8), (1, 1, 0, 0), (255, 255, 3, 255))          # INS, DEL, band, SPLIT


def make_words(rng, runs_of_words, max_cuts=3, hi=256):
    """(splits, run rows, piece rows, first_run, n_of) of words with the given run counts and random cut counts."""
    n_of = np.asarray(runs_of_words, np.int32)
    first = np.concatenate([[0], np.cumsum(n_of)[:-1]]).astype(np.int32)
    cuts = rng.integers(0, max_cuts + 1, int(n_of.sum()))
    npc = [LD.n_pieces(int(k)) for k in cuts]
    sp = np.zeros(len(cuts), SPLIT_DTYPE)
    sp["n_cuts"], sp["first_piece"] = cuts, np.concatenate([[0], np.cumsum(npc)[:-1]]) if len(cuts) else []
    rows = lambda n: rng.integers(0, hi, (n, 65)).astype(np.uint8)
    rr, pr = rows(len(cuts)), rows(int(sum(npc)))
    rr = np.where(rng.random(rr.shape) < 0.1, rr // 8, rr).astype(np.uint8)
    pr = np.where(rng.random(pr.shape) < 0.1, pr // 8, pr).astype(np.uint8)
    return sp, rr, pr, first, n_of


def lexicon(rng, n, lo, hi, fold, labels=12):
    return WM.Lexicon(["".join(WM.ALPHABET[a] for a in rng.integers(65 - labels, 65, int(l))) for l in rng.integers(lo, hi + 1, n)], fold)


@pytest.mark.parametrize("ins,dele,band,split", PARAMS)
def test_the_sum_of_the_members_enumerations(ins, dele, band, split):
    rng = np.random.default_rng(51 + ins)
    for trial in range(6):
        sp, rr, pr, first, n_of = make_words(rng, rng.integers(0, 4, 4))
        members = [int(w) for w in rng.integers(0, 4, int(rng.integers(1, 4)))]          # (a word may be a member twice)
        lex = lexicon(rng, 60, 1, 9, bool(trial & 1))
        rec, mrec, src, parts = LT.match_track(sp, rr, pr, first, n_of, members, lex, ins, dele, band, split)
        lats = [LT.word_lattice(sp, rr, pr, first, n_of, w, lex.fold) for w in members]
        keys = []
        for l, (ix, E) in lex.by_len.items():
            if any(max(1, len(L.atoms) - band) <= l <= min(32, L.N + band) for L in lats):
                total = sum(LM.enumerate_costs(L, E, ins, dele, split) if L.N else np.full(len(ix), l * ins) for L in lats)
                keys += list(zip(np.asarray(total).tolist(), ix.tolist()))
        keys.sort()
        assert rec[5] == len(keys) and rec[6] == len(members)
        assert rec[:4] == ((keys[0][1], keys[0][0]) if keys else (-1, -1)) + ((keys[1][1], keys[1][0]) if len(keys) > 1 else (-1, -1))
        if keys:
            assert sum(m[0] for m in mrec) == rec[1]
            for L, m, s, pt in zip(lats, mrec, src, parts):
                e = [WM.LABEL_OF[ch] for ch in lex.words[rec[0]]]
                assert m[1] - m[2] + m[3] == len(e) and len(pt) == m[1] and len(s) == len(e)


def test_a_track_of_one_member_is_that_words_lattice_match():
    rng = np.random.default_rng(52)
    sp, rr, pr, first, n_of = make_words(rng, [0, 1, 2, 3, 5, 9])
    for ins, dele, band, split in PARAMS:
        lex = lexicon(rng, 120, 1, 12, True)
        for w in range(len(first)):
            rec, mrec, src, parts = LT.match_track(sp, rr, pr, first, n_of, [w], lex, ins, dele, band, split)
            f, k = int(first[w]), int(n_of[w])
            one = LM.match_word(sp["n_cuts"][f:f + k].tolist(), sp["first_piece"][f:f + k].tolist(), rr, pr, lex, ins, dele, band, split, f)
            assert rec[:6] == one[0][:6] and rec[6] == (1 if sum(sp["n_cuts"][f:f + k] + 1) <= 32 else 0)
            if rec[0] >= 0:
                assert (mrec[0][0],) + mrec[0][1:4] == (one[0][1],) + one[0][6:9] and src[0] == one[1] and parts[0] == one[2] and rec[7] == w
            else:
                assert mrec[0][:4] == (-1, 0, 0, 0) and rec[7] == -1


def test_without_cuts_it_is_the_track_match_on_the_runs():
    rng = np.random.default_rng(53)
    sp, rr, pr, first, n_of = make_words(rng, [0, 1, 2, 4, 8, 9, 32, 33, 3, 3], max_cuts=0)
    tracks = [[1], [2, 3, 8], [0, 4, 5], [6, 7, 9], [7], [8, 9, 8]]
    for ins, dele, band, split in PARAMS:
        lex = lexicon(rng, 150, 1, 10, False)
        for members in tracks:
            rec, mrec, src, parts = LT.match_track(sp, rr, pr, first, n_of, members, lex, ins, dele, band, split)
            plain, mc = TR.match_track(rr, first, n_of, members, lex, ins, dele, band)
            assert rec == plain and [m[0] for m in mrec] == mc
            for w, m, pt in zip(members, mrec, parts):
                if m[0] >= 0:
                    assert pt == [(int(first[w]) + t, -1) for t in range(int(n_of[w]))]


def test_it_never_costs_more_than_the_track_match_on_the_unsplit_runs():
    rng = np.random.default_rng(54)
    cut_members = 0
    for trial in range(12):
        sp, rr, pr, first, n_of = make_words(rng, rng.integers(1, 5, 5))
        members = [int(w) for w in rng.integers(0, 5, int(rng.integers(1, 5)))]
        ins, dele, band, split = PARAMS[trial % 4]
        lex = lexicon(rng, 150, 1, 10, bool(trial & 2))
        rec, mrec, src, parts = LT.match_track(sp, rr, pr, first, n_of, members, lex, ins, dele, band, split)
        plain, mc = TR.match_track(rr, first, n_of, members, lex, ins, dele, band)
        if plain[5] > 0:
            assert rec[5] >= plain[5] and 0 <= rec[1] <= plain[1]
        cut_members += sum(int(sp["n_cuts"][int(first[w]):int(first[w]) + int(n_of[w])].max() > 0) for w in members)
    assert cut_members >= 10


def test_every_track_of_a_call_and_the_slots_of_no_track():
    rng = np.random.default_rng(55)
    sp, rr, pr, first, n_of = make_words(rng, [2, 1, 3, 2])
    lex = lexicon(rng, 80, 1, 8, True)
    members = [0, 1, 3, 2, 2, 0]
    out, mrec, src, parts = LT.match_tracks(sp, rr, pr, first, n_of, [0, 3], [2, 2], members, lex)          # (slots 2 and 5: of no track)
    assert len(out) == 2 and mrec[2][0] == mrec[5][0] == -1 and mrec[2][5] == mrec[5][5] == -1 and (src[2] == 255).all()
    assert [m[1] for m in mrec] == np.concatenate([[0], np.cumsum([m[2] for m in mrec])])[:-1].tolist() and len(parts) == sum(m[2] for m in mrec)
    one = LT.match_track(sp, rr, pr, first, n_of, [2, 2], lex)
    assert out[1] == one[0] and out[1][7] == 2 and mrec[3][0] == mrec[4][0]          # (the same word twice: the earlier slot is the best member)
