"""The host statement of the track decode (str_er_decode_tracks_host, csrc/track_decode_rules.h: prefix and suffix tables) against the
numpy reference (track_decode_ref.py: the full recurrence for every neighbour), every value with ==, and the five properties the
contract lists.  CPU only.  The tracks are made by the recipe of the issue: a truth string of 3 .. 9 labels and 2 .. 8 members that
drop, add and confuse runs; the generator's seed was chosen so that the tracks contain what test_the_tracks_cover_the_search asserts."""
import numpy as np
import pytest

import track_decode_ref as TD
import word_decode_ref as WD

SEED = 5
N_TRACKS = 14
ROUNDS = 8


def make_case(seed=SEED, n_tracks=N_TRACKS):
    rng = np.random.default_rng(seed)
    B = rng.integers(0, 90, (66, 66)).astype(np.uint8)
    tracks = []
    for _ in range(n_tracks):
        truth = [int(a) for a in rng.integers(0, 65, int(rng.integers(3, 10)))]
        tracks.append(TD.make_track(rng, truth, int(rng.integers(2, 9))))
    return B, TD.pack(tracks)


@pytest.fixture(scope="module")
def case():
    B, packed = make_case()
    runs = {(di, dd, r): TD.decode_tracks(*packed, B, di, dd, 64, 64, r) for di, dd, r in ((0, 0, ROUNDS), (0, 0, 1), (0, 0, 0), (64, 64, ROUNDS))}
    return B, packed, runs


def test_the_tracks_cover_the_search(case):
    """With the reference alone: the tracks hold every kind of step the search can take."""
    _, _, runs = case
    recs, _, _, edits = runs[(0, 0, ROUNDS)]
    assert any(r[3] >= 2 for r in recs)                              # n_edits >= 2
    assert any(r[3] == 0 and r[4] == 1 for r in recs)                # the set median is a local optimum already
    assert all(r[4] == 1 for r in recs)                              # all converge within 8 rounds
    assert any(r[4] == 0 for r in runs[(0, 0, 1)][0])                # left unconverged at rounds = 1
    kinds = {k for ed in edits for k, _, _ in ed}
    assert kinds == {"SUB", "DEL", "INS"}


def test_host_equals_the_reference(S, case):
    B, packed, runs = case
    for (di, dd, rounds), (recs, chars, mc, _) in runs.items():
        got, ch, own = S.decode_tracks_host(*packed, B, di, dd, 64, 64, rounds)
        assert TD.as_tuples(got) == recs, (di, dd, rounds)
        assert (ch == chars).all() and own.tolist() == mc.tolist(), (di, dd, rounds)
    few = packed[:3] + (packed[3][:4], packed[4][:4], packed[5])          # the first four tracks, other INS / DEL
    for ins, dele in ((1, 255), (255, 1), (40, 90)):
        recs, chars, mc, _ = TD.decode_tracks(*few, B, 0, 0, ins, dele, 3)
        got, ch, own = S.decode_tracks_host(*few, B, 0, 0, ins, dele, 3)
        assert TD.as_tuples(got) == recs and (ch == chars).all() and own.tolist() == mc.tolist(), (ins, dele)


def test_the_five_properties(S, case):
    B, packed, _ = case
    costs, first, n_of, tf, tc, members = packed
    for rounds in (0, 1, ROUNDS):
        got, ch, own = S.decode_tracks_host(*packed, B, 0, 0, 64, 64, rounds)
        dec, dchars, _ = S.decode_words_host(costs, first, n_of, B, 0, 0)
        for g, r in enumerate(got):
            slots = range(int(tf[g]), int(tf[g]) + int(tc[g]))
            rows = [costs[int(first[members[i]]):int(first[members[i]]) + int(n_of[members[i]])] for i in slots]
            s = [int(a) for a in ch[g, :int(r["n_chars"])]]
            # 1. cost = lm_cost + the sum of the member costs >= 0
            assert int(r["cost"]) == int(r["lm_cost"]) + sum(int(own[i]) for i in slots) >= 0
            assert int(r["lm_cost"]) == TD.lm(s, B) and (ch[g, int(r["n_chars"]):] == 0xFF).all()
            # 2. cost <= seed_cost <= J(every seed)
            seeds = [[int(a) for a in dchars[members[i], :int(dec[members[i]]["n_chars"])]] for i in slots if 1 <= int(dec[members[i]]["n_chars"]) <= 32][:32]
            assert int(r["cost"]) <= int(r["seed_cost"]) <= min(TD.score(rows, t, B, 64, 64) for t in seeds)
            # 3. converged = 1: no neighbour scores below cost
            if int(r["converged"]):
                assert min(TD.neighbour_scores(rows, s, B, 64, 64))[0] >= int(r["cost"])
            # 4. rounds = 0: the winning seed's decoder string, byte for byte
            if rounds == 0:
                w = int(r["seed_member"])
                assert (ch[g] == np.where(np.arange(32) < int(dec[w]["n_chars"]), dchars[w, :32], 0xFF)).all() and int(r["n_edits"]) == 0 == int(r["converged"])
                assert int(r["cost"]) == int(r["seed_cost"])
    # 5. a track of one usable member, the decoder's INS = DEL = 0: seed_cost <= the word's decoder cost
    n_words = len(first)
    got, _, _ = S.decode_tracks_host(costs, first, n_of, np.arange(n_words), np.ones(n_words, np.int32), np.arange(n_words), B, 0, 0, 64, 64, 0)
    dec, _, _ = S.decode_words_host(costs, first, n_of, B, 0, 0)
    for w in range(n_words):
        if 1 <= int(n_of[w]) <= 32:
            assert int(got[w]["seed_cost"]) <= int(dec[w]["cost"]) and int(got[w]["seed_member"]) == w and int(got[w]["n_used"]) == 1
            assert WD.decode_word(costs[int(first[w]):int(first[w]) + int(n_of[w])], B)[0][0] == int(dec[w]["cost"])
