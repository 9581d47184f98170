"""The host statement of the track decode over the members' piece lattices (str_er_lattice_decode_tracks_host,
csrc/lattice_track_decode_rules.h: prefix and suffix tables over the nodes) against the numpy reference (lattice_track_decode_ref.py: the
full lattice recurrence for every neighbour), every value with ==, and the seven properties the contract lists.  CPU only.  The tracks
are made by the recipe of the reference: a truth string of 3 .. 7 labels and 2 .. 5 members that drop, add and confuse runs and merge
touching glyphs into runs with 1 .. 3 cuts; the generator's seed was chosen so that the tracks contain what
test_the_tracks_cover_the_search asserts."""
import numpy as np
import pytest

import lattice_decode_ref as LD
import lattice_track_decode_ref as R
import track_decode_ref as TD
import word_match_ref as WM

SEED = 1
N_TRACKS = 8
ROUNDS = 8
SETTINGS = ((0, 0, 64, 64, ROUNDS, 8), (0, 0, 64, 64, 1, 8), (0, 0, 64, 64, 0, 8), (64, 64, 64, 64, ROUNDS, 8))      # dec INS / DEL, INS, DEL, rounds, SPLIT


def make_case(seed=SEED, n_tracks=N_TRACKS):
    rng = np.random.default_rng(seed)
    B = rng.integers(0, 90, (66, 66)).astype(np.uint8)
    tracks = []
    for _ in range(n_tracks):
        truth = [int(a) for a in rng.integers(0, 65, int(rng.integers(3, 8)))]
        tracks.append(R.make_track(rng, truth, int(rng.integers(2, 6))))
    return B, R.pack(tracks)


@pytest.fixture(scope="module")
def case():
    B, packed = make_case()
    return B, packed, {k: R.decode_tracks(*packed, B, *k) for k in SETTINGS}


def parts_list(parts):
    return [[int(p["run"]), int(p["piece"])] for p in parts]


def equal(got, ref):
    out, ch, mrec, src, parts = got
    assert R.as_tuples(out) == ref[0]
    assert (ch == ref[1]).all()
    assert R.members_as_tuples(mrec) == ref[2]
    assert (src == ref[3]).all()
    assert parts_list(parts) == ref[4].tolist()


def test_the_tracks_cover_the_search(S, case):
    """On the reference's output: the tracks hold what makes the comparison worth something."""
    B, packed, runs = case
    sp, rr, pr, first, n_of, tf, tc, members = packed
    recs, chars, mrec, _, parts, edits = runs[SETTINGS[0]]
    assert any(r[3] >= 2 for r in recs)                              # n_edits >= 2
    assert any(r[3] == 0 and r[4] == 1 for r in recs)                # the seed is a local optimum already
    assert sp["n_cuts"].max() == 3 and (sp["n_cuts"] == 1).any() and (sp["n_cuts"] == 2).any()
    # a member whose parts under the track's string differ from its own lattice decode's
    own = LD.decode_words(sp, rr, pr, first, n_of, B, 0, 0, 8)
    differ = 0
    for m in mrec:
        if m[0] >= 0:
            d = own[0][m[5]]
            differ += parts[m[1]:m[1] + m[2]].tolist() != own[3][d[6]:d[6] + d[7]].tolist()
    assert differ >= 1
    # a track whose string differs from the track decode's on the split sequence of str_er_run_split
    ws, pt, prow = S.split_words_host(sp, rr, pr, first, n_of, 8)[:3]
    plain = S.decode_tracks_host(prow, ws["first_part"], ws["n_parts"], tf, tc, members, B, 0, 0, 64, 64, ROUNDS)
    assert sum(int((plain[1][g] != chars[g]).any()) for g in range(len(recs))) >= 1


def test_host_equals_the_reference(S, case):
    B, packed, runs = case
    for k, ref in runs.items():
        equal(S.lattice_decode_tracks_host(*packed, B, *k), ref)
    few = packed[:5] + (packed[5][:3], packed[6][:3], packed[7])          # the first three tracks, other INS / DEL / SPLIT
    for ins, dele, split in ((1, 255, 0), (255, 1, 255), (40, 90, 8), (64, 64, 0)):
        equal(S.lattice_decode_tracks_host(*few, B, 0, 0, ins, dele, 3, split), R.decode_tracks(*few, B, 0, 0, ins, dele, 3, split))


def test_the_first_four_properties(S, case):
    B, packed, _ = case
    sp, rr, pr, first, n_of, tf, tc, members = packed
    dec, dchars, _, _ = S.lattice_decode_words_host(sp, rr, pr, first, n_of, B, 0, 0, 8)
    for rounds in (0, 1, ROUNDS):
        out, ch, mrec, src, parts = S.lattice_decode_tracks_host(*packed, B, 0, 0, 64, 64, rounds, 8)
        for g, r in enumerate(out):
            slots = range(int(tf[g]), int(tf[g]) + int(tc[g]))
            lats = [R.word_lattice(sp, rr, pr, first, n_of, int(members[i])) for i in slots]
            s = [int(a) for a in ch[g, :int(r["n_chars"])]]
            # 1. cost = lm_cost + the sum of the member costs
            assert int(r["cost"]) == int(r["lm_cost"]) + sum(int(mrec[i]["cost"]) for i in slots)
            assert int(r["lm_cost"]) == TD.lm(s, B) and (ch[g, int(r["n_chars"]):] == 0xFF).all()
            # 2. cost <= seed_cost <= J(every seed)
            seeds = [[int(a) for a in dchars[members[i], :int(dec[members[i]]["n_chars"])]] for i in slots if 1 <= int(dec[members[i]]["n_chars"]) <= 32][:32]
            assert int(r["cost"]) <= int(r["seed_cost"]) <= min(R.score(lats, t, B, 64, 64, 8) for t in seeds)
            # 3. n_parts - n_del + n_ins = n_chars for every usable member
            for i in slots:
                assert int(mrec[i]["n_parts"]) - int(mrec[i]["n_del"]) + int(mrec[i]["n_ins"]) == int(r["n_chars"]) and int(mrec[i]["word"]) == int(members[i])
                assert (src[i, int(r["n_chars"]):] == 0xFF).all() and (src[i, :int(r["n_chars"])] != 0xFF).all()
            if int(r["converged"]):
                assert min(R.neighbour_scores(lats, s, B, 64, 64, 8))[0] >= int(r["cost"])
            # 4. rounds = 0: the winning seed's lattice decoder string, byte for byte
            if rounds == 0:
                w = int(r["seed_member"])
                assert (ch[g] == np.where(np.arange(32) < int(dec[w]["n_chars"]), dchars[w, :32], 0xFF)).all() and int(r["n_edits"]) == 0 == int(r["converged"])
                assert int(r["cost"]) == int(r["seed_cost"])
        assert mrec["first_part"].tolist() == np.concatenate([[0], np.cumsum(mrec["n_parts"])[:-1]]).tolist() and len(parts) == int(mrec["n_parts"].sum())


def test_without_cuts_it_is_the_track_decode_on_the_runs(S):
    """5. no member has a cut: record, labels and member costs are str_er_decode_tracks' on the runs' rows, the parts are the runs."""
    rng = np.random.default_rng(71)
    B = rng.integers(0, 90, (66, 66)).astype(np.uint8)
    tracks = [TD.make_track(rng, [int(a) for a in rng.integers(0, 65, int(rng.integers(3, 9)))], int(rng.integers(1, 7))) for _ in range(6)]
    tracks.append([np.zeros((0, 65), np.uint8), rng.integers(0, 256, (33, 65)).astype(np.uint8), rng.integers(0, 256, (32, 65)).astype(np.uint8)])
    costs, first, n_of, tf, tc, members = TD.pack(tracks)
    sp = np.zeros(len(costs), S.RUN_SPLIT_DTYPE)
    sp["cut"] = -1
    none = np.zeros((0, 65), np.uint8)
    for di, dd, ins, dele, rounds, split in ((0, 0, 64, 64, 8, 8), (64, 64, 30, 200, 2, 255), (0, 0, 255, 1, 0, 0)):
        out, ch, mrec, src, parts = S.lattice_decode_tracks_host(sp, costs, none, first, n_of, tf, tc, members, B, di, dd, ins, dele, rounds, split)
        plain, pch, pmc = S.decode_tracks_host(costs, first, n_of, tf, tc, members, B, di, dd, ins, dele, rounds)
        assert out.tobytes() == plain.tobytes() and ch.tobytes() == pch.tobytes() and mrec["cost"].tolist() == pmc.tolist()
        for i, m in enumerate(mrec):
            if int(m["cost"]) >= 0:
                w = int(members[i])
                assert parts_list(parts[int(m["first_part"]):int(m["first_part"]) + int(m["n_parts"])]) == [[int(first[w]) + t, -1] for t in range(int(n_of[w]))]


def test_a_track_of_one_member_and_the_final_string_as_a_lexicon(S, case):
    B, packed, _ = case
    sp, rr, pr, first, n_of, tf, tc, members = packed
    n_words = len(first)
    # 6. a track of one usable member, the decoder's INS = DEL = 0: seed_cost <= the word's lattice decoder cost
    one = S.lattice_decode_tracks_host(sp, rr, pr, first, n_of, np.arange(n_words), np.ones(n_words, np.int32), np.arange(n_words), B, 0, 0, 64, 64, 0, 8)
    dec = S.lattice_decode_words_host(sp, rr, pr, first, n_of, B, 0, 0, 8)[0]
    seen = 0
    for w in range(n_words):
        if 1 <= int(dec[w]["n_chars"]) <= 32:
            assert int(one[0][w]["seed_cost"]) <= int(dec[w]["cost"]) and int(one[0][w]["seed_member"]) == w and int(one[0][w]["n_used"]) == 1
            seen += 1
    assert seen >= 10
    # 7. the final string as a one-entry lexicon without fold: every member's cost, parts, n_del, n_ins and sources are
    # str_er_lattice_match_words' on that word, wherever the band admits l
    out, ch, mrec, src, parts = S.lattice_decode_tracks_host(*packed, B, 0, 0, 64, 64, ROUNDS, 8)
    held = 0
    for g, r in enumerate(out):
        word = "".join(WM.ALPHABET[int(a)] for a in ch[g, :int(r["n_chars"])])
        lrec, lsrc, lparts = S.lattice_match_words_host(sp, rr, pr, first, n_of, [word], False, 64, 64, 31, 8)
        for i in range(int(tf[g]), int(tf[g]) + int(tc[g])):
            w, m = int(members[i]), mrec[i]
            if int(lrec[w]["entry"]) == 0:
                assert (int(m["cost"]), int(m["n_parts"]), int(m["n_del"]), int(m["n_ins"])) == tuple(int(lrec[w][k]) for k in ("cost", "n_parts", "n_del", "n_ins"))
                assert (src[i] == lsrc[w]).all()
                assert parts[int(m["first_part"]):int(m["first_part"]) + int(m["n_parts"])].tobytes() == \
                       lparts[int(lrec[w]["first_part"]):int(lrec[w]["first_part"]) + int(lrec[w]["n_parts"])].tobytes()
                held += 1
    assert held == len(members)


def test_slots_of_no_track_unusable_members_and_bad_arguments(S):
    rng = np.random.default_rng(72)
    B = rng.integers(0, 90, (66, 66)).astype(np.uint8)
    packed = R.pack([R.make_track(rng, [3, 9, 40, 22], 3), R.make_track(rng, [7, 7, 1], 2)])
    sp, rr, pr, first, n_of, tf, tc, members = packed
    mem = np.array([0, 1, 4, 2, 3, 3, 0], np.int32)          # slots 2 and 6: of no track; word 3 twice
    tf2, tc2 = np.array([0, 3], np.int32), np.array([2, 3], np.int32)
    got = S.lattice_decode_tracks_host(sp, rr, pr, first, n_of, tf2, tc2, mem, B, 0, 0, 64, 64, 4, 8)
    equal(got, R.decode_tracks(sp, rr, pr, first, n_of, tf2, tc2, mem, B, 0, 0, 64, 64, 4, 8))
    assert [int(got[2][i]["word"]) for i in (2, 6)] == [-1, -1] and int(got[2][4]["cost"]) == int(got[2][5]["cost"]) >= 0
    # a track of none, and no tracks at all
    got = S.lattice_decode_tracks_host(sp, rr, pr, first, n_of, [0, 0], [0, 2], mem[:2], B)
    assert R.as_tuples(got[0])[0] == TD.NOT_DECODED and int(got[0][1]["cost"]) >= 0
    got = S.lattice_decode_tracks_host(sp, rr, pr, first, n_of, [], [], [], B)
    assert got[0].shape == (0,) and got[1].shape == (0, 32) and got[2].shape == (0,) and got[4].shape == (0,)
    for bad in (dict(ins=0), dict(dele=256), dict(rounds=65), dict(split_cost=256), dict(dec_ins=-1)):
        with pytest.raises(S.StrErError):
            S.lattice_decode_tracks_host(*packed, B, **bad)
    with pytest.raises(S.StrErError):
        S.lattice_decode_tracks_host(sp, rr, pr, first, n_of, [0], [1025], np.zeros(1025, np.int32), B)
