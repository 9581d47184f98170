"""The numpy reference of the word tracks and the track match (track_read_ref.py) against hand-made cases whose answers are worked
out by hand, and its match against a brute-force statement of the contract.  CPU only; the library's host entry points are held
against the same cases in test_track_read_abi.py."""
import numpy as np

import track_read_ref as TR
import word_match_ref as WM

# every case: the lines (frame, text track, pixels), the level-0 sizes of the frames, the words (line, x, y, w, h, pixels), num / den
# and by hand: the reading flags, the links, the track of every word, the tracks (first_frame, last_frame, first, count, rep,
# text_track) and the member array
CASES = {
    # three duplicate lines of one frame (two tie on pixels: the smaller index reads), a box that meets two boxes of the next frame,
    # and the closure that puts those two words of one frame into one track
    "ties_duplicates_closure": dict(
        lines=[(0, 0, 50), (0, 0, 80), (0, 0, 80), (1, 0, 10)], wh=[(100, 50), (100, 50)],
        words=[(1, 0, 0, 20, 10, 150), (2, 0, 0, 20, 10, 150), (3, 0, 0, 10, 10, 90), (3, 10, 0, 10, 10, 95), (0, 0, 0, 20, 10, 150)], num=1, den=2,
        reading=[0, 1, 0, 1], links=[(0, 2, 100, 1), (0, 3, 100, 1)], track_of=[0, -1, 0, 0, -1], tracks=[(0, 1, 0, 3, 0, 0)], members=[0, 2, 3]),
    # a change of size (frame 2 -> 3) and a track with lines in frames 0 and 2 only: no links; lines out of frame order, so that the
    # order of the tracks (first frame, then smallest member) is not the order of the words
    "sizes_gaps_order": dict(
        lines=[(1, 0, 10), (0, 0, 10), (2, 0, 10), (3, 0, 10), (0, 1, 10), (2, 1, 10)], wh=[(100, 50), (100, 50), (100, 50), (90, 50)],
        words=[(0, 0, 0, 10, 10, 5), (1, 0, 0, 10, 10, 5), (2, 0, 0, 10, 10, 7), (3, 0, 0, 10, 10, 9), (4, 50, 0, 10, 10, 5), (5, 50, 0, 10, 10, 5)],
        num=1, den=2, reading=[1, 1, 1, 1, 1, 1], links=[(0, 2, 100, 1), (1, 0, 100, 1)], track_of=[0, 0, 0, 3, 1, 2],
        tracks=[(0, 2, 0, 3, 2, 0), (0, 0, 3, 1, 4, 1), (2, 2, 4, 1, 5, 1), (3, 3, 5, 1, 3, 0)], members=[0, 1, 2, 4, 5, 3]),
    # an overlap of 10 of a union of 190: no link at 1 / 2 ...
    "overlap_no_link": dict(
        lines=[(0, 0, 10), (1, 0, 10)], wh=[(100, 50), (100, 50)], words=[(0, 0, 0, 10, 10, 5), (1, 9, 0, 10, 10, 5)], num=1, den=2,
        reading=[1, 1], links=[(0, 1, 10, 0)], track_of=[0, 1], tracks=[(0, 0, 0, 1, 0, 0), (1, 1, 1, 1, 1, 0)], members=[0, 1]),
    # ... and a link at 1 / 65535
    "overlap_link": dict(
        lines=[(0, 0, 10), (1, 0, 10)], wh=[(100, 50), (100, 50)], words=[(0, 0, 0, 10, 10, 5), (1, 9, 0, 10, 10, 5)], num=1, den=65535,
        reading=[1, 1], links=[(0, 1, 10, 1)], track_of=[0, 0], tracks=[(0, 1, 0, 2, 0, 0)], members=[0, 1]),
    # boxes that touch along an edge share no area; words of different tracks never meet
    "touching_and_tracks": dict(
        lines=[(0, 0, 10), (1, 0, 10), (1, 1, 10)], wh=[(64, 64), (64, 64)],
        words=[(0, 0, 0, 10, 10, 5), (1, 10, 0, 10, 10, 5), (2, 0, 0, 10, 10, 5)], num=1, den=2,
        reading=[1, 1, 1], links=[], track_of=[0, 1, 2], tracks=[(0, 0, 0, 1, 0, 0), (1, 1, 1, 1, 1, 0), (1, 1, 2, 1, 2, 1)], members=[0, 1, 2]),
    "nothing": dict(lines=[], wh=[], words=[], num=1, den=2, reading=[], links=[], track_of=[], tracks=[], members=[]),
}
TRACK_KEYS = ("first_frame", "last_frame", "first", "count", "rep", "text_track")


def case_tables(case):
    frames = np.array([l[0] for l in case["lines"]], np.uint32)
    tracks = np.array([l[1] for l in case["lines"]], np.int32)
    pixels = np.array([l[2] for l in case["lines"]], np.uint32)
    return pixels, frames, tracks, np.array(case["wh"], np.int32).reshape(-1, 2), TR.make_words(case["words"])


def test_hand_made_links_and_tracks():
    for name, case in CASES.items():
        pixels, frames, tracks, wh, words = case_tables(case)
        reading, links = TR.word_links(pixels, frames, tracks, wh, words, case["num"], case["den"])
        assert reading.tolist() == case["reading"], name
        assert links == case["links"], name
        track_of, wt, members = TR.word_tracks(frames, tracks, reading, words, links)
        assert track_of.tolist() == case["track_of"], name
        assert [tuple(t[k] for k in TRACK_KEYS) for t in wt] == case["tracks"], name
        assert members.tolist() == case["members"], name


def reads(costs_by_run):
    """Cost rows: per run a dict character -> cost, every other byte 255."""
    C = np.full((len(costs_by_run), 65), 255, np.uint8)
    for i, d in enumerate(costs_by_run):
        for ch, v in d.items():
            C[i, WM.LABEL_OF[ch]] = v
    return C


POOLED_ROWS = reads([{"A": 0, "D": 40}, {"B": 10, "C": 0}, {"A": 10, "D": 0}, {"B": 0, "C": 40}])
POOLED_LEXICON = ["AC", "DB", "AB"]


def test_pooled_example():
    """Two members that each take another entry alone; pooled, the track takes a third."""
    for fold in (True, False):
        lex = WM.Lexicon(POOLED_LEXICON, fold)
        alone = WM.match_words(POOLED_ROWS, [0, 2], [2, 2], lex)
        assert alone[0][:2] == (0, 0) and alone[1][:2] == (1, 0)
        sums = [sum(int(WM.entry_costs(POOLED_ROWS[f:f + 2].astype(np.int64), np.array([[WM.LABEL_OF[c] for c in w]]), 64, 64)[0]) for f in (0, 2))
                for w in POOLED_LEXICON]
        assert sums == [50, 50, 20]
        rec, own = TR.match_track(POOLED_ROWS, [0, 2], [2, 2], [0, 1], lex)
        assert rec == (2, 20, 0, 50, 0, 3, 2, 0) and own == [10, 10]
        one, own1 = TR.match_track(POOLED_ROWS, [0, 2], [2, 2], [1], lex)          # a track of one: the word's own match
        assert one[:6] == alone[1] and one[6:] == (1, 1) and own1 == [0]


def brute_match(costs, first_run, n_of, members, words, fold, ins, dele, band):
    """The contract once more, entry by entry."""
    usable = [w for w in members if n_of[w] <= 32]
    keys, tried = [], 0
    for e, text in enumerate(words):
        l = len(text)
        if not any(abs(l - n_of[w]) <= band for w in usable):
            continue
        tried += 1
        E = np.array([[WM.LABEL_OF[c] for c in text]])
        total = 0
        for w in usable:
            C = costs[first_run[w]:first_run[w] + n_of[w]]
            total += int(WM.entry_costs((WM.fold_rows(C) if fold else C).astype(np.int64), E, ins, dele)[0])
        keys.append((total, e))
    keys.sort()
    return keys, tried, len(usable)


def test_union_of_bands_with_a_gap():
    costs = np.zeros((22, 65), np.uint8)
    costs[:, WM.LABEL_OF["B"]] = 255          # A is free everywhere, B is dear: the entry of ten A would be the cheapest by far
    words = ["A" * 10] + ["B" * l for l in (1, 2, 3, 19, 20, 21, 4, 18, 22)]
    lex = WM.Lexicon(words, False)
    rec, own = TR.match_track(costs, [0, 2], [2, 20], [0, 1], lex, 64, 64, 1)
    assert rec[5] == 6 and rec[0] in (1, 2, 3, 4, 5, 6) and rec[0] != 0          # lengths 1 .. 3 and 19 .. 21 only
    keys, tried, used = brute_match(costs, [0, 2], [2, 20], [0, 1], words, False, 64, 64, 1)
    assert (rec[0], rec[1], rec[2], rec[3], rec[5], rec[6]) == (keys[0][1], keys[0][0], keys[1][1], keys[1][0], tried, used)
    assert sum(own) == rec[1]


def test_match_against_brute_force():
    rng = np.random.default_rng(11)
    letters = list(WM.ALPHABET)
    for trial in range(12):
        n_of = [int(x) for x in rng.choice([0, 1, 2, 3, 5, 8, 9, 33, 34], 6)]
        first = np.concatenate([[0], np.cumsum(n_of)[:-1]]).tolist()
        costs = rng.integers(0, 256, (sum(n_of), 65)).astype(np.uint8)
        words = ["".join(rng.choice(letters, int(rng.integers(1, 12)))) for _ in range(25)]
        fold, (ins, dele, band) = bool(trial % 2), [(64, 64, 2), (40, 90, 1), (64, 64, 0)][trial % 3]
        members = [int(x) for x in rng.integers(0, 6, int(rng.integers(1, 6)))]          # (a word may appear twice)
        rec, own = TR.match_track(costs, first, n_of, members, WM.Lexicon(words, fold), ins, dele, band)
        keys, tried, used = brute_match(costs, first, n_of, members, words, fold, ins, dele, band)
        best = keys[0] if keys else (-1, -1)
        second = keys[1] if len(keys) > 1 else (-1, -1)
        assert rec[:4] == (best[1], best[0], second[1], second[0]) and rec[5] == tried and rec[6] == used
        assert rec[4] == sum(int(costs[first[w] + i].min()) for w in members for i in range(n_of[w]))
        assert [c >= 0 for c in own] == [rec[0] >= 0 and n_of[w] <= 32 for w in members]
        if rec[0] >= 0:
            assert sum(c for c in own if c >= 0) == rec[1]
            i = min((i for i in range(len(members)) if own[i] >= 0), key=lambda i: (own[i], i))
            assert rec[7] == members[i]
        else:
            assert rec[7] == -1 and rec[1] == -1


def test_a_track_of_unusable_members_tries_nothing():
    costs = np.full((70, 65), 7, np.uint8)
    rec, own = TR.match_track(costs, [0, 33], [33, 37], [0, 1], WM.Lexicon(["A", "AB"], True))
    assert rec == (-1, -1, -1, -1, 70 * 7, 0, 0, -1) and own == [-1, -1]
