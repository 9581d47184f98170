"""The inputs of test_read_chain_reuse.py: seeded inputs for every single-stage entry point of the reading chain in two sizes, two
lexicons and a bigram table, from the makers the entry points' own modules have.  No GPU.

small   the records a kernel writes as constants -- a word of no runs, a word of 33 runs (unusable), a word of 9 runs whose lattice has
        36 nodes (usable by its rows, unusable by its lattice), a track of no members, a track of unusable members only, GAP member slots
        of no track behind every track, a track whose members' decoder strings are no seeds (members without rows: with the decoder's
        INS / DEL off a string has one label a row), a footprint without a bit -- with an ordinary word, track and footprint beside them.
large   at least 16 times the words, member slots, part slots and footprints, and a live record in every slot: every word usable with a
        cut run, every member slot in a track, every footprint with runs and most with a cut run.  The track decode's large case holds tracks of exactly 252
        and 253 rows of usable members (the two sides of TD_RES = 16384 bytes of 65-byte rows) and a track of nine members of 32 rows
        (288 rows: not resident, and the polish runs on members of 32 rows).

The lattice track decode has the tracks of the matchers and more (`ltd`): in the small case a track of the word without runs alone, in the
large one 32 further tracks.  The line
decoder and its margins have lines over the words' run rows, repeated to the length they need (lines_case): small is a line without rows,
a line of 1025 rows (one more than the decoder takes), an ordinary line, and GAP rows of no line behind each of the latter two; large is
17 lines of 1024 rows and 64 short ones, every row in a line."""
import numpy as np

import lexicon_layout as LL
import test_run_read as RRD
import test_run_split as RSP
from test_lattice_decode_abi import cheapen, make_rows
from test_lattice_track import _spans, _words
from test_track_decode import confident, pack

W, H = 320, 128                         # the frame of the hand-made footprints of test_run_read.py / test_run_split.py
GAP = 2                                 # member slots of no track behind every track of a small case
SIZES = ("small", "large")
TD_RES_ROWS = 16384 // 65               # rows of usable members that stay resident in k_track_decode
LINE_MAX = 1024                         # rows of the longest line the line decoder takes


def feet_case(size):
    """{items: [(x, y, bits)], slopes}: footprints in the W x H frame."""
    rng = np.random.default_rng(9001)
    if size == "small":
        split, read = {c[0]: c for c in RSP._cases(rng)}, {c[0]: c for c in RRD._cases(rng)}
        cases = [split["empty"], split["straddle_63"], read["one_pixel"], split["width_2"], split["slope"]]
    else:
        cases = RSP._many(rng, 64) + RRD._many(rng, 16)          # necked runs (they are cut), and runs with a gap between them
    return {"items": [(x, y, b) for _, x, y, b, _ in cases], "slopes": [s for *_, s in cases]}


def _track_table(n_words, tracks, gap):
    """(track_first, track_count, members) of the member lists, `gap` slots of no track (they hold word 0) behind every track: the layout
    of test_track_decode.pack."""
    _, _, _, tf, tc, mem = pack([np.zeros((0, 65), np.uint8)] * n_words, tracks, gap)
    return tf, tc, mem


def rows_case(S, size):
    """The words and tracks of the matchers, the decoders and the segmentation: {sp, rc, pc (split records, run rows, piece rows), first,
    n_of, tf, tc, mem, tracks (the member lists), shapes (the cut counts of every word's runs)}."""
    if size == "small":
        rng = np.random.default_rng(9101)
        # 0: no runs; 1: 33 runs; 2: 9 runs of 3 cuts (36 nodes); 3 and 4: ordinary
        shapes = [[], [0] * 33, [3] * 9, [1, 0, 2, 0], [0, 1, 0]]
        tracks, gap = [[], [1, 1], [3, 4], [2, 2]], GAP          # none, unusable members only, ordinary, usable by the rows alone
    else:
        rng = np.random.default_rng(9102)
        shapes = []
        for _ in range(192):
            cuts = rng.integers(0, 4, int(rng.integers(1, 9)))
            cuts[rng.integers(0, len(cuts))] = rng.integers(1, 4)          # (a cut run in every word)
            shapes.append([int(k) for k in cuts])
        tracks, gap = [[int(w) for w in rng.integers(0, len(shapes), int(k))] for k in rng.integers(1, 12, 56)], 0
    first, n_of = _spans([len(c) for c in shapes])
    sp, rc, pc = make_rows(S, rng, np.array([k for c in shapes for k in c], np.int64))
    rc, pc = cheapen(rng, rc), cheapen(rng, pc)
    tf, tc, mem = _track_table(len(shapes), tracks, gap)
    # the lattice track decode: in the small case a track of the word without runs alone as well (no seeds); in the large one 32 more
    # tracks, 16 times the small case's
    more = np.random.default_rng(9103)
    ltd_tracks = tracks + ([[0, 0]] if size == "small" else [[int(w) for w in more.integers(0, len(shapes), int(k))] for k in more.integers(1, 12, 32)])
    return {"sp": sp, "rc": rc, "pc": pc, "first": first, "n_of": n_of, "tf": tf, "tc": tc, "mem": mem, "tracks": tracks, "shapes": shapes,
            "ltd": _track_table(len(shapes), ltd_tracks, gap), "ltd_tracks": ltd_tracks}


def lines_case(rows, size):
    """The lines of the line decoder and its margins over the run rows of rows_case, repeated: {costs, gaps, first, n_of, no_line (the
    rows of no line)}.  Both moves are on at every gap inside a line; the first row of a line and a row of no line have (0, 255), as
    str_er_line_gap_costs gives them."""
    if size == "small":
        rng = np.random.default_rng(9501)
        n_of, gap = [0, LINE_MAX + 1, 3], [0, GAP, GAP]          # no rows; one row too many; ordinary
    else:
        rng = np.random.default_rng(9502)
        n_of = [LINE_MAX] * 17 + [int(k) for k in rng.integers(1, 13, 64)]
        gap = [0] * len(n_of)
    first = np.concatenate([[0], np.cumsum(np.add(n_of, gap))[:-1]]).astype(np.int32)
    total = int(first[-1]) + n_of[-1] + gap[-1]
    costs = np.ascontiguousarray(np.resize(rows["rc"], (total, 65)))
    gaps = rng.integers(0, 48, (total, 2)).astype(np.uint8)
    in_line = np.zeros(total, bool)
    for a, k in zip(first, n_of):
        in_line[a:a + k] = True
    gaps[~in_line] = (0, 255)
    gaps[first[np.array(n_of) > 0]] = (0, 255)
    return {"costs": costs, "gaps": gaps, "first": first, "n_of": np.array(n_of, np.int32), "no_line": np.flatnonzero(~in_line)}


def _variant(rng, truth, n_sub):
    """Rows that read `truth` with n_sub labels replaced."""
    labels = np.array(truth)
    at = rng.choice(len(labels), n_sub, replace=False)
    labels[at] = (labels[at] + rng.integers(1, 65, n_sub)) % 65
    return confident([int(a) for a in labels], rng, lo=60)


def track_decode_case(size):
    """The words (their own rows) and tracks of the track decode: {packed: (costs, first, n_of, tf, tc, mem), tracks, rows_of (rows per
    word)}."""
    if size == "small":
        rng = np.random.default_rng(9301)
        # 0: ordinary; 1: 33 rows; 2: 40 rows; 3: no rows (its decoder string is no seed); 4: ordinary
        words = [confident([1, 2, 3], rng), rng.integers(0, 256, (33, 65)).astype(np.uint8), rng.integers(0, 256, (40, 65)).astype(np.uint8),
                 np.zeros((0, 65), np.uint8), confident([1, 9, 3, 4], rng)]
        tracks, gap = [[], [1, 2], [3, 3], [0, 4, 0]], GAP       # none, unusable members only, no seeds, ordinary
    else:
        rng = np.random.default_rng(9302)
        truth = [int(a) for a in rng.integers(0, 65, 32)]
        words = [_variant(rng, truth, 3) for _ in range(9)]                    # 0 .. 8: 32 rows each
        words += [_variant(rng, truth[:28], 2), _variant(rng, truth[:29], 2)]   # 9: 28 rows; 10: 29 rows
        short = [7, 30, 52]
        words += [confident(short[:int(rng.integers(1, 4))], rng, lo=40) for _ in range(80)]          # 11 .. 90: 1 .. 3 rows
        tracks = [list(range(9)), list(range(7)) + [9], list(range(7)) + [10]]                        # 288 rows, 252 rows, 253 rows
        tracks += [[int(w) for w in rng.integers(11, 91, int(k))] for k in rng.integers(2, 12, 40)]
        gap = 0
    return {"packed": pack(words, tracks, gap), "tracks": tracks, "rows_of": [len(C) for C in words]}


def lexicons():
    """(one, big): one chunk on both sides; about 5000 entries of mixed lengths that span several track-side and two word-side chunks."""
    rng = np.random.default_rng(9201)
    one = _words(rng, 180, 1, 12, labels=12)
    big = _words(rng, 5000, 3, 8) + _words(rng, 40, 1, 2) + _words(rng, 40, 9, 32, labels=8)
    return one, big


def chunks(words):
    """(track-side chunks, word-side chunks) of a lexicon, by the host mirror of its layout."""
    lay = LL.place(words)
    return lay.tm_chunks, lay.wm_chunks


def bigram():
    return np.random.default_rng(9401).integers(0, 60, (66, 66)).astype(np.uint8)
