"""The lexicons and the planted scenarios of test_lexicon_layout.py (no GPU: the layout mirror and the numpy references alone) and
test_big_lexicon.py (the kernels).  Every size comes from lexicon_layout's constants: T = TM_CHUNK_GROUPS groups a track-side chunk,
W = WM_CHUNK_GROUPS groups a word-side chunk, G = WM_GROUP entries a group, V = WAVE chunks a pass of a lane-strided merge.

A lexicon is background strings (lower case k .. z, which no scenario makes cheap) with a few planted entries; a scenario is a set of
words whose rows read the planted entries at costs worked out by hand (`want`), with everything else at 255:
  an uncut run costs its character h, a dropped run DEL, a character without a run INS; a run cut into atoms is read atom by atom for
  SPLIT per atom after its first -- the cut runs cover only characters that every planted entry of the scenario has, so a lattice
  word costs what its flattened twin costs plus SPLIT per extra atom; a noise run (all 255) is dropped by every entry.
The references are computed once per process and shared by both modules."""
import functools

import numpy as np

import lattice_decode_ref as LD
import lattice_match_ref as LM
import lattice_track_ref as LT
import lexicon_layout as LL
import track_read_ref as TR
import word_match_ref as WM

T, W, G, V = LL.TM_CHUNK_GROUPS, LL.WM_CHUNK_GROUPS, LL.WM_GROUP, LL.WAVE
SPLIT_DTYPE = np.dtype([("n_cuts", "<i4"), ("cut", "<i4", (3,)), ("thr", "<u4"), ("first_piece", "<i4"), ("n_pieces", "<i4"), ("n_parts", "<i4")])      # str_er_run_split
DEAR = 255


# ---- the lexicons -----------------------------------------------------------------------------------------------------------------
def _spec_full():
    """V * T groups: exactly V track chunks, the last full single pass.  Chunk 0 is the length 3, the last chunk the length 7."""
    groups = {3: T, 4: 20 * T, 5: 25 * T, 7: T}
    groups[6] = V * T - sum(groups.values())
    counts = {l: g * G for l, g in groups.items()}
    counts[4] -= 13; counts[5] -= 40
    lay = LL.Layout(counts)
    planted = {"LO": ("ABC", 3, 5, 9), "HI": ("ABCDEFG", 7, lay.n_groups - 1, G - 1)}
    return counts, planted, (), False


def _spec_pass2():
    """V * T + 1 groups: V + 1 track chunks, the last of one group (the length 7, 41 entries and 23 padding slots).  Folds case."""
    groups = {3: T, 4: 20 * T, 5: 25 * T, 7: 1}
    groups[6] = V * T + 1 - sum(groups.values())
    counts = {l: g * G for l, g in groups.items()}
    counts[4] -= 13; counts[5] -= 40; counts[7] -= 23
    lay = LL.Layout(counts)
    last = lay.n_groups - 1
    planted = {"P12.LO": ("abc", 3, 7, 3), "P12.HI": ("ABCDEFG", 7, last, 5),
               "P4.BEST": ("1234567", 7, last, lay.last_real()[1] % G), "P4.SECOND": ("123456", 6, 50 * T + 2, 17)}
    return counts, planted, (), True


def _spec_pass3():
    """2 * V * T + 1 groups: 2 V + 1 track chunks, a third pass for lane 0.  Chunk 0 holds the lengths 2, 3 and 4, chunk V lies in the
    length 5 and the last group has the length 6.  The index order is the lengths 6, 4, 5, 2, 3: the longest entries have the lowest
    indices."""
    groups = {2: 1, 3: 2, 4: 40 * T - 3, 5: 50 * T}
    groups[6] = 2 * V * T + 1 - sum(groups.values())
    counts = {l: g * G for l, g in groups.items()}
    counts[2] -= 14; counts[3] -= 7; counts[4] -= 5; counts[6] -= 30
    lay = LL.Layout(counts)
    planted = {"P3.BEST": ("ABCDE", 5, (V + 6) * T + 1, 10), "P3.SECOND": ("ABCDG", 5, (V + 6) * T + 9, 60), "P3.THIRD": ("ABCD", 4, 6 * T + 4, 33),
               "P5.SHORT": ("EEEE", 4, 30 * T + 2, 7), "P5.LONG": ("EEEEEE", 6, (30 + V) * T + 11, 50),
               "P6.A": ("HHHH", 4, 5, 1), "P6.B": ("JHHHH", 5, V * T + 3, 2), "P6.C": ("HHHHHH", 6, lay.n_groups - 1, 20)}
    return counts, planted, (6, 4, 5), False


def _spec_word2():
    """V * W + 1 groups: V + 1 word-side chunks for a word whose band starts at the length 1.  Chunk 0 holds the lengths 2, 3 and 4,
    the last group has the length 6 (44 entries).  Index order 6, 4, 5, 2, 3."""
    groups = {2: 1, 3: 2, 4: 20 * W - 3, 5: 25 * W}
    groups[6] = V * W + 1 - sum(groups.values())
    counts = {l: g * G for l, g in groups.items()}
    counts[2] -= 14; counts[3] -= 7; counts[5] -= 9; counts[6] -= 20
    lay = LL.Layout(counts)
    last = lay.n_groups - 1
    planted = {"P12.LO": ("ABCD", 4, 9, 4), "P12.HI": ("ABCDEF", 6, last, 3),
               "P3.BEST": ("KLMNOP", 6, last, 8), "P3.SECOND": ("KLMNOQ", 6, last, 30), "P3.THIRD": ("KLMN", 4, 20, 0),
               "P4.BEST": ("123456", 6, last, lay.last_real()[1] % G), "P4.SECOND": ("12345", 5, 30 * W + 5, 9),
               "P5.SHORT": ("EEEE", 4, 40, 11), "P5.LONG": ("EEEEEE", 6, last, 12)}
    return counts, planted, (6, 4, 5), False


def max_triple(lay, lens=(5, 6, 7)):
    """Groups (a, b, c) of the three lengths that a word whose band starts at lens[0] meets in the relative word chunks r, r + V and
    r + 2 V, and that the track side meets in three passes of one lane."""
    base = int(lay.len_first[lens[0]])
    for a in range(*lay.groups_of(lens[0])):
        r, lane = (a - base) // W, lay.tm_chunk(a) % V
        found = [a]
        for k, l in ((1, lens[1]), (2, lens[2])):
            lo, hi = lay.groups_of(l)
            cand = [g for g in range(max(lo, base + (r + k * V) * W), min(hi, base + (r + k * V + 1) * W)) if lay.tm_chunk(g) % V == lane]
            if cand:
                found.append(cand[0])
        if len(found) == 3 and len({lay.tm_chunk(g) // V for g in found}) == 3:
            return tuple(found)
    raise AssertionError("no such groups: the lexicon is too small for these constants")


def _spec_max():
    """MAX_ENTRIES entries, every length a multiple of G: the lengths 2 and 3 fill the first groups (their number is no multiple of W),
    the lengths 5, 6 and 7 the rest, more than 2 V word-side chunks of it; there is no length 4, so a band that starts at 4 starts at
    the first group of 5.  Index order 7, 5, 6, 2, 3."""
    total = LL.MAX_ENTRIES // G
    early = total // 2 - W - 27
    groups = {2: 101, 3: early - 101}
    late = total - early
    groups[5] = groups[6] = late // 3 + 39
    groups[7] = late - 2 * groups[5]
    counts = {l: g * G for l, g in groups.items()}
    lay = LL.Layout(counts)
    a, b, c = max_triple(lay)
    base, k = early, 50
    planted = {"P6.A": ("HHHHH", 5, a, 21), "P6.B": ("JHHHHH", 6, b, 40), "P6.C": ("HHHHHHH", 7, c, 2),
               "ENDS.BEST": ("ABCDEFG", 7, total - 1, G - 1), "ENDS.SECOND": ("ABCDE", 5, base, 0),
               "P7.BEST": ("STUVWX", 6, base + k * W, 0), "P7.SECOND": ("STUVWY", 6, base + k * W - 1, G - 1)}
    return counts, planted, (7, 5, 6), False


SPECS = {"full": _spec_full, "pass2": _spec_pass2, "pass3": _spec_pass3, "word2": _spec_word2, "max": _spec_max}


class Lex:
    def __init__(self, name):
        counts, planted, order, self.fold = SPECS[name]()
        self.name, self.plan = name, LL.Layout(counts)
        slots = {key: (text, l, self.plan.slot_at(l, g, lane)) for key, (text, l, g, lane) in planted.items()}
        self.words, index_of = LL.build(counts, list(slots.values()), order, seed=len(name))
        self.index = {key: index_of[l, s] for key, (text, l, s) in slots.items()}
        self.text = {key: text for key, (text, l, s) in slots.items()}
        self.lay = LL.place(self.words)

    @functools.cached_property
    def ref(self):
        return WM.Lexicon(self.words, self.fold)


@functools.lru_cache(maxsize=None)
def lexicon(name) -> Lex:
    return Lex(name)


# ---- the words --------------------------------------------------------------------------------------------------------------------
def reads(text, h=2, alt=None):
    """The atoms of a word that reads `text` at h a character; alt: {position: {character: cost}} beside it."""
    atoms = [{ch: h} for ch in text]
    for i, more in (alt or {}).items():
        atoms[i].update(more)
    return atoms


def word(atoms, cut=None, noise=0):
    """A word as a list of runs (a run: a list of atoms): the atoms grouped into runs of the sizes `cut` (default: every atom a run),
    then `noise` runs that read nothing."""
    sizes = list(cut) if cut else [1] * len(atoms)
    assert sum(sizes) == len(atoms) and all(1 <= s <= 4 for s in sizes)
    runs, at = [], 0
    for s in sizes:
        runs.append(atoms[at:at + s])
        at += s
    return runs + [[{}] for _ in range(noise)]


def flatten(w):
    return [[a] for run in w for a in run]


def _row(atom, free0):
    r = np.full(65, DEAR, np.uint8)
    for ch, c in atom.items():
        r[WM.LABEL_OF[ch]] = c
    if free0:
        r[0] = 0
    return r


def make_rows(words, free0=False):
    """(splits, run rows, piece rows, first_run, n_runs_of_word) of the words.  A run of several atoms has a dear row of its own and
    dear rows for its pieces of several atoms; the piece (i, i + 1) reads atom i.  free0: the label 0 is free on every row."""
    n_cuts = [len(run) - 1 for w in words for run in w]
    sp = np.zeros(len(n_cuts), SPLIT_DTYPE)
    sp["cut"] = -1
    sp["n_cuts"] = n_cuts
    sp["n_pieces"] = [LD.n_pieces(k) for k in n_cuts]
    sp["first_piece"] = np.concatenate([[0], np.cumsum(sp["n_pieces"])[:-1]]) if len(n_cuts) else []
    rc = np.full((len(n_cuts), 65), DEAR, np.uint8)
    pc = np.full((int(sp["n_pieces"].sum()), 65), DEAR, np.uint8)
    if free0:
        rc[:, 0], pc[:, 0] = 0, 0
    r = 0
    for w in words:
        for run in w:
            A = len(run)
            for i, atom in enumerate(run):
                k = LD.piece_of(A, i, i + 1)
                (rc[r:r + 1] if k < 0 else pc[int(sp["first_piece"][r]) + k:int(sp["first_piece"][r]) + k + 1])[0] = _row(atom, free0)
            r += 1
    n_of = np.array([len(w) for w in words], np.int32)
    first = np.concatenate([[0], np.cumsum(n_of)[:-1]]).astype(np.int32)
    return sp, rc, pc, first, n_of


def flat(lists):
    tc = np.array([len(t) for t in lists], np.int32)
    tf = (np.concatenate([[0], np.cumsum(tc)[:-1]]) if len(lists) else np.zeros(0)).astype(np.int32)
    return tf, tc, np.array([w for t in lists for w in t], np.int32)


# ---- the scenarios ----------------------------------------------------------------------------------------------------------------
class Case:
    """side "track": one track of the members `words` (`track`: their order); want = (best, cost, second, cost) of the track on the
    flattened members, want_lattice on the members as they are.  side "word": want per word of `words`, want_plain for the first word
    flattened.  setting = (INS, DEL, band, SPLIT); the fold is the lexicon's."""

    def __init__(self, name, lex, side, setting, words, want, want_lattice=None, track=None, free0=False, about=""):
        self.name, self.lex, self.side, self.setting, self.words, self.free0, self.about = name, lex, side, setting, words, free0, about
        self.want, self.want_lattice = want, want_lattice
        self.track = list(range(len(words))) if track is None else track

    def __repr__(self):
        return self.name

    def rows(self, lattice):
        """The call's tables: the lattice families get the words as they are, the others the flattened ones (side word: the first)."""
        ws = self.words if lattice else [flatten(w) for w in (self.words if self.side == "track" else self.words[:1])]
        return make_rows(ws, self.free0)

    def wanted(self, lattice):
        """What the reference must return: side track -> (entry, cost, second_entry, second_cost); side word -> a list of them."""
        L = lexicon(self.lex)
        key = lambda w: (L.index[w[0]], w[1], L.index[w[2]], w[3])
        if self.side == "track":
            return key(self.want_lattice if lattice else self.want)
        return [key(w) for w in (self.want_lattice if lattice else self.want[:1])]


H5, SPLIT = reads("HHHHH", 0), 8
J5 = reads("HHHHH", 0, {0: {"J": 64}})
J6 = reads("HHHHHH", 0, {0: {"J": 64}})
NOISE33 = word([], noise=33)
ABCDE, E5 = reads("ABCDE"), reads("EEEEE", 0)
P3 = reads("ABCDE", 2, {4: {"G": 9}})
D7 = reads("1234567", 1)

TRACK_CASES = [
    # 64 chunks, every lane with a key: best in the last chunk, second in chunk 0.  HI = 5 h + 2 INS = 90, LO = 3 h + 2 DEL = 186
    Case("full", "full", "track", (40, 90, 31, SPLIT), [word(ABCDE, (2, 1, 1, 1)), word(ABCDE)], ("HI", 180, "LO", 372), ("HI", 188, "LO", 380)),
    # P1: LO = 3 h + 2 DEL = 86 a member, HI = 5 h + 2 INS = 190; the member of 12 runs drops 7 (280) beside; 33 runs: unusable
    Case("P1", "pass2", "track", (90, 40, 31, SPLIT), [word(ABCDE, (2, 1, 1, 1)), word(ABCDE, noise=7), NOISE33],
         ("P12.LO", 86 + 86 + 280, "P12.HI", 190 + 190 + 280), ("P12.LO", 94 + 86 + 280, "P12.HI", 198 + 190 + 280)),
    # P2: HI = 5 h + 2 INS = 90, LO = 3 h + 2 DEL = 186; the member of 20 runs drops 15 (1350) beside
    Case("P2", "pass2", "track", (40, 90, 31, SPLIT), [word(ABCDE, (2, 1, 1, 1)), word(ABCDE, noise=15)],
         ("P12.HI", 90 + 90 + 1350, "P12.LO", 186 + 186 + 1350), ("P12.HI", 98 + 90 + 1350, "P12.LO", 194 + 186 + 1350), track=[1, 0]),
    # P4 / P8: the label 0 is free; BEST = 7 h = 7 a member in the last real lane of the last group, SECOND = 6 h + DEL = 70
    Case("P4_P8", "pass2", "track", (64, 64, 31, SPLIT), [word(D7, (2, 1, 1, 1, 1, 1)), word(D7)], ("P4.BEST", 14, "P4.SECOND", 140),
         ("P4.BEST", 22, "P4.SECOND", 148), free0=True),
    # P3: BEST = 5 h = 10, SECOND = 4 h + 9 = 17, THIRD = 4 h + DEL = 72; the run of four atoms pays 3 SPLIT
    Case("P3", "pass3", "track", (64, 64, 31, SPLIT), [word(P3, (4, 1)), word(P3), word(P3)], ("P3.BEST", 30, "P3.SECOND", 51), ("P3.BEST", 54, "P3.SECOND", 75)),
    # P5: only E is free, INS = DEL: one edit each, 64 a member; the member of 9 runs drops 4 (256) beside
    Case("P5", "pass3", "track", (64, 64, 31, SPLIT), [word(E5, (1, 2, 1, 1)), word(E5, noise=4)], ("P5.LONG", 64 + 64 + 256, "P5.SHORT", 64 + 64 + 256),
         ("P5.LONG", 72 + 64 + 256, "P5.SHORT", 72 + 64 + 256)),
    # P6: H is free and the first run reads J at 64 = INS = DEL: HHHH, JHHHH and HHHHHH cost 64 a member
    Case("P6", "pass3", "track", (64, 64, 31, SPLIT), [word(J5, (1, 2, 1, 1)), word(J5)], ("P6.C", 128, "P6.A", 128), ("P6.C", 136, "P6.A", 136)),
    # P6 at 2^20 entries, band 1: the lengths 5, 6 and 7 only
    Case("P6max", "max", "track", (64, 64, 1, SPLIT), [word(J6, (1, 2, 1, 1, 1)), word(J6), NOISE33], ("P6.C", 128, "P6.A", 128), ("P6.C", 136, "P6.A", 136)),
]

K6 = reads("KLMNOP", 2, {5: {"Q": 9}})
D6 = reads("123456", 1)
S6 = reads("STUVWX", 2, {5: {"Y": 9}})
ABCDEF = reads("ABCDEF")

WORD_CASES = [
    # (every case: the word uncut, then with its first two characters in one run of two atoms: + SPLIT)
    Case("P1", "word2", "word", (90, 40, 31, SPLIT), [word(ABCDE), word(ABCDE, (2, 1, 1, 1))], [("P12.LO", 48, "P12.HI", 100)] * 2,
         [("P12.LO", 48, "P12.HI", 100), ("P12.LO", 56, "P12.HI", 108)]),               # LO = 4 h + DEL, HI = 5 h + INS
    Case("P2", "word2", "word", (40, 90, 31, SPLIT), [word(ABCDE), word(ABCDE, (2, 1, 1, 1))], [("P12.HI", 50, "P12.LO", 98)] * 2,
         [("P12.HI", 50, "P12.LO", 98), ("P12.HI", 58, "P12.LO", 106)]),
    Case("P3", "word2", "word", (64, 64, 31, SPLIT), [word(K6), word(K6, (2, 1, 1, 1, 1))], [("P3.BEST", 12, "P3.SECOND", 19)] * 2,
         [("P3.BEST", 12, "P3.SECOND", 19), ("P3.BEST", 20, "P3.SECOND", 27)]),         # THIRD = 4 h + 2 DEL = 136
    Case("P4", "word2", "word", (64, 64, 31, SPLIT), [word(D6), word(D6, (2, 1, 1, 1, 1))], [("P4.BEST", 6, "P4.SECOND", 69)] * 2,
         [("P4.BEST", 6, "P4.SECOND", 69), ("P4.BEST", 14, "P4.SECOND", 77)], free0=True),
    Case("P5", "word2", "word", (64, 64, 31, SPLIT), [word(E5), word(E5, (1, 2, 1, 1))], [("P5.LONG", 64, "P5.SHORT", 64)] * 2,
         [("P5.LONG", 64, "P5.SHORT", 64), ("P5.LONG", 72, "P5.SHORT", 72)]),
    Case("P6max", "max", "word", (64, 64, 1, SPLIT), [word(J6), word(J6, (1, 2, 1, 1, 1))], [("P6.C", 64, "P6.A", 64)] * 2,
         [("P6.C", 64, "P6.A", 64), ("P6.C", 72, "P6.A", 72)]),
    Case("ENDSmax", "max", "word", (40, 90, 1, SPLIT), [word(ABCDEF), word(ABCDEF, (2, 1, 1, 1, 1))], [("ENDS.BEST", 52, "ENDS.SECOND", 100)] * 2,
         [("ENDS.BEST", 52, "ENDS.SECOND", 100), ("ENDS.BEST", 60, "ENDS.SECOND", 108)]),       # BEST = 6 h + INS, SECOND = 5 h + DEL
    Case("P7max", "max", "word", (64, 64, 1, SPLIT), [word(S6), word(S6, (2, 1, 1, 1, 1))], [("P7.BEST", 12, "P7.SECOND", 19)] * 2,
         [("P7.BEST", 12, "P7.SECOND", 19), ("P7.BEST", 20, "P7.SECOND", 27)]),
]
CASES = {(c.side, c.name): c for c in TRACK_CASES + WORD_CASES}


@functools.lru_cache(maxsize=None)
def reference(side, name, lattice):
    """The numpy reference's answer to a case: side track -> track_read_ref.match_tracks / lattice_track_ref.match_tracks, side word ->
    word_match_ref.match_words / lattice_match_ref.match_words."""
    c = CASES[side, name]
    L = lexicon(c.lex)
    ins, dele, band, split = c.setting
    sp, rc, pc, first, n_of = c.rows(lattice)
    if side == "track":
        tf, tc, mem = flat([c.track])
        if lattice:
            return LT.match_tracks(sp, rc, pc, first, n_of, tf, tc, mem, L.ref, ins, dele, band, split)
        return TR.match_tracks(rc, first, n_of, tf, tc, mem, L.ref, ins, dele, band)
    if lattice:
        return LM.match_words(sp, rc, pc, first, n_of, L.ref, ins, dele, band, split)
    return WM.match_words(rc, first, n_of, L.ref, ins, dele, band)
