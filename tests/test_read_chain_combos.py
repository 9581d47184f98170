"""The reading chain behind the run scorer under every legal combination of its flags (STR_ER_WANT_WORD_MATCH, _WORD_DECODE, _RUN_SPLIT,
_LATTICE_DECODE, _TRACK_READ and a lexicon that folds or does not): every table of every call is byte for byte the same table of the
SMALLEST call that produces it, so which consumers run beside each other moves no byte of any of them.

    base tables                                                        the unflagged call
    run_splits, run_pieces, piece_reads, split_parts, word_splits      split alone
    word_matches                                                       match (with the call's split and fold)
    word_decodes, word_decode_chars, word_decode_src                   decode (with the call's split)
    the lattice tables                                                 split and lattice
    word links and word tracks                                         match and track
    track_matches, track_member_costs                                  match and track (with the call's split and fold)

The smallest calls themselves are held to the host references by the five *_pipeline.py modules.  run_costs is
word_match_ref.cost_rows of the call's own run_probs (of the decoder's where the call returns none), folded iff the matcher runs
with a lexicon that folds.  The pieces' probabilities are not part of a result: piece_costs is the unfolded rows of the call with split
alone (test_run_split_pipeline.py holds those to the probabilities), folded in the same case -- cost_rows(p, labels, True) is by
definition fold_rows(cost_rows(p, labels, False)).  A table whose flag is off raises ValueError.

Scene 1: the `proto` fixture of test_lattice_decode_pipeline.py (two frames, a prototype model with which words split, a bigram table,
INS / DEL 40 / 90, split 1 / 2 / 8), the 18 combinations without track.  Scene 2: the equal-size prefix of test_line_links.make_video
as one batch call, the shipped model and the lexicon of test_track_read_pipeline.py's scene, the 12 combinations with track."""
import numpy as np
import pytest

import word_match_ref as WM
from test_frame_lines import GROUPED
from test_lattice_decode_pipeline import INS, DEL, LATTICE_TABLES, proto  # noqa: F401  (the fixture)
from test_run_split_pipeline import NUM, DEN, SPLIT, scene as split_scene  # noqa: F401  (the fixture proto builds on)
from test_svm_exact import _shipped
from test_track_read_pipeline import NEW, TABLES as TRACK_TABLES, scene as track_scene  # noqa: F401  (the fixture)
from test_word_match_pipeline import TABLES, WANTS

pytestmark = pytest.mark.gpu
scene = split_scene          # (proto asks for the fixture by this name)
SPLIT_TABLES = ("run_splits", "run_pieces", "piece_reads", "split_parts", "word_splits")
DECODE_TABLES = ("word_decodes", "word_decode_chars", "word_decode_src")
LINKED = dict(want_line_links=True, **WANTS)


def key_of(match=False, decode=False, split=False, lattice=False, track=False, fold=None):
    return (match, decode, split, lattice, track, bool(fold) if match else None)


class Calls:
    """The detect call of a scene under a key, each made once."""

    def __init__(self, f, detect, lexicon):
        self.f, self.detect, self.lexicon, self.fold, self.made = f, detect, lexicon, None, {}

    def get(self, key):
        if key not in self.made:
            match, decode, split, lattice, track, fold = key
            if match and fold != self.fold:
                self.f.set_lexicon(self.lexicon, fold_case=fold)
                self.fold = fold
            self.made[key] = self.detect(want_word_match=match, want_word_decode=decode, want_run_split=split, want_lattice_decode=lattice, want_track_read=track)
        return self.made[key]


def check_call(calls, key, base_tables, labels):
    match, decode, split, lattice, track, fold = key
    res = calls.get(key)

    def same(ref_key, names):
        ref = calls.get(ref_key)
        for k in names:
            assert getattr(ref, k).tobytes() == getattr(res, k).tobytes(), (key, k)

    def absent(names):
        for k in names:
            with pytest.raises(ValueError):
                getattr(res, k)

    same(key_of(), base_tables)
    same(key_of(split=True), SPLIT_TABLES) if split else absent(SPLIT_TABLES + ("piece_costs",))
    same(key_of(match=True, split=split, fold=fold), ("word_matches",)) if match else absent(("word_matches",))
    same(key_of(decode=True, split=split), DECODE_TABLES) if decode else absent(DECODE_TABLES)
    same(key_of(split=True, lattice=True), LATTICE_TABLES) if lattice else absent(LATTICE_TABLES)
    if track:
        same(key_of(match=True, track=True, fold=True), NEW[:4])
        same(key_of(match=True, track=True, split=split, fold=fold), NEW[4:])
    else:
        absent(NEW)
    folded = bool(match and fold)
    if match or decode:
        same(key_of(decode=True) if decode else key_of(match=True, fold=fold), ("run_probs",))
        probs = res.run_probs
    else:
        absent(("run_probs",))
        probs = calls.get(key_of(decode=True)).run_probs
    if match or decode or split:
        assert res.run_costs.shape == (len(res.line_runs), 65) and (res.run_costs == WM.cost_rows(probs, labels, folded)).all(), key
    else:
        absent(("run_costs",))
    if split:
        rows = calls.get(key_of(split=True)).piece_costs
        assert res.piece_costs.shape == rows.shape and (res.piece_costs == (WM.fold_rows(rows) if folded else rows)).all(), key


@pytest.fixture(scope="module")
def calls1(proto):  # noqa: F811
    S, g, prm, model, uniform, crops, base, base_crops, table, read = proto
    calls = Calls(g, lambda **kw: g.text_detect(uniform, GROUPED, **kw, **WANTS), read + ["HOTEL", "hotel"])
    yield calls
    g.set_lexicon([])


KEYS1 = [key_of(match=m, decode=d, split=s, lattice=l, fold=f) for m in (False, True) for d in (False, True) for s, l in ((False, False), (True, False), (True, True))
         for f in ((False, True) if m else (None,))]


def test_the_scenes_have_the_18_and_12_combinations():
    assert len(KEYS1) == len(set(KEYS1)) == 18 and len(KEYS2) == len(set(KEYS2)) == 12


@pytest.mark.parametrize("key", KEYS1, ids=lambda k: "-".join(n for n, on in zip(("match", "decode", "split", "lattice", "track", "fold"), k) if on) or "plain")
def test_words_that_split(calls1, key):
    alone = calls1.get(key_of(split=True))
    assert (alone.word_splits["n_parts"] > alone.words["n_runs"]).any() and (alone.split_parts["piece"] >= 0).any()          # the scene's conditions
    check_call(calls1, key, TABLES, np.arange(65, dtype=np.int64))


@pytest.fixture(scope="module")
def calls2(track_scene, tmp_path_factory):  # noqa: F811
    S, f, prm, path, frames, seg_of, lexicon, plain, res = track_scene
    labels = np.asarray(_shipped(S, tmp_path_factory, 5)[1].label, np.int64)
    batch = np.stack(frames[:sum(s < 2 for s in seg_of)])
    read = sorted({plain.word_text(w) for w in range(len(plain.words))})
    f.set_bigram(S.bigram_from_words([t for t in read if 1 <= len(t) <= 32 and all(ch in WM.ALPHABET for ch in t)]))
    f.set_word_decode(INS, DEL)
    f.set_run_split(NUM, DEN, SPLIT)
    calls = Calls(f, lambda **kw: f.text_detect(batch, GROUPED, **kw, **LINKED), lexicon)
    yield calls, labels
    f.set_lexicon(lexicon)
    f.set_run_split()
    f.set_word_decode()
    f.set_bigram(None)


KEYS2 = [key_of(match=True, track=True, decode=d, split=s, lattice=l, fold=f) for d in (False, True) for s, l in ((False, False), (True, False), (True, True))
         for f in (False, True)]


@pytest.mark.parametrize("key", KEYS2, ids=lambda k: "-".join(n for n, on in zip(("match", "decode", "split", "lattice", "track", "fold"), k) if on))
def test_word_tracks_of_a_video(calls2, key):
    calls, labels = calls2
    assert (calls.get(key_of(match=True, track=True, fold=True)).word_tracks["count"] >= 2).any()          # the scene's conditions
    assert (calls.get(key_of(split=True)).run_splits["n_cuts"] > 0).any()
    check_call(calls, key, TRACK_TABLES[:-3], labels)
