"""The reading chain behind the run scorer under the legal combinations of its thirteen consumers -- the flags STR_ER_WANT_WORD_MATCH,
_WORD_DECODE, _RUN_SPLIT, _LATTICE_DECODE, _TRACK_READ, _LATTICE_MATCH, _LATTICE_TRACK and _TRACK_DECODE, the context settings
set_word_margin, set_lattice_margin, set_lattice_track_decode, set_line_decode and set_line_margin, and a lexicon that folds or does
not: every table of every call is byte for byte the same table of the SMALLEST call that produces it, so which consumers run beside each
other moves no byte of any of them.  A setting is switched on before its call and back to the default after it, and a table is only
ever compared between calls made on the same context.

    tables                                                             the smallest call
    base tables                                                        no flag, no setting
    run_splits, run_pieces, piece_reads, split_parts, word_splits      split alone
    word_matches                                                       match (with the call's split and fold)
    word_decodes, word_decode_chars, word_decode_src                   decode (with the call's split)
    the word margin tables                                             decode and set_word_margin (with the call's split)
    the line decode tables                                             decode and set_line_decode (with the call's split)
    the line margin tables                                             decode, set_line_decode and set_line_margin (with the call's split)
    the lattice tables                                                 split and lattice
    the lattice margin tables                                          split, lattice and set_lattice_margin
    the lattice match tables                                           match, split and lattice match (with the call's fold)
    word links and word tracks                                         match and track; decode and track decode where the call has no track read
    track_matches, track_member_costs                                  match and track (with the call's split and fold)
    the track decode tables                                            decode and track decode (with the call's split)
    the lattice track decode tables                                    decode, split, lattice, track decode and set_lattice_track_decode
    the lattice track match tables                                     match, split, lattice match, track and lattice track (with the call's fold)

The smallest calls themselves are held to the host references by the *_pipeline.py modules.  run_costs is word_match_ref.cost_rows of
the call's own run_probs (of the decoder's where the call returns none), folded iff the matcher runs with a lexicon that folds.  The
pieces' probabilities are not part of a result: piece_costs is the unfolded rows of the call with split alone
(test_run_split_pipeline.py holds those to the probabilities), folded in the same case -- cost_rows(p, labels, True) is by definition
fold_rows(cost_rows(p, labels, False)).  A table whose flag or setting is off, or whose dependency is missing (read_plan.h zeroes it),
raises ValueError.

The key lists are derived from a restatement of stage_rules.h (legal) and read_plan.h (plan), below; the first test, which needs no GPU,
holds their counts, that every pair of consumers that can legally run together in a scene does so in one of its keys, and that the 18 + 12
keys of the five original flags are among them.

Scene 1: the `proto` fixture of test_lattice_decode_pipeline.py (two frames, a prototype model with which words split, a bigram table,
INS / DEL 40 / 90, split 1 / 2 / 8; the table is made here, from the strings it reads in the other case), no links: the full legal product of match (off, on, on and folding), decode, (split, lattice, lattice
margin) in {none, s, s + l, s + l + margin}, the lattice match where match and split are on, the word margin where decode is on, the line
decode and its margin where decode is on: 126 keys.  Scene 2: the equal-size prefix of test_line_links.make_video as one batch call, the
shipped model and the lexicon of test_track_read_pipeline.py's scene, under a table that makes a word of one character dear: the product of the track-side consumers (track read, lattice track,
track decode, lattice track decode), each at the fewest other flags its rules allow and once more with every other consumer and setting
on, fold on and off, and the 12 keys of before: 43 keys.

What keeps the comparison from passing vacuously is asserted on the reference side, by the host entry points on the smallest calls'
tables (conditions1, conditions2): under the folding lexicon A and U differ on some row of some word, and the word decoder and the line
decoder give another record on the folded rows than on the unfolded ones, so a decoder that read the wrong set would change a byte; some
line has two words and a break, some line margin and some word margin are positive and finite, some lattice margin record has a cut
margin, some member of a lattice track decode takes more parts than it has runs; words split, and a word track has two members."""
import itertools
from collections import namedtuple

import numpy as np
import pytest

import word_match_ref as WM
from test_frame_lines import GROUPED
from test_lattice_decode_pipeline import INS, DEL, LATTICE_TABLES, proto  # noqa: F401  (the fixture)
from test_lattice_margin_pipeline import MARGIN_TABLES as LATTICE_MARGIN_TABLES
from test_lattice_match_pipeline import MATCH_TABLES
from test_lattice_track_decode_pipeline import NEW as LATTICE_TRACK_DECODE_TABLES
from test_lattice_track_pipeline import TRACK_TABLES as LATTICE_TRACK_TABLES
from test_line_decode_pipeline import LINE_TABLES
from test_line_margin_pipeline import MARGIN_TABLES as LINE_MARGIN_TABLES
from test_run_split_pipeline import NUM, DEN, SPLIT, _part_rows, scene as split_scene  # noqa: F401  (the fixture proto builds on)
from test_svm_exact import _shipped
from test_track_decode_pipeline import NEW as TRACK_DECODE_TABLES
from test_track_read_pipeline import NEW, TABLES as TRACK_TABLES, scene as track_scene  # noqa: F401  (the fixture)
from test_word_margin_pipeline import MARGIN_TABLES as WORD_MARGIN_TABLES
from test_word_match_pipeline import TABLES, WANTS

scene = split_scene          # (proto asks for the fixture by this name)
SPLIT_TABLES = ("run_splits", "run_pieces", "piece_reads", "split_parts", "word_splits")
DECODE_TABLES = ("word_decodes", "word_decode_chars", "word_decode_src")
LINKED = dict(want_line_links=True, **WANTS)
INF = 1 << 20                # (str_er_line_decode's: a margin at or above it is no path)

# the thirteen consumers of run_read_stage, as a call names them: eight flags (split is k_split_words) and five settings
FLAGS = ("match", "decode", "split", "lattice", "track", "lmatch", "ltrack", "tdecode")
SETTINGS = ("wmargin", "lmargin", "ltdecode", "ldecode", "lnmargin")
CONSUMERS = FLAGS + SETTINGS
Key = namedtuple("Key", ("match", "decode", "split", "lattice", "track", "fold") + CONSUMERS[5:])


def key_of(match=False, decode=False, split=False, lattice=False, track=False, fold=None, lmatch=False, ltrack=False, tdecode=False, wmargin=False, lmargin=False,
           ltdecode=False, ldecode=False, lnmargin=False):
    return Key(match, decode, split, lattice, track, bool(fold) if match else None, lmatch, ltrack, tdecode, wmargin, lmargin, ltdecode, ldecode, lnmargin)


def legal(k, links):
    """stage_rules.h on the consumers' flags, in a call that carries STR_ER_WANT_RUN_READ and what it rides on, and STR_ER_WANT_LINE_LINKS
    iff `links`.  The settings meet no rule."""
    return ((not k.lattice or k.split) and (not k.lmatch or (k.split and k.match)) and (not k.track or (k.match and links))
            and (not k.ltrack or (k.track and k.lmatch)) and (not k.tdecode or (k.decode and links)))


def plan(k):
    """read_plan.h: the consumers that run in a legal call of the key (a setting whose dependency is missing does nothing)."""
    lattice, track = k.lattice and k.split, k.track and k.match
    lmatch = k.lmatch and k.split and k.match
    tdecode, ldecode = k.tdecode and k.decode, k.ldecode and k.decode
    return k._replace(lattice=lattice, track=track, lmatch=lmatch, ltrack=k.ltrack and lmatch and track, tdecode=tdecode, wmargin=k.wmargin and k.decode,
                      lmargin=k.lmargin and lattice, ltdecode=k.ltdecode and tdecode and lattice, ldecode=ldecode, lnmargin=k.lnmargin and ldecode)


def running(k):
    p = plan(k)
    return {c for c in CONSUMERS if getattr(p, c)}


def legal_pairs(links):
    """Every pair of consumers that some legal call of the scene runs together."""
    pairs = set()
    for bits in itertools.product((False, True), repeat=len(CONSUMERS)):
        k = key_of(fold=False, **dict(zip(CONSUMERS, bits)))
        if legal(k, links):
            pairs |= set(itertools.combinations(sorted(running(k)), 2))
    return pairs


def key_id(k):
    return "-".join(n for n in Key._fields if getattr(k, n)) or "plain"


FOLDS = {False: (None,), True: (False, True)}
# scene 1: the full legal product, no links
KEYS1 = [key_of(match=m, fold=f, decode=d, split=s, lattice=l, lmargin=g, lmatch=x, wmargin=wm, ldecode=ld, lnmargin=ln)
         for m in (False, True) for f in FOLDS[m] for d in (False, True)
         for s, l, g in ((False, False, False), (True, False, False), (True, True, False), (True, True, True))
         for x in ((False, True) if m and s else (False,)) for wm in ((False, True) if d else (False,))
         for ld, ln in (((False, False), (True, False), (True, True)) if d else ((False, False),))]
OLD1 = [key_of(match=m, decode=d, split=s, lattice=l, fold=f) for m in (False, True) for d in (False, True) for s, l in ((False, False), (True, False), (True, True))
        for f in FOLDS[m]]


def _fewest(want):
    """The key of the fewest flags and settings with which the rules let the track-side consumers `want` run."""
    k = dict.fromkeys(CONSUMERS, False)
    k.update(want)
    for _ in range(len(CONSUMERS)):          # (to the fixed point: a dependency has dependencies)
        k["lmatch"] |= k["ltrack"]
        k["track"] |= k["ltrack"]
        k["tdecode"] |= k["ltdecode"]
        k["lattice"] |= k["ltdecode"]
        k["split"] |= k["lattice"] or k["lmatch"]
        k["match"] |= k["track"] or k["lmatch"]
        k["decode"] |= k["tdecode"]
    return k


TRACK_SIDE = [dict(track=t, ltrack=lt, tdecode=td, ltdecode=ltd) for t, lt in ((False, False), (True, False), (True, True))
              for td, ltd in ((False, False), (True, False), (True, True))]
OLD2 = [key_of(match=True, track=True, decode=d, split=s, lattice=l, fold=f) for d in (False, True) for s, l in ((False, False), (True, False), (True, True)) for f in (False, True)]
KEYS2 = list(dict.fromkeys([key_of(fold=f, **_fewest(w)) for w in TRACK_SIDE for f in FOLDS[_fewest(w)["match"]]]
                           + [key_of(fold=f, **dict(dict.fromkeys(CONSUMERS, True), **w)) for w in TRACK_SIDE for f in (False, True)] + OLD2))


def test_the_scenes_have_the_18_and_12_combinations():
    assert len(OLD1) == len(set(OLD1)) == 18 and len(OLD2) == len(set(OLD2)) == 12 and set(OLD1) <= set(KEYS1) and set(OLD2) <= set(KEYS2)
    assert len(KEYS1) == len(set(KEYS1)) == 126 and len(KEYS2) == len(set(KEYS2)) == 43
    assert all(legal(k, False) for k in KEYS1) and all(legal(k, True) for k in KEYS2)
    # the product of the track-side consumers, at the fewest flags and with everything else on
    assert len(TRACK_SIDE) == 9 and sorted(len(running(key_of(fold=False, **_fewest(w)))) for w in TRACK_SIDE) == [0, 2, 2, 4, 5, 5, 7, 7, 9]
    for w in TRACK_SIDE:
        few = key_of(fold=False, **_fewest(w))
        assert legal(few, True) and {c for c in w if w[c]} <= running(few)
        for c in running(few):                                 # fewest: no flag or setting can go without a wanted consumer going or a rule refusing
            less = few._replace(**{c: False})
            assert w[c] if c in w else not (legal(less, True) and {c for c in w if w[c]} <= running(less)), (w, c)
        full = key_of(fold=True, **dict(dict.fromkeys(CONSUMERS, True), **w))
        assert running(full) == set(CONSUMERS) - {c for c in w if not w[c]}
    # every pair of consumers that can legally run together in a scene does so in one of its keys
    assert len(CONSUMERS) == 13
    for keys, links in ((KEYS1, False), (KEYS2, True)):
        met = set()
        for k in keys:
            met |= set(itertools.combinations(sorted(running(k)), 2))
        assert met == legal_pairs(links), sorted(legal_pairs(links) - met)
    assert len(legal_pairs(True)) == 13 * 12 // 2 and len(legal_pairs(False)) == 9 * 8 // 2          # (without links: no track-side consumer)


class Calls:
    """The detect call of a scene under a key, each made once."""

    def __init__(self, f, detect, lexicon):
        self.f, self.detect, self.lexicon, self.fold, self.made = f, detect, lexicon, None, {}

    def settings(self, k=key_of()):
        self.f.set_word_margin(k.wmargin); self.f.set_lattice_margin(k.lmargin); self.f.set_lattice_track_decode(k.ltdecode)
        self.f.set_line_decode(k.ldecode); self.f.set_line_margin(k.lnmargin)

    def get(self, key):
        if key not in self.made:
            if key.match and key.fold != self.fold:
                self.f.set_lexicon(self.lexicon, fold_case=key.fold)
                self.fold = key.fold
            self.settings(key)
            try:
                self.made[key] = self.detect(want_word_match=key.match, want_word_decode=key.decode, want_run_split=key.split, want_lattice_decode=key.lattice,
                                             want_track_read=key.track, want_lattice_match=key.lmatch, want_lattice_track=key.ltrack, want_track_decode=key.tdecode)
            finally:
                self.settings()
        return self.made[key]


def check_call(calls, key, base_tables, labels):
    p = plan(key)
    split, fold = p.split, p.fold
    res = calls.get(key)

    def same(ref_key, names):
        ref = calls.get(ref_key)
        for k in names:
            assert getattr(ref, k).tobytes() == getattr(res, k).tobytes(), (key_id(key), k)

    def absent(names):
        for k in names:
            with pytest.raises(ValueError):
                getattr(res, k)

    def held(on, ref_key, names):
        same(ref_key, names) if on else absent(names)

    same(key_of(), base_tables)
    held(split, key_of(split=True), SPLIT_TABLES)
    if not split:
        absent(("piece_costs",))
    held(p.match, key_of(match=True, split=split, fold=fold), ("word_matches",))
    held(p.decode, key_of(decode=True, split=split), DECODE_TABLES)
    held(p.wmargin, key_of(decode=True, split=split, wmargin=True), WORD_MARGIN_TABLES)
    held(p.ldecode, key_of(decode=True, split=split, ldecode=True), LINE_TABLES)
    held(p.lnmargin, key_of(decode=True, split=split, ldecode=True, lnmargin=True), LINE_MARGIN_TABLES)
    held(p.lattice, key_of(split=True, lattice=True), LATTICE_TABLES)
    held(p.lmargin, key_of(split=True, lattice=True, lmargin=True), LATTICE_MARGIN_TABLES)
    held(p.lmatch, key_of(match=True, split=True, lmatch=True, fold=fold), MATCH_TABLES)
    if p.track:
        same(key_of(match=True, track=True, fold=True), NEW[:4])
        same(key_of(match=True, track=True, split=split, fold=fold), NEW[4:])
    else:
        absent(NEW[4:])
    if p.tdecode:
        same(key_of(decode=True, tdecode=True), NEW[:4])
    if not (p.track or p.tdecode):
        absent(NEW[:4])
    held(p.tdecode, key_of(decode=True, split=split, tdecode=True), TRACK_DECODE_TABLES)
    held(p.ltdecode, key_of(decode=True, split=True, lattice=True, tdecode=True, ltdecode=True), LATTICE_TRACK_DECODE_TABLES)
    held(p.ltrack, key_of(match=True, split=True, lmatch=True, track=True, ltrack=True, fold=fold), LATTICE_TRACK_TABLES)
    folded = bool(p.match and fold)
    if p.match or p.decode:
        same(key_of(decode=True) if p.decode else key_of(match=True, fold=fold), ("run_probs",))
        probs = res.run_probs
    else:
        absent(("run_probs",))
        probs = calls.get(key_of(decode=True)).run_probs
    if p.match or p.decode or split:
        assert res.run_costs.shape == (len(res.line_runs), 65) and (res.run_costs == WM.cost_rows(probs, labels, folded)).all(), key_id(key)
    else:
        absent(("run_costs",))
    if split:
        rows = calls.get(key_of(split=True)).piece_costs
        assert res.piece_costs.shape == rows.shape and (res.piece_costs == (WM.fold_rows(rows) if folded else rows)).all(), key_id(key)


def differ(a, b):
    """Some record of a host entry point's first table differs between two inputs."""
    return a[0].tobytes() != b[0].tobytes()


def told_apart(S, calls, table, c):
    """A and U differ where it matters: the unfolded rows of the decoder's smallest calls against the same rows folded, through the word
    decoder and the line decoder, on the runs and on the words' parts."""
    dec = calls.get(key_of(decode=True))
    U, first, n_of = dec.run_costs, dec.words["first_run"], dec.words["n_runs"]
    in_word = np.concatenate([np.arange(a, a + k) for a, k in zip(first, n_of)] + [np.zeros(0, np.int64)]).astype(np.int64)
    c["A and U differ on a row of a word"] = bool((WM.fold_rows(U) != U)[in_word].any())
    lines = {}
    for name, split in (("runs", False), ("parts", True)):
        ln = calls.get(key_of(decode=True, split=split, ldecode=True))
        rows, a, n = (_part_rows(ln), ln.word_splits["first_part"], ln.word_splits["n_parts"]) if split else (ln.run_costs, first, n_of)
        c[f"the word decoder tells A from U ({name})"] = differ(S.decode_words_host(rows, a, n, table, INS, DEL), S.decode_words_host(WM.fold_rows(rows), a, n, table, INS, DEL))
        win, gaps = ln.line_decode_windows, ln.line_gap_costs
        d = S.decode_lines_host(rows, gaps, win[:, 0], win[:, 1], table, INS, DEL)
        c[f"the line decoder tells A from U ({name})"] = differ(d, S.decode_lines_host(WM.fold_rows(rows), gaps, win[:, 0], win[:, 1], table, INS, DEL))
        lines[name] = (ln, rows, a, n, win, gaps, d)
    return lines


def conditions1(S, calls, table):
    """The conditions of scene 1, by the host entry points on the smallest calls' tables; made once."""
    if not hasattr(calls, "conditions"):
        alone = calls.get(key_of(split=True))
        c = {"words split": bool((alone.word_splits["n_parts"] > alone.words["n_runs"]).any() and (alone.split_parts["piece"] >= 0).any())}
        for name, (ln, rows, a, n, win, gaps, d) in told_apart(S, calls, table, c).items():
            c[f"a line of two words with a break ({name})"] = bool(((ln.line_words["n_words"] >= 2) & (d[0]["n_breaks"] > 0)).any())
            m = S.line_margins_host(rows, gaps, win[:, 0], win[:, 1], table, INS, DEL)[0]["margin"]
            c[f"a positive line margin ({name})"] = bool(((m > 0) & (m < INF)).any())
            m = S.word_margins_host(rows, a, n, table, INS, DEL)[0]["margin"]
            c[f"a positive word margin ({name})"] = bool(((m > 0) & (m < INF)).any())
        lg = S.lattice_margins_host(alone.run_splits, alone.run_costs, alone.piece_costs, alone.words["first_run"], alone.words["n_runs"], table, INS, DEL, SPLIT)
        c["a lattice margin record with a cut margin"] = bool((lg[0]["cut_margin"] >= 0).any())
        calls.conditions = c
        print("scene 1:", c)
    return calls.conditions


@pytest.fixture(scope="module")
def calls1(proto):  # noqa: F811
    S, g, prm, model, uniform, crops, base, base_crops, table, read = proto
    # the table of the fixture is made from the strings the model reads: it likes the case that was read, and the decoders give the same
    # records on the runs' folded and unfolded rows (measured: two run rows of 29 differ under the fold, M / m and O / o at 45 / 49 and
    # 48 / 49).  This one is made from the same strings in the other case: it likes m, which costs 49 unfolded and 45 folded
    mixed = S.bigram_from_words([t.swapcase() for t in read], alpha=0.05)
    g.set_bigram(mixed)
    calls = Calls(g, lambda **kw: g.text_detect(uniform, GROUPED, **kw, **WANTS), read + ["HOTEL", "hotel"])
    calls.settings()
    yield S, calls, mixed
    calls.settings()
    g.set_lexicon([])
    g.set_bigram(table)


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS1, ids=key_id)
def test_words_that_split(calls1, key):
    S, calls, table = calls1
    check_call(calls, key, TABLES, np.arange(65, dtype=np.int64))
    c = conditions1(S, calls, table)
    assert all(c.values()), [k for k, v in c.items() if not v]          # the scene's conditions


def conditions2(S, calls, table):
    """The conditions of scene 2, by the host entry points on the smallest calls' tables; made once."""
    if not hasattr(calls, "conditions"):
        tr, alone = calls.get(key_of(match=True, track=True, fold=True)), calls.get(key_of(split=True))
        c = {"a word track of two members": bool((tr.word_tracks["count"] >= 2).any()), "a cut run": bool((alone.run_splits["n_cuts"] > 0).any())}
        told_apart(S, calls, table, c)
        first, n_of, mem = alone.words["first_run"], alone.words["n_runs"], tr.word_track_members
        got = S.lattice_decode_tracks_host(alone.run_splits, alone.run_costs, alone.piece_costs, first, n_of, tr.word_tracks["first"], tr.word_tracks["count"], mem, table, INS, DEL,
                                           split_cost=SPLIT)
        c["a member of a lattice track decode with more parts than runs"] = bool((got[2]["n_parts"] > n_of[mem]).any())
        calls.conditions = c
        print("scene 2:", c, "members with more parts than runs:", int((got[2]["n_parts"] > n_of[mem]).sum()), "of", len(mem))
    return calls.conditions


@pytest.fixture(scope="module")
def calls2(track_scene, tmp_path_factory):  # noqa: F811
    S, f, prm, path, frames, seg_of, lexicon, plain, res = track_scene
    labels = np.asarray(_shipped(S, tmp_path_factory, 5)[1].label, np.int64)
    batch = np.stack(frames[:sum(s < 2 for s in seg_of)])
    # with the shipped model a row costs 45 .. 48 at every label, so under a table of the words that are read two pieces (45 + 45 +
    # SPLIT) never beat their run (measured: 0 members of 188 with more parts than runs).  This table knows one thing: a word begins
    # with one of the first 33 labels and ends with one of the last 32, so a word of one character is dear, and a member of one cut run
    # whose track reads two characters takes two parts rather than an insertion (measured: 69 members)
    table = np.zeros((66, 66), np.uint8)
    table[65, 33:65] = table[:33, 65] = 200
    f.set_bigram(table)
    f.set_word_decode(INS, DEL)
    f.set_run_split(NUM, DEN, SPLIT)
    calls = Calls(f, lambda **kw: f.text_detect(batch, GROUPED, **kw, **LINKED), lexicon)
    calls.settings()
    yield S, calls, labels, table
    calls.settings()
    f.set_lexicon(lexicon)
    f.set_run_split()
    f.set_word_decode()
    f.set_bigram(None)


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS2, ids=key_id)
def test_word_tracks_of_a_video(calls2, key):
    S, calls, labels, table = calls2
    check_call(calls, key, TRACK_TABLES[:-3], labels)
    c = conditions2(S, calls, table)
    assert all(c.values()), [k for k, v in c.items() if not v]          # the scene's conditions
