"""The lexicon matcher on the GPU (str_er_set_lexicon, str_er_match_words, str_er_run_costs; the contract is at str_er_word_match):
every field of every record against the numpy reference (word_match_ref.py) with ==, at the kernels' own edges -- a wave of 64
entries, a chunk of the lexicon, the buckets of the run count (8, 16, 32), the band of lengths."""

import numpy as np
import pytest

import word_match_ref as WM
from test_svm_exact import _shipped

pytestmark = pytest.mark.gpu
LETTERS = list(WM.ALPHABET)


@pytest.fixture(scope="module")
def f(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    yield ctx
    ctx.close()


def _word(rng, n):
    return "".join(rng.choice(LETTERS, n))


def _rows(rng, n):
    """Random cost rows: a few cheap characters per run among dear ones, so that substitutions, INS and DEL all win somewhere."""
    c = rng.integers(60, 256, (n, 65))
    cheap = rng.random((n, 65)) < 0.08
    c[cheap] = rng.integers(0, 24, int(cheap.sum()))
    return c.astype(np.uint8)


def _reads(text, hit=0, miss=255):
    """Cost rows of runs that read `text`: `hit` at the character, `miss` elsewhere."""
    c = np.full((len(text), 65), miss, np.uint8)
    for i, ch in enumerate(text):
        c[i, WM.LABEL_OF[ch]] = hit
    return c


def _spans(n_of):
    n_of = np.asarray(n_of, np.int64)
    return np.concatenate([[0], np.cumsum(n_of)[:-1]]).astype(np.int32), n_of.astype(np.int32)


def check(f, words, costs, n_of, fold=True, ins=64, dele=64, band=2):
    """set_lexicon, set_word_match and match_words against the reference; returns the records as tuples (MATCH_FIELDS)."""
    first, n_of = _spans(n_of)
    f.set_lexicon(words, fold_case=fold)
    f.set_word_match(ins, dele, band)
    got = WM.as_tuples(f.match_words(costs, first, n_of))
    want = WM.match_words(costs, first, n_of, WM.Lexicon(words, fold), ins, dele, band)
    assert got == want, [(w, g, x) for w, (g, x) in enumerate(zip(got, want)) if g != x][:5]
    return got


def test_lexicon_sizes_around_a_wave_and_a_chunk(f):
    rng = np.random.default_rng(1)
    chunk = f.lexicon_info()["chunk_entries"]
    assert chunk >= 64 and chunk % 64 == 0
    costs = _rows(rng, 15)
    for n in (1, 63, 64, 65, chunk + 1):
        words = [_word(rng, 5) for _ in range(n)]
        words[-1] = words[0]                               # the last entry (the lane past the wave, the entry past the chunk) ties with the first
        got = check(f, words, costs, [5, 5, 5])
        info = f.lexicon_info()
        assert info["n"] == n and info["flags"] == 1 and info["device_bytes"] > 0
        assert all(g[5] == n for g in got)
        if n > 1:
            assert all(g[0] != g[2] and g[2] >= 0 for g in got)
    # the entry past the chunk wins alone
    words = [_word(rng, 5) for _ in range(chunk)] + ["HOTEL"]
    got = check(f, words, _reads("HOTEL", 1), [5])
    assert got[0][:2] == (chunk, 5)


def test_run_counts_and_entry_lengths(f):
    rng = np.random.default_rng(2)
    words = [_word(rng, l) for l in range(1, 33) for _ in range(3)]
    n_of = [1, 2, 8, 9, 16, 17, 31, 32, 33, 0]
    costs = _rows(rng, sum(n_of))
    for band in (2, 0, 31):
        got = check(f, words, costs, n_of, band=band)
        assert got[8][:4] == (-1, -1, -1, -1) and got[8][5] == 0 and got[8][4] > 0         # 33 runs: nothing is tried
        assert got[9][5] == (0 if band == 0 else 3 * band) and got[9][4] == 0                # no runs: the entries up to the band, all INS
    # entries of length 1 and of length 32 alone
    for l, m in ((1, 1), (1, 3), (32, 32), (32, 30)):
        words = [_word(rng, l) for _ in range(70)]
        check(f, words, _rows(rng, m), [m])


def test_band(f):
    rng = np.random.default_rng(3)
    costs = np.zeros((32, 65), np.uint8)                      # every character is free: the cost is the difference of the lengths
    for band, m in ((2, 10), (0, 10), (31, 1), (31, 32), (30, 32), (5, 30)):
        for l in (m - band - 1, m - band, m + band, m + band + 1):
            if not 1 <= l <= 32:
                continue
            got = check(f, [_word(rng, l)], costs, [m], band=band)[0]
            if abs(l - m) <= band:
                assert got == (0, abs(l - m) * 64, -1, -1, 0, 1), (band, m, l)
            else:
                assert got == (-1, -1, -1, -1, 0, 0), (band, m, l)                           # a word with no entry in its band
    words = [_word(rng, l) for l in range(1, 33)]
    for band, m, tried in ((2, 10, 5), (0, 10, 1), (31, 1, 32), (31, 32, 32), (2, 1, 3), (2, 32, 3), (31, 33, 0)):
        got = check(f, words, np.zeros((33, 65), np.uint8), [m], band=band)[0]
        assert got[5] == tried and got[0] == (m - 1 if tried else -1)


def test_ties_and_extremes(f):
    got = check(f, ["AB", "CD", "AB"], _reads("AB", 3), [2])[0]
    assert got == (0, 6, 2, 6, 6, 3)                          # two equal entries: the lower index wins, the other is second at the same cost
    got = check(f, ["AB"], _reads("AB", 3), [2])[0]
    assert got == (0, 6, -1, -1, 6, 1)                        # a one-entry lexicon has no second
    rng = np.random.default_rng(4)
    words = [_word(rng, 32) for _ in range(65)]
    got = check(f, words, np.full((32, 65), 255, np.uint8), [32], ins=255, dele=255)[0]
    assert got == (0, 32 * 255, 1, 32 * 255, 32 * 255, 65)
    got = check(f, words, np.zeros((32, 65), np.uint8), [32], ins=255, dele=255)[0]
    assert got == (0, 0, 1, 0, 0, 65)


def test_hand_made_paths(f):
    noise = np.full((1, 65), 200, np.uint8)
    three = np.concatenate([_reads("A", 0, 200), noise, _reads("B", 0, 200)])
    got = check(f, ["AB", "ABC", "B"], three, [3])[0]
    assert got[:2] == (0, 64)                                 # A, a run with no character of its own, B
    one = np.full((1, 65), 255, np.uint8)
    one[0, WM.LABEL_OF["A"]], one[0, WM.LABEL_OF["B"]] = 8, 16
    got = check(f, ["AB", "XY"], one, [1])[0]
    assert got[:2] == (0, 72)                                 # the run is the A, the B has no run of its own
    hotel = _reads("HOTEL", 2)
    got = check(f, ["motel", "hotel", "HOTELS"], hotel, [5], fold=True)[0]
    assert got[:2] == (1, 10) and got[4] == 10                # a fold-case hit, reported as given
    got = check(f, ["motel", "hotel", "HOTELS"], hotel, [5], fold=False)[0]
    assert got[:2] == (2, 10 + 64)
    zero = _reads("H0TEL", 2)
    zero[1, WM.LABEL_OF["O"]] = 30                            # run 2 read 0, and O was its second guess
    got = check(f, ["HOTEL", "H0TEL", "MOTEL"], zero, [5])[0]
    assert got == (1, 10, 0, 38, 10, 3)


def test_random_words_against_random_entries(S, f):
    rng = np.random.default_rng(5)
    words = [_word(rng, int(rng.integers(1, 33))) for _ in range(3000)]
    n_of = rng.integers(1, 33, 200)
    n_of[:3] = (33, 0, 32)
    costs = _rows(rng, int(n_of.sum()))
    # entries near the words' own readings, so that the best is not always all INS and DEL
    first, _ = _spans(n_of)
    for w in range(0, 200, 2):
        m = int(n_of[w])
        if 1 <= m <= 32:
            text = "".join(WM.ALPHABET[int(a)] for a in costs[first[w]:first[w] + m].argmin(axis=1))
            words[int(rng.integers(0, 3000))] = text if w % 4 else (text[:-1] or "A")
    got = check(f, words, costs, n_of)
    assert sum(g[1] <= g[4] + 64 for g in got if g[0] >= 0) > 40          # (many words find their own reading, or it less a character)
    host = WM.as_tuples(S.match_words_host(costs, first, n_of, words, True, 64, 64, 2))
    assert host == got
    check(f, words, costs, n_of[:60], fold=False, ins=23, dele=120, band=4)


def test_no_words_and_the_same_call_twice(S, f):
    rng = np.random.default_rng(6)
    words = [_word(rng, int(rng.integers(1, 12))) for _ in range(500)]
    f.set_lexicon(words)
    f.set_word_match()
    costs = _rows(rng, 40)
    out = f.match_words(costs, [], [])
    assert out.shape == (0,) and out.dtype == S.WORD_MATCH_DTYPE
    assert f.match_words(np.zeros((0, 65), np.uint8), [], []).shape == (0,)
    first, n_of = _spans([5, 0, 7, 8, 9, 11])
    a = f.match_words(costs, first, n_of)
    b = f.match_words(costs, first, n_of)
    assert a.tobytes() == b.tobytes() and len(a) == 6
    # overlapping words are words too
    c = f.match_words(costs, [0, 0, 3], [5, 5, 6])
    assert c[0].tobytes() == c[1].tobytes() == a[0].tobytes()


def test_run_costs_equal_prob_costs(S, f, tmp_path_factory):
    path, m = _shipped(S, tmp_path_factory, 5)
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    try:
        with pytest.raises(S.StrErError) as e:
            ctx.run_costs(np.zeros((1, 65)))
        assert e.value.code == -6
        ctx.load_svm_model(path, 1800)
        k = ctx.svm_info()[0]
        labels = np.asarray(m.label, np.int64)
        assert k == len(labels) == m.k
        T = WM.T
        vals = np.concatenate([T, np.nextafter(T, 0.0), np.nextafter(T, 2.0), [0.0, 1.0, np.nan, -1.0, np.inf, 2.0, 5e-324]])
        n = (len(vals) + k - 1) // k + 300
        rng = np.random.default_rng(7)
        prob = np.exp2(-rng.uniform(0, 36, (n, k)))
        prob.reshape(-1)[:len(vals)] = vals
        for fold in (False, True):
            ctx.set_lexicon(["A"], fold_case=fold)
            got = ctx.run_costs(prob)
            assert got.shape == (n, 65)
            assert (got == S.prob_costs(prob, labels, fold)).all() and (got == WM.cost_rows(prob, labels, fold)).all()
        ctx.set_lexicon([])                                   # without a lexicon: not folded
        assert (ctx.run_costs(prob) == WM.cost_rows(prob, labels, False)).all()
        assert ctx.run_costs(np.zeros((0, k))).shape == (0, 65)
    finally:
        ctx.close()


def test_errors_leave_the_context_as_it_was(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    L = ctx.L
    try:
        costs = _reads("AB", 1)
        with pytest.raises(S.StrErError) as e:                # no lexicon
            ctx.match_words(costs, [0], [2])
        assert e.value.code == -6 and "lexicon" in str(e.value)
        ctx.set_lexicon(["AB", "ab", "B"], fold_case=False)
        before = ctx.lexicon_info()
        want = ctx.match_words(costs, [0], [2])
        assert WM.as_tuples(want) == [(0, 2, 2, 65, 2, 3)]
        for bad in (["AB", "A B"], ["AB", ""], ["A" * 33], ["AB", "A-B"], ["é"]):
            with pytest.raises(S.StrErError) as e:            # a byte outside the alphabet, a length of 0 or above 32
                ctx.set_lexicon(bad)
            assert e.value.code == -1
            assert ctx.lexicon_info() == before
        raw = np.frombuffer(b"ABCD", np.uint8)
        for off in ([1, 2, 4], [0, 2, 1], [0, 0, 4], [0, 2, 40]):
            o = np.array(off, np.int32)                       # offsets that do not lie back to back
            assert L.str_er_set_lexicon(ctx.h, raw.ctypes.data, o.ctypes.data, 2, 0) == -1
        o = np.array([0, 2, 4], np.int32)
        assert L.str_er_set_lexicon(ctx.h, raw.ctypes.data, o.ctypes.data, 2, 2) == -1       # an unknown flag
        assert L.str_er_set_lexicon(ctx.h, raw.ctypes.data, o.ctypes.data, (1 << 20) + 1, 0) == -7
        for ins, dele, band in ((0, 64, 2), (64, 256, 2), (64, 64, 32), (64, 64, -1)):
            with pytest.raises(S.StrErError) as e:
                ctx.set_word_match(ins, dele, band)
            assert e.value.code == -1
        with pytest.raises(S.StrErError) as e:                # a word outside the cost rows
            ctx.match_words(costs, [1], [2])
        assert e.value.code == -1
        with pytest.raises(S.StrErError) as e:
            ctx.match_words(costs, [0], [-1])
        assert e.value.code == -1
        assert ctx.lexicon_info() == before
        assert ctx.match_words(costs, [0], [2]).tobytes() == want.tobytes()
        ctx.set_lexicon([])                                   # cleared
        assert ctx.lexicon_info()["n"] == 0 and ctx.lexicon_info()["device_bytes"] == 0
        with pytest.raises(S.StrErError) as e:
            ctx.match_words(costs, [0], [2])
        assert e.value.code == -6
    finally:
        ctx.close()
