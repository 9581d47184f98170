"""The numpy reference of the glyph runs and words of a text line (STR_ER_WANT_LINE_WORDS, str_er_feet_words,
str_er_words_from_runs): the contract at str_er_line_run (include/str_er.h) from a boolean footprint, in numpy and Python integers.
It shares no code with the library."""
import numpy as np


def runs_of(bits, x=0, y=0):
    """(colmax, runs) of a footprint: bits (h, w) bool over the foot box at (x, y); a run is (x0, x1, y0, y1, pixels) in frame
    columns and rows, half open, ordered by x0."""
    bits = np.asarray(bits, bool)
    if bits.size == 0 or not bits.any():
        return 0, []
    n = bits.sum(axis=0).astype(np.int64)                       # the column counts
    on = np.concatenate([[False], n > 0, [False]])
    c0 = np.nonzero(on[1:] & ~on[:-1])[0]                       # column c is set and c - 1 is not
    c1 = np.nonzero(~on[1:] & on[:-1])[0]                       # column c is not set and c - 1 is
    runs = []
    for a, b in zip(c0.tolist(), c1.tolist()):
        rows = np.nonzero(bits[:, a:b].any(axis=1))[0]
        runs.append((x + a, x + b, y + int(rows[0]), y + int(rows[-1]) + 1, int(n[a:b].sum())))
    return int(n.max()), runs


def is_break(gap, colmax, num, den):
    return gap * den >= num * colmax                            # (Python integers: exact)


def words_of(runs, colmax, num=1, den=3, line=0, first_run=0):
    """(words, word index of every run) of one line: a word is (line, first_run, n_runs, x, y, w, h, pixels); the word indices
    count from 0 within the line."""
    words, idx = [], []
    for k, r in enumerate(runs):
        if k == 0 or is_break(r[0] - runs[k - 1][1], colmax, num, den):
            words.append([line, first_run + k, 0, r[0], r[2], r[1], r[3], 0])       # (x0, y0, x1, y1 for now)
        w = words[-1]
        w[2] += 1
        w[4], w[5], w[6] = min(w[4], r[2]), r[1], max(w[6], r[3])
        w[7] += r[4]
        idx.append(len(words) - 1)
    return [(w[0], w[1], w[2], w[3], w[4], w[5] - w[3], w[6] - w[4], w[7]) for w in words], idx


def tables(feet, num=1, den=3):
    """The three tables of footprints [(x, y, bits), ...] as lists of tuples in the field order of the records: line_words
    (first_word, n_words, first_run, n_runs, colmax, 0), runs (x0, x1, y0, y1, pixels, word), words."""
    lw, runs, words = [], [], []
    for t, (x, y, bits) in enumerate(feet):
        colmax, rs = runs_of(bits, x, y)
        ws, idx = words_of(rs, colmax, num, den, t, len(runs))
        lw.append((len(words), len(ws), len(runs), len(rs), colmax, 0))
        runs += [r + (len(words) + i,) for r, i in zip(rs, idx)]
        words += ws
    return lw, runs, words


def as_lists(line_words, runs, words):
    """Record arrays of the binding as the lists of tuples `tables` returns."""
    return ([tuple(int(v) for v in r) for r in line_words.tolist()], [tuple(int(v) for v in r) for r in runs.tolist()],
            [tuple(int(v) for v in r) for r in words.tolist()])
