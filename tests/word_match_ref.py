"""A numpy reference of the lexicon matcher (str_er_word_match in include/str_er.h), written from the definition: the threshold table
from the eight literals of the issue (not from the library), cost(), the cost row of a run, the edit distance vectorised over the
entries of one length, and the best / second result of a word."""
import numpy as np

ALPHABET = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz&()"
assert len(ALPHABET) == 65
LABEL_OF = {ch: a for a, ch in enumerate(ALPHABET)}
M = [float.fromhex(h) for h in ("0x1.0000000000000p+0", "0x1.d5818dcfba487p-1", "0x1.ae89f995ad3adp-1", "0x1.8ace5422aa0dbp-1",
                                "0x1.6a09e667f3bcdp-1", "0x1.4bfdad5362a27p-1", "0x1.306fe0a31b715p-1", "0x1.172b83c7d517bp-1")]
T = np.array([np.ldexp(M[c % 8], -(c // 8)) for c in range(255)], np.float64)
assert (np.diff(T) < 0).all() and T[0] == 1.0 and T[8] == 0.5
MATCH_FIELDS = ("entry", "cost", "second_entry", "second_cost", "free_cost", "n_tried")


def cost(p) -> np.ndarray:
    """The smallest c in 0 .. 254 with p >= T[c], otherwise 255 (NaN and negative values: 255), elementwise."""
    p = np.asarray(p, np.float64)
    with np.errstate(invalid="ignore"):
        ge = p[..., None] >= T                      # (a comparison with NaN is False)
    return np.where(ge.any(-1), ge.argmax(-1), 255).astype(np.uint8)


def partner(a: int) -> int:
    ch = ALPHABET[a]
    return LABEL_OF[ch.swapcase()] if ch.isalpha() else a


PARTNER = np.array([partner(a) for a in range(65)])


def fold_rows(C: np.ndarray) -> np.ndarray:
    """Both letters of a case pair get the minimum of the two."""
    C = np.asarray(C, np.uint8).reshape(-1, 65)
    return np.minimum(C, C[:, PARTNER])


def cost_rows(prob, labels, fold=False) -> np.ndarray:
    """(n, 65) uint8: C[a] = cost(prob[j]) for the first class j whose label is a, 255 without one."""
    prob = np.asarray(prob, np.float64)
    assert prob.ndim == 2 and prob.shape[1] == len(labels)
    C = np.full((len(prob), 65), 255, np.uint8)
    seen = set()
    for j, a in enumerate(labels):
        a = int(a)
        if 0 <= a < 65 and a not in seen:
            seen.add(a)
            C[:, a] = cost(prob[:, j])
    return fold_rows(C) if fold else C


def entry_costs(C: np.ndarray, E: np.ndarray, ins: int, dele: int) -> np.ndarray:
    """D[m][l] of the m cost rows C (m, 65) for every row of E (n entries, l labels): the recurrence as it is written, row by row."""
    m, (n, l) = len(C), E.shape
    D = np.zeros((m + 1, l + 1, n), np.int64)
    D[:, 0, :] = (np.arange(m + 1) * dele)[:, None]
    D[0, :, :] = (np.arange(l + 1) * ins)[:, None]
    for i in range(1, m + 1):
        for j in range(1, l + 1):
            D[i, j] = np.minimum(np.minimum(D[i - 1, j - 1] + C[i - 1][E[:, j - 1]], D[i - 1, j] + dele), D[i, j - 1] + ins)
    return D[m, l]


class Lexicon:
    def __init__(self, words, fold_case=True):
        self.words = [w if isinstance(w, str) else bytes(w).decode("latin-1") for w in words]
        self.fold = bool(fold_case)
        self.by_len = {}
        for e, w in enumerate(self.words):
            assert 1 <= len(w) <= 32
            self.by_len.setdefault(len(w), []).append(e)
        self.by_len = {l: (np.array(ix), np.array([[LABEL_OF[ch] for ch in self.words[e]] for e in ix])) for l, ix in self.by_len.items()}


def match_word(C: np.ndarray, lex: Lexicon, ins=64, dele=64, band=2) -> tuple:
    """The str_er_word_match of one word with the cost rows C (m, 65), as a tuple in the order of MATCH_FIELDS."""
    C = np.asarray(C, np.uint8).reshape(-1, 65)
    m = len(C)
    free = int(C.min(axis=1).astype(np.int64).sum()) if m else 0
    keys = []
    if m <= 32:
        Cm = fold_rows(C) if lex.fold else C
        for l, (ix, E) in lex.by_len.items():
            if abs(l - m) <= band:
                keys += list(zip(entry_costs(Cm.astype(np.int64), E, ins, dele).tolist(), ix.tolist()))
    keys.sort()
    best = keys[0] if keys else (-1, -1)
    second = keys[1] if len(keys) > 1 else (-1, -1)
    return (best[1], best[0], second[1], second[0], free, len(keys))


def match_words(costs, first_run, n_of, lex: Lexicon, ins=64, dele=64, band=2) -> list:
    costs = np.asarray(costs, np.uint8).reshape(-1, 65)
    return [match_word(costs[f:f + n], lex, ins, dele, band) for f, n in zip(first_run, n_of)]


def as_tuples(matches) -> list:
    """The library's WORD_MATCH_DTYPE records as tuples in the order of MATCH_FIELDS."""
    return [tuple(int(r[k]) for k in MATCH_FIELDS) for r in matches]
