"""A numpy reference of the open-vocabulary word decoder (str_er_word_decode in include/str_er.h), written from the definition: the
recurrence over a word's cost rows and a bigram table with the optional DEL and INS moves, the backtrack, read_cost, and an enumeration
of every path (a run dropped, read, or read with one character inserted after it) for small alphabets.  The alphabet size is a
parameter: the library's is 65, the boundary symbol is E = n."""
import itertools

import numpy as np

INF = 1 << 20
MAX_RUNS = 32
DECODE_FIELDS = ("cost", "read_cost", "n_chars", "n_sub", "n_del", "n_ins")


def _first_argmin(v) -> int:
    return int(np.argmin(np.asarray(v)))                 # (numpy: the first of equal minima)


def read_cost(C, B, n=65) -> int:
    """The plain reading under B: the first arg min of every row, all SUB, with the boundary terms."""
    C = np.asarray(C, np.int64).reshape(-1, n)
    B = np.asarray(B, np.int64).reshape(n + 1, n + 1)
    prev, s = n, 0
    for row in C:
        r = _first_argmin(row)
        s += int(B[prev, r]) + int(row[r])
        prev = r
    return s + int(B[prev, n])


def decode_word(C, B, ins=0, dele=0, n=65):
    """One word: (record as a tuple in the order of DECODE_FIELDS, labels, sources)."""
    C = np.asarray(C, np.int64).reshape(-1, n)
    B = np.asarray(B, np.int64).reshape(n + 1, n + 1)
    m, E = len(C), n
    rc = read_cost(C, B, n)
    if m > MAX_RUNS:
        return (-1, rc, 0, 0, 0, 0), [], []
    V = np.full(n + 1, INF, np.int64)
    V[E] = 0
    steps = []                                            # per run: (sub_pred, is_del, is_ins, ins_pred)
    for i in range(1, m + 1):
        cand = V[:, None] + B[:, :n]                      # [a, b]
        sub_pred = np.zeros(n + 1, np.int64)
        sub_pred[:n] = cand.argmin(axis=0)
        U = np.full(n + 1, INF, np.int64)
        U[:n] = cand.min(axis=0) + C[i - 1]
        is_del = np.zeros(n + 1, bool)
        if dele > 0:
            D = V + dele
            is_del = D < U
            U = np.where(is_del, D, U)
        is_ins = np.zeros(n + 1, bool)
        ins_pred = np.zeros(n + 1, np.int64)
        W = U.copy()
        if ins > 0:
            ci = U[:n, None] + B[:n, :n]                  # [b, c]
            I = ci.min(axis=0) + ins
            ins_pred[:n] = ci.argmin(axis=0)
            is_ins[:n] = I < U[:n]
            W[:n] = np.where(is_ins[:n], I, U[:n])
        steps.append((sub_pred, is_del, is_ins, ins_pred))
        V = W
    end = V + B[:, E]
    state = _first_argmin(end)
    cost = int(end[state])
    assert cost < INF
    labels, src = [], []
    n_sub = n_del = n_ins = 0
    for i in range(m, 0, -1):
        sub_pred, is_del, is_ins, ins_pred = steps[i - 1]
        if is_ins[state]:
            labels.append(state); src.append((i - 1) | 0x80); n_ins += 1
            state = int(ins_pred[state])
        if is_del[state]:
            n_del += 1
        else:
            labels.append(state); src.append(i - 1); n_sub += 1
            state = int(sub_pred[state])
    assert state == E
    labels.reverse(); src.reverse()
    return (cost, rc, len(labels), n_sub, n_del, n_ins), labels, src


def decode_words(costs, first_run, n_of, B, ins=0, dele=0, n=65):
    """Every word: the records as tuples, chars (n_words, 64) and src (n_words, 64) uint8, padded with 0xFF."""
    costs = np.asarray(costs, np.uint8).reshape(-1, n)
    recs = []
    chars = np.full((len(first_run), 64), 0xFF, np.uint8)
    src = np.full((len(first_run), 64), 0xFF, np.uint8)
    for w, (f, k) in enumerate(zip(first_run, n_of)):
        rec, lab, s = decode_word(costs[int(f):int(f) + int(k)], B, ins, dele, n)
        recs.append(rec)
        chars[w, :len(lab)] = lab
        src[w, :len(s)] = s
    return recs, chars, src


def path_cost(C, B, labels, src, ins, dele, n=65):
    """The cost of a returned string under the definition: every run is read once or dropped, inserted characters pay INS."""
    C = np.asarray(C, np.int64).reshape(-1, n)
    B = np.asarray(B, np.int64).reshape(n + 1, n + 1)
    prev, s, used = n, 0, set()
    for a, r in zip(labels, src):
        s += int(B[prev, a])
        if r & 0x80:
            s += ins
        else:
            s += int(C[r, a]); used.add(r)
        prev = a
    return s + int(B[prev, n]) + dele * (len(C) - len(used))


def enumerate_best(C, B, ins, dele, n):
    """The cheapest of every path, by brute force: per run one of DEL, SUB b, or SUB b followed by INS c."""
    C = np.asarray(C, np.int64).reshape(-1, n)
    B = np.asarray(B, np.int64).reshape(n + 1, n + 1)
    m = len(C)
    moves = ([("del",)] if dele > 0 else []) + [("sub", b) for b in range(n)]
    if ins > 0:
        moves += [("subins", b, c) for b in range(n) for c in range(n)]
        if dele > 0:
            moves += [("delins", c) for c in range(n)]       # a dropped run, then a character inserted after some character
    best = None
    for path in itertools.product(moves, repeat=m):
        prev, s, ok = n, 0, True
        for i, mv in enumerate(path):
            if mv[0] == "del":
                s += dele
            elif mv[0] == "sub":
                s += int(B[prev, mv[1]]) + int(C[i, mv[1]]); prev = mv[1]
            elif mv[0] == "subins":
                s += int(B[prev, mv[1]]) + int(C[i, mv[1]]) + int(B[mv[1], mv[2]]) + ins; prev = mv[2]
            else:
                if prev == n:                                  # only after some character
                    ok = False
                    break
                s += dele + int(B[prev, mv[1]]) + ins; prev = mv[1]
        if ok:
            s += int(B[prev, n])
            best = s if best is None or s < best else best
    return best


def as_tuples(recs) -> list:
    """The library's WORD_DECODE_DTYPE records as tuples in the order of DECODE_FIELDS."""
    return [tuple(int(r[k]) for k in DECODE_FIELDS) for r in recs]
