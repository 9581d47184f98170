"""A numpy reference of the line decoder (str_er_line_decode in include/str_er.h), written from the definition: the recurrence over a
line's cost rows, the (join, break) costs of its gaps and a bigram table with the optional DEL and INS moves, the backtrack with its
blanks, the gap costs from the geometry, and an enumeration of every path (per row: dropped, read, or read with one character inserted
after it; per gap: join or break) for small alphabets.  The alphabet size is a parameter: the library's is 65, the boundary symbol
and the blank's label are E = n."""
import itertools

import numpy as np

INF = 1 << 20
MAX_ROWS = 1024
OFF = 255
SRC_INS, SRC_BREAK = 0x8000, 0x4000
LINE_FIELDS = ("cost", "n_chars", "n_breaks", "n_sub", "n_del", "n_ins")


def decode_line(C, G, B, ins=0, dele=0, n=65):
    """One line: rows C (m, n), gap pairs G (m, 2) (G[0] is ignored), table B (n + 1, n + 1).  Returns (record as a tuple in the
    order of LINE_FIELDS, labels, sources, word_of_row)."""
    C = np.asarray(C, np.int64).reshape(-1, n)
    G = np.asarray(G, np.int64).reshape(-1, 2)
    B = np.asarray(B, np.int64).reshape(n + 1, n + 1)
    m, E = len(C), n
    if m > MAX_ROWS:
        return (-1, 0, 0, 0, 0, 0), [], [], [-1] * m
    V = np.full(n + 1, INF, np.int64)
    V[E] = 0
    steps, brk = [], []
    for i in range(1, m + 1):
        come = -1                                             # the state the break in front of row i comes from (-1: a join)
        if i >= 2:
            J, K = int(G[i - 1, 0]), int(G[i - 1, 1])
            W = np.full(n + 1, INF, np.int64) if J == OFF else V + J
            if K != OFF:
                end = V + B[:, E]
                a = int(np.argmin(end))                       # (numpy: the first of equal minima)
                X = int(end[a]) + K
                if X < W[E]:
                    W[E] = X
                    come = a
            V = W
        brk.append(come)
        # the run step of str_er_word_decode
        cand = V[:, None] + B[:, :n]                          # [a, b]
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
        Vn = U.copy()
        if ins > 0:
            ci = U[:n, None] + B[:n, :n]                      # [b, c]
            I = ci.min(axis=0) + ins
            ins_pred[:n] = ci.argmin(axis=0)
            is_ins[:n] = I < U[:n]
            Vn[:n] = np.where(is_ins[:n], I, U[:n])
        steps.append((sub_pred, is_del, is_ins, ins_pred))
        V = Vn
    end = V + B[:, E]
    state = int(np.argmin(end))
    cost = int(end[state])
    assert cost < INF
    labels, src, word_of_row = [], [], [-1] * m
    n_sub = n_del = n_ins = n_brk = 0
    for i in range(m, 0, -1):
        sub_pred, is_del, is_ins, ins_pred = steps[i - 1]
        if is_ins[state]:
            labels.append(state); src.append((i - 1) | SRC_INS); n_ins += 1
            state = int(ins_pred[state])
        if is_del[state]:
            n_del += 1
        else:
            labels.append(state); src.append(i - 1); n_sub += 1
            word_of_row[i - 1] = n_brk                        # (the breaks behind it; turned round below)
            state = int(sub_pred[state])
        if state == E and brk[i - 1] >= 0:
            labels.append(E); src.append((i - 1) | SRC_BREAK); n_brk += 1
            state = brk[i - 1]
    assert state == E
    labels.reverse(); src.reverse()
    word_of_row = [n_brk - v if v >= 0 else -1 for v in word_of_row]
    return (cost, len(labels), n_brk, n_sub, n_del, n_ins), labels, src, word_of_row


def decode_lines(costs, gaps, first_row, n_of, B, ins=0, dele=0, n=65):
    """Every line: the records as tuples, chars (3 rows,) uint8, src (3 rows,) uint16 and word_of_row (rows,) int32, 0xFF / 0xFFFF / -1
    where nothing is written."""
    costs = np.asarray(costs, np.uint8).reshape(-1, n)
    gaps = np.asarray(gaps, np.uint8).reshape(-1, 2)
    recs = []
    chars = np.full(3 * len(costs), 0xFF, np.uint8)
    src = np.full(3 * len(costs), 0xFFFF, np.uint16)
    wor = np.full(len(costs), -1, np.int32)
    for f, k in zip(first_row, n_of):
        f, k = int(f), max(0, int(k))
        rec, lab, s, w = decode_line(costs[f:f + k], gaps[f:f + k], B, ins, dele, n)
        recs.append(rec)
        chars[3 * f:3 * f + len(lab)] = lab
        src[3 * f:3 * f + len(s)] = s
        wor[f:f + k] = w
    return recs, chars, src, wor


def path_cost(C, G, B, labels, src, ins, dele, n=65):
    """The cost of a returned string under the definition: every row is read once or dropped, inserted characters pay INS, a blank ends
    a word and pays the gap's K, every other gap its J."""
    C = np.asarray(C, np.int64).reshape(-1, n)
    G = np.asarray(G, np.int64).reshape(-1, 2)
    B = np.asarray(B, np.int64).reshape(n + 1, n + 1)
    prev, s, used, broken = n, 0, set(), set()
    for a, r in zip(labels, src):
        s += int(B[prev, a])
        if r & SRC_BREAK:
            s += int(G[r & 0x3FFF, 1]); broken.add(r & 0x3FFF)
        elif r & SRC_INS:
            s += ins
        else:
            s += int(C[r, a]); used.add(r)
        prev = a
    s += sum(int(G[i, 0]) for i in range(1, len(C)) if i not in broken)
    return s + int(B[prev, n]) + dele * (len(C) - len(used))


def enumerate_best(C, G, B, ins, dele, n):
    """The cheapest of every path, by brute force: per row one of DEL, SUB b, or either followed by INS c (only after some character);
    per gap a join (J on) or a break (K on)."""
    C = np.asarray(C, np.int64).reshape(-1, n)
    G = np.asarray(G, np.int64).reshape(-1, 2)
    B = np.asarray(B, np.int64).reshape(n + 1, n + 1)
    m = len(C)
    moves = ([("del",)] if dele > 0 else []) + [("sub", b) for b in range(n)]
    if ins > 0:
        moves += [("subins", b, c) for b in range(n) for c in range(n)]
        if dele > 0:
            moves += [("delins", c) for c in range(n)]
    best = None
    for gaps in itertools.product((0, 1), repeat=max(0, m - 1)):
        if any(int(G[i + 1, g]) == OFF for i, g in enumerate(gaps)):
            continue
        gsum = sum(int(G[i + 1, g]) for i, g in enumerate(gaps))
        for path in itertools.product(moves, repeat=m):
            prev, s, ok = n, gsum, True
            for i, mv in enumerate(path):
                if i >= 1 and gaps[i - 1] == 1:                # a break: the word ends on prev, the next begins at the boundary
                    s += int(B[prev, n]); prev = n
                if mv[0] == "del":
                    s += dele
                elif mv[0] == "sub":
                    s += int(B[prev, mv[1]]) + int(C[i, mv[1]]); prev = mv[1]
                elif mv[0] == "subins":
                    s += int(B[prev, mv[1]]) + int(C[i, mv[1]]) + int(B[mv[1], mv[2]]) + ins; prev = mv[2]
                else:
                    if prev == n:
                        ok = False
                        break
                    s += dele + int(B[prev, mv[1]]) + ins; prev = mv[1]
            if ok:
                s += int(B[prev, n])
                best = s if best is None or s < best else best
    return best


def gap_pair(g, colmax, num=1, den=3, w=16):
    """(J, K) of a gap of g columns (Python integers: exact)."""
    x = min(16, (8 * max(0, int(g)) * int(den)) // (int(num) * int(colmax)))
    return (w * x) // 8, (w * (16 - x)) // 8


def gap_costs(runs, first_row, n_of, colmax, num=1, den=3, w=16, row_run=None, n_rows=None):
    """(n_rows, 2) uint8 from runs as (x0, x1) pairs: (0, 255) for a line's first row, a row of the run of the row before it, and a
    row of no line."""
    n = n_rows if n_rows is not None else len(runs) if row_run is None else len(row_run)
    run_of = (lambda r: r) if row_run is None else (lambda r: int(row_run[r]))
    out = np.zeros((n, 2), np.uint8)
    out[:, 1] = OFF
    for t, (f, k) in enumerate(zip(first_row, n_of)):
        for r in range(int(f) + 1, int(f) + int(k)):
            p, q = run_of(r - 1), run_of(r)
            if p != q:
                out[r] = gap_pair(int(runs[q][0]) - int(runs[p][1]), colmax[t], num, den, w)
    return out


def as_tuples(recs) -> list:
    """The library's LINE_DECODE_DTYPE records as tuples in the order of LINE_FIELDS."""
    return [tuple(int(r[k]) for k in LINE_FIELDS) for r in recs]
