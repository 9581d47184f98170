"""The numpy reference of the joint decode of a line over its runs' piece lattices (line_lattice_ref.py, written from the definition at
str_er_line_lattice_decode) against an enumeration of every segmentation, break / join choice, string and choice of moves on alphabets
of 2 and 3 characters, the five identities of the contract against the references of its parents (line_decode_ref.py,
lattice_decode_ref.py, run_split_ref.py), the bound of the recurrence, and the pure host entry point against the reference, every
value with ==."""
import itertools

import numpy as np
import pytest

import lattice_decode_ref as LR
import line_decode_ref as LN
import line_lattice_ref as LL
import run_split_ref as RS

MOVES = ((0, 0), (64, 0), (0, 64), (64, 64))          # (INS, DEL) at the library's alphabet: off, each move alone, both
KINDS = ("i1", "i2", "i3", "break", "break_from_E", "del", "ins", "tie_split", "tie_gap")


def scaled(moves, hi):
    """The moves at a table whose entries lie below hi: 64 is a quarter of 256."""
    return tuple(v * hi // 256 for v in moves)


def first_pieces(cuts):
    fp, at = [], 0
    for k in cuts:
        fp.append(at)
        at += LR.n_pieces(k)
    return fp, at


def random_line(rng, cuts, n, hi):
    """Rows of a line whose runs have the given cut counts: (first_piece, run rows, piece rows, gap pairs)."""
    fp, at = first_pieces(cuts)
    G = rng.integers(0, min(hi, 255), (len(cuts), 2))
    off = rng.integers(0, 6, len(cuts))
    G[off == 0, 0] = 255
    G[off == 1, 1] = 255
    return fp, rng.integers(0, hi, (len(cuts), n)), rng.integers(0, hi, (at, n)), G


def tie_gap_line(rng, cuts, n, hi):
    """A line that is dropped whole under DEL = hi / 4, with J = K at every gap and B[E][E] = 0: at every gap join and break tie."""
    fp, at = first_pieces(cuts)
    B = rng.integers(0, hi, (n + 1, n + 1))
    B[n, n] = 0
    g = rng.integers(0, min(hi, 255), len(cuts))
    return fp, np.full((len(cuts), n), hi - 1), np.full((at, n), hi - 1), np.stack([g, g], axis=1), B


SHAPES = [()] + [c for R in (1, 2) for c in itertools.product(range(3), repeat=R)] + [(0, 0, 0), (1, 0, 2), (2, 1, 0), (0, 2, 1), (1, 1, 1)]


@pytest.mark.parametrize("n", (2, 3))
@pytest.mark.parametrize("moves", MOVES)
def test_reference_equals_the_enumeration_of_every_path(n, moves):
    """Lines of up to 3 runs of up to 3 atoms; the three-run lines on the alphabet of 2 (the enumeration grows with moves ^ atoms)."""
    rng = np.random.default_rng(400 + n + moves[0] + 3 * moves[1])
    stats, cases = {}, 0
    for cuts in SHAPES:
        if n == 3 and (len(cuts) > 2 or sum(cuts) > 3):
            continue
        for rep in range(12 if len(cuts) < 3 else 6):
            hi = (4, 16, 256)[rep % 3]                              # small ranges tie often
            split = (0, hi // 32, 255 * hi // 256)[(rep + len(cuts)) % 3]
            ins, dele = scaled(moves, hi)
            fp, runs, pieces, G = random_line(rng, cuts, n, hi)
            B = rng.integers(0, hi, (n + 1, n + 1))
            rec, lab, src, parts, wop = LL.decode_line(cuts, fp, runs, pieces, G, B, ins, dele, split, 0, n, stats)
            assert rec[0] == LL.enumerate_best(cuts, fp, runs, pieces, G, B, ins, dele, split, n), (cuts, ins, dele, split, runs, pieces, G, B)
            assert rec[0] == LL.path_cost(LR.Word(cuts, fp, runs, pieces, 0, n), G, B, lab, src, parts, ins, dele, split, n)
            N = sum(k + 1 for k in cuts)
            assert rec[3] + rec[5] + rec[2] == rec[1] == len(lab) <= max(0, 3 * N - 1) and rec[3] + rec[4] == rec[6] == len(parts) == len(wop)
            assert len(cuts) <= rec[6] <= N and lab.count(n) == rec[2] and (ins > 0 or rec[5] == 0) and (dele > 0 or rec[4] == 0)
            assert [w for w in wop if w >= 0] == sorted(w for w in wop if w >= 0) and wop.count(-1) == rec[4] and max(wop, default=0) <= rec[2]
            cases += 1
    assert cases >= 30
    # a join that costs what the break costs is met at E alone, and a later node is at E only behind DEL: rows too dear to read
    for cuts in ((0, 0), (1, 2), (0, 1, 0)) if moves[1] else ():
        fp, runs, pieces, G, B = tie_gap_line(rng, cuts, n, 4)
        ins, dele = scaled(moves, 4)
        rec, lab, src, parts, wop = LL.decode_line(cuts, fp, runs, pieces, G, B, ins, dele, 0, 0, n, stats)
        assert rec[0] == LL.enumerate_best(cuts, fp, runs, pieces, G, B, ins, dele, 0, n) and rec[2] == 0          # (on a tie the join stays)
    assert stats["i1"] >= 1 and stats["break"] >= 1 and stats.get("tie_split", 0) >= 1          # (ties included)
    assert stats.get("tie_gap", 0) >= (1 if moves[1] else 0)


def big_line(rng, R, cuts=None, hi=256, cheap=0.1):
    """A line of R runs at the library's alphabet: a few cheap characters per row among dear ones."""
    cuts = [int(k) for k in rng.integers(0, 4, R)] if cuts is None else list(cuts)
    fp, at = first_pieces(cuts)
    rows = lambda m: np.where(rng.random((m, 65)) < cheap, rng.integers(0, 24, (m, 65)), rng.integers(60, 256, (m, 65))).astype(np.uint8)
    G = rng.integers(0, 255, (R, 2))
    off = rng.integers(0, 6, R)
    G[off == 0, 0] = 255
    G[off == 1, 1] = 255
    return cuts, fp, rows(R), rows(at), G


def test_the_ground_is_really_covered():
    """The random lines the device comparison stands on hold every kind of step at least once: parts from the local nodes 1, 2 and 3,
    breaks, a break from E (an empty word), DEL, INS, and both ties.  The ties come from small tables, the break from E from a table
    that makes the boundary cheap to repeat."""
    rng = np.random.default_rng(410)
    stats = {}
    for t in range(60):
        cuts, fp, runs, pieces, G = big_line(rng, int(rng.integers(1, 12)))
        hi = (6, 256)[t % 2]
        LL.decode_line(cuts, fp, runs, pieces, G, rng.integers(0, hi, (66, 66)), 20, 30, (0, 8)[t % 2], 0, 65, stats)
    for t in range(60):                                      # small values everywhere: equal costs are common
        cuts, fp, runs, pieces, G = big_line(rng, int(rng.integers(2, 8)))
        LL.decode_line(cuts, fp, runs // 64, pieces // 64, G // 64, rng.integers(0, 3, (66, 66)), 1, 1, 0, 0, 65, stats)
    for cuts in ((0, 0), (3, 1, 2)):                         # (a join that ties with the break is met behind DEL alone: made cheap)
        fp, runs, pieces, G, B = tie_gap_line(rng, cuts, 65, 256)
        assert LL.decode_line(cuts, fp, runs, pieces, G, B, 20, 64, 8, 0, 65, stats)[0][2] == 0
    for kind in KINDS:
        assert stats.get(kind, 0) >= 1, (kind, stats)


@pytest.mark.parametrize("ins,dele", MOVES)
def test_identity_1_without_cuts_it_is_the_line_decoder(ins, dele):
    rng = np.random.default_rng(420 + ins + 7 * dele)
    for R in (0, 1, 2, 7, 40):
        for hi in (6, 256):
            cuts, fp, runs, pieces, G = big_line(rng, R, [0] * R)
            B = rng.integers(0, hi, (66, 66))
            rec, lab, src, parts, wop = LL.decode_line(cuts, fp, runs, pieces, G, B, ins, dele, 8)
            want, wlab, wsrc, wwor = LN.decode_line(runs, G, B, ins, dele)
            assert rec[:6] == want and lab == wlab and src == wsrc and wop == wwor and parts == [(r, -1) for r in range(R)]


def lattice_words(cuts, fp, runs, pieces, lengths, B, ins, dele, split):
    """(the sum of the words' lattice decode costs, their labels joined by one blank, their parts, their counts summed)."""
    at, total, labels, parts, counts = 0, 0, [], [], np.zeros(4, np.int64)
    for w, k in enumerate(lengths):
        rec, lab, src, pt = LR.decode_word(cuts[at:at + k], fp[at:at + k], runs, pieces, B, ins, dele, split, at)
        assert rec[0] >= 0
        total += rec[0]
        labels += ([65] if w else []) + lab
        parts += pt
        counts += [rec[3], rec[4], rec[5], rec[6]]
        at += k
    return total, labels, parts, counts.tolist()


@pytest.mark.parametrize("ins,dele", MOVES)
def test_identities_2_and_3_against_the_lattice_decoder(ins, dele):
    rng = np.random.default_rng(430 + ins + 7 * dele)
    for rep in range(10):
        lengths = [int(k) for k in rng.integers(1, 6, int(rng.integers(1, 5)))]
        R, split = sum(lengths), (0, 8, 255)[rep % 3]
        cuts, fp, runs, pieces, G = big_line(rng, R)
        B = rng.integers(0, (6, 64, 256)[rep % 3], (66, 66))             # (B[E][E] != 0 almost always)
        # (2) joins alone: the word of all runs (5 runs of 4 atoms at the most here: inside the lattice decoder's 32)
        k = min(R, 5)
        rec, lab, src, parts, wop = LL.decode_line(cuts[:k], fp[:k], runs, pieces, np.tile([0, 255], (R, 1)), B, ins, dele, split)
        wrec, wlab, wsrc, wparts = LR.decode_word(cuts[:k], fp[:k], runs, pieces, B, ins, dele, split)
        assert (rec[0], rec[1], rec[3], rec[4], rec[5], rec[6]) == (wrec[0],) + wrec[2:] and rec[2] == 0
        assert lab == wlab and parts == wparts and src == [(s & 0x7F) | (0x8000 if s & 0x80 else 0) for s in wsrc]
        # (3) a segmentation forced by its gaps, every word gap at a cost of its own
        ks = rng.integers(0, 255, R)
        starts = set(np.cumsum(lengths)[:-1].tolist())
        Gs = np.array([(255, int(ks[r])) if r in starts else (0, 255) for r in range(R)])
        total, labels, wparts, counts = lattice_words(cuts, fp, runs, pieces, lengths, B, ins, dele, split)
        rec, lab, src, parts, wop = LL.decode_line(cuts, fp, runs, pieces, Gs, B, ins, dele, split)
        assert rec[0] == total + sum(int(ks[r]) for r in starts) and lab == labels and parts == wparts and rec[2] == len(lengths) - 1
        assert [rec[3], rec[4], rec[5], rec[6]] == counts


def split_sequence(cuts, fp, runs, pieces, split):
    """The parts of str_er_run_split on the same runs (run_split_ref.py): (their rows, the run of every part)."""
    splits = [(k, -1, -1, -1, 0, f, LR.n_pieces(k), 0) for k, f in zip(cuts, fp)]
    words, parts, rows = RS.split_words(splits, runs, pieces, [0], [len(cuts)], split)
    return rows.astype(np.int64), [p[0] for p in parts]


def test_identities_4_and_5_against_the_line_decoder():
    rng = np.random.default_rng(440)
    seen_cut = seen_less = 0
    for t in range(80):
        ins, dele = MOVES[t % 4]
        split = (0, 8, 255)[t % 3]
        cuts, fp, runs, pieces, G = big_line(rng, int(rng.integers(0, 10)))
        G = rng.integers(0, 255, G.shape)                             # both moves on
        B = rng.integers(0, (6, 256)[t % 2], (66, 66))
        rec, lab, src, parts, wop = LL.decode_line(cuts, fp, runs, pieces, G, B, ins, dele, split)
        assert rec[0] == LL.path_cost(LR.Word(cuts, fp, runs, pieces), G, B, lab, src, parts, ins, dele, split)
        whole = LN.decode_line(runs, G, B, ins, dele)[0]
        assert rec[0] <= whole[0]                                     # (4)
        rows, run_of = split_sequence(cuts, fp, runs, pieces, split)
        Gp = np.array([(0, 255) if k and run_of[k] == run_of[k - 1] else tuple(G[run_of[k]]) for k in range(len(rows))]).reshape(-1, 2)
        seq = LN.decode_line(rows, Gp, B, ins, dele)[0]
        assert rec[0] <= seq[0] + split * (len(rows) - len(cuts))     # (5)
        seen_cut += any(cuts)
        seen_less += rec[0] < whole[0]
    assert seen_cut >= 40 and seen_less >= 10


def test_not_decoded_past_1024_runs_and_the_bound_at_1024_runs_of_four_atoms():
    R = 1024
    cuts = [3] * R
    fp, at = first_pieces(cuts)
    runs, pieces, B = np.full((R, 65), 255, np.uint8), np.full((at, 65), 255, np.uint8), np.full((66, 66), 255, np.uint8)
    G = np.full((R, 2), 254, np.uint8)
    rec, lab, src, parts, wop = LL.decode_line(cuts + [0], fp + [at], np.full((R + 1, 65), 255, np.uint8), pieces, np.full((R + 1, 2), 254, np.uint8), B)
    assert rec == (-1, 0, 0, 0, 0, 0, 0) and lab == [] and parts == [] and wop == []
    rec, lab, src, parts, wop = LL.decode_line(cuts, fp, runs, pieces, G, B, 0, 0, 255)
    assert rec[0] == 510 + (255 + 255 + 254) * 1023 + 255 < 1043202 < LL.INF and rec[2] == 0 and rec[6] == R      # (every run whole, a join at every gap)
    G[:, 0] = 255
    rec, lab, src, parts, wop = LL.decode_line(cuts, fp, runs, pieces, G, B, 0, 0, 255)                              # (the reference asserts every value < 2^25)
    assert rec[0] == 1043202 and rec[2] == 1023 and rec[1] == 2047 and parts == [(r, -1) for r in range(R)]


# ---- the host entry point -----------------------------------------------------------------------------------------------------------

def make_call(S, rng, n_of, cuts=None, gap_rows=2, hi=256, cheap=0.1):
    """A call of str_er_lattice_decode_lines: lines of n_of runs each, gap_rows runs of no line in front of every line but the first.
    Returns (splits, run rows, piece rows, gaps, first_run, n_of)."""
    first, at = [], 0
    for t, k in enumerate(n_of):
        at += gap_rows if t else 0
        first.append(at)
        at += int(k)
    R = at + 1                                                     # (and one run of no line behind the last)
    cs, fp, runs, pieces, G = big_line(rng, R, cuts, hi, cheap)
    splits = np.zeros(R, S.RUN_SPLIT_DTYPE)
    splits["n_cuts"], splits["first_piece"], splits["n_pieces"] = cs, fp, [LR.n_pieces(k) for k in cs]
    splits["cut"] = -1
    return splits, runs, pieces, G.astype(np.uint8), np.array(first, np.int32), np.array(n_of, np.int32)


def check_tables(S, got, call, B, ins, dele, split, stats=None):
    """What an entry point returned against the reference, every table with ==."""
    dec, chars, src, parts, wop = got
    want = LL.decode_lines(*call, B, ins, dele, split, 65, stats)
    assert dec.dtype == S.LINE_LATTICE_DECODE_DTYPE and chars.dtype == np.uint8 and src.dtype == np.uint16 and parts.dtype == S.SPLIT_PART_DTYPE and wop.dtype == np.int32
    assert LL.as_tuples(dec) == want[0]
    assert chars.shape == want[1].shape and (chars == want[1]).all() and (src == want[2]).all()
    assert [(int(p["run"]), int(p["piece"])) for p in parts] == [tuple(p) for p in want[3].tolist()] and wop.tolist() == want[4].tolist()
    return want


@pytest.mark.parametrize("ins,dele", MOVES)
def test_lattice_decode_lines_host_equals_the_reference(S, ins, dele):
    rng = np.random.default_rng(450 + ins + 7 * dele)
    call = make_call(S, rng, [0, 1, 2, 31, 33, 64, 65] + list(rng.integers(0, 13, 6)))
    for hi, split in ((6, 0), (256, 8)):
        B =rng.integers(0, hi, (66, 66)).astype(np.uint8)
        want = check_tables(S, S.lattice_decode_lines_host(*call, B, ins, dele, split), call, B, ins, dele, split)
    slot = S.line_lattice_node_slots(call[0], call[4])
    assert (slot == LL.node_slots(call[0])[call[4]]).all()
    assert (want[1][3 * int(slot[1]) - 6:3 * int(slot[1])] == 0xFF).all()          # (the runs of no line in front of the second line)


def test_lattice_decode_lines_host_at_the_run_limit_and_on_no_line(S):
    rng = np.random.default_rng(460)
    call = make_call(S, rng, [1023, 1024, 1025], gap_rows=0)
    B = rng.integers(0, 6, (66, 66)).astype(np.uint8)
    want = check_tables(S, S.lattice_decode_lines_host(*call, B, 20, 30, 8), call, B, 20, 30, 8)
    assert want[0][2] == (-1, 0, 0, 0, 0, 0, want[0][2][6], 0) and want[0][1][0] >= 0
    dec, chars, src, parts, wop = S.lattice_decode_lines_host(*call[:4], [], [], B)
    assert dec.shape == (0,) and (chars == 0xFF).all() and (src == 0xFFFF).all() and len(parts) == 0 and len(wop) == 0
    empty = S.lattice_decode_lines_host(np.zeros(0, S.RUN_SPLIT_DTYPE), np.zeros((0, 65), np.uint8), np.zeros((0, 65), np.uint8), np.zeros((0, 2), np.uint8), [0], [0], B)
    assert LL.as_tuples(empty[0]) == [(int(B[65, 65]), 0, 0, 0, 0, 0, 0, 0)] and len(empty[1]) == 0
