"""A numpy mirror of the lattice decode pool (the contract is at "The lattice decode pool" in str_er.h), written from the contract: the
keys serial << 32 | index in the call's member array, the kept list of a slot (the `keep` largest keys of everything usable ever added
or joined, N <= 32 nodes), its age order, and a member's evidence rebased into a cell of fixed strides -- 32 split records and run
rows, 80 piece rows, the pieces of its runs back to back in run order whatever their places in the call's piece table.  track() lays a
slot's kept list out as the one track of the defining property; check_slots() holds a pool read against
str_er_lattice_decode_tracks_host on it, and check_members() the evidence handed back against the mirror's, all with ==."""
import numpy as np

CELL_RUNS, CELL_PIECES, MAX_NODES = 32, 80, 32
FIELDS = ("cost", "seed_cost", "n_chars", "n_edits", "converged", "n_used", "seed_member", "lm_cost", "n_members", "n_kept")
MEMBER_FIELDS = ("cost", "first_part", "n_parts", "n_del", "n_ins", "word")
EMPTY = (-1, -1, 0, 0, 0, 0, -1, -1, 0, 0)
RUN_SPLIT_DTYPE = np.dtype([("n_cuts", "<i4"), ("cut", "<i4", (3,)), ("thr", "<u4"), ("first_piece", "<i4"), ("n_pieces", "<i4"), ("n_parts", "<i4")])          # str_er_run_split


def as_tuples(recs) -> list:
    return [tuple(int(r[k]) for k in FIELDS) for r in recs]


class Member:
    def __init__(self, key, splits, run_rows, piece_rows):
        """splits: the records of the member's runs as they came; the rows of the call."""
        self.key, self.n_runs = int(key), len(splits)
        self.splits = np.zeros(CELL_RUNS, RUN_SPLIT_DTYPE)
        self.run_rows = np.zeros((CELL_RUNS, 65), np.uint8)
        self.piece_rows = np.zeros((CELL_PIECES, 65), np.uint8)
        self.splits[:len(splits)] = splits
        self.run_rows[:len(splits)] = run_rows
        base = 0
        for t, s in enumerate(splits):
            n = int(s["n_pieces"])
            self.piece_rows[base:base + n] = piece_rows[int(s["first_piece"]):int(s["first_piece"]) + n]
            self.splits["first_piece"][t] = base
            base += n
        self.n_pieces = base
        assert base <= 72


class Mirror:
    def __init__(self, cap: int, keep: int):
        self.cap, self.keep, self.serial = cap, keep, 0
        self.kept = [[] for _ in range(cap)]          # per slot, ascending keys
        self.n_members = [0] * cap

    def _merge(self, slot, incoming):
        u = sorted(self.kept[slot] + incoming, key=lambda m: m.key)
        self.kept[slot] = u[-self.keep:]

    def add(self, splits, run_costs, piece_costs, first_run, n_of, track_first, track_count, members, slots):
        if len(track_first) == 0:
            return
        self.serial += 1
        run_costs, piece_costs = np.asarray(run_costs).reshape(-1, 65), np.asarray(piece_costs).reshape(-1, 65)
        for g, slot in enumerate(slots):
            usable = []
            for j in range(int(track_count[g])):
                at = int(track_first[g]) + j
                w = int(members[at])
                f, m = int(first_run[w]), int(n_of[w])
                if int((splits["n_cuts"][f:f + m] + 1).sum()) <= MAX_NODES:
                    usable.append((at, f, m))
            # (the keys of a call ascend with the index: only its newest `keep` can be kept)
            incoming = [Member(self.serial << 32 | at, splits[f:f + m], run_costs[f:f + m], piece_costs) for at, f, m in usable[-self.keep:]]
            self._merge(slot, incoming)
            self.n_members[slot] += int(track_count[g])

    def clear(self, slots):
        for s in slots:
            self.kept[s], self.n_members[s] = [], 0

    def join(self, dst, srcs):
        for s in srcs:
            self._merge(dst, self.kept[s])
            self.n_members[dst] += self.n_members[s]
            self.clear([s])

    def reset(self):
        self.clear(range(self.cap))
        self.serial = 0

    def track(self, slot):
        """The kept list as one track for lattice_decode_tracks_host: word i at the runs 32 * i and the piece rows 80 * i."""
        kept = self.kept[slot]
        n = len(kept)
        sp = np.zeros(n * CELL_RUNS, RUN_SPLIT_DTYPE)
        rr, pr = np.zeros((n * CELL_RUNS, 65), np.uint8), np.zeros((n * CELL_PIECES, 65), np.uint8)
        for i, m in enumerate(kept):
            sp[i * CELL_RUNS:(i + 1) * CELL_RUNS] = m.splits
            sp["first_piece"][i * CELL_RUNS:(i + 1) * CELL_RUNS] += i * CELL_PIECES
            rr[i * CELL_RUNS:(i + 1) * CELL_RUNS] = m.run_rows
            pr[i * CELL_PIECES:(i + 1) * CELL_PIECES] = m.piece_rows
        first = np.arange(n, dtype=np.int32) * CELL_RUNS
        n_of = np.array([m.n_runs for m in kept], np.int32)
        return sp, rr, pr, first, n_of, np.zeros(1, np.int32), np.array([n], np.int32), np.arange(n, dtype=np.int32)


def check_slots(S, pool, mirror, slots, B, dec=(0, 0), ins=64, dele=64, rounds=8, split=8):
    """read_lattice(slots) against lattice_decode_tracks_host on the mirror's kept lists; read() must give the same triple.  Returns
    what read_lattice gave."""
    got = pool.read_lattice(slots)
    rec, ch, mc, mrec, src, parts = got
    plain = pool.read(slots)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, got[:3]))
    assert rec.shape == (len(slots),) and ch.shape == (len(slots), 32) and mc.shape == (len(slots), mirror.keep)
    at = 0
    for i, slot in enumerate(slots):
        n = len(mirror.kept[slot])
        host, hch, hm, hsrc, hparts = S.lattice_decode_tracks_host(*mirror.track(slot), B, dec[0], dec[1], ins, dele, rounds, split)
        want = tuple(int(host[0][k]) for k in FIELDS[:8]) + (mirror.n_members[slot], n)
        assert as_tuples(rec[i:i + 1])[0] == want, (slot, as_tuples(rec[i:i + 1])[0], want)
        assert ch[i].tobytes() == hch[0].tobytes(), slot
        assert mc[i][:n].tolist() == [int(c) for c in hm["cost"]] and (mc[i][n:] == -1).all(), slot
        g = mrec[i][:n].copy()
        g["first_part"] -= at
        assert g.tobytes() == hm.tobytes(), (slot, g, hm)
        assert src[i][:n].tobytes() == hsrc.tobytes() and (src[i][n:] == 255).all(), slot
        k = int(hm["n_parts"].sum())
        assert parts[at:at + k].tobytes() == hparts.tobytes(), (slot, parts[at:at + k], hparts)
        at += k
        rest = mrec[i][n:]
        assert (rest["cost"] == -1).all() and (rest["word"] == -1).all() and (rest["n_parts"] == 0).all() and (rest["first_part"] == at).all()
        if n == 0:
            assert want[:8] == EMPTY[:8]
    assert at == len(parts)
    return got


def check_members(pool, mirror, slot):
    """members(slot) against the mirror, byte for byte; returns the keys."""
    keys, nr, sp, rr, pr = pool.members(slot)
    kept = mirror.kept[slot]
    assert keys.tolist() == [m.key for m in kept] and nr.tolist() == [m.n_runs for m in kept]
    for i, m in enumerate(kept):
        assert sp[i].tobytes() == m.splits.tobytes(), (slot, i)
        assert rr[i].tobytes() == m.run_rows.tobytes() and pr[i].tobytes() == m.piece_rows.tobytes(), (slot, i)
    return keys.tolist()


def snapshot(pool, slots) -> bytes:
    """Everything a caller can see of the slots: read_lattice and members."""
    out = b"".join(a.tobytes() for a in pool.read_lattice(slots))
    for s in slots:
        out += b"".join(a.tobytes() for a in pool.members(s))
    return out
