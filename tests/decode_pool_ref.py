"""A numpy statement of the decode pool's bookkeeping (str_er_pool_decode): the serials and keys of the additions, everything usable
a slot was ever given, and the kept list as the definition states it -- the `keep` largest keys, ascending.  The reading of a kept list
is S.decode_tracks_host on it as one track whose words are numbered in that order; nothing here is computed by the pool.  No GPU."""
import numpy as np

EMPTY = (-1, -1, 0, 0, 0, 0, -1, -1, 0, 0)
FIELDS = ("cost", "seed_cost", "n_chars", "n_edits", "converged", "n_used", "seed_member", "lm_cost", "n_members", "n_kept")


def as_tuples(recs):
    return [tuple(int(r[k]) for k in FIELDS) for r in recs]


class Mirror:
    def __init__(self, cap, keep):
        self.cap, self.keep = cap, keep
        self.reset()

    def reset(self):
        self.serial = 0
        self.all = [[] for _ in range(self.cap)]          # per slot: (key, rows (m, 65)) of every usable member ever given
        self.n_members = [0] * self.cap

    def add(self, costs, first, n_of, tf, tc, members, slots):
        if len(slots) == 0:
            return
        self.serial += 1
        costs = np.asarray(costs, np.uint8).reshape(-1, 65)
        for g, s in enumerate(slots):
            for j in range(int(tc[g])):
                at = int(tf[g]) + j
                w = int(members[at])
                self.n_members[s] += 1
                if int(n_of[w]) <= 32:
                    self.all[s].append((self.serial << 32 | at, costs[int(first[w]):int(first[w]) + int(n_of[w])].copy()))

    def join(self, dst, srcs):
        for s in srcs:
            self.all[dst] += self.all[s]
            self.n_members[dst] += self.n_members[s]
            self.clear([s])

    def clear(self, slots):
        for s in slots:
            self.all[s], self.n_members[s] = [], 0

    def kept(self, slot):
        """[(key, rows)] of the slot's kept list in age order."""
        return sorted(self.all[slot], key=lambda m: m[0])[-self.keep:]

    def read(self, S, slot, B, dec=(0, 0), ins=64, dele=64, rounds=8):
        """(record as a tuple of FIELDS, 32 labels, keep member costs) of a slot, by the host entry point on its kept list."""
        return read_kept(S, self.kept(slot), self.n_members[slot], self.keep, B, dec, ins, dele, rounds)


def read_kept(S, kept, n_members, keep, B, dec=(0, 0), ins=64, dele=64, rounds=8):
    """The reading of a kept list [(key, rows)] in age order: S.decode_tracks_host on one track of its members, numbered in that order."""
    rows = [r for _, r in kept]
    n_of = np.array([len(r) for r in rows], np.int32)
    first = np.concatenate([[0], np.cumsum(n_of)[:-1]]).astype(np.int32) if len(rows) else np.zeros(0, np.int32)
    costs = np.concatenate(rows + [np.zeros((0, 65), np.uint8)])
    rec, ch, mc = S.decode_tracks_host(costs, first, n_of, [0], [len(rows)], np.arange(len(rows), dtype=np.int32), B, dec[0], dec[1], ins, dele, rounds)
    out = np.full(keep, -1, np.int32)
    out[:len(rows)] = mc
    return tuple(int(rec[0][k]) for k in FIELDS[:8]) + (n_members, len(rows)), ch[0].copy(), out


def check_slots(S, pool, mirror, slots, B, dec=(0, 0), ins=64, dele=64, rounds=8):
    """One read of `slots` against the mirror, every field, label and cost with ==; returns what the pool gave."""
    rec, ch, mc = pool.read(slots)
    assert rec.dtype == S.POOL_DECODE_DTYPE and ch.shape == (len(slots), 32) and mc.shape == (len(slots), pool.keep)
    got = as_tuples(rec)
    memo = {}
    for i, s in enumerate(slots):
        if s not in memo:
            memo[s] = mirror.read(S, s, B, dec, ins, dele, rounds)
        want, wch, wmc = memo[s]
        assert got[i] == want, (i, s, got[i], want)
        assert ch[i].tolist() == wch.tolist() and mc[i].tolist() == wmc.tolist(), (i, s)
    return rec, ch, mc


def check_members(pool, mirror, slot):
    """members(slot) against the mirror's kept list: keys, run counts, and the rows up to every member's run count."""
    keys, n_runs, rows = pool.members(slot)
    kept = mirror.kept(slot)
    assert keys.tolist() == [k for k, _ in kept] and n_runs.tolist() == [len(r) for _, r in kept]
    assert rows.shape == (len(kept), 32, 65)
    for i, (_, r) in enumerate(kept):
        assert (rows[i, :len(r)] == r).all(), (slot, i)
    return keys
