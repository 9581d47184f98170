"""A numpy statement of WordTracker.update with a decode pool (binding.py): the ids, joins and closings are WordTrackerRef's
(word_tracker_ref.py), taken by import; what an id holds is a kept list instead of a sum.  Every update with a word track takes the next
serial; a member's key is serial << 32 | its index in the result's word_track_members; joined ids pool their usable members and their
counts; the record of an id is S.decode_tracks_host on the `keep` largest keys in ascending order (decode_pool_ref.read_kept).  closed
holds (id, (record, labels)) where the lexicon's reference holds (id, record)."""
import numpy as np

import decode_pool_ref as DP
from word_tracker_ref import WordTrackerRef


class DecodeTrackerRef(WordTrackerRef):
    def __init__(self, S, table, keep, dec=(0, 0), ins=64, dele=64, rounds=8, num=1, den=2):
        super().__init__(None, num=num, den=den)
        self.S, self.table, self.keep, self.args = S, table, keep, (dec, ins, dele, rounds)
        self.serial, self.keyed, self.count = 0, {}, {}

    def _sync(self):
        """The joins since the last look: an id that is no root any more gives what it holds to its root."""
        for i in sorted(self.keyed):
            r = self.find(i)
            if r != i:
                self.keyed[r] += self.keyed.pop(i)
                self.count[r] += self.count.pop(i)

    def record(self, i):
        self._sync()
        r = self.find(i)
        kept = sorted(self.keyed[r], key=lambda m: m[0])[-self.keep:]
        rec, ch, _ = DP.read_kept(self.S, kept, self.count[r], self.keep, self.table, *self.args)
        return rec, tuple(int(a) for a in ch)

    def update(self, words, track_of, tracks, members, rows, *rest):
        costs, first, n_of = rows
        base = len(self.parent)
        if len(tracks):
            self.serial += 1
        for g, t in enumerate(tracks):
            at0, n = int(t["first"]), int(t["count"])
            self.count[base + g] = n
            self.keyed[base + g] = [(self.serial << 32 | at, np.asarray(costs[int(first[w]):int(first[w]) + int(n_of[w])], np.uint8).reshape(-1, 65))
                                    for at, w in zip(range(at0, at0 + n), members[at0:at0 + n]) if int(n_of[w]) <= 32]
        return super().update(words, track_of, tracks, members, rows, *rest)
