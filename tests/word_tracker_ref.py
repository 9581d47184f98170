"""A numpy statement of WordTracker.update (binding.py), written from its rules on top of track_read_ref.py: every word track of a
result gets a fresh id; across the boundary between two results whose last and first frame have equal sizes, an eligible word u of the
one and an eligible word v of the other on lines of one persistent text id are linked iff their boxes share pixels and inter * den >=
num * (area(u) + area(v) - inter); linked ids are joined and the smaller id stays; a track without a member in the result's last frame is
closed with its final record.  The record of an id is the track match (track_read_ref.match_track) on the rows of all members it ever got,
with the member count in the eighth place.  The persistent text ids come from the caller (TextTracker has its own tests)."""
import numpy as np

import track_read_ref as TR


class WordTrackerRef:
    def __init__(self, lex, ins=64, dele=64, band=2, num=1, den=2):
        self.lex, self.prm, self.link = lex, (ins, dele, band), (num, den)
        self.parent, self.rows, self.live, self.closed, self.prev = [], {}, set(), [], None

    def find(self, i):
        while self.parent[i] != i:
            i = self.parent[i]
        return i

    def record(self, i):
        rows = self.rows[self.find(i)]
        n_of = [len(C) for C in rows]
        first = np.concatenate([[0], np.cumsum(n_of)[:-1]]).astype(int) if rows else []
        costs = np.concatenate(rows) if rows else np.zeros((0, 65), np.uint8)
        rec, _ = TR.match_track(costs, first, n_of, list(range(len(rows))), self.lex, *self.prm)
        return tuple(rec[:7]) + (len(rows),)

    def update(self, words, track_of, tracks, members, rows, first_lines, last_lines, first_wh, last_wh, text_ids, resolve_text):
        """words: LINE_WORD records; track_of, tracks, members: the result's word tracks; rows: (costs, first, n) the track match read;
        first_lines / last_lines: the lines of the result's first and last frame and first_wh / last_wh those frames' sizes; text_ids:
        the persistent text id of every line; resolve_text: ids -> their current ids.  Returns one id per word, -1 where not eligible."""
        costs, first, n_of = rows
        base = len(self.parent)
        for g, t in enumerate(tracks):
            self.parent.append(base + g)
            self.rows[base + g] = [np.asarray(costs[int(first[w]):int(first[w]) + int(n_of[w])], np.uint8).reshape(-1, 65)
                                   for w in members[int(t["first"]):int(t["first"]) + int(t["count"])]]
            self.live.add(base + g)
        box = lambda w: tuple(int(words[w][k]) for k in ("x", "y", "w", "h"))
        in_frame = lambda lines: [w for w in range(len(words)) if track_of[w] >= 0 and int(words[w]["line"]) in set(int(t) for t in lines)]
        if self.prev is not None and self.prev[0] == tuple(first_wh):
            num, den = self.link
            for ub, ut, ui in self.prev[1]:
                for v in in_frame(first_lines):
                    if int(resolve_text([ut])[0]) != int(resolve_text([text_ids[int(words[v]["line"])]])[0]):
                        continue
                    vb = box(v)
                    iw = min(ub[0] + ub[2], vb[0] + vb[2]) - max(ub[0], vb[0])
                    ih = min(ub[1] + ub[3], vb[1] + vb[3]) - max(ub[1], vb[1])
                    inter = iw * ih if iw > 0 and ih > 0 else 0
                    if inter > 0 and inter * den >= num * (ub[2] * ub[3] + vb[2] * vb[3] - inter):
                        i, j = self.find(ui), self.find(base + int(track_of[v]))
                        if i != j:
                            lo, hi = min(i, j), max(i, j)
                            self.parent[hi] = lo
                            self.rows[lo] += self.rows.pop(hi)
                            self.live.discard(hi)
        ids = np.array([self.find(base + int(t)) if t >= 0 else -1 for t in track_of], np.int64)
        ends = in_frame(last_lines)
        still = {int(ids[w]) for w in ends}
        for i in sorted(self.live - still):
            self.closed.append((i, self.record(i)))
            self.live.discard(i)
        self.prev = (tuple(last_wh), [(box(w), int(text_ids[int(words[w]["line"])]), int(ids[w])) for w in ends])
        return ids
