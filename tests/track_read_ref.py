"""A numpy reference of the word tracks and the track match (str_er_word_link in include/str_er.h), written from the contract alone on
top of word_match_ref.py: the reading lines, the word links, the word tracks as connected components and the match of a track over
the summed costs of its members."""
import numpy as np

import word_match_ref as WM

TRACK_FIELDS = WM.MATCH_FIELDS + ("n_used", "best_member")
LINE_WORD = np.dtype([("line", "<i4"), ("first_run", "<i4"), ("n_runs", "<i4"), ("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"), ("pixels", "<u4")])


def make_words(rows) -> np.ndarray:
    """rows of (line, x, y, w, h, pixels) -> a word table."""
    out = np.zeros(len(rows), LINE_WORD)
    for i, (line, x, y, w, h, px) in enumerate(rows):
        out[i] = (line, 0, 0, x, y, w, h, px)
    return out


def reading_lines(pixels, frames_of_lines, line_tracks) -> np.ndarray:
    """1 per line that is R(k, f): the member line of track k in frame f with the most pixels, ties to the smallest index."""
    n = len(pixels)
    reading = np.zeros(n, np.uint8)
    best = {}
    for t in range(n):
        key = (int(line_tracks[t]), int(frames_of_lines[t]))
        if key not in best or int(pixels[t]) > int(pixels[best[key]]):
            best[key] = t
    for t in best.values():
        reading[t] = 1
    return reading


def box_inter(u, v) -> int:
    w = min(int(u["x"]) + int(u["w"]), int(v["x"]) + int(v["w"])) - max(int(u["x"]), int(v["x"]))
    h = min(int(u["y"]) + int(u["h"]), int(v["y"]) + int(v["h"])) - max(int(u["y"]), int(v["y"]))
    return w * h if w > 0 and h > 0 else 0


def word_links(pixels, frames_of_lines, line_tracks, frame_wh, words, num=1, den=2):
    """(reading, [(a, b, inter, link)] sorted by (a, b))."""
    reading = reading_lines(pixels, frames_of_lines, line_tracks)
    frame_wh = np.asarray(frame_wh).reshape(-1, 2)
    out = []
    elig = [(i, w) for i, w in enumerate(words) if reading[int(w["line"])]]
    for a, u in elig:
        for b, v in elig:
            lu, lv = int(u["line"]), int(v["line"])
            fu, fv = int(frames_of_lines[lu]), int(frames_of_lines[lv])
            if not (reading[lu] and reading[lv]) or int(line_tracks[lu]) != int(line_tracks[lv]) or fv != fu + 1:
                continue
            if tuple(frame_wh[fu]) != tuple(frame_wh[fv]):
                continue
            inter = box_inter(u, v)
            if inter > 0:
                au, av = int(u["w"]) * int(u["h"]), int(v["w"]) * int(v["h"])
                out.append((a, b, inter, 1 if inter * den >= num * (au + av - inter) else 0))
    return reading, sorted(out)


def word_tracks(frames_of_lines, line_tracks, reading, words, links):
    """(track_of_words, tracks as dicts of the fields of str_er_word_track, members)."""
    n = len(words)
    eligible = [bool(reading[int(w["line"])]) for w in words]
    comp = list(range(n))
    for a, b, _, link in links:          # the closure, naively: relabel until nothing changes
        if link:
            ca, cb = comp[a], comp[b]
            if ca != cb:
                comp = [min(ca, cb) if c in (ca, cb) else c for c in comp]
    groups = {}
    for w in range(n):
        if eligible[w]:
            groups.setdefault(comp[w], []).append(w)
    frame = lambda w: int(frames_of_lines[int(words[w]["line"])])
    order = sorted(groups.values(), key=lambda g: (min(frame(w) for w in g), min(g)))
    track_of = np.full(n, -1, np.int32)
    tracks, members = [], []
    for g, ws in enumerate(order):
        ws = sorted(ws)
        rep = min(ws, key=lambda w: (-int(words[w]["pixels"]), w))
        tracks.append(dict(first_frame=min(frame(w) for w in ws), last_frame=max(frame(w) for w in ws), first=len(members), count=len(ws), rep=rep,
                           text_track=int(line_tracks[int(words[ws[0]]["line"])])))
        members += ws
        track_of[ws] = g
    return track_of, tracks, np.array(members, np.int32)


def match_track(costs, first_run, n_of, members, lex: WM.Lexicon, ins=64, dele=64, band=2):
    """(the str_er_track_match of one track as a tuple in the order of TRACK_FIELDS, member_cost list)."""
    costs = np.asarray(costs, np.uint8).reshape(-1, 65)
    rows = [costs[int(first_run[w]):int(first_run[w]) + int(n_of[w])] for w in members]
    free = sum(int(C.min(axis=1).astype(np.int64).sum()) if len(C) else 0 for C in rows)
    usable = [i for i, C in enumerate(rows) if len(C) <= 32]
    fold = [(WM.fold_rows(C) if lex.fold else C).astype(np.int64) for C in rows]
    keys, own = [], {}
    for l, (ix, E) in lex.by_len.items():
        if not any(abs(l - len(rows[i])) <= band for i in usable):
            continue
        per = np.array([WM.entry_costs(fold[i], E, ins, dele) for i in usable], np.int64).reshape(len(usable), len(ix))
        for col, e in enumerate(ix.tolist()):
            keys.append((int(per[:, col].sum()), e))
            own[e] = per[:, col].tolist()
    keys.sort()
    best = keys[0] if keys else (-1, -1)
    second = keys[1] if len(keys) > 1 else (-1, -1)
    member_cost = [-1] * len(members)
    if keys:
        for i, c in zip(usable, own[best[1]]):
            member_cost[i] = int(c)
    have = [i for i in range(len(members)) if member_cost[i] >= 0]
    best_member = int(members[min(have, key=lambda i: (member_cost[i], i))]) if have else -1
    return (best[1], best[0], second[1], second[0], free, len(keys), len(usable), best_member), member_cost


def match_tracks(costs, first_run, n_of, track_first, track_count, members, lex: WM.Lexicon, ins=64, dele=64, band=2):
    """(a tuple per track, member_cost per slot of members: -1 in a slot of no track)."""
    out, mc = [], np.full(len(members), -1, np.int64)
    for f, n in zip(track_first, track_count):
        rec, own = match_track(costs, first_run, n_of, [int(w) for w in members[int(f):int(f) + int(n)]], lex, ins, dele, band)
        out.append(rec)
        mc[int(f):int(f) + int(n)] = own
    return out, mc


def as_tuples(matches) -> list:
    """The library's TRACK_MATCH_DTYPE records as tuples in the order of TRACK_FIELDS."""
    return [tuple(int(r[k]) for k in TRACK_FIELDS) for r in matches]


def tracks_as_dicts(tracks) -> list:
    """The library's WORD_TRACK_DTYPE records as the dicts word_tracks returns."""
    return [{k: int(r[k]) for k in ("first_frame", "last_frame", "first", "count", "rep", "text_track")} for r in tracks]
