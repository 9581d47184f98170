"""The numpy reference of the line links (STR_ER_WANT_LINE_LINKS, str_er_link_feet, str_er_text_tracks_from_links): the contract at
str_er_line_link (include/str_er.h) in boolean arrays and Python integers.  Footprints are frame_lines_ref.Foot."""
from frame_lines_ref import inter


def adjacent_links(feet, frames, frame_sizes):
    """(a, b, inter) of every line a of a frame f and line b of frame f + 1 with inter > 0, where the two frames have the same size
    (frame_sizes[f] = (w, h)); sorted by (a, b)."""
    out = []
    for a in range(len(feet)):
        for b in range(len(feet)):
            f = int(frames[a])
            if int(frames[b]) == f + 1 and tuple(frame_sizes[f]) == tuple(frame_sizes[f + 1]):
                k = inter(feet[a], feet[b])
                if k > 0:
                    out.append((a, b, k))
    return sorted(out)


def set_links(feet_a, feet_b, num=1, den=2):
    """str_er_link_feet: (a, b, inter, link) of every foot of set a with every foot of set b, inter > 0, sorted by (a, b)."""
    out = []
    for a, fa in enumerate(feet_a):
        for b, fb in enumerate(feet_b):
            k = inter(fa, fb)
            if k > 0:
                out.append((a, b, k, 1 if is_link(fa.pixels, fb.pixels, k, num, den) else 0))
    return out


def is_link(pa, pb, k, num, den):
    return k > 0 and k * den >= num * (pa + pb - k)


def text_tracks(pixels, frames, pairs_dup, links, num=1, den=2):
    """pixels[t], frames[t]; pairs_dup = (a, b, dup) within a frame; links = (a, b, inter) across adjacent frames.  Returns (link per
    record, track per line, tracks as dicts, members): the components by repeated relabelling (no union-find), representative and
    order by the contract."""
    n = len(pixels)
    label = list(range(n))
    link = [1 if is_link(int(pixels[a]), int(pixels[b]), int(k), num, den) else 0 for a, b, k in links]
    edges = [(a, b) for a, b, d in pairs_dup if d] + [(a, b) for (a, b, _), l in zip(links, link) if l]
    changed = True
    while changed:
        changed = False
        for a, b in edges:
            m = min(label[a], label[b])
            if label[a] != m or label[b] != m:
                label[a] = label[b] = m
                changed = True
    comp = {}
    for t in range(n):
        comp.setdefault(label[t], []).append(t)
    groups = sorted((sorted(g) for g in comp.values()), key=lambda g: (min(int(frames[t]) for t in g), g[0]))
    track = [0] * n
    tracks, members = [], []
    for i, g in enumerate(groups):
        rep = max(g, key=lambda t: (int(pixels[t]), -t))
        for t in g:
            track[t] = i
        tracks.append(dict(first_frame=min(int(frames[t]) for t in g), last_frame=max(int(frames[t]) for t in g), first=len(members), count=len(g),
                           rep=rep, pixels=int(pixels[rep])))
        members += g
    return link, track, tracks, members
