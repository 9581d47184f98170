"""CPU checks of the track match over the members' piece lattices (STR_ER_WANT_LATTICE_TRACK, str_er_lattice_match_tracks; the contract is
at str_er_lattice_track_member): header, record layout, exports, binding, and the pure host entry point
str_er_lattice_match_tracks_host against the reference (lattice_track_ref.py), every value with ==, with every validation and capacity
code."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import lattice_match_ref as LM
import lattice_track_ref as LT
import word_match_ref as WM
from test_lattice_decode_abi import cheapen, make_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "str_er.h")
FUNCS = ("str_er_lattice_match_tracks", "str_er_lattice_match_tracks_host", "str_er_lattice_track_stats", "str_er_result_lattice_track_matches",
         "str_er_result_lattice_track_members", "str_er_result_lattice_track_src", "str_er_result_lattice_track_parts")
RECORD = (("cost", 0), ("first_part", 4), ("n_parts", 8), ("n_del", 12), ("n_ins", 16), ("word", 20))
PARAMS = ((64, 64, 2, 8), (1, 1, 0, 0), (255, 255, 31, 255), (3, 200, 1, 8))          # INS, DEL, band, SPLIT


def test_header_declares_the_flag_the_record_and_the_prototypes():
    full = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert re.search(r"#define\s+STR_ER_WANT_LATTICE_TRACK\s+\(268435456u\)", txt)
    assert re.search(r"#define\s+STR_ER_ABI_VERSION\s+2\b", txt)
    assert re.search(r"typedef\s+struct\s+str_er_lattice_track_member\s*\{\s*int32_t\s+cost;\s*int32_t\s+first_part,\s*n_parts;\s*int32_t\s+n_del,\s*n_ins;"
                     r"\s*int32_t\s+word;\s*\}\s*str_er_lattice_track_member;", txt)
    for name in FUNCS:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
    flat = re.sub(r"\s*\n \*\s*", " ", full)
    for words in ("A definition of this library; integers only, exact", "A member is usable iff N_i <= 32", "whatever l is",
                  "plus SPLIT * (|P| - R_i)", "max(1, R_i - band) <= l <= min(32, N_i + band) for at least one usable member", "which may have gaps",
                  "A member with N_i = 0 behaves as str_er_lattice_match says for N = 0", "the unusable ones included", "ties to the earliest slot",
                  "at most 64 * 255, so the sum stays inside int32", "SUB(i) and DEL(i) for i ascending, then INS", "cost = -1 and the counts are 0",
                  "back to back in slot order", "a track of one usable member has the first six fields of that word's str_er_lattice_match",
                  "if no member has a cut, the record and every member cost equal str_er_track_match's", "the entries tried are a superset",
                  "only the winning entry gets segmentations", "no bigram table enters",
                  # the two sentences that named the gap point here
                  "a separate output, str_er_lattice_track_member (STR_ER_WANT_LATTICE_TRACK)",
                  "output but a separate one, str_er_lattice_track_member (STR_ER_WANT_LATTICE_TRACK)"):
        assert words in flat, words
    assert "still reads the matcher's rows: pooling" not in flat


def test_record_layout_c99(tmp_path):
    src = tmp_path / "t.c"
    at = " && ".join(f"offsetof(str_er_lattice_track_member, {f}) == {o}" for f, o in RECORD)
    src.write_text('#include <stddef.h>\n#include "str_er.h"\n'
                   f"typedef char rec_ok[sizeof(str_er_lattice_track_member) == 24 && sizeof(str_er_track_match) == 32 && {at} ? 1 : -1];\n"
                   "typedef char fl[STR_ER_WANT_LATTICE_TRACK == 268435456u && STR_ER_WANT_LATTICE_TRACK == (1u << 28) && STR_ER_WANT_LATTICE_MATCH == (1u << 27) ? 1 : -1];\n"
                   "int main(void) { rec_ok a; fl b;\n"
                   "  int (*g)(str_er_ctx *, const str_er_run_split *, int32_t, const uint8_t *, const uint8_t *, int32_t, const int32_t *, const int32_t *, int32_t,\n"
                   "           const int32_t *, const int32_t *, const int32_t *, int32_t, int32_t, str_er_track_match *, str_er_lattice_track_member *, uint8_t *,\n"
                   "           str_er_split_part *, int32_t, int32_t *) = str_er_lattice_match_tracks;\n"
                   "  int (*k)(const str_er_run_split *, int32_t, const uint8_t *, const uint8_t *, int32_t, const int32_t *, const int32_t *, int32_t, const int32_t *,\n"
                   "           const int32_t *, const int32_t *, int32_t, int32_t, const char *, const int32_t *, int32_t, uint32_t, int32_t, int32_t, int32_t, int32_t,\n"
                   "           str_er_track_match *, str_er_lattice_track_member *, uint8_t *, str_er_split_part *, int32_t, int32_t *) = str_er_lattice_match_tracks_host;\n"
                   "  int (*j)(const str_er_ctx *, uint64_t *) = str_er_lattice_track_stats;\n"
                   "  const str_er_track_match *(*p)(const str_er_result *, int32_t *) = str_er_result_lattice_track_matches;\n"
                   "  const str_er_lattice_track_member *(*m)(const str_er_result *, int32_t *) = str_er_result_lattice_track_members;\n"
                   "  const uint8_t *(*q)(const str_er_result *, uint64_t *) = str_er_result_lattice_track_src;\n"
                   "  const str_er_split_part *(*r)(const str_er_result *, int32_t *) = str_er_result_lattice_track_parts;\n"
                   "  (void)a; (void)b; (void)g; (void)j; (void)k; (void)m; (void)p; (void)q; (void)r; return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_library_exports_the_symbols(S):
    L = S.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in FUNCS:
        assert hasattr(L, name) and re.search(r"\bT\s+" + name + r"\b", out), name
    syms = subprocess.run(["nm", "-C", S.lib_path()], capture_output=True, text=True, check=True).stdout
    for k in ("k_lattice_track_table", "k_lattice_track_match", "k_lattice_track_merge", "k_lattice_track_members", "k_lattice_track_best"):
        assert re.search(r"\b" + k + r"\b", syms), k


def random_lexicon(rng, n, lo=1, hi=12, labels=65):
    return ["".join(WM.ALPHABET[a] for a in rng.integers(65 - labels, 65, int(l))) for l in rng.integers(lo, hi + 1, n)]


def same(S, got, want):
    rec, mrec, src, parts = got
    assert rec.dtype == S.TRACK_MATCH_DTYPE and mrec.dtype == S.LATTICE_TRACK_MEMBER_DTYPE and parts.dtype == S.SPLIT_PART_DTYPE and src.shape == (len(mrec), 32)
    assert LT.as_tuples(rec) == want[0]
    assert LT.members_as_tuples(mrec) == want[1]
    assert (src == want[2]).all()
    assert np.stack([parts["run"], parts["piece"]], 1).tolist() == want[3].tolist()


def test_host_equals_the_reference_on_random_tracks(S):
    rng = np.random.default_rng(61)
    n_of = np.array([0, 1, 2, 8, 13, 32, 33] + list(rng.integers(0, 7, 10)))
    first = np.concatenate([[0], np.cumsum(n_of)[:-1]])
    cuts = rng.integers(0, 4, int(n_of.sum()))
    cuts[first[5]:first[5] + 32] = 0                                      # (32 uncut runs: N = 32 exactly; 33: an unusable member)
    cuts[first[6]:first[6] + 33] = 0
    cuts[first[4]:first[4] + 13] = 3                                      # (13 runs of 3 cuts: N = 52, unusable by its atoms)
    sp, rc, pc = make_rows(S, rng, cuts)
    rc, pc = cheapen(rng, rc), cheapen(rng, pc)
    members = np.array([1, 2, 7, 0, 3, 6, 8, 5, 5, 4, 6, 9, 10, 11, 12, 13, 14, 15, 16, 2, 2], np.int32)
    tf, tc = [0, 3, 6, 7, 9, 11, 11, 19], [3, 3, 1, 2, 2, 0, 8, 2]          # (a track of unusable members, one of no members, a word twice)
    words = random_lexicon(rng, 120, labels=14) + ["a" * 32, "B" * 31, "c" * 30]
    for fold in (True, False):
        lex = WM.Lexicon(words, fold)
        for ins, dele, band, split in PARAMS[:2] + PARAMS[3:]:
            want = LT.match_tracks(sp, rc, pc, first, n_of, tf, tc, members, lex, ins, dele, band, split)
            same(S, S.lattice_match_tracks_host(sp, rc, pc, first, n_of, tf, tc, members, words, fold, ins, dele, band, split), want)
            assert want[0][4][:4] == (-1, -1, -1, -1) and want[0][4][5:] == (0, 0, -1) and want[0][4][4] > 0          # (members 4 and 6: nothing tried, free_cost made)
            assert want[0][5] == (-1, -1, -1, -1, 0, 0, 0, -1)
            assert want[0][7][7] == 2 and want[1][19][0] == want[1][20][0]                                              # (the same word twice: the earlier slot)
    # band 31 on the small tracks alone (every length is tried: the reference takes a while per member)
    ins, dele, band, split = PARAMS[2]
    want = LT.match_tracks(sp, rc, pc, first, n_of, tf[:1], tc[:1], members, WM.Lexicon(words[:60], True), ins, dele, band, split)
    same(S, S.lattice_match_tracks_host(sp, rc, pc, first, n_of, tf[:1], tc[:1], members, words[:60], True, ins, dele, band, split), want)
    # no tracks, members of no track, and an empty lexicon
    rec, mrec, src, parts = S.lattice_match_tracks_host(sp, rc, pc, first, n_of, [], [], [], words)
    assert rec.shape == (0,) and mrec.shape == (0,) and src.shape == (0, 32) and parts.shape == (0,)
    rec, mrec, src, parts = S.lattice_match_tracks_host(sp, rc, pc, first, n_of, [1], [1], [1, 2, 3], words)
    assert LT.members_as_tuples(mrec)[0][0] == -1 and LT.members_as_tuples(mrec)[0][5] == -1 and mrec["word"].tolist() == [-1, 2, -1] and (src[0] == 255).all()
    rec, mrec, src, parts = S.lattice_match_tracks_host(sp, rc, pc, first, n_of, tf, tc, members, [])
    assert [r[:4] + r[5:] for r in LT.as_tuples(rec)] == [(-1, -1, -1, -1, 0, n, -1) for n in (3, 2, 1, 2, 0, 0, 8, 2)]
    assert (mrec["cost"] == -1).all() and (mrec["word"] == members).all() and (src == 0xFF).all() and len(parts) == 0


def test_the_identities_on_the_host(S):
    rng = np.random.default_rng(62)
    n_of = np.array([1, 2, 3, 5, 8, 0, 4])
    first = np.concatenate([[0], np.cumsum(n_of)[:-1]])
    sp, rc, pc = make_rows(S, rng, rng.integers(0, 4, int(n_of.sum())))
    rc, pc = cheapen(rng, rc), cheapen(rng, pc)
    words = random_lexicon(rng, 200, 1, 12, labels=12)
    for ins, dele, band, split in PARAMS:
        # (1) tracks of one member: the lattice match of that word
        nw = len(n_of)
        rec, mrec, src, parts = S.lattice_match_tracks_host(sp, rc, pc, first, n_of, np.arange(nw), np.ones(nw), np.arange(nw), words, True, ins, dele, band, split)
        one, osrc, oparts = S.lattice_match_words_host(sp, rc, pc, first, n_of, words, True, ins, dele, band, split)
        assert [r[:6] for r in LT.as_tuples(rec)] == [r[:6] for r in LM.as_tuples(one)]
        assert src.tobytes() == osrc.tobytes() and parts.tobytes() == oparts.tobytes()
        for k in ("first_part", "n_parts", "n_del", "n_ins"):
            assert mrec[k].tolist() == one[k].tolist()
        assert mrec["cost"].tolist() == one["cost"].tolist() and rec["best_member"].tolist() == [w if one["entry"][w] >= 0 else -1 for w in range(nw)]
        # (3) every member usable: never more than the track match on the unsplit runs
        tf, tc, mem = [0, 3], [3, 4], [0, 1, 2, 3, 4, 5, 6]
        rec, mrec, src, parts = S.lattice_match_tracks_host(sp, rc, pc, first, n_of, tf, tc, mem, words, True, ins, dele, band, split)
        plain, mc = S.match_tracks_host(rc, first, n_of, tf, tc, mem, words, True, ins, dele, band)
        for g in range(2):
            if plain["n_tried"][g] > 0:
                assert rec["n_tried"][g] >= plain["n_tried"][g] and 0 <= rec["cost"][g] <= plain["cost"][g]
    # (2) without cuts: the track match on the runs, field for field
    sp0, rc0, pc0 = make_rows(S, rng, np.zeros(int(n_of.sum()), np.int64))
    rc0 = cheapen(rng, rc0)
    for fold in (True, False):
        for ins, dele, band, split in PARAMS:
            rec, mrec, src, parts = S.lattice_match_tracks_host(sp0, rc0, pc0, first, n_of, tf, tc, mem, words, fold, ins, dele, band, split)
            plain, mc = S.match_tracks_host(rc0, first, n_of, tf, tc, mem, words, fold, ins, dele, band)
            assert rec.tobytes() == plain.tobytes() and mrec["cost"].tolist() == mc.tolist()
            runs = [r for i, w in enumerate(mem) if mrec["cost"][i] >= 0 for r in range(first[w], first[w] + n_of[w])]
            assert parts["run"].tolist() == runs and (parts["piece"] == -1).all()


def test_argument_and_capacity_errors(S):
    rng = np.random.default_rng(63)
    words = ["ab", "cde", "f"]
    sp, rc, pc = make_rows(S, rng, [1, 0, 3])
    host = lambda sp_=sp, first=(0,), n_of=(3,), tf=(0,), tc=(1,), mem=(0,), **kw: S.lattice_match_tracks_host(sp_, rc, pc, list(first), list(n_of), list(tf), list(tc),
                                                                                                                  list(mem), words, **kw)
    host()
    for first, n_of in (([1], [3]), ([0], [-1]), ([-1], [1]), ([3], [1])):
        with pytest.raises(S.StrErError) as e:                           # a word outside the runs
            host(first=first, n_of=n_of)
        assert e.value.code == -1
    for field, value in (("n_cuts", 4), ("n_cuts", -1), ("n_pieces", 3), ("first_piece", -1), ("first_piece", len(pc) - 1)):
        bad = sp.copy()
        bad[field][0] = value                                            # cuts outside 0 .. 3, pieces that do not follow, a piece outside the rows
        with pytest.raises(S.StrErError) as e:
            host(sp_=bad)
        assert e.value.code == -1, (field, value)
    for mem in ([1], [-1]):
        with pytest.raises(S.StrErError) as e:                           # a member outside the words
            host(mem=mem)
        assert e.value.code == -1
    for tf, tc, mem in (([1, 0], [1, 1], [0, 0]), ([0, 0], [1, 1], [0, 0]), ([0], [2], [0]), ([0], [-1], [0]), ([-1], [1], [0])):
        with pytest.raises(S.StrErError) as e:                           # tracks that do not ascend, that overlap, or that leave the member array
            host(tf=tf, tc=tc, mem=mem)
        assert e.value.code == -1
    with pytest.raises(S.StrErError) as e:                               # more than 65536 members
        host(tf=[0], tc=[65537], mem=[0] * 65537)
    assert e.value.code == -7
    for ins, dele, band, split in ((0, 64, 2, 8), (64, 256, 2, 8), (64, 64, -1, 8), (64, 64, 32, 8), (64, 64, 2, -1), (64, 64, 2, 256)):
        with pytest.raises(S.StrErError) as e:                           # a bad INS, DEL, band or SPLIT
            host(fold_case=True, ins=ins, dele=dele, band=band, split_cost=split)
        assert e.value.code == -1
    # the raw entry point: NULL arguments, negative counts, a lexicon byte outside the alphabet, cap_parts too small with *n_parts still set
    L = S.load_library()
    fr, no, tf, tc, mem = np.zeros(1, np.int32), np.full(1, 3, np.int32), np.zeros(1, np.int32), np.full(1, 2, np.int32), np.zeros(2, np.int32)
    rec, mrec, sr, parts, n = np.zeros(1, S.TRACK_MATCH_DTYPE), np.zeros(2, S.LATTICE_TRACK_MEMBER_DTYPE), np.zeros(64, np.uint8), np.zeros(16, S.SPLIT_PART_DTYPE), C.c_int32(-5)
    raw, off = np.frombuffer(b"abcdef", np.uint8).copy(), np.array([0, 2, 5, 6], np.int32)
    p = lambda a: a.ctypes.data
    good = [p(sp), 3, p(rc), p(pc), len(pc), p(fr), p(no), 1, p(tf), p(tc), p(mem), 2, 1, p(raw), p(off), 3, 1, 64, 64, 2, 8, p(rec), p(mrec), p(sr), p(parts), 16, C.byref(n)]
    assert L.str_er_lattice_match_tracks_host(*good) == 0 and 6 <= n.value <= 14 and int(mrec["n_parts"].sum()) == n.value and int(rec["entry"][0]) >= 0
    assert mrec["first_part"].tolist() == [0, n.value // 2] and mrec["word"].tolist() == [0, 0] and sr[:32].tobytes() == sr[32:].tobytes()
    want = n.value
    for at in (0, 2, 3, 5, 6, 8, 9, 10, 13, 14, 21, 22, 23, 24, 26):
        bad = list(good)
        bad[at] = None
        assert L.str_er_lattice_match_tracks_host(*bad) == -1, at
    for at, value in ((1, -1), (4, -1), (7, -1), (11, -1), (12, -1), (15, -1), (16, 2), (25, -1)):
        bad = list(good)
        bad[at] = value
        assert L.str_er_lattice_match_tracks_host(*bad) == -1, at
    dirty = raw.copy()
    dirty[3] = ord("-")
    bad = list(good)
    bad[13] = p(dirty)
    assert L.str_er_lattice_match_tracks_host(*bad) == -1
    small = list(good)
    small[25] = want - 1
    n.value = -5
    before = rec.copy()
    assert L.str_er_lattice_match_tracks_host(*small) == -7 and n.value == want and rec.tobytes() == before.tobytes()          # STR_ER_ECAPACITY
    # a NULL context
    assert L.str_er_lattice_match_tracks(None, *good[:13], *good[21:]) == -1 and L.str_er_lattice_track_stats(None, None) == -1


def test_binding_constants_dtypes_and_keywords(S):
    assert S.WANT_LATTICE_TRACK == 1 << 28 == 268435456
    d = S.LATTICE_TRACK_MEMBER_DTYPE
    assert d.itemsize == 24 and tuple((n, d.fields[n][1]) for n in d.names) == RECORD
    for m in ("text_detect", "text_detect_list"):
        assert inspect.signature(getattr(S.ERFilter, m)).parameters["want_lattice_track"].default is False
    for m in ("submit", "submit_nv12", "submit_copy", "submit_list", "submit_nv12_list", "submit_copy_list"):
        assert inspect.signature(getattr(S.FrameStream, m)).parameters["want_lattice_track"].default is False
    binding = __import__("importlib").import_module("scene-text-recognition_amd.binding")
    assert binding._want_flags(lattice_track=True) == 268435456
    assert binding._want_flags(lattice_match=True, track_read=True, lattice_track=True) == 268435456 | 134217728 | S.WANT_TRACK_READ
    for m in ("lattice_match_tracks", "lattice_track_stats"):
        assert callable(getattr(S.ERFilter, m)), m
    sig = inspect.signature(S.lattice_match_tracks_host).parameters
    assert (sig["fold_case"].default, sig["ins"].default, sig["dele"].default, sig["band"].default, sig["split_cost"].default) == (True, 64, 64, 2, 8)
    for m in ("lattice_track_matches", "lattice_track_members", "lattice_track_src", "lattice_track_parts"):
        assert isinstance(getattr(S.Result, m), property)
    for m in ("word_track_lattice_text", "text_track_lattice_match_text", "track_member_lattice_parts"):
        assert callable(getattr(S.Result, m))


def test_result_accessors_without_the_flag_and_on_a_made_up_result(S):
    r = S.Result.__new__(S.Result)                                        # (a result made by hand with none of the new attributes)
    for name in ("lattice_track_matches", "lattice_track_members", "lattice_track_src", "lattice_track_parts"):
        with pytest.raises(ValueError):
            getattr(r, name)
    L = S.load_library()
    for fn in (L.str_er_result_lattice_track_matches, L.str_er_result_lattice_track_members, L.str_er_result_lattice_track_parts):
        n = C.c_int32(7)
        assert fn(None, n) is None and n.value == 0
    nb = C.c_uint64(7)
    assert L.str_er_result_lattice_track_src(None, nb) is None and nb.value == 0
    r._words = np.zeros(2, S.LINE_WORD_DTYPE)
    r._words["first_run"], r._words["n_runs"] = [0, 2], [2, 1]
    r._run_reads = np.zeros(3, S.RUN_READ_DTYPE)
    r._run_reads["ch"] = [ord("A"), ord("B"), ord("Z")]
    r._lexicon = ("corn", "com")
    r._word_links = np.zeros(0, S.WORD_LINK_DTYPE)
    r._word_tracks = np.zeros(2, S.WORD_TRACK_DTYPE)
    r._word_tracks["first"], r._word_tracks["count"], r._word_tracks["rep"] = [0, 1], [1, 1], [0, 1]
    r._word_track_members = np.array([0, 1], np.int32)
    r._lattice_track_matches = np.zeros(2, S.TRACK_MATCH_DTYPE)
    r._lattice_track_matches["entry"] = [0, -1]
    r._lattice_track_members = np.zeros(2, S.LATTICE_TRACK_MEMBER_DTYPE)
    r._lattice_track_members["first_part"], r._lattice_track_members["n_parts"] = [0, 3], [3, 0]
    r._lattice_track_parts = np.array([(0, -1), (1, 0), (1, 1)], S.SPLIT_PART_DTYPE)
    assert r.word_track_lattice_text(0) == "corn" and r.word_track_lattice_text(1) == "Z"
    assert r.track_member_lattice_parts(0).tolist() == [(0, -1), (1, 0), (1, 1)] and len(r.track_member_lattice_parts(1)) == 0


def test_cpp_mirror_and_example_compile():
    host = os.path.join(ROOT, "scene-text-recognition_amd", "host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    os.path.join(host, "example_lattice_track.cpp")], check=True)
    txt = open(os.path.join(host, "er_filter_hip.hpp")).read()
    for name in ("lattice_match_tracks", "lattice_match_tracks_host", "word_track_lattice_text", "lattice_track_matches") + FUNCS[:2] + FUNCS[3:]:
        assert re.search(r"\b" + name + r"\(", txt), name
