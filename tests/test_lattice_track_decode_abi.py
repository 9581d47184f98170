"""CPU checks of the track decode over the members' piece lattices (str_er_set_lattice_track_decode; the contract is at
str_er_lattice_track_decode): the header compiles as plain C with the new prototypes, the library exports them, the two reused records
keep their sizes, STR_ER_ABI_VERSION stays 2, the set of STR_ER_WANT_* names is what it was, the contract's key sentences stand, the
binding has its parts, and the pure host entry point and the setter refuse what they must."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lattice_track_decode_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "str_er.h")
FUNCS = ("str_er_set_lattice_track_decode", "str_er_lattice_decode_tracks", "str_er_lattice_decode_tracks_host", "str_er_lattice_track_decode_stats",
         "str_er_result_lattice_track_decodes", "str_er_result_lattice_track_decode_chars", "str_er_result_lattice_track_decode_members",
         "str_er_result_lattice_track_decode_src", "str_er_result_lattice_track_decode_parts")
WANTS = {"STR_ER_WANT_NODES", "STR_ER_WANT_MASKS", "STR_ER_WANT_LINE_CROPS", "STR_ER_WANT_LINE_GLYPHS", "STR_ER_WANT_SHAPES", "STR_ER_WANT_STROKES", "STR_ER_WANT_TEXT_MAP",
         "STR_ER_WANT_LINE_MAP", "STR_ER_WANT_FRAME_LINES", "STR_ER_WANT_LINE_LINKS", "STR_ER_WANT_LINE_GEOM", "STR_ER_WANT_LINE_WORDS", "STR_ER_WANT_RUN_READ",
         "STR_ER_WANT_WORD_MATCH", "STR_ER_WANT_WORD_DECODE", "STR_ER_WANT_RUN_SPLIT", "STR_ER_WANT_TRACK_READ", "STR_ER_WANT_LATTICE_DECODE", "STR_ER_WANT_LATTICE_MATCH",
         "STR_ER_WANT_LATTICE_TRACK", "STR_ER_WANT_TRACK_DECODE"}


def test_header_keeps_the_flags_and_states_the_contract():
    full = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert set(re.findall(r"#define\s+(STR_ER_WANT_\w+)", txt)) == WANTS          # no new flag, and no new define with that prefix
    assert re.search(r"#define\s+STR_ER_ABI_VERSION\s+2\b", txt)
    for name in FUNCS:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
    flat = re.sub(r"\s*\n \*\s*", " ", full)
    for words in ("here called str_er_lattice_track_decode", "A member is usable iff N_i <= 32; N_i = 0 is usable", "A track has at most 1024 members",
                  "J(s) = lm(s) + the sum of L_i(s) over the usable members", "J <= 25075935 < 2^31",
                  "the first 32 usable members in slot order whose str_er_lattice_decode string has 1 .. 32 labels",
                  "word for word that of str_er_track_decode", "SUB j * 65 + a, DEL 2080 + j, INS 2112 + j * 65 + a",
                  "(1) cost = lm_cost + the sum of the member costs", "(2) cost <= seed_cost <= J(every seed)", "(3) n_parts - n_del + n_ins = n_chars",
                  "(4) rounds = 0 gives the winning seed's str_er_lattice_decode string byte for byte", "(5) if no member has a cut",
                  "(6) a track of one usable member decoded with the decoder's INS = DEL = 0", "(7) for the final string s taken as a one-entry lexicon without fold",
                  "the result is a local optimum of single edits", "still has no lattice mode", "Nothing here is tuned on labelled text",
                  "It is a setting of the context and no stage flag",
                  # the sentences other tests quote stay word for word; the first now points here
                  "a joint search over the members' piece lattices is not part of it: it is a separate output, str_er_lattice_track_decode",
                  "There is no lattice mode", "pooling lattices over a word track is not part of this", "no tracks, no pool, no lattice match"):
        assert words in flat, words


def test_plain_c_compile_and_the_reused_records(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "str_er.h"\n'
                   "typedef char rec_ok[sizeof(str_er_track_decode) == 32 && sizeof(str_er_lattice_track_member) == 24 && sizeof(str_er_split_part) == 8 ? 1 : -1];\n"
                   "typedef char abi_ok[STR_ER_ABI_VERSION == 2 && STR_ER_WANT_TRACK_DECODE == (1u << 29) && STR_ER_WANT_LATTICE_DECODE == (1u << 26) ? 1 : -1];\n"
                   "int main(void) { rec_ok a; abi_ok b;\n"
                   "  int (*f)(str_er_ctx *, int32_t) = str_er_set_lattice_track_decode;\n"
                   "  int (*g)(str_er_ctx *, const str_er_run_split *, int32_t, const uint8_t *, const uint8_t *, int32_t, const int32_t *, const int32_t *, int32_t,\n"
                   "           const int32_t *, const int32_t *, const int32_t *, int32_t, int32_t, str_er_track_decode *, uint8_t *, str_er_lattice_track_member *,\n"
                   "           uint8_t *, str_er_split_part *, int32_t, int32_t *) = str_er_lattice_decode_tracks;\n"
                   "  int (*h)(const str_er_run_split *, int32_t, const uint8_t *, const uint8_t *, int32_t, const int32_t *, const int32_t *, int32_t, const int32_t *,\n"
                   "           const int32_t *, const int32_t *, int32_t, int32_t, const uint8_t *, int32_t, int32_t, int32_t, int32_t, int32_t, int32_t,\n"
                   "           str_er_track_decode *, uint8_t *, str_er_lattice_track_member *, uint8_t *, str_er_split_part *, int32_t, int32_t *) = str_er_lattice_decode_tracks_host;\n"
                   "  int (*s)(const str_er_ctx *, uint64_t *) = str_er_lattice_track_decode_stats;\n"
                   "  const str_er_track_decode *(*p)(const str_er_result *, int32_t *) = str_er_result_lattice_track_decodes;\n"
                   "  const uint8_t *(*q)(const str_er_result *, uint64_t *) = str_er_result_lattice_track_decode_chars;\n"
                   "  const str_er_lattice_track_member *(*r)(const str_er_result *, int32_t *) = str_er_result_lattice_track_decode_members;\n"
                   "  const uint8_t *(*t)(const str_er_result *, uint64_t *) = str_er_result_lattice_track_decode_src;\n"
                   "  const str_er_split_part *(*u)(const str_er_result *, int32_t *) = str_er_result_lattice_track_decode_parts;\n"
                   "  (void)a; (void)b; (void)f; (void)g; (void)h; (void)s; (void)p; (void)q; (void)r; (void)t; (void)u; return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_library_exports_the_symbols(S):
    L = S.load_library()
    assert L.str_er_abi_version() == 2
    for name in FUNCS:
        assert hasattr(L, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in FUNCS:
        assert re.search(r"\bT\s+" + name + r"\b", out), name
    syms = subprocess.run(["nm", "-C", S.lib_path()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bk_lattice_track_decode\b", syms) and re.search(r"\bk_lattice_track_decode_members\b", syms)


def test_binding_has_its_parts(S):
    assert S.TRACK_DECODE_DTYPE.itemsize == 32 and S.LATTICE_TRACK_MEMBER_DTYPE.itemsize == 24
    assert S.LATTICE_TRACK_MEMBER_DTYPE.names == R.MEMBER_FIELDS and S.TRACK_DECODE_DTYPE.names == R.DECODE_FIELDS
    for m in ("set_lattice_track_decode", "lattice_decode_tracks", "lattice_track_decode_stats"):
        assert callable(getattr(S.ERFilter, m)), m
    assert callable(S.FrameStream.set_lattice_track_decode) and callable(S.lattice_decode_tracks_host)
    props = ("lattice_track_decodes", "lattice_track_decode_chars", "lattice_track_decode_members", "lattice_track_decode_src", "lattice_track_decode_parts")
    for m in props:
        assert isinstance(getattr(S.Result, m), property)
    for m in ("word_track_lattice_decode_text", "text_track_lattice_decode_text", "track_member_lattice_decode_parts"):
        assert callable(getattr(S.Result, m))
    r = S.Result.__new__(S.Result)
    for name in props:
        with pytest.raises(ValueError):
            getattr(r, name)
    L = S.load_library()
    for name, n in ((FUNCS[4], C.c_int32(7)), (FUNCS[5], C.c_uint64(7)), (FUNCS[6], C.c_int32(7)), (FUNCS[7], C.c_uint64(7)), (FUNCS[8], C.c_int32(7))):
        assert getattr(L, name)(None, C.byref(n)) is None and n.value == 0


def test_host_entry_point_errors_and_the_setter(S):
    L = S.load_library()
    rng = np.random.default_rng(3)
    B = rng.integers(0, 100, (66, 66)).astype(np.uint8)
    sp, rr, pr, first, n_of, tf, tc, mem = R.pack([R.make_track(rng, [4, 50, 9], 3)])
    args = (sp, rr, pr, first, n_of)
    got = S.lattice_decode_tracks_host(*args, tf, tc, mem, B)
    want = R.decode_tracks(*args, tf, tc, mem, B)
    assert R.as_tuples(got[0]) == want[0] and (got[1] == want[1]).all() and R.members_as_tuples(got[2]) == want[2] and (got[3] == want[3]).all()
    for t_first, t_count, members in (([0], [1], [3]), ([0], [1], [-1]), ([0], [2], [0]), ([1], [1], [0]), ([0], [-1], [0]), ([0, 0], [1, 1], [0])):
        with pytest.raises(S.StrErError) as e:
            S.lattice_decode_tracks_host(*args, t_first, t_count, members, B)
        assert e.value.code == -1, (t_first, t_count, members)
    with pytest.raises(S.StrErError) as e:
        S.lattice_decode_tracks_host(*args, [0], [1025], np.zeros(1025, np.int32), B)
    assert e.value.code == -7
    got = S.lattice_decode_tracks_host(*args, [0], [1024], np.zeros(1024, np.int32), B, rounds=0)
    assert int(got[0][0]["n_used"]) == 1024 and int(got[0][0]["cost"]) == int(got[0][0]["lm_cost"]) + int(got[2]["cost"].sum())
    for kw in (dict(ins=0), dict(ins=256), dict(dele=0), dict(dele=256), dict(rounds=-1), dict(rounds=65), dict(dec_ins=-1), dict(dec_ins=256), dict(dec_dele=256),
               dict(split_cost=-1), dict(split_cost=256)):
        with pytest.raises(S.StrErError) as e:
            S.lattice_decode_tracks_host(*args, tf, tc, mem, B, **kw)
        assert e.value.code == -1, kw
    for kw in (dict(ins=1, dele=255, rounds=0), dict(ins=255, dele=1, rounds=64, split_cost=255), dict(dec_ins=255, dec_dele=255, split_cost=0)):
        S.lattice_decode_tracks_host(*args, tf, tc, mem, B, **kw)
    n = C.c_int32(5)
    one = np.zeros(1, np.int32)
    none = (None, 0, None, None, 0, None, None, 0, None, None, None, 0, 0)
    assert L.str_er_lattice_decode_tracks_host(*none, None, 0, 0, 64, 64, 8, 8, None, None, None, None, None, 0, C.byref(n)) == -1          # no table
    assert L.str_er_lattice_decode_tracks_host(*none, B.ctypes.data, 0, 0, 64, 64, 8, 8, None, None, None, None, None, 0, None) == -1     # no count
    assert L.str_er_lattice_decode_tracks_host(*none, B.ctypes.data, 0, 0, 64, 64, 8, 8, None, None, None, None, None, 0, C.byref(n)) == 0 and n.value == 0
    # cap_parts too small: the count is still set and nothing is written
    out, ch = np.zeros(1, S.TRACK_DECODE_DTYPE), np.full((1, 32), 7, np.uint8)
    mrec, src = np.zeros(len(mem), S.LATTICE_TRACK_MEMBER_DTYPE), np.full((len(mem), 32), 7, np.uint8)
    sp2 = np.ascontiguousarray(sp, dtype=S.RUN_SPLIT_DTYPE)
    p = lambda a: a.ctypes.data
    rc = L.str_er_lattice_decode_tracks_host(p(sp2), len(sp2), p(rr), p(pr), len(pr), p(first), p(n_of), len(first), p(tf), p(tc), p(mem), len(mem), 1, p(B), 0, 0, 64, 64,
                                             8, 8, p(out), p(ch), p(mrec), p(src), p(one), 1, C.byref(n))
    assert rc == -7 and n.value == int(S.lattice_decode_tracks_host(*args, tf, tc, mem, B)[2]["n_parts"].sum()) > 1 and (ch == 7).all() and (src == 7).all()
    assert L.str_er_set_lattice_track_decode(None, 1) == -1
    assert L.str_er_lattice_track_decode_stats(None, None) == -1
    assert L.str_er_lattice_decode_tracks(None, *none, None, None, None, None, None, 0, C.byref(n)) == -1
