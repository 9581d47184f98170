"""The decode pool's ABI (str_er_track_pool_create_decode, _keep, _read_decode, _members; the contract is at str_er_pool_decode).
Without a GPU: the header, the record's layout, the exports, the binding and the NULL arguments.  On the GPU: the error matrix -- every
refused call gives its code and leaves the pool as it was, a read of all slots giving the same bytes before and after."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "str_er.h")
FUNCS = ("str_er_track_pool_create_decode", "str_er_track_pool_keep", "str_er_track_pool_read_decode", "str_er_track_pool_members")
RECORD = (("cost", 0), ("seed_cost", 4), ("n_chars", 8), ("n_edits", 12), ("converged", 16), ("n_used", 20), ("seed_member", 24), ("lm_cost", 28), ("n_members", 32),
          ("n_kept", 36))
EINVAL, ESTATE, ECAPACITY = -1, -6, -7


def test_header_declares_the_record_the_flag_and_the_prototypes():
    full = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert re.search(r"#define\s+STR_ER_POOL_DECODE\s+2u", txt) and re.search(r"#define\s+STR_ER_POOL_LATTICE\s+1u", txt)
    assert re.search(r"#define\s+STR_ER_ABI_VERSION\s+2\b", txt) and re.search(r"\}\s*str_er_pool_decode;", txt)
    for name in FUNCS:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
    flat = re.sub(r"\s*\n \*\s*", " ", full)
    for words in ("the members' cost rows themselves stay on the device", "make every decode pool of the context stale -- and no lexicon pool",
                  "make every lexicon pool stale -- and no decode pool", "serial << 32 | its index in that call's member array", "the unusable members (more than 32 rows) included",
                  "The top-keep of a union is the top-keep of the union of top-keeps", "the kept list in ascending key order", "seed_member is therefore an age rank",
                  "-1, -1, 0, 0, 0, 0, -1, -1, n_members = n_kept = 0", "evicted evidence is gone", "There is no lattice mode", "there is no cache of clean slots",
                  # the two sentences that named the gap point here
                  "a pool of another kind, the decode pool (str_er_pool_decode, below)", "a decode pool (str_er_pool_decode) keeps the newest members of a track"):
        assert words in flat, words
    assert not re.search(r"STR_ER_WANT_\w+\s+\((?:1073741824|2147483648)u\)", txt)          # the last two bits are not spent


def test_record_layout_c99(tmp_path):
    src = tmp_path / "t.c"
    at = " && ".join(f"offsetof(str_er_pool_decode, {f}) == {o}" for f, o in RECORD)
    src.write_text('#include <stddef.h>\n#include "str_er.h"\n'
                   f"typedef char rec_ok[sizeof(str_er_pool_decode) == 40 && sizeof(str_er_pool_decode) == sizeof(str_er_track_decode) + 8 && {at} ? 1 : -1];\n"
                   "typedef char fl[STR_ER_POOL_DECODE == 2u && STR_ER_POOL_LATTICE == 1u && STR_ER_ABI_VERSION == 2 ? 1 : -1];\n"
                   "int main(void) { rec_ok a; fl b;\n"
                   "  int (*c)(str_er_ctx *, int32_t, int32_t, str_er_track_pool **) = str_er_track_pool_create_decode;\n"
                   "  int (*k)(const str_er_track_pool *, int32_t *) = str_er_track_pool_keep;\n"
                   "  int (*r)(str_er_track_pool *, const int32_t *, int32_t, str_er_pool_decode *, uint8_t *, int32_t *) = str_er_track_pool_read_decode;\n"
                   "  int (*m)(str_er_track_pool *, int32_t, uint64_t *, int32_t *, uint8_t *, int32_t *) = str_er_track_pool_members;\n"
                   "  int (*o)(str_er_ctx *, int32_t, uint32_t, str_er_track_pool **) = str_er_track_pool_create;\n"
                   "  (void)a; (void)b; (void)c; (void)k; (void)r; (void)m; (void)o; return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_library_exports_the_symbols_and_the_kernels(S):
    L = S.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in FUNCS:
        assert hasattr(L, name) and re.search(r"\bT\s+" + name + r"\b", out), name
    syms = subprocess.run(["nm", "-C", S.lib_path()], capture_output=True, text=True, check=True).stdout
    for kernel in ("k_dpool_keep", "k_dpool_join", "k_dpool_plan", "k_dpool_records", "k_dpool_clear", "k_dpool_reset"):
        assert re.search(r"\b" + kernel + r"\b", syms), kernel


def test_binding_and_null_arguments(S):
    L = S.load_library()
    assert S.POOL_DECODE == 2 and S.POOL_DECODE_DTYPE.itemsize == 40 and S.POOL_DECODE_DTYPE.names == tuple(f for f, _ in RECORD)
    assert [S.POOL_DECODE_DTYPE.fields[f][1] for f, _ in RECORD] == [o for _, o in RECORD]
    assert S.POOL_DECODE_DTYPE.names[:8] == S.TRACK_DECODE_DTYPE.names and issubclass(S.DecodePool, S.TrackPool)
    h, k, n = C.c_void_p(), C.c_int32(), C.c_int32()
    assert L.str_er_track_pool_create_decode(None, 1, 1, C.byref(h)) == EINVAL
    assert L.str_er_track_pool_keep(None, C.byref(k)) == EINVAL
    assert L.str_er_track_pool_read_decode(None, None, 0, None, None, None) == EINVAL
    assert L.str_er_track_pool_members(None, 0, None, None, None, C.byref(n)) == EINVAL


@pytest.fixture(scope="module")
def f(S):
    ctx = S.ERFilter(params=S.Params(max_width=64, max_height=64, max_frames=1))
    yield ctx
    ctx.close()


def _code(S, call):
    with pytest.raises(S.StrErError) as e:
        call()
    return e.value.code


@pytest.mark.gpu
def test_creation_errors(S, f):
    f.set_bigram(None)
    assert _code(S, lambda: S.DecodePool(f, 4, 4)) == ESTATE                  # no table
    f.set_bigram(np.zeros((66, 66), np.uint8))
    for cap, keep in ((4, 0), (4, 1025), (0, 4), (4, -1), (-1, 1)):
        assert _code(S, lambda: S.DecodePool(f, cap, keep)) == EINVAL
    assert _code(S, lambda: S.DecodePool(f, (1 << 14) + 1, 1024)) == ECAPACITY      # cap * keep > 2^24
    assert _code(S, lambda: S.DecodePool(f, (1 << 24) + 1, 1)) == ECAPACITY
    h = C.c_void_p()
    assert f.L.str_er_track_pool_create(f.h, 4, 2, C.byref(h)) == EINVAL and not h.value          # _create knows no new flag
    pool = S.DecodePool(f, 3, 1024)                                            # no lexicon, no model
    info = pool.info()
    assert info["decode"] and info["keep"] == 1024 and info["n_entries"] == 0 and info["cap_tracks"] == 3 and info["in_use"] == 0 and not info["stale"]
    assert info["device_bytes"] >= 3 * 1024 * 2184
    pool.close()


@pytest.mark.gpu
def test_error_matrix_leaves_the_pool_unchanged(S, f):
    rng = np.random.default_rng(51)
    B = rng.integers(0, 60, (66, 66)).astype(np.uint8)
    f.set_bigram(B)
    f.set_word_decode(0, 0)
    f.set_track_decode(64, 64, 2)
    f.set_lexicon(["AB", "CD"])
    costs = rng.integers(0, 256, (7, 65)).astype(np.uint8)
    words = (costs, [0, 3], [3, 4])
    pool, lex = S.DecodePool(f, 3, 2), S.TrackPool(f, 3)
    try:
        pool.add(*words, [0, 2], [2, 1], [0, 1, 1], [0, 2])
        lex.add(*words, [0, 2], [2, 1], [0, 1, 1], [0, 2])
        before, lex_before = pool.read([0, 1, 2]), lex.read([0, 1, 2]).tobytes()
        members_before = [pool.members(s) for s in range(3)]
        assert before[0]["n_members"].tolist() == [2, 0, 1]
        sp = np.zeros(7, S.RUN_SPLIT_DTYPE)
        refused = (
            (ESTATE, lambda: S.TrackPool.add_lattice(pool, sp, costs, np.zeros((0, 65), np.uint8), [0, 3], [3, 4], [0], [1], [0], [1])),      # _add_lattice on a decode pool
            (ESTATE, lambda: S.TrackPool.read(pool, [0])),                                            # _read on a decode pool
            (ESTATE, lambda: S.DecodePool.read(lex, [0])),                                            # _read_decode on a lexicon pool
            (ESTATE, lambda: S.DecodePool.members(lex, 0)),
            (EINVAL, lambda: pool.add(*words, [0, 1], [1, 1], [0, 1], [1, 1])),                       # a slot named twice
            (EINVAL, lambda: pool.add(*words, [0], [1], [0], [3])),                                   # ... out of range
            (EINVAL, lambda: pool.add(*words, [0], [1], [0], [-1])),
            (EINVAL, lambda: pool.add(*words, [0], [1], [2], [1])),                                   # a member that is no word
            (EINVAL, lambda: pool.add(costs, [0, 5], [3, 4], [0], [1], [0], [1])),                    # a word outside the rows
            (EINVAL, lambda: pool.join(0, [2, 2])),
            (EINVAL, lambda: pool.join(0, [0])),
            (EINVAL, lambda: pool.join(3, [0])),
            (EINVAL, lambda: pool.join(0, [3])),
            (EINVAL, lambda: pool.clear([0, 3])),
            (EINVAL, lambda: pool.read([0, 3])),
            (EINVAL, lambda: pool.read([-1])),
            (EINVAL, lambda: pool.members(3)),
        )
        lex.keep = 2          # (DecodePool.read sizes its arrays by it)
        for code, call in refused:
            assert _code(S, call) == code
            assert all(a.tobytes() == b.tobytes() for a, b in zip(before, pool.read([0, 1, 2])))
            assert all(a.tobytes() == b.tobytes() for s in range(3) for a, b in zip(members_before[s], pool.members(s)))
            assert lex.read([0, 1, 2]).tobytes() == lex_before
        k = C.c_int32(-1)
        assert f.L.str_er_track_pool_keep(lex.h, C.byref(k)) == 0 and k.value == 0
        pool.add(*words, [0], [1], [1], [1])          # the refused additions took no serial: this is the second
        assert pool.members(1)[0].tolist() == [2 << 32]
    finally:
        pool.close()
        lex.close()
        f.set_lexicon([])
