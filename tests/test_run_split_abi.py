"""Checks of the ABI of the splitting of touching glyphs (STR_ER_WANT_RUN_SPLIT, str_er_feet_split, str_er_split_words; the contract is at
str_er_run_split): header, record layouts, exports, the binding's dtypes, the pure host entry points against the reference
(run_split_ref.py) with every argument check -- on the CPU -- and the argument checks of the entry points that take a context, after
each of which the context stays usable (gpu)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import run_split_ref as RS
from test_run_split_ref import HAND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "str_er.h")
FUNCS = ("str_er_set_run_split", "str_er_run_split_stats", "str_er_cuts_from_counts", "str_er_feet_split", "str_er_split_words", "str_er_split_words_host",
         "str_er_result_run_splits", "str_er_result_run_pieces", "str_er_result_piece_reads", "str_er_result_piece_costs", "str_er_result_split_parts",
         "str_er_result_word_splits")
RECORDS = {
    "str_er_run_split": (32, (("n_cuts", 0), ("cut", 4), ("thr", 16), ("first_piece", 20), ("n_pieces", 24), ("n_parts", 28))),
    "str_er_run_piece": (32, (("run", 0), ("from", 4), ("to", 8), ("x0", 12), ("x1", 16), ("y0", 20), ("y1", 24), ("pixels", 28))),
    "str_er_split_part": (8, (("run", 0), ("piece", 4))),
    "str_er_word_split": (16, (("first_part", 0), ("n_parts", 4), ("cost", 8), ("read_cost", 12))),
}


def test_header_declares_the_flag_the_records_and_the_prototypes():
    full = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert re.search(r"#define\s+STR_ER_WANT_RUN_SPLIT\s+\(16777216u\)", txt)
    for name in FUNCS + tuple(RECORDS):
        assert re.search(r"\b" + name + r"\b", txt), name
    flat = re.sub(r"\s*\n \*\s*", " ", full)
    for words in ("thr = floor(H * num / den)", "touches either end of the run is no valley", "p = floor((cf + cl) / 2)", "the 3 with the smallest (d, p)",
                  "A run with W > 1024 is not split", "thr = 0 gives no valley", "2, 5 or 9", "ordered by (i, j)",
                  "D[j] = min over 0 <= i < j of D[i] + m(i, j) + (i > 0 ? SPLIT : 0)", "the smallest i that attains the minimum", "8 by default",
                  "cost <= read_cost and n_parts >= n_runs", "no slanted or curved cuts", "no joint decode over the piece lattice",
                  "not tuned on labelled data", "str_er_run_split (STR_ER_WANT_RUN_SPLIT)"):
        assert words in flat, words
    assert "runs are not split in the image" not in flat


def test_record_layouts_c99(tmp_path):
    src = tmp_path / "t.c"
    body = ""
    for k, (name, (size, fields)) in enumerate(RECORDS.items()):
        at = " && ".join(f"offsetof({name}, {f}) == {o}" for f, o in fields)
        body += f"typedef char ok{k}[sizeof({name}) == {size} && {at} ? 1 : -1];\n"
    src.write_text('#include <stddef.h>\n#include "str_er.h"\n' + body +
                   "typedef char fl[STR_ER_WANT_RUN_SPLIT == 16777216u && STR_ER_WANT_RUN_SPLIT == (1u << 24) && STR_ER_RUN_SPLIT_MAX_W == 1024 ? 1 : -1];\n"
                   "int main(void) { ok0 a; ok1 b; ok2 c; ok3 d; fl e;\n"
                   "  int (*f)(str_er_ctx *, int32_t, int32_t, int32_t) = str_er_set_run_split;\n"
                   "  int (*g)(const uint32_t *, int32_t, int32_t, int32_t, int32_t, int32_t *, int32_t *, uint32_t *) = str_er_cuts_from_counts;\n"
                   "  const str_er_run_split *(*p)(const str_er_result *, int32_t *) = str_er_result_run_splits;\n"
                   "  const uint8_t *(*q)(const str_er_result *, uint64_t *) = str_er_result_piece_costs;\n"
                   "  (void)a; (void)b; (void)c; (void)d; (void)e; (void)f; (void)g; (void)p; (void)q; return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_library_exports_and_dtypes(S):
    L = S.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in FUNCS:
        assert hasattr(L, name) and re.search(r"\bT\s+" + name + r"\b", out), name
    syms = subprocess.run(["nm", "-C", S.lib_path()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bk_run_cuts\b", syms) and re.search(r"\bk_split_words\b", syms)
    for dt, name in ((S.RUN_SPLIT_DTYPE, "str_er_run_split"), (S.RUN_PIECE_DTYPE, "str_er_run_piece"), (S.SPLIT_PART_DTYPE, "str_er_split_part"),
                     (S.WORD_SPLIT_DTYPE, "str_er_word_split")):
        size, fields = RECORDS[name]
        assert dt.itemsize == size and [(f, dt.fields[f][1]) for f, _ in fields] == list(fields), name
    assert S.WANT_RUN_SPLIT == 1 << 24


def test_cuts_from_counts_and_its_checks(S):
    for n, h, want in HAND:
        assert S.cuts_from_counts(n, h) == (want, h // 4)
    rng = np.random.default_rng(12)
    for _ in range(300):
        W, h = int(rng.choice([1, 2, 3, 9, 64, 65, 200, 1024, 1025])), int(rng.integers(1, 40))
        n = np.where(rng.random(W) < 0.3, 1, rng.integers(1, h + 1, W))
        num, den = (int(rng.integers(1, 65536)), int(rng.integers(1, 65536))) if rng.random() < 0.3 else (1, int(rng.integers(1, 6)))
        assert S.cuts_from_counts(n, h, num, den) == RS.cuts(n, h, num, den)
    # a height whose H * num leaves 32 bits and comes back small: the threshold is the 64-bit quotient, every column is low, no valley
    inv = pow(65535, -1, 2 ** 32)
    tall = next(h for h in ((r * inv) % 2 ** 32 for r in range(32768, 33000)) if 65537 <= h < 2 ** 31)
    assert (tall * 65535) % 2 ** 32 < 33000 and tall * 65535 >= 2 ** 32
    assert S.cuts_from_counts([40000, 100, 40000], tall, 65535, 1) == ([], 2 ** 32 - 1) and RS.cuts([40000, 100, 40000], tall, 65535, 1)[0] == []
    L = S.load_library()
    n = np.array([8, 8, 1, 8, 8], np.uint32)
    cut, k, thr = np.zeros(3, np.int32), C.c_int32(), C.c_uint32()
    ok = lambda *a: L.str_er_cuts_from_counts(*a)
    assert ok(n.ctypes.data, 5, 8, 1, 4, cut.ctypes.data, C.byref(k), C.byref(thr)) == 0 and k.value == 1 and cut.tolist() == [2, -1, -1] and thr.value == 2
    assert ok(n.ctypes.data, 5, 8, 1, 4, cut.ctypes.data, C.byref(k), None) == 0
    for bad in ((None, 5, 8, 1, 4, cut.ctypes.data, C.byref(k), None), (n.ctypes.data, 5, 8, 1, 4, None, C.byref(k), None),
                (n.ctypes.data, 5, 8, 1, 4, cut.ctypes.data, None, None), (n.ctypes.data, 0, 8, 1, 4, cut.ctypes.data, C.byref(k), None),
                (n.ctypes.data, 5, 0, 1, 4, cut.ctypes.data, C.byref(k), None), (n.ctypes.data, 5, 8, 0, 4, cut.ctypes.data, C.byref(k), None),
                (n.ctypes.data, 5, 8, 1, 0, cut.ctypes.data, C.byref(k), None), (n.ctypes.data, 5, 8, 65536, 4, cut.ctypes.data, C.byref(k), None),
                (n.ctypes.data, 5, 8, 1, 65536, cut.ctypes.data, C.byref(k), None)):
        assert ok(*bad) == -1, bad


def test_cpp_mirror_and_example_compile():
    host = os.path.join(ROOT, "scene-text-recognition_amd", "host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    os.path.join(host, "example_run_split.cpp")], check=True)
    txt = open(os.path.join(host, "er_filter_hip.hpp")).read()
    for name in ("set_run_split", "feet_split", "split_words", "run_splits", "cuts_from_counts", "word_split_text", "line_split_text") + FUNCS[:1] + FUNCS[2:5] + FUNCS[6:]:
        assert re.search(r"\b" + name + r"\(", txt), name


def _rows(S, rng, n_runs, hi):
    sp = np.zeros(n_runs, S.RUN_SPLIT_DTYPE)
    sp["cut"] = -1
    sp["n_cuts"] = rng.integers(0, 4, n_runs)
    sp["n_pieces"] = [len(RS.piece_nodes(int(k) + 1)) for k in sp["n_cuts"]]
    sp["first_piece"] = np.concatenate([[0], np.cumsum(sp["n_pieces"])[:-1]])
    return sp, rng.integers(0, hi, (n_runs, 65)).astype(np.uint8), rng.integers(0, hi, (int(sp["n_pieces"].sum()), 65)).astype(np.uint8)


def _ref_splits(sp):
    return [(int(s["n_cuts"]), -1, -1, -1, 0, int(s["first_piece"]), int(s["n_pieces"]), 0) for s in sp]


def test_split_words_host_equals_the_brute_force(S):
    rng = np.random.default_rng(8)
    for hi, split in ((256, 8), (256, 0), (3, 0), (16, 255), (2, 8)):
        sp, rc, pc = _rows(S, rng, 300, hi)
        first, n_of = rng.integers(0, 295, 120), rng.integers(0, 6, 120)
        hw, hp, hr = S.split_words_host(sp, rc, pc, first, n_of, split)
        bw, bp, br = RS.split_words(_ref_splits(sp), rc, pc, first, n_of, split)
        assert [tuple(int(v) for v in w) for w in hw.tolist()] == bw and [tuple(int(v) for v in p) for p in hp.tolist()] == bp and (hr == br).all()


def _call(fn, sp, rc, pc, first, n_of, cap, extra=(), rows=True, lead=()):
    """A raw call of str_er_split_words[_host]: returns (code, n_parts)."""
    ptr = lambda a: a.ctypes.data if a is not None and len(a) else None
    ws, parts, out, n = np.zeros(max(1, len(first)), np.dtype("<i4, <i4, <i4, <i4")), np.zeros((max(1, cap), 2), np.int32), np.zeros((max(1, cap), 65), np.uint8), C.c_int32(-7)
    n_pc = len(pc) if pc is not None else 9                         # (a missing table that is said to have rows)
    rc_ = fn(*lead, ptr(sp), len(sp), ptr(rc), ptr(pc), n_pc, ptr(first), ptr(n_of), len(first), *extra, ws.ctypes.data, parts.ctypes.data, cap, C.byref(n),
             out.ctypes.data if rows else None)
    return rc_, n.value


def _bad_calls(S, rng):
    """[(what, arguments of _call, the code)]: every refusal of str_er_split_words and its host twin."""
    sp, rc, pc = _rows(S, rng, 20, 256)
    first, n_of = np.array([0, 5, 19], np.int32), np.array([5, 10, 1], np.int32)
    atoms = int((sp["n_cuts"][0:5] + 1).sum() + (sp["n_cuts"][5:15] + 1).sum() + sp["n_cuts"][19] + 1)
    out = [("fine", (sp, rc, pc, first, n_of, atoms), 0), ("no part rows", (sp, rc, pc, first, n_of, atoms), 0)]
    out.append(("a window past the runs", (sp, rc, pc, first, np.array([5, 10, 2], np.int32), atoms + 4), -1))
    out.append(("a negative window", (sp, rc, pc, np.array([0, -1, 19], np.int32), n_of, atoms), -1))
    out.append(("a negative count", (sp, rc, pc, first, np.array([5, -1, 1], np.int32), atoms), -1))
    for field, value in (("n_cuts", 4), ("n_cuts", -1), ("n_pieces", 1), ("first_piece", len(pc))):
        bad = sp.copy()
        k = int(np.flatnonzero(bad["n_cuts"] > 0)[0])
        bad[field][k] = value
        out.append((f"{field} = {value}", (bad, rc, pc, first, n_of, atoms), -1))
    return sp, rc, pc, first, n_of, atoms, out


def test_split_words_host_argument_checks(S):
    L, rng = S.load_library(), np.random.default_rng(3)
    sp, rc, pc, first, n_of, atoms, calls = _bad_calls(S, rng)
    fn = L.str_er_split_words_host
    for what, args, code in calls:
        assert _call(fn, *args, extra=(8,), rows=what != "no part rows")[0] == code, what
    want = int(S.split_words_host(sp, rc, pc, first, n_of, 8)[0]["n_parts"].sum())
    assert _call(fn, sp, rc, pc, first, n_of, want, extra=(8,)) == (0, want)
    assert _call(fn, sp, rc, pc, first, n_of, want - 1, extra=(8,)) == (-7, want)                 # capacity: the count is still set
    for split in (-1, 256):
        assert _call(fn, sp, rc, pc, first, n_of, atoms, extra=(split,))[0] == -1
    assert _call(fn, sp, None, pc, first, n_of, atoms, extra=(8,))[0] == -1 and _call(fn, sp, rc, None, first, n_of, atoms, extra=(8,))[0] == -1
    assert _call(fn, sp, rc, pc, first, None, atoms, extra=(8,))[0] == -1
    assert _call(fn, sp[:0], rc[:0], pc[:0], first[:0], n_of[:0], 0, extra=(8,)) == (0, 0)


@pytest.mark.gpu
def test_context_argument_checks_leave_it_usable(S, cascade_paths):
    from test_frame_lines import _ctx
    from test_line_words import _feet
    rng = np.random.default_rng(3)
    L = S.load_library()
    f = _ctx(S, cascade_paths, max_width=320, max_height=128, max_frames=1)
    try:
        sp, rc, pc, first, n_of, atoms, calls = _bad_calls(S, rng)
        good = S.split_words_host(sp, rc, pc, first, n_of, 8)
        for what, args, code in calls:
            assert _call(L.str_er_split_words, *args, rows=what != "no part rows", lead=(f.h,))[0] == code, what
            got = f.split_words(sp, rc, pc, first, n_of)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, good)), what
        want = int(good[0]["n_parts"].sum())
        assert _call(L.str_er_split_words, sp, rc, pc, first, n_of, want - 1, lead=(f.h,)) == (-7, want)
        assert _call(L.str_er_split_words, sp, rc, pc, first, n_of, atoms, lead=(None,))[0] == -1
        for bad in ((0, 4, 8), (1, 0, 8), (65536, 4, 8), (1, 65536, 8), (1, 4, -1), (1, 4, 256)):
            with pytest.raises(S.StrErError) as e:
                f.set_run_split(*bad)
            assert e.value.code == -1 and "str_er_set_run_split" in str(e.value)
        assert L.str_er_set_run_split(None, 1, 4, 8) == -1
        assert all(a.tobytes() == b.tobytes() for a, b in zip(f.split_words(sp, rc, pc, first, n_of), good))      # (the parameters are what they were)
        # str_er_feet_split: nulls and capacities
        b = np.zeros((8, 9), bool)
        b[:, 0:3] = b[:, 6:9] = True
        b[3, 3:6] = True
        ft, bits = _feet(S, [(10, 20, b)])
        lw, runs, words = np.zeros(1, S.LINE_WORDS_DTYPE), np.zeros(4, S.LINE_RUN_DTYPE), np.zeros(4, S.LINE_WORD_DTYPE)
        splits, pieces = np.zeros(4, S.RUN_SPLIT_DTYPE), np.zeros(8, S.RUN_PIECE_DTYPE)
        nr, nw, npc = C.c_int32(), C.c_int32(), C.c_int32(-7)
        head = (f.h, 320, 128, ft.ctypes.data, bits.ctypes.data, None, 1, lw.ctypes.data, runs.ctypes.data, 4, C.byref(nr), words.ctypes.data, 4, C.byref(nw), None, None)
        fs = L.str_er_feet_split
        assert fs(*head, splits.ctypes.data, pieces.ctypes.data, 8, C.byref(npc), None, None) == 0 and (nr.value, npc.value) == (1, 2)
        assert splits[0]["n_cuts"] == 1 and splits[0]["cut"][0] == 10 + 4 and pieces[:2]["pixels"].tolist() == [24 + 1, 24 + 2]
        assert fs(*head, None, pieces.ctypes.data, 8, C.byref(npc), None, None) == -1
        assert fs(*head, splits.ctypes.data, pieces.ctypes.data, 8, None, None, None) == -1
        assert fs(*head, splits.ctypes.data, pieces.ctypes.data, -1, C.byref(npc), None, None) == -1
        assert fs(*head, splits.ctypes.data, pieces.ctypes.data, 1, C.byref(npc), None, None) == -7 and npc.value == 2       # the count is still set
        assert fs(*head, splits.ctypes.data, None, 0, C.byref(npc), None, None) == 0 and npc.value == 2                    # the pieces counted only
        reads = np.zeros(8, S.RUN_READ_DTYPE)
        assert fs(*head, splits.ctypes.data, pieces.ctypes.data, 8, C.byref(npc), reads.ctypes.data, None) == -6           # piece reads need a model
        assert "str_er_feet_split" in (L.str_er_last_error(f.h) or b"").decode()
        counting = head[:8] + (None, 0, C.byref(nr), None, 0, C.byref(nw), None, None)
        assert fs(*counting, splits.ctypes.data, pieces.ctypes.data, 8, C.byref(npc), None, None) == 0 and (nr.value, npc.value) == (1, 0)
        got = f.feet_split(320, 128, ft, bits, None, want_reads=False)
        assert got["splits"]["n_cuts"].tolist() == [1] and len(got["pieces"]) == 2 and got["piece_q"].shape == (2, 1800)
    finally:
        f.close()
