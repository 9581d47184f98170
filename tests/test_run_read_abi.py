"""CPU checks of the run reading (STR_ER_WANT_RUN_READ, str_er_feet_read, str_er_ocr_char): header, record layout, exports, binding,
the C++ mirror and example, and str_er_ocr_char, every value with ==."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

import run_read_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "str_er.h")
HOST = os.path.join(ROOT, "scene-text-recognition_amd", "host")
FUNCS = ("str_er_result_run_reads", "str_er_result_run_features", "str_er_feet_read", "str_er_ocr_char", "str_er_run_atlas_stats")
READ = (("label", 0), ("ch", 4), ("prob", 8))


def test_header_declares_the_flag_the_record_and_the_prototypes():
    full = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert re.search(r"#define\s+STR_ER_WANT_RUN_READ\s+\(2097152u\)", txt)
    assert re.search(r"typedef\s+struct\s+str_er_run_read\s*\{\s*int32_t\s+label;\s*int32_t\s+ch;\s*double\s+prob;\s*\}\s*str_er_run_read;", txt)
    assert re.search(r"const\s+str_er_run_read\s*\*\s*str_er_result_run_reads\s*\(\s*const\s+str_er_result\s*\*\s*r\s*,\s*int32_t\s*\*\s*n\s*\)", txt)
    assert re.search(r"const\s+uint8_t\s*\*\s*str_er_result_run_features\s*\(\s*const\s+str_er_result\s*\*\s*r\s*,\s*uint64_t\s*\*\s*n_bytes\s*\)", txt)
    assert re.search(r"int32_t\s+str_er_ocr_char\s*\(\s*int32_t\s+label\s*\)", txt)
    assert re.search(r"int\s+str_er_feet_read\s*\(\s*str_er_ctx\s*\*\s*ctx\s*,\s*int32_t\s+W\s*,\s*int32_t\s+H\s*,\s*const\s+str_er_line_foot\s*\*\s*feet\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*bits\s*,\s*const\s+double\s*\*\s*slopes\s*,\s*int32_t\s+n\s*,", txt)
    # the contract says what the slope is, and what is not done
    for words in ("used as it is", "no spelling correction and no language model", "touching glyphs reads as one character", "the caller filters"):
        assert words in re.sub(r"\s*\n \*\s*", " ", full), words


def test_record_layout_c99(tmp_path):
    src = tmp_path / "t.c"
    at = " && ".join(f"offsetof(str_er_run_read, {f}) == {o}" for f, o in READ)
    src.write_text('#include <stddef.h>\n#include "str_er.h"\n'
                   f"typedef char read_ok[sizeof(str_er_run_read) == 16 && {at} ? 1 : -1];\n"
                   "typedef char fl[STR_ER_WANT_RUN_READ == 2097152u && STR_ER_WANT_RUN_READ == (1u << 21) && STR_ER_WANT_LINE_WORDS == (1u << 20) ? 1 : -1];\n"
                   "typedef int (*read_fn)(str_er_ctx *, int32_t, int32_t, const str_er_line_foot *, const uint32_t *, const double *, int32_t,"
                   " str_er_line_words *, str_er_line_run *, int32_t, int32_t *, str_er_line_word *, int32_t, int32_t *, str_er_run_read *, uint8_t *);\n"
                   "int main(void) { read_ok a; fl b; read_fn f = str_er_feet_read; int32_t (*g)(int32_t) = str_er_ocr_char;\n"
                   "  const str_er_run_read *(*p)(const str_er_result *, int32_t *) = str_er_result_run_reads;\n"
                   "  const uint8_t *(*q)(const str_er_result *, uint64_t *) = str_er_result_run_features;\n"
                   "  (void)a; (void)b; (void)f; (void)g; (void)p; (void)q; return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_library_exports_the_symbols(S):
    L = S.load_library()
    for name in FUNCS:
        assert hasattr(L, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", S.lib_path()], capture_output=True, text=True, check=True).stdout
    for name in FUNCS:
        assert re.search(r"\bT\s+" + name + r"\b", out), name
    assert re.search(r"\bk_run_tiles\b", subprocess.run(["nm", "-C", S.lib_path()], capture_output=True, text=True, check=True).stdout)


def test_ocr_char(S):
    L = S.load_library()
    want = {0: "0", 9: "9", 10: "A", 35: "Z", 36: "a", 61: "z", 62: "&", 64: ")", 65: "?", -1: "?"}
    for label, ch in want.items():
        assert L.str_er_ocr_char(label) == ord(ch) and S.ocr_char(label) == ch == RR.ocr_char(label), label
    assert "".join(S.ocr_char(k) for k in range(65)) == RR.TABLE and len(RR.TABLE) == 65
    assert S.ocr_char(2 ** 31 - 1) == "?" and S.ocr_char(-2 ** 31) == "?"


def test_binding_constants_dtypes_and_keywords(S):
    assert S.WANT_RUN_READ == 1 << 21 == 2097152
    d = S.RUN_READ_DTYPE
    assert d.itemsize == 16 and tuple((n, d.fields[n][1]) for n in d.names) == READ
    for m in ("text_detect", "text_detect_list"):
        assert inspect.signature(getattr(S.ERFilter, m)).parameters["want_run_read"].default is False
    for m in ("submit", "submit_nv12", "submit_copy", "submit_list", "submit_nv12_list", "submit_copy_list"):
        assert inspect.signature(getattr(S.FrameStream, m)).parameters["want_run_read"].default is False
    binding = __import__("importlib").import_module("scene-text-recognition_amd.binding")
    assert binding._want_flags(run_read=True) == 2097152 and binding._want_flags(run_read=True, line_words=True) == 2097152 | 1048576
    assert callable(S.ERFilter.feet_read) and callable(S.ERFilter.run_atlas_stats) and callable(S.FrameStream.load_svm_model)
    for m in ("run_reads", "run_features"):
        assert isinstance(getattr(S.Result, m), property)
    for m in ("word_text", "words_text_of_line", "frame_line_text"):
        assert callable(getattr(S.Result, m))


def test_result_accessors_without_the_flag(S):
    r = S.Result.__new__(S.Result)
    r._run_reads = r._run_features = None
    for name in ("run_reads", "run_features"):
        with pytest.raises(ValueError):
            getattr(r, name)
    L = S.load_library()
    n = C.c_int32(7)
    assert L.str_er_result_run_reads(None, n) is None and n.value == 0
    nb = C.c_uint64(7)
    assert L.str_er_result_run_features(None, nb) is None and nb.value == 0


def test_cpp_mirror_and_example_compile():
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    os.path.join(HOST, "example_read_words.cpp")], check=True)
