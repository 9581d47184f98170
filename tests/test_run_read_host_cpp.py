"""The flag rules of STR_ER_WANT_RUN_READ, the shelf packer of the run tiles' atlas and str_er_ocr_char under the host sanitizers:
tests/cpp/run_read_rules_check.cpp is a program of its own (with its own main) that is compiled together with csrc/words_host.cpp --
the file the library takes the packer from, HIP-free -- with -fsanitize=address,undefined and run on the CPU.  Nothing sanitized is
loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scene-text-recognition_amd", "csrc")


def test_rules_packer_and_chars_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "run_read_rules_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    "-Werror", os.path.join(ROOT, "tests", "cpp", "run_read_rules_check.cpp"), os.path.join(CSRC, "words_host.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.endswith(" 0 wrong") and int(last.split()[0]) > 1000, out.stdout
