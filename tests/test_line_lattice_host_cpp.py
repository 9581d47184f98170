"""The rules of the joint decode of a line over its runs' piece lattices under the host sanitizers:
tests/cpp/line_lattice_rules_check.cpp is a program of its own (with its own main) around csrc/line_lattice_rules.h -- the header the
library's host entry point runs, HIP-free -- compiled with -fsanitize=address,undefined and run on the CPU.  Nothing sanitized is
loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_line_lattice_rules_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "line_lattice_rules_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    "-Werror", os.path.join(ROOT, "tests", "cpp", "line_lattice_rules_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.endswith(" 0 wrong") and int(last.split()[0]) > 1000, out.stdout
