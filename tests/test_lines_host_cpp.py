"""The host functions of the line stage under the host sanitizers: tests/cpp/lines_host_check.cpp is a program of its own (with its own
main) that is compiled together with csrc/lines_host.cpp alone -- the file the library takes str_er_frame_lines_from_pairs,
str_er_text_tracks_from_links, str_er_hull_of_points and str_er_quad_from_hull from, HIP-free -- with -fsanitize=address,undefined
and run on the CPU.  Nothing sanitized is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scene-text-recognition_amd", "csrc")


def test_lines_host_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "lines_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    "-Werror", os.path.join(ROOT, "tests", "cpp", "lines_host_check.cpp"), os.path.join(CSRC, "lines_host.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.strip().splitlines()[-1].split()
    # 3000 random partitions with two checks for each function, 1500 random point sets with their hull: the floor of the program's own count
    assert last[1:] == ["checked,", "0", "wrong"] and int(last[0]) > 3000 * 4 + 1500, out.stdout


def test_lines_host_source_is_hip_free():
    txt = open(os.path.join(CSRC, "lines_host.cpp")).read()
    assert "hip" not in txt.replace("HIP-free", "").lower() and "str_er_ctx.h" not in txt
