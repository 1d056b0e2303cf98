"""The block-cyclic stripe map (csrc/stripes.h: owns, count, global_index, runs) checked on the HOST against a brute-force owner map.
tests/emu/stripes_check.cpp is a stand-alone program: it is compiled here with g++ under the address and undefined-behaviour sanitizers
and run as a child process -- a stripe of 4 elements exhaustively, the product's 2^10 stripe at and around the stripe boundaries, worlds
1..9 and every rank.  The header is the text the kernels, the run-time compiled row programs and the host copies all use."""
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "sirius_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "emu", "stripes_check.cpp")


def test_stripe_map_against_brute_force(tmp_path):
    exe = str(tmp_path / "stripes_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + CSRC, SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    m = re.fullmatch(r"ok tiny=(\d+) real=(\d+)\s*", r.stdout)
    assert m, r.stdout[-1000:]
    # 45 (world, rank) pairs x every a <= b: 81 * 82 / 2 ranges of the tiny stripe, 83 * 84 / 2 of the real one
    assert (int(m.group(1)), int(m.group(2))) == (45 * 3321, 45 * 3486)


def test_header_is_plain_integer_cpp():
    """stripes.h includes nothing but <stddef.h> / <stdint.h> (hiprtc takes it as an in-memory include) and names no HIP type or call."""
    text = open(os.path.join(CSRC, "stripes.h")).read()
    assert re.findall(r"#include\s*(\S+)", text) == ["<stdint.h>", "<stddef.h>"]
    code = re.sub(r"//[^\n]*", "", text)
    assert not re.search(r"\bhip[A-Z_]\w*", code)
