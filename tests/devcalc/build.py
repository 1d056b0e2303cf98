"""Builds the two calculators of the field / curve arithmetic (TEST INFRASTRUCTURE): tests/devcalc/libdevcalc.so from devcalc.hip with
hipcc for gfx950 and the product's own flags (build()), and tests/emu/field29_check, the host twin, with g++ (build_host()).  One compiler
call each; a content-hash stamp over the source, the headers it includes and the flags makes a second call a no-op."""
import glob
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from sirius_amd.build import CSRC, FLAGS, HIPCC  # noqa: E402

SRC = os.path.join(HERE, "devcalc.hip")
OUT = os.path.join(HERE, "libdevcalc.so")
EMU = os.path.join(ROOT, "tests", "emu")
INCLUDES = ["-I" + CSRC, "-I" + EMU]


def command(extra, out):
    """The hipcc call of the calculator with the product's flags (`extra`: what to make of it, e.g. ["-shared"] or ["-S", ...])."""
    return [HIPCC] + FLAGS + INCLUDES + extra + [SRC, "-o", out]


HOST_SRC = os.path.join(EMU, "field29_check.cpp")
HOST_OUT = os.path.join(EMU, "field29_check")
HOST_FLAGS = ["g++", "-std=c++20", "-O2", "-DSRS_EMU", "-pthread", "-Wno-unknown-pragmas", "-Wno-attributes"]      # what the stamp covers: no paths
HOST_CMD = HOST_FLAGS + ["-I" + EMU, "-I" + CSRC, HOST_SRC, "-o", HOST_OUT]


def _digest(src=SRC, flags=FLAGS):
    deps = [src, os.path.join(EMU, "field29_calc.h"), os.path.join(EMU, "hipemu.h")] + glob.glob(os.path.join(CSRC, "*.cuh")) + glob.glob(os.path.join(CSRC, "*.inc")) + \
        glob.glob(os.path.join(CSRC, "*.h"))
    h = hashlib.sha256(" ".join(flags).encode())
    for p in sorted(deps):
        if os.path.basename(p) == "jit_embed.inc":      # written by the product's build, not included here
            continue
        h.update(os.path.basename(p).encode())
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


LAST_BUILD = None      # "compiled" or "cached": what the last build() call did


def build(force=False):
    global LAST_BUILD
    tag, stamp = _digest(), OUT + ".sha"
    if not force and os.path.exists(OUT) and os.path.exists(stamp) and open(stamp).read().strip() == tag:
        LAST_BUILD = "cached"
        return OUT
    r = subprocess.run(command(["-shared"], OUT), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on devcalc.hip:\n{r.stderr[-4000:]}")
    with open(stamp, "w") as f:
        f.write(tag)
    LAST_BUILD = "compiled"
    return OUT


def build_host(force=False):
    """tests/emu/field29_check: the same operations through the headers' plain C++ bodies, a line-oriented program"""
    tag, stamp = _digest(HOST_SRC, HOST_FLAGS), HOST_OUT + ".sha"
    if not force and os.path.exists(HOST_OUT) and os.path.exists(stamp) and open(stamp).read().strip() == tag:
        return HOST_OUT
    r = subprocess.run(HOST_CMD, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"g++ failed on field29_check.cpp:\n{r.stderr[-4000:]}")
    with open(stamp, "w") as f:
        f.write(tag)
    return HOST_OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv), LAST_BUILD)
    print(build_host(force="--force" in sys.argv))
