"""The generated device sources under sirius_amd/csrc are what their generators emit today (no hand edits, no stale output).
rowprog_spec.inc comes out of the library's own row-program compiler, so its generator runs on the CPU emulator build."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("gen,inc", [("gen_field_fips.py", "field_fips.inc"), ("gen_field29_chain.py", "field29_chain.inc")])
def test_generated_inc_is_current(tmp_path, gen, inc):
    out = tmp_path / inc
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", gen), str(out)], stdout=subprocess.DEVNULL)
    assert out.read_text() == open(os.path.join(ROOT, "sirius_amd", "csrc", inc)).read(), f"{inc} is not what tools/{gen} generates"


def test_rowprog_spec_inc_is_current(tmp_path):
    emu_dir = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["make", "-C", emu_dir, "-j4"], stdout=subprocess.DEVNULL)        # as tests/test_emu_jit.py builds it
    out = tmp_path / "rowprog_spec.inc"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_rowprog_spec.py"), str(out)], stdout=subprocess.DEVNULL)
    committed = open(os.path.join(ROOT, "sirius_amd", "csrc", "rowprog_spec.inc"), "rb").read()
    assert out.read_bytes() == committed, "rowprog_spec.inc is not what tools/gen_rowprog_spec.py generates"
