"""tests/devcalc (the device calculator of the field / curve arithmetic, TEST INFRASTRUCTURE) cross-compiles for gfx950 without a GPU, exports
its two entries, and holds the GENERATED device bodies: that is what tells it from the host calculator, and it shows in the binary."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT
from field29_cases import devcalc_build


def test_devcalc_builds_and_exports():
    DB = devcalc_build()
    path = DB.build()
    assert os.path.exists(path)
    assert DB.build() == path and DB.LAST_BUILD == "cached"            # the content-hash stamp: a second call compiles nothing
    lib = ctypes.CDLL(path)
    assert lib.devcalc_run and lib.devcalc_info
    assert lib.devcalc_info() == 3                                     # chained Fp29 bodies | FIPS body of Fp::mul
    # never part of the product: the product globs sirius_amd/csrc/*.hip and nothing else
    assert not os.path.exists(os.path.join(ROOT, "sirius_amd", "csrc", "devcalc.hip"))


def _kernels(asm):
    """{mangled name: body} of the functions of a device assembly listing"""
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur:
            out[cur].append(line)
            if "s_endpgm" in line or "s_setpc_b64" in line:
                cur = None
    return {k: "\n".join(v) for k, v in out.items()}


def test_devcalc_device_code_is_the_chained_form(tmp_path):
    """The device assembly of the same file with the same flags.  The Fr `mul` kernel (k_field<FrP, 0>) holds the 81 + 81 multiply-accumulates
    of one product (plus the two of its address arithmetic) and NOT the v_lshl_add_u64 that joins every column of the plain C++ body
    (field29.cuh: 16 per product) -- the instruction the chained form exists to remove.  The difference IS visible: the same kernel compiled
    without SRS_F29_CHAIN shows 164 v_mad_u64_u32 and 18 v_lshl_add_u64, with it 164 and 2 (both counts include the address arithmetic).
    The called forms keep the body out of line: one s_swappc in the kernel, the 162 in the callee."""
    DB = devcalc_build()
    out = str(tmp_path / "devcalc.s")
    r = subprocess.run(DB.command(["-S", "--cuda-device-only", "-Wno-unused-command-line-argument"], out), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    k = _kernels(open(out).read())
    find = lambda pat: [v for n, v in k.items() if re.search(pat, n)]
    (mul,) = find(r"k_fieldIN3srs3FrPELi0E")
    assert mul.count("v_mad_u64_u32") >= 162 and mul.count("v_lshl_add_u64") < 8, (mul.count("v_mad_u64_u32"), mul.count("v_lshl_add_u64"))
    (mul_ni,) = find(r"k_fieldIN3srs3FrPELi1E")
    (callee,) = find(r"mul29_calledIN3srs3FrPE")
    assert mul_ni.count("s_swappc_b64") == 1 and mul_ni.count("v_mad_u64_u32") < 16 and callee.count("v_mad_u64_u32") >= 162
    assert callee.count("v_lshl_add_u64") < 8
    (mul8,) = find(r"k_fieldIN3srs3FrPELi11E")
    assert mul8.count("v_mad_u64_u32") >= 128 and mul8.count("v_addc_co_u32") >= 128          # FIPS: one carry fold per product
    for body in k.values():                                            # every case is written with vector stores
        assert "global_store" in body or "s_setpc_b64" in body
