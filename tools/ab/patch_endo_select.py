"""A/B build of the compact keys' level 0 (profiles/compact_key_ab.txt section 4b): the per-lane endomorphism flag as an UNCONDITIONAL product
of the gathered x with beta-or-one instead of the library's branch.
    python tools/ab/patch_endo_select.py sirius_amd/csrc/msm.hip /tmp/msm_select.hip && python tools/build_variant.py select msm.hip @/tmp/msm_select.hip
    SRS_AMD_LIB=variants/select.so SRS_TEST_TUNING=msm_compact=1 python tools/msm_probe.py 24 16777216"""
import sys
s = open(sys.argv[1]).read()
old = '''        if (v & PAY_ENDO) {
            f29_t beta;
#pragma unroll
            for (int i = 0; i < 9; ++i) beta.v[i] = GlvConsts<C::ID>::beta29(i);
            q.x = Ec29<C>::F::mul(q.x, beta);        // < 2P norm: within the bounds of every use of a table x (curve29.cuh)
        }'''
new = '''        f29_t f;
#pragma unroll
        for (int i = 0; i < 9; ++i) f.v[i] = (v & PAY_ENDO) ? GlvConsts<C::ID>::beta29(i) : Ec29<C>::one_limb(i);
        q.x = Ec29<C>::F::mul(q.x, f);'''
assert s.count(old) == 1, "load_entry has changed: re-anchor the patch"
open(sys.argv[2], "w").write(s.replace(old, new))
