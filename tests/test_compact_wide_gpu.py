"""GPU parity of compact commitment keys that also carry the wide table (tuning msm_compact = 2 when the key is created: 8 narrow
windows + 7 wide ones, the other halves through the curve endomorphism) against the CPU oracle.  The wide flow -- 7 signed 20-bit digits
of |k1| and 7 of |k2| per scalar -- is forced on sizes the oracle can do (msm_wide = 1, msm_wide_min = 0): sizes around the 512-scalar
tile of the segment passes, the digit boundaries of a half, every entry in one bucket, P and phi(P) meeting in a bucket, the other MSM
flows on a key that holds both tables, and the settings under which such a key stays narrow.  Bit-exact (integer / group arithmetic)."""
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, seeded_scalars, tune_env
from compact_wide_cases import TUNE, boundary_ints, check_bookkeeping, commit_counted, compact_wide_key, dev, one_bucket_ints

pytestmark = pytest.mark.gpu

KEY_N = 3000
SIZES = (1, 5, 513, KEY_N)          # 513: one scalar past a tile of the segment passes


@pytest.fixture(scope="module")
def keys(srs, oracle):
    """Per curve: oracle bases of a 3000-base key and the msm_compact = 2 key over them (shared, read-only)."""
    out = {}
    for cid in (0, 1):
        bases = oracle.make_bases(cid, 5321 + cid, KEY_N)
        out[cid] = (bases, compact_wide_key(srs, cid, bases))
    yield out
    for _, ck in out.values():
        ck.close()


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("kind", ["uniform", "trace"])
@pytest.mark.parametrize("n", SIZES)
def test_compact_wide_sizes(srs, oracle, keys, cid, n, kind):
    bases, ck = keys[cid]
    sc = seeded_scalars(oracle, cid, n, 700 + n, kind)
    want = oracle.msm(cid, sc, bases[:n])
    with srs.tuning(**TUNE):
        assert np.array_equal(commit_counted(ck, dev(sc)), want)
        assert np.array_equal(commit_counted(ck, sc), want)


@pytest.mark.parametrize("cid,n,kind", [(0, 70000, "uniform"), (1, 33333, "trace")])
def test_compact_wide_many_tiles(srs, oracle, cid, n, kind):
    """Several tiles of the segment passes, all 16 segments in use, hot low buckets (trace)."""
    bases = oracle.make_bases(cid, 4, n)
    ck = compact_wide_key(srs, cid, bases)
    with srs.tuning(**TUNE):
        for j in range(2):
            sc = seeded_scalars(oracle, cid, n, 9 + j, kind)
            assert np.array_equal(commit_counted(ck, dev(sc)), oracle.msm(cid, sc, bases)), j
    ck.close()


@pytest.mark.parametrize("cid", [0, 1])
def test_compact_wide_digit_boundaries(srs, oracle, cid):
    from oracle import pyref as P
    from sirius_amd import _lib
    O = oracle
    q = P.CURVES[cid].q
    vals = boundary_ints(_lib.load(), cid, q)
    sc = O.ints_to_mont(O.SCALAR_FIELD[cid], vals)
    bases = O.make_bases(cid, 6, len(vals))
    want = O.msm(cid, sc, bases)
    ck = compact_wide_key(srs, cid, bases)
    with srs.tuning(**TUNE):
        assert np.array_equal(commit_counted(ck, dev(sc)), want)
        assert np.array_equal(commit_counted(ck, O.ints_to_limbs(vals), repr=1), want)         # canonical scalars
        for i in range(0, len(vals), 4):                                # the four forms of one value on their own: a wrong digit cannot cancel
            part = sc[i:i + 4]
            assert np.array_equal(ck.commit(dev(part)), O.msm(cid, part, bases[:len(part)])), [hex(v) for v in vals[i:i + 4]]
    ck.close()


@pytest.mark.parametrize("cid", [0, 1])
def test_compact_wide_one_bucket(srs, oracle, keys, cid):
    """3000 equal scalars: every entry of a digit row in one bucket of one segment (parts of one bucket through the levels)."""
    from oracle import pyref as P
    from sirius_amd import _lib
    O = oracle
    bases, ck = keys[cid]
    with srs.tuning(**TUNE):
        for x in one_bucket_ints(_lib.load(), cid, P.CURVES[cid].q):
            sc = O.ints_to_mont(O.SCALAR_FIELD[cid], [x] * KEY_N)
            assert np.array_equal(commit_counted(ck, dev(sc)), O.msm(cid, sc, bases)), hex(x)


@pytest.mark.parametrize("cid", [0, 1])
def test_compact_wide_endomorphism_collisions(srs, oracle, cid):
    """P and phi(P) meet in one bucket of the wide flow as equal points (a doubling inside a chain) and as opposite points (the running
    sum cancels): the key and scalars of the narrow compact test, n = 6000, resident commit."""
    from sirius_amd import _lib
    from test_compact_key_gpu import _endo_key_and_scalars
    n = 6000
    bases, sc = _endo_key_and_scalars(oracle, _lib.load(), cid, n, n + cid)
    ck = compact_wide_key(srs, cid, bases)
    with srs.tuning(**TUNE):
        assert np.array_equal(commit_counted(ck, dev(sc)), oracle.msm(cid, sc, bases))
    ck.close()


@pytest.mark.parametrize("cid", [0, 1])
def test_compact_wide_other_flows(srs, oracle, cid):
    from oracle import pyref as P
    O = oracle
    q = P.CURVES[cid].q
    sf = O.SCALAR_FIELD[cid]
    n = 1 << 14
    bases = O.make_bases(cid, 15 + cid, n)
    bases[7] = 0                                                        # an identity base in the key
    ck = compact_wide_key(srs, cid, bases)
    m = 9001
    sc = seeded_scalars(O, cid, n, 31, "trace")
    want_m, want_n = O.msm(cid, sc[:m], bases[:m]), O.msm(cid, sc, bases)
    with srs.tuning(**TUNE):
        assert np.array_equal(commit_counted(ck, dev(sc[:m])), want_m)
        vals = [(i * 0x9E3779B97F4A7C15) % q for i in range(2048)]      # canonical scalars
        assert np.array_equal(ck.commit(O.ints_to_limbs(vals), repr=1), O.msm(cid, O.ints_to_mont(sf, vals), bases[:2048]))
        # a batch runs the narrow flow on a key that holds both tables
        vs = [sc[:m], seeded_scalars(O, cid, 63, 8, "uniform"), sc[:4097]]
        ws = [want_m, O.msm(cid, vs[1], bases[:63]), O.msm(cid, sc[:4097], bases[:4097])]
        assert np.array_equal(ck.commit_batch(vs), np.stack(ws))
        for chunks in (1, 3):                                           # one chunk: a whole MSM; three: slot mode on the narrow strides
            with srs.tuning(commit_chunks=chunks):
                assert np.array_equal(ck.commit_upload(sc[:m]), want_m), chunks
    with srs.tuning(msm_compact=2, msm_wide=1, msm_wide_min=14):        # one key, both flows: below the threshold narrow, from it wide
        assert np.array_equal(commit_counted(ck, dev(sc[:m])), want_m)
        assert np.array_equal(commit_counted(ck, dev(sc)), want_n)
    ck.close()
    with srs.tuning(**TUNE):
        parts = []
        for r in range(3):                                              # three logical ranks on the one device, summed on the host
            rk = compact_wide_key(srs, cid, bases[:m], rank=r, world=3)
            parts.append(commit_counted(rk, dev(sc[:m])))
            rk.close()
        assert np.array_equal(srs.point_sum(cid, np.stack(parts)), want_m)
        mk = srs.CommitmentKey.create_multi(cid, bases[:m], 1)
        check_bookkeeping(mk, m)
        assert np.array_equal(mk.commit(dev(sc[:m])), want_m) and np.array_equal(mk.commit_upload(sc[:m]), want_m)
        assert np.array_equal(mk.bases(), bases[:m])
        mk.close()


@pytest.mark.parametrize("cid", [0, 1])
def test_compact_wide_fall_through(srs, oracle, cid):
    """msm_compact = 2 only ALLOWS the wide table: msm_wide = 0 refuses it, and unset the key-size rule decides (2^13 bases: none)."""
    O = oracle
    n = 1 << 13
    bases = O.make_bases(cid, 77, n)
    sc = seeded_scalars(O, cid, n, 78, "uniform")
    want = O.msm(cid, sc, bases)
    with srs.tuning(msm_compact=2, msm_wide=0, msm_wide_min=0):
        ck = srs.CommitmentKey(cid, bases)
        assert ck.is_compact() and not ck.has_wide_table() and ck.table_bytes() == 8 * n * 64
        assert np.array_equal(ck.commit(dev(sc)), want) and np.array_equal(ck.commit_upload(sc), want)
    ck.close()
    with srs.tuning(msm_compact=2):
        ck = srs.CommitmentKey(cid, bases)
        assert ck.is_compact() and not ck.has_wide_table() and ck.table_bytes() == 8 * n * 64
        assert np.array_equal(ck.commit(dev(sc)), want)
    ck.close()


def test_compact_wide_equals_compact_narrow_at_scale(srs):
    """3 * 2^20 + 77 trace-like device scalars on a synthetic key: msm_compact = 2 through the wide flow against msm_compact = 1, one
    subprocess each -- same seeded inputs, same affine point."""
    code = (
        "import sys, numpy as np, torch; sys.path.insert(0, '.')\n"
        "import sirius_amd as S\n"
        "n = (3 << 20) + 77\n"
        "ck = S.CommitmentKey.setup_synthetic(0, n, seed=21)\n"
        "g = torch.Generator(device='cuda').manual_seed(8)\n"
        "v = torch.randint(0, 1 << 62, (n, 4), dtype=torch.int64, device='cuda', generator=g); v[:, 3] &= (1 << 60) - 1\n"
        "v[torch.rand(n, device='cuda', generator=g) < 0.5] = 0\n"
        "v[torch.rand(n, device='cuda', generator=g) < 0.2, 1:] = 0\n"
        "print('K', int(ck.is_compact()), int(ck.has_wide_table()), ck.table_bytes() // (64 * n))\n"
        "print('C', ck.commit(v).tobytes().hex())\n")
    outs = []
    for env, form in ((tune_env(msm_compact=1), "K 1 0 8"), (tune_env(msm_compact=2, msm_wide=1, msm_wide_min=20), "K 1 1 15")):
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-1500:]
        assert form in r.stdout.splitlines(), r.stdout[-300:]
        outs.append([l for l in r.stdout.splitlines() if l.startswith("C ")][-1])
    assert outs[0] == outs[1] and len(outs[0]) > 100
