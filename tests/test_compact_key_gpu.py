"""GPU parity of compact commitment keys (tuning msm_compact = 1 when the key is created: 8 stored windows, the other 8 through the
curve endomorphism) against the CPU oracle: every MSM flow, the scalars and bases at which the split or the flagged additions can go
wrong, and the key's bookkeeping.  Bit-exact (integer / group arithmetic)."""
import numpy as np
import pytest

from conftest import seeded_scalars
import glv_cases as G

pytestmark = pytest.mark.gpu

KEY_LOG = 15
SIZES = (1, 63, 4097, 1 << KEY_LOG)


def _dev(a):
    import torch
    return torch.from_numpy(a.view(np.int64)).cuda()


@pytest.fixture(scope="module")
def keys(srs, oracle):
    """Per curve: oracle bases of a 2^15 key and the compact key over them (shared, read-only)."""
    out = {}
    for cid in (0, 1):
        bases = oracle.make_bases(cid, 4321 + cid, 1 << KEY_LOG)
        with srs.tuning(msm_compact=1):
            ck = srs.CommitmentKey(cid, bases)
        assert ck.is_compact()
        out[cid] = (bases, ck)
    yield out
    for _, ck in out.values():
        ck.close()


@pytest.fixture(scope="module")
def cases(oracle):
    """(cid, n, kind) -> (scalars, oracle commitment over the shared bases): computed once."""
    out = {}
    for cid in (0, 1):
        bases = oracle.make_bases(cid, 4321 + cid, 1 << KEY_LOG)
        for n in SIZES:
            for kind in ("uniform", "trace"):
                sc = seeded_scalars(oracle, cid, n, 900 + n, kind)
                out[cid, n, kind] = (sc, oracle.msm(cid, sc, bases[:n]))
    return out


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("kind", ["uniform", "trace"])
@pytest.mark.parametrize("n", SIZES)
def test_compact_commit_sizes(keys, cases, cid, n, kind):
    _, ck = keys[cid]
    sc, want = cases[cid, n, kind]
    assert np.array_equal(ck.commit(sc), want)
    assert np.array_equal(ck.commit(_dev(sc)), want)


@pytest.mark.parametrize("cid", [0, 1])
def test_compact_edge_scalars(srs, oracle, cid):
    """The list of test_commit_edge_scalars plus what is special to the split: lambda (k1 = 0), lambda + 1, and the scalars with the
    largest |k1| / |k2| the host test finds at the rounding boundaries; an identity base in the key; the canonical entry."""
    from oracle import pyref as P
    from sirius_amd import _lib
    O = oracle
    q = P.CURVES[cid].q
    sf = O.SCALAR_FIELD[cid]
    n = 2048
    bases = O.make_bases(cid, 5, n)
    bases[7] = 0                       # identity point in the key
    with srs.tuning(msm_compact=1):
        ck = srs.CommitmentKey(cid, bases)
    lam, _ = G.constants(_lib.load(), cid)
    big1, big2 = G.extreme_scalars(_lib.load(), cid, q)
    for vals in ([0] * n, [1] * n, [q - 1] * n, [(1 << 128) - 1] * n, [0x8000] * n, [0x8001] * n,
                 [(i % 3) * (q - 1) // 2 for i in range(n)], [lam] * n, [lam + 1] * n, [big1] * n, [big2] * n,
                 [(big1, big2, q - big1, q - big2)[i % 4] for i in range(n)]):
        sc = O.ints_to_mont(sf, vals)
        assert np.array_equal(ck.commit(sc), O.msm(cid, sc, bases)), hex(vals[-1])
    vals = [(i * 0x9E3779B97F4A7C15) % q for i in range(n)]
    got = ck.commit(O.ints_to_limbs(vals), repr=1)
    assert np.array_equal(got, O.msm(cid, O.ints_to_mont(sf, vals), bases))
    ck.close()


def _endo_key_and_scalars(O, lib, cid, n, seed):
    """bases[2j + 1] = phi(bases[2j]) for j < 1024, bases[2049] = -phi(bases[2048]); scalars lambda d on a base and +-d on its partner:
    the k2 half of the base and the k1 half of the partner land in the same buckets as the SAME point (a doubling inside a chain)
    or as opposite points (the running sum cancels to the identity).  Several pairs share a d, so the chains have further entries."""
    from oracle import pyref as P
    q = P.CURVES[cid].q
    bf, sf = O.BASE_FIELD[cid], O.SCALAR_FIELD[cid]
    lam, beta = G.constants(lib, cid)
    beta_m = O.ints_to_mont(bf, [beta])[0]
    bases = O.make_bases(cid, 60 + cid, n)
    pairs = 1025
    bases[1:2 * pairs:2, :4] = O.fe_mul(bf, bases[0:2 * pairs:2, :4], np.repeat(beta_m[None, :], pairs, axis=0))
    bases[1:2 * pairs:2, 4:] = bases[0:2 * pairs:2, 4:]
    bases[2049, 4:] = O.fe_sub(bf, np.zeros((1, 4), np.uint64), bases[2049:2050, 4:])          # -phi(bases[2048])
    assert all(O.is_on_curve(cid, bases[i]) for i in (0, 1, 2047, 2048, 2049))
    rng = np.random.default_rng(seed)
    vals = [int.from_bytes(rng.bytes(40), "little") % q for _ in range(n)]
    for j in range(pairs):
        d = (1 + j % 37) + ((1 + j % 5) << 16) * (j % 3 == 0)         # one or two non-zero digits; a d is shared by many pairs
        vals[2 * j] = lam * d % q
        vals[2 * j + 1] = (d, q - d, q - lam * d % q, lam * d % q)[j % 4]
    return bases, O.ints_to_mont(sf, vals)


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("n", [6000, 70000])
def test_compact_endomorphism_collisions(srs, oracle, cid, n):
    from sirius_amd import _lib
    O = oracle
    bases, sc = _endo_key_and_scalars(O, _lib.load(), cid, n, n + cid)
    want = O.msm(cid, sc, bases)
    with srs.tuning(msm_compact=1):
        ck = srs.CommitmentKey(cid, bases)
    assert np.array_equal(ck.commit(_dev(sc)), want)                    # resident: the level flow
    with srs.tuning(commit_chunks=3):
        assert np.array_equal(ck.commit_upload(sc), want)               # streamed: slot mode, three sets
    assert np.array_equal(ck.commit_upload(sc), want)
    ck.close()


@pytest.mark.parametrize("cid", [0, 1])
def test_compact_pipelines(srs, oracle, keys, cases, cid):
    O = oracle
    bases, ck = keys[cid]
    n = 9001
    sc = seeded_scalars(O, cid, n, 31, "trace")
    want = O.msm(cid, sc, bases[:n])
    hb = srs.HostBuffer(n)
    hb.array[:] = sc
    before = ck.msm_stats()
    for chunks in (1, 3, 7):                                            # streamed commits, slot mode, pageable and page-locked sources
        with srs.tuning(commit_chunks=chunks):
            assert np.array_equal(ck.commit_upload(sc), want), chunks
            assert np.array_equal(ck.commit_upload(hb.array), want), chunks
    after = ck.msm_stats()
    # (a commit of one chunk is a whole MSM, outside slot mode; chunks end on stripe boundaries, so 7 is an upper bound for 9001 scalars)
    assert after["slot_sets"] - before["slot_sets"] >= 2 * (3 + 4) and after["hot_sets"] > before["hot_sets"], (before, after)
    with srs.tuning(msm_slots=0, commit_chunks=3):                      # bucket fold instead of the slots
        assert np.array_equal(ck.commit_upload(hb.array), want)
    hb.close()
    assert ck.msm_stats()["other_sets"] >= after["other_sets"] + 3
    for sort in (1, 2):                                                 # single-pass scatter / k_group + k_scatter2
        with srs.tuning(msm_sort=sort):
            v, w = cases[cid, 4097, "uniform"]
            assert np.array_equal(ck.commit(v), w), sort
            assert np.array_equal(ck.commit_upload(sc), want), sort
    vs = [cases[cid, 4097, "trace"][0], cases[cid, 63, "uniform"][0], sc]
    ws = [cases[cid, 4097, "trace"][1], cases[cid, 63, "uniform"][1], want]
    assert np.array_equal(ck.commit_batch(vs), np.stack(ws))
    # forced overflow: 4 slots per bucket and a key that does not expect hot buckets -- the first commit is run again (redo)
    with srs.tuning(msm_compact=1, msm_slot_log=2, msm_expect_ovf=0, commit_chunks=3):
        cold = srs.CommitmentKey(cid, bases[:n])
        assert np.array_equal(cold.commit_upload(sc), want)
        assert np.array_equal(cold.commit_upload(sc), want)
        st = cold.msm_stats()
        assert st["redo"] >= 1 and st["hot_sets"] >= 1, st
        cold.close()
    # three logical ranks on the one device: partial sums added on the host
    parts = []
    for r in range(3):
        with srs.tuning(msm_compact=1):
            rk = srs.CommitmentKey(cid, bases[:n], rank=r, world=3)
        assert rk.is_compact()
        parts.append(rk.commit(sc))
        rk.close()
    assert np.array_equal(srs.point_sum(cid, np.stack(parts)), want)
    with srs.tuning(msm_compact=1):
        mk = srs.CommitmentKey.create_multi(cid, bases[:n], 1)
    assert mk.is_compact() and mk.table_bytes() == 8 * n * 64
    assert np.array_equal(mk.commit(sc), want) and np.array_equal(mk.commit_upload(sc), want)
    assert np.array_equal(mk.bases(), bases[:n])
    mk.close()


def test_compact_never_takes_the_wide_windows(srs, oracle):
    O = oracle
    cid, n = 0, 1 << 13
    bases = O.make_bases(cid, 77, n)
    sc = seeded_scalars(O, cid, n, 78, "uniform")
    with srs.tuning(msm_compact=1, msm_wide=1, msm_wide_min=12):
        ck = srs.CommitmentKey(cid, bases)
        assert ck.is_compact() and not ck.has_wide_table()
        assert np.array_equal(ck.commit(_dev(sc)), O.msm(cid, sc, bases))
    ck.close()


@pytest.mark.parametrize("cid", [0, 1])
def test_compact_bookkeeping_and_default(srs, oracle, tmp_path, cid):
    O = oracle
    n = 1 << 10
    bases = O.make_bases(cid, 91, n)
    sc = seeded_scalars(O, cid, n, 92, "trace")
    want = O.msm(cid, sc, bases)
    with srs.tuning(msm_wide=0):
        full = srs.CommitmentKey(cid, bases)
        with srs.tuning(msm_compact=1):
            ck = srs.CommitmentKey(cid, bases)
    assert not full.is_compact() and ck.is_compact()                    # the tunable unset: the key of every earlier release
    assert full.table_bytes() == 16 * n * 64 and 2 * ck.table_bytes() == full.table_bytes()
    assert np.array_equal(full.commit(sc), want) and np.array_equal(ck.commit(sc), want)
    assert np.array_equal(ck.bases(), bases) and ck.count_off_curve() == 0
    ck.save_to_file(tmp_path / "compact.bin")
    full.save_to_file(tmp_path / "full.bin")
    assert (tmp_path / "compact.bin").read_bytes() == (tmp_path / "full.bin").read_bytes() == bases.tobytes()
    st = ck.msm_stats()
    assert st["other_sets"] == 1 and st["slot_sets"] == 0, st           # srs_ck_msm_stats counts a compact key's sets like any other's
    with srs.tuning(commit_chunks=2):
        assert np.array_equal(ck.commit_upload(sc[:1000]), O.msm(cid, sc[:1000], bases[:1000]))
    st = ck.msm_stats()
    assert st["slot_sets"] + st["other_sets"] >= 2 and st["other_sets"] >= 1, st
    syn = srs.CommitmentKey.setup_synthetic(cid, n, seed=3)
    with srs.tuning(msm_compact=1):
        syn_c = srs.CommitmentKey.setup_synthetic(cid, n, seed=3)
        loaded = srs.CommitmentKey.load_from_file(cid, tmp_path / "full.bin", 10)
    assert syn_c.is_compact() and loaded.is_compact() and not syn.is_compact()
    with srs.tuning(msm_compact=1):
        empty = srs.CommitmentKey(cid, bases, rank=2, world=3)            # 1024 bases are one stripe: rank 2 holds none, and is compact all the same
    assert empty.is_compact() and empty.table_bytes() == 0
    assert np.array_equal(empty.commit(sc), np.zeros(8, np.uint64))
    empty.close()
    assert np.array_equal(syn_c.bases(), syn.bases()) and np.array_equal(syn_c.commit(sc), syn.commit(sc))
    assert np.array_equal(loaded.commit(sc), want)
    for k in (full, ck, syn, syn_c, loaded):
        k.close()
