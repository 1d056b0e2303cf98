"""GPU parity of plain commitment keys of form 2 (tuning msm_plain = 2 when the key is created: the bases alone, every MSM over the split
scalar k = k1 + lambda k2 in 8 windows of two entries per scalar) against the CPU oracle: the sizes, scalars and bases at which the split
digits, the grouping into 8 populated and 8 empty segments, the flagged additions of level 0 or the Horner chain of 8 window weights can go
wrong, every entry that takes a key, the key's bookkeeping and what such a key refuses.  Bit-exact; never compared with another key form."""
import numpy as np
import pytest

from conftest import seeded_scalars
import glv_cases as G
from plain_glv_cases import (KEY_N, TUNE, boundary_vector, boundary_vector_ints, check_form2, commit_counted, dev, glv_plain_key,
                             one_bucket_ints, split_coverage)

pytestmark = pytest.mark.gpu

SIZES = (1, 511, 512, 513, KEY_N)      # around a tile of the segment passes (512 scalars), and three tiles
BIG_LOG = 13


def _q(cid):
    from oracle import pyref as P
    return P.CURVES[cid].q


def _lib():
    from sirius_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def keys(srs, oracle):
    """Per curve: oracle bases of a 1100-base key and the form-2 key over them (shared, read-only)."""
    out = {}
    for cid in (0, 1):
        bases = oracle.make_bases(cid, 911 + cid, KEY_N)
        out[cid] = (bases, glv_plain_key(srs, cid, bases))
    yield out
    for _, ck in out.values():
        ck.close()


@pytest.fixture(scope="module")
def big_keys(srs, oracle):
    """Per curve: a 2^13-base form-2 key for the other entries."""
    out = {}
    for cid in (0, 1):
        bases = oracle.make_bases(cid, 921 + cid, 1 << BIG_LOG)
        out[cid] = (bases, glv_plain_key(srs, cid, bases))
    yield out
    for _, ck in out.values():
        ck.close()


# ---- 1. form and bookkeeping ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [0, 1])
def test_plain_glv_form_and_bookkeeping(srs, oracle, keys, cid):
    """msm_plain = 2 makes a plain key of form 2 (a release without the form makes a 16-window key here), msm_plain = 1 one of form 1, and
    nothing set the default key, each with its table size."""
    O = oracle
    bases, ck = keys[cid]
    assert ck.plain_form() == 2 and ck.is_plain() is True
    assert not ck.is_compact() and not ck.has_wide_table() and ck.table_bytes() == 64 * KEY_N
    assert np.array_equal(ck.bases(), bases) and ck.count_off_curve() == 0
    n = 600
    with srs.tuning(**TUNE):
        empty = srs.CommitmentKey(cid, bases[:0])
        syn = srs.CommitmentKey.setup_synthetic(cid, n, seed=3)
    check_form2(empty, 0)
    check_form2(syn, n)
    assert not empty.commit_batch([np.zeros((0, 4), np.uint64)]).any()          # an empty vector: the identity (0, 0)
    sc = seeded_scalars(O, cid, n, 5, "trace")
    assert np.array_equal(syn.commit(sc), O.msm(cid, sc, syn.bases()))
    with srs.tuning(msm_plain=1):
        one = srs.CommitmentKey(cid, bases[:n])
    full = srs.CommitmentKey(cid, bases[:n])
    assert one.plain_form() == 1 and one.is_plain() is True and one.table_bytes() == 64 * n
    assert full.plain_form() == 0 and full.is_plain() is False and full.table_bytes() == 16 * 64 * n
    for key in (one, full):
        assert np.array_equal(key.commit(sc), O.msm(cid, sc, bases[:n]))
    for key in (empty, syn, one, full):
        key.close()


# ---- 2. the boundary vector -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def boundary_cases(oracle, keys):
    """cid -> (Montgomery scalars, the same as canonical limbs, {n: oracle commitment of the first n}): computed once."""
    O = oracle
    out = {}
    for cid in (0, 1):
        sc = boundary_vector(O, _lib(), cid, _q(cid), KEY_N, 4)
        canon = O.ints_to_limbs(O.mont_to_ints(O.SCALAR_FIELD[cid], sc))
        out[cid] = (sc, canon, {n: O.msm(cid, np.ascontiguousarray(sc[:n]), keys[cid][0][:n]) for n in SIZES})
    return out


@pytest.mark.parametrize("cid", [0, 1])
def test_plain_glv_boundary_vector_covers_the_split(cid):
    """A condition on the inputs: all four sign pairs of (k1, k2), a scalar with k1 = 0 and one with k2 = 0, by the host entry that runs
    the digit kernel's split -- and within the first 511 scalars, so that every size above 1 sees them."""
    vals = boundary_vector_ints(_lib(), cid, _q(cid))
    assert len(vals) <= 511
    signs, k1_zero, k2_zero = split_coverage(_lib(), cid, vals)
    assert signs == {(False, False), (False, True), (True, False), (True, True)} and k1_zero and k2_zero


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_plain_glv_boundary_vector(oracle, keys, boundary_cases, cid, n):
    _, ck = keys[cid]
    sc, canon, want = boundary_cases[cid]
    sc, canon, want = np.ascontiguousarray(sc[:n]), np.ascontiguousarray(canon[:n]), want[n]
    assert np.array_equal(commit_counted(ck, dev(sc)), want)                     # device, Montgomery form
    assert np.array_equal(commit_counted(ck, dev(canon), repr=1), want)          # device, canonical form
    assert np.array_equal(commit_counted(ck, sc), want)                          # host memory
    assert np.array_equal(commit_counted(ck, canon, repr=1), want)
    st = ck.msm_stats()
    assert st["slot_sets"] == 0 and st["hot_sets"] == 0 and st["redo"] == 0, st


@pytest.mark.parametrize("cid", [0, 1])
def test_plain_glv_single_scalars(oracle, keys, cid):
    """n = 1 with each scalar of the boundary list's split part alone: a wrong digit cannot cancel against another."""
    O = oracle
    bases, ck = keys[cid]
    lam, _ = G.constants(_lib(), cid)
    q = _q(cid)
    vals = G.fixed_scalars(q, lam) + list(G.extreme_scalars(_lib(), cid, q)) + [(lam << 112) % q, q - lam]
    for v in vals:
        sc = O.ints_to_mont(O.SCALAR_FIELD[cid], [v])
        assert np.array_equal(ck.commit(dev(sc)), O.msm(cid, sc, bases[:1])), hex(v)


# ---- 3. one bucket --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [0, 1])
def test_plain_glv_one_bucket(oracle, keys, cid):
    """1100 equal scalars: every entry of a window falls into one bucket -- flagged and unflagged ones mixed where both halves are non-zero
    (2200 entries in parts of 4: more parts than the 512 the wave-level pass takes, so level 1 runs on them)."""
    O = oracle
    bases, ck = keys[cid]
    lam, _ = G.constants(_lib(), cid)
    for x in one_bucket_ints(lam, _q(cid)):
        sc = O.ints_to_mont(O.SCALAR_FIELD[cid], [x] * KEY_N)
        assert np.array_equal(ck.commit(dev(sc)), O.msm(cid, sc, bases)), hex(x)


# ---- 4. degenerate bases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [0, 1])
def test_plain_glv_degenerate_bases(srs, oracle, cid):
    """Bases P, phi(P), -phi(P), phi^2(P), the identity, then ordinary ones: a flagged entry of P and a plain entry of +-phi(P) meet in one
    bucket as the same point (the doubling branch) or as opposite points (the sum cancels), and P + phi(P) + phi^2(P) = O."""
    O = oracle
    q, sf, bf = _q(cid), O.SCALAR_FIELD[cid], O.BASE_FIELD[cid]
    lam, beta = G.constants(_lib(), cid)
    beta_m = O.ints_to_mont(bf, [beta])
    bases = O.make_bases(cid, 931 + cid, KEY_N)
    P0 = bases[0].copy()
    phi = P0.copy()
    phi[:4] = O.fe_mul(bf, P0[None, :4], beta_m)[0]
    neg_phi = phi.copy()
    neg_phi[4:] = O.fe_sub(bf, np.zeros((1, 4), np.uint64), phi[None, 4:])[0]
    phi2 = phi.copy()
    phi2[:4] = O.fe_mul(bf, phi[None, :4], beta_m)[0]
    bases[1], bases[2], bases[3], bases[4] = phi, neg_phi, phi2, 0
    assert all(O.is_on_curve(cid, bases[i]) for i in range(4))
    # beta matches lambda: [lambda] P = phi(P) by the oracle
    assert np.array_equal(O.msm(cid, O.ints_to_mont(sf, [lam]), bases[:1]), phi)
    ck = glv_plain_key(srs, cid, bases)
    fill = O.mont_to_ints(sf, seeded_scalars(O, cid, KEY_N, 932, "uniform"))
    for d in (1, 0x7FFF, 0x8000):
        for head, name in (([lam * d % q, d], "double"), ([lam * d % q, 0, d], "cancel")):
            for rest in ([0] * (KEY_N - len(head)), fill[len(head):]):
                sc = O.ints_to_mont(sf, head + list(rest))
                want = O.msm(cid, sc, bases)
                assert np.array_equal(ck.commit(dev(sc)), want), (name, hex(d), rest[0] != 0)
                if name == "cancel" and rest[0] == 0:
                    assert not want.any()                                        # the identity: the all-zero affine encoding
    for rest in ([0] * (KEY_N - 4), fill[4:]):
        sc = O.ints_to_mont(sf, [1, 1, 0, 1] + list(rest))
        want = O.msm(cid, sc, bases)
        assert np.array_equal(ck.commit(dev(sc)), want), "P + phi(P) + phi^2(P)"
        if rest[0] == 0:
            assert not want.any()
    assert ck.count_off_curve() == 0
    ck.close()


# ---- 5. consumers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [0, 1])
def test_plain_glv_batch_and_streamed(srs, oracle, big_keys, cid):
    O = oracle
    bases, ck = big_keys[cid]
    vs = [seeded_scalars(O, cid, n, 40 + n, "uniform") for n in (300, 63, 1)] + [np.zeros((0, 4), np.uint64)]
    ws = [O.msm(cid, v, bases[:len(v)]) for v in vs[:3]] + [np.zeros(8, np.uint64)]
    before = ck.msm_stats()
    assert np.array_equal(ck.commit_batch(vs), np.stack(ws))
    assert np.array_equal(ck.commit_batch([dev(v) for v in vs[:3]]), np.stack(ws[:3]))
    m = 4500                                                                     # three chunks: the second and third start at a non-zero base
    sc = seeded_scalars(O, cid, m, 31, "trace")
    want = O.msm(cid, sc, bases[:m])
    hb = srs.HostBuffer(m)
    hb.array[:] = sc
    with srs.tuning(commit_chunks=3):
        mid = ck.msm_stats()
        assert np.array_equal(ck.commit_upload(sc), want)                        # pageable source
        assert np.array_equal(ck.commit_upload(hb.array), want)                  # page-locked source
        after = ck.msm_stats()
    hb.close()
    assert after["other_sets"] >= mid["other_sets"] + 2 * 3, (mid, after)
    # msm_stats counts other_sets only
    assert after["other_sets"] > before["other_sets"]
    assert (after["slot_sets"], after["hot_sets"], after["redo"]) == (0, 0, 0), after


@pytest.mark.parametrize("cid", [0, 1])
def test_plain_glv_is_sat_witness_commit(srs, oracle, big_keys, cid):
    from workloads import rand_fe
    S, O = srs, oracle
    bases, ck = big_keys[cid]
    rng = np.random.default_rng(95 + cid)
    W = [rand_fe(rng, 5001, 0.5), rand_fe(rng, 1 << 11, 0.5)]
    E = rand_fe(rng, 700)
    cw = np.stack([O.msm(cid, w, bases[:len(w)]) for w in W])
    ce = O.msm(cid, E, bases[:len(E)])
    assert S.VanillaFS.is_sat_witness_commit(ck, W, cw, E, ce) == (0, False)
    assert S.VanillaFS.is_sat_witness_commit(ck, [dev(w) for w in W], cw) == (0, False)
    W[1][7] = rand_fe(rng, 1)[0]                                        # one witness element changed: that round is reported
    assert S.VanillaFS.is_sat_witness_commit(ck, W, cw, E, ce) == (1, False)
    E[0] = rand_fe(rng, 1)[0]
    assert S.VanillaFS.is_sat_witness_commit(ck, W, cw, E, ce) == (1, True)
    st = ck.msm_stats()
    assert (st["slot_sets"], st["hot_sets"], st["redo"]) == (0, 0, 0), st


def test_plain_glv_commit_cross_terms(srs, oracle, big_keys):
    """srs_commit_cross_terms on a 2^10-row MainGate structure: every commitment is the oracle's MSM of the term it commits to."""
    from workloads import gates_for, rand_fe
    S, O = srs, oracle
    cid = field = 0
    bases, ck = big_keys[cid]
    k, rows, gate_T = 10, 1 << 10, [5, 3]
    gates, nfix, nadv = gates_for(gate_T)
    rng = np.random.default_rng(97)
    fixed = [rand_fe(rng, rows, 0.3) for _ in range(nfix)]
    St = S.PlonkStructure(field, k, [], fixed, nadv, gates)
    y1, y2, u1 = rand_fe(rng, St.num_challenges), rand_fe(rng, St.num_challenges), rand_fe(rng, 1)[0]
    W1, W2 = rand_fe(rng, nadv * rows), rand_fe(rng, nadv * rows)
    terms, _ = S.VanillaFS.commit_cross_terms(None, St, y1, u1, W1, y2, W2)     # the evaluation half alone: no key
    want = np.stack([O.msm(cid, np.ascontiguousarray(t), bases[:len(t)]) for t in terms])
    before = ck.msm_stats()
    _, commits = S.VanillaFS.commit_cross_terms(ck, St, y1, u1, W1, y2, W2)
    assert np.array_equal(commits, want)
    _, commits = S.VanillaFS.commit_cross_terms(ck, St, y1, u1, dev(W1), y2, dev(W2), want_terms=False)
    assert np.array_equal(commits, want)
    after = ck.msm_stats()
    assert after["other_sets"] > before["other_sets"] and (after["slot_sets"], after["hot_sets"], after["redo"]) == (0, 0, 0), after
    St.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_plain_glv_refusals(srs, oracle, tmp_path):
    O = oracle
    n = 1 << 10
    bases = O.make_bases(0, 961, n)
    bases.tofile(tmp_path / "key.bin")

    def refused(make, *names):
        with pytest.raises(srs.SiriusAmdError) as e:
            make().close()
        assert e.value.rc == 4, e.value                                 # SRS_ERR_INVALID
        assert all(name in str(e.value) for name in names), e.value

    for compact in (1, 2):
        with srs.tuning(msm_plain=2, msm_compact=compact):
            refused(lambda: srs.CommitmentKey(0, bases), "msm_plain = 2", f"msm_compact = {compact}")
            refused(lambda: srs.CommitmentKey.setup_synthetic(0, n, seed=1), "msm_plain = 2", f"msm_compact = {compact}")
    with srs.tuning(**TUNE):
        refused(lambda: srs.CommitmentKey(0, bases, rank=1, world=2), "msm_plain = 2")
        refused(lambda: srs.CommitmentKey.setup_synthetic(0, n, seed=1, rank=0, world=2), "msm_plain = 2")
        refused(lambda: srs.CommitmentKey.load_from_file(0, tmp_path / "key.bin", 10, rank=1, world=2), "msm_plain = 2")
        refused(lambda: srs.CommitmentKey.create_multi(0, bases, 2), "msm_plain = 2")
        refused(lambda: srs.CommitmentKey.setup_synthetic_multi(0, n, seed=1, n_devices=2), "msm_plain = 2")
        one = srs.CommitmentKey.create_multi(0, bases, 1)               # one shard on one device is a plain key like any other
    check_form2(one, n)
    sc = seeded_scalars(O, 0, n, 962, "uniform")
    want = O.msm(0, sc, bases)
    assert np.array_equal(one.commit(sc), want) and np.array_equal(one.commit_upload(sc), want)
    one.close()
    full = srs.CommitmentKey(0, bases)                                  # a default key can still be created and used afterwards
    assert full.plain_form() == 0 and full.table_bytes() == 16 * n * 64 and np.array_equal(full.commit(sc), want)
    full.close()


# ---- 7. one size where tiles, segments and levels are all multiple ---------------------------------------------------------------------
def test_plain_glv_many_tiles(srs, oracle):
    O = oracle
    cid, n = 0, 1 << 17
    bases = O.make_bases(cid, 971, n)
    ck = glv_plain_key(srs, cid, bases)
    for kind in ("uniform", "trace"):
        sc = seeded_scalars(O, cid, n, 972, kind)
        assert np.array_equal(commit_counted(ck, dev(sc)), O.msm(cid, sc, bases)), kind
    ck.close()
