"""GPU parity: PlonkStructure::run_sps_protocol (src/plonk/mod.rs:413-662) as one library call -- srs_run_sps_protocol -- against the
literal protocol composed from oracle parts (tests/sps_cases.py): every round vector, commitment and challenge bit for bit, the
step-wise calls under the same challenges, the commitment and gate / log-derivative deciders on the returned device vector.

Keys: synthetic, 2^14 bases per curve.  k = 5 is the reference's own size; k = 11 = 2 x 1024 rows gives two h/g workgroups of
128 x 8 and eight 256-thread table blocks per lookup, so a wrong per-lookup offset or block bound shows.  Round 0 of the "two"
variant at k = 11 is 9 * 2^11 elements, more than 2^14: that one case brings its own key of exactly that length."""
import numpy as np
import pytest

import space_cases as SC
import sps_cases as SPS

pytestmark = pytest.mark.gpu

BN256, GRUMPKIN = 0, 1
FR_MODULUS = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001


@pytest.fixture
def sp():
    return SC.Spaces.torch_cuda()


def _key(srs, curve, n):
    ck = srs.CommitmentKey.setup_synthetic(curve, n, seed=21 + curve)
    return ck, ck.bases()


@pytest.fixture(scope="module")
def keys(srs):
    ks = {c: _key(srs, c, 1 << 14) for c in (BN256, GRUMPKIN)}
    yield ks
    for ck, _ in ks.values():
        ck.close()


@pytest.mark.parametrize("variant,k,space", [("vector", 5, "host"), ("vector", 5, "dev"), ("vector", 11, "host"), ("scalar", 5, "host"),
                                              ("scalar", 5, "dev"), ("scalar", 11, "host"), ("two", 5, "host"), ("two", 5, "dev")])
def test_sps_lookups_bn256(srs, oracle, sp, keys, variant, k, space):
    SPS.run_case(srs, oracle, sp, keys[BN256], BN256, variant, k, space=space)


@pytest.mark.parametrize("variant", ["scalar", "two"])
def test_sps_round0_chunked_advice(srs, oracle, sp, keys, variant):
    """round 0 of the two-round protocol with the advice in three streamed chunks (one per column) and (ls, ts, ms) as a further set of
    the same commit, at the size where each chunk is more than one block"""
    with srs.tuning(commit_chunks=3):
        SPS.run_case(srs, oracle, sp, keys[BN256], BN256, variant, 10)


def test_sps_two_lookups_k11(srs, oracle, sp):
    key = _key(srs, BN256, 9 << 11)
    SPS.run_case(srs, oracle, sp, key, BN256, "two", 11)
    key[0].close()


@pytest.mark.parametrize("k", [5, 11])
def test_sps_scalar_lookup_grumpkin_reduced_instance(srs, oracle, sp, keys, k):
    """grumpkin's scalar field is the larger one: the instance bn256-Fr-modulus + 5 enters the transcript as 5"""
    inst = (FR_MODULUS + 5, 3)
    _, out, _ = SPS.run_case(srs, oracle, sp, keys[GRUMPKIN], GRUMPKIN, "scalar", k, instances_int=inst)
    if k == 5:      # the reduction decides the challenge: the unreduced neighbour 5 gives the same one, 6 another
        same = SPS.run_case(srs, oracle, sp, keys[GRUMPKIN], GRUMPKIN, "scalar", k, instances_int=(5, 3))[1]
        other = SPS.run_case(srs, oracle, sp, keys[GRUMPKIN], GRUMPKIN, "scalar", k, instances_int=(6, 3))[1]
        assert np.array_equal(out["W_commitments"][0], same["W_commitments"][0]) and np.array_equal(out["W_commitments"][0], other["W_commitments"][0])
        assert np.array_equal(out["challenges"], same["challenges"]) and not np.array_equal(out["challenges"], other["challenges"])


@pytest.mark.parametrize("variant", ["one", "gates"])
@pytest.mark.parametrize("k", [5, 10])
@pytest.mark.parametrize("space", ["host", "dev"])
def test_sps_without_lookups_padding(srs, oracle, sp, keys, variant, k, space):
    rows = 1 << k
    SPS.run_case(srs, oracle, sp, keys[BN256], BN256, variant, k, space=space, lens=[rows, rows - 3, 0])


def test_sps_supplied_challenges_zero_denominators(srs, oracle, sp, keys):
    SPS.zero_denominator_case(srs, oracle, sp, keys[BN256], BN256, 6)


def test_sps_refusals(srs, oracle, sp, keys):
    SPS.refusal_cases(srs, oracle, sp, keys[BN256], BN256)
