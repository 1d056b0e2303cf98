"""GPU: host operands and device operands of every staged C-ABI entry agree, and agree with the oracle (tests/space_cases.py)."""
import pytest

import space_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sp():
    return SC.Spaces.torch_cuda()


@pytest.fixture(scope="module")
def key(srs, oracle):
    k = SC.make_key(srs, oracle)
    yield k
    k[0].close()


@pytest.mark.parametrize("n", SC.VECTOR_SIZES)
def test_vector_entries(srs, oracle, sp, key, n):
    for field in (0, 1):
        for n_terms in (0, 1, 3):
            SC.fold_case(srs, oracle, sp, field, n, n_terms)
        SC.lookup_hg_case(srs, oracle, sp, field, n)
        SC.assigned_case(srs, oracle, sp, field, n)
    for J in (1, 3):
        SC.lincomb_case(srs, oracle, sp, n, J)
    SC.commit_batch_case(srs, oracle, sp, key, n)
    SC.sparse_case(srs, oracle, sp, n)


@pytest.mark.parametrize("shape", SC.NTT_SHAPES)
def test_ntt_batch(srs, oracle, sp, shape):
    SC.ntt_case(srs, oracle, sp, *shape)


@pytest.mark.parametrize("k", SC.STRUCTURE_KS)
def test_main_gate_structure(srs, oracle, sp, key, k):
    SC.main_gate_case(srs, oracle, sp, k, key)


@pytest.mark.parametrize("k", SC.STRUCTURE_KS)
def test_lookup_structure(srs, oracle, sp, k):
    SC.lookup_structure_case(srs, oracle, sp, k)


def test_arenas_regrow(srs, oracle, sp, key):
    SC.regrow_case(srs, oracle, sp, key)
