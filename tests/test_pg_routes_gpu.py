"""GPU: the routes of the ProtoGalaxy sums that the other tests do not reach directly (tests/pg_route_cases.py) -- the reference's leaf rows
through every route with the same bits, and the intended leaf rows on a row-sharded structure."""
import pytest

from pg_route_cases import run_reference_rows_case, run_sharded_true_rows_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k,gate_T", [(10, [5, 3]), (10, [2]), (11, [5, 3])])
def test_reference_rows_every_route_same_bits(srs, oracle, k, gate_T):
    """the ahead-of-time gate set, the interpreter, two tiles per gate"""
    run_reference_rows_case(srs, oracle, k, gate_T)


_whole = {}      # (k, gates) -> the unsharded F, G, e of this module's library


@pytest.mark.parametrize("k,world,gate_T,nonzero_ranks", [(7, 2, [2], 1), (11, 2, [5, 3], 2), (11, 3, [5, 3], 2), (11, 3, [2], 2)])
def test_true_rows_sharded_partials(srs, oracle, k, world, gate_T, nonzero_ranks):
    run_sharded_true_rows_case(srs, oracle, k, world, gate_T, nonzero_ranks, _whole)
