"""GPU: the closed-form ProtoGalaxy sums of the reference's leaf rows against the oracle's literal restatement and,
bit for bit, against the weighted trees (`pg_compat_tree=1`) -- at the smallest shapes where each branch of the gate-value launch and of
the tree route it is compared with can go wrong: one leaf per thread with tile_log = min(7, k) (k = 3, 7), the first k above that tile
(8), the 8-leaves-per-thread route and its first k with two tiles per gate (10, 11); one, two and three gates (three pad the table with
a block of zero leaves); the ahead-of-time gate set (MainGate<5> + MainGate<3> at k >= 10) and the interpreter."""
import pytest

from pg_closed_cases import run_closed_case, run_sharded_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", [3, 7, 8, 10, 11])
@pytest.mark.parametrize("n_gates", [1, 2, 3])
def test_closed_form_one_incoming_trace(srs, oracle, k, n_gates):
    """L = 1: integer-point G; compute_G evaluates every node, prove takes G(1) from the same launch (the trees: from `g_at_one`)."""
    run_closed_case(srs, oracle, k, n_gates, 1)


@pytest.mark.parametrize("k", [10, 11])
def test_closed_form_specialised_gate_set(srs, oracle, k):
    """MainGate<5> + MainGate<3>: the ahead-of-time sweep kernel evaluates the gates at row 0 (k >= 10)."""
    run_closed_case(srs, oracle, k, ("main", [5, 3]), 1)


def test_closed_form_three_incoming_traces(srs, oracle):
    """L = 3 at k = 10, the reference's own test shape: G on the 16 roots of unity (inverse DFT on the host), K over 2^16 coefficients."""
    ctx = run_closed_case(srs, oracle, 10, ("main", [5]), 3, ro=False)
    assert (ctx.fft_points_count_G, ctx.fft_log_domain_size_K) == (16, 16)


@pytest.mark.parametrize("k,L", [(7, 1), (10, 1), (7, 3)])
def test_closed_form_challenges_folded_per_point(srs, oracle, k, L):
    """num_challenges > 0: the traces' challenges are folded with L_j(X_p) for every evaluation point of G."""
    run_closed_case(srs, oracle, k, "primary+challenge", L)


@pytest.mark.parametrize("world", [2, 3])
def test_closed_form_sharded_partials(srs, oracle, world):
    run_sharded_case(srs, oracle, 11, 3, world)
