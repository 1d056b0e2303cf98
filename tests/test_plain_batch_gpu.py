"""GPU parity of sets of MSMs on plain commitment keys (tuning msm_plain = 1 / 2) that run as one linked flow -- the segment is the pair
(member, window), up to 256 of them -- against the CPU oracle's MSM of every member, never against another key form or the sequential
flow.  Keys of 3000 oracle bases (2^14 for the prover entries), form 1 on bn256 and form 2 on grumpkin; the shapes also run on the two
crossed pairs.  What a set is counted as (plain_batch_stats(), plain_stats(), msm_stats()) is asserted with every batch: a condition on
the inputs.  Bit-exact."""
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, seeded_scalars, tune_env
import plain_batch_cases as PB
from plain_batch_cases import CROSSED, KEY_N, KEYS, SHAPES, counted, mont, oracle_batch
from plain_key_cases import boundary_ints, dev, one_bucket_ints

pytestmark = pytest.mark.gpu

BIG_LOG = 14


def _lib():
    from sirius_amd import _lib
    return _lib.load()


def _q(cid):
    return PB.PF.order(cid)


@pytest.fixture(scope="module")
def keys(srs, oracle):
    """(curve, form) -> (oracle bases of a 3000-base key, the plain key of that form over them); shared, read-only."""
    out = {}
    for cid, form in KEYS + CROSSED:
        bases = oracle.make_bases(cid, 1211 + cid, KEY_N)
        out[cid, form] = (bases, PB.batch_key(srs, cid, form, bases))
    yield out
    for _, ck in out.values():
        ck.close()


@pytest.fixture(scope="module")
def big_keys(srs, oracle):
    out = {}
    for cid, form in KEYS:
        bases = oracle.make_bases(cid, 1221 + cid, 1 << BIG_LOG)
        out[cid, form] = (bases, PB.batch_key(srs, cid, form, bases))
    yield out
    for _, ck in out.values():
        ck.close()


@pytest.fixture(scope="module")
def shape_vectors(oracle):
    """(curve, shape) -> (member vectors, the oracle's commitments over the keys' bases): computed once, for both forms of a curve."""
    out = {}
    for cid in (0, 1):
        bases = oracle.make_bases(cid, 1211 + cid, KEY_N)
        for name, (lens, _) in SHAPES.items():
            vs = PB.member_vectors(oracle, cid, lens, 1230 + len(lens))
            out[cid, name] = (vs, oracle_batch(oracle, cid, vs, bases))
    return out


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,form", KEYS + CROSSED)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_plain_batch_shapes(oracle, keys, shape_vectors, cid, form, shape):
    O = oracle
    _, ck = keys[cid, form]
    vs, want = shape_vectors[cid, shape]
    sets, msms = SHAPES[shape][1]
    ran = sum(1 for v in vs if len(v))
    assert np.array_equal(counted(ck, lambda: ck.commit_batch(vs), sets, msms, ran), want)                        # host scalars
    assert np.array_equal(counted(ck, lambda: ck.commit_batch([dev(v) for v in vs]), sets, msms, ran), want)      # device-resident
    limbs = [O.ints_to_limbs(O.mont_to_ints(O.SCALAR_FIELD[cid], v)) if len(v) else v for v in vs]
    assert np.array_equal(counted(ck, lambda: ck.commit_batch(limbs, repr=1), sets, msms, ran), want)             # canonical integers


# ---- 2. members do not share buckets --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,form", KEYS)
def test_plain_batch_members_apart(oracle, keys, cid, form):
    O = oracle
    bases, ck = keys[cid, form]
    one = mont(O, cid, [0x7FFF])
    want = O.msm(cid, one, bases[:1])
    got = counted(ck, lambda: ck.commit_batch([one] * 16), 1, 16, 16)
    assert all(np.array_equal(g, want) for g in got)                      # 0x7FFF P0 sixteen times, never a multiple of it
    q, sf = _q(cid), O.SCALAR_FIELD[cid]
    v = O.mont_to_ints(sf, seeded_scalars(O, cid, 600, 1241 + cid, "uniform"))
    a, b = mont(O, cid, v), mont(O, cid, [(q - x) % q for x in v])
    got = counted(ck, lambda: ck.commit_batch([dev(a), dev(b)]), 1, 2, 2)
    wa, wb = O.msm(cid, a, bases[:600]), O.msm(cid, b, bases[:600])
    assert np.array_equal(got[0], wa) and np.array_equal(got[1], wb)
    neg = wa.copy()
    neg[4:] = O.fe_sub(O.BASE_FIELD[cid], np.zeros((1, 4), np.uint64), wa[None, 4:])[0]
    assert np.array_equal(got[1], neg)                                    # the negative of its neighbour


# ---- 3. segment order -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,form", KEYS)
def test_plain_batch_segment_order(oracle, keys, cid, form):
    """Member w is the one scalar 2^(16 w) on base 0: result w is 2^(16 w) P0 -- a transposed (member, window) index or a wrong landing
    offset moves it.  Form 2 also takes lambda 2^(16 w), entries of k2 alone (a second set)."""
    O = oracle
    bases, ck = keys[cid, form]
    ints = [1 << (16 * w) for w in range(16)]
    if form == 2:
        import glv_cases as G
        lam, _ = G.constants(_lib(), cid)
        ints += [(lam << (16 * w)) % _q(cid) for w in range(8)]
    vs = [mont(O, cid, [x]) for x in ints]
    want = np.stack([O.msm(cid, v, bases[:1]) for v in vs])
    sets = 1 if form == 1 else 2
    got = counted(ck, lambda: ck.commit_batch(vs), sets, len(vs), len(vs))
    for j in range(len(vs)):
        assert np.array_equal(got[j], want[j]), j
    assert len({w.tobytes() for w in want}) == len(vs)


# ---- 4. digits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,form", KEYS)
def test_plain_batch_digits(oracle, keys, cid, form):
    O = oracle
    bases, ck = keys[cid, form]
    q = _q(cid)
    vals = boundary_ints(q)
    cut = (len(vals) + 3) // 4
    vs = [mont(O, cid, vals[i:i + cut]) for i in range(0, len(vals), cut)]
    assert len(vs) == 4
    assert np.array_equal(counted(ck, lambda: ck.commit_batch(vs), 1, 4, 4), oracle_batch(O, cid, vs, bases))
    # one value per member, repeated: every bucket's parts go through the levels at a different depth per segment
    reps = (3000, 1000, 513, 1)
    vs = [mont(O, cid, [x] * reps[j % 4]) for j, x in enumerate(one_bucket_ints(q))]
    assert np.array_equal(counted(ck, lambda: ck.commit_batch([dev(v) for v in vs]), 1, len(vs), len(vs)), oracle_batch(O, cid, vs, bases))


# ---- 5. degenerate bases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,form", KEYS)
def test_plain_batch_degenerate_bases(srs, oracle, cid, form):
    O = oracle
    q, fld, n = _q(cid), O.BASE_FIELD[cid], 1100
    pool = O.make_bases(cid, 3, 4)
    neg = pool.copy()
    neg[:, 4:] = O.fe_sub(fld, np.zeros_like(pool[:, 4:]), pool[:, 4:])
    # the same point repeated, equal scalars per member
    bases = np.repeat(pool[:1], n, axis=0)
    ck = PB.batch_key(srs, cid, form, bases)
    vs = [mont(O, cid, [x] * m) for x, m in ((1, n), (0x10001, 513), (q - 1, 700), ((1 << 200) + 12345, 64))]
    assert np.array_equal(counted(ck, lambda: ck.commit_batch(vs), 1, 4, 4), oracle_batch(O, cid, vs, bases))
    ck.close()
    # P, -P interleaved: members of an even count of equal scalars give the identity (the all-zero encoding), the others do not
    bases = np.empty((n, 8), np.uint64)
    bases[0::2], bases[1::2] = pool[1], neg[1]
    ck = PB.batch_key(srs, cid, form, bases)
    vs = [mont(O, cid, [0x123456789ABCDEF] * m) for m in (n, 513, 2, 1)]
    got = counted(ck, lambda: ck.commit_batch(vs), 1, 4, 4)
    assert np.array_equal(got, oracle_batch(O, cid, vs, bases))
    assert not got[0].any() and not got[2].any() and got[1].any() and got[3].any()
    ck.close()
    # an identity base inside an otherwise ordinary key
    bases = O.make_bases(cid, 1251 + cid, n)
    bases[7] = 0
    bases[n // 3] = 0
    ck = PB.batch_key(srs, cid, form, bases)
    vs = PB.member_vectors(O, cid, (n, 8, 600), 1252)
    assert np.array_equal(counted(ck, lambda: ck.commit_batch(vs), 1, 3, 3), oracle_batch(O, cid, vs, bases))
    assert ck.count_off_curve() == 0
    ck.close()


# ---- 6. the entries built on the batch --------------------------------------------------------------------------------------------------
def _rose(ck, run):
    before = ck.plain_batch_stats()["sets"]
    out = run()
    assert ck.plain_batch_stats()["sets"] > before
    return out


@pytest.mark.parametrize("cid,form", KEYS)
def test_plain_batch_sangria_entries(srs, oracle, big_keys, cid, form):
    """srs_commit_cross_terms and srs_sangria_prove at k = 5 with gates [3, 2]; srs_sangria_prove_incoming on a challenge-free structure
    (d + 1 members: the incoming trace rides in the cross terms' set)."""
    import torch
    from workloads import gates_for, rand_fe
    S, O = srs, oracle
    field = O.SCALAR_FIELD[cid]
    bases, ck = big_keys[cid, form]
    msm = lambda v: O.msm(cid, np.ascontiguousarray(v), bases[:len(v)])
    host = lambda t: t.cpu().numpy().view(np.uint64).reshape(-1, 4)
    k, rows = 5, 32
    rng = np.random.default_rng(1260 + cid)
    for gate_T in ([3, 2], [3]):
        gates, nfix, nadv = gates_for(gate_T)
        fixed = [rand_fe(rng, rows, 0.3) for _ in range(nfix)]
        St = S.PlonkStructure(field, k, [], fixed, nadv, gates)
        assert bool(St.num_challenges) == (len(gate_T) > 1)                 # one gate: the challenge-free structure of the incoming entry
        y1, y2, u1 = rand_fe(rng, St.num_challenges), rand_fe(rng, St.num_challenges), rand_fe(rng, 1)[0]
        W1, W2, E, r = rand_fe(rng, nadv * rows), rand_fe(rng, nadv * rows), rand_fe(rng, rows), rand_fe(rng, 1)[0]
        terms, _ = S.VanillaFS.commit_cross_terms(None, St, y1, u1, W1, y2, W2)
        want_commits = np.stack([msm(t) for t in terms])
        cW1, cW2, cE = msm(W1), msm(W2), msm(E)
        if St.num_challenges:
            _, commits = _rose(ck, lambda: S.VanillaFS.commit_cross_terms(ck, St, y1, u1, W1, y2, W2))
            assert np.array_equal(commits, want_commits)
            dW1, dE = dev(W1), dev(E)
            pr = _rose(ck, lambda: S.sangria_prove(ck, St, y1, u1, dW1, y2, dev(W2), dE, np.stack([cW1, cW2]), cE, r=r))
            assert np.array_equal(pr["commits"], want_commits)
            assert np.array_equal(pr["W_commitment"].wait(), msm(host(dW1))) and np.array_equal(pr["E_commitment"].wait(), msm(host(dE)))
        else:
            dW1, dE = dev(W1), dev(E)
            pr = _rose(ck, lambda: S.sangria_prove(ck, St, y1, u1, dW1, y2, dev(W2), dE, cW1, cE, r=r, incoming=True))
            assert np.array_equal(pr["incoming_commitment"], cW2) and np.array_equal(pr["commits"], want_commits)
            assert np.array_equal(host(dW1), O.fold_w(field, W1, W2, r)) and np.array_equal(host(dE), O.fold_e(field, E, terms, r))
            assert np.array_equal(pr["W_commitment"].wait(), msm(host(dW1))) and np.array_equal(pr["E_commitment"].wait(), msm(host(dE)))
        torch.cuda.synchronize()
        St.close()


@pytest.mark.parametrize("cid,form", KEYS)
def test_plain_batch_is_sat_witness_commit(srs, oracle, big_keys, cid, form):
    from workloads import rand_fe
    S, O = srs, oracle
    bases, ck = big_keys[cid, form]
    rng = np.random.default_rng(1270 + cid)
    W = [rand_fe(rng, 9001, 0.5), rand_fe(rng, 1 << 12, 0.5)]
    E = rand_fe(rng, 700)
    cw = np.stack([O.msm(cid, w, bases[:len(w)]) for w in W])
    ce = O.msm(cid, E, bases[:len(E)])
    assert _rose(ck, lambda: S.VanillaFS.is_sat_witness_commit(ck, W, cw, E, ce)) == (0, False)
    W[1][7] = rand_fe(rng, 1)[0]
    assert _rose(ck, lambda: S.VanillaFS.is_sat_witness_commit(ck, W, cw, E, ce)) == (1, False)
    E[0] = rand_fe(rng, 1)[0]
    assert S.VanillaFS.is_sat_witness_commit(ck, W, cw, E, ce) == (1, True)


# ---- 7. state between sets --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,form", KEYS)
def test_plain_batch_state(srs, oracle, big_keys, shape_vectors, cid, form):
    """Batch, resident single commit, streamed folded commit, the first batch again on one key: nothing of the arena or of the running
    buckets leaks either way.  Then the batch with msm_plain_batch = 0: the same points, no batched set."""
    O = oracle
    bases, ck = big_keys[cid, form]                                         # (the streamed commit takes 3072 bases)
    vs = shape_vectors[cid, "tiles"][0]
    want = oracle_batch(O, cid, vs, bases)
    B = seeded_scalars(O, cid, 2500, 1280 + cid, "uniform")
    A = seeded_scalars(O, cid, PB.PF.N_FULL, 1281 + cid, "trace")
    assert np.array_equal(counted(ck, lambda: ck.commit_batch(vs), 1, 4, 4), want)
    assert np.array_equal(counted(ck, lambda: ck.commit(dev(B)), 0, 0, 1), O.msm(cid, B, bases[:2500]))
    assert np.array_equal(PB.PF.streamed(srs, ck, A), O.msm(cid, A, bases[:PB.PF.N_FULL]))
    assert np.array_equal(counted(ck, lambda: ck.commit_batch(vs), 1, 4, 4), want)
    with srs.tuning(msm_plain_batch=0):
        assert np.array_equal(counted(ck, lambda: ck.commit_batch(vs), 0, 0, 4), want)
    assert np.array_equal(counted(ck, lambda: ck.commit_batch([dev(v) for v in vs]), 1, 4, 4), want)      # (read per set: on again)


# ---- 8. other keys ----------------------------------------------------------------------------------------------------------------------
def test_plain_batch_stats_of_other_keys(srs, oracle, keys, shape_vectors):
    bases, _ = keys[0, 1]
    vs, want = shape_vectors[0, "tiles"]
    full = srs.CommitmentKey(0, bases)
    with srs.tuning(msm_compact=1):
        compact = srs.CommitmentKey(0, bases)
    for ck in (full, compact):
        assert not ck.is_plain()
        assert np.array_equal(ck.commit_batch(vs), want)
        assert ck.plain_batch_stats() == dict(sets=0, msms=0)
        ck.close()


# ---- 9. one larger set ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [1, 2])
def test_plain_batch_equals_default_at_scale(srs, form):
    """6 x 2^17 trace-like device scalars on a synthetic 2^17 key (the Sangria primary's cross-term shape): the batched plain flow against
    a default key, one subprocess each -- same seeded inputs, the same six affine points."""
    code = (
        "import sys, numpy as np, torch; sys.path.insert(0, '.')\n"
        "import sirius_amd as S\n"
        "n = 1 << 17\n"
        "ck = S.CommitmentKey.setup_synthetic(0, n, seed=23)\n"
        "g = torch.Generator(device='cuda').manual_seed(9)\n"
        "vs = []\n"
        "for j in range(6):\n"
        "    v = torch.randint(0, 1 << 62, (n, 4), dtype=torch.int64, device='cuda', generator=g); v[:, 3] &= (1 << 60) - 1\n"
        "    v[torch.rand(n, device='cuda', generator=g) < 0.5] = 0\n"
        "    v[torch.rand(n, device='cuda', generator=g) < 0.2, 1:] = 0\n"
        "    vs.append(v)\n"
        "out = ck.commit_batch(vs)\n"
        "print('K', ck.plain_form(), ck.plain_batch_stats()['sets'], ck.plain_batch_stats()['msms'])\n"
        "print('C', out.tobytes().hex())\n")
    outs = []
    for env, head in ((tune_env(msm_plain=form), f"K {form} 1 6"), (tune_env(), "K 0 0 0")):
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-1500:]
        assert head in r.stdout.splitlines(), r.stdout[-300:]
        outs.append([l for l in r.stdout.splitlines() if l.startswith("C ")][-1])
    assert outs[0] == outs[1] and len(outs[0]) > 700
