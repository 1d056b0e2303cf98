"""GPU parity of plain commitment keys (tuning msm_plain = 1 when the key is created: the bases alone, no window table) against the CPU
oracle: the plain flow at the sizes, scalars and bases at which its window grouping, its 16 linked bucket sets or the Horner chain of
window weights can go wrong, every entry that takes a key, the key's bookkeeping and what such a key refuses.  Bit-exact."""
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, seeded_scalars, tune_env
from plain_key_cases import (boundary_ints, check_bookkeeping, commit_counted, dev, limbs16, one_bucket_ints, plain_key,
                             window_powers)

pytestmark = pytest.mark.gpu

KEY_N = 3000
SIZES = (1, 5, 513, KEY_N)             # 513: one scalar past a tile of the segment passes
BIG_LOG = 14


def _q(cid):
    from oracle import pyref as P
    return P.CURVES[cid].q


@pytest.fixture(scope="module")
def keys(srs, oracle):
    """Per curve: oracle bases of a 3000-base key and the plain key over them (shared, read-only)."""
    out = {}
    for cid in (0, 1):
        bases = oracle.make_bases(cid, 811 + cid, KEY_N)
        out[cid] = (bases, plain_key(srs, cid, bases))
    yield out
    for _, ck in out.values():
        ck.close()


@pytest.fixture(scope="module")
def big_keys(srs, oracle):
    """Per curve: a 2^14-base plain key for the other entries."""
    out = {}
    for cid in (0, 1):
        bases = oracle.make_bases(cid, 821 + cid, 1 << BIG_LOG)
        out[cid] = (bases, plain_key(srs, cid, bases))
    yield out
    for _, ck in out.values():
        ck.close()


@pytest.mark.parametrize("cid", [0, 1])
def test_plain_bookkeeping(srs, oracle, keys, tmp_path, cid):
    O = oracle
    bases, ck = keys[cid]
    check_bookkeeping(ck, KEY_N)
    assert np.array_equal(ck.bases(), bases) and ck.count_off_curve() == 0
    k, n = 10, 1 << 10
    full = srs.CommitmentKey(cid, bases[:n])                              # the tunable unset: the key of every earlier release
    assert not full.is_plain() and full.table_bytes() == 16 * n * 64
    pk = plain_key(srs, cid, bases[:n])
    pk.save_to_file(tmp_path / "plain.bin")
    full.save_to_file(tmp_path / "full.bin")
    assert (tmp_path / "plain.bin").read_bytes() == (tmp_path / "full.bin").read_bytes() == bases[:n].tobytes()
    sc = seeded_scalars(O, cid, n, 5, "trace")
    want = O.msm(cid, sc, bases[:n])
    with srs.tuning(msm_plain=1):
        loaded_plain = srs.CommitmentKey.load_from_file(cid, tmp_path / "plain.bin", k)
        syn_plain = srs.CommitmentKey.setup_synthetic(cid, n, seed=3)
    loaded_full = srs.CommitmentKey.load_from_file(cid, tmp_path / "plain.bin", k)
    syn = srs.CommitmentKey.setup_synthetic(cid, n, seed=3)
    check_bookkeeping(loaded_plain, n)
    check_bookkeeping(syn_plain, n)
    assert not loaded_full.is_plain() and not syn.is_plain() and loaded_full.table_bytes() == 16 * n * 64
    for key in (full, pk, loaded_plain, loaded_full):
        assert np.array_equal(key.commit(sc), want)
    assert np.array_equal(syn_plain.bases(), syn.bases()) and np.array_equal(syn_plain.commit(sc), O.msm(cid, sc, syn.bases()))
    for key in (full, pk, loaded_plain, loaded_full, syn, syn_plain):
        key.close()


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("kind", ["uniform", "trace"])
@pytest.mark.parametrize("n", SIZES)
def test_plain_commit_sizes(oracle, keys, cid, n, kind):
    bases, ck = keys[cid]
    sc = seeded_scalars(oracle, cid, n, 700 + n, kind)
    want = oracle.msm(cid, sc, bases[:n])
    assert np.array_equal(commit_counted(ck, sc), want)                   # host scalars
    assert np.array_equal(commit_counted(ck, dev(sc)), want)              # device-resident
    st = ck.msm_stats()
    assert st["slot_sets"] == 0 and st["hot_sets"] == 0 and st["redo"] == 0, st


@pytest.mark.parametrize("cid,n,kind", [(0, 70000, "uniform"), (1, 33333, "trace")])
def test_plain_many_tiles(srs, oracle, cid, n, kind):
    O = oracle
    bases = O.make_bases(cid, 831 + cid, n)
    ck = plain_key(srs, cid, bases)
    sc = seeded_scalars(O, cid, n, 832, kind)
    assert np.array_equal(commit_counted(ck, dev(sc)), O.msm(cid, sc, bases))
    ck.close()


@pytest.mark.parametrize("cid", [0, 1])
def test_plain_digit_boundaries(oracle, keys, cid):
    """The whole boundary list at once, then in groups of four (a wrong digit cannot cancel against another), as Montgomery scalars and
    as canonical integers (repr = 1); the sixteen window weights 2^(16 w) each alone (n = 1: the result is 2^(16 w) P_0)."""
    O = oracle
    sf = O.SCALAR_FIELD[cid]
    bases, ck = keys[cid]
    vals = boundary_ints(_q(cid))
    groups = [vals] + [vals[i:i + 4] for i in range(0, len(vals), 4)] + [[p] for p in window_powers()]
    for g in groups:
        sc = O.ints_to_mont(sf, g)
        want = O.msm(cid, sc, bases[:len(g)])
        assert np.array_equal(ck.commit(sc), want), [hex(v) for v in g]
        assert np.array_equal(ck.commit(O.ints_to_limbs(g), repr=1), want), [hex(v) for v in g]


def test_plain_boundary_list_is_what_it_says():
    """The two all-windows scalars of the list have the limbs they are named for (the helper is shared with the emulator test)."""
    tie, carry = limbs16([0x8000] * 15), limbs16([0x8001] * 15 + [0x2FFF])
    assert [(tie >> (16 * w)) & 0xFFFF for w in range(16)] == [0x8000] * 15 + [0]
    assert [(carry >> (16 * w)) & 0xFFFF for w in range(16)] == [0x8001] * 15 + [0x2FFF]
    for cid in (0, 1):
        assert tie in boundary_ints(_q(cid)) and carry in boundary_ints(_q(cid)) and carry < _q(cid)


@pytest.mark.parametrize("cid", [0, 1])
def test_plain_one_bucket(oracle, keys, cid):
    """3000 equal scalars: every entry of a window falls into one bucket, whose parts go through the accumulation levels."""
    O = oracle
    bases, ck = keys[cid]
    for x in one_bucket_ints(_q(cid)):
        sc = O.ints_to_mont(O.SCALAR_FIELD[cid], [x] * KEY_N)
        assert np.array_equal(ck.commit(dev(sc)), O.msm(cid, sc, bases)), hex(x)


@pytest.mark.parametrize("cid", [0, 1])
def test_plain_degenerate_bases(srs, oracle, cid):
    """Keys of repeated and negated points (built as test_commit_degenerate_bases builds them) and an identity base."""
    O = oracle
    q, sf, fld, n = _q(cid), O.SCALAR_FIELD[cid], O.BASE_FIELD[cid], KEY_N
    pool = O.make_bases(cid, 3, 4)
    neg = pool.copy()
    neg[:, 4:] = O.fe_sub(fld, np.zeros_like(pool[:, 4:]), pool[:, 4:])          # (x, -y)
    # one point repeated n times, equal scalars: the running sum of a part equals the next entry (the doubling behind the sticky flag)
    bases = np.repeat(pool[:1], n, axis=0)
    ck = plain_key(srs, cid, bases)
    for v in (1, 5, 0x10001, q - 1, (1 << 200) + 12345):
        sc = O.ints_to_mont(sf, [v] * n)
        assert np.array_equal(ck.commit(sc), O.msm(cid, sc, bases)), ("repeat", hex(v))
    ck.close()
    # P, -P interleaved with equal scalars: the partial sums cancel, the total is the identity (all-zero affine encoding)
    bases = np.empty((n, 8), np.uint64)
    bases[0::2], bases[1::2] = pool[1], neg[1]
    ck = plain_key(srs, cid, bases)
    sc = O.ints_to_mont(sf, [0x123456789ABCDEF] * n)
    got = ck.commit(sc)
    assert not got.any() and np.array_equal(got, O.msm(cid, sc, bases))
    ck.close()
    # an identity base inside an otherwise ordinary key
    bases = O.make_bases(cid, 841 + cid, n)
    bases[7] = 0
    bases[n // 3] = 0
    ck = plain_key(srs, cid, bases)
    for kind in ("uniform", "trace"):
        sc = seeded_scalars(O, cid, n, 842, kind)
        assert np.array_equal(ck.commit(sc), O.msm(cid, sc, bases)), kind
    assert ck.count_off_curve() == 0
    ck.close()


def test_plain_vs_eip196_known_answers(srs, oracle):
    """ecMul / ecAdd as MSMs over plain bn256 keys made of the vectors' points, against the EIP-196 known answers."""
    import eip196_cases as E

    def msm(scalars, bases):
        ck = plain_key(srs, 0, bases)
        try:
            return ck.commit(np.ascontiguousarray(scalars))
        finally:
            ck.close()
    E.check_adder(oracle, lambda a, b: srs.point_sum(0, np.stack([a, b])), lambda k, p: srs.point_mul(0, k, p), msm)


@pytest.mark.parametrize("cid", [0, 1])
def test_plain_other_entries(srs, oracle, big_keys, cid):
    """Prefix commit, batch, the streamed commits (every chunk a whole plain MSM over its base range) and the column form."""
    O = oracle
    bases, ck = big_keys[cid]
    m = 9001
    sc = seeded_scalars(O, cid, m, 31, "trace")
    want = O.msm(cid, sc, bases[:m])
    assert np.array_equal(commit_counted(ck, dev(sc)), want)
    vs = [sc, seeded_scalars(O, cid, 63, 32, "uniform"), seeded_scalars(O, cid, 1, 33, "uniform")]
    ws = [want] + [O.msm(cid, v, bases[:len(v)]) for v in vs[1:]]
    assert np.array_equal(ck.commit_batch(vs), np.stack(ws))
    assert np.array_equal(ck.commit_batch([dev(v) for v in vs]), np.stack(ws))
    hb = srs.HostBuffer(m)
    hb.array[:] = sc
    for chunks in (1, 3):
        with srs.tuning(commit_chunks=chunks):
            before = ck.msm_stats()
            assert np.array_equal(ck.commit_upload(sc), want), chunks                      # pageable source
            assert np.array_equal(ck.commit_upload(hb.array), want), chunks                # page-locked source
            after = ck.msm_stats()
            assert after["other_sets"] >= before["other_sets"] + 2 and after["slot_sets"] == 0, (chunks, before, after)
    hb.close()
    import torch
    rows, ncol = 1 << 11, 4
    cols = [seeded_scalars(O, cid, rows - 5 * j, 40 + j, "trace") for j in range(ncol)]
    W = np.zeros((ncol * rows, 4), np.uint64)                                              # util::concatenate_with_padding
    for j, c in enumerate(cols):
        W[j * rows:j * rows + len(c)] = c
    want_cols = O.msm(cid, W, bases[:len(W)])
    for chunks in (1, 3):
        with srs.tuning(commit_chunks=chunks):
            d = torch.zeros((ncol * rows, 4), dtype=torch.int64, device="cuda")
            assert np.array_equal(ck.commit_upload_columns(cols, rows, dev_copy=d), want_cols), chunks
            assert np.array_equal(d.cpu().numpy().view(np.uint64), W)
    st = ck.msm_stats()
    assert st["slot_sets"] == 0 and st["hot_sets"] == 0 and st["redo"] == 0, st


@pytest.mark.parametrize("cid", [0, 1])
def test_plain_sangria_prove(srs, oracle, big_keys, cid):
    """srs_commit_cross_terms and srs_sangria_prove over a plain key: every commitment is the oracle's MSM of the vector it commits to."""
    import torch
    from workloads import gates_for, rand_fe
    S, O = srs, oracle
    field = O.SCALAR_FIELD[cid]
    bases, ck = big_keys[cid]
    k, rows, gate_T = 5, 32, [3, 2]
    gates, nfix, nadv = gates_for(gate_T)
    rng = np.random.default_rng(90 + cid)
    fixed = [rand_fe(rng, rows, 0.3) for _ in range(nfix)]
    St = S.PlonkStructure(field, k, [], fixed, nadv, gates)
    y1, y2, u1 = rand_fe(rng, St.num_challenges), rand_fe(rng, St.num_challenges), rand_fe(rng, 1)[0]
    W1, W2, E, r = rand_fe(rng, nadv * rows), rand_fe(rng, nadv * rows), rand_fe(rng, rows), rand_fe(rng, 1)[0]
    msm = lambda v: O.msm(cid, np.ascontiguousarray(v), bases[:len(v)])
    terms, _ = S.VanillaFS.commit_cross_terms(None, St, y1, u1, W1, y2, W2)               # the evaluation half alone: no key
    want_commits = np.stack([msm(t) for t in terms])
    _, commits = S.VanillaFS.commit_cross_terms(ck, St, y1, u1, W1, y2, W2)
    assert np.array_equal(commits, want_commits)
    cW1, cW2, cE = msm(W1), msm(W2), msm(E)
    dW1, dE = dev(W1), dev(E)
    pr = S.sangria_prove(ck, St, y1, u1, dW1, y2, dev(W2), dE, np.stack([cW1, cW2]), cE, r=r)
    assert np.array_equal(pr["commits"], want_commits)
    host = lambda t: t.cpu().numpy().view(np.uint64).reshape(-1, 4)
    assert all(np.array_equal(host(a), b) for a, b in zip(pr["terms"], terms))
    assert np.array_equal(host(dW1), O.fold_w(field, W1, W2, r)) and np.array_equal(host(dE), O.fold_e(field, E, terms, r))
    assert np.array_equal(pr["W_commitment"].wait(), msm(host(dW1))) and np.array_equal(pr["E_commitment"].wait(), msm(host(dE)))
    torch.cuda.synchronize()
    St.close()


@pytest.mark.parametrize("cid", [0, 1])
def test_plain_is_sat_witness_commit(srs, oracle, big_keys, cid):
    from workloads import rand_fe
    S, O = srs, oracle
    bases, ck = big_keys[cid]
    rng = np.random.default_rng(95 + cid)
    W = [rand_fe(rng, 9001, 0.5), rand_fe(rng, 1 << 12, 0.5)]
    E = rand_fe(rng, 700)
    cw = np.stack([O.msm(cid, w, bases[:len(w)]) for w in W])
    ce = O.msm(cid, E, bases[:len(E)])
    assert S.VanillaFS.is_sat_witness_commit(ck, W, cw, E, ce) == (0, False)
    assert S.VanillaFS.is_sat_witness_commit(ck, [dev(w) for w in W], cw) == (0, False)
    W[1][7] = rand_fe(rng, 1)[0]                                        # one witness element changed: that round is reported
    assert S.VanillaFS.is_sat_witness_commit(ck, W, cw, E, ce) == (1, False)
    E[0] = rand_fe(rng, 1)[0]
    assert S.VanillaFS.is_sat_witness_commit(ck, W, cw, E, ce) == (1, True)


@pytest.mark.parametrize("variant,chunks", [("vector", 0), ("two", 3)])
def test_plain_run_sps_protocol(srs, oracle, big_keys, variant, chunks):
    """srs_run_sps_protocol over a plain key, against the literal protocol of tests/sps_cases.py: the advice commit and the device-computed
    (ls, ts, ms) tail are further whole MSMs of one streamed commit; with the advice in three chunks as well."""
    import space_cases as SC
    import sps_cases as SPS
    bases, ck = big_keys[0]
    with srs.tuning(commit_chunks=chunks):
        SPS.run_case(srs, oracle, SC.Spaces.torch_cuda(), (ck, bases), 0, variant, 10 if chunks else 5)


def test_plain_refusals(srs, oracle, tmp_path):
    O = oracle
    n = 1 << 10
    bases = O.make_bases(0, 861, n)
    bases.tofile(tmp_path / "key.bin")

    def refused(make, *names):
        with pytest.raises(srs.SiriusAmdError) as e:
            make().close()
        assert e.value.rc == 4, e.value                                 # SRS_ERR_INVALID
        assert all(name in str(e.value) for name in names), e.value

    with srs.tuning(msm_plain=1, msm_compact=1):
        refused(lambda: srs.CommitmentKey(0, bases), "msm_plain", "msm_compact")
        refused(lambda: srs.CommitmentKey.setup_synthetic(0, n, seed=1), "msm_plain", "msm_compact")
    with srs.tuning(msm_plain=1, msm_compact=2):
        refused(lambda: srs.CommitmentKey(0, bases), "msm_plain", "msm_compact")
    with srs.tuning(msm_plain=1):
        refused(lambda: srs.CommitmentKey(0, bases, rank=1, world=2), "msm_plain")
        refused(lambda: srs.CommitmentKey.setup_synthetic(0, n, seed=1, rank=0, world=2), "msm_plain")
        refused(lambda: srs.CommitmentKey.load_from_file(0, tmp_path / "key.bin", 10, rank=1, world=2), "msm_plain")
        refused(lambda: srs.CommitmentKey.create_multi(0, bases, 2), "msm_plain")
        refused(lambda: srs.CommitmentKey.setup_synthetic_multi(0, n, seed=1, n_devices=2), "msm_plain")
        one = srs.CommitmentKey.create_multi(0, bases, 1)               # one shard on one device is a plain key like any other
    check_bookkeeping(one, n)
    sc = seeded_scalars(O, 0, n, 862, "uniform")
    want = O.msm(0, sc, bases)
    assert np.array_equal(one.commit(sc), want) and np.array_equal(one.commit_upload(sc), want)
    one.close()
    full = srs.CommitmentKey(0, bases)                                  # a default key can still be created and used afterwards
    assert not full.is_plain() and full.table_bytes() == 16 * n * 64 and np.array_equal(full.commit(sc), want)
    full.close()


def test_plain_equals_default_at_scale(srs):
    """3 * 2^20 + 77 trace-like device scalars on a synthetic key: a plain key against a default one, one subprocess each -- same
    seeded inputs, same affine point."""
    code = (
        "import sys, numpy as np, torch; sys.path.insert(0, '.')\n"
        "import sirius_amd as S\n"
        "n = (3 << 20) + 77\n"
        "ck = S.CommitmentKey.setup_synthetic(0, n, seed=21)\n"
        "g = torch.Generator(device='cuda').manual_seed(8)\n"
        "v = torch.randint(0, 1 << 62, (n, 4), dtype=torch.int64, device='cuda', generator=g); v[:, 3] &= (1 << 60) - 1\n"
        "v[torch.rand(n, device='cuda', generator=g) < 0.5] = 0\n"
        "v[torch.rand(n, device='cuda', generator=g) < 0.2, 1:] = 0\n"
        "print('K', int(ck.is_plain()), ck.table_bytes() // (64 * n))\n"
        "print('C', ck.commit(v).tobytes().hex())\n")
    outs = []
    for env, form in ((tune_env(msm_plain=1), "K 1 1"), (tune_env(), "K 0 16")):
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-1500:]
        assert form in r.stdout.splitlines(), r.stdout[-300:]
        outs.append([l for l in r.stdout.splitlines() if l.startswith("C ")][-1])
    assert outs[0] == outs[1] and len(outs[0]) > 100
