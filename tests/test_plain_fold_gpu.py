"""GPU parity of streamed commits on plain commitment keys (tuning msm_plain = 1 / 2) whose chunks fold their finished window buckets into
the key's running buckets -- one bucket set per window, one bucket reduction, landing and host chain per commit -- against the CPU oracle's
MSM, never against another key form.  Keys of 2^13 bases, one per curve and form; commit_chunks = 3 cuts n = 3072 into 1024 / 1024 / 1024
and n = 2053 into 1024 / 1024 / 5 (the last set: every bucket single, its finished buckets lie in the level buffers at the segment's linked
offset).  Every streamed commit is asserted, through plain_stats(), to have folded its sets under ONE reduction: a condition on the
inputs.  Bit-exact."""
import numpy as np
import pytest

from conftest import seeded_scalars
import plain_fold_cases as PF
from plain_fold_cases import CHUNKS, DIGITS, N_FULL, N_RAGGED, counted, streamed
from plain_key_cases import dev

pytestmark = pytest.mark.gpu

KEY_LOG = 13
KEYS = [(0, 1), (0, 2), (1, 1), (1, 2)]          # (curve, form)


def _lib():
    from sirius_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def keys(srs, oracle):
    """(curve, form) -> (oracle bases of a 2^13-base key, the plain key of that form over them); shared, read-only."""
    out = {}
    for cid, form in KEYS:
        bases = oracle.make_bases(cid, 1011 + cid, 1 << KEY_LOG)
        out[cid, form] = (bases, PF.fold_key(srs, cid, form, bases))
    yield out
    for _, ck in out.values():
        ck.close()


@pytest.fixture(scope="module")
def vectors(oracle):
    """(curve, form, kind, n) -> (scalars, the oracle's commitment over the keys' bases): computed once."""
    O = oracle
    out = {}
    for cid, form in KEYS:
        bases = O.make_bases(cid, 1011 + cid, 1 << KEY_LOG)
        for n in (N_FULL, N_RAGGED):
            for kind in ("boundary", "trace"):
                sc = (PF.boundary_scalars(O, _lib(), cid, form, n, 1020 + n) if kind == "boundary"
                      else seeded_scalars(O, cid, n, 1030 + n, "trace"))
                assert len(sc) == n
                out[cid, form, kind, n] = (sc, O.msm(cid, sc, bases[:n]))
    return out


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,form", KEYS)
@pytest.mark.parametrize("n", [N_FULL, N_RAGGED])
@pytest.mark.parametrize("kind", ["boundary", "trace"])
def test_plain_fold_parity(srs, keys, vectors, cid, form, n, kind):
    _, ck = keys[cid, form]
    sc, want = vectors[cid, form, kind, n]
    assert np.array_equal(streamed(srs, ck, sc), want)                           # pageable source
    hb = srs.HostBuffer(n)
    hb.array[:] = sc
    got = streamed(srs, ck, hb.array)                                            # page-locked source
    hb.close()
    assert np.array_equal(got, want)


# ---- 2. one bucket across chunks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,form", KEYS)
def test_plain_fold_one_bucket(srs, oracle, keys, cid, form):
    """3072 equal scalars: every chunk's levels run, one running bucket per window carries everything and every other one is the sum of
    three identities."""
    O = oracle
    bases, ck = keys[cid, form]
    for x in PF.one_bucket_values(_lib(), cid, form):
        sc = O.ints_to_mont(O.SCALAR_FIELD[cid], [x] * N_FULL)
        assert np.array_equal(streamed(srs, ck, sc), O.msm(cid, sc, bases[:N_FULL])), hex(x)


# ---- 3. chunks of zeros ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,form", KEYS)
def test_plain_fold_zero_chunks(srs, oracle, keys, cid, form):
    """A whole chunk of zeros as the first set (FOLD_FIRST copies identities), as a middle set (adds nothing) and as the last set (reduces
    what the others left)."""
    O = oracle
    bases, ck = keys[cid, form]
    full = seeded_scalars(O, cid, N_FULL, 1040 + cid, "uniform")
    for j in range(CHUNKS):
        sc = PF.zero_chunk(full, j)
        assert np.array_equal(streamed(srs, ck, sc), O.msm(cid, sc, bases[:N_FULL])), j


# ---- 4. equal and opposite points meeting in a running bucket --------------------------------------------------------------------------
@pytest.mark.parametrize("cid,form", KEYS)
def test_plain_fold_degenerate_bases(srs, oracle, cid, form):
    O = oracle
    bases = PF.degenerate_bases(O, _lib(), cid, form, 1051 + cid)
    ck = PF.fold_key(srs, cid, form, bases)
    fill = O.mont_to_ints(O.SCALAR_FIELD[cid], seeded_scalars(O, cid, N_FULL, 1052, "uniform"))
    for d in DIGITS:
        for name, head in PF.degenerate_heads(_lib(), cid, form, d).items():
            for rest in (None, fill):
                sc = PF.with_head(O, cid, head, rest)
                want = O.msm(cid, sc, bases)
                assert np.array_equal(streamed(srs, ck, sc), want), (name, hex(d), rest is not None)
                if name == "cancel" and rest is None:
                    assert not want.any()                                        # the identity: the all-zero affine encoding
    assert ck.count_off_curve() == 0
    ck.close()


# ---- 5. state between commits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,form", KEYS)
def test_plain_fold_state_between_commits(srs, oracle, keys, vectors, cid, form):
    """Streamed A, resident B, streamed C, streamed A again on one key: nothing of an earlier commit's running buckets or arena is left in a
    later one.  Then A with the fold off: the same point from three whole MSMs."""
    O = oracle
    bases, ck = keys[cid, form]
    A, want_A = vectors[cid, form, "trace", N_FULL]
    C_, want_C = vectors[cid, form, "boundary", N_RAGGED]
    B = seeded_scalars(O, cid, 4000, 1060 + cid, "uniform")
    assert np.array_equal(streamed(srs, ck, A), want_A)
    assert np.array_equal(counted(ck, lambda: ck.commit(dev(B)), 0, 1), O.msm(cid, B, bases[:4000]))
    assert np.array_equal(streamed(srs, ck, C_), want_C)
    assert np.array_equal(streamed(srs, ck, A), want_A)
    with srs.tuning(commit_chunks=CHUNKS, msm_plain_fold=0):
        assert np.array_equal(counted(ck, lambda: ck.commit_upload(A), 0, CHUNKS), want_A)
    assert np.array_equal(streamed(srs, ck, A), want_A)                          # (read per commit: on again)


# ---- 6. the other entries that stream -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,form", KEYS)
def test_plain_fold_upload_columns(srs, oracle, keys, cid, form):
    """Three columns of 1024 rows holding 1024 / 700 / 0 scalars: one chunk per column, the last one padding alone."""
    O = oracle
    bases, ck = keys[cid, form]
    cols = [seeded_scalars(O, cid, n, 1070 + n, "uniform") for n in (1024, 700)] + [np.zeros((0, 4), np.uint64)]
    whole = np.concatenate([np.concatenate([c, np.zeros((1024 - len(c), 4), np.uint64)]) for c in cols])
    with srs.tuning(commit_chunks=CHUNKS):
        got = counted(ck, lambda: ck.commit_upload_columns(cols, 1024), CHUNKS, 1)
    assert np.array_equal(got, O.msm(cid, whole, bases[:N_FULL]))


def test_plain_fold_run_sps_protocol(srs, oracle, keys):
    """run_sps_protocol on a one-lookup structure at k = 10: round 0 is the advice in three streamed chunks and (ls, ts, ms), computed on
    the device, as a further set of the same commit."""
    import space_cases as SC
    import sps_cases as SPS
    bases, ck = keys[0, 2]
    before = ck.plain_stats()
    with srs.tuning(commit_chunks=CHUNKS):
        SPS.run_case(srs, oracle, SC.Spaces.torch_cuda(), (ck, bases), 0, "scalar", 10)
    after = ck.plain_stats()
    assert after["fold_sets"] >= before["fold_sets"] + CHUNKS + 1, (before, after)        # the chunks and the tail set


@pytest.mark.parametrize("cid,form", KEYS)
def test_plain_fold_is_sat_witness_commit(srs, oracle, keys, cid, form):
    """A 5001-element round from host memory: a batch of whole MSMs, nothing folds."""
    from workloads import rand_fe
    S, O = srs, oracle
    bases, ck = keys[cid, form]
    rng = np.random.default_rng(1080 + cid)
    W = [rand_fe(rng, 5001, 0.5), rand_fe(rng, 1 << 11, 0.5)]
    cw = np.stack([O.msm(cid, w, bases[:len(w)]) for w in W])
    with srs.tuning(commit_chunks=CHUNKS):
        assert counted(ck, lambda: S.VanillaFS.is_sat_witness_commit(ck, W, cw), 0, 2) == (0, False)
        W[0][5000] = rand_fe(rng, 1)[0]
        assert S.VanillaFS.is_sat_witness_commit(ck, W, cw) == (1, False)


# ---- 7. bookkeeping -------------------------------------------------------------------------------------------------------------------
def test_plain_fold_stats_of_other_keys(srs, oracle):
    """plain_stats() stays {0, 0} on a default and on a compact key, whatever they commit."""
    O = oracle
    bases = O.make_bases(0, 1091, N_FULL)
    sc = seeded_scalars(O, 0, N_FULL, 1092, "trace")
    want = O.msm(0, sc, bases)
    full = srs.CommitmentKey(0, bases)
    with srs.tuning(msm_compact=1):
        compact = srs.CommitmentKey(0, bases)
    for ck in (full, compact):
        assert not ck.is_plain()
        with srs.tuning(commit_chunks=CHUNKS):
            assert np.array_equal(ck.commit_upload(sc), want)
        assert np.array_equal(ck.commit(sc), want)
        assert ck.plain_stats() == dict(fold_sets=0, reductions=0)
        ck.close()


@pytest.mark.parametrize("cid,form", KEYS)
def test_plain_fold_bookkeeping(srs, oracle, keys, vectors, cid, form):
    O = oracle
    bases, ck = keys[cid, form]
    sc, want = vectors[cid, form, "trace", N_FULL]
    assert np.array_equal(counted(ck, lambda: ck.commit(dev(sc)), 0, 1), want)                    # a resident commit: one reduction
    vs = [seeded_scalars(O, cid, n, 1093 + n, "uniform") for n in (300, 63, 1)] + [np.zeros((0, 4), np.uint64)]
    ws = [O.msm(cid, v, bases[:len(v)]) for v in vs[:3]] + [np.zeros(8, np.uint64)]
    assert np.array_equal(counted(ck, lambda: ck.commit_batch(vs), 0, 3), np.stack(ws))           # the empty vector runs nothing
    small = np.ascontiguousarray(sc[:600])
    with srs.tuning(commit_chunks=CHUNKS):                                                        # 600 scalars: one chunk, nothing to fold
        assert np.array_equal(counted(ck, lambda: ck.commit_upload(small), 0, 1), O.msm(cid, small, bases[:600]))
    assert np.array_equal(streamed(srs, ck, sc), want)
    assert ck.is_plain() and ck.plain_form() == form and ck.table_bytes() == 64 << KEY_LOG        # run state is not table
    st = ck.msm_stats()
    assert (st["slot_sets"], st["hot_sets"], st["redo"]) == (0, 0, 0), st
