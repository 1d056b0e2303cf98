"""A streamed column commit on sharded keys with a chunk boundary INSIDE a column's data (the column cases of tests/test_commit_gpu.py
take the default cuts: one chunk at their size): shared by the emulator test (tests/test_emu_logic.py) and the GPU test
(tests/test_commit_gpu.py).

Five columns padded to 2^12 rows -- full, short with its data ending in the middle of a stripe (3 * 2^10 + 5 elements), empty, full, 17
elements -- so n = 20 480 against a key of 20 480 bases, under tuning commit_chunks = 4.  On three shards / ranks the chunk boundaries
are multiples of 3 * 2^10: 6 144 / 12 288 / 18 432, the first one inside the short column's data (4 096 .. 7 173)."""
import numpy as np

from conftest import seeded_scalars

ROWS, SL, WORLD, CHUNKS = 1 << 12, 1 << 10, 3, 4
LENS = (ROWS, 3 * SL + 5, 0, ROWS, 17)
N = len(LENS) * ROWS


def equal_cuts(n, align, chunks):
    """commit_cuts (csrc/capi.hip) for a forced number of chunks: equal pieces, rounded up to a multiple of `align`."""
    per = -(-(-(-n // chunks)) // align) * align
    return list(range(0, n, per)) + [n]


def run_chunk_boundary_case(S, O, make_dev, cid=0):
    """make_dev(n): an (n, 4) int64 tensor filled with 7 that the library can write to (the device copy)."""
    cuts = equal_cuts(N, WORLD * SL, CHUNKS)
    assert cuts == [0, 6144, 12288, 18432, 20480] and ROWS < cuts[1] < ROWS + LENS[1] and cuts[1] % SL == 0 and (ROWS + LENS[1]) % SL == 5
    bases = O.make_bases(cid, 31, N)
    v = seeded_scalars(O, cid, N, 43, "trace")
    cols = [v[c * ROWS:c * ROWS + m] for c, m in enumerate(LENS)]
    W = np.zeros((N, 4), np.uint64)                        # util::concatenate_with_padding
    data = np.zeros(N, dtype=bool)
    for c, m in enumerate(LENS):
        W[c * ROWS:c * ROWS + m] = cols[c]
        data[c * ROWS:c * ROWS + m] = True
    want = O.msm(cid, W, bases)
    stripes_of = lambda r: range(r, N // SL, WORLD)
    # the chunks in which a rank owns a stripe: one set of launches each (the last chunk is stripes 18 and 19 -- none of rank 2's)
    sets = [sum(1 for a, b in zip(cuts, cuts[1:]) if any(a <= s * SL < b for s in stripes_of(r))) for r in range(WORLD)]
    assert sets == [4, 4, 3]
    got_of = lambda d: d.cpu().numpy().view(np.uint64).reshape(-1, 4)
    with S.tuning(commit_chunks=CHUNKS):
        # (a) a multi-device key: every shard uploads its stripes, the device copy is assembled on the process's device
        mk = S.CommitmentKey.create_multi(cid, bases, WORLD)
        d = make_dev(N)
        assert np.array_equal(mk.commit_upload_columns(cols, ROWS, dev_copy=d), want)
        assert np.array_equal(got_of(d), W)
        st = mk.msm_stats()
        print("multi-device key:", st, [mk.shard_stats(j) for j in range(WORLD)])
        assert st["slot_sets"] + st["other_sets"] == sum(sets) and st["redo"] == 0, st            # four chunks per shard, as cut above
        for j in range(WORLD):
            mine = sum(int(data[s * SL:(s + 1) * SL].sum()) for s in stripes_of(j))
            assert mk.shard_stats(j)["h2d_bytes"] == 32 * mine, (j, mk.shard_stats(j), mine)
        mk.close()
        # (b) the same key sharded over ranks 0..2 of world 3: partial commitments, own stripes up, foreign stripes untouched
        parts = []
        for r in range(WORLD):
            rk = S.CommitmentKey(cid, bases, rank=r, world=WORLD)
            d = make_dev(N)
            parts.append(rk.commit_upload_columns(cols, ROWS, dev_copy=d))
            got = got_of(d)
            for s in range(N // SL):
                blk = got[s * SL:(s + 1) * SL]
                assert np.array_equal(blk, W[s * SL:(s + 1) * SL]) if s % WORLD == r else (blk == 7).all(), (r, s)
            st = rk.msm_stats()
            assert st["slot_sets"] + st["other_sets"] == sets[r] and st["redo"] == 0, (r, st)
            rk.close()
        assert np.array_equal(S.point_sum(cid, np.stack(parts)), want)
