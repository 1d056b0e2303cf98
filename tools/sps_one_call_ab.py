"""A/B on the GPU: srs_run_sps_protocol (one call) against the step-wise sequence it replaces, and its _0 route against
srs_commit_upload_columns.  Host advice columns in (pageable NumPy memory, what a Rust Vec is), a device vector and the
commitments / challenges out; bn256, one synthetic key of 2^23 bases.

  python tools/sps_one_call_ab.py OUT.txt [k ...]        (default k = 16 18 20)

Per size: the "scalar" lookup circuit of tests/lookup_cases.py (3 advice columns, one range lookup: run_sps_protocol_2) and a one-gate
circuit without lookups (run_sps_protocol_0) on the same three columns.  The two sides of a pair alternate; every sample ends in a
device synchronise; WARMUP untimed rounds first.  Both sides of the lookup pair must give the same vector, commitments and challenges."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle as O            # noqa: E402
import sirius_amd as S        # noqa: E402

WARMUP, SAMPLES = 3, 12
RO = (5, 4, 10, 10)
FIELD, CURVE = 0, S.CURVE_BN256


def small(vals):
    """(n,) integers below 2^63 -> (n, 4) Montgomery elements"""
    raw = np.zeros((len(vals), 4), dtype=np.uint64)
    raw[:, 0] = vals
    return O.to_mont(FIELD, raw)


def circuit(k, rng):
    X = S.expression
    rows, q = 1 << k, (1 << k) // 4
    s_add = np.zeros(rows, np.uint8); s_add[:q] = 1
    s_rc = np.zeros(rows, np.uint8); s_rc[q:2 * q] = 1
    table = small(np.arange(rows, dtype=np.uint64) % 8)
    a, b = rng.integers(0, 1 << 61, size=rows, dtype=np.uint64), rng.integers(0, 1 << 61, size=rows, dtype=np.uint64)
    c = rng.integers(0, 1 << 61, size=rows, dtype=np.uint64)
    c[:q] = a[:q] + b[:q]
    a[q:2 * q] = rng.integers(0, 8, size=q, dtype=np.uint64)
    cols = [small(a), small(b), small(c)]
    sa, sr, t0 = X.Polynomial(0, 0), X.Polynomial(1, 0), X.Polynomial(2, 0)
    A, B, Cc = [X.Polynomial(3 + i, 0) for i in range(3)]
    gate = X.Product(sa, X.Sum(X.Sum(A, B), X.Negated(Cc)))
    lookup = S.PlonkStructure(FIELD, k, [s_add, s_rc], [table], 3, [gate], lookups=[([X.Product(sr, A)], [t0])])
    plain = S.PlonkStructure(FIELD, k, [s_add, s_rc], [table], 3, [gate])
    assert lookup.num_challenges == 2 and plain.num_challenges == 0
    return lookup, plain, cols


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def line(tag, ms):
    return f"{tag}: median {statistics.median(ms):.3f} ms, min {min(ms):.3f}, max {max(ms):.3f} ({len(ms)} samples)"


def main():
    out_path = sys.argv[1]
    ks = [int(x) for x in sys.argv[2:]] or [16, 18, 20]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    log = open(out_path, "w")
    O.build()

    def emit(s):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()
    emit(f"# srs_run_sps_protocol vs the step-wise sequence; {torch.cuda.get_device_name(0)}; key 2^23 (bn256, synthetic); warm-up {WARMUP}, "
         f"{SAMPLES} samples per side, sides alternating, host clock around a device synchronise")
    ck = S.CommitmentKey.setup_synthetic(CURVE, 1 << 23, seed=9)
    inst = O.ints_to_mont(FIELD, [11, 12])
    zero = np.zeros(4, np.uint64)
    for k in ks:
        rows = 1 << k
        St, Pl, cols = circuit(k, np.random.default_rng(k))
        W = torch.empty((St.num_witness_columns * rows, 4), dtype=torch.int64, device="cuda")
        W0 = torch.empty((3 * rows, 4), dtype=torch.int64, device="cuda")

        def one_call():
            ro = S.PoseidonHash(1, *RO)
            r = St.run_sps_protocol(ck, inst, cols, ro=ro, W=W)
            return r["W"], r["W_commitments"], r["challenges"]

        def step_wise():       # INTEGRATION.md 3, "Lookup prover rounds", every vector kept on the device
            ro = S.PoseidonHash(1, *RO)
            adv = torch.from_numpy(np.concatenate(cols).view(np.int64)).cuda()
            ls, ts, ms = St.lookup_coeff_1(adv, zero)
            w0 = torch.cat([adv] + ls + ts + ms)
            c0 = ck.commit(w0)
            ro.absorb_field(O.ints_to_mont(1, [11, 12]))
            r1 = ro.absorb_point(CURVE, c0).squeeze(128, FIELD)
            hs, gs = St.lookup_coeff_2(ls, ts, ms, r1)
            w1 = torch.cat(hs + gs)
            c1 = ck.commit(w1)
            r2 = ro.absorb_point(CURVE, c1).squeeze(128, FIELD)
            return torch.cat([w0, w1]), np.stack([c0, c1]), np.stack([r1, r2])

        def sps_0():
            return Pl.run_sps_protocol(ck, inst, cols, W=W0)["W_commitments"][0]

        def upload_columns():
            return ck.commit_upload_columns(cols, rows, dev_copy=W0)

        a, b = one_call(), step_wise()
        same = torch.equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        same0 = np.array_equal(sps_0(), upload_columns())
        emit(f"k={k} results equal: lookup pair {same}, _0 pair {same0}")
        assert same and same0
        for pair in (("one_call", one_call, "step_wise", step_wise), ("sps_0", sps_0, "commit_upload_columns", upload_columns)):
            t = {pair[0]: [], pair[2]: []}
            for i in range(WARMUP + SAMPLES):
                for name, fn in ((pair[0], pair[1]), (pair[2], pair[3])):
                    ms, _ = timed(fn)
                    if i >= WARMUP:
                        t[name].append(ms)
            for name in (pair[0], pair[2]):
                emit(line(f"k={k} {name}", t[name]))
        St.close()
        Pl.close()
    log.close()


if __name__ == "__main__":
    main()
