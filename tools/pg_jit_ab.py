"""A/B of the ProtoGalaxy leaf kernels with the intended leaf rows (reference_compat=False) on the GPU: interpreter (tuning no_jit) or
ahead-of-time kernels against the run-time compiled ones bounded for two waves per SIMD and for one (tuning pg_jit_waves; pg_jit_force
sends the ahead-of-time gate set [5, 3] through them).  Per variant: `repeats` x (one warm-up prove, then the mean of `reps` proves with
given alpha / gamma) -> one JSON line with prove_ms and the leaf kernels' ms per launch (srs_profile_get).  With SRS_JIT_DUMP=<dir> the
library keeps every compiled unit (srs_jit_<n>.co, in the order of the `compiled` lines printed here) for llvm-readelf --notes.
The record: profiles/pg_leaves_jit_ab.txt.      usage: python tools/pg_jit_ab.py [--k-main 20] [--k-high 22] [--reps 5] [--repeats 2]"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cheap_fe(rng, n):
    """n field elements below 2^252 (timing only: the kernels' work does not depend on the values)"""
    a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(3)
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k-main", type=int, default=20)
    ap.add_argument("--k-high", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=2)
    args = ap.parse_args()
    import torch
    import sirius_amd as S
    from sirius_amd import protogalaxy as PG
    from sirius_amd.field import FR, ints_to_mont
    from sirius_amd.workloads import gates_for, high_degree_gate
    g53, nfix53, nadv53 = gates_for([5, 3])
    sets = [("main_2", args.k_main, gates_for([2]), False),
            ("main_5_3", args.k_main, (g53, nfix53, nadv53), True),
            ("degree15_5_3", args.k_high, ([high_degree_gate(5, 15, 0, 0, 0, nfix53), g53[1]], nfix53, nadv53), False)]
    S.profile_enable(True)
    for name, k, (gates, nfix, nadv), has_aot in sets:
        rng = np.random.default_rng(k)
        rows = 1 << k
        fixed = [cheap_fe(rng, rows) for _ in range(nfix)]
        Ws = [torch.from_numpy(cheap_fe(rng, nadv * rows).view(np.int64)).cuda() for _ in range(2)]
        rnd = random.Random(4)
        m = lambda v: ints_to_mont(0, list(v))
        variants = [("ahead-of-time" if has_aot else "interpreter", dict(no_jit=1)),
                    ("compiled, 2 waves", dict(pg_jit_waves=2, **({"pg_jit_force": 1} if has_aot else {}))),
                    ("compiled, 1 wave", dict(pg_jit_waves=1, **({"pg_jit_force": 1} if has_aot else {})))]
        for label, tun in variants:
            with S.tuning(**tun):
                St = S.PlonkStructure(0, k, [], fixed, nadv, gates)
                secs = None
                if "no_jit" not in tun:
                    secs = St.prepare_pg_leaves()
                    print(f"compiled {name} [{label}] in {secs:.2f} s", flush=True)
                kind = St.kernel_kind(2)
                ctx = PG.PolyContext(St, 1)
                betas, delta = m([rnd.randrange(FR) for _ in range(ctx.betas_count)]), m([rnd.randrange(FR)])[0]
                alpha, gamma = m([rnd.randrange(FR)])[0], m([rnd.randrange(FR)])[0]
                prove = lambda: PG.prove(ctx, betas, delta, Ws, alpha=alpha, gamma=gamma, reference_compat=False, fold=False)
                runs = []
                for _ in range(args.repeats):
                    prove()
                    torch.cuda.synchronize()
                    S.profile_reset()
                    t0 = time.perf_counter()
                    for _ in range(args.reps):
                        prove()
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) / args.reps * 1e3
                    prof = {}
                    for kn in ("pg_F_leaves", "pg_G_leaves"):
                        st = S.profile_get(kn)
                        if st and st["launches"]:
                            prof[kn + "_ms"] = round(st["total_ms"] / st["launches"], 4)
                    runs.append(dict(prove_ms=round(dt, 3), **prof))
                print(json.dumps(dict(gate_set=name, k=k, variant=label, kernel_kind=kind, compile_s=secs, runs=runs)), flush=True)
                St.close()
        del Ws, fixed


if __name__ == "__main__":
    main()
