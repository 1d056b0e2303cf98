"""Full vs compact commitment keys (tuning msm_compact = 0 / 1 / 2: full, compact, compact that may hold the 7-window wide table) on one
device: key setup time, table bytes and wide_table at 2^log_key on both curves, then the streamed commit of a 12 * 2^k witness (55 % zero
/ 45 % uniform, page-locked source, device copy kept -- bench.py's witness commit) on bn256.  The resident MSM is tools/msm_probe.py
under SRS_TEST_TUNING=msm_compact=1 (or 2).
usage: python tools/compact_key_probe.py [log_key] [k]     (k = 0: key setup only)"""
import os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import sirius_amd as S
from workloads import trace_like

log_key = int(sys.argv[1]) if len(sys.argv) > 1 else 24
k = int(sys.argv[2]) if len(sys.argv) > 2 else 20


def make(cid, n, compact):
    torch.cuda.synchronize()
    t = time.perf_counter()
    with S.tuning(msm_compact=compact):
        ck = S.CommitmentKey.setup_synthetic(cid, n, seed=3)
    torch.cuda.synchronize()
    return ck, time.perf_counter() - t


for cid in (S.CURVE_BN256, S.CURVE_GRUMPKIN):
    for compact in (0, 1, 2, 0, 1, 2):
        ck, dt = make(cid, 1 << log_key, compact)
        print(f"key_setup curve={cid} 2^{log_key} compact={compact}: {dt:6.3f} s  table_bytes={ck.table_bytes()} ({ck.table_bytes() / 2**30:.2f} GiB) "
              f"wide_table={int(ck.has_wide_table())}", flush=True)
        ck.close()

if k == 0:
    sys.exit(0)
n = 12 << k
hb = S.HostBuffer(n)
hb.array[:] = trace_like(np.random.default_rng(1), n)
d = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
keys = {c: make(S.CURVE_BN256, n, c)[0] for c in (0, 1, 2)}
ref = None
for rnd in range(3):                     # the two keys alternate: drift of the box shows as a spread between rounds
    for c in (0, 1, 2):
        ck = keys[c]
        for _ in range(2):
            out = ck.commit_upload(hb.array, dev_copy=d)
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            t = time.perf_counter()
            out = ck.commit_upload(hb.array, dev_copy=d)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
        ref = out if ref is None else ref
        assert np.array_equal(out, ref), "compact and full keys disagree"
        print(f"streamed commit 12*2^{k} compact={c} round {rnd}: median {sorted(ts)[2]:7.3f} ms  min {min(ts):7.3f}  max {max(ts):7.3f}  {ck.msm_stats()}", flush=True)
