"""Wall time of ck.commit on device-resident scalars over a range of sizes (one key of 2^24 bases); run once per setting of the
tunables (SRS_TEST_TUNING="msm_sort=2,..." of the Python mirror: the key is created under them, so msm_compact / msm_plain choose its
form; the set-up line prints plain=0 / 1 / 2, the plain form).  usage: python tools/msm_probe.py [log_key] [sizes...] [--setup] [--spread] [--batch COUNT N] [--streamed N]
  --setup          also print the key's set-up time and srs_ck_table_bytes
  --spread         print min - max over the repeats instead of their mean (one synchronised call per repeat)
  --batch C N      then a commit_batch of C vectors of N uniform scalars
  --streamed N     then the streamed commit of N scalars (55 % zero / 45 % uniform, page-locked source, device copy kept)"""
import sys, time, os
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sirius_amd as S

args = sys.argv[1:]


def flag(name, nvals=0):
    """pops `name` and its values from the argument list -> None when absent, else the list of its int values"""
    if name not in args:
        return None
    at = args.index(name)
    vals = [int(x) for x in args[at + 1:at + 1 + nvals]]
    del args[at:at + 1 + nvals]
    return vals


setup, spread, batch, streamed = flag("--setup"), flag("--spread"), flag("--batch", 2), flag("--streamed", 1)
log_key = int(args[0]) if args else 24
sizes = [int(x) for x in args[1:]] or [1 << 20, 3 << 20, 5 << 20, 12 << 20, 1 << 24]
tag = os.environ.get("PROBE_TAG", "")
REPS = 5


def timed(fn):
    """two warm-up calls, then REPS calls -> 'mean' or 'min - max' in ms, and the mean"""
    fn(); fn()
    torch.cuda.synchronize()
    if spread is None:
        t = time.perf_counter()
        for _ in range(REPS):
            fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t) / REPS * 1e3
        return f"{ms:8.3f} ms", ms
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return f"{min(ts):8.3f} - {max(ts):8.3f} ms", sum(ts) / REPS


torch.cuda.synchronize()
t0 = time.perf_counter()
ck = S.CommitmentKey.setup_synthetic(0, 1 << log_key, seed=3)
torch.cuda.synchronize()
if setup is not None:
    print(f"key_setup 2^{log_key}: {time.perf_counter() - t0:6.3f} s  table_bytes={ck.table_bytes()} ({ck.table_bytes() / 2**30:.2f} GiB) "
          f"plain={ck.plain_form()} compact={int(ck.is_compact())} wide_table={int(ck.has_wide_table())}  tag={tag}", flush=True)
g = torch.Generator(device="cuda").manual_seed(1)


def scalars(n, kind):
    v = torch.randint(0, 1 << 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)
    v[:, 3] &= (1 << 60) - 1
    if kind == "trace":
        v[torch.rand(n, device="cuda", generator=g) < 0.55] = 0
    return v


for n in sizes:
    for kind in ("uniform", "trace"):
        v = scalars(n, kind)
        txt, ms = timed(lambda: ck.commit(v))
        print(f"n={n:>9} {kind:8s} {txt}  {n / ms / 1e3:8.1f} M scalars/s  tag={tag}", flush=True)
if batch:
    vs = [scalars(batch[1], "uniform") for _ in range(batch[0])]
    txt, _ = timed(lambda: ck.commit_batch(vs))
    print(f"batch {batch[0]} x {batch[1]} uniform {txt}  {ck.plain_batch_stats()}  tag={tag}", flush=True)
if streamed:
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from workloads import trace_like
    n = streamed[0]
    hb = S.HostBuffer(n)
    hb.array[:] = trace_like(np.random.default_rng(1), n)
    d = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    txt, _ = timed(lambda: ck.commit_upload(hb.array, dev_copy=d))
    print(f"streamed commit n={n} {txt}  point={ck.commit_upload(hb.array, dev_copy=d).tobytes().hex()[:16]}  {ck.msm_stats()}  {ck.plain_stats()}  tag={tag}", flush=True)
