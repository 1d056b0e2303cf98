"""CPU, world_size 2 over gloo: the multi-GPU MSM path (sharded keys -> per-rank partial -> all-gather ->
host sum).  The kernels run through the logic emulator (tests/emu) because there is no GPU here;
sharding arithmetic, the exchange and the combination are the product's own code."""
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT


def _free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return str(so.getsockname()[1])

WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["SRS_ROOT"]); sys.path.insert(0, os.path.join(os.environ["SRS_ROOT"], "tests"))
import torch, torch.distributed as dist
dist.init_process_group(backend="gloo")
rank, world = dist.get_rank(), dist.get_world_size()
import sirius_amd._lib as L
L.load(os.path.join(os.environ["SRS_ROOT"], "tests", "emu", "libsirius_emu.so"))
import sirius_amd as S
import oracle as O
from conftest import seeded_scalars
from sirius_amd.distributed import all_gather_commitments
ok = True
for cid, N, n in ((0, 2600, 2600), (1, 3000, 2047)):
    full = S.CommitmentKey.setup_synthetic(cid, N, seed=3).bases()
    ck = S.CommitmentKey.setup_synthetic(cid, N, seed=3, rank=rank, world=world)
    sc = seeded_scalars(O, cid, n, 9, "trace" if cid else "uniform")
    got = all_gather_commitments(cid, ck.commit(sc))
    ok &= bool(np.array_equal(got, O.msm(cid, sc, full[:n])))
    batch = all_gather_commitments(cid, ck.commit_batch([sc[:1500], sc[:7]]))
    ok &= bool(np.array_equal(batch[0], O.msm(cid, sc[:1500], full[:1500])) and np.array_equal(batch[1], O.msm(cid, sc[:7], full[:7])))
t = torch.tensor([1 if ok else 0]); dist.all_reduce(t, op=dist.ReduceOp.MIN)
dist.destroy_process_group()
sys.exit(0 if int(t.item()) == 1 else 1)
'''


def test_sharded_commit_world2_gloo(tmp_path, oracle):
    emu_dir = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["make", "-C", emu_dir, "-j4"], stdout=subprocess.DEVNULL)
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, SRS_ROOT=ROOT, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


PROVE_WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["SRS_ROOT"]); sys.path.insert(0, os.path.join(os.environ["SRS_ROOT"], "tests"))
import torch, torch.distributed as dist
dist.init_process_group(backend="gloo")
rank, world = dist.get_rank(), dist.get_world_size()
import sirius_amd._lib as L
L.load(os.path.join(os.environ["SRS_ROOT"], "tests", "emu", "libsirius_emu.so"))
import sirius_amd as S
import oracle as O
from oracle import expr as OE
from sirius_amd.distributed import all_gather_commitments
from test_sangria_gpu import _oracle_gates
from workloads import gates_for, rand_fe
field, curve, k, gate_T = 1, 1, 11, [2]
rows = 1 << k
gates, nfix, nadv = gates_for(gate_T)
rng = np.random.default_rng(77)                       # same stream on every rank: identical inputs
fixed = [rand_fe(rng, rows, 0.3) for _ in range(nfix)]
W1, W2, E = rand_fe(rng, nadv * rows), rand_fe(rng, nadv * rows), rand_fe(rng, rows)
St = S.PlonkStructure(field, k, [], fixed, nadv, gates)
St.set_shard(rank, world)
nch = St.num_challenges
u1c, u1u, u2c, r = rand_fe(rng, nch), rand_fe(rng, 1)[0], rand_fe(rng, nch), rand_fe(rng, 1)[0]
bases = O.make_bases(curve, 9, rows)
ck = S.CommitmentKey(curve, bases, rank=rank, world=world)
# VanillaFS::prove, sharded: local cross-term stripes -> partial commitments -> all-gather -> host sum; folds on local data
terms, partial = S.VanillaFS.commit_cross_terms(ck, St, u1c, u1u, W1, u2c, W2)
commits = all_gather_commitments(curve, partial)
acc = S.RelaxedPlonkWitness(field, [W1], E).fold([W2], terms, r)
ch = S.VanillaFS.cross_term_challenges(u1c, u1u, u2c, field)
_, exp = OE.cross_terms_oracle(O, field, _oracle_gates(gate_T), 0, nfix, nadv, [], fixed, W1, W2, ch)
mine = ((np.arange(rows) >> 10) % world) == rank
ok = len(terms) == len(exp) == St.num_cross_terms
rb = lambda x: np.broadcast_to(x, (rows, 4)).copy()
Eo, rk = E.copy(), r.reshape(1, 4).copy()
for j, (t, e) in enumerate(zip(terms, exp)):
    ok &= bool(np.array_equal(t[mine], e[mine]) and not t[~mine].any())
    ok &= bool(np.array_equal(commits[j], O.msm(curve, e, bases)))           # the partials add up to commit(T_k) of ALL rows
    Eo = O.fe_add(field, Eo, O.fe_mul(field, rb(rk[0]), e))
    rk = O.fe_mul(field, rk, r.reshape(1, 4))
ok &= bool(np.array_equal(acc.E[mine], Eo[mine]) and np.array_equal(acc.E[~mine], E[~mine]))   # error fold: this rank's stripes
Wo = O.fe_add(field, W1, O.fe_mul(field, np.broadcast_to(r, W2.shape).copy(), W2))
ok &= bool(np.array_equal(acc.W[0], Wo))                                                       # witness fold: every row
t = torch.tensor([1 if ok else 0]); dist.all_reduce(t, op=dist.ReduceOp.MIN)
dist.destroy_process_group()
sys.exit(0 if int(t.item()) == 1 else 1)
'''


def test_sharded_prove_world2_gloo(tmp_path, oracle):
    """bench.py's N > 1 prove: row-sharded cross terms (srs_structure_set_shard) + sharded key + all-gather of the partial
    commitments + folds, two processes over gloo; every rank checks its stripes and the combined commitments."""
    emu_dir = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["make", "-C", emu_dir, "-j4"], stdout=subprocess.DEVNULL)
    script = tmp_path / "prove_worker.py"
    script.write_text(PROVE_WORKER)
    env = dict(os.environ, SRS_ROOT=ROOT, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


PG_WORKER = r'''
import os, sys, random
import numpy as np
sys.path.insert(0, os.environ["SRS_ROOT"]); sys.path.insert(0, os.path.join(os.environ["SRS_ROOT"], "tests"))
import torch, torch.distributed as dist
dist.init_process_group(backend="gloo")
rank, world = dist.get_rank(), dist.get_world_size()
import sirius_amd._lib as L
L.load(os.path.join(os.environ["SRS_ROOT"], "tests", "emu", "libsirius_emu.so"))
import sirius_amd as S
import oracle as O
from oracle import expr as OE, protogalaxy as OPG, pyref as P
from sirius_amd import protogalaxy as PG
from sirius_amd.distributed import all_gather_commitments, all_gather_field_sum
from workloads import gates_for, rand_fe
k, gate_T = 11, [5, 3]
rows = 1 << k
gates, nfix, nadv = gates_for(gate_T)
og, fo, ao = [], 0, 0
for T in gate_T:
    og.append(OE.main_gate_expression(T, 0, fo, ao, nfix)); fo += 2 * T + 5; ao += T + 2
rng = np.random.default_rng(5)                         # same stream on every rank: identical inputs
fixed = [rand_fe(rng, rows, 0.3) for _ in range(nfix)]
Ws = [rand_fe(rng, nadv * rows) for _ in range(2)]
mine = np.tile(((np.arange(rows) >> 10) % world) == rank, nadv)
junk = np.random.default_rng(100 + rank)
local = [np.where(mine[:, None], w, rand_fe(junk, nadv * rows)) for w in Ws]      # other ranks' stripes: garbage that must never be read
St = S.PlonkStructure(0, k, [], fixed, nadv, gates)
St.set_shard(rank, world)
ctx = PG.PolyContext(St, 1)
oS = OPG.Structure(O, og, k, [], fixed, nadv, 0)
octx = oS.context(1)
rnd = random.Random(8)
betas = OPG.new_accumulator_betas(rnd.randrange(P.FR), ctx.betas_count)
delta, alpha = rnd.randrange(P.FR), rnd.randrange(P.FR)
m = lambda v: O.ints_to_mont(O.FR, list(v))
ok = True
pF = all_gather_field_sum(0, PG.compute_F(ctx, m(betas), m([delta])[0], local[0], reference_compat=False))
ok &= O.mont_to_ints(O.FR, pF) == OPG.compute_F_fast(oS, octx, betas, delta, Ws[0], [], False)
bs = OPG.beta_stroke(betas, alpha, delta)
pG = all_gather_field_sum(0, PG.compute_G(ctx, m(bs), local, reference_compat=False))
ok &= O.mont_to_ints(O.FR, pG) == OPG.compute_G_fast(oS, octx, bs, Ws, [[] for _ in Ws], False)
pe = all_gather_field_sum(0, PG.evaluate_e_from_trace(ctx, m(betas), local[0], reference_compat=False))
ok &= O.mont_to_ints(O.FR, pe) == [OPG.evaluate_e_fast(oS, octx, betas, Ws[0], [], False)]
# the whole-prove entry refuses a sharded structure (its challenges would come from partial polynomials)
try:
    PG.prove(ctx, m(betas), m([delta])[0], local, alpha=m([alpha])[0], gamma=m([alpha])[0], reference_compat=False)
    ok = False
except Exception:
    pass
# witness commit through the sharded key: only this rank's stripes go up, the partial commitments add up to the commitment
n = nadv * rows
bases = O.make_bases(0, 9, n)
ck = S.CommitmentKey(0, bases, rank=rank, world=world)
dev = torch.full((n, 4), 7, dtype=torch.int64)
got = all_gather_commitments(0, ck.commit_upload(Ws[1], dev_copy=dev))
ok &= bool(np.array_equal(got, O.msm(0, Ws[1], bases)))
d = dev.numpy().view(np.uint64)
ok &= bool(np.array_equal(d[mine], Ws[1][mine]) and (d[~mine] == 7).all())
t = torch.tensor([1 if ok else 0]); dist.all_reduce(t, op=dist.ReduceOp.MIN)
dist.destroy_process_group()
sys.exit(0 if int(t.item()) == 1 else 1)
'''


def test_sharded_protogalaxy_world2_gloo(tmp_path, oracle):
    """bench.py's N > 1 ProtoGalaxy prove: leaves sharded by the key's row stripes (srs_structure_set_shard), partial F / G / e
    all-gathered and added == the oracle's polynomials although every rank holds garbage in the other rank's stripes; the
    sharded witness commit uploads this rank's stripes only."""
    emu_dir = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["make", "-C", emu_dir, "-j4"], stdout=subprocess.DEVNULL)
    script = tmp_path / "pg_worker.py"
    script.write_text(PG_WORKER)
    env = dict(os.environ, SRS_ROOT=ROOT, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2", HIPEMU_THREADS="4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


def test_bench_world2_matches_world1_on_emulator(tmp_path):
    """bench.py --gpus 2 (torchrun, gloo, emulator) folds the same chain as --gpus 1: MSMs sharded by key stripes, ProtoGalaxy
    leaves and cross terms by row stripes, witness uploads of 1 / world, partial commitments and polynomials exchanged --
    `state_digest` (e, the instance commitments, the support accumulator's commitments after the same steps) is identical."""
    import json
    emu_dir = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["make", "-C", emu_dir, "-j4"], stdout=subprocess.DEVNULL)
    common = ["--emu", "--k", "11", "--log-key", "15", "--steps", "1", "--warmup", "0", "--no-extras", "--no-cpu-baseline"]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2", HIPEMU_THREADS="4")
    # no torchrun around the 2-rank runs: `bench.py --gpus 2` launches its two ranks itself (spawn_ranks).  The four runs are independent:
    # side by side (N > 1 secondary object in the first 2-rank run: the sharded MSM microbenchmark)
    env2 = {k: v for k, v in env.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    bench = [sys.executable, os.path.join(ROOT, "bench.py")]
    jobs = {"r1": (bench + ["--gpus", "1"] + common, env),
            "r2": (bench + ["--gpus", "2", "--dist-backend", "gloo", "--full"] + [a for a in common if a != "--no-extras"], env2),
            "r1t": (bench + ["--gpus", "1", "--leaf-rows", "true"] + common, env),
            "r2t": (bench + ["--gpus", "2", "--dist-backend", "gloo", "--leaf-rows", "true"] + common, env2),
            "r3s": (bench + ["--gpus", "3", "--single-process"] + common, env2),       # one process, multi-device keys of 3 logical shards
            "r2th": (bench + ["--gpus", "2", "--threads"] + common, env2)}            # one process, one host thread per (logical) device, sharded handles
    procs = {k: subprocess.Popen(a, cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for k, (a, e) in jobs.items()}
    res = {}
    for k, p in procs.items():
        so, se = p.communicate(timeout=900)
        res[k] = (p.returncode, so, se)
        assert p.returncode == 0, (k, so[-2000:], se[-4000:])
    last_json = lambda so: json.loads([l for l in so.strip().splitlines() if l.startswith("{")][-1])
    one, two = last_json(res["r1"][1]), last_json(res["r2"][1])
    assert two["n_gpus"] == 2 and two["config"]["parallelism"] == "msm+leaf-shard2"
    assert one["state_digest"] == two["state_digest"]
    assert one["config"]["leaf_rows"] == "compat" and one["config"]["challenges"] == "poseidon-ro"      # the headline configuration
    assert two["secondary"]["microbench_msm_sharded"]["msm_uniform"]["n_gpus"] == 2
    thr = last_json(res["r2th"][1])           # r06: srs_init_thread -- the process-per-GPU decomposition on threads, exchanges in memory
    assert thr["n_gpus"] == 2 and thr["config"]["parallelism"].startswith("msm+leaf-shard2-threads") and thr["state_digest"] == one["state_digest"]
    multi = last_json(res["r3s"][1])
    assert multi["n_gpus"] == 3 and multi["config"]["parallelism"].startswith("msm-multi3-single-process") and multi["state_digest"] == one["state_digest"]
    # ... and every link carried its third of the 12 * 2^11 * 32 B witness, once (srs_ck_shard_stats): nothing goes to device 0 first
    md = multi["multi_device"]
    assert md["shards"] == 3 and sum(md["h2d_bytes_per_commit"]) == 12 * 2048 * 32 and max(md["h2d_bytes_per_commit"]) == 12 * 2048 * 32 // 3
    assert md["peer_bytes_per_commit"][0] == 0 and md["peer_bytes_per_commit"][1:] == md["h2d_bytes_per_commit"][1:]
    # the intended leaf rows shard the same way
    d1, d2 = last_json(res["r1t"][1])["state_digest"], last_json(res["r2t"][1])["state_digest"]
    assert d1 == d2 and d1 != one["state_digest"]
