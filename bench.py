#!/usr/bin/env python
"""bench.py -- IVC fold-steps/s of the folding-prover hot path on synthetic Poseidon-shaped traces (MI355X).

Default workload = BASELINE.json configs[2], the north-star target: one `CyclefoldIVC::next`
(reference src/ivc/cyclefold/incrementally_verifiable_computation/mod.rs:210-335; bench benches/cyclefold_poseidon.rs:27-34,116-126)
at k = 20 with a 2^24 commitment key.  One "step" = the hot-path work of one `next`, in the reference's order:
  A. ProtoGalaxy::prove on the primary (bn256) circuit, src/nifs/protogalaxy/mod.rs:400-481:
       compute_F (2^21 leaves), compute_G (accumulator + incoming trace), compute_K_from_G (256 points), calculate_e,
       fold_instance (host scalar-muls, off the critical path), fold_witness (12 * 2^20)
  B. fold_support_circuit, :404-473 -- the support circuit (grumpkin, k = 15, support_circuit/tiny_gate.rs:56-82):
       its witness arrives from the host and is committed (3 * 2^15 scalars), then SangriaFS::prove: 2 cross terms evaluated and
       committed (batched MSM), witness and error-vector folds
  C. the new primary witness arrives FROM THE HOST (halo2 synthesis is CPU work, src/table/circuit_runner.rs:71-107) and is
       committed: 12 * 2^20 scalars -- uploaded inside the timed region, in chunks that overlap the MSM of the
       chunks already in HBM (srs_commit_upload); the device copy is the incoming trace of the next step
Accumulators, fixed columns and the expanded keys stay resident in HBM.  Defaults = the reference's computation: every challenge is
squeezed from the library's off-circuit Poseidon sponge over the transcript (`--challenges poseidon-ro`; `seeded` takes constants), and
every ProtoGalaxy leaf is evaluated at row 0 as the reference does (`--leaf-rows compat`: src/plonk/mod.rs:714); the
intended computation -- the leaf's own row, `--leaf-rows true` -- is timed beside it as `secondary.true_leaf_rows`.
`--witness survey` commits SURVEY.md 8d(ii)'s value mixture instead of the bench witness (hot buckets on every commit; by default
reported as `secondary.survey_mixture`); `--verify` recomputes the first step on the CPU oracle (oracle/chain.py) and prints both digests.

`--config sangria` runs BASELINE configs[1] (one SangriaIVC::fold_step at k = 17) as the main line instead; by default it is
reported as a secondary object next to the 2^24 MSM / NTT microbenchmark (configs[4]), each with its own roofline.

Multi-GPU (torchrun, one rank per GPU): every MSM is sharded block-cyclically over the ranks, the 64-byte partial commitments
are all-gathered over RCCL and summed on the host; the row programs are sharded by the same row stripes (cross terms; the
ProtoGalaxy leaves: partial F / G polynomials all-gathered and added), the witness upload is 1 / world per rank; K, the transcript
and the folds over whole vectors stay replicated.  One IVC chain is sequential, so this is STRONG scaling of a single step.
`--gpus N --threads` runs the same decomposition in ONE process, one host thread per GPU (srs_init_thread), partial sums exchanged in memory;
`--gpus N --single-process` uses multi-device keys instead (the library owns the devices; the prove stays on device 0).

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times --steps steps and prints the headline; everything else it used
to measure beside the headline -- the roofline and per-kernel timers, the secondary objects, the CPU baseline, the N > 1 sharded MSM
-- runs with `--full` only.  `roofline` (--full): dominant kernel = MSM bucket accumulation; achieved = 96 B x scalars / launch time
(HIP events on the launch stream, inside the library).  `cpu_baseline` (--full): the CPU oracle (oracle/, a C port of the reference's
algorithms -- the Rust reference cannot be built in this image) on ONE step of the same workload, rank 0 / N = 1 only.
`--dump-outputs DIR` writes what the last timed step handed its caller as DIR/<name>.npy (see dump_outputs).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s; 6.29 TB/s measured copy)
MSM_BYTES_PER_SCALAR = 96.0    # 64 B base + 32 B scalar, each read once
NTT_BYTES_PER_ELEMENT = 64.0   # read once + write once
# ALU side note: the bucket accumulation is integer-multiplier bound.  One mixed addition = 8 products + 2 squares on the
# 9 x 29-bit limb form = 8 * 171 + 2 * 135 multiplier instructions (v_mad_u64_u32 / v_mul_lo_u32), minus the 81 + 9 of the one
# Montgomery reduction that Y3 = t r - Y1 ppp shares since r03 (Fp29::mul2); the chip issues 31.2 T v_mad_u64_u32 per second
# (profiles/r02_ubench29_gfx950.txt: 50.7 lane-ops/clk/CU x 256 CUs x 2.4 GHz).
# HIP events on every n-th bucket-accumulation launch of the headline loop.  1 = every launch: the rocprofv3 trace shows 6-10 us of idle device in front of an
# event-bracketed launch, but with 1 launch in 4 sampled the step is the same within noise (10.72 / 10.74 against 10.74 / 10.71 ms, profiles/r05_ab_small_msm.txt)
PROF_SAMPLE = int(os.environ.get("SRS_BENCH_PROF_SAMPLE", "1"))
MAD_ISSUE_PER_S = 31.16e12
MADD_MULT_INSNS = 8 * 171 + 2 * 135 - 90


# No multi-GPU node was available to r01-r06: what the first measured SCALE record can be diffed against (derived from the
# kernel trace of the N = 1 step: per-row / per-scalar work divides by N, the chain's latency-bound part does not).
PREDICTED_SCALING = {
    "note": "PREDICTION, not a measurement: k = 20 CycleFold step; strong scaling of ONE sequential chain",
    "process_per_gpu": {
        "how": "bench.py --gpus N (torchrun or self-launched): MSMs, leaves, cross terms, folds and the witness upload sharded by key / row stripes; RCCL all-gathers",
        "ms_per_step": {"1": 10.5, "2": 7.1, "4": 4.6, "8": 3.6}, "speedup": {"1": 1.0, "2": 1.5, "4": 2.3, "8": 2.9},
        "divisible_ms_at_1": 8.0, "replicated_ms": 2.5, "per_rank_overhead_ms_at_n_gt_1": 0.55,
        "replicated": "transcript (Poseidon, host) 0.35, compute_F tree upper levels + K + e 0.35, bucket reductions + host finish 0.3, k_plan_s / "
                      "k_hist floors 0.07 per chunk (10 chunks at N <= 2, 2 at N >= 4), support circuit's latency-bound MSM 0.5, step-wise calls + five <= 2 KB all-gathers 0.45"},
    "single_process": {
        "how": "bench.py --gpus N --single-process (srs_ck_create_multi: what a single-process Rust IVC driver calls): every shard streams ITS stripes of the witness "
               "over its own link, overlapped with its MSM; the device copy is assembled on device 0 by peer copies; prove and support circuit on device 0",
        "ms_per_step": {"1": 10.5, "2": 7.2, "4": 5.0, "8": 3.9}, "speedup": {"1": 1.0, "2": 1.5, "4": 2.1, "8": 2.7},
        "divisible_ms_at_1": 8.0, "device0_ms": 1.9, "per_commit_overhead_ms_at_n_gt_1": 0.5,
        "device0": "srs_pg_prove 0.87 (F / G / K / e + transcript), srs_sangria_prove_incoming 0.63 (the support key is a single-device key), Python 0.1, "
                   "the deferred witness fold 0.24 under the upload; per commit: slot + bucket reductions per shard 0.3, worker hand-off and the peer-copy tail 0.2"},
    "msm_2p24_uniform_ms": {"1": 19.3, "2": 10.0, "4": 5.3, "8": 3.0},
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="cyclefold", choices=["cyclefold", "sangria"])
    ap.add_argument("--k", type=int, default=0, help="log2 rows (default: 20 for cyclefold, 17 for sangria)")
    ap.add_argument("--log-key", type=int, default=0, help="log2 commitment-key length (default: 24 / 21)")
    ap.add_argument("--leaf-rows", default="compat", choices=["true", "compat"],
                    help="ProtoGalaxy leaf row: row 0 like the reference (default: bit-exact with src/plonk/mod.rs:714, SURVEY.md Q1) "
                         "or the leaf's own row (`true`: the intended computation, reported as secondary.true_leaf_rows by default)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: roofline and per-kernel timers, the secondary objects and the CPU baseline (a plain run "
                         "times the headline only)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float64, each 64-bit limb as two "
                         "exact 32-bit words; vectors longer than 2^16 rows as a fixed, seeded sample of rows)")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the secondary objects (k=17 Sangria step, 2^24 MSM / NTT)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--resident", action="store_true",
                    help="time the step with its inputs already in HBM (the new witness and the support trace are not uploaded inside the step): "
                         "what the default run reports as secondary.device_resident; the headline keeps the upload inside the step")
    ap.add_argument("--challenges", default="poseidon-ro", choices=["poseidon-ro", "seeded"],
                    help="poseidon-ro (default): every challenge is squeezed from the off-circuit Poseidon oracle over the transcript, as the "
                         "reference does (protogalaxy/mod.rs:80-133, sangria/mod.rs:162-179); seeded: constants (no oracle on the critical path)")
    ap.add_argument("--ro-challenge", action="store_true", help="(r02 spelling of --challenges poseidon-ro; now the default)")
    ap.add_argument("--cpu-threads", type=int, default=0)
    ap.add_argument("--witness", default="bench", choices=["bench", "survey"],
                    help="bench (default): 55 %% zero / 45 %% uniform scalars, 7.2 bucket additions per scalar, no hot bucket; survey: SURVEY.md "
                         "8d(ii)'s mixture as canonical values (55 %% zero, 20 %% bits, 15 %% < 2^64, 10 %% uniform): ~2.3 additions per scalar, "
                         "bucket 0 hot in every chunk (slot mode's overflow kernels on every set)")
    ap.add_argument("--verify", action="store_true",
                    help="checker, outside the timed region: the chain's FIRST step is recomputed on the CPU oracle (oracle/chain.py) and both "
                         "digests are printed as `verify` (k = 20: ~10 s of CPU)")
    ap.add_argument("--emu", action="store_true",
                    help="harness self-test without a GPU: loads the CPU logic emulator (tests/emu, test infrastructure) and keeps "
                         "'device' tensors in host memory; use a tiny --k.  The numbers it prints are meaningless")
    ap.add_argument("--single-process", action="store_true",
                    help="with --gpus N: ONE process, the commitment keys are multi-device keys (srs_ck_create_multi: the library owns N devices / "
                         "shards, partitions the scalars, adds the partial sums on the host) -- the path a single-process Rust IVC driver calls. "
                         "More logical shards than physical devices are allowed (shard d runs on device d % count)")
    ap.add_argument("--threads", action="store_true",
                    help="with --gpus N: ONE process, N host threads, thread r bound to device r %% count (srs_init_thread) with its own SHARDED handles -- "
                         "the process-per-GPU decomposition (commits, leaves, cross terms, folds and uploads sharded by stripes) without processes and "
                         "without a collective: partial commitments / polynomials are exchanged in memory")
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL, default) | gloo (CPU exchange; lets 2 ranks share one GPU in tests)")
    args = ap.parse_args()
    args.ro_challenge = args.challenges == "poseidon-ro" or args.ro_challenge
    # a plain run is the headline alone: the secondary objects and the CPU baseline need --full
    args.no_extras = args.no_extras or not args.full
    args.no_cpu_baseline = args.no_cpu_baseline or not args.full
    return args


def spawn_ranks(args):
    """`python bench.py --gpus N` outside torchrun: launch the N ranks ourselves (one process per GPU, `torch.distributed.run`
    on 127.0.0.1) and hand the job over to them.  Fails loudly when the node has fewer than N devices."""
    import socket
    import subprocess
    if not args.emu and args.dist_backend == "nccl":
        import torch
        have = torch.cuda.device_count()
        if have < args.gpus:
            sys.exit(f"bench.py --gpus {args.gpus}: only {have} GPU(s) visible (one rank per GPU; no oversubscription)")
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # the host driver only supports dmabuf IPC (RCCL needs it)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.run(cmd, env=env).returncode)


def host_cpus():
    """CPUs this process may actually use: min(affinity, cgroup v2 quota)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except Exception:
        pass
    return n


class Dist:
    """world / rank / exchange of partial commitments (RCCL all-gather of raw bytes + host sum)."""

    def __init__(self, args):
        import torch
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.emu = args.emu
        if self.emu:
            self.dev = torch.device("cpu")
        else:
            local_rank = int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count()
            torch.cuda.set_device(local_rank)
            self.dev = torch.device("cuda", local_rank)
        self.dist = None
        if self.world > 1:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if args.dist_backend == "nccl":
                dist.init_process_group(backend="nccl", device_id=self.dev)
            else:
                dist.init_process_group(backend=args.dist_backend)
            self.dist = dist
        # --single-process: one rank whatever --gpus says; the keys are multi-device keys with `multi` shards
        self.multi = args.gpus if getattr(args, "single_process", False) and args.gpus > 1 else 0
        assert self.world == (1 if self.multi else args.gpus), f"--gpus {args.gpus} but WORLD_SIZE={self.world}"

    def combine(self, curve, partial):
        if self.world == 1:
            return partial
        from sirius_amd.distributed import all_gather_commitments
        return all_gather_commitments(curve, partial, device=self.dev if self.dist.get_backend() == "nccl" else None)

    def sum_field(self, field, partial):
        if self.world == 1:
            return partial
        from sirius_amd.distributed import all_gather_field_sum
        return all_gather_field_sum(field, partial, device=self.dev if self.dist.get_backend() == "nccl" else None)

    def barrier(self):
        import torch
        if self.world > 1:
            self.dist.barrier()
        if not self.emu:
            torch.cuda.synchronize()

    def max_over_ranks(self, dt):
        import torch
        if self.world == 1:
            return dt
        red = self.dev if self.dist.get_backend() == "nccl" else "cpu"
        tt = torch.tensor([dt], dtype=torch.float64, device=red)
        self.dist.all_reduce(tt, op=self.dist.ReduceOp.MAX)
        return float(tt.item())


class ThreadGroup:
    """what N threads of one process share: a barrier and one slot per rank for the exchanges"""

    def __init__(self, world):
        import threading
        self.world, self.barrier = world, threading.Barrier(world)
        self.slots = [None] * world


class DistThreads:
    """Dist for `--gpus N --threads`: rank = host thread, bound to device rank % count; exchanges go through ThreadGroup's slots (two
    barriers per exchange: all written, all read), the sums through the library's host entries as in sirius_amd.distributed."""

    def __init__(self, args, rank, group):
        import torch
        import sirius_amd as S
        self.world, self.rank, self.group, self.emu, self.multi, self.dist = group.world, rank, group, args.emu, 0, None
        if self.emu:
            self.dev = torch.device("cpu")
        else:
            d = rank % group.n_devices
            torch.cuda.set_device(d)
            self.dev = torch.device("cuda", d)
            S.init_thread(d)

    def _all(self, x):
        g = self.group
        g.slots[self.rank] = x
        g.barrier.wait()
        out = list(g.slots)
        g.barrier.wait()
        return out

    def combine(self, curve, partial):
        import sirius_amd as S
        parts = np.stack([np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 8) for p in self._all(partial)])     # (world, m, 8)
        res = np.stack([S.point_sum(curve, parts[:, j, :]) for j in range(parts.shape[1])])
        return res if np.ndim(partial) == 2 else res[0]

    def sum_field(self, field, partial):
        from sirius_amd.field import ints_to_mont
        from sirius_amd.protogalaxy import fold_witness
        parts = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4) for p in self._all(partial)]
        return fold_witness(field, parts, ints_to_mont(field, [1] * self.world)).reshape(np.shape(partial))

    def barrier(self):
        import torch
        if not self.emu:
            torch.cuda.synchronize()
        self.group.barrier.wait()

    def max_over_ranks(self, dt):
        return max(self._all(dt))


def make_key(S, D, curve, n, seed):
    """the commitment key of one circuit: sharded over the ranks (process per GPU), a multi-device key (--single-process), or plain"""
    if getattr(D, "multi", 0):
        return S.CommitmentKey.setup_synthetic_multi(curve, n, seed=seed, n_devices=D.multi)
    return S.CommitmentKey.setup_synthetic(curve, n, seed=seed, rank=D.rank, world=D.world)


def up(D, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(D.dev)


def pinned_copy(S, a):
    hb = S.HostBuffer(a.shape[0])
    hb.array[:] = a
    return hb


# ------------------------------------------------------------------------------------------ Sangria side (configs[1], support circuit)
class SangriaSide:
    """One Sangria-folded circuit: structure + key + running accumulator (W, E) in HBM + the incoming witness on the HOST."""

    def __init__(self, S, D, w, log_key, tag):
        self.w, self.tag = w, tag
        self.field, self.curve, self.rows = w["field"], w["curve"], w["rows"]
        self.S = S.PlonkStructure(self.field, w["k"], w.get("selectors", []), w["fixed"], w["num_advice"], w["gates"])
        if D.world > 1:
            self.S.set_shard(D.rank, D.world)
        assert w["num_advice"] * self.rows <= (1 << log_key)
        self.ck = make_key(S, D, self.curve, 1 << log_key, 42 + self.curve)
        self.accW, self.accE = up(D, w["W1"]), up(D, w["E"])
        self.host_W = pinned_copy(S, w["W2"])                    # the incoming witness as the CPU synthesis leaves it
        self.inW = up(D, w["W2"])                                # its device copy (rewritten by every witness commit)
        self.u1c, self.u1u, self.u2c, self.r = w["u1_challenges"], w["u1_u"], w["u2_challenges"], w["r"]
        self.d = self.S.num_cross_terms
        from sirius_amd.field import MODULUS, from_mont, ints_to_mont
        self.sf = 0 if self.curve == 0 else 1
        rv = from_mont(self.sf, self.r)
        self.rpows = ints_to_mont(self.sf, [pow(rv, i + 1, MODULUS[self.sf]) for i in range(self.d)])
        self.accCW = np.zeros(8, dtype=np.uint64)
        self.accCE = np.zeros(8, dtype=np.uint64)
        self.inC = np.zeros(8, dtype=np.uint64)
        self.pending = None
        self.ro = S.PoseidonHash(1 if self.curve == 0 else 0, 5, 4, 10, 10)
        self.nz_terms = 0

    def settle(self):
        if self.pending is not None:
            self.accCE, self.accCW = self.pending[0].wait(), self.pending[1].wait()
            self.pending = None

    def witness_commit(self, S, D, from_host):
        """run_sps_protocol_0: ck.commit(W1) (src/plonk/mod.rs:441-447).  from_host: the witness comes up from host memory
        inside this call (chunked, overlapped with the MSM); otherwise it is already resident."""
        if from_host:
            c = self.ck.commit_upload(self.host_W.array, dev_copy=self.inW)
        else:
            c = self.ck.commit(self.inW)
        self.inC = D.combine(self.curve, c)

    def prove_incoming(self, S, ro_challenge=False, from_host=True):
        """The freshly synthesised trace (host; from_host=False: already resident) is uploaded, committed and folded by ONE library
        call: its commitment and the cross terms' come out of the same batched MSM (srs_sangria_prove_incoming; one process only)."""
        self.settle()
        ro = None
        if ro_challenge:
            ro = self.ro.reset()
            for pt in (self.accCW, self.accCE):
                ro.absorb_point(self.curve, pt)
        pr = S.sangria_prove(self.ck, self.S, self.u1c, self.u1u, self.accW, self.u2c, self.inW, self.accE, self.accCW, self.accCE,
                             r=None if ro_challenge else self.r, ro=ro, incoming=True, incoming_host=self.host_W.array if from_host else None)
        self.r, self.inC = pr["r"], pr["incoming_commitment"]
        self.pending = (pr["E_commitment"], pr["W_commitment"])
        self._keep = pr

    def prove(self, S, D, ro_challenge=False, count_nonzero=False):
        """VanillaFS::prove hot path (src/nifs/sangria/mod.rs:253-277)."""
        self.settle()
        if D.world == 1 and not count_nonzero:
            # one library call (srs_sangria_prove): cross terms + commitments, challenge, folds in place, instance fold on host workers
            ro = None
            if ro_challenge:      # generate_challenge (:162-179): the instances are absorbed here, the commitments inside the call
                ro = self.ro.reset()
                for pt in (self.accCW, self.accCE, self.inC):
                    ro.absorb_point(self.curve, pt)
            pr = S.sangria_prove(self.ck, self.S, self.u1c, self.u1u, self.accW, self.u2c, self.inW, self.accE,
                                 np.stack([self.accCW, self.inC]), self.accCE, r=None if ro_challenge else self.r, ro=ro)
            self.r = pr["r"]
            self.pending = (pr["E_commitment"], pr["W_commitment"])
            self._keep = pr
            return
        terms, commits = S.VanillaFS.commit_cross_terms(self.ck, self.S, self.u1c, self.u1u, self.accW, self.u2c, self.inW)
        if count_nonzero:
            self.nz_terms = sum(int((t != 0).any(dim=1).sum().item()) for t in terms)
        commits = D.combine(self.curve, commits)
        if ro_challenge:      # VanillaFS::generate_challenge (sangria/mod.rs:162-179)
            from sirius_amd.field import MODULUS, from_mont, ints_to_mont
            ro = self.ro.reset()
            for pt in (self.accCW, self.accCE, self.inC):
                ro.absorb_point(self.curve, pt)
            for pt in commits:
                ro.absorb_point(self.curve, pt)
            self.r = ro.squeeze(128, self.sf)
            from sirius_amd.field import powers
            self.rpows = powers(self.sf, self.r, self.d)
        acc = S.RelaxedPlonkWitness(self.field, [self.accW], self.accE).fold([self.inW], terms, self.r)
        self.accW, self.accE = acc.W[0], acc.E
        self.pending = (S.point_lincomb_async(self.curve, self.accCE, commits, self.rpows),
                        S.point_lincomb_async(self.curve, self.accCW, self.inC.reshape(1, 8), self.r.reshape(1, 4)))


def sangria_step(S, D, pri, sec, from_host, ro=False, count=False):
    """SangriaIVC::fold_step hot path (src/ivc/sangria/incrementally_verifiable_computation.rs:429-635)."""
    if not from_host and D.world == 1 and not count and not SPLIT_SUPPORT:
        # resident traces: a trace's commitment shares the batched MSM of the prove that folds it (the secondary's at the start of the
        # next step, where both are first needed).  Traces coming from the host keep the streamed commit: its upload overlaps the MSM.
        # Only a structure WITHOUT challenges may do that (the secondary: one gate): with challenges, U2's are squeezed after its
        # commitment has been absorbed (src/plonk/mod.rs:465-495), so the primary (two gates, one challenge) commits, then proves.
        for side, other in ((sec, pri), (pri, sec)):
            if side.S.num_challenges == 0:
                side.prove_incoming(S, ro, False)
            else:
                side.witness_commit(S, D, False)
                side.prove(S, D, ro, count)
        return
    sec.prove(S, D, ro, count)
    pri.witness_commit(S, D, from_host)
    pri.prove(S, D, ro, count)
    sec.witness_commit(S, D, from_host)


# ------------------------------------------------------------------------------------------ ProtoGalaxy side (configs[2])
class PgPrimary:
    """The primary (bn256) circuit of CyclefoldIVC: ProtoGalaxy accumulator in HBM, incoming trace in HBM (uploaded by the
    previous step's witness commit), the next witness on the host."""

    def __init__(self, S, D, k, log_key, compat):
        from sirius_amd import protogalaxy as PG
        from sirius_amd.field import FR, ints_to_mont
        from sirius_amd.workloads import make_structure_inputs, trace_like
        import random
        self.PG, self.compat = PG, compat
        w = make_structure_inputs("primary", k, seed=0x5349524955530000 + 3)
        self.w, self.k, self.rows = w, k, w["rows"]
        self.S = S.PlonkStructure(0, k, [], w["fixed"], w["num_advice"], w["gates"])
        # process-per-GPU: the leaves are sharded by the key's row stripes, so F / G / e come out as partial polynomials and the
        # witness upload is 1 / world each (reference_compat pins every leaf to row 0: that row goes up to every rank as a halo)
        self.sharded = D.world > 1 and k >= 10 and ((1 << k) >> 10) % D.world == 0        # row stripes == key stripes of every column
        self.D = D
        if self.sharded:
            self.S.set_shard(D.rank, D.world)
        self.ctx = PG.PolyContext(self.S, 1)
        n = w["num_advice"] * self.rows
        assert n <= (1 << log_key)
        self.ck = make_key(S, D, S.CURVE_BN256, 1 << log_key, 42)
        self.accW, self.inW = up(D, w["W1"]), up(D, w["W2"])
        # fold_witness deferred (DEFER_FOLD): nothing reads the folded witness before the next prove, so the 1.2 GB pass is queued on
        # a second stream when the next witness starts to come up (the device waits for PCIe there) -- into a SECOND incoming buffer
        self.inW_next = up(D, w["W2"]) if DEFER_FOLD and not self.sharded else None
        self.lag, self.side, self.fold_pending = None, None, False
        if self.inW_next is not None and self.inW.is_cuda:
            import torch
            self.side = torch.cuda.Stream()
        rng = np.random.default_rng(77)
        self.host_W = [pinned_copy(S, w["W2"]), pinned_copy(S, trace_like(rng, n))]      # two witnesses, alternating
        self.witness_kind = "bench"
        rnd = random.Random(3)
        self.m = lambda v: ints_to_mont(0, list(v))
        self.FR = FR
        self.betas_i = [rnd.randrange(FR) for _ in range(self.ctx.betas_count)]
        self.betas = self.m(self.betas_i)
        self.chal = [rnd.randrange(FR) for _ in range(3)]            # delta, alpha, gamma: seeded (the RO is host code)
        self.accC = np.zeros(8, dtype=np.uint64)
        self.inC = np.zeros(8, dtype=np.uint64)
        self.pending = None
        self.ro = S.PoseidonHash(0, 5, 4, 10, 10)
        self.step_no = 0
        self.last = {}                # the dict the last prove returned
        self.dev_W, self.seen_C = None, {}
        self.page_W = None            # secondary.pageable_witness: plain (pageable) copies of the two host witnesses

    def set_pageable(self, on):
        """secondary.pageable_witness: the step's new witness comes from ordinary pageable host memory (a Rust Vec<F>), not from a page-locked buffer"""
        self.page_W = [np.array(hb.array, copy=True) for hb in self.host_W] if on else None

    def set_resident(self, D, on):
        """secondary.device_resident: the two witnesses the steps alternate between are ALREADY in HBM when a step starts (the contract's
        "inputs resident" form; the headline uploads them inside the step) -- C becomes one MSM over the resident 12 * 2^k vector"""
        self.fold_done()
        self.dev_W = [up(D, hb.array) for hb in self.host_W] if on else None

    def set_witness(self, kind):
        """the two host witnesses the steps alternate between: `bench` (as built) or `survey` (SURVEY.md 8d(ii)'s mixture)"""
        from sirius_amd.workloads import survey_mixture, trace_like
        if kind == self.witness_kind:
            return
        n = self.w["num_advice"] * self.rows
        if kind == "survey":
            a = survey_mixture(np.random.default_rng(78), n, 0)
            self.host_W[0].array[:] = a
            self.host_W[1].array[:] = np.roll(a, 12345, axis=0)      # a second witness of the same mixture
        else:
            self.host_W[0].array[:] = self.w["W2"]
            self.host_W[1].array[:] = trace_like(np.random.default_rng(77), n)
        self.witness_kind = kind

    def settle(self):
        if self.pending is not None:
            self.accC = self.pending.wait()
            self.pending = None

    def prove(self, S, D, ro_challenge=False):
        """ProtoGalaxy::prove (src/nifs/protogalaxy/mod.rs:400-481)."""
        PG, ctx, m = self.PG, self.ctx, self.m
        self.settle()
        delta, alpha, gamma = self.chal
        ro = None
        if ro_challenge:      # Challenges::generate_one (mod.rs:80-133): the accumulator and the incoming instance are absorbed here
            ro = self.ro.reset()
            ro.absorb_field(np.concatenate([self.accC.reshape(2, 4), self.inC.reshape(2, 4)]))
            ro.absorb_field(self.betas)
            delta_m = ro.squeeze(255, 0)               # MAX_BITS (src/constants.rs:4), as Challenges::generate_one squeezes it
        else:
            delta_m = m([delta])[0]
        if self.sharded:
            return self.prove_sharded(S, D, ro, delta_m, alpha, gamma)
        # one library call (srs_pg_prove): F -> alpha -> betas' -> G -> K -> gamma -> L(gamma), e, fold_witness
        defer = self.inW_next is not None
        self.fold_done()
        pr = PG.prove(ctx, self.betas, delta_m, [self.accW, self.inW], ro=ro, alpha=None if ro else m([alpha])[0],
                      gamma=None if ro else m([gamma])[0], reference_compat=self.compat, fold=not defer)
        self.e, self.betas = pr["e"], pr["betas_stroke"]
        self.last = pr                                # (what --dump-outputs writes)
        if defer:
            self.lag = pr["lagrange"]
        else:
            self.accW = pr["W"]
        self.pending = S.point_lincomb_async(S.CURVE_BN256, None, np.stack([self.accC, self.inC]), pr["lagrange"][:2])   # fold_instance

    def fold_start(self):
        """the deferred fold_witness: accW <- L_0(gamma) accW + L_1(gamma) inW, on the side stream"""
        if self.lag is None:
            return
        import torch
        if self.side is not None:
            self.side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self.side):
                self.PG.fold_witness(0, [self.accW, self.inW], self.lag, out=self.accW)
        else:
            self.PG.fold_witness(0, [self.accW, self.inW], self.lag, out=self.accW)
        self.lag = None
        self.fold_pending = True

    def fold_done(self):
        """whatever reads accW next (the next prove, the digest) comes after the deferred fold"""
        self.fold_start()
        if self.fold_pending and self.side is not None:
            import torch
            torch.cuda.current_stream().wait_stream(self.side)
        self.fold_pending = False

    def prove_sharded(self, S, D, ro, delta_m, alpha, gamma):
        """The same prove with the leaves sharded over the ranks: every rank evaluates the tiles of ITS stripes, the partial
        polynomials (33 / 8 coefficients) are all-gathered and added; K, e and the transcript are replicated host work."""
        PG, ctx, m = self.PG, self.ctx, self.m
        pF = D.sum_field(0, PG.compute_F(ctx, self.betas, delta_m, self.accW, reference_compat=self.compat))
        if ro:
            ro.absorb_field(pF)
        alpha_m = ro.squeeze(255, 0) if ro else m([alpha])[0]
        bs = PG.beta_stroke(self.betas, alpha_m, delta_m)
        pG = D.sum_field(0, PG.compute_G(ctx, bs, [self.accW, self.inW], reference_compat=self.compat))
        pK = PG.compute_K_from_G(ctx, pG, PG.poly_eval(pF, alpha_m))
        if ro:
            ro.absorb_field(pK)
        gamma_m = ro.squeeze(255, 0) if ro else m([gamma])[0]
        self.e = PG.calculate_e(pF, pK, gamma_m, alpha_m, ctx.lagrange_domain)
        lag = PG.eval_lagrange_poly_for_cyclic_group(gamma_m, ctx.lagrange_domain)
        # in place: the rank's stripes and the rows its kernels read beyond them (rotation halo; row 0 of every column with the
        # reference's row-0 leaves) -- srs_structure_fold_sharded
        PG.fold_witness(0, [self.accW, self.inW], lag, out=self.accW, structure=self.S, reference_compat=self.compat)
        self.betas = bs
        self.last = dict(alpha=alpha_m, gamma=gamma_m, poly_F=pF, poly_K=pK, lagrange=lag)
        self.pending = S.point_lincomb_async(S.CURVE_BN256, None, np.stack([self.accC, self.inC]), lag[:2])       # fold_instance

    def witness_commit(self, S, D):
        """generate_plonk_trace -> run_sps_protocol_1: ck.commit(W1) of the NEW witness, host -> HBM inside the call."""
        hb = self.host_W[self.step_no & 1]
        if self.page_W is not None:
            hb = _Plain(self.page_W[self.step_no & 1])
        if self.dev_W is not None:                    # resident form: nothing crosses PCIe; the deferred fold of the previous incoming trace
            w = self.dev_W[self.step_no & 1]          # (another buffer) runs on the side stream under this MSM
            self.fold_start()
            self.inC = D.combine(S.CURVE_BN256, self.ck.commit(w))
            want = self.seen_C.get((self.witness_kind, self.step_no & 1))
            assert want is None or np.array_equal(self.inC, want), "resident commit != streamed commit of the same witness"
            self.inW = w
            self.step_no += 1
            return
        self.step_no += 1
        if D.world > 1 and not self.sharded:          # stripes of the columns are not key stripes: the whole vector goes up
            import torch
            self.fold_done()                          # (a deferred fold still reads the old incoming trace)
            self.inW.copy_(torch.from_numpy(hb.array.view(np.int64)))
            self.inC = D.combine(S.CURVE_BN256, self.ck.commit(self.inW))
            return
        if self.inW_next is not None:                 # the fold of the PREVIOUS incoming trace runs under this upload, which lands in the other buffer
            self.fold_start()
            self.inC = D.combine(S.CURVE_BN256, self.ck.commit_upload(hb.array, dev_copy=self.inW_next))
            self.inW, self.inW_next = self.inW_next, self.inW
            self.seen_C[(self.witness_kind, (self.step_no - 1) & 1)] = self.inC
            return
        self.inC = D.combine(S.CURVE_BN256, self.ck.commit_upload(hb.array, dev_copy=self.inW))
        if self.sharded:                              # rows the rank's leaf tiles read beyond its stripes (row 0 under reference_compat)
            self.S.upload_shard_halo(hb.array, self.inW, self.compat)


class _Plain:
    """a pageable numpy array behind the `.array` attribute the witness code reads"""
    def __init__(self, a):
        self.array = a


def PGint(fe):
    from sirius_amd.field import from_mont
    return from_mont(0, fe)


DEFER_FOLD = os.environ.get("SRS_BENCH_DEFER_FOLD", "1") == "1"             # A/B: the primary's fold_witness under the next witness upload
SPLIT_SUPPORT = os.environ.get("SRS_BENCH_SPLIT_SUPPORT", "0") == "1"      # A/B: the support trace committed, then folded (two MSM chains)


def cyclefold_step(S, D, pri, sup, ro=False, count=False, resident=False):
    """CyclefoldIVC::next hot path (src/ivc/cyclefold/incrementally_verifiable_computation/mod.rs:210-335).  resident: the support trace and
    (PgPrimary.set_resident) the new primary witness are in HBM already -- secondary.device_resident; the headline brings both up inside the step"""
    pri.prove(S, D, ro)                       # A
    if D.world == 1 and not count and not SPLIT_SUPPORT:
        sup.prove_incoming(S, ro, not resident)   # B: support-circuit trace committed + folded, one batched MSM (srs_sangria_prove_incoming)
    else:
        sup.witness_commit(S, D, True)        # B: support-circuit trace ...
        sup.prove(S, D, ro, count)            #    ... folded into the support accumulator
    pri.witness_commit(S, D)                  # C


def build_cyclefold(S, D, k, log_key, compat, ks=15):
    """The state of a CycleFold chain before its first step: primary ProtoGalaxy accumulator + incoming trace (committed), the
    support circuit's Sangria accumulator + incoming trace (committed).  Shared by main() and tests/chain_cases.py."""
    from sirius_amd.workloads import make_support_inputs
    pri = PgPrimary(S, D, k, log_key, compat)
    sup = SangriaSide(S, D, make_support_inputs(ks, seed=0x5349524955530000 + 4), ks + 2, "support")
    sup.witness_commit(S, D, False)
    pri.inC = D.combine(S.CURVE_BN256, pri.ck.commit(pri.inW))
    return pri, sup, ks


def sangria_chain_digest(pri, sec):
    """What a Sangria chain has folded so far: both circuits' folded instance commitments, last witness commitments and challenges --
    what tests/chain_cases.py::oracle_chain_sangria recomputes on the CPU oracle."""
    import hashlib
    pri.settle(); sec.settle()
    return hashlib.sha256(b"".join(np.ascontiguousarray(x, dtype=np.uint64).tobytes() for sd in (pri, sec) for x in
                                   (sd.accCW, sd.accCE, sd.inC, sd.r))).hexdigest()


def chain_digest(pri, sup):
    """What the chain has folded so far (the primary's e and instance commitments, the support accumulator's commitments): the
    same for every --gpus N, and -- with the reference's leaf rows and oracle-derived challenges -- what tests/chain_cases.py
    recomputes on the CPU oracle."""
    import hashlib
    pri.settle(); sup.settle()
    return hashlib.sha256(b"".join(np.ascontiguousarray(x, dtype=np.uint64).tobytes() for x in
                                   (pri.e, pri.accC, pri.inC, sup.accCW, sup.accCE, sup.inC))).hexdigest()


# ------------------------------------------------------------------------------------------ measurement helpers
_GC_HOLD = {"depth": 0, "was": False}


def gc_hold():
    """Run the interpreter's cycle collector NOW and keep it off until the matching gc_release().  With torch loaded a generation-2 pass of
    CPython's collector takes ~35 ms, and where it lands is a matter of allocation counts: r06 found one inside the ten timed steps of
    `secondary.device_resident` in every default run (13.0 instead of 9.5 ms per step; profiles/r06_bench_gc_pause.txt).  Called BEFORE a
    leg's warm-up steps, not right before its timed region: 35 ms of idle device let the clocks fall, and the first three timed steps
    after it ran 1.3 / 0.4 / 0.3 ms slow (same record).  `timeit` of the standard library keeps the collector off too; the product is
    called from Rust and has none."""
    import gc
    if _GC_HOLD["depth"] == 0:
        _GC_HOLD["was"] = gc.isenabled()
        gc.collect()
        gc.disable()
    _GC_HOLD["depth"] += 1


def gc_release():
    import gc
    _GC_HOLD["depth"] -= 1
    if _GC_HOLD["depth"] == 0 and _GC_HOLD["was"]:
        gc.enable()


class quiet_gc:
    """a region without a pass of the collector (nested inside gc_hold() it changes nothing: the collection happened before the warm-up)"""

    def __enter__(self):
        gc_hold()

    def __exit__(self, *exc):
        gc_release()


def timed(D, fn, steps, after=None):
    with quiet_gc():
        D.barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        if after:
            after()
        D.barrier()
        dt = time.perf_counter() - t0
    return D.max_over_ranks(dt)


def msm_roofline(S, units_note, nz_madds=None, world=1, total_units=None, sample_every=1, gather_peak_g=40.0):
    """roofline object of the dominant kernel from the library's HIP-event timers (srs_profile_*).  With event sampling
    (srs_profile_sampling) the timers cover every n-th launch: total_units = the scalars of ALL launches, so that the mixed additions of
    the sampled launches are nz_madds x (sampled scalars / all scalars)."""
    acc0 = S.profile_get("msm_accum0") or dict(total_ms=0.0, launches=0, units=0)
    if not acc0["launches"]:
        return None
    sec = acc0["total_ms"] * 1e-3
    if nz_madds and total_units and sample_every > 1:
        nz_madds = nz_madds * acc0["units"] / total_units
    achieved = MSM_BYTES_PER_SCALAR * acc0["units"] / sec / 1e9
    traffic, src = None, None
    for name in ("r06_pmc_accum0.json", "r05_pmc_accum0.json", "r04_pmc_accum0.json", "r03_pmc_accum0.json", "r02_pmc_accum0.json", "r01_pmc_accum0.json"):
        try:   # HBM bytes per launch from the committed PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, corrected)
            pmc = json.load(open(os.path.join(ROOT, "profiles", name)))
            if world == 1:
                traffic = round(pmc["hbm_bytes_per_scalar"] * acc0["units"] / acc0["launches"])
                src = f"profiles/{name} (PMC bytes/scalar x scalars per launch)"
            break
        except Exception:
            continue
    roof = {"bound": "hbm", "kernel": "msm::k_accum0s / k_accum0 (bucket accumulation: the chunks of a streamed commit in slot mode / every other MSM)", "achieved": round(achieved, 3), "peak": HBM_PEAK_GBS,
            "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 6), "traffic": traffic, "traffic_source": src,
            "avg_launch_ms": round(acc0["total_ms"] / acc0["launches"], 4), "launches": acc0["launches"],
            "scalars_per_launch": round(acc0["units"] / acc0["launches"]), "units_note": units_note,
            "traffic_note": "PMC FETCH_SIZE x 2 (the guide's correction for wide streaming reads) + WRITE_SIZE; FETCH_SIZE counts requests x 64 B and a random 64-byte "
                            "gather is ONE request of 64 B (profiles/r05_ubench_gather.txt), so the gather share (~80 %) of this figure is counted twice: ~0.7 KB per scalar move",
            "binding": "alu", "event_sampling": f"1 launch in {sample_every}" if sample_every > 1 else "every launch",
            "note": "`bound` / `frac` are the mandated HBM figures; the roof that BINDS this kernel is integer-multiplier issue (256-bit modular "
                    "products: v_mad_u64_u32), see the `alu` object and DESIGN.md 2"}
    if nz_madds:
        rate = nz_madds / sec
        peak = MAD_ISSUE_PER_S / MADD_MULT_INSNS
        # the other candidate roof: every mixed addition gathers one 64-byte table entry.  tools/ubench_gather (profiles/r05_ubench_gather.txt): random
        # 64-byte gathers saturate at ~40 G/s while the pages touched stay within ~2 GiB (a chunk of a streamed commit), at 19.7 G/s over a 16 GiB table
        gp = gather_peak_g * 1e9
        roof["gather"] = {"unit": "G gathers/s", "achieved": round(rate / 1e9, 3), "peak": gather_peak_g, "frac": round(rate / gp, 4),
                          "peak_source": "tools/ubench_gather.hip, profiles/r05_ubench_gather.txt: measured random 64-byte gather rate for this table footprint "
                                         "(a gather moves 64 B, not 128: 128-byte entries saturate at half the rate)"}
        roof["alu"] = {"unit": "G mixed-add/s", "achieved": round(rate / 1e9, 3), "peak": round(peak / 1e9, 3),
                       "frac": round(rate / peak, 4),
                       "peak_source": "instruction issue: 31.2 T v_mad_u64_u32/s (profiles/r02_ubench29_gfx950.txt) / 1548 multiplier "
                                      "instructions per mixed addition (8 products x 171 + 2 squares x 135 - 90: one shared reduction)",
                       "clock": "power-managed: 2.20-2.25 GHz inside k_accum0s under the product's chunk schedule, 1.8-2.0 GHz when the launches "
                                "run back to back (advertised 2.4 GHz); per shader cycle the kernel is at the multiplier's issue rate "
                                "(profiles/r06_clock_under_load.txt)"}
    return roof


def nonzero_rows(t):
    return int((t != 0).any(dim=1).sum().item())


# ------------------------------------------------------------------------------------------ --dump-outputs
DUMP_ROWS = 1 << 16            # a longer vector is written as this many of its rows, drawn with a fixed seed
DUMP_LIMIT = 64 * 10 ** 6      # bytes of all arrays of one dump


def _words(x):
    """field elements / points as the library hands them out (Montgomery form, 64-bit little-endian limbs), every limb as its two 32-bit
    words in float64: exact, so that two builds compare bit for bit.  (..., L) limbs -> (..., 2 L) float64."""
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x).view(np.uint64).view(np.uint32).astype(np.float64)


def _rows(name, t, rows):
    """(n, 4) vector -> (its words, None) or, above `rows` rows, (the words of a seeded sample of `rows` rows, the sorted row indices)"""
    import zlib
    n = t.shape[0]
    if n <= rows:
        return _words(t), None
    idx = np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(n, rows, replace=False))
    if hasattr(t, "index_select"):
        import torch
        return _words(t.index_select(0, torch.from_numpy(idx).to(t.device))), idx
    return _words(np.asarray(t)[idx]), idx


def dump_outputs(path, scalars, vectors):
    """--dump-outputs: scalars (name -> small array) are written whole, vectors (name -> (n, 4) array or tensor) through _rows, a
    sample's row indices beside it as <name>_rows.npy.  The vectors share what the scalars leave of DUMP_LIMIT: at most DUMP_ROWS rows
    each, fewer when many vectors would not fit (the scalars are bounded by the protocol -- the largest, poly_K, has at most 2^16
    coefficients = 4 MiB of words).  The row count depends on the shapes alone, so the same arguments give the same dump.
    -> what the result line reports about the dump."""
    arrays = {name: _words(v) for name, v in scalars.items()}
    left = DUMP_LIMIT - sum(a.nbytes for a in arrays.values())
    per_row = 4 * 2 * 8 + 8                  # 4 limbs as 8 float64 words, + the row index of a sample
    rows = min(DUMP_ROWS, max(left, 0) // (per_row * max(len(vectors), 1)))
    for name, v in vectors.items():
        arrays[name], idx = _rows(name, v, rows)
        if idx is not None:
            arrays[name + "_rows"] = idx.astype(np.float64)
    total = sum(a.nbytes for a in arrays.values())
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return {"dir": path, "arrays": len(arrays), "bytes": int(total)}


def cyclefold_outputs(pri, sup, vectors):
    """what the last CycleFold step handed its caller: the primary's prove (e, betas', F, K, alpha, gamma, the Lagrange values), folded
    instance and new witness commitment, the support circuit's challenge and commitments; with `vectors` (one rank holds whole vectors)
    also the folded primary witness, the device copy of the uploaded witness, the support accumulator (W, E) and its cross terms"""
    pri.settle()
    sup.settle()
    pri.fold_done()
    sc = {"primary_e": pri.e, "primary_betas": pri.betas, "primary_acc_commitment": pri.accC, "primary_incoming_commitment": pri.inC,
          "support_acc_W_commitment": sup.accCW, "support_acc_E_commitment": sup.accCE, "support_incoming_commitment": sup.inC,
          "support_r": sup.r}
    sc.update({"primary_" + k: v for k, v in pri.last.items() if k in ("alpha", "gamma", "poly_F", "poly_K", "lagrange")})
    keep = getattr(sup, "_keep", None)
    if keep is not None:
        sc["support_cross_term_commitments"] = keep["commits"]
    vec = {}
    if vectors:
        vec = {"primary_acc_W": pri.accW, "primary_incoming_W": pri.inW, "support_acc_W": sup.accW, "support_acc_E": sup.accE}
        if keep is not None:
            vec.update({f"support_cross_term_{j}": t for j, t in enumerate(keep["terms"])})
    return sc, vec


def sangria_outputs(sides, vectors):
    """what the last Sangria fold step handed its caller, per circuit: challenge, folded W / E commitments, the incoming trace's commitment
    and the cross terms' commitments; with `vectors` also the folded accumulator (W, E)"""
    sc, vec = {}, {}
    for sd in sides:
        sd.settle()
        t = sd.tag
        sc.update({f"{t}_acc_W_commitment": sd.accCW, f"{t}_acc_E_commitment": sd.accCE, f"{t}_incoming_commitment": sd.inC, f"{t}_r": sd.r})
        keep = getattr(sd, "_keep", None)
        if keep is not None:
            sc[f"{t}_cross_term_commitments"] = keep["commits"]
        if vectors:
            vec.update({f"{t}_acc_W": sd.accW, f"{t}_acc_E": sd.accE})
    return sc, vec


# ------------------------------------------------------------------------------------------ CPU baselines (oracle/)
def cpu_baseline_sangria(args, pri, sec, k):
    import oracle as O
    from oracle import expr as OE
    quota = host_cpus()
    threads = args.cpu_threads or min(2 * quota, os.cpu_count() or 1)
    t_all = 0.0
    for side in (sec, pri):
        w = side.w
        bases = side.ck.bases()
        ch = np.concatenate([w["u1_challenges"].reshape(-1, 4), w["u1_u"].reshape(1, 4), w["u2_challenges"].reshape(-1, 4),
                             O.ints_to_mont(side.field, [1])])
        t0 = time.perf_counter()
        cg, T = OE.cross_terms_oracle(O, side.field, w["gates"], len(w.get("selectors", [])), w["num_fixed"], w["num_advice"],
                                      w.get("selectors", []), w["fixed"], w["W1"], w["W2"], ch, threads)
        for t in T:
            O.msm(side.curve, t, bases, threads)
        O.fold_w(side.field, w["W1"], w["W2"], w["r"], threads)
        O.fold_e(side.field, w["E"], T, w["r"], threads)
        O.msm(side.curve, w["W2"], bases, threads)
        t_all += time.perf_counter() - t0
    return dict(value=1.0 / t_all, unit="fold-steps/s", cores=threads, kind="port",
                sample=f"1 fold step, k={k} (same synthetic workload; oracle/ = C port of best_multiexp + GroupedPoly/GraphEvaluator "
                       f"interpreter, OpenMP {threads} threads; host grants {quota} CPUs of {os.cpu_count()} via cgroup cpu.max)")


def cpu_baseline_cyclefold(args, pri, sup, compat):
    """ONE CyclefoldIVC::next hot path on the CPU oracle: ProtoGalaxy F / G / K + fold_witness, the support-circuit Sangria
    prove + commits, the 12 * 2^k witness commit."""
    import oracle as O
    from oracle import expr as OE
    from oracle import protogalaxy as OPG
    quota = host_cpus()
    threads = args.cpu_threads or min(2 * quota, os.cpu_count() or 1)
    w = pri.w
    bases = pri.ck.bases()
    sbases = sup.ck.bases()
    oS = OPG.Structure(O, w["gates"], w["k"], [], w["fixed"], w["num_advice"], 0)     # GraphEvaluator per gate (plonk/mod.rs:697-701)
    octx = oS.context(1)
    betas = pri.betas_i[:octx.betas_count()]
    delta, alpha, gamma = pri.chal
    t0 = time.perf_counter()
    pF = OPG.compute_F_fast(oS, octx, betas, delta, w["W1"], [], compat, threads)
    bs = OPG.beta_stroke(betas, alpha, delta)
    pG = OPG.compute_G_fast(oS, octx, bs, [w["W1"], w["W2"]], [[], []], compat, threads)
    OPG.compute_K_from_G(octx, pG, OPG.poly_eval(pF, alpha))
    from oracle import pyref as P
    Lg = P.eval_lagrange_poly_for_cyclic_group(gamma, octx.lagrange_domain())
    O.lincomb(O.FR, [w["W1"], w["W2"]], O.ints_to_mont(O.FR, [int(l) for l in Lg[:2]]), threads)
    t_pg = time.perf_counter() - t0
    sw = sup.w
    ch = np.concatenate([sw["u1_u"].reshape(1, 4), O.ints_to_mont(sup.field, [1])])
    t1 = time.perf_counter()
    O.msm(sup.curve, sw["W2"], sbases, threads)
    cg, T = OE.cross_terms_oracle(O, sup.field, sw["gates"], 1, sw["num_fixed"], sw["num_advice"], sw["selectors"], sw["fixed"],
                                  sw["W1"], sw["W2"], ch, threads)
    for t in T:
        O.msm(sup.curve, t, sbases, threads)
    O.fold_w(sup.field, sw["W1"], sw["W2"], sw["r"], threads)
    O.fold_e(sup.field, sw["E"], T, sw["r"], threads)
    t_sup = time.perf_counter() - t1
    t2 = time.perf_counter()
    O.msm(0, w["W2"], bases, threads)
    t_msm = time.perf_counter() - t2
    t_all = t_pg + t_sup + t_msm
    return dict(value=1.0 / t_all, unit="fold-steps/s", cores=threads, kind="port",
                sample=f"1 CycleFold step, k={w['k']} (same synthetic workload: ProtoGalaxy F/G/K + fold {t_pg:.2f} s, support circuit "
                       f"{t_sup:.2f} s, {w['num_advice']}*2^{w['k']} witness commit {t_msm:.2f} s; oracle/ = C port of best_multiexp, the "
                       f"GraphEvaluator interpreter and the reference's reduction trees, OpenMP {threads} threads; host grants "
                       f"{quota} CPUs of {os.cpu_count()} via cgroup cpu.max)")


# ------------------------------------------------------------------------------------------ secondary objects
def extras_sangria(S, D, args, k=17, log_key=21, steps=20, warmup=3):
    """BASELINE configs[1]: one SangriaIVC::fold_step at k = 17, (a) with every operand resident in HBM (r01's line) and
    (b) with the two incoming witnesses coming up from host memory inside the step (what a shim on the Rust side pays)."""
    from sirius_amd.workloads import make_structure_inputs
    pri = SangriaSide(S, D, make_structure_inputs("primary", k, seed=0x5349524955530000 + 2), log_key, "primary")
    sec = SangriaSide(S, D, make_structure_inputs("secondary", k, seed=0x5349524955530000 + 3), log_key, "secondary")
    pri.witness_commit(S, D, False)
    sec.witness_commit(S, D, False)
    ro = args.ro_challenge
    sangria_step(S, D, pri, sec, False, ro, count=True)
    out = {"challenges": "poseidon-ro" if ro else "seeded"}
    legs = (("device_resident", False), ("host_witness", True)) if args.full else (("host_witness", True),)   # (host_witness: the headline of --config sangria)
    for name, from_host in legs:
        gc_hold()
        for _ in range(warmup):
            sangria_step(S, D, pri, sec, from_host, ro)
        S.profile_reset()
        dt = timed(D, lambda: sangria_step(S, D, pri, sec, from_host, ro), steps, after=lambda: (pri.settle(), sec.settle()))
        gc_release()
        out[name] = {"fold_steps_per_s": round(steps / dt, 3), "ms_per_step": round(dt / steps * 1e3, 4)}
        if not from_host:
            nz = sum(nonzero_rows(sd.inW) + sd.nz_terms for sd in (pri, sec))
            out["roofline"] = msm_roofline(S, "30 * 2^17 scalars per step over 2 batched launches (a trace and its cross terms each)", 16.0 * nz * steps / D.world, D.world)
            ct = S.profile_get("rowprog_cross_terms")
            out["cross_terms_ms_per_launch"] = round(ct["total_ms"] / ct["launches"], 4) if ct and ct["launches"] else None
    # 1 counting step + (warmup + steps) x the legs, all on the same two accumulators: the digest of that chain (with Poseidon-derived r it
    # equals tests/chain_cases.py::oracle_chain_sangria after the same number of steps; checked at k = 10 / 12 in tests/test_chain_gpu.py)
    out["state_digest"] = sangria_chain_digest(pri, sec)
    out["steps_folded"] = 1 + len(legs) * (warmup + steps)
    out["transcript"] = ("synthetic: r absorbs the accumulator's W / E commitments, the incoming W commitment and the cross-term commitments "
                         "(generate_challenge, src/nifs/sangria/mod.rs:162-179, without pp_digest / instances / u); the gate-compression "
                         "challenges and u of both instances are seeded constants")
    out["workload"] = f"sangria_poseidon fold_step hot path, k={k}, bn256/grumpkin, key 2^{log_key} (BASELINE configs[1])"
    out["host_path_ms_per_step"] = out["host_witness"]["ms_per_step"]
    cpu = None
    if D.world == 1 and not args.no_cpu_baseline and args.config == "sangria":
        cpu = cpu_baseline_sangria(args, pri, sec, k)
    return out, cpu, (pri, sec)


def extras_microbench(S, D, ck24, log_n=24, reps=3):
    """BASELINE configs[4]: 2^24-point MSM (bn256 G1) and 2^24-point NTT (Fr), device resident."""
    import torch
    from sirius_amd.workloads import rand_fe
    n = 1 << log_n
    rng = np.random.default_rng(5)
    out = {"workload": f"2^{log_n}-point MSM (bn256 G1) + 2^{log_n}-point NTT (Fr), device-resident (BASELINE configs[4])"}

    def timeit(fn):
        gc_hold()
        for _ in range(3):           # plan / table creation and the clock ramp stay outside (the first transforms of a process run ~10 % slower)
            fn()
        with quiet_gc():
            D.barrier()
            t = time.perf_counter()
            for _ in range(reps):
                fn()
            D.barrier()
            dt = (time.perf_counter() - t) / reps
        gc_release()
        return dt
    a = up(D, rand_fe(rng, n))
    S.fft.fft(a)
    pmc = None
    try:   # HBM bytes per transform of the kernels that ship, from the committed PMC passes (profiles/r05_pmc_ntt.json)
        pmc = json.load(open(os.path.join(ROOT, "profiles", "r05_pmc_ntt.json")))
    except Exception:
        pass
    for name, fn in (("fft", S.fft.fft), ("ifft", S.fft.ifft)):
        S.profile_reset()
        dt = timeit(lambda: fn(a))
        # modular products of one transform: (n / 2) log2 n butterflies + one inter-pass twiddle per element and non-final pass (3 passes
        # at 2^24); the chip issues 31.2 T v_mad_u64_u32/s and a 9 x 29-bit product takes 171 of them
        passes = 1 if log_n <= 10 else -(-log_n // 8)          # digits of <= 8 bits (csrc/ntt.hip)
        modmul = (n // 2) * log_n + (passes - 1) * n      # (ifft's 2^-k is folded into the first inter-pass table)
        alu_peak = MAD_ISSUE_PER_S / 171.0
        traffic = None
        if pmc and log_n == 24 and name in pmc.get("per_transform", {}):
            traffic = round(pmc["per_transform"][name]["hbm_bytes"])
        out[f"ntt_{name}"] = {"ms": round(dt * 1e3, 3), "elements_per_s": round(n / dt),
                              "roofline": {"bound": "hbm", "binding": "alu", "achieved": round(NTT_BYTES_PER_ELEMENT * n / dt / 1e9, 2), "peak": HBM_PEAK_GBS,
                                           "unit": "GB/s", "frac": round(NTT_BYTES_PER_ELEMENT * n / dt / 1e9 / HBM_PEAK_GBS, 5),
                                           "traffic": traffic, "traffic_source": "profiles/r05_pmc_ntt.json" if traffic else None, "passes": passes,
                                           "alu": {"unit": "G modmul/s", "achieved": round(modmul / dt / 1e9, 2), "peak": round(alu_peak / 1e9, 1),
                                                   "frac": round(modmul / dt / alu_peak, 4), "modmul_per_transform": modmul,
                                                   "peak_source": "31.2 T v_mad_u64_u32/s (profiles/r02_ubench29_gfx950.txt) / 171 multiplier instructions per 9 x 29-bit product"},
                                           "hbm_frac_ceiling": round(NTT_BYTES_PER_ELEMENT * n / (modmul / alu_peak) / 1e9 / HBM_PEAK_GBS, 4),
                                           "note": "whole transform, wall clock around the call.  `hbm_frac_ceiling` = the HBM fraction this transform would "
                                                   "show if its modular products ran at the multiplier's issue peak with everything else free: the north "
                                                   "star's >= 0.6 of HBM is not reachable for a 256-bit field on this chip (SURVEY.md H1), the binding roof is `alu`"}}
    del a
    if not D.emu:
        torch.cuda.empty_cache()
    for kind in ("uniform", "trace"):
        d = up(D, rand_fe(rng, n, zero_frac=0.55 if kind == "trace" else 0.0))
        S.profile_reset()
        dt = timeit(lambda: ck24.commit(d))
        roof = msm_roofline(S, f"2^{log_n} scalars per launch")
        out[f"msm_{kind}"] = {"ms": round(dt * 1e3, 3), "scalars_per_s": round(n / dt), "roofline": roof,
                              "whole_call_frac_of_hbm": round(MSM_BYTES_PER_SCALAR * n / dt / 1e9 / HBM_PEAK_GBS, 5)}
        del d
    return out


def extras_high_degree(S, D, args, k=22, degree=15, reps=5):
    """BASELINE configs[3] as named -- "ProtoGalaxy NIFS high-degree-gate fold, k=22": ProtoGalaxy::prove (one incoming trace) on the CycleFold
    primary shape with its first gate raised to `degree` (workloads.high_degree_gate: same 12 advice / 26 fixed columns).  16 evaluation
    points of G instead of 8, K on 2^16 points (quirk Q2), its 65536 coefficients absorbed by the transcript.  The prove only: the k = 22
    witness commit needs a 2^26 key and is timed by `bench.py --k 22 --log-key 26` (profiles/*_bench_cyclefold_k22_key26_*.json)."""
    import random
    from sirius_amd import _lib as _L
    from sirius_amd import protogalaxy as PG
    from sirius_amd.field import FR, ints_to_mont
    from sirius_amd.workloads import high_degree_gate, make_structure_inputs
    w = make_structure_inputs("primary", k, seed=0x5349524955530000 + 5)
    gates = [high_degree_gate(5, degree, 0, 0, 0, w["num_fixed"]), w["gates"][1]]
    t0 = time.perf_counter()
    St = S.PlonkStructure(0, k, [], w["fixed"], w["num_advice"], gates)
    t_create = time.perf_counter() - t0
    ctx = PG.PolyContext(St, 1)
    accW, inW = up(D, w["W1"]), up(D, w["W2"])
    rnd = random.Random(4)
    m = lambda v: ints_to_mont(0, list(v))
    betas, delta = m([rnd.randrange(FR) for _ in range(ctx.betas_count)]), m([rnd.randrange(FR)])[0]
    ro = S.PoseidonHash(0, 5, 4, 10, 10)
    compat = args.leaf_rows == "compat"

    def prove():
        ro.reset().absorb_field(delta.reshape(1, 4))
        return PG.prove(ctx, betas, delta, [accW, inW], ro=ro, reference_compat=compat, fold=True)
    gc_hold()
    prove()
    S.profile_reset()
    dt = timed(D, prove, reps)
    gc_release()
    prof = {}
    for name in ("pg_F_leaves", "pg_G_leaves"):
        st = S.profile_get(name)
        if st and st["launches"]:
            prof[name + "_ms"] = round(st["total_ms"] / st["launches"], 4)
    out = {"workload": f"ProtoGalaxy::prove, k={k}, 2 gates (degree {degree} + MainGate<3>), n = 2^{k + 1} leaves, F {ctx.fft_points_count_F} / G "
                       f"{ctx.fft_points_count_G} points, K 2^{ctx.fft_log_domain_size_K} points (BASELINE configs[3]: high-degree gate)",
           "prove_ms": round(dt / reps * 1e3, 3), "kernel_ms": prof, "structure_create_s": round(t_create, 3), "leaf_rows": args.leaf_rows,
           "leaf_kernels": "ahead-of-time sweep kernels" if _L.lib().srs_structure_kernel_kind(St._h, 2) == 1 else "interpreter (k_pg_leaves: no ahead-of-time kernel for this gate set)",
           "note": "prove = F, alpha, G, K, gamma, e, fold_witness in one call (srs_pg_prove); of it ~16 k Poseidon permutations on the host absorb "
                   "K's 2^16 coefficients (the reference's quirk Q2 sizes K's domain 2^16 for 16 points of G)"}
    St.close()
    del accW, inW
    return out


def extras_key_setup(S, D, ck24):
    """What a drop-in's `IVC::new` pays once: srs_ck_create of a 2^24-base key from host memory (upload + window expansion, with and without
    the second, 20-bit-window table) and the HBM it holds."""
    import torch
    bases = ck24.bases()
    n = bases.shape[0]
    out = {"bases": n, "host_bytes": int(bases.nbytes)}
    for name, wide in (("with_wide_table", 1), ("narrow_only", 0)):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        with S.tuning(msm_wide=wide):
            t0 = time.perf_counter()
            ck = S.CommitmentKey(S.CURVE_BN256, bases)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        held = free0 - torch.cuda.mem_get_info()[0]
        out[name] = {"create_s": round(dt, 3), "hbm_bytes": int(held), "has_wide_table": bool(ck.has_wide_table())}
        ck.close()
    out["note"] = ("srs_ck_create(2^24 bn256 bases from pageable host memory): 1 GiB upload + 15 (+ 13) windows of doublings and batched normalisations; "
                   "`narrow_only` = tuning msm_wide = 0 / environment SRS_MSM_WIDE=0 (whole MSMs of >= 2^23 scalars then stay on the 16-bit windows)")
    return out


def extras_msm_sharded(S, D, ck, log_n, reps=3):
    """BASELINE configs[4] on N ranks: the 2^log_n-point MSM over the SHARDED key -- every rank adds up its block-cyclic stripes of the
    same device-resident vector, the 64-byte partials are all-gathered and summed (inside the timed call).  scalars_per_s at
    N = 1, 2, 4, 8 is the MSM scaling curve of the north star."""
    from sirius_amd.workloads import rand_fe
    n = 1 << log_n
    rng = np.random.default_rng(5)                 # the same vector on every rank
    out = {"workload": f"2^{log_n}-point MSM (bn256 G1), key and work sharded over {D.world} ranks, device-resident"}
    for kind in ("uniform", "trace"):
        d = up(D, rand_fe(rng, n, zero_frac=0.55 if kind == "trace" else 0.0))
        fn = lambda: D.combine(S.CURVE_BN256, ck.commit(d))
        gc_hold()
        fn()
        with quiet_gc():
            D.barrier()
            t = time.perf_counter()
            for _ in range(reps):
                fn()
            D.barrier()
            dt = (time.perf_counter() - t) / reps
        gc_release()
        dt = D.max_over_ranks(dt)
        out[f"msm_{kind}"] = {"ms": round(dt * 1e3, 3), "scalars_per_s": round(n / dt), "n_gpus": D.world}
        del d
    return out


# ------------------------------------------------------------------------------------------ main
def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and not args.single_process and not args.threads:
        spawn_ranks(args)
    import torch
    if args.emu:
        from sirius_amd import _lib
        _lib.load(os.path.join(ROOT, "tests", "emu", "libsirius_emu.so"))
    else:
        assert torch.cuda.is_available(), "bench.py needs a GPU (there is no CPU path)"
    if args.threads and args.gpus > 1:
        import threading
        group, errs = ThreadGroup(args.gpus), []
        if not args.emu:
            torch.cuda.init()                    # (torch's lazy CUDA initialisation is not safe to enter from several threads at once)
            group.n_devices = torch.cuda.device_count()

        def body(rank):
            try:
                run(args, DistThreads(args, rank, group))
            except BaseException as e:           # a dead rank must not leave the others in a barrier
                errs.append((rank, repr(e)))
                group.barrier.abort()
                raise
        ts = [threading.Thread(target=body, args=(r,)) for r in range(args.gpus)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        if errs:
            sys.exit(f"bench.py --threads: {errs}")
        return
    run(args, Dist(args))


def run(args, D):
    import torch
    import sirius_amd as S

    out = None
    if args.config == "cyclefold":
        k = args.k or 20
        log_key = args.log_key or 24
        compat = args.leaf_rows == "compat"
        pri, sup, ks = build_cyclefold(S, D, k, log_key, compat, 15 if not args.emu else min(k, 5))
        pri.set_witness(args.witness)
        cyclefold_step(S, D, pri, sup, args.ro_challenge, count=True)           # untimed: also counts the non-zero cross-term rows
        verify = None
        if args.verify and D.rank == 0:
            # CHECKER (never timed, never on the product path): the same first step on the CPU oracle
            assert args.witness == "bench" and args.ro_challenge, "--verify: the oracle chain folds the bench witness with Poseidon-derived challenges"
            import oracle as O
            from oracle.chain import oracle_chain
            first = chain_digest(pri, sup)
            t0 = time.perf_counter()
            want = oracle_chain(O, S, k, log_key, ks, 1, compat, fast=True, threads=args.cpu_threads or min(2 * host_cpus(), os.cpu_count() or 1))
            verify = {"first_step_digest": first, "oracle_first_step_digest": want, "match": first == want,
                      "oracle_seconds": round(time.perf_counter() - t0, 2),
                      "note": "state_digest after ONE step of this chain vs oracle/chain.py::oracle_chain(steps=1); the timed steps continue the same chain"}
        resident = bool(args.resident) and D.world == 1 and not D.multi
        if resident:
            cyclefold_step(S, D, pri, sup, args.ro_challenge)      # (both witnesses have been committed from the host once: set_resident's check)
            pri.set_resident(D, True)
        gc_hold()                  # (the collector runs here, BEFORE the warm-up steps, and stays off through the timed ones)
        for _ in range(args.warmup):
            cyclefold_step(S, D, pri, sup, args.ro_challenge, resident=resident)
        S.profile_enable(args.full)          # (the roofline's HIP events: --full only)
        S.profile_sampling(PROF_SAMPLE)
        S.profile_reset()
        dt = timed(D, lambda: cyclefold_step(S, D, pri, sup, args.ro_challenge, resident=resident), args.steps, after=lambda: (pri.settle(), sup.settle()))
        gc_release()
        if resident:
            pri.set_resident(D, False)
        S.profile_enable(False)
        S.profile_sampling(1)
        scalars_per_step = pri.w["num_advice"] * pri.rows + (3 + 2) * sup.rows
        if D.rank == 0:
            dumped = None
            if args.dump_outputs:
                dumped = dump_outputs(args.dump_outputs, *cyclefold_outputs(pri, sup, D.world == 1))
            roof, prof = None, {}
            if args.full:
                nz = sum(nonzero_rows(torch.from_numpy(hb.array.view(np.int64))) for hb in pri.host_W) / 2.0 + nonzero_rows(sup.inW) + sup.nz_terms
                roof = msm_roofline(S, f"{pri.w['num_advice']}*2^{k} witness scalars in 10 chunks + the support circuit's 5*2^15 per step",
                                    16.0 * nz * args.steps / D.world if args.witness == "bench" else None, D.world,
                                    total_units=scalars_per_step * args.steps / D.world, sample_every=PROF_SAMPLE)
                for name in ("pg_F_leaves", "pg_G_leaves", "rowprog_cross_terms"):
                    st = S.profile_get(name)
                    if st and st["launches"]:
                        prof[name + "_ms"] = round(st["total_ms"] / st["launches"], 4)
            digest = chain_digest(pri, sup)
            out = {
                "metric": "IVC fold-steps/s (CycleFold IVC::next hot path, Poseidon-shaped synthetic trace, 2^k rows)",
                "value": round(args.steps / dt, 4), "unit": "fold-steps/s", "n_gpus": D.multi or D.world, "steps": args.steps,
                "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True,
                "scaling": "strong", "vs_baseline": None, "dtype": "u256 (modular; 9 x 29-bit / 8 x 32-bit limbs)",
                "data": "synthetic",
                "config": {"workload": f"cyclefold_poseidon IVC::next hot path, k={k}, bn256/grumpkin cycle, key 2^{log_key} (BASELINE configs[2])",
                           "primary": f"ProtoGalaxy prove: 12 advice / 26 fixed / 2 gates, n = 2^{k + 1} leaves, F 32 / G 8 / K 256 points; "
                                      f"12*2^{k} witness commit with the witness uploaded from host memory inside the step",
                           "support": f"Sangria prove on the support circuit: k={ks}, 3 advice / 4 fixed / 1 selector, 2 cross terms; 3*2^{ks} witness commit",
                           "leaf_rows": args.leaf_rows, "challenges": "poseidon-ro" if args.ro_challenge else "seeded",
                           "transcript": "synthetic content, the reference's order and widths: delta absorbs the 4 coordinates of the accumulator's and "
                                         "the incoming W commitments + the betas (Challenges::generate_one absorbs pp_digest, the accumulator and the "
                                         "instances as limbs, src/nifs/protogalaxy/mod.rs:80-101) and is squeezed with MAX_BITS = 255; alpha / gamma absorb "
                                         "poly_F / poly_K, 255 bits (:424-448); the support circuit's r as generate_challenge (sangria/mod.rs:162-179), 128 bits",
                           "witness": "55 % zero scalars, 45 % uniform 254-bit: 7.2 non-zero 16-bit digits (= bucket additions) per scalar, no hot buckets; "
                                      "SURVEY.md 8d(ii)'s mixture with bits and small values costs ~2.4 per scalar (tests/conftest.py seeded_scalars 'trace')",
                           "msm": "16 x 16-bit windows, streamed commit in 10 chunks, slot mode (per-bucket persistent partial sums, one reduction per commit)",
                           "parallelism": ((f"msm+leaf-shard{D.world}" if getattr(pri, "sharded", False) else f"msm-shard{D.world}") +
                                           ("-threads (one process, one host thread per device)" if isinstance(D, DistThreads) else "")) if D.world > 1
                                          else (f"msm-multi{D.multi}-single-process ({pri.ck.num_shards} shards on {torch.cuda.device_count() if not D.emu else 0} device(s))"
                                                if D.multi else "single-gpu")},
                "msm_scalars_per_s": round(scalars_per_step * args.steps / dt, 1),
                "witness_upload_bytes_per_step": int(pri.w["num_advice"] * pri.rows * 32 + 3 * sup.rows * 32),
                "state_digest": digest,
            }
            if args.full:
                out["roofline"], out["kernel_ms"] = roof, prof
            if dumped is not None:
                out["dump_outputs"] = dumped
            if verify is not None:
                out["verify"] = verify
            if resident:
                out["config"]["inputs"] = "--resident: witness and support trace in HBM before the step starts (NOT the headline: no upload inside the step)"
            if D.multi:      # in-library multi-device path: what every link carried (srs_ck_shard_stats; logical shards report the traffic of a real node)
                sts = [pri.ck.shard_stats(j) for j in range(pri.ck.num_shards)]
                commits = max(1, sts[0]["streamed_commits"])
                out["multi_device"] = {"shards": pri.ck.num_shards, "streamed_commits": commits,
                                       "h2d_bytes_per_commit": [x["h2d_bytes"] // commits for x in sts],
                                       "peer_bytes_per_commit": [x["peer_bytes"] // commits for x in sts], "devices": [x["device"] for x in sts],
                                       "note": "every shard uploads ITS stripes of the witness over its own link (1 / shards of 12 * 2^k * 32 B), overlapped with "
                                               "its MSM; the device copy for the next prove is assembled on device 0 by peer copies (xGMI)"}
            if args.witness != "bench":
                out["config"]["witness"] = ("SURVEY.md 8d(ii) mixture as canonical values: 55 % zero, 20 % bits, 15 % < 2^64, 10 % uniform (~2.3 bucket "
                                            "additions per scalar; bucket 0 of window 0 hot in every chunk)")
                out["msm_stats"] = pri.ck.msm_stats()
            if compat and D.world == 1 and not args.no_extras:
                # beside the headline: the same step with every leaf at ITS OWN row (what the reference's `index & 2^k` was meant
                # to be) -- more memory traffic in compute_F / compute_G, everything else identical
                pri.compat = False
                gc_hold()
                for _ in range(min(args.warmup, 2)):
                    cyclefold_step(S, D, pri, sup, args.ro_challenge)
                n_true = max(1, min(args.steps, 5))
                dt_true = timed(D, lambda: cyclefold_step(S, D, pri, sup, args.ro_challenge), n_true, after=lambda: (pri.settle(), sup.settle()))
                gc_release()
                pri.compat = True
                out["true_leaf_rows"] = {"fold_steps_per_s": round(n_true / dt_true, 4), "ms_per_step": round(dt_true / n_true * 1e3, 4),
                                         "steps": n_true, "note": "--leaf-rows true: leaf i evaluated at row i mod 2^k instead of row 0"}
            if D.world == 1 and not args.no_extras and args.witness == "bench" and not D.emu:
                # beside the headline: the same step on SURVEY.md 8d(ii)'s value mixture -- the regime real traces are assumed to live in
                # (0 / 1 / small values): a third of the bucket additions, and slot mode's hot-bucket path (overflow parts -> k_accum1
                # levels -> k_ovf_final) on EVERY set of every commit
                st0 = pri.ck.msm_stats()
                pri.set_witness("survey")
                gc_hold()
                for _ in range(3):                      # the first commit meets the hot buckets unexpectedly (one redo), then they are expected
                    cyclefold_step(S, D, pri, sup, args.ro_challenge)
                st1 = pri.ck.msm_stats()
                n_sv = max(1, min(args.steps, 5))
                S.profile_reset()
                dt_sv = timed(D, lambda: cyclefold_step(S, D, pri, sup, args.ro_challenge), n_sv, after=lambda: (pri.settle(), sup.settle()))
                gc_release()
                st2 = pri.ck.msm_stats()
                acc_sv = S.profile_get("msm_accum0") or dict(total_ms=0.0, launches=0)
                out["survey_mixture"] = {
                    "fold_steps_per_s": round(n_sv / dt_sv, 4), "ms_per_step": round(dt_sv / n_sv * 1e3, 4), "steps": n_sv,
                    "witness": "SURVEY.md 8d(ii): 55 % zero, 20 % bits, 15 % < 2^64, 10 % uniform, as canonical values (an ASSUMED mixture: no trace "
                               "histogram is published); ~2.3 bucket additions per scalar",
                    "msm_stats_warmup": {k2: st1[k2] - st0[k2] for k2 in st0}, "msm_stats_timed": {k2: st2[k2] - st1[k2] for k2 in st1},
                    "accum0_ms_per_step": round(acc_sv["total_ms"] / n_sv, 4),
                    "upload_floor_ms": round(pri.w["num_advice"] * pri.rows * 32 / 56e9 * 1e3, 3),
                    "note": "hot_sets == slot_sets in the timed steps: every chunk's bucket 0 overflows its 63 slots and goes through the overflow "
                            "kernels; redo == 0 once the key expects them.  Kernel times: profiles/r05_kernel_stats_survey_mixture.csv "
                            "(`bench.py --witness survey`)"}
                pri.set_witness("bench")
            if D.world == 1 and not D.multi and not args.no_extras and args.witness == "bench" and not resident:
                # beside the headline: the SAME step with its inputs already in HBM (the bench contract's "inputs resident" form): the new
                # witness is not uploaded but committed where it lies -- one 12 * 2^k MSM (20-bit windows from 2^23 scalars on) instead of the
                # streamed, PCIe-paced commit.  Same witnesses, same chain: every resident commitment is asserted equal to the streamed one.
                pri.set_resident(D, True)
                gc_hold()
                for _ in range(2):
                    cyclefold_step(S, D, pri, sup, args.ro_challenge, resident=True)
                n_rs = max(1, min(args.steps, 10))
                dt_rs = timed(D, lambda: cyclefold_step(S, D, pri, sup, args.ro_challenge, resident=True), n_rs, after=lambda: (pri.settle(), sup.settle()))
                gc_release()
                out["device_resident"] = {
                    "fold_steps_per_s": round(n_rs / dt_rs, 4), "ms_per_step": round(dt_rs / n_rs * 1e3, 4), "steps": n_rs,
                    "note": "the step with the new primary witness and the support trace already in HBM when it starts (no PCIe inside the timed "
                            "region); `value` above is the PCIe-inclusive step -- the reference's witness is synthesised on the host every step "
                            "(403 MB = 7.3 ms of upload at 56 GB/s, overlapped with the streamed commit)"}
                pri.set_resident(D, False)
            if D.world == 1 and not D.multi and not args.no_extras and args.witness == "bench" and not resident:
                # beside the headline: the same step fed from PAGEABLE host memory (a Rust Vec<F>; the headline alternates between two page-locked
                # buffers): the runtime stages pageable sources through its own pinned buffers
                pri.set_pageable(True)
                gc_hold()
                for _ in range(2):
                    cyclefold_step(S, D, pri, sup, args.ro_challenge)
                n_pg = max(1, min(args.steps, 10))
                dt_pg = timed(D, lambda: cyclefold_step(S, D, pri, sup, args.ro_challenge), n_pg, after=lambda: (pri.settle(), sup.settle()))
                gc_release()
                pri.set_pageable(False)
                out["pageable_witness"] = {"fold_steps_per_s": round(n_pg / dt_pg, 4), "ms_per_step": round(dt_pg / n_pg * 1e3, 4), "steps": n_pg,
                                           "note": "the new 12 * 2^k witness comes from plain pageable numpy memory (what a Rust Vec<F> is) instead of the "
                                                   "page-locked buffers of the headline; same chunked upload inside the step"}
            if D.world == 1 and not args.no_cpu_baseline:
                try:
                    out["cpu_baseline"] = cpu_baseline_cyclefold(args, pri, sup, compat)
                except Exception as e:   # the baseline is a reported number, never the product path
                    out["cpu_baseline"] = {"error": repr(e)}
        if not args.no_extras and D.world == 1:
            ck24 = pri.ck if log_key == 24 else None
            del pri.accW, pri.inW
            for hb in pri.host_W:
                hb.close()
            if not D.emu:
                torch.cuda.empty_cache()
            S.profile_enable(True)
            sec_obj, _, sides = extras_sangria(S, D, args) if not D.emu else extras_sangria(S, D, args, 4, 8, 1, 0)
            del sides
            if not D.emu:
                torch.cuda.empty_cache()
            micro = extras_microbench(S, D, ck24) if ck24 is not None else (extras_microbench(S, D, pri.ck, log_key, 1) if D.emu else None)
            S.profile_enable(False)
            if D.rank == 0:
                S.profile_enable(True)
                hd = extras_high_degree(S, D, args) if not D.emu else extras_high_degree(S, D, args, 4, 6, 1)
                S.profile_enable(False)
                setup = extras_key_setup(S, D, ck24) if ck24 is not None else None
                out["secondary"] = {"true_leaf_rows": out.pop("true_leaf_rows", None), "survey_mixture": out.pop("survey_mixture", None),
                                    "device_resident": out.pop("device_resident", None), "pageable_witness": out.pop("pageable_witness", None),
                                    "sangria_k17": sec_obj, "microbench_2p24": micro, "high_degree_k22": hd, "key_setup": setup,
                                    "predicted_scaling": PREDICTED_SCALING}
                out["host_path_ms_per_step"] = sec_obj["host_path_ms_per_step"]
                # LAST in the line (a reader that keeps only the tail of a long line still gets the figures of every configuration)
                mb = micro or {}
                out["summary"] = {
                    "cyclefold_k20_ms_per_step": out["ms_per_step"], "fold_steps_per_s": out["value"],
                    "resident_ms": (out["secondary"]["device_resident"] or {}).get("ms_per_step"),
                    "resident_fold_steps_per_s": (out["secondary"]["device_resident"] or {}).get("fold_steps_per_s"),      # inputs in HBM before the step (`value` is PCIe-inclusive: the conservative figure)
                    "pageable_ms": (out["secondary"]["pageable_witness"] or {}).get("ms_per_step"),
                    "survey_mixture_ms": (out["secondary"]["survey_mixture"] or {}).get("ms_per_step"),
                    "true_rows_ms": (out["secondary"]["true_leaf_rows"] or {}).get("ms_per_step"),
                    "sangria_k17_ms": [sec_obj["device_resident"]["ms_per_step"], sec_obj["host_witness"]["ms_per_step"]],
                    "msm_2p24_ms": [mb.get("msm_uniform", {}).get("ms"), mb.get("msm_trace", {}).get("ms")],
                    "ntt_2p24_ms": [mb.get("ntt_fft", {}).get("ms"), mb.get("ntt_ifft", {}).get("ms")],
                    "ntt_2p24_hbm_frac": [mb.get("ntt_fft", {}).get("roofline", {}).get("frac"), mb.get("ntt_ifft", {}).get("roofline", {}).get("frac")],
                    "high_degree_k22_prove_ms": (hd or {}).get("prove_ms"),
                    "accum_hbm_frac": (out["roofline"] or {}).get("frac"), "accum_alu_frac": ((out["roofline"] or {}).get("alu") or {}).get("frac"),
                    "cpu_fold_steps_per_s": (out.get("cpu_baseline") or {}).get("value")}
        if not args.no_extras and D.world > 1 and (log_key == 24 or D.emu):
            del pri.accW, pri.inW
            for hb in pri.host_W:
                hb.close()
            if not D.emu:
                torch.cuda.empty_cache()
            micro = extras_msm_sharded(S, D, pri.ck, log_key, 3 if not D.emu else 1)
            if D.rank == 0:
                out["secondary"] = {"microbench_msm_sharded": micro}
    else:
        k = args.k or 17
        log_key = args.log_key or 21
        S.profile_enable(args.full)
        obj, cpu, sides = extras_sangria(S, D, args, k, log_key, args.steps, args.warmup)
        S.profile_enable(False)
        if D.rank == 0:
            dumped = dump_outputs(args.dump_outputs, *sangria_outputs(sides, D.world == 1)) if args.dump_outputs else None
            main_leg = obj["host_witness"]
            out = {
                "metric": "IVC fold-steps/s (Sangria, Poseidon-shaped synthetic trace, 2^k rows)",
                "value": main_leg["fold_steps_per_s"], "unit": "fold-steps/s", "n_gpus": D.world, "steps": args.steps,
                "warmup": args.warmup, "ms_per_step": main_leg["ms_per_step"], "higher_is_better": True, "scaling": "strong",
                "vs_baseline": None, "dtype": "u256 (modular; 9 x 29-bit / 8 x 32-bit limbs)", "data": "synthetic",
                "config": {"workload": obj["workload"] + "; incoming witnesses uploaded from host memory inside the step",
                           "primary": "12 advice / 26 fixed / 2 gates / 6 cross terms", "secondary": "7 advice / 15 fixed / 1 gate / 5 cross terms",
                           "parallelism": f"msm-shard{D.world}" if D.world > 1 else "single-gpu"},
                "msm_scalars_per_s": round(30 * (1 << k) * main_leg["fold_steps_per_s"], 1),
            }
            if args.full:
                out.update({"device_resident_ms_per_step": obj["device_resident"]["ms_per_step"],
                            "roofline": obj["roofline"], "cross_terms_ms_per_launch": obj["cross_terms_ms_per_launch"]})
            if dumped is not None:
                out["dump_outputs"] = dumped
            if cpu is not None:
                out["cpu_baseline"] = cpu
    if D.rank == 0:
        print(json.dumps(out), flush=True)
    if D.world > 1 and D.dist is not None:
        D.dist.barrier()
        D.dist.destroy_process_group()


if __name__ == "__main__":
    main()
