#!/usr/bin/env python3
"""bench.py -- BASELINE.json headline metric on MI355X: MSM Mpoints/s, BLS12-381 G1, 2^20 points per GPU.

One step = one pass of the hot path (zkhip_msm_dev: scalars and bases resident in HBM, Jacobian result left in
HBM) over one batch of synthetic input.  N = 1: BASELINE configs[1].

N > 1 (`--gpus N`): one process per GPU.  Started under torch.distributed.run (WORLD_SIZE in the environment) this
process is one rank; started plainly, bench.py itself launches `python -m torch.distributed.run --nproc-per-node N`
on this file BEFORE touching the GPU and relays rank 0's line.  The job is ONE MSM of N x 2^20 points (weak scaling),
partitioned over the ranks in one of two ways (`--split`):
  points   rank g owns points [g 2^20, (g+1) 2^20) and runs the full single-GPU pipeline over them;
  windows  every rank holds ALL N x 2^20 points but only the window tables {w : w mod N == g} and sums those
           Pippenger windows (the bucket-window shard north_star names).
Either way the only exchange is one RCCL all-gather of the 144-byte Jacobian partial sums + an on-device fold.

A plain run sets up, warms up, times `--steps` steps and prints ONE JSON line (rank 0) with the contract fields
(`ms_per_step`: milliseconds per timed step).  `--dump-outputs DIR` writes the point the last timed step computed
(dump_outputs).

`--full` adds everything else: HIP events around the dominant kernel in the timed region, the other legs, and after
the timed region every leg CHECKS its output at full size ("verified" fields): the MSM against (sum s_i k_i) G
computed without Pippenger, the NTT at sampled indices against Horner evaluation, the Groth16 proof against the
trapdoor identity of a valid device-generated key, the KZG commitments / opening proof in the exponent.  Its line
adds `roofline`, `cpu_baseline` and one entry per leg; the sidecar file has every leg's full object.
"""
import argparse
import csv
import glob
import importlib.util
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
LOG_N = 20
ALG_BYTES_PER_POINT = 128  # BLS12-381 G1: 96 B affine base + 32 B scalar, each read once
HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: 8 TB/s spec
R_BLS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
R_BN = 21888242871839275222246405745257275088548364400416034343698204186575808495617
# per curve: scalar-field modulus, its multiplicative generator (arithmetic_params<F>::multiplicative_generator), two-adicity, and SURVEY 8d's
# algorithmic bytes per MSM point (affine base + 32-byte scalar, each read once) for G1 / G2
CURVE = {0: {"name": "BLS12-381", "r": R_BLS, "gen": 7, "s": 32, "bytes": {1: 128, 2: 224}},
         1: {"name": "BN254", "r": R_BN, "gen": 5, "s": 28, "bytes": {1: 96, 2: 160}}}
MASK64 = (1 << 64) - 1
LINE_LIMIT = 6144          # the driver keeps an 8 KiB tail of the output: the ONE line must fit with room to spare


def load_pkg():
    pkg_dir = os.path.join(ROOT, "crypto3-zk_amd")
    spec = importlib.util.spec_from_file_location("crypto3_zk_amd", os.path.join(pkg_dir, "__init__.py"),
                                                  submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["crypto3_zk_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def random_scalars(np, n, seed):
    """uniform in [0, r) by rejection from 255-bit draws; (n, 4) u64 canonical little-endian"""
    r_limbs = [0xffffffff00000001, 0x53bda402fffe5bfe, 0x3339d80809a1d805, 0x73eda753299d7d48]
    rng = np.random.default_rng(seed)
    out = np.empty((n, 4), dtype=np.uint64)
    todo = np.arange(n)
    while todo.size:
        v = rng.integers(0, 1 << 64, size=(todo.size, 4), dtype=np.uint64)
        v[:, 3] &= np.uint64((1 << 63) - 1)
        lt = np.zeros(todo.size, dtype=bool)
        eq = np.ones(todo.size, dtype=bool)
        for k in (3, 2, 1, 0):
            lt |= eq & (v[:, k] < np.uint64(r_limbs[k]))
            eq &= v[:, k] == np.uint64(r_limbs[k])
        out[todo[lt]] = v[lt]
        todo = todo[~lt]
    return out


def to_ints(a):
    """(n, 4) u64 canonical limbs -> list of python ints"""
    o = a.astype(object)
    return list(o[:, 0] + (o[:, 1] << 64) + (o[:, 2] << 128) + (o[:, 3] << 192))


def lim(np, v):
    return np.array([(v >> (64 * i)) & MASK64 for i in range(4)], dtype=np.uint64)


def launch_ranks(args, argv):
    """`python bench.py --gpus N` without a launcher: start the N rank processes ourselves.  Nothing in this process has
    touched the GPU (no HIP call, not even torch.cuda.is_available()), the ranks are fresh children."""
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + argv
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)    # ~0.15 s timed: the clocks need tens of milliseconds of load to settle
    ap.add_argument("--warmup", type=int, default=10)   # (10 / 2: 334, 50 / 10: 345, 200 / 20: 349 Mpoints/s on the same box)
    ap.add_argument("--log-n", type=int, default=LOG_N, help="points per GPU = 2^log_n (default: the BASELINE size)")
    ap.add_argument("--split", choices=("points", "windows"), default="points",
                    help="N > 1: partition of the N x 2^log_n-point MSM over the ranks (see the module docstring)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-groth16-log", type=int, default=20, help="constraints of the CPU prover sample = 2^k (default: the headline instance; 17 = quick)")
    ap.add_argument("--no-groth16", action="store_true", help="skip the Groth16 constraints/s leg")
    ap.add_argument("--force-dist", action="store_true", help="run the RCCL all-gather + fold at N = 1 too (checks the N > 1 path on one GPU)")
    ap.add_argument("--sync-exchange", action="store_true", help="N > 1: finish every step's all-gather + fold before the next multiexp is enqueued (A/B of the pipelined exchange)")
    ap.add_argument("--no-kzg", action="store_true", help="skip the KZG commit / opening-proof leg (BASELINE config 5's commitment layer, N = 1 only)")
    ap.add_argument("--no-ntt", action="store_true", help="skip the NTT leg (BASELINE config 3, N = 1 only)")
    ap.add_argument("--no-other-msm", action="store_true", help="skip the BLS12-381 G2 and BN254 G1 MSM legs (N = 1 only)")
    ap.add_argument("--no-two-in-flight", action="store_true", help="skip the two-MSMs-in-flight throughput figure (N = 1 only)")
    ap.add_argument("--no-pmc", action="store_true", help="do not collect roofline.traffic with rocprofv3 --pmc child passes")
    ap.add_argument("--no-verify", action="store_true", help="skip the post-timing full-size checks")
    ap.add_argument("--dist-backend", choices=("nccl", "gloo"), default="nccl",
                    help="nccl (= RCCL, the default) or gloo: the tiny exchanges staged through the host -- for the test that runs two REAL ranks on one GPU")
    ap.add_argument("--same-device", action="store_true", help="every rank uses GPU 0 (two ranks sharing the one GPU of a test box)")
    ap.add_argument("--log-constraints", type=int, default=20, help="constraints of the sharded Groth16 leg = 2^k (tests use a smaller instance)")
    ap.add_argument("--kzg-log-rows", type=int, default=20, help="rows of the sharded KZG leg's columns = 2^k")
    ap.add_argument("--ntt-log-m", type=int, default=22, help="domain of the sharded NTT leg = 2^k (tests use a smaller one)")
    ap.add_argument("--detail", default=None, help="where the sidecar with every leg's full object goes (default: bench_detail.json next to bench.py, "
                                                   "and a copy under gpurun_out/ when that directory exists)")
    ap.add_argument("--group-child", default=None, metavar="DEVICES",
                    help="internal: run the device-group legs over these devices (comma-separated) in THIS process and print their JSON -- bench.py "
                         "starts itself this way as a child, so that a group over GPUs no round could test on (RCCL single-process over xGMI) cannot take the line down")
    ap.add_argument("--child-legs", default="groth16,kzg", help="internal: which group legs the child runs")
    ap.add_argument("--dry-run", action="store_true",
                    help="no GPU: launch the ranks, run the all-gather + fold plumbing over gloo with stand-in partial sums, print the line's frame")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: HIP events around the dominant kernel, the post-timing checks (verified), the other legs, "
                         "the sharded and device-group legs, the live PMC passes, the CPU baseline and the sidecar (the --no-* options select among them); "
                         "without it a run sets up, warms up, times the steps and prints the headline line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed to DIR/<name>.npy (see dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(launch_ranks(args, sys.argv[1:]))
    if args.dry_run:
        return dry_run(args)
    if args.group_child is not None:
        return group_child(args)

    # stdout carries exactly ONE line, rank 0's JSON: libraries that print to the C stdout (librccl announces its path there,
    # flushed at exit, i.e. AFTER our line) are sent to stderr for the whole run; the line is written to the saved descriptor
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    import numpy as np
    import torch  # first: libzkhip.so must share torch's HIP runtime

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = 0 if args.same_device else int(os.environ.get("LOCAL_RANK", "0"))
    if world != max(1, args.gpus) and rank == 0:
        print("bench.py: --gpus %d but the launcher started %d rank(s); using the launcher's world size" % (args.gpus, world), file=sys.stderr)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: zkhip has no CPU fallback")
    torch.cuda.set_device(local_rank)
    dist = None
    use_dist = world > 1 or args.force_dist
    if use_dist:
        import torch.distributed as tdist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        if args.dist_backend == "nccl":
            tdist.init_process_group(backend="nccl", rank=rank, world_size=world,  # nccl == RCCL on ROCm
                                     device_id=torch.device("cuda", local_rank))
        else:
            tdist.init_process_group(backend="gloo", rank=rank, world_size=world)
        dist = Comm(torch, tdist, args.dist_backend, local_rank)

    zk = load_pkg()
    ctx = zk.Context(local_rank)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)

    n = 1 << args.log_n
    dev = f"cuda:{local_rank}"
    # synthetic input: bases P_i = k_i * G (device fixed-base kernel), scalars uniform in [0, r); block b of the job (the
    # 2^log_n points rank b owns under the point split) is seeded by b, so both splits run the same N x 2^log_n-point MSM
    windows = args.split == "windows" and world > 1
    blocks = list(range(world)) if windows else [rank]
    ks = np.concatenate([random_scalars(np, n, 1000 + b) for b in blocks])
    scalars = np.concatenate([random_scalars(np, n, 2000 + b) for b in blocks])
    if windows:
        ctx.set_option("msm_shard_world", world)
        ctx.set_option("msm_shard_rank", rank)
    bases = ctx.bases_from_scalars(zk.BLS12_381, zk.G1, ks)
    ctx.set_option("msm_shard_world", 1)
    n_local = len(scalars)
    d_scalars = torch.from_numpy(scalars.view(np.int64)).to(dev)
    d_outs = [torch.zeros(3 * 6, dtype=torch.int64, device=dev) for _ in range(2)]  # two: step i + 1 writes one while step i's exchange reads the other
    d_out = d_outs[0]
    d_total = torch.zeros(3 * 6, dtype=torch.int64, device=dev)

    from crypto3_zk_amd import dist as zd

    def fold(gathered, w):
        ctx.jacobian_sum_dev(zk.BLS12_381, zk.G1, gathered.data_ptr(), w, d_total.data_ptr())
        return d_total

    # N > 1: one all-gather of the 144-byte partial sums over RCCL per step, then the on-device fold -- the exchange of step i runs on RCCL's
    # stream UNDER the multiexp of step i + 1 (AllgatherFoldPipeline); every step's sum is produced, in order, inside the timed region
    pipe = zd.AllgatherFoldPipeline(world, lambda o, i: dist.all_gather_into_tensor(o, i, async_op=not args.sync_exchange), fold,
                                    lambda count: torch.zeros(count, dtype=torch.int64, device=dev)) if use_dist else None
    step_no = [0]

    def step():
        out = d_outs[step_no[0] & 1]
        step_no[0] += 1
        ctx.msm_dev(bases, d_scalars.data_ptr(), out.data_ptr(), 0, n_local)
        return pipe.push(out) if pipe else out

    def drain(last):
        """the last step's exchange and fold (the steps before it were finished one step late)"""
        return pipe.flush() if pipe else last

    def fence():
        if use_dist:
            dist.barrier(device_ids=[local_rank])
        torch.cuda.synchronize()

    result = None
    for _ in range(args.warmup):
        result = step()
    result = drain(result)
    fence()
    if args.full:
        # the timed region carries HIP events around the dominant kernel only (roofline.achieved); the full per-kernel breakdown
        # comes from three extra, untimed steps below
        ctx.profile_reset()
        ctx.profile_filter("msm_bucket_acc")
        ctx.profile(True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        result = step()
    result = drain(result)
    fence()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(np, zk, ctx, args.dump_outputs, result.cpu().numpy().view(np.uint64).reshape(3, 6))
    if not args.full:
        if use_dist:
            t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        if rank == 0:
            line = headline(args, world, n, windows, elapsed)
            line["verified"] = None  # the post-timing checks run under --full
            os.write(json_fd, (json.dumps(line, separators=(",", ":")) + "\n").encode())
        fence()
        bases.free()
        ctx.close()
        if use_dist:
            dist.destroy_process_group()
        return
    ctx.profile(False)
    dom_ms, dom_cnt = ctx.profile_get("msm_bucket_acc")
    ctx.profile_filter("")
    ctx.profile_reset()
    ctx.profile(True)
    for _ in range(3):
        step()
    drain(None)
    fence()
    ctx.profile(False)
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    prof = ctx.profile_dump()
    # ---- how much of a lone MSM's time is latency: the same steps with TWO MSMs in flight (a second context = a second stream with
    # its own copy of the bases).  Reported next to `value`, never instead of it: `value` is one MSM at a time, as the reference works.
    two_in_flight = None
    if world == 1 and not args.no_two_in_flight:
        ctx2 = zk.Context(local_rank)
        bases2 = ctx2.bases_from_scalars(zk.BLS12_381, zk.G1, ks)
        d_out2 = torch.zeros(3 * 6, dtype=torch.int64, device=dev)
        pair = ((ctx, bases, d_out), (ctx2, bases2, d_out2))
        for c, b, o in pair:
            c.msm_dev(b, d_scalars.data_ptr(), o.data_ptr(), 0, n_local)
        ctx.sync(), ctx2.sync()
        reps = max(2, args.steps // 2)
        t0 = time.perf_counter()
        for _ in range(reps):
            for c, b, o in pair:
                c.msm_dev(b, d_scalars.data_ptr(), o.data_ptr(), 0, n_local)
        ctx.sync(), ctx2.sync()
        dt2 = time.perf_counter() - t0
        two_in_flight = {"value": round(2 * reps * n / dt2 / 1e6, 4), "unit": "Mpoints/s", "ms_per_msm": round(dt2 / (2 * reps) * 1e3, 4),
                         "note": "two contexts (two streams), %d MSMs each, alternating launches: one MSM's reduction runs under the other's accumulation" % reps}
        bases2.free()
        ctx2.close()
    # ---- post-timing check of the timed output: sum_i s_i P_i with P_i = k_i G is (sum_i s_i k_i) G; the exponent is host
    # big-integer arithmetic, the single scalar multiplication the fixed-base kernel -- no bucket method involved.
    msm_verified = None
    if not args.no_verify:
        e = sum(a * b for a, b in zip(to_ints(ks), to_ints(scalars))) % R_BLS
        if use_dist and not windows:  # point split: the job's exponent is the sum over the ranks' blocks
            parts = [None] * world
            dist.all_gather_object(parts, e)
            e = sum(parts) % R_BLS
        if rank == 0:
            jac = result.cpu().numpy().view(np.uint64).reshape(3, 6)
            got, got_inf = ctx.jacobian_to_affine(zk.BLS12_381, zk.G1, jac)
            eb = ctx.bases_from_scalars(zk.BLS12_381, zk.G1, lim(np, e).reshape(1, 4))
            exp, exp_inf = eb.download()
            eb.free()
            msm_verified = bool(int(exp_inf[0]) == got_inf and (exp[0] == got).all())
    g16_sharded = None
    if use_dist and not args.no_groth16:
        # BASELINE config 4: ONE 2^20-constraint proof sharded over all ranks (every rank takes part in the exchange)
        g16_sharded = groth16_sharded_leg(np, torch, dist, rank, world, local_rank, log_constraints=args.log_constraints, verify=not args.no_verify)
    ntt_sharded = None
    if use_dist and not args.no_ntt:
        # BASELINE config 3: the 8 polynomials of 2^22 dealt over the ranks, no collective
        ntt_sharded = ntt_sharded_leg(np, torch, dist, zk, ctx, rank, world, local_rank, log_m=args.ntt_log_m, verify=not args.no_verify)
    kzg_sharded = None
    if use_dist and not args.no_kzg:
        # BASELINE config 5's commitment leg: the 50 columns dealt over the ranks, one all-gather of the commitments
        kzg_sharded = kzg_sharded_leg(np, torch, dist, zk, ctx, rank, world, local_rank, log_n=args.kzg_log_rows, verify=not args.no_verify)
    g16_group, group_out = None, {}
    if use_dist and world > 1 and not args.no_groth16:
        # the SAME sharded proof as ONE process sees it: rank 0 drives a device group over all `world` GPUs (the drop-in class's own
        # multi-GPU path, the exchange inside libzkhip.so) while the other ranks wait on the host; their GPUs are idle then
        torch.cuda.synchronize()
        devs = [0] * world if args.same_device else list(range(world))
        group_out = dist.host_wait_for_rank0(rank, lambda: run_group_child(devs, ["groth16"] + ([] if args.no_kzg else ["kzg", "lpc"]), args, timeout=420)) or {}
        g16_group = group_out.get("groth16_device_group")
    dist_info = None
    if use_dist:
        # evidence that the collective saw `world` DISTINCT devices: every rank reports the uuid of the GPU it runs on
        props = torch.cuda.get_device_properties(local_rank)
        mine = {"rank": rank, "local_rank": local_rank, "uuid": str(getattr(props, "uuid", "")) or None, "name": props.name}
        parts = [None] * world
        dist.all_gather_object(parts, mine)
        uu = [p_["uuid"] for p_ in parts]
        dist_info = {"backend": "rccl" if args.dist_backend == "nccl" else "gloo", "world_size": world, "devices": uu,
                     "distinct_devices": len(set(uu)), "same_device_flag": bool(args.same_device),
                     "exchange": "synchronous" if (args.sync_exchange or args.dist_backend != "nccl") else "pipelined: step i's all-gather + fold under step i+1's multiexp",
                     "note": "value: weak scaling (2^log_n points per GPU, one all-gather of 144 B per rank per step); the *_sharded legs are STRONG scaling of fixed jobs "
                             "and saturate at the replicated witness map + the small-MSM floor (DESIGN.md section 9; this line carries only what this run measured)"}
    if rank == 0:
        dom_avg_ms = dom_ms / max(1, dom_cnt)
        alg_bytes = ALG_BYTES_PER_POINT * n_local if not windows else ALG_BYTES_PER_POINT * n_local // world  # a rank's share of the job's bytes
        achieved = alg_bytes / (dom_avg_ms * 1e-3) / 1e9 if dom_avg_ms > 0 else 0.0
        full = headline(args, world, n, windows, elapsed)
        full.update({
            "verified": msm_verified,
            "verified_vs": ["(sum s_i k_i) G by the fixed-base kernel"] if msm_verified is not None else [],
            "timing": {"regime": "%d timed steps after %d warm-up steps (%.0f ms timed; the clocks settle over ~100 ms of load: 50/10 reads 3-4 %% above 20/5)"
                                 % (args.steps, args.warmup, elapsed * 1e3),
                       "hip_events_in_timed_region": "around msm_bucket_acc only (roofline.avg_launch_ms); every other figure comes from untimed extra steps"},
            "two_in_flight": two_in_flight,
            "roofline": {"bound": "hbm", "kernel": "msm_bucket_acc", "achieved": round(achieved, 3), "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 6), "traffic": None,
                         "avg_launch_ms": round(dom_avg_ms, 4), "algorithmic_bytes_per_launch": alg_bytes,
                         "honest_bound": "integer VALU issue (DESIGN.md section 4): the kernel moves 128 algorithmic bytes per ~4.9 k VALU instructions"},
            "kernel_ms_per_step": {k: round(v[0] / 3, 4) for k, v in sorted(prof.items())},
            "kernel_ms_per_step_source": "three extra untimed steps with HIP events around every launch (the timed region times msm_bucket_acc only)",
        })
        if dist_info is not None:
            full["dist"] = dist_info
        if world == 1:
            full["host_scalars"] = host_scalars_leg(np, zk, ctx, bases, scalars, result)
        traffic = None
        if world == 1 and not args.no_pmc:
            traffic = pmc_traffic_live(args.log_n)
        if traffic is not None:
            full["roofline"]["traffic"] = traffic["msm_bucket_acc"]
            full["roofline"]["traffic_source"] = "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE child passes of this run (2 x FETCH_SIZE + WRITE_SIZE, KiB -> B)"
            if traffic.get("valu", {}).get("msm_bucket_acc"):
                full["roofline"]["valu"] = dict(traffic["valu"]["msm_bucket_acc"], bound="VALU issue on 1024 SIMDs: issue_frac prices every wave instruction at 4 cycles; issue_frac_of_hw prices this kernel's mix (multiply-adds / VOP3 4 cycles, VOP2 2)",
                                                source="SQ_INSTS_VALU, GRBM_GUI_ACTIVE / 8 of a third child pass")
        else:
            full["roofline"]["traffic_source"] = ("not collected: bench.py itself runs under a profiler (no nested rocprofv3)" if under_profiler() else
                                                  "not collected in this run (rocprofv3 unavailable, --no-pmc, or N > 1); see profiles/ for the offline passes")
        group_child_out = None
        if world == 1 and not args.no_ntt:
            full["ntt"] = ntt_leg(np, zk, ctx, verify=not args.no_verify, traffic=traffic)
        if world == 1 and not args.no_groth16:
            valu = (traffic or {}).get("valu", {}).get("msm_bucket_acc")
            # BASELINE cfg 4's instance (M = 2^20, n = 10) over the domain the reference reduces over (step radix-2, 2^20 + 16 points),
            # the same instance over the basic domain of 2^21 points (round 2's figure), and the m = 2^20 variant (M = 2^20 - 11)
            full["groth16"] = groth16_leg(np, steps=8, verify=not args.no_verify, valu=valu, lanes=2)
            full["groth16_basic_2p21"] = groth16_leg(np, steps=6, verify=not args.no_verify, domain="basic", valu=valu)
            full["groth16_m2p20"] = groth16_leg(np, constraints=(1 << 20) - 11, steps=6, verify=not args.no_verify, valu=valu)
            # the other curve north_star names, same instance shape (BN254's make_evaluation_domain picks the step domain of 2^20 + 16 points too)
            full["groth16_bn254"] = groth16_leg(np, steps=5, verify=not args.no_verify, curve=1)
            # ... and the drop-in classes over a device group inside ONE process: every GPU this box has (at least two members, so that the
            # exchange runs; on a one-GPU box they share device 0 and the leg is labelled an emulation)
            have = max(1, torch.cuda.device_count())
            group_members = list(range(have)) if have > 1 else [0, 0]
            group_legs = ["groth16"] + ([] if args.no_kzg else ["kzg", "lpc"])
            group_child_out = run_group_child(group_members, group_legs, args)
            full["groth16_device_group"] = group_child_out.get("groth16_device_group")
        if world == 1 and not args.no_other_msm:
            full["msm_g2"] = msm_other_leg(np, zk, ctx, 0, 2, verify=not args.no_verify)
            full["msm_bn254_g1"] = msm_other_leg(np, zk, ctx, 1, 1, verify=not args.no_verify)
        if g16_sharded is not None:
            full["groth16_sharded"] = g16_sharded
        if g16_group is not None:
            full["groth16_device_group"] = g16_group
        if use_dist and world > 1 and not args.no_groth16 and group_out.get("kzg_device_group"):
            full["kzg_device_group"] = group_out["kzg_device_group"]
        if use_dist and world > 1 and not args.no_groth16 and group_out.get("lpc_device_group"):
            full["lpc_device_group"] = group_out["lpc_device_group"]
        if kzg_sharded is not None:
            full["kzg_sharded"] = kzg_sharded
        if ntt_sharded is not None:
            full["ntt_sharded"] = ntt_sharded
        if world == 1 and not args.no_kzg:
            full["kzg"] = kzg_leg(np, zk, ctx, verify=not args.no_verify, valu=(traffic or {}).get("valu", {}).get("msm_bucket_acc"))
            if group_child_out is not None and group_child_out.get("kzg_device_group"):
                full["kzg"]["device_group"] = group_child_out["kzg_device_group"]
            full["lpc"] = lpc_leg(np)
            if group_child_out is not None and group_child_out.get("lpc_device_group"):
                full["lpc_device_group"] = group_child_out["lpc_device_group"]
            full["quotient_chain"] = quotient_leg(np, verify=not args.no_verify)
            full["gate_argument"] = gate_argument_leg(np, verify=not args.no_verify)
            full["permutation_argument"] = permutation_leg(np, verify=not args.no_verify)
            full["lookup_argument"] = lookup_leg(np, verify=not args.no_verify)
            full["placeholder_round"] = placeholder_round_leg(np, verify=not args.no_verify)
        if world == 1 and not args.no_cpu_baseline:
            global CPU_GROTH16_LOG
            CPU_GROTH16_LOG = args.cpu_groth16_log
            jac = result.cpu().numpy().view(np.uint64).reshape(3, 6)
            gpu_affine = ctx.jacobian_to_affine(zk.BLS12_381, zk.G1, jac)
            others = {k: full[k] for k in ("msm_g2", "msm_bn254_g1") if isinstance(full.get(k), dict) and "_inputs" in full[k]}
            if not args.no_verify and isinstance(full.get("lpc"), dict) and "_fold" in full["lpc"]:
                others["lpc"] = full["lpc"]
            full["cpu_baseline"] = cpu_baseline(np, bases, scalars, gpu_affine, zk=zk, ctx=ctx, others=others if not args.no_verify else None)
            same = full["cpu_baseline"].pop("gpu_result_equals_oracle")
            if not args.no_verify:
                # the timed launch's output against the ORACLE's Pippenger over the same 2^log_n points and scalars (bit-exact, affine)
                full["verified"] = bool(full["verified"] and same)
                full["verified_vs"].append("oracle (cport) BDLO12 MSM of the same points and scalars, affine, bit-exact")
        for k in ("msm_g2", "msm_bn254_g1"):
            if isinstance(full.get(k), dict) and "_inputs" in full[k]:
                full[k].pop("_inputs")[0].free()
        if isinstance(full.get("lpc"), dict):
            full["lpc"].pop("_fold", None), full["lpc"].pop("_shape", None)
        detail = write_detail(full, args.detail)
        line = compact_line(full, detail)
        text = json.dumps(line, separators=(",", ":"))
        if len(text) > LINE_LIMIT:  # never hand the driver a line its parser cannot hold: drop the optional parts, the sidecar has them
            for k in ("legs_note", "two_in_flight", "host_scalars", "timing", "value_note"):
                line.pop(k, None)
            text = json.dumps(line, separators=(",", ":"))
        if len(text) > LINE_LIMIT:  # still too long: the legs shrink to value + verified, then go altogether
            line["legs"] = {k: _pick(v, "value", "verified", "error") for k, v in line.get("legs", {}).items()}
            text = json.dumps(line, separators=(",", ":"))
        if len(text) > LINE_LIMIT:
            line["legs"] = {"dropped": "see detail"}
            line.pop("dist", None)
            text = json.dumps(line, separators=(",", ":"))
        os.write(json_fd, (text + "\n").encode())
    fence()
    bases.free()
    ctx.close()
    if use_dist:
        dist.destroy_process_group()


def headline(args, world, n, windows, elapsed):
    """The contract fields of the line: the MSM of the timed steps, whatever else the run does."""
    return {
        "metric": "MSM Mpoints/sec, BLS12-381 G1 Pippenger, 2^%d points per GPU" % args.log_n,
        "value": round(world * n * args.steps / elapsed / 1e6, 4),
        "unit": "Mpoints/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u32",
        "dtype_note": "29-bit lazy limbs in u32 registers, 64-bit multiply-accumulate (381-bit Montgomery Fq, 255-bit Fr)",
        "data": "synthetic",
        "config": {"workload": "BLS12-381 G1 Pippenger MSM, ONE MSM of %d x 2^%d random points/scalars, bases resident" % (world, args.log_n),
                   "points_per_gpu": n,
                   "parallelism": ("window partition x%d (every rank: all points, 1/%d of the window tables)" % (world, world) if windows
                                   else "point-range partition x%d" % world) + " + one all-gather of the 144-B partial sums"},
    }


def dump_outputs(np, zk, ctx, path, jac):
    """--dump-outputs DIR: the point the last timed step computed (the job's MSM sum, Jacobian (3, 6) canonical u64 limbs), in affine
    form -- a Jacobian triple of a point is not unique, its affine coordinates are:
      msm_affine_xy.npy    (2, 24) float64: x and y as 16-bit little-endian words of their canonical 381-bit values (exact in float64)
      msm_is_infinity.npy  (1,) float64: 1.0 when the sum is the point at infinity (x, y then zero)
    The inputs come from fixed seeds, so runs with the same arguments compare output for output."""
    aff, inf = ctx.jacobian_to_affine(zk.BLS12_381, zk.G1, jac)
    words = np.ascontiguousarray(aff.reshape(2, 6), dtype="<u8").view("<u2").astype(np.float64)
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "msm_affine_xy.npy"), words)
    np.save(os.path.join(path, "msm_is_infinity.npy"), np.array([float(inf)], dtype=np.float64))


def write_detail(full, path=None):
    """Every leg's full object (per-kernel tables, per-run times, prose about what was measured and how it was checked) goes to a
    sidecar file; the line on stdout carries numbers only.  Returns the path relative to the repository."""
    paths = [path] if path else [os.path.join(ROOT, "bench_detail.json")]
    if not path and os.path.isdir(os.path.join(ROOT, "gpurun_out")):
        paths.append(os.path.join(ROOT, "gpurun_out", "bench_detail.json"))
    wrote = None
    for p in paths:
        try:
            with open(p, "w") as f:
                json.dump(full, f, indent=1)
            wrote = wrote or p
        except OSError:
            pass
    if wrote is None:
        return None
    return os.path.relpath(wrote, ROOT) if wrote.startswith(ROOT) else wrote


def _pick(d, *keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d and d[k] is not None}


def compact_line(full, detail_path):
    """The ONE line: the contract fields, `roofline`, `cpu_baseline`, and one number + `verified` per leg (<= LINE_LIMIT bytes)."""
    c = {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                              "dtype", "data", "config", "verified")}
    c["verified_vs"] = full.get("verified_vs")
    g = full.get("groth16") or full.get("groth16_sharded")
    if g and "value" in g:
        # BASELINE.json's metric names both halves: the Groth16 figure sits at top level too
        c["groth16_constraints_per_s"] = g["value"]
        c["groth16_verified"] = g.get("verified")
    r = full["roofline"]
    c["roofline"] = _pick(r, "bound", "kernel", "achieved", "peak", "unit", "frac", "avg_launch_ms", "algorithmic_bytes_per_launch")
    c["roofline"]["traffic"] = r.get("traffic")
    if r.get("valu"):
        c["roofline"]["valu"] = _pick(r["valu"], "issue_frac_of_hw", "issue_frac", "wave_insts_per_launch", "gpu_cycles_per_launch",
                                      "priced_cycles_per_wave_instruction")
    if full.get("timing"):
        c["timing"] = {"timed_ms": round(full["ms_per_step"] * full["steps"], 1), "hip_events_in_timed_region": "msm_bucket_acc only",
                       "note": "50/10 steps/warmup reads 3-4 % above 20/5 (clocks settle over ~100 ms)"}
    if full.get("host_scalars"):
        c["host_scalars"] = _pick(full["host_scalars"], "value", "unit", "ms_per_msm", "verified")
        c["value_note"] = "value: scalars resident (prover-internal MSMs); host_scalars: what a caller of algebra::multiexp sees (scalars H2D + result D2H per call)"
    if full.get("two_in_flight"):
        c["two_in_flight"] = _pick(full["two_in_flight"], "value", "ms_per_msm")
    if full.get("dist"):
        c["dist"] = full["dist"]
    legs = {}

    def leg(name, *extra):
        o = full.get(name)
        if not o:
            return
        if "error" in o:
            legs[name] = {"error": o["error"]}
            return
        e = _pick(o, "value", "unit", "verified", *extra)
        if isinstance(o.get("roofline"), dict) and "frac" in o["roofline"]:
            e["hbm_frac"] = o["roofline"]["frac"]
        legs[name] = e

    leg("ntt", "ms_per_transform_batch")
    leg("groth16", "ms_per_proof_mean", "domain_points")
    leg("groth16_basic_2p21", "ms_per_proof_mean")
    leg("groth16_m2p20", "ms_per_proof_mean")
    if (full.get("groth16") or {}).get("lanes_over_one_key"):
        legs["groth16"]["two_lanes_constraints_per_s"] = full["groth16"]["lanes_over_one_key"]["constraints_per_s"]
    leg("groth16_bn254", "ms_per_proof_mean", "domain_points")
    leg("groth16_device_group", "ms_per_proof_mean", "members", "distinct_gpus", "transport")
    leg("msm_g2", "ms_per_msm")
    leg("msm_bn254_g1", "ms_per_msm")
    leg("groth16_sharded", "ms_per_proof_mean", "scaling")
    leg("ntt_sharded", "scaling")
    leg("kzg_sharded", "scaling")
    leg("kzg", "ms_per_commit_mean", "opening_proof_ms_mean")
    if (full.get("kzg") or {}).get("scheme_class"):
        legs["kzg_scheme_class_from_host"] = _pick(full["kzg"]["scheme_class"], "value", "unit", "verified")
    kg = (full.get("kzg") or {}).get("device_group") or full.get("kzg_device_group")
    if kg:
        legs["kzg_device_group"] = _pick(kg, "value", "unit", "verified", "members", "distinct_gpus", "error")
    leg("lpc", "proof_eval_ms")
    leg("lpc_device_group", "members", "distinct_gpus", "leaf_owners")
    leg("quotient_chain")
    leg("gate_argument", "per_term_ms", "speedup_vs_per_term", "gate_eval_kernel_ms")
    leg("permutation_argument", "ms_grand_product")
    leg("lookup_argument", "ms_grand_product", "ms_sort_polynomials")
    leg("placeholder_round", "round_ms")
    c["legs"] = legs
    b = full.get("cpu_baseline")
    if b:
        cb = _pick(b, "value", "unit", "cores", "kind", "sample")
        if b.get("one_thread"):
            cb["one_thread"] = _pick(b["one_thread"], "value", "cores")
        if b.get("ntt"):
            cb["ntt"] = _pick(b["ntt"], "value", "unit", "cores")
        if b.get("groth16"):
            cb["groth16"] = _pick(b["groth16"], "value", "unit", "cores", "constraints", "seconds_per_proof")
        c["cpu_baseline"] = cb
    c["detail"] = detail_path
    return c


def host_scalars_leg(np, zk, ctx, bases, scalars, d_result, reps=10):
    """SURVEY 8d's timing protocol (ii): the call algebra::multiexp's callers actually make -- zkhip_msm: the scalars start in HOST
    memory (32 MiB H2D at 2^20 points), the Jacobian result comes back to the host (144 B D2H) -- over the same points and scalars as
    the headline.  Its result must equal the resident path's."""
    sc = np.ascontiguousarray(scalars)
    ctx.msm(bases, sc)
    ctx.msm(bases, sc)
    t0 = time.perf_counter()
    for _ in range(reps):
        jac = ctx.msm(bases, sc)
    dt = (time.perf_counter() - t0) / reps
    want = d_result.cpu().numpy().view(np.uint64).reshape(-1)
    a, b = ctx.jacobian_to_affine(zk.BLS12_381, zk.G1, np.asarray(jac).reshape(3, 6)), ctx.jacobian_to_affine(zk.BLS12_381, zk.G1, want.reshape(3, 6))
    return {"value": round(len(sc) / dt / 1e6, 3), "unit": "Mpoints/s", "ms_per_msm": round(dt * 1e3, 4), "verified": bool(a[1] == b[1] and (a[0] == b[0]).all()),
            "what": "zkhip_msm: H2D of the %d-byte scalar vector (pageable host memory) + the resident pipeline + D2H of the result, %d calls" % (sc.nbytes, reps)}


class Comm:
    """The collectives the legs use -- one all-gather of a few hundred bytes per step, a barrier, a max-reduction of the timings --
    over RCCL (backend "nccl": device tensors, ordered on torch's current stream, which the zkhip context runs on) or over gloo
    (tensors staged through the host).  gloo exists for the test-suite: RCCL cannot put two ranks on ONE GPU, and that is the only
    way a one-GPU box runs two real rank PROCESSES over the real kernels (tests/test_gpu_two_ranks.py)."""

    def __init__(self, torch, tdist, backend, local_rank):
        self.torch, self.d, self.backend, self.local_rank = torch, tdist, backend, local_rank
        self.ReduceOp = tdist.ReduceOp

    def all_gather_into_tensor(self, out, inp, async_op=False):
        """async_op: over RCCL the collective's handle (its .wait() orders the CURRENT stream after it, the host does not block); gloo is staged through
        the host and finished on return (None)"""
        if self.backend == "nccl":
            return self.d.all_gather_into_tensor(out, inp, async_op=async_op)
        host = self.torch.empty(out.shape, dtype=out.dtype)
        self.d.all_gather_into_tensor(host, inp.cpu())  # .cpu() waits for the stream the partial sums were computed on
        out.copy_(host)
        return None

    def all_reduce(self, t, op=None):
        if self.backend == "nccl":
            return self.d.all_reduce(t, op=op)
        host = t.cpu()
        self.d.all_reduce(host, op=op)
        t.copy_(host)

    def barrier(self, device_ids=None):
        if self.backend == "nccl":
            return self.d.barrier(device_ids=device_ids)
        self.torch.cuda.synchronize()
        self.d.barrier()

    def all_gather_object(self, parts, obj):
        return self.d.all_gather_object(parts, obj)

    def host_wait_for_rank0(self, rank, work=None):
        """Rank 0 runs `work` while every other rank waits ON THE HOST (a key of the rendezvous store) -- an RCCL barrier would park a
        spinning kernel on the other ranks' GPUs, and `work` (the device-group leg) uses exactly those GPUs.  Returns work()'s result on
        rank 0, None elsewhere."""
        store = None
        try:
            store = self.d.distributed_c10d._get_default_store()
        except Exception:
            pass
        out = None
        if rank == 0:
            try:
                out = work() if work else None
            finally:
                if store is not None:
                    store.set("zkhip_bench_rank0_work_done", "1")
        elif store is not None:
            import datetime
            store.wait(["zkhip_bench_rank0_work_done"], datetime.timedelta(seconds=900))  # rank 0's work is bounded well below this (run_group_child's timeout)
        if store is None:  # no store to wait on: the collective barrier after all (the leg then shares the GPUs with spinning kernels)
            self.barrier(device_ids=[self.local_rank])
        return out

    def destroy_process_group(self):
        return self.d.destroy_process_group()


def dry_run(args):
    """The launch + exchange plumbing without a GPU (CPU test of `--gpus N`): every rank contributes a stand-in partial sum,
    one all-gather over gloo, a fold; rank 0 prints the frame of the JSON line with the world size the launcher gave."""
    import torch
    import torch.distributed as dist

    load_pkg()
    from crypto3_zk_amd import dist as zd

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    part = torch.full((18,), rank + 1, dtype=torch.int64)
    total = zd.allgather_fold(part, world, lambda o, i: dist.all_gather_into_tensor(o, i), lambda g, w: g.view(w, 18).sum(0))
    ok = bool((total == sum(range(1, world + 1))).all())
    windows = [zd.shard_windows(16, r, world) for r in range(world)]
    parts = [{"rank": rank, "uuid": "dry-run-device-%d" % rank}]
    if world > 1:
        # the `dist` field of the real line (one device uuid per rank, all-gathered), with stand-in uuids
        parts = [None] * world
        dist.all_gather_object(parts, {"rank": rank, "uuid": "dry-run-device-%d" % rank})
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        # the frame of the real line (same builder, stand-in numbers), so that its size limit is checked without a GPU too
        frame = {"metric": "MSM Mpoints/sec, BLS12-381 G1 Pippenger, 2^%d points per GPU" % args.log_n, "value": 0.0, "unit": "Mpoints/s", "n_gpus": world,
                 "steps": args.steps, "warmup": args.warmup, "ms_per_step": 0.0, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u32",
                 "data": "synthetic", "config": {"workload": "dry run: launch + exchange plumbing only", "points_per_gpu": 1 << args.log_n, "parallelism": args.split},
                 "verified": None, "roofline": {"bound": "hbm", "kernel": "msm_bucket_acc", "achieved": 0.0, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": 0.0, "traffic": None}}
        frame["dist"] = {"backend": "gloo", "world_size": world, "devices": [p_["uuid"] for p_ in parts], "distinct_devices": len({p_["uuid"] for p_ in parts}),
                         "same_device_flag": False}
        line = compact_line(frame, None)
        line.update({"dry_run": True, "split": args.split, "exchange_ok": ok, "windows_per_rank": windows,
                     "point_ranges": [zd.shard_range(world << args.log_n, r, world) for r in range(world)]})
        text = json.dumps(line, separators=(",", ":"))
        assert len(text) <= LINE_LIMIT
        print(text, flush=True)
    return 0


def _profiler_var(name):
    return name in ("LD_PRELOAD", "ROCP_TOOL_LIBRARIES", "HSA_TOOLS_LIB") or name.startswith(("ROCPROF", "ROCP_", "ROCTRACER_", "ROCTX_"))


def under_profiler():
    """True when this process runs under rocprofv3 / rocprof (its tool library is preloaded into every child): the live PMC
    passes are skipped then -- the launcher of a nested rocprofv3 would initialise the GPU before exec'ing its target."""
    env = os.environ
    if any("rocprof" in env.get(k, "").lower() or "roctracer" in env.get(k, "").lower() for k in ("LD_PRELOAD", "HSA_TOOLS_LIB")):
        return True
    return any(k == "ROCP_TOOL_LIBRARIES" or k.startswith(("ROCPROFILER_", "ROCPROF_")) for k in env)


def pmc_traffic_live(log_n):
    """HBM bytes per launch of the dominant kernels -- and how busy their SIMDs are --, measured in THIS run: child passes of
    tools/pmc_child.py (the same MSM and NTT workloads) under `rocprofv3 --pmc`, FETCH_SIZE and WRITE_SIZE in passes of their
    own (they do not fit one pass: MI355X_MICROARCH.md), counters only.  gfx950 reports half the bytes of 16-B-per-lane reads:
    2 x FETCH_SIZE (KiB) + WRITE_SIZE (KiB).  A third pass reads SQ_INSTS_VALU and GRBM_GUI_ACTIVE: a 64-lane wave instruction
    occupies its 16-lane SIMD for 4 cycles, so insts x 4 / 1024 SIMDs over the GPU cycles of the launch (GRBM_GUI_ACTIVE / 8
    XCDs) is the fraction of the VALU issue capacity in use -- the bound these integer kernels actually sit on.
    {kernel: bytes, "valu": {kernel: {...}}}; None when rocprofv3 is absent or a traffic pass fails (bounded by a timeout)."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe) or under_profiler():
        return None  # a profiled bench.py must not start a nested profiler (its launcher would inherit the preloaded tool library)
    sums = {}
    tmp = tempfile.mkdtemp(prefix="zkhip_pmc_", dir="/tmp")
    env = {k: v for k, v in os.environ.items() if not _profiler_var(k)}
    env["TMPDIR"] = "/tmp"
    try:
        for group in (("FETCH_SIZE",), ("WRITE_SIZE",), ("SQ_INSTS_VALU", "GRBM_GUI_ACTIVE")):
            out = os.path.join(tmp, group[0])
            cmd = [exe, "--pmc"] + list(group) + ["-d", out, "-o", "pmc", "--output-format", "csv", "--", sys.executable,
                                                  os.path.join(ROOT, "tools", "pmc_child.py"), str(log_n)]
            try:
                subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300, check=True)
            except Exception:
                if len(group) == 1:
                    return None
                continue  # the issue-rate pass is an extra: the traffic figures stand without it
            acc = {}
            for path in glob.glob(out + "/**/*counter_collection.csv", recursive=True):
                for row in csv.DictReader(open(path)):
                    if row["Counter_Name"] not in group:
                        continue
                    name = row["Kernel_Name"]
                    key = "msm_bucket_acc" if "msm_bucket_acc" in name else ("ntt_pass" if "ntt_pass" in name else None)
                    if key:
                        a = acc.setdefault((key, row["Counter_Name"]), [0.0, set()])
                        a[0] += float(row["Counter_Value"])
                        a[1].add(row["Dispatch_Id"])
            if len(group) == 1 and ("msm_bucket_acc", group[0]) not in acc:
                return None
            for (key, counter), (tot, ids) in acc.items():
                sums.setdefault(key, {})[counter] = tot / max(1, len(ids))
        res = {k: int((2 * v["FETCH_SIZE"] + v["WRITE_SIZE"]) * 1024) for k, v in sums.items() if "FETCH_SIZE" in v and "WRITE_SIZE" in v}
        valu = {}
        mix = isa_mix()
        for k, v in sums.items():
            if v.get("SQ_INSTS_VALU") and v.get("GRBM_GUI_ACTIVE"):
                cycles = v["GRBM_GUI_ACTIVE"] / 8  # summed over the 8 XCDs
                valu[k] = {"wave_insts_per_launch": int(v["SQ_INSTS_VALU"]), "gpu_cycles_per_launch": int(cycles),
                           "issue_frac": round(v["SQ_INSTS_VALU"] * 4 / 1024 / cycles, 4),
                           "issue_frac_convention": "every wave instruction priced at 4 cycles (what SQ_ACTIVE_INST_VALU counts)"}
                if mix and k in mix:
                    # price the kernel's OWN instruction mix with the measured issue costs (tools/microbench2.hip,
                    # tools/mulbench4.hip): 64-bit-encoded instructions (multiply-adds, 64-bit shifts / adds) 4 cycles, VOP2 2
                    # cycles when a second wave is resident (both kernels run 3+ waves per SIMD), 4 for a lone wave
                    fr, cost = mix[k]["fractions"], mix["cycles_per_wave_instruction"]
                    per_inst = sum(fr[c] * cost[c] for c in ("mad64", "vop3", "vop2"))
                    lone = sum(fr[c] * (cost["vop2_lone_wave"] if c == "vop2" else cost[c]) for c in ("mad64", "vop3", "vop2"))
                    valu[k].update({"issue_frac_of_hw": round(v["SQ_INSTS_VALU"] * per_inst / 1024 / cycles, 4),
                                    "issue_frac_if_lone_wave": round(v["SQ_INSTS_VALU"] * lone / 1024 / cycles, 4),
                                    "priced_cycles_per_wave_instruction": round(per_inst, 3), "mix": fr,
                                    "mix_source": "profiles/isa_mix.json (tools/isa_mix.py: static ISA of the shipped kernel, stamped with the hash of csrc/)",
                                    "cost_source": cost["source"]})
        res["valu"] = valu
        return res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def isa_mix():
    """{kernel: {"fractions": {mad64, vop3, vop2}}, "cycles_per_wave_instruction": {...}} from profiles/isa_mix.json, or None when the
    file is absent or was made from other kernel sources than the tree's (its `source_sha256` stamp: tools/isa_mix.py)."""
    try:
        mix = json.load(open(os.path.join(ROOT, "profiles", "isa_mix.json")))
        spec = importlib.util.spec_from_file_location("zk_isa_mix", os.path.join(ROOT, "tools", "isa_mix.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mix if mix.get("source_sha256") == mod.sources_hash() else None
    except Exception:
        return None


def ntt_leg(np, zk, ctx, log_m=22, batch=8, steps=5, verify=True, traffic=None):
    """BASELINE config 3: radix-2 NTT over BLS12-381 Fr, domain 2^22, batch of 8, device resident, in place."""
    r = R_BLS
    w = pow(7, (r - 1) >> log_m, r)
    omega = lim(np, w)
    m = 1 << log_m
    data = random_scalars(np, batch * m, 3)
    d = ctx.malloc(data.nbytes)
    ctx.h2d(d, data)
    verified = None
    if verify:
        # out[i] = f(omega^i): the transform of the resident batch at sampled indices against the block-Horner evaluation
        # kernel (poly_eval_dev, no butterflies) of the same coefficients -- all 8 polynomials, 6 indices each
        idx = [0, 1, m // 2 + 3, m - 1, 123457, (7 * m) // 9]
        pts = np.stack([lim(np, pow(w, i, r)) for i in idx])
        want = ctx.poly_eval_dev(zk.BLS12_381, d, m, batch, pts)
        ctx.ntt_dev(zk.BLS12_381, d, log_m, batch, omega)
        got = np.zeros((batch, m, 4), dtype=np.uint64)
        ctx.d2h(got, d)
        verified = bool(all((got[b, i] == want[b, k]).all() for b in range(batch) for k, i in enumerate(idx)))
        ctx.ntt_dev(zk.BLS12_381, d, log_m, batch, omega, inverse=True)  # and back: the timed loop below starts from the same data
        ctx.d2h(got, d)
        verified = verified and bool((got.reshape(-1, 4) == data).all())
    else:
        ctx.ntt_dev(zk.BLS12_381, d, log_m, batch, omega)  # warm-up: builds the twiddle tables
    for _ in range(2):  # the host-side comparison above let the clocks drop: two untimed transforms first
        ctx.ntt_dev(zk.BLS12_381, d, log_m, batch, omega)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        ctx.ntt_dev(zk.BLS12_381, d, log_m, batch, omega)
    ctx.sync()
    dt = (time.perf_counter() - t0) / steps  # `value`: a plain loop; the per-launch HIP events come from a second one
    ctx.profile_reset()
    ctx.profile(True)
    for _ in range(steps):
        ctx.ntt_dev(zk.BLS12_381, d, log_m, batch, omega)
    ctx.sync()
    ctx.profile(False)
    k_ms, k_cnt = ctx.profile_get("ntt_pass")
    ctx.free(d)
    alg = batch * m * 64  # one read + one write of every element per transform
    achieved = alg / (k_ms / steps * 1e-3) / 1e9
    passes = k_cnt // steps
    leg = {"metric": "NTT elements/sec, BLS12-381 Fr, 2^%d x %d" % (log_m, batch), "value": round(batch * m / dt / 1e6, 2), "unit": "Melements/s",
           "ms_per_transform_batch": round(dt * 1e3, 4), "verified": verified,
           "roofline": {"bound": "hbm", "kernel": "ntt_pass (x%d per transform)" % passes, "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                        "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5),
                        "traffic": traffic["ntt_pass"] * passes if traffic and "ntt_pass" in traffic else None,  # per transform batch, like `achieved`
                        "algorithmic_bytes_per_transform_batch": alg}}
    if traffic and traffic.get("valu", {}).get("ntt_pass"):
        leg["roofline"]["valu"] = traffic["valu"]["ntt_pass"]  # per pass
    return leg


def _bench_lib():
    import ctypes

    so = os.path.join(ROOT, "crypto3-zk_amd", "libzkhip_bench.so")
    if not os.path.exists(so):
        # never build from here: this process has initialised the GPU (and may be profiled) -- spawning a compiler driver from it
        # is exactly the exec the pool forbids
        raise SystemExit("bench.py: %s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` first" % so)
    return ctypes.CDLL(so)


def groth16_leg(np, constraints=1 << 20, inputs=10, steps=4, verify=True, domain="ref", valu=None, lanes=1, curve=0):
    """The other half of BASELINE.json's metric: Groth16 prove constraints/s on one GPU (config 4's single-GPU leg: M = 2^20,
    n = 10) through the header-only shim, assignment H2D and result D2H included.  domain = "ref": the evaluation domain the
    reference reduces over, make_evaluation_domain(M + n + 1) (r1cs_to_qap.hpp:229-230) -- for M = 2^20, n = 10 the step radix-2
    domain of 2^20 + 16 points; "basic": the basic radix-2 domain of the next power of two (2^21: round 2's figure).  The key is a
    VALID key generated on the device from a fixed trapdoor over that domain; after the timed proofs the last one is held against
    the trapdoor identity (bench/groth16_bench.cpp)."""
    import ctypes

    lib = _bench_lib()
    lib.zkhip_bench_last_instance_ms.restype = ctypes.c_double
    r, g = CURVE[curve]["r"], CURVE[curve]["gen"]
    M = constraints
    m = 1
    while m < M + inputs + 1:
        m <<= 1
    # the one root both domains use: the primitive 2^ceil(log2(M + n + 1))-th (step domain: big = m / 2, omega of order 2 big)
    omega, coset = lim(np, pow(g, (r - 1) // m, r)), lim(np, g)
    times = np.zeros(steps, dtype=np.float64)
    setup = ctypes.c_double()
    verified = ctypes.c_int(-1)
    prof = ctypes.create_string_buffer(16384)
    lib.zkhip_bench_set_domain(0 if domain == "basic" else -1, ctypes.c_size_t(m if domain == "basic" else 0))
    lib.zkhip_bench_set_lanes(int(lanes))
    try:
        rc = lib.zkhip_bench_groth16(0, curve, ctypes.c_size_t(M), ctypes.c_size_t(inputs), ctypes.c_uint64(1), steps, omega.ctypes.data_as(ctypes.c_void_p),
                                     coset.ctypes.data_as(ctypes.c_void_p), times.ctypes.data_as(ctypes.c_void_p), ctypes.byref(setup),
                                     ctypes.byref(verified) if verify else None, prof, ctypes.c_size_t(16384))
    finally:
        lib.zkhip_bench_set_domain(-1, ctypes.c_size_t(0))
        lib.zkhip_bench_set_lanes(1)
    if rc != 0:
        return {"error": rc}
    lane_info = np.zeros(4, dtype=np.float64)
    lib.zkhip_bench_last_lanes(lane_info.ctypes.data_as(ctypes.c_void_p))
    info = np.zeros(8, dtype=np.uint64)
    lib.zkhip_bench_last_info(info.ctypes.data_as(ctypes.c_void_p))
    kind, dm, qa, qb, qh, ql = (int(x) for x in info[:6])
    timed = times[1:] if steps > 1 else times  # the first proof allocates the key's work buffers
    mean = float(timed.mean())
    kern = {}
    for ln in prof.value.decode(errors="ignore").splitlines():
        f = ln.split()
        if len(f) == 3:
            kern[f[0]] = round(float(f[1]), 4)
    # SURVEY 8d's algorithmic bytes of a proof: 7 transforms x m x 64 B + every G1 base and its scalar once (96 + 32 B) + the G2
    # bases of the B query (192 + 32 B)
    alg = 7 * dm * 64 + (qa + qb + qh + ql) * CURVE[curve]["bytes"][1] + qb * CURVE[curve]["bytes"][2]
    ach = alg / (mean * 1e-3) / 1e9
    tot = sum(kern.values()) or 1.0
    dom_k = max(kern, key=kern.get) if kern else None
    roof = {"bound": "hbm", "achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 6), "traffic": None,
            "algorithmic_bytes_per_proof": alg, "per": "whole proof (wall time of process(), H2D of the assignment and D2H of the results included)",
            "dominant_kernel": dom_k, "dominant_kernel_share_of_kernel_time": round(kern[dom_k] / tot, 4) if dom_k else None,
            "honest_bound": "integer VALU issue: 5 G1 + 1 G2 bucket accumulations are %.0f %% of the kernel time of a proof" %
                            (100 * sum(v for k, v in kern.items() if k.startswith("msm_bucket_acc")) / tot)}
    if valu:
        roof["valu"] = dict(valu, note="msm_bucket_acc<G1> as measured by this run's PMC child pass (the same kernel a proof spends most of its time in)")
    lanes_obj = None
    if lane_info[0] > 1:
        lanes_obj = {"lanes": int(lane_info[0]), "proofs_per_s": round(float(lane_info[1]), 2), "constraints_per_s": round(float(lane_info[1]) * M, 1),
                     "ms_per_proof_seen_by_a_lane": round(float(lane_info[2]), 2), "every_proof_equals_the_verified_one": bool(lane_info[3] == 1),
                     "what": "the THROUGHPUT arrangement, not the headline: %d provers at once on %d host threads over the SAME resident key "
                             "(r1cs_gg_ppzksnark_proving_key_hip lane constructor: the queries are shared in HBM, each lane has its own streams and "
                             "work buffers), %d proofs each; they fill each other's latency-bound phases" % (int(lane_info[0]), int(lane_info[0]), steps)}
    return {"metric": "Groth16 prove constraints/sec, %s, %d constraints, 1 GPU" % (CURVE[curve]["name"], M), "value": round(M / mean * 1e3, 1),
            "unit": "constraints/s", "statistic": "mean of the proofs after the first", "ms_per_proof": [round(float(x), 2) for x in times],
            "ms_per_proof_mean": round(mean, 3), "domain_points": dm,
            "domain": {"kind": ("basic_radix2", "extended_radix2", "step_radix2")[kind], "points": dm,
                       "chosen_by": "make_evaluation_domain(M + n + 1), as the reference (r1cs_to_qap.hpp:229-230)" if domain == "ref" else "named: next power of two"},
            "query_sizes": {"A": qa, "B": qb, "H": qh, "L": ql},
            "key": "valid Groth16 key, generated on the device from a fixed trapdoor (r1cs_gg_ppzksnark_generator_hip), resident",
            "key_setup_ms": round(setup.value, 1),
            "key_setup_what": "r1cs_gg_ppzksnark_generator_hip::deterministic_basic_process alone (generator.hpp:240-377: QAP at the trapdoor with the "
                              "Lagrange basis on the device, five batch exponentiations, window tables); building the synthetic circuit took instance_build_ms",
            "instance_build_ms": round(float(lib.zkhip_bench_last_instance_ms()), 1),
            "verified": None if not verify else bool(verified.value == 1),
            "verification": "proof == (a G1, b G2, c G1) with a, b, c from the trapdoor identities (prover.hpp:141-153)",
            "roofline": roof, "kernel_ms_serial_proof": kern,
            "kernel_ms_source": "HIP events around every launch of ONE extra, untimed proof with the G2 multiexp on the main stream: a single in-order "
                                "stream makes the event pairs exact kernel durations (the timed proofs run the G2 multiexp on a second stream and carry no events)", **({"lanes_over_one_key": lanes_obj} if lanes_obj else {})}


def msm_other_leg(np, zk, ctx, curve, group, log_n=20, steps=10, warmup=3, verify=True):
    """north_star names both curves and both groups; the headline is BLS12-381 G1.  The same step for another (curve, group): ONE MSM of
    2^log_n device-generated points (P_i = k_i G) and uniform scalars, bases and scalars resident.  Checked after the timing against
    (sum s_i k_i) G from the fixed-base kernel (host big integers for the exponent, no bucket method); cpu_baseline() additionally holds a
    2^16-point prefix of the same inputs against the oracle's Pippenger."""
    n = 1 << log_n
    seed = 3000 + 10 * curve + group
    r = CURVE[curve]["r"]
    ks, sc = random_scalars(np, n, seed), random_scalars(np, n, seed + 1)
    if curve != 0:  # random_scalars draws below the BLS12-381 modulus; BN254's is smaller: 252-bit values are canonical for both
        ks[:, 3] &= np.uint64(0x0FFFFFFFFFFFFFFF)
        sc[:, 3] &= np.uint64(0x0FFFFFFFFFFFFFFF)
    bases = ctx.bases_from_scalars(curve, group, ks)
    cl = zk.coord_limbs(curve, group)
    d_s, d_o = ctx.malloc(sc.nbytes), ctx.malloc(3 * cl * 8)
    ctx.h2d(d_s, sc)
    for _ in range(warmup):
        ctx.msm_dev(bases, d_s, d_o, 0, n)
    ctx.sync()
    ctx.profile_reset()
    ctx.profile_filter("msm_bucket_acc")
    ctx.profile(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        ctx.msm_dev(bases, d_s, d_o, 0, n)
    ctx.sync()
    dt = (time.perf_counter() - t0) / steps
    ctx.profile(False)
    acc_ms, acc_cnt = ctx.profile_get("msm_bucket_acc")
    ctx.profile_filter("")
    ctx.profile_reset()
    jac = np.zeros((3, cl), dtype=np.uint64)
    ctx.d2h(jac, d_o)
    ok = None
    if verify:
        e = sum(a * b for a, b in zip(to_ints(ks), to_ints(sc))) % r
        got, got_inf = ctx.jacobian_to_affine(curve, group, jac)
        eb = ctx.bases_from_scalars(curve, group, lim(np, e).reshape(1, 4))
        exp, exp_inf = eb.download()
        eb.free()
        ok = bool(int(exp_inf[0]) == got_inf and (exp[0] == got).all())
    ctx.free(d_s), ctx.free(d_o)
    alg = CURVE[curve]["bytes"][group] * n
    avg = acc_ms / max(1, acc_cnt)
    ach = alg / (avg * 1e-3) / 1e9 if avg > 0 else 0.0
    out = {"metric": "MSM Mpoints/sec, %s G%d Pippenger, 2^%d points" % (CURVE[curve]["name"], group, log_n), "value": round(n / dt / 1e6, 3), "unit": "Mpoints/s",
           "ms_per_msm": round(dt * 1e3, 4), "verified": ok, "verified_vs": "(sum s_i k_i) G by the fixed-base kernel",
           "roofline": {"bound": "hbm", "kernel": "msm_bucket_acc", "achieved": round(ach, 3), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 6),
                        "traffic": None, "avg_launch_ms": round(avg, 4), "algorithmic_bytes_per_launch": alg},
           "_inputs": (bases, ks, sc)}  # kept for cpu_baseline()'s oracle check of a prefix; dropped before the line is written
    return out


def groth16_group_leg(np, devices, transport=0, log_constraints=20, inputs=10, steps=4, verify=True, curve=0):
    """BASELINE cfg 4's arrangement AS A C++ CALLER OF THE DROP-IN CLASS REACHES IT: one process, one host thread, a device_group of
    len(devices) contexts, r1cs_gg_ppzksnark_prover_hip::process(group key, x, w) -- every member holds a point-range slice of every query
    (generated on its own GPU), runs the replicated witness map and its five partial multiexps, and the 864-byte exchange happens INSIDE
    the library (zkhip_group_all_gather: RCCL over xGMI between distinct GPUs, peer copies between members that share one).  On a one-GPU
    box the members share device 0: that measures the orchestration, not a speed-up, and the leg says so."""
    import ctypes

    lib = _bench_lib()
    r, g = CURVE[curve]["r"], CURVE[curve]["gen"]
    M = 1 << log_constraints
    m = 1
    while m < M + inputs + 1:
        m <<= 1
    omega, coset = lim(np, pow(g, (r - 1) // m, r)), lim(np, g)
    times = np.zeros(steps, dtype=np.float64)
    setup = ctypes.c_double()
    verified = ctypes.c_int(-1)
    info = np.zeros(5, dtype=np.float64)
    devs = (ctypes.c_int * len(devices))(*devices)
    rc = lib.zkhip_bench_groth16_group(devs, len(devices), int(transport), curve, ctypes.c_size_t(M), ctypes.c_size_t(inputs), ctypes.c_uint64(1), steps,
                                       omega.ctypes.data_as(ctypes.c_void_p), coset.ctypes.data_as(ctypes.c_void_p), times.ctypes.data_as(ctypes.c_void_p),
                                       ctypes.byref(setup), ctypes.byref(verified) if verify else None, info.ctypes.data_as(ctypes.c_void_p))
    if rc != 0:
        return {"error": rc}
    mean = float(times.mean())
    distinct = len(set(devices))
    return {"metric": "Groth16 prove constraints/sec, %s, 2^%d constraints, ONE proof over a device group of %d member(s) on %d GPU(s), one process" %
                      (CURVE[curve]["name"], log_constraints, len(devices), distinct),
            "value": round(M / mean * 1e3, 1), "unit": "constraints/s", "scaling": "strong", "ms_per_proof": [round(float(x), 2) for x in times],
            "ms_per_proof_mean": round(mean, 3), "members": len(devices), "distinct_gpus": distinct, "devices": list(devices),
            "transport": ("auto", "rccl", "peer", "staged")[int(info[4])],
            "host_phase_ms": {"launches_all_members": round(float(info[0]), 3), "host_products": round(float(info[1]), 3),
                              "exchange_and_wait": round(float(info[2]), 3), "assembly": round(float(info[3]), 3)},
            "key_setup_ms": round(setup.value, 1), "verified": None if not verify else bool(verified.value == 1),
            "verification": "every timed proof equal to the first and to (a G1, b G2, c G1) from the trapdoor identities (prover.hpp:141-153)",
            "what": ("members on distinct GPUs: the single-process form of groth16_sharded" if distinct == len(devices) else
                     "EMULATION: %d members share %d GPU(s) -- the group's orchestration and exchange at work, not a speed-up (their kernels queue on one device)"
                     % (len(devices), distinct))}


def group_child(args):
    """`bench.py --group-child 0,1,...`: the device-group legs in a process of their own (see run_group_child); ONE JSON line on stdout."""
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)  # librccl announces itself on the C stdout
    import numpy as np
    import torch  # noqa: F401  (first: libzkhip.so shares torch's HIP runtime and, for the group's exchange, its librccl)

    devices = [int(x) for x in args.group_child.split(",") if x != ""]
    legs = set(args.child_legs.split(","))
    out = {}
    if "groth16" in legs:
        out["groth16_device_group"] = groth16_group_leg(np, devices, log_constraints=args.log_constraints, steps=4, verify=not args.no_verify)
    if "kzg" in legs:
        import ctypes

        log_n, cols = args.kzg_log_rows, 50
        data = random_scalars(np, (1 << log_n) * cols, 5).reshape(cols, 1 << log_n, 4)  # the columns of kzg_leg (same seed)
        raw = None
        if not args.no_verify:
            # the single-device scheme class over the same columns (its commitments are what kzg_leg checks against f(alpha) G in the parent)
            lib = _bench_lib()
            ms = np.zeros(3, dtype=np.float64)
            raw = np.zeros((cols, 12), dtype=np.uint64)
            rc = lib.zkhip_bench_kzg_scheme(devices[0], ctypes.c_size_t(log_n), ctypes.c_size_t(cols), 1, 2, ctypes.c_size_t(10), data.ctypes.data_as(ctypes.c_void_p),
                                            ms.ctypes.data_as(ctypes.c_void_p), raw.ctypes.data_as(ctypes.c_void_p))
            if rc != 0:
                raw = None
        out["kzg_device_group"] = kzg_group_leg(np, data, log_n, cols, raw, devices)
        out["kzg_device_group"]["verification"] = "all %d commitments equal the single-device scheme class's over the same columns (same process); the parent checks those against f(alpha) G" % cols
    if "lpc" in legs:
        out["lpc_device_group"] = lpc_group_leg(np, devices, verify=not args.no_verify)
    os.write(json_fd, (json.dumps(out, separators=(",", ":")) + "\n").encode())
    return 0


def lpc_group_leg(np, devices, log_n=20, cols=16, steps=4, verify=True):
    """The LPC commit of lpc_leg -- 16 polynomial_dfs of 2^20 rows from host memory, D[0] = 2^21, 1.07 GB of leaves to a streaming tree builder --
    through lpc_commitment_scheme_hip over a DEVICE GROUP: the polynomials dealt over the members (own uploads, own extensions), the leaves cut by
    range over the leaf owners (segments packed and pushed device to device, each owner's leaves over its own PCIe link), absorbed in leaf order."""
    import ctypes

    lib = _bench_lib()
    ms = np.zeros(steps, dtype=np.float64)
    root, owners = ctypes.c_uint64(0), ctypes.c_uint64(0)
    devs = (ctypes.c_int * len(devices))(*devices)
    rc = lib.zkhip_bench_lpc_scheme_group(devs, len(devices), ctypes.c_size_t(log_n), ctypes.c_size_t(cols), ctypes.c_size_t(1), steps, 16,
                                          ms.ctypes.data_as(ctypes.c_void_p), ctypes.byref(root), ctypes.byref(owners))
    if rc != 0:
        return {"error": rc}
    single = None
    if verify:  # one commit of the same seeded polynomials through the scheme on one context: the same position-weighted fold
        ms1 = np.zeros(1, dtype=np.float64)
        r1 = ctypes.c_uint64(0)
        if lib.zkhip_bench_lpc_scheme(devices[0], ctypes.c_size_t(log_n), ctypes.c_size_t(cols), ctypes.c_size_t(1), 1, 1, 16, ms1.ctypes.data_as(ctypes.c_void_p),
                                      ctypes.byref(r1)) == 0:
            single = r1.value
    distinct = len(set(devices))
    return {"metric": "LPC commit through lpc_commitment_scheme_hip over a device group of %d member(s) on %d GPU(s), %d polynomial_dfs x 2^%d rows from HOST memory, "
                      "domain 2^%d" % (len(devices), distinct, cols, log_n, log_n + 1),
            "value": round(float(ms[1:].mean()) if steps > 1 else float(ms[0]), 2), "unit": "ms per commit", "higher_is_better": False, "scaling": "strong",
            "ms_per_commit": [round(float(x), 2) for x in ms], "members": len(devices), "distinct_gpus": distinct, "leaf_owners": int(owners.value),
            "verified": None if single is None else bool(single == root.value),
            "verification": "the position-weighted fold over the leaves equals the single-context scheme's over the same polynomials (same process); the parent's "
                            "cpu_baseline holds THAT fold against the oracle's leaf layout",
            "what": "members on distinct GPUs" if distinct == len(devices) else "EMULATION: the members share %d GPU(s) -- the orchestration at work, not a speed-up" % distinct}


def run_group_child(devices, legs, args, timeout=900):
    """The device-group legs in a CHILD process (python bench.py --group-child ...): the group over several distinct GPUs runs RCCL single-process
    communicators over xGMI, which no round of this build could test on hardware -- a failure or a hang there must cost the leg, not the line (the
    child is started the ordinary way, a new process, never an exec from this one)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--group-child", ",".join(str(d) for d in devices), "--child-legs", ",".join(legs),
           "--log-constraints", str(args.log_constraints), "--kzg-log-rows", str(args.kzg_log_rows)] + (["--no-verify"] if args.no_verify else [])
    names = {"groth16": "groth16_device_group", "kzg": "kzg_device_group", "lpc": "lpc_device_group"}
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, text=True)
        lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
        if r.returncode != 0 or not lines:
            raise RuntimeError("exit code %d: %s" % (r.returncode, r.stderr[-300:].replace("\n", " | ")))
        return json.loads(lines[-1])
    except Exception as e:  # noqa: BLE001  (a timeout, a crash, a malformed line: the leg says so)
        return {names[l]: {"error": "device-group child failed: %s" % str(e)[:400]} for l in legs}


def _last_domain(np, lib):
    import ctypes

    info = np.zeros(8, dtype=np.uint64)
    lib.zkhip_bench_last_info(info.ctypes.data_as(ctypes.c_void_p))
    return {"kind": ("basic_radix2", "extended_radix2", "step_radix2")[int(info[0])], "points": int(info[1])}


def groth16_sharded_leg(np, torch, dist, rank, world, local_rank, log_constraints=20, inputs=10, steps=3, verify=True):
    """BASELINE config 4: one Groth16 proof (M = 2^20, n = 10) sharded over `world` GPUs, one process each: every rank holds
    a point-range slice of each query of the SAME valid key (generated per rank on its device), runs the witness map in
    full and its five partial MSMs; the only exchange is one RCCL all-gather of 864 bytes per rank per proof, after which
    every rank assembles the proof and checks it against the trapdoor identity.  Strong scaling: the work of one proof is fixed."""
    import ctypes

    if rank == 0:
        _bench_lib()
    dist.barrier(device_ids=[local_rank])
    lib = _bench_lib()
    r, g = R_BLS, 7
    M = 1 << log_constraints
    m = 1
    while m < M + inputs + 1:
        m <<= 1
    omega, coset = lim(np, pow(g, (r - 1) // m, r)), lim(np, g)
    dev = torch.device("cuda", local_rank)

    @ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)
    def all_gather(mine, words, out):  # host-buffer form (kept for callers without device buffers; not used below)
        src = np.ctypeslib.as_array(ctypes.cast(mine, ctypes.POINTER(ctypes.c_uint64)), (words,))
        t = torch.from_numpy(src.view(np.int64).copy()).to(dev)
        gathered = torch.empty(world * words, dtype=torch.int64, device=dev)
        dist.all_gather_into_tensor(gathered, t)
        dst = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_uint64)), (world * words,))
        dst[:] = gathered.cpu().numpy().view(np.uint64)

    # the exchange stays on the device: the prover copies its 864 bytes of partial sums into t_mine (device to device), the
    # collective runs on the two tensors, one download of t_all follows (r1cs_gg_ppzksnark_prover_hip::process_device_gather)
    words = 4 * 18 + 36  # 4 G1 + 1 G2 Jacobian points
    t_mine = torch.zeros(words, dtype=torch.int64, device=dev)
    t_all = torch.zeros(world * words, dtype=torch.int64, device=dev)

    @ctypes.CFUNCTYPE(None)
    def gather_dev():
        dist.all_gather_into_tensor(t_all, t_mine)  # RCCL (or gloo through the host: Comm)
        torch.cuda.synchronize()

    lib.zkhip_bench_set_device_gather(gather_dev, ctypes.c_void_p(t_mine.data_ptr()), ctypes.c_void_p(t_all.data_ptr()))
    times = np.zeros(steps, dtype=np.float64)
    setup = ctypes.c_double()
    verified = ctypes.c_int(-1)
    rc = lib.zkhip_bench_groth16_sharded(local_rank, ctypes.c_size_t(rank), ctypes.c_size_t(world), all_gather, 0, ctypes.c_size_t(M),
                                         ctypes.c_size_t(inputs), ctypes.c_uint64(1), steps, omega.ctypes.data_as(ctypes.c_void_p),
                                         coset.ctypes.data_as(ctypes.c_void_p), times.ctypes.data_as(ctypes.c_void_p), ctypes.byref(setup),
                                         ctypes.byref(verified) if verify else None)
    lib.zkhip_bench_set_device_gather(None, None, None)
    if rc != 0:
        # this rank left the proof loop early: its peers are inside an all-gather it will never join.  Joining a DIFFERENT collective
        # now would mismatch them until the RCCL timeout -- leave, non-zero, so that the launcher tears the job down at once.
        print("bench.py: rank %d failed inside the sharded Groth16 leg (rc = %d): aborting the job" % (rank, rc), file=sys.stderr, flush=True)
        os._exit(3)
    bad = float(verify and verified.value != 1)
    t = torch.tensor(list(times) + [bad], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)  # a proof is done when the slowest rank is; `bad` is set when ANY rank's check failed
    t = t.cpu().numpy()
    timed = t[1:-1] if steps > 1 else t[:1]
    mean = float(timed.mean())
    return {"metric": "Groth16 prove constraints/sec, BLS12-381, 2^%d constraints, ONE proof sharded over %d GPU(s)" % (log_constraints, world),
            "value": round(M / mean * 1e3, 1), "unit": "constraints/s", "scaling": "strong", "statistic": "mean of the proofs after the first",
            "ms_per_proof": [round(float(x), 2) for x in t[:-1]], "ms_per_proof_mean": round(mean, 3),
            "domain": _last_domain(np, lib), "exchange": "one all-gather of 864 B per rank per proof, on device buffers (no host round trip before the collective)",
            "key": "valid key from a fixed trapdoor, each rank generates and holds 1/%d of every query" % world,
            "verified": None if not verify else bool(t[-1] == 0)}


def kzg_leg(np, zk, ctx, log_n=20, cols=50, steps=2, verify=True, valu=None, group_devices=None):
    """BASELINE config 5's commitment layer on one GPU: KZG commit of 50 witness columns of 2^20 rows (per column one
    inverse NTT + one G1 MSM against the resident SRS alpha^i G, alpha = 7 as placeholder.cpp:175; kzg_v2.hpp:208-226)
    and the device part of the batched opening proof of the same columns at two points (kzg_v2.hpp:236-305), the
    coefficient forms staying resident in between.  Checked afterwards in the exponent (alpha is known here):
    every commitment == f(alpha) G, the coefficient forms reproduce sampled rows, and pi_1, pi_2 satisfy the division
    identities they are defined by."""
    n = 1 << log_n
    r, alpha = R_BLS, 7
    w = pow(7, (r - 1) >> log_n, r)
    omega = lim(np, w)
    x, pw = 1, np.empty((n, 4), dtype=np.uint64)
    for i in range(n):  # alpha^i as canonical limbs
        pw[i, 0], pw[i, 1], pw[i, 2], pw[i, 3] = x & MASK64, (x >> 64) & MASK64, (x >> 128) & MASK64, x >> 192
        x = x * alpha % r
    srs = ctx.bases_from_scalars(zk.BLS12_381, zk.G1, pw)
    data = random_scalars(np, n * cols, 5).reshape(cols, n, 4)
    d = ctx.malloc(data.nbytes)
    d_out = ctx.malloc(cols * 144)
    ptrs = [d + 32 * n * c for c in range(cols)]
    commit = []
    for _ in range(steps + 1):
        ctx.h2d(d, data)
        t0 = time.perf_counter()
        ctx.ntt_dev(zk.BLS12_381, d, log_n, cols, omega, inverse=True)
        ctx.msm_batch_dev([srs] * cols, ptrs, [d_out + 144 * c for c in range(cols)], ns=[n] * cols)
        ctx.sync()
        commit.append((time.perf_counter() - t0) * 1e3)
    pts = random_scalars(np, 2, 9)
    th = random_scalars(np, cols + 1, 10)
    d_f, d_l, d_pi = ctx.malloc(n * 32), ctx.malloc(n * 32), ctx.malloc(2 * 144)
    opening = []
    for _ in range(steps + 1):
        t0 = time.perf_counter()
        zvals = ctx.poly_eval_dev(zk.BLS12_381, d, n, cols, pts)
        ctx.poly_lincomb_dev(zk.BLS12_381, ptrs, [n] * cols, th[:cols], 1, d_f, n, False)
        ctx.poly_div_linear_dev(zk.BLS12_381, d_f, n, pts[0], d_f)
        ctx.poly_div_linear_dev(zk.BLS12_381, d_f + 32, n - 1, pts[1], d_f + 32)
        ctx.msm_dev(srs, d_f + 64, d_pi, 0, n - 2)
        ctx.poly_lincomb_dev(zk.BLS12_381, ptrs + [d_f + 64], [n] * cols + [n - 2], th, 1, d_l, n, False)
        ctx.poly_div_linear_dev(zk.BLS12_381, d_l, n, pts[0], d_l)
        ctx.msm_dev(srs, d_l + 32, d_pi + 144, 0, n - 1)
        ctx.sync()
        opening.append((time.perf_counter() - t0) * 1e3)
    verified = None
    if verify:
        def affine_of(dptr):
            jac = np.zeros((3, 6), dtype=np.uint64)
            ctx.d2h(jac, dptr)
            return ctx.jacobian_to_affine(zk.BLS12_381, zk.G1, jac)

        def times_g(e):  # e G by the fixed-base kernel
            b = ctx.bases_from_scalars(zk.BLS12_381, zk.G1, lim(np, e % r).reshape(1, 4))
            p, inf = b.download()
            b.free()
            return p[0], int(inf[0])

        def same(a, b):
            return a[1] == b[1] and bool((a[0] == b[0]).all())

        # f_c(alpha), f_c(z0), f_c(z1) for all columns from the resident coefficient forms (block-Horner kernel)
        z0, z1 = to_ints(pts)
        ev = ctx.poly_eval_dev(zk.BLS12_381, d, n, cols, np.stack([lim(np, alpha), pts[0], pts[1]]))
        fa = [to_ints(ev[c]) for c in range(cols)]
        ok = all(same(affine_of(d_out + 144 * c), times_g(fa[c][0])) for c in range(cols))  # 50 commitments == f(alpha) G
        # the coefficient forms are the inverse transforms of the rows: sampled rows j reproduce data[c, j] = f_c(omega^j)
        rows = [0, 1, n // 3, n - 1]
        back = ctx.poly_eval_dev(zk.BLS12_381, d, n, cols, np.stack([lim(np, pow(w, j, r)) for j in rows]))
        ok = ok and bool(all((back[c, k] == data[c, j]).all() for c in range(cols) for k, j in enumerate(rows)))
        ok = ok and bool((zvals == ev[:, 1:]).all())
        # pi_1 = commit(q), q = floor(f / ((X - z0)(X - z1))), f = sum theta_c f_c:  f - U = q V with U the interpolation of f at z0, z1
        thi = to_ints(th)
        f_a, f_0, f_1 = (sum(thi[c] * fa[c][k] for c in range(cols)) % r for k in range(3))
        slope = (f_1 - f_0) * pow(z1 - z0, -1, r) % r
        u_a = (f_0 + slope * (alpha - z0)) % r
        q_a = (f_a - u_a) * pow((alpha - z0) * (alpha - z1) % r, -1, r) % r
        ok = ok and same(affine_of(d_pi), times_g(q_a))
        # pi_2 = commit((L - L(z0)) / (X - z0)), L = sum theta_c f_c + theta_cols q
        l_a = (f_a + thi[cols] * q_a) % r
        q_0 = to_ints(ctx.poly_eval_dev(zk.BLS12_381, d_f + 64, n - 2, 1, pts[:1])[0])[0]  # q(z0) by Horner on the resident quotient
        l_0 = (f_0 + thi[cols] * q_0) % r
        ok = ok and same(affine_of(d_pi + 144), times_g((l_a - l_0) * pow(alpha - z0, -1, r)))
        verified = bool(ok)
    # per-kernel times of one more commit (HIP events around every launch), for the leg's roofline object
    ctx.h2d(d, data)
    ctx.profile_reset()
    ctx.profile(True)
    ctx.ntt_dev(zk.BLS12_381, d, log_n, cols, omega, inverse=True)
    ctx.msm_batch_dev([srs] * cols, ptrs, [d_out + 144 * c for c in range(cols)], ns=[n] * cols)
    ctx.sync()
    ctx.profile(False)
    kern = {k: round(v[0], 3) for k, v in sorted(ctx.profile_dump().items())}
    raw_affine = None
    if verify:  # the commitments of the raw path (checked above), for the scheme-class run below to be held against
        jac = np.zeros((cols, 3, 6), dtype=np.uint64)
        ctx.d2h(jac, d_out)
        raw_affine = np.stack([ctx.jacobian_to_affine(zk.BLS12_381, zk.G1, jac[c])[0] for c in range(cols)])
    for p in (d, d_out, d_f, d_l, d_pi):
        ctx.free(p)
    srs.free()
    mean = sum(commit[1:]) / len(commit[1:])
    # per column one read + one write of the vector by the transform (64 B / row), the coefficients read by the
    # multiexp (32 B / row) and the SRS point (96 B / row) -- the SRS counted once PER COLUMN (50 x), as each column's MSM reads it
    alg = cols * n * (64 + 32 + 96)
    ach = alg / (mean * 1e-3) / 1e9
    tot = sum(kern.values()) or 1.0
    dom_k = max(kern, key=kern.get) if kern else None
    roof = {"bound": "hbm", "achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 6), "traffic": None,
            "algorithmic_bytes_per_commit": alg, "srs_reads_counted": "%d x (once per column); %d B if counted once" % (cols, cols * n * 96 + n * 96),
            "per": "whole commit (%d inverse transforms + %d multiexps, columns resident)" % (cols, cols),
            "dominant_kernel": dom_k, "dominant_kernel_share_of_kernel_time": round(kern[dom_k] / tot, 4) if dom_k else None,
            "honest_bound": "integer VALU issue: the bucket accumulations are %.0f %% of the kernel time" %
                            (100 * sum(v for k, v in kern.items() if k.startswith("msm_bucket_acc")) / tot)}
    if valu:
        roof["valu"] = dict(valu, note="msm_bucket_acc<G1> as measured by this run's PMC child pass")
    leg = {"metric": "KZG commit columns/sec, BLS12-381, %d columns x 2^%d rows, 1 GPU (columns and SRS resident)" % (cols, log_n),
           "value": round(cols / mean * 1e3, 2), "unit": "columns/s", "statistic": "mean of the commits after the first",
           "ms_per_commit": [round(t, 2) for t in commit], "ms_per_commit_mean": round(mean, 3),
           "opening_proof_ms": [round(t, 2) for t in opening], "opening_proof_ms_mean": round(sum(opening[1:]) / len(opening[1:]), 3),
           "opening_proof": "device part of kzg_v2 proof_eval for the same %d columns at 2 points, coefficient forms resident" % cols,
           "verified": verified,
           "verification": "50 commitments == f(alpha) G; sampled rows reproduced from the coefficient forms; pi_1, pi_2 == their division identities in the exponent",
           "roofline": roof, "kernel_ms_one_commit": kern}
    leg["scheme_class"] = kzg_scheme_leg(np, data, log_n, cols, raw_affine)
    if group_devices:
        leg["device_group"] = kzg_group_leg(np, data, log_n, cols, raw_affine, group_devices)
    return leg


def kzg_scheme_leg(np, data, log_n, cols, raw_affine, steps=3):
    """The same 50 columns THROUGH kzg_commitment_scheme_v2_hip (hip/kzg_v2.hpp), starting in HOST memory as placeholder hands them
    over: append_to_batch (lent: std::cref) + commit (upload in chunks under the previous chunk's kernels, inverse transforms,
    multiexps, download of the commitments) + proof_eval at two points.  Its commitments must equal the raw path's."""
    import ctypes

    lib = _bench_lib()
    ms = np.zeros(3 * steps, dtype=np.float64)
    out = np.zeros((cols, 12), dtype=np.uint64)
    rc = lib.zkhip_bench_kzg_scheme(0, ctypes.c_size_t(log_n), ctypes.c_size_t(cols), steps, 2, ctypes.c_size_t(10), data.ctypes.data_as(ctypes.c_void_p),
                                    ms.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    if rc != 0:
        return {"error": rc}
    ms = ms.reshape(steps, 3)
    mean = float(ms[1:, 1].mean())
    return {"metric": "KZG commit columns/sec through kzg_commitment_scheme_v2_hip, %d columns x 2^%d rows from HOST memory (PCIe-inclusive)" % (cols, log_n),
            "value": round(cols / mean * 1e3, 2), "unit": "columns/s", "statistic": "mean of the commits after the first",
            "ms_append_to_batch": [round(float(x), 2) for x in ms[:, 0]], "ms_commit": [round(float(x), 2) for x in ms[:, 1]],
            "ms_proof_eval": [round(float(x), 2) for x in ms[:, 2]],
            "handover": "append_to_batch(std::cref): lent, no host copy; upload in chunks of 10 columns on a second stream",
            "verified": None if raw_affine is None else bool((out == raw_affine).all()),
            "verification": "all %d commitments equal the raw-ABI path's (themselves checked against f(alpha) G)" % cols}


def kzg_group_leg(np, data, log_n, cols, raw_affine, devices, steps=3):
    """BASELINE cfg 5's commitment leg AS A C++ CALLER OF THE DROP-IN CLASS REACHES SEVERAL GPUs: kzg_commitment_scheme_v2_hip over
    kzg_params_group_hip -- one process, the key replicated on every member of the device group, commit(batch) dealing the 50 columns (each
    member uploads, transforms and commits its own on a host thread of its own), the coefficient forms gathered on member 0 device to device,
    proof_eval there.  On a one-GPU box the members share device 0 (an emulation: the orchestration, not a speed-up)."""
    import ctypes

    lib = _bench_lib()
    ms = np.zeros(2 * steps, dtype=np.float64)
    out = np.zeros((cols, 12), dtype=np.uint64)
    devs = (ctypes.c_int * len(devices))(*devices)
    rc = lib.zkhip_bench_kzg_scheme_group(devs, len(devices), ctypes.c_size_t(log_n), ctypes.c_size_t(cols), steps, data.ctypes.data_as(ctypes.c_void_p),
                                          ms.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    if rc != 0:
        return {"error": rc}
    ms = ms.reshape(steps, 2)
    mean = float(ms[1:, 0].mean()) if steps > 1 else float(ms[0, 0])
    distinct = len(set(devices))
    return {"metric": "KZG commit columns/sec through kzg_commitment_scheme_v2_hip over a device group of %d member(s) on %d GPU(s), %d columns x 2^%d rows from HOST memory"
                      % (len(devices), distinct, cols, log_n),
            "value": round(cols / mean * 1e3, 2), "unit": "columns/s", "scaling": "strong", "ms_commit": [round(float(x), 2) for x in ms[:, 0]],
            "ms_proof_eval": [round(float(x), 2) for x in ms[:, 1]], "members": len(devices), "distinct_gpus": distinct,
            "verified": None if raw_affine is None else bool((out == raw_affine).all()),
            "verification": "all %d commitments equal the single-device raw-ABI path's (themselves checked against f(alpha) G)" % cols,
            "what": "members on distinct GPUs" if distinct == len(devices) else "EMULATION: the members share %d GPU(s) -- the orchestration at work, not a speed-up" % distinct}


def lpc_leg(np, log_n=20, cols=16, steps=4):
    """lpc_commitment_scheme_hip::commit of 16 polynomial_dfs of 2^20 rows from host memory over D[0] = 2^21: upload, inverse NTTs,
    extension, coset-ordered leaf layout and 1.07 GB of leaves handed to the caller's tree builder -- in the streaming shape (slices
    absorbed by 16 host threads while the next one is in flight) and as a std::vector (round 2's shape).  The builder only folds
    the leaves (XOR): hashing is the caller's; both shapes must yield the same fold."""
    import ctypes

    lib = _bench_lib()
    res = {}
    roots = []
    for name, streaming in (("streaming_builder", 1), ("vector_builder", 0)):
        ms = np.zeros(steps, dtype=np.float64)
        root = ctypes.c_uint64(0)
        rc = lib.zkhip_bench_lpc_scheme(0, ctypes.c_size_t(log_n), ctypes.c_size_t(cols), ctypes.c_size_t(1), steps, streaming, 16,
                                        ms.ctypes.data_as(ctypes.c_void_p), ctypes.byref(root))
        if rc != 0:
            return {"error": rc}
        res[name] = {"ms_per_commit": [round(float(x), 2) for x in ms], "mean_after_first_ms": round(float(ms[1:].mean()), 2)}
        roots.append(root.value)
    # the opening proof of the same batch (two points per polynomial) up to and including the FRI commit phase
    pe_steps = 4
    ms = np.zeros(2 * pe_steps, dtype=np.float64)
    rounds = ctypes.c_uint64(0)
    rc = lib.zkhip_bench_lpc_proof_eval(0, ctypes.c_size_t(log_n), ctypes.c_size_t(cols), ctypes.c_size_t(1), pe_steps, 16, ms.ctypes.data_as(ctypes.c_void_p),
                                        ctypes.byref(rounds))
    if rc == 0:
        pe = ms.reshape(pe_steps, 2)[1:, 1]
        res["proof_eval"] = {"workload": "lpc_commitment_scheme_hip::proof_eval of the same %d polynomials at 2 points each: evaluations, combined quotient, its extension "
                                         "to D[0], %d FRI rounds (one fold each) with every round's leaves to the tree builder" % (cols, int(rounds.value)),
                             "ms_per_proof": [round(float(x), 2) for x in ms.reshape(pe_steps, 2)[:, 1]], "median_after_first_ms": round(float(np.median(pe)), 2)}
    return {"metric": "LPC commit, %d polynomial_dfs x 2^%d rows from host memory, domain 2^%d, leaves to the caller's tree builder" % (cols, log_n, log_n + 1),
            "value": res["streaming_builder"]["mean_after_first_ms"], "unit": "ms per commit", "higher_is_better": False,
            "leaf_bytes": cols * (2 << log_n) * 32, **res, "proof_eval_ms": (res.get("proof_eval") or {}).get("median_after_first_ms"),
            "verified": roots[0] == roots[1],
            "verification": "the streaming and the vector builder yield the same POSITION-WEIGHTED fold sum_k (k + 1) w_k mod 2^64 over the leaves' u64 words",
            "_fold": roots[0], "_shape": (log_n, cols)}  # cpu_baseline() holds the fold against the oracle's leaf layout of the same polynomials


def quotient_leg(np, log_n=20, steps=6, verify=True):
    """placeholder's quotient-polynomial chain at BASELINE config 5's row count (hip/placeholder_quotient.hpp mirrors
    prover.hpp:220-277, 314-317 and the polynomial_dfs side of gates_argument.hpp:203-216), every column resident: one gate of four
    factors over the 4n-point extended domain, a second part over 2n points, F / (X^n - 1), the split into 4 parts and
    commit(QUOTIENT_BATCH) through kzg_commitment_scheme_v2_hip from the resident parts (bench/scheme_bench.cpp)."""
    import ctypes

    lib = _bench_lib()
    ms = np.zeros(5 * steps, dtype=np.float64)
    verified = ctypes.c_int(-1)
    rc = lib.zkhip_bench_quotient(0, ctypes.c_size_t(log_n), steps, ms.ctypes.data_as(ctypes.c_void_p), ctypes.byref(verified) if verify else None)
    if rc != 0:
        return {"error": rc}
    ms = ms.reshape(steps, 5)
    timed = ms[2:] if steps > 2 else ms    # the first two runs warm the transforms' tables and the context's block cache
    mean = np.median(timed, axis=0)
    total = float(np.median(timed.sum(axis=1)))
    n = 1 << log_n
    # SURVEY 8d's accounting, 64 B per element per transform + 128 B per (base, scalar) of a multiexp:
    #   gate argument   4 factors + the mask, each iNTT(n) + NTT(4n)                      25 n
    #   second part     w1, w2, w3: iNTT(n) + NTT(2n)                                      9 n
    #   quotient        F1 2n -> 4n: iNTT(2n) + NTT(4n); coefficients(): iNTT(4n)         10 n
    #   split           4 x from_coefficients: NTT(n)                                      4 n
    #   commit          4 x coefficients(): iNTT(n); 4 multiexps of n points               4 n   (+ 4 n x 128 B)
    alg = 52 * n * 64 + 4 * n * 128
    ach = alg / (total * 1e-3) / 1e9
    names = ("gate_argument", "second_part", "quotient_polynomial", "split_from_coefficients", "commit_quotient_batch")
    return {"metric": "placeholder quotient chain, BLS12-381, 2^%d rows (one 4-factor gate over the 4x extended domain + one part over 2x), columns resident" % log_n,
            "value": round(total, 3), "unit": "ms per chain", "higher_is_better": False, "statistic": "median of the runs after the first two",
            "ms_by_phase": {k: round(float(v), 3) for k, v in zip(names, mean)}, "ms_per_run": [round(float(x), 2) for x in ms.sum(axis=1)],
            "verified": None if not verify else bool(verified.value == 1),
            "verification": "T(y) (y^n - 1) == alpha_0 G(y) + alpha_1 F1(y) at a random y; every commitment == part_k(alpha) G1",
            "roofline": {"bound": "hbm", "achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 6), "traffic": None,
                         "algorithmic_bytes_per_chain": alg, "per": "whole chain: 52 n transform elements x 64 B + 4 multiexps x n x 128 B (list in bench.py)",
                         "dominant_kernels": "ntt_pass (the resizes to the extended domains) and msm_bucket_acc (the three non-zero parts' commitments)"}}


def gate_argument_leg(np, log_n=20, n_gates=32, n_wit=24, steps=3, verify=True):
    """The gate argument of a circuit with many gates (gates_argument.hpp:93-121, 203-216): 32 gates = 96 products of 3 - 5 factors
    (selector included) over 56 columns and ~100 distinct (column, rotation) pairs, 2^20 rows, the 8 n-point extended domain, masked --
    evaluated as ONE launch over a flat program (zkhip_gate_eval_dev) and, beside it, as round 5's two launches per product.  Both
    figures include the extensions of the 24 witness columns (the selectors' and the mask's are cached: preprocessed)."""
    import ctypes

    lib = _bench_lib()
    ms = np.zeros(2 * steps, dtype=np.float64)
    info = np.zeros(4, dtype=np.float64)
    verified = ctypes.c_int(-1)
    rc = lib.zkhip_bench_gate_argument(0, ctypes.c_size_t(log_n), ctypes.c_size_t(n_gates), ctypes.c_size_t(n_wit), steps, ms.ctypes.data_as(ctypes.c_void_p),
                                       info.ctypes.data_as(ctypes.c_void_p), ctypes.byref(verified) if verify else None)
    if rc != 0:
        return {"error": rc}
    m = ms.reshape(steps, 2)
    t = m[1:] if steps > 1 else m
    fused, per_term = float(t[:, 0].mean()), float(t[:, 1].mean())
    ext = 8 << log_n
    # algorithmic bytes of the fused pass: every distinct column's extension read once + F written once (SURVEY 8d's convention)
    alg = (int(info[1]) + 1 + 1) * ext * 32
    ach = alg / (float(info[3]) * 1e-3) / 1e9 if info[3] > 0 else 0.0
    return {"metric": "placeholder gate argument, %d gates / %d products over %d columns, 2^%d rows, 8 n extended domain" % (n_gates, int(info[0]), int(info[1]), log_n),
            "value": round(fused, 3), "unit": "ms per gate argument", "per_term_ms": round(per_term, 3), "speedup_vs_per_term": round(per_term / fused, 2),
            "gate_eval_kernel_ms": round(float(info[3]), 3), "products": int(info[0]), "distinct_columns": int(info[1]), "distinct_column_rotation_pairs": int(info[2]),
            "ms_per_run": {"fused": [round(float(x), 2) for x in m[:, 0]], "per_term": [round(float(x), 2) for x in m[:, 1]]},
            "verified": None if not verify else bool(verified.value == 1),
            "verification": "fused == per-term bit for bit; F(y) == mask(y) sum sel(y) sum c prod col(omega^rot y) at a random y from coefficient forms",
            "roofline": {"bound": "hbm", "kernel": "gate_eval", "achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 5),
                         "traffic": None, "algorithmic_bytes": alg,
                         "honest_bound": "VALU: one Montgomery product per factor and row (no per-factor lift), %d products x ~3.5 factors x 8 n rows; by PMC "
                                         "(profiles/r06_pmc_gate.json, not re-measured in this run) 0.95 of the VALU issue capacity, 60.9 GB of HBM traffic per launch" % int(info[0])},
            "what": "both figures include the witness columns' extensions to 8 n (one per distinct COLUMN fused, one per distinct (column, rotation) pair per-term)"}


def permutation_leg(np, log_n=20, k=4, steps=6, verify=True):
    """placeholder's permutation argument, prover side, at BASELINE config 5's row count (hip/placeholder_permutation.hpp mirrors
    permutation_argument.hpp:70-224): k permuted columns resident; the grand product V_P (one inversion per ROW in a serial loop in the
    reference; prefix / suffix product scans and ONE inversion per call here) and the three constraint polynomials; the preprocessed
    polynomials (S_id, S_sigma, the selectors) keep their extensions across proofs (device_polynomial_dfs::enable_extension_cache)."""
    import ctypes

    lib = _bench_lib()
    ms = np.zeros(2 * steps, dtype=np.float64)
    verified = ctypes.c_int(-1)
    rc = lib.zkhip_bench_permutation(0, ctypes.c_size_t(log_n), ctypes.c_size_t(k), steps, ms.ctypes.data_as(ctypes.c_void_p), ctypes.byref(verified) if verify else None)
    if rc != 0:
        return {"error": rc}
    ms = ms.reshape(steps, 2)
    timed = ms[2:] if steps > 2 else ms    # the first two runs warm the transforms' tables and the context's block cache
    gp, whole = (float(x) for x in np.median(timed, axis=0))
    n = 1 << log_n
    # the grand product reads 3 k vectors and writes 2 k + 1: 32 B per element each
    alg_gp = (5 * k + 1) * n * 32
    ach = alg_gp / (gp * 1e-3) / 1e9
    return {"metric": "placeholder permutation argument (prover side), BLS12-381, %d permuted columns x 2^%d rows, resident" % (k, log_n),
            "value": round(whole, 3), "unit": "ms per prove_eval", "higher_is_better": False, "statistic": "median of the runs after the first two",
            "ms_grand_product": round(gp, 3), "ms_per_run": [round(float(x), 2) for x in ms[:, 1]],
            "verified": None if not verify else bool(verified.value == 1),
            "verification": "V_P[0] = 1 and the recurrence at 64 sampled rows; F_1(y) against its definition at a random y",
            "roofline": {"bound": "hbm", "kernel": "perm_grand_product (gp_rows: coalesced row products; gp_local / gp_top: prefix + suffix product scans and the call's ONE "
                                                   "inversion; gp_apply)", "achieved": round(ach, 2),
                         "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 6), "traffic": None, "algorithmic_bytes": alg_gp,
                         "per": "the grand product alone: 3 k input vectors read, 2 k + 1 written, 32 B per element"}}


def lookup_leg(np, log_n=20, k_in=2, k_val=1, steps=6, verify=True):
    """placeholder's lookup argument, prover side, at BASELINE config 5's row count (hip/placeholder_lookup.hpp mirrors lookup_argument.hpp:153-296):
    a genuine instance -- k_in inputs drawn from k_val table columns --, resident; sort_polynomials ON THE DEVICE (zkhip_lookup_sort_dev; the
    reference: an unordered_map count + one serial walk, :565-638), V_L (compute_V_L: one inversion per ROW in a serial loop in the reference;
    the permutation argument's scan here) and the four constraint polynomials."""
    import ctypes

    lib = _bench_lib()
    ms = np.zeros(3 * steps, dtype=np.float64)
    verified = ctypes.c_int(-1)
    rc = lib.zkhip_bench_lookup(0, ctypes.c_size_t(log_n), ctypes.c_size_t(k_in), ctypes.c_size_t(k_val), steps, ms.ctypes.data_as(ctypes.c_void_p),
                                ctypes.byref(verified) if verify else None)
    if rc != 0:
        return {"error": rc}
    ms = ms.reshape(steps, 3)
    timed = ms[2:] if steps > 2 else ms    # the first two runs warm the transforms' tables and the context's block cache
    srt, gp, whole = (float(x) for x in np.median(timed, axis=0))
    n = 1 << log_n
    # V_L reads the k_in + k_val + (k_in + k_val) reduced vectors and writes one: 32 B per element each
    alg_gp = (2 * (k_in + k_val) + 1) * n * 32
    ach = alg_gp / (gp * 1e-3) / 1e9
    # sort_polynomials reads k_in + k_val vectors and writes as many
    alg_sort = 2 * (k_in + k_val) * n * 32
    return {"metric": "placeholder lookup argument (prover side, sort_polynomials included), BLS12-381, %d inputs over %d table columns x 2^%d rows, resident"
                      % (k_in, k_val, log_n),
            "value": round(whole, 3), "unit": "ms per prove_eval", "higher_is_better": False, "statistic": "median of the runs after the first two",
            "ms_sort_polynomials": round(srt, 3), "ms_grand_product": round(gp, 3), "ms_per_run": [round(float(x), 2) for x in ms[:, 2]],
            "sort_polynomials_gbs": round(alg_sort / (srt * 1e-3) / 1e9, 1),
            "verified": None if not verify else bool(verified.value == 1),
            "verification": "the device's sorted vectors == the host's construction of them, entry by entry, no status flag; V_L[0] = 1, V_L[usable_rows] = 1 "
                            "(the product over all rows closes: the reference's own check, lookup_argument.hpp:217), zeros behind, "
                            "the recurrence at 64 sampled rows; F_2(y) against its definition at a random y",
            "roofline": {"bound": "hbm", "kernel": "perm_grand_product (gp_rows, gp_local, gp_top, gp_apply: one inversion per call)", "achieved": round(ach, 2),
                         "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 6), "traffic": None, "algorithmic_bytes": alg_gp,
                         "per": "V_L alone: 2 (k_in + k_val) input vectors read, 1 written, 32 B per element"}}


def placeholder_round_leg(np, log_n=20, steps=5, verify=True, witness_cols=50):
    """BASELINE config 5's proof shape on the device, the pieces composed as placeholder_prover::process strings them (prover.hpp:130-142, 170-218,
    262-277, 220-259, 314-317, 363-410) over genuine instances, every polynomial resident from the table to the opening proof:
    commit(VARIABLE_VALUES_BATCH) of 50 witness columns, the permutation argument (4 columns), the lookup argument (2 inputs over 1 table), a gate
    argument, the quotient of their eight constraint polynomials, its split into 8 parts, the commitments of V_P, V_L, the sorted vectors and the
    quotient parts (13 more MSMs of 2^20), and the opening proof of all four batches.  `round_ms` = everything between the witness commit and the
    opening proof."""
    import ctypes

    lib = _bench_lib()
    ms = np.zeros(9 * steps, dtype=np.float64)
    verified = ctypes.c_int(-1)
    rc = lib.zkhip_bench_placeholder_round(0, ctypes.c_size_t(log_n), ctypes.c_size_t(witness_cols), steps, ms.ctypes.data_as(ctypes.c_void_p),
                                           ctypes.byref(verified) if verify else None)
    if rc != 0:
        return {"error": rc}
    ms = ms.reshape(steps, 9)
    timed = ms[2:] if steps > 2 else ms    # the first two runs warm the transforms' tables and the context's block cache
    names = ["witness_commit", "permutation_argument", "lookup_argument_with_lookup_batch_commit", "permutation_batch_commit", "gate_argument",
             "quotient_polynomial", "split", "quotient_batch_commit", "proof_eval"]
    return {"metric": "placeholder-shaped proof, device side, BLS12-381, 2^%d rows x %d witness columns: witness commit + permutation (4 columns) + lookup (2 inputs, "
                      "1 table) + gate arguments + quotient of 8 parts split in 8 + 13 more commitments + the opening proof; resident" % (log_n, witness_cols),
            "value": round(float(np.median(timed.sum(axis=1))), 3), "unit": "ms per proof", "higher_is_better": False,
            "statistic": "median of the runs after the first two",
            "round_ms": round(float(np.median(timed[:, 1:8].sum(axis=1))), 3),
            "ms_by_phase": {k: round(float(v), 3) for k, v in zip(names, np.median(timed, axis=0))},
            "ms_per_run": [round(float(x), 2) for x in ms.sum(axis=1)],
            "verified": None if not verify else bool(verified.value == 1),
            "verification": "V_P[usable] = V_L[usable] = 1 (both grand products close over 2^20 rows), the division by X^n - 1 is exact, "
                            "T(y)(y^n - 1) = sum_i alpha_i F_i(y) at a random y (the commitments and the opening proof are what the `kzg` leg verifies)"}


def ntt_sharded_leg(np, torch, dist, zk, ctx, rank, world, local_rank, log_m=22, batch=8, steps=5, verify=True):
    """BASELINE config 3 over N GPUs (north_star: "independent polynomial NTT batches shard across the 8 GPUs"): the 8
    polynomials of 2^22 are dealt round-robin over the ranks (dist.shard_polys); every rank transforms its own polynomials in place --
    NO collective in the data path --; the timed region is bracketed by barriers and the slowest rank counts (strong scaling: the
    job is fixed).  Every rank checks its own outputs at sampled indices against the block-Horner evaluation of its inputs and the
    verdicts are gathered."""
    from crypto3_zk_amd import dist as zd

    r = R_BLS
    w = pow(7, (r - 1) >> log_m, r)
    omega = lim(np, w)
    m = 1 << log_m
    mine = zd.shard_polys(batch, rank, world)
    cnt = len(mine)
    dev = f"cuda:{local_rank}"
    data = np.concatenate([random_scalars(np, m, 300 + c) for c in mine]) if cnt else np.zeros((0, 4), dtype=np.uint64)
    d = ctx.malloc(max(1, cnt) * m * 32)
    ok = True
    if cnt:
        ctx.h2d(d, data)
        if verify:
            idx = [0, 1, m // 2 + 3, m - 1, 123457 % m, (7 * m) // 9]
            pts = np.stack([lim(np, pow(w, i, r)) for i in idx])
            want = ctx.poly_eval_dev(zk.BLS12_381, d, m, cnt, pts)
            ctx.ntt_dev(zk.BLS12_381, d, log_m, cnt, omega)
            got = np.zeros((cnt, m, 4), dtype=np.uint64)
            ctx.d2h(got, d)
            ok = bool(all((got[b, i] == want[b, k]).all() for b in range(cnt) for k, i in enumerate(idx)))
        else:
            ctx.ntt_dev(zk.BLS12_381, d, log_m, cnt, omega)
        ctx.ntt_dev(zk.BLS12_381, d, log_m, cnt, omega)
    times = []
    for _ in range(steps + 1):
        dist.barrier(device_ids=[local_rank])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if cnt:
            ctx.ntt_dev(zk.BLS12_381, d, log_m, cnt, omega)
            ctx.sync()
        dist.barrier(device_ids=[local_rank])
        torch.cuda.synchronize()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        times.append(float(t.item()) * 1e3)
    ctx.free(d)
    verified = None
    if verify:
        parts = [None] * world
        dist.all_gather_object(parts, bool(ok))
        verified = bool(all(parts))
    mean = sum(times[1:]) / len(times[1:])
    return {"metric": "NTT elements/sec, BLS12-381 Fr, 2^%d x %d dealt over %d GPU(s)" % (log_m, batch, world),
            "value": round(batch * m / mean / 1e3, 2), "unit": "Melements/s", "scaling": "strong", "statistic": "mean of the transforms after the first, slowest rank",
            "ms_per_transform_batch": [round(t, 3) for t in times], "polynomials_per_rank": (batch + world - 1) // world,
            "exchange": "none: the polynomials are independent (SURVEY 8e); two barriers bracket the timed region", "verified": verified}


def kzg_sharded_leg(np, torch, dist, zk, ctx, rank, world, local_rank, log_n=20, cols=50, steps=2, verify=True):
    """BASELINE config 5's commitment leg over N GPUs: the 50 columns are dealt round-robin over the ranks
    (dist.shard_polys), every rank holds the whole SRS, commits its own columns (one batched inverse NTT + one MSM batch, no
    collective) and ONE all-gather of the 144-byte commitments follows.  Weak in nothing: the job is fixed, `value` = 50 columns /
    the slowest rank's time (strong scaling).  Checked on rank 0: every gathered commitment == f_c(alpha) G, f_c(alpha) evaluated by
    the rank that owns column c."""
    from crypto3_zk_amd import dist as zd

    n = 1 << log_n
    r, alpha = R_BLS, 7
    omega = lim(np, pow(7, (r - 1) >> log_n, r))
    x, pw = 1, np.empty((n, 4), dtype=np.uint64)
    for i in range(n):
        pw[i, 0], pw[i, 1], pw[i, 2], pw[i, 3] = x & MASK64, (x >> 64) & MASK64, (x >> 128) & MASK64, x >> 192
        x = x * alpha % r
    srs = ctx.bases_from_scalars(zk.BLS12_381, zk.G1, pw)
    mine = zd.shard_polys(cols, rank, world)
    cnt, slots = len(mine), (cols + world - 1) // world
    dev = f"cuda:{local_rank}"
    data = np.stack([random_scalars(np, n, 500 + c) for c in mine]) if cnt else np.zeros((0, n, 4), dtype=np.uint64)
    d = ctx.malloc(max(1, cnt) * n * 32)
    d_out = torch.zeros(slots * 18, dtype=torch.int64, device=dev)  # this rank's commitments (Jacobian, 144 B each), padded to `slots`
    gathered = torch.zeros(world * slots * 18, dtype=torch.int64, device=dev)
    times = []
    for _ in range(steps + 1):
        if cnt:
            ctx.h2d(d, data)
        dist.barrier(device_ids=[local_rank])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if cnt:
            ctx.ntt_dev(zk.BLS12_381, d, log_n, cnt, omega, inverse=True)
            ctx.msm_batch_dev([srs] * cnt, [d + 32 * n * j for j in range(cnt)], [d_out.data_ptr() + 144 * j for j in range(cnt)], ns=[n] * cnt)
        dist.all_gather_into_tensor(gathered, d_out)  # RCCL; the context runs on torch's current stream: ordered after the commits
        dist.barrier(device_ids=[local_rank])
        torch.cuda.synchronize()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        times.append(float(t.item()) * 1e3)
    verified = None
    if verify:
        ev = ctx.poly_eval_dev(zk.BLS12_381, d, n, cnt, lim(np, alpha).reshape(1, 4)) if cnt else np.zeros((0, 1, 4), dtype=np.uint64)
        parts = [None] * world
        dist.all_gather_object(parts, {c: to_ints(ev[j])[0] for j, c in enumerate(mine)})
        if rank == 0:
            fa = {c: v for part in parts for c, v in part.items()}
            got = gathered.cpu().numpy().view(np.uint64).reshape(world, slots, 3, 6)
            ok = len(fa) == cols
            for c in range(cols):
                p, inf = ctx.jacobian_to_affine(zk.BLS12_381, zk.G1, got[c % world, c // world])
                eb = ctx.bases_from_scalars(zk.BLS12_381, zk.G1, lim(np, fa[c] % r).reshape(1, 4))
                exp, exp_inf = eb.download()
                eb.free()
                ok = ok and int(exp_inf[0]) == inf and bool((exp[0] == p).all())
            verified = bool(ok)
    ctx.free(d)
    srs.free()
    mean = sum(times[1:]) / len(times[1:])
    return {"metric": "KZG commit columns/sec, BLS12-381, %d columns x 2^%d rows dealt over %d GPU(s)" % (cols, log_n, world),
            "value": round(cols / mean * 1e3, 2), "unit": "columns/s", "scaling": "strong", "statistic": "mean of the commits after the first, slowest rank",
            "ms_per_commit": [round(t, 2) for t in times], "columns_per_rank": slots,
            "exchange": "one RCCL all-gather of %d B per rank per commit (the commitments); SRS replicated, no collective in the transforms or the multiexps" % (slots * 144),
            "verified": verified}


CPU_GROTH16_LOG = 20  # --cpu-groth16-log: size of the CPU prover sample next to the 2^17 one (20 = the headline instance)


def cpu_baseline(np, bases, scalars, gpu_affine, zk=None, ctx=None, others=None):
    """The oracle's BDLO12 Pippenger (the CPU restatement of algebra::multiexp with chunks = #threads, as prover.hpp:94-99)
    timed on this host on bounded samples of the same workloads: the headline's OWN 2^20 points and scalars on
    the best thread count of a short sweep (the headline `value`; its result is held against the GPU's: `gpu_result_equals_oracle`),
    on ONE thread at 2^18 of them; the radix-2 NTT on all 8 polynomials of config 3; ONE Groth16 proof at the headline's 2^20
    constraints.  Bounded to about half a minute of CPU work in total (VERDICT r4 #8d).  Reported, not a target."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import cport as cp

    omp = cp.omp_default_threads()
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = os.cpu_count() or omp
    cores = max(1, min(omp, usable))  # threads beyond the CPUs this process may run on only add contention
    cp.set_threads(cores)
    sample = bases.n
    lg = sample.bit_length() - 1
    pts, inf = bases.download(0, sample)
    hb = cp.Bases(0, 1, pts, inf)
    sc = np.ascontiguousarray(scalars[:sample])
    hb.msm(sc[: 1 << 16], chunks=cores)  # spin the thread pool up

    def timed_msm(threads, min_s, count=sample):
        cp.set_threads(threads)
        reps, t0 = 0, time.perf_counter()
        while reps < 1 or time.perf_counter() - t0 < min_s:
            res = hb.msm(sc[:count], chunks=threads, n=count)
            reps += 1
        dt = time.perf_counter() - t0
        return reps * count / dt / 1e6, reps, dt, res

    # more threads than the host can keep busy at once (a CPU quota, two hyper-threads per core, two sockets' worth of memory
    # traffic) make this MSM SLOWER, so the headline is the best count of a short sweep, and the sweep stays in the detail file
    sweep = {}
    for th in sorted({cores, min(cores, 32), min(cores, 8)}, reverse=True):
        sweep[th] = timed_msm(th, 1.0)[0]
    best = max(sweep, key=sweep.get)
    v_all, reps, dt, res = timed_msm(best, 3.0)
    same = bool(res[1] == gpu_affine[1] and (res[0] == gpu_affine[0]).all())
    quota = None
    try:
        q = open("/sys/fs/cgroup/cpu.max").read().split()
        quota = None if q[0] == "max" else round(int(q[0]) / int(q[1]), 1)
    except Exception:
        pass
    out = {"value": round(v_all, 5), "unit": "Mpoints/s", "cores": best, "kind": "port", "gpu_result_equals_oracle": same,
           "host": {"omp_max_threads": omp, "usable_cpus": usable, "cpu_count": os.cpu_count(), "cgroup_cpu_quota": quota},
           "sample": "%d MSMs over the headline's 2^%d points and scalars, chunks = %d threads (best of %s), %.1f s" % (reps, lg, best, sorted(sweep), dt)}
    one_lg = min(lg, 18)
    v_one, _, dt1, _ = timed_msm(1, 0.0, 1 << one_lg)  # ONE thread, a quarter of the points (the window the oracle picks barely moves: 2.6 s instead of 10.5)
    out["one_thread"] = {"value": round(v_one, 5), "unit": "Mpoints/s", "cores": 1, "sample": "one MSM over the first 2^%d of the points, %.1f s" % (one_lg, dt1)}
    sweep[best] = max(sweep[best], v_all)
    out["thread_scaling"] = {"Mpoints_per_s_by_threads": {str(k): round(v, 4) for k, v in sorted(sweep.items())},
                             "note": "chunks = threads cuts the MSM into n / threads points per thread (prover.hpp:94-99): every chunk runs its own bucket "
                                     "method with a smaller window, and beyond the host's physical parallelism more threads only contend"}
    cp.set_threads(cores)
    # NTT: config 3 in full -- 8 polynomials of 2^22, the oracle's transform parallel over the batch
    r = R_BLS
    a = random_scalars(np, 8 << 22, 78).reshape(8, 1 << 22, 4)
    ntt_threads = best  # the thread count the MSM sweep found this host can keep busy (more only contend)
    cp.set_threads(ntt_threads)
    t0 = time.perf_counter()
    cp.ntt(0, a, 22, lim(np, pow(7, (r - 1) >> 22, r)))
    dtn = time.perf_counter() - t0
    cp.set_threads(cores)
    inside = 16 <= ntt_threads  # cport.ntt puts the threads INSIDE each transform when the batch is smaller than half of them
    out["ntt"] = {"value": round((8 << 22) / dtn / 1e6, 3), "unit": "Melements/s", "cores": ntt_threads if inside else min(8, ntt_threads),
                  "sample": ("all 8 polynomials of 2^22 (config 3), one after the other with %d threads inside each transform, %.1f s" % (ntt_threads, dtn)) if inside
                            else "all 8 polynomials of 2^22 (config 3), one thread per polynomial (%d of %d usable threads busy), %.1f s" % (min(8, ntt_threads), cores, dtn)}
    del a
    # the other (curve, group) MSM legs: a 2^16-point prefix of their inputs through the oracle's Pippenger against the GPU's MSM of the same prefix
    if others and "lpc" in others:
        # the LPC commit leg: the oracle's extension of the SAME 16 x 2^20 polynomials to D[0] = 2^21 and its coset-ordered leaf layout
        # (cport.fri_leaves = basic_fri.hpp:456-492), folded like the tree builders of the leg fold theirs
        leg = others.pop("lpc")
        lg, cols = leg["_shape"]
        t0 = time.perf_counter()
        with np.errstate(over="ignore"):
            k = np.arange(1, cols * (4 << lg) + 1, dtype=np.uint64)
            z = np.uint64(5) + k * np.uint64(0x9E3779B97F4A7C15)   # the bench library's splitmix (seed 5), word by word
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
        w = z.reshape(cols, 1 << lg, 4)
        w[:, :, 3] &= np.uint64(0x0FFFFFFFFFFFFFFF)
        del k, z
        coeffs = cp.ntt(0, w, lg, lim(np, pow(7, (R_BLS - 1) >> lg, R_BLS)), inverse=True)
        ext = np.zeros((cols, 2 << lg, 4), dtype=np.uint64)
        ext[:, : 1 << lg] = coeffs
        del coeffs, w
        ext = cp.ntt(0, ext, lg + 1, lim(np, pow(7, (R_BLS - 1) >> (lg + 1), R_BLS)))
        flat = cp.fri_leaves(list(ext), 1).reshape(-1)
        del ext
        with np.errstate(over="ignore"):
            fold = int((np.arange(1, flat.size + 1, dtype=np.uint64) * flat).sum(dtype=np.uint64))
        del flat
        okl = fold == leg["_fold"]
        leg["verified"] = bool(leg.get("verified") and okl)
        leg["verification"] += "; == the same fold over the ORACLE's leaves (cport: extension of the same %d x 2^%d polynomials to 2^%d, fri_leaves), %.1f s" % (
            cols, lg, lg + 1, time.perf_counter() - t0)
    if others and zk is not None and ctx is not None:
        for name, leg in others.items():
            ob, _, osc = leg["_inputs"]
            cnt = min(ob.n, 1 << 16)
            opts, oinf = ob.download(0, cnt)
            exp, einf = cp.msm(ob.curve, ob.group, opts, np.ascontiguousarray(osc[:cnt]), chunks=cores)
            got, ginf = ctx.msm_affine(ob, np.ascontiguousarray(osc[:cnt]), 0, cnt)
            okp = bool(einf == ginf and (exp == got).all())
            leg["verified"] = bool(leg.get("verified") and okp)
            leg["verified_vs"] = str(leg.get("verified_vs")) + "; oracle (cport) MSM of the first 2^%d points, affine, bit-exact" % (cnt.bit_length() - 1)
    # Groth16 AT THE SIZE OF THE HEADLINE METRIC (2^20 constraints, over the domain the reference reduces over): the oracle generates its
    # own valid key from a fixed trapdoor (outside the timing) and ONE proof is timed on the best thread count of the MSM sweep
    def cpu_proof(log_m):
        Mg, ng = 1 << log_m, 10
        g = cp.Groth16(0, Mg, ng, seed=1)
        kind, m = cp.domain_choice(Mg + ng + 1, 32)
        wq = lim(np, pow(7, (r - 1) >> ((Mg + ng).bit_length()), r))
        g.set_domain(kind, m, wq)
        cp.set_threads(cores)
        tk = time.perf_counter()
        g.keygen(random_scalars(np, 5, 79), wq)
        tk = time.perf_counter() - tk
        cp.set_threads(best)
        t0 = time.perf_counter()
        g.prove(lim(np, 5), lim(np, 6), wq, lim(np, 7), chunks=best)
        dtg = time.perf_counter() - t0
        return {"value": round(Mg / dtg, 1), "unit": "constraints/s", "cores": best, "constraints": Mg, "seconds_per_proof": round(dtg, 2),
                "keygen_seconds_untimed": round(tk, 1),
                "sample": "one proof at 2^%d constraints, domain of %d points (make_evaluation_domain's choice), chunks = %d threads, %.1f s; "
                          "the oracle's own key generation took %.1f s on %d threads (not timed as proving)" % (log_m, m, best, dtg, tk, cores)}
    out["groth16"] = cpu_proof(CPU_GROTH16_LOG)
    return out


if __name__ == "__main__":
    main()
