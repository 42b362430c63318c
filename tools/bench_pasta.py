#!/usr/bin/env python3
"""Pallas and Vesta next to the curves whose limb counts they share (run on the GPU box): writes profiles/pasta_bench.json.
  * the G1 MSM over 2^20 resident points (device-generated, window tables): Pallas and Vesta next to BN254 (all three: 10-limb coordinates),
    wall time of zkhip_msm_dev + sync around HIP events of the whole call, and the per-kernel event sums;
  * the NTT at 2^22 x 8 over F_p (id 3) and F_q (id 2) next to BLS12-381 Fr (all three: 9 limbs);
  * the device side of an LPC commit of 16 x 2^20 -> domain 2^21 at fri_step 1 with the device tree builder -- zkhip_poly_resize_dev, then
    zkhip_merkle_build_fri_dev -- over F_p next to BLS12-381 Fr (the hash is the same; the extension is the field's).
Every figure: warm-up first, then `--runs` timed runs of the per-kernel HIP events (zkhip_profile_get, the method of tools/bench_pow.py);
median, min and max.  The counterparts run in the same process, interleaved run by run, so that clock and box are shared.
python3 tools/bench_pasta.py [--runs 10] [--out profiles/pasta_bench.json] [--log-n 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
P = 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001
Q = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001
BLS_R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
NAMES = {0: "bls12_381", 1: "bn254", 2: "pallas", 3: "vesta"}
FR = {0: (BLS_R, 7), 2: (Q, 5), 3: (P, 5)}  # scalar field and its multiplicative generator


def spread(v):
    v = sorted(float(x) for x in v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}


def limbs(v):
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def root(curve, log_m):
    r, g = FR[curve]
    return limbs(pow(g, (r - 1) >> log_m, r))


def random_scalars(seed, n):
    """below 2^252: canonical in every scalar field here"""
    a = np.random.default_rng(seed).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(11)
    return a


def timed(ctx, runs, subjects, prefixes):
    """subjects: {name: callable}; run them interleaved, `runs` times after one warm-up each; per run the event sum of every kernel (prefix "")
    and of the listed prefixes, and before that the host's wall time per call"""
    for fn in subjects.values():
        fn()
    ctx.sync()
    out = {k: {"total_ms": [], "wall_ms": [], **{p: [] for p in prefixes}} for k in subjects}
    for _ in range(runs):  # host wall time of the call and the stream's drain, profiler off (what a caller waits for: the kernels and the gaps between them)
        for k, fn in subjects.items():
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            out[k]["wall_ms"].append((time.perf_counter() - t0) * 1e3)
    ctx.profile(True)
    for _ in range(runs):
        for k, fn in subjects.items():
            ctx.profile_reset()
            fn()
            ctx.sync()
            out[k]["total_ms"].append(ctx.profile_get("")[0])
            for p in prefixes:
                out[k][p].append(ctx.profile_get(p)[0])
    ctx.profile(False)
    return {k: {name: spread(v) for name, v in d.items()} for k, d in out.items()}


def ratios(res, pairs):
    return {f"{a}_over_{b}": res[a]["total_ms"]["median"] / res[b]["total_ms"]["median"] for a, b in pairs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--log-n", type=int, default=20, help="log2 of the MSM's points and of the LPC rows; the NTT runs at 2^(log_n + 2) x 8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pasta_bench.json"))
    args = ap.parse_args()
    import bench_merkle

    zk = bench_merkle.load_pkg()
    ctx = zk.Context(0)
    n = 1 << args.log_n
    res = {"what": "Pallas / Vesta next to BN254 (MSM) and BLS12-381 Fr (NTT, LPC commit): per-kernel HIP event sums, ms", "log_n": args.log_n, "runs": args.runs}

    # ---- MSM over resident points
    d_s, d_o = ctx.malloc(n * 32), ctx.malloc(512)
    ctx.h2d(d_s, random_scalars(2, n))
    bases = {c: ctx.bases_from_scalars(c, zk.G1, random_scalars(1, n)) for c in (1, 2, 3)}
    subjects = {NAMES[c]: (lambda b=b: ctx.msm_dev(b, d_s, d_o)) for c, b in bases.items()}
    res["msm_g1"] = timed(ctx, args.runs, subjects, ["msm_digits", "msm_sort", "msm_bucket_acc", "msm_bucket_red", "msm_fold"])
    res["msm_g1"]["ratios"] = ratios(res["msm_g1"], [("pallas", "bn254"), ("vesta", "bn254")])
    print("msm_g1", json.dumps(res["msm_g1"]), flush=True)
    for b in bases.values():
        b.free()
    ctx.free(d_s)
    ctx.free(d_o)

    # ---- NTT
    log_m, batch = args.log_n + 2, 8
    d = ctx.malloc((batch << log_m) * 32)
    ctx.h2d(d, random_scalars(3, batch << log_m))
    subjects = {NAMES[c] + "_fr": (lambda c=c: ctx.ntt_dev(c, d, log_m, batch, root(c, log_m))) for c in (0, 3, 2)}
    res["ntt"] = {"log_m": log_m, "batch": batch, **timed(ctx, args.runs, subjects, [])}
    res["ntt"]["ratios"] = ratios(res["ntt"], [("vesta_fr", "bls12_381_fr"), ("pallas_fr", "bls12_381_fr")])
    print("ntt", json.dumps(res["ntt"]), flush=True)
    ctx.free(d)

    # ---- LPC commit, device side: extend 16 x 2^log_n to the 2^(log_n + 1)-point domain, hash the tree on the device
    cols, log_d = 16, args.log_n + 1
    d_in, d_ext = ctx.malloc((cols << args.log_n) * 32), ctx.malloc((cols << log_d) * 32)
    evals = random_scalars(4, cols << args.log_n)

    def commit(c):
        ctx.h2d(d_in, evals)  # the extension leaves coefficients behind: every run starts from the evaluations (the copy is not a kernel: not counted)
        ctx.poly_resize_dev(c, d_in, args.log_n, cols, root(c, args.log_n), d_ext, log_d, root(c, log_d))
        ctx.merkle_build_fri(d_ext, log_d, cols, 1).free()

    subjects = {NAMES[c] + "_fr": (lambda c=c: commit(c)) for c in (0, 3)}
    res["lpc_commit_device_side"] = {"cols": cols, "log_rows": args.log_n, "log_domain": log_d, **timed(ctx, args.runs, subjects, ["merkle", "ntt"])}
    res["lpc_commit_device_side"]["ratios"] = ratios(res["lpc_commit_device_side"], [("vesta_fr", "bls12_381_fr")])
    print("lpc_commit_device_side", json.dumps(res["lpc_commit_device_side"]), flush=True)
    ctx.free(d_in)
    ctx.free(d_ext)
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
