#!/usr/bin/env python3
"""Groth16 batch verification on the device (run on the GPU box): writes profiles/groth16_verify_bench.json.
  * zkhip_groth16_verify_batch over n = 2^10, 2^13, 2^16 resident proofs of a synthetic key with 11 inputs (tests/groth16_verify_ref.py: keys
    and proofs from trapdoor scalars).  Every size is first checked: ok is 1 everywhere but at one spoiled proof, whose compared value equals
    the model's; then timed warm, the three kernels from the per-kernel HIP events (zkhip_profile_get), the whole call (with the upload of the
    inputs and the copy of ok) from the host clock, median and spread;
  * baseline (a), n = 2^10 only: the route there was before, zkhip_pairing_products with 3 n one-pair terms and n outputs, over -acc and -C
    made from the trapdoor scalars (so it is not even charged the accumulation); its final exponentiations run on the host;
  * baseline (b): one host thread running the host twin (zkt_groth16_verify), per proof from the difference of a 48-proof and a 16-proof
    call, which cancels the making of the key.
python3 tools/bench_groth16_verify.py [--runs 7] [--out profiles/groth16_verify_bench.json]"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import groth16_verify_ref as gr  # noqa: E402
from bench_pairing import fr_arr, gt_ints, load_pkg, spread  # noqa: E402

R = gr.R
L_INPUTS = 11
SPOILED = 5


def fq_limbs(v):
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groth16_verify_bench.json"))
    ap.add_argument("--sizes", default="10,13,16")
    args = ap.parse_args()
    logs = [int(x) for x in args.sizes.split(",")]
    zk = load_pkg()
    ctx = zk.Context(0)
    host = ctypes.CDLL(os.path.join(ROOT, "crypto3-zk_amd", "libzkhip_hosttest.so"))
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    BLS, G1, G2 = zk.BLS12_381, zk.G1, zk.G2

    key = gr.Key(2025, L_INPUTS)
    gamma, delta, ic = key.points()
    g2l = lambda q: np.array(fq_limbs(q[0][0]) + fq_limbs(q[0][1]) + fq_limbs(q[1][0]) + fq_limbs(q[1][1]), dtype=np.uint64)
    ab = np.array([l for v in key.alpha_beta() for l in fq_limbs(v)], dtype=np.uint64)
    abc = np.array([fq_limbs(p[0]) + fq_limbs(p[1]) for p in ic], dtype=np.uint64)
    t0 = time.perf_counter()
    vk = ctx.groth16_vk_upload(ab, g2l(gamma), g2l(delta), abc)
    res = {"what": "zkhip_groth16_verify_batch, 11 public inputs per proof: per-kernel HIP event sums and host wall time of the whole call, ms, warm; "
                   "before timing ok is 1 everywhere but at one spoiled proof, whose compared value equals the model's",
           "vk_upload_ms_11_inputs": (time.perf_counter() - t0) * 1e3, "sizes": {}}

    n_max = 1 << max(logs)
    rnd = random.Random(7)
    xs = [[rnd.randrange(R) for _ in range(L_INPUTS)] for _ in range(n_max)]
    sc = [key.prove(x) for x in xs]
    sc[SPOILED] = (sc[SPOILED][0], sc[SPOILED][1], (sc[SPOILED][2] + 1) % R)
    a, b, c = (ctx.bases_from_scalars(BLS, grp, fr_arr([s[k] for s in sc])) for k, grp in ((0, G1), (1, G2), (2, G1)))
    inputs = fr_arr([x for row in xs for x in row]).reshape(n_max, L_INPUTS, 4)
    exp_ok = np.ones(n_max, dtype=np.uint8)
    exp_ok[SPOILED] = 0
    exp_gt = key.expected_gt(sc[SPOILED], xs[SPOILED])
    assert exp_gt != key.alpha_beta()

    for log_n in logs:
        n = 1 << log_n
        ok, gt = ctx.groth16_verify(vk, a, b, c, inputs[:n], n=n, want_gt=True)
        assert (ok == exp_ok[:n]).all(), f"n = 2^{log_n}: a verdict differs"
        assert gt_ints(gt[SPOILED]) == exp_gt and gt_ints(gt[0]) == key.alpha_beta(), f"n = 2^{log_n}: a compared value differs from the model"
        ctx.groth16_verify(vk, a, b, c, inputs[:n], n=n)  # warm
        ctx.profile(True)
        acc, mill, fe, wall = [], [], [], []
        for _ in range(args.runs):
            ctx.profile_reset()
            t0 = time.perf_counter()
            ok = ctx.groth16_verify(vk, a, b, c, inputs[:n], n=n)
            wall.append((time.perf_counter() - t0) * 1e3)
            acc.append(ctx.profile_get("groth16_accumulate")[0])
            mill.append(ctx.profile_get("groth16_miller3")[0])
            fe.append(ctx.profile_get("groth16_final_exp")[0])
            assert (ok == exp_ok[:n]).all()
        ctx.profile(False)
        w = spread(wall)
        res["sizes"][f"2^{log_n}"] = {"n": n, "accumulate_kernel_ms": spread(acc), "miller3_kernel_ms": spread(mill), "final_exp_kernel_ms": spread(fe),
                                      "call_wall_ms": w, "proofs_per_s_call": n / (w["median"] * 1e-3)}

    # (a) the route there was: 3 n one-pair terms into n outputs, final exponentiations on the host
    n = 1 << 10
    if 10 in logs:
        nacc = ctx.bases_from_scalars(BLS, G1, fr_arr([(-key.s(x)) % R for x in xs[:n]]))
        negc = ctx.bases_from_scalars(BLS, G1, fr_arr([(-s[2]) % R for s in sc[:n]]))
        gam, dlt = ctx.bases_from_scalars(BLS, G2, fr_arr([key.gamma])), ctx.bases_from_scalars(BLS, G2, fr_arr([key.delta]))
        terms = [t for i in range(n) for t in ((a, i, b, i, 1, i), (nacc, i, gam, 0, 1, i), (negc, i, dlt, 0, 1, i))]
        out = ctx.pairing_products(terms, n)
        assert gt_ints(out[0]) == key.alpha_beta() and gt_ints(out[SPOILED]) == exp_gt and gt_ints(out[n - 1]) == key.alpha_beta()
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            ctx.pairing_products(terms, n)
            t.append((time.perf_counter() - t0) * 1e3)
        res["baseline_a_pairing_products_3n_terms"] = {"n": n, "call_wall_ms": spread(t), "proofs_per_s": n / (spread(t)["median"] * 1e-3),
                                                       "note": "-acc and -C from the trapdoor scalars: no accumulation charged; n final exponentiations on the host"}
        for x in (nacc, negc, gam, dlt):
            x.free()

    # (b) one host thread, the host twin
    def host_ms(k):
        (A, _), (B, _), (C, _) = a.download(0, k), b.download(0, k), c.download(0, k)
        u32 = lambda m: np.ascontiguousarray(m).view(np.uint32).reshape(-1)
        z = np.zeros(k, dtype=np.uint8)
        ok = np.zeros(k, dtype=np.uint8)
        inp = u32(inputs[:k])
        t0 = time.perf_counter()
        rc = host.zkt_groth16_verify(ptr(ab), ptr(g2l(gamma)), ptr(g2l(delta)), ptr(abc), None, ctypes.c_size_t(len(ic)), ptr(u32(A)), ptr(z), ptr(u32(B)), ptr(z),
                                     ptr(u32(C)), ptr(z), ctypes.c_size_t(k), ptr(inp), ctypes.c_size_t(L_INPUTS), ptr(ok), None, None)
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0 and (ok == exp_ok[:k]).all()
        return dt

    per = sorted((host_ms(48) - host_ms(16)) / 32 for _ in range(3))[1]
    res["baseline_b_one_host_thread"] = {"ms_per_proof": per, "proofs_per_s": 1e3 / per,
                                         "note": "the same groth16_verify.hpp / pairing.hpp bodies compiled for the CPU at -O2; (48 proofs - 16 proofs) / 32"}
    for k, v in res["sizes"].items():
        v["x_one_host_thread"] = v["proofs_per_s_call"] / res["baseline_b_one_host_thread"]["proofs_per_s"]
        if k == "2^10" and "baseline_a_pairing_products_3n_terms" in res:
            v["x_baseline_a"] = res["baseline_a_pairing_products_3n_terms"]["call_wall_ms"]["median"] / v["call_wall_ms"]["median"]
    for x in (a, b, c):
        x.free()
    vk.free()
    ctx.close()
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
