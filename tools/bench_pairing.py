#!/usr/bin/env python3
"""Inner pairing products on the device (run on the GPU box): writes profiles/pairing_bench.json.
  * one product (one term, one output) over resident structured keys P_i = a_i G1, Q_i = b_i G2 at n = 2^10, 2^14, 2^17; every output is
    first checked against the big-integer model's e(G1, G2)^(sum a_i b_i) (tests/pairing_ref.py), then timed warm: the Miller kernel and
    the product kernels from the per-kernel HIP events (zkhip_profile_get), the whole call from the host clock, median and spread;
  * the host final exponentiation alone (the same pairing.hpp body through libzkhip_hosttest.so), which every call pays once per output;
  * the yardstick: the same pairing.hpp Miller loop and products on ONE host thread (zkt_pairing_products over 64 of the pairs), which is
    how the reference runs an inner pairing product.
python3 tools/bench_pairing.py [--runs 7] [--out profiles/pairing_bench.json]"""
import argparse
import ctypes
import importlib.util
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pairing_ref as pr  # noqa: E402


def load_pkg():
    pkg_dir = os.path.join(ROOT, "crypto3-zk_amd")
    spec = importlib.util.spec_from_file_location("crypto3_zk_amd", os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["crypto3_zk_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def spread(v):
    v = sorted(float(x) for x in v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}


def fr_arr(vals):
    return np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def gt_ints(row):
    return [sum(int(x) << (64 * i) for i, x in enumerate(row[k * 6:(k + 1) * 6])) for k in range(12)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairing_bench.json"))
    args = ap.parse_args()
    zk = load_pkg()
    ctx = zk.Context(0)
    host = ctypes.CDLL(os.path.join(ROOT, "crypto3-zk_amd", "libzkhip_hosttest.so"))
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    res = {"what": "zkhip_pairing_products, one term and one output over resident structured keys: per-kernel HIP event sums and host wall "
                   "time of the whole call, ms, warm; every timed output equals the model's e(G1, G2)^(sum a_i b_i)", "sizes": {}}
    rnd = random.Random(2024)
    for log_n in (10, 14, 17):
        n = 1 << log_n
        a = [rnd.randrange(1, pr.R) for _ in range(n)]
        b = [rnd.randrange(1, pr.R) for _ in range(n)]
        p, q = ctx.bases_from_scalars(zk.BLS12_381, zk.G1, fr_arr(a)), ctx.bases_from_scalars(zk.BLS12_381, zk.G2, fr_arr(b))
        exp = pr.structured_expectation(sum(x * y for x, y in zip(a, b)) % pr.R)
        terms = [(p, 0, q, 0, n, 0)]
        assert gt_ints(ctx.pairing_products(terms, 1)[0]) == exp, f"n = 2^{log_n}: the product differs from the model"
        ctx.pairing_products(terms, 1)  # warm
        ctx.profile(True)
        mill, prod, wall = [], [], []
        for _ in range(args.runs):
            ctx.profile_reset()
            t0 = time.perf_counter()
            out = ctx.pairing_products(terms, 1)
            wall.append((time.perf_counter() - t0) * 1e3)
            mill.append(ctx.profile_get("pairing_miller")[0])
            prod.append(ctx.profile_get("pairing_product")[0])
            assert gt_ints(out[0]) == exp
        ctx.profile(False)
        m = spread(mill)
        res["sizes"][f"2^{log_n}"] = {"n": n, "miller_kernel_ms": m, "product_kernels_ms": spread(prod), "call_wall_ms": spread(wall),
                                      "pairs_per_s_miller_kernel": n / (m["median"] * 1e-3), "pairs_per_s_call": n / (spread(wall)["median"] * 1e-3)}
        if log_n == 10:  # the yardstick: one host thread over 64 of these pairs, and the final exponentiation alone
            (P1, _), (P2, _) = p.download(0, 64), q.download(0, 64)
            g1 = np.ascontiguousarray(P1).view(np.uint32).reshape(-1)
            g2 = np.ascontiguousarray(P2).view(np.uint32).reshape(-1)
            z = np.zeros(64, dtype=np.uint8)
            one = lambda v, dt: np.array([v], dtype=dt)
            out = np.zeros(144, dtype=np.uint32)
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                assert host.zkt_pairing_products(ptr(g1), ptr(z), ptr(g2), ptr(z), ptr(one(0, np.uint64)), ptr(one(64, np.uint64)), ptr(one(0, np.uint32)),
                                                 ctypes.c_size_t(1), ctypes.c_size_t(1), ptr(out)) == 0
                t.append((time.perf_counter() - t0) * 1e3)
            fe = []
            for _ in range(5):
                t0 = time.perf_counter()
                assert host.zkt_fq12_op(6, ptr(out), None, ptr(np.zeros(144, dtype=np.uint32))) == 0
                fe.append((time.perf_counter() - t0) * 1e3)
            res["host_final_exponentiation_ms"] = spread(fe)
            host_ms = spread(t)["median"] - spread(fe)["median"]
            res["one_host_thread"] = {"pairs": 64, "ms_with_final_exponentiation": spread(t), "pairs_per_s": 64 / (host_ms * 1e-3),
                                      "note": "the same pairing.hpp bodies compiled for the CPU at -O2; includes the conversion of the points"}
        p.free(), q.free()
    for k, v in res["sizes"].items():
        v["speedup_over_one_host_thread"] = v["pairs_per_s_call"] / res["one_host_thread"]["pairs_per_s"]
    ctx.close()
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
