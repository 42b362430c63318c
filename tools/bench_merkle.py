#!/usr/bin/env python3
"""The device Merkle builder at size (run on the GPU box): for 16 x 2^20 -> domain 2^21 at fri_step 1 (the headline LPC commit) and for
1 x 2^21 (a FRI round's tree)
  * the LPC commit through the shim class with the device tree builder (hip/merkle.hpp: SHA2-256 on the GPU, nothing over PCIe but the root);
  * the same commit with the streaming host builder that only touches every leaf element (what the project's LPC figures were taken with:
    the leaves cross PCIe and NOTHING is hashed);
  * the fused leaf kernel and the level chain on their own, from the per-kernel HIP events (zkhip_profile_get), with the leaf kernel's rate
    in compressions/s.
Writes profiles/merkle_bench.json.   python3 tools/bench_merkle.py [--steps 6] [--out profiles/merkle_bench.json]"""
import argparse
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_pkg():
    pkg_dir = os.path.join(ROOT, "crypto3-zk_amd")
    spec = importlib.util.spec_from_file_location("crypto3_zk_amd", os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["crypto3_zk_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def median(v):
    return float(np.median(np.asarray(v)))


def commits(bench, log_n, cols, steps):
    """commit wall times through lpc_commitment_scheme_hip: device builder, then the streaming touch-only builder"""
    ms_dev, ms_host = (ctypes.c_double * steps)(), (ctypes.c_double * steps)()
    root, fold = (ctypes.c_uint8 * 32)(), ctypes.c_uint64()
    assert bench.zkhip_bench_lpc_scheme_device(0, ctypes.c_size_t(log_n), ctypes.c_size_t(cols), ctypes.c_size_t(1), steps, ms_dev, root) == 0
    assert bench.zkhip_bench_lpc_scheme(0, ctypes.c_size_t(log_n), ctypes.c_size_t(cols), ctypes.c_size_t(1), steps, 1, 8, ms_host, ctypes.byref(fold)) == 0
    return {"device_builder_ms": list(ms_dev), "device_builder_ms_median_warm": median(list(ms_dev)[1:]),
            "streaming_no_hash_ms": list(ms_host), "streaming_no_hash_ms_median_warm": median(list(ms_host)[1:]), "root": bytes(root).hex()}


def kernels(ctx, log_domain, batch, fri_step, steps):
    """per-kernel device times of zkhip_merkle_build_fri_dev over resident evaluations (random limbs: the hash does not care)"""
    n = batch << log_domain
    rng = np.random.default_rng(5)
    d = ctx.malloc(n * 32)
    ctx.h2d(d, rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64))
    ctx.merkle_build_fri(d, log_domain, batch, fri_step).free()  # warm: allocation, code load
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(steps):
        ctx.merkle_build_fri(d, log_domain, batch, fri_step).free()
    leaf_ms, leaf_n = ctx.profile_get("merkle_fri_leaf_hash")
    level_ms, level_n = ctx.profile_get("merkle_level_hash")
    ctx.profile(False)
    ctx.free(d)
    leaves = 1 << (log_domain - fri_step)
    blocks = leaves * ((batch << fri_step) // 2 + 1)  # compressions of the leaf kernel: one per pair of elements, one of padding
    leaf = leaf_ms / leaf_n
    return {"leaves": leaves, "leaf_bytes": (batch << fri_step) * 32, "leaf_kernel_ms": leaf, "leaf_kernel_compressions": blocks,
            "leaf_kernel_compressions_per_s": blocks / (leaf * 1e-3), "leaf_kernel_input_GBps": n * 32 / (leaf * 1e-3) / 1e9,
            "level_chain_ms": level_ms / steps, "level_chain_launches": level_n // steps,
            "level_chain_compressions": 2 * (leaves - 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle_bench.json"))
    args = ap.parse_args()
    zk = load_pkg()
    bench = ctypes.CDLL(os.path.join(ROOT, "crypto3-zk_amd", "libzkhip_bench.so"))
    ctx = zk.Context(0)
    res = {"what": "SHA2-256 Merkle trees on the device: LPC commit with the device builder vs the streaming builder that ships the leaves and hashes nothing",
           "fri_step": 1, "steps": args.steps, "cases": {}}
    for name, cols in (("16x2^20->2^21", 16), ("1x2^20->2^21 (a FRI round's tree)", 1)):
        case = {"commit": commits(bench, 20, cols, args.steps), "kernels": kernels(ctx, 21, cols, 1, args.steps)}
        res["cases"][name] = case
        print(name, json.dumps(case), flush=True)
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
