#!/usr/bin/env python3
"""FRI's proof of work on the device (run on the GPU box): writes profiles/pow_bench.json.
  * candidates/s of the grinding kernel: one launch over 2^28 offsets under a mask nothing in that range satisfies, from the per-kernel HIP
    events (zkhip_profile_get), median and spread over the timed runs;
  * the same rate of the reference's loop on ONE host thread (zkt_pow_grind_cpu over the same pow.hpp: the baseline), and the ratio;
  * the sanity bound: the Merkle leaf kernel's compressions/s measured in the same session -- a candidate is two compressions;
  * the latency of a whole zkhip_pow_grind call at masks of 16, 20 and 24 bits for chunk_log in {16, 20, 24}, over the same seeded states;
  * lpc proof_eval on the README's instance (16 x 2^20 -> domain 2^21) with the device tree builder and the SHA2-256 transcript: grinding
    off, 16-bit, 20-bit; and the long-standing proof_eval driver (streaming builder) of this tree and, with --parent-lib, of a build of the
    parent commit, each in a process of its own (the two libraries export the same names).
python3 tools/bench_pow.py [--runs 10] [--parent-lib DIR/libzkhip_bench.so] [--out profiles/pow_bench.json]"""
import argparse
import ctypes
import hashlib
import importlib.util
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
FULL = 0xFFFFFFFF


def st(i):
    return hashlib.sha256(b"zkhip-pow-bench-%d" % i).digest()


def spread(v):
    v = sorted(float(x) for x in v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}


def kernel_rate(ctx, runs):
    tries = 1 << 28
    i = 0
    while ctx.pow_grind(st(i), 0, FULL, max_tries=tries, chunk_log=28)[0] is not None:  # also the warm-up
        i += 1
    ctx.pow_grind(st(i), 0, FULL, max_tries=tries, chunk_log=28)
    ctx.profile(True)
    rates = []
    for _ in range(runs):
        ctx.profile_reset()
        assert ctx.pow_grind(st(i), 0, FULL, max_tries=tries, chunk_log=28) == (None, tries)
        ms, n = ctx.profile_get("pow_grind_chunk")
        assert n == 1
        rates.append(tries / (ms * 1e-3))
    ctx.profile(False)
    return {"state_index": i, "max_tries": tries, "mask": FULL, "candidates_per_s": spread(rates)}


def cpu_rate(runs=3, tries=1 << 22):
    lib = ctypes.CDLL(os.path.join(ROOT, "crypto3-zk_amd", "libzkhip_hosttest.so"))
    lib.zkt_pow_grind_cpu.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)]
    nonce, tried = ctypes.c_uint32(), ctypes.c_uint64()
    rates = []
    for r in range(runs):
        t0 = time.perf_counter()
        rc = lib.zkt_pow_grind_cpu(st(100 + r), 0, FULL, tries, ctypes.byref(nonce), ctypes.byref(tried))
        dt = time.perf_counter() - t0
        if rc == 1:  # nothing accepted: all `tries` candidates were computed
            rates.append(tries / dt)
    return {"what": "zkt_pow_grind_cpu, one host thread", "max_tries": tries, "candidates_per_s": spread(rates)}


def latency(ctx, bits, chunk_logs, n_states):
    mask = (1 << bits) - 1
    out = {"mask": mask, "states": n_states, "tried_mean": None, "chunk_log": {}}
    for cl in chunk_logs:
        ms, tried = [], []
        for i in range(n_states):
            start = int.from_bytes(st(1000 + i)[:4], "big")
            t0 = time.perf_counter()
            nonce, k = ctx.pow_grind(st(i), start, mask, chunk_log=cl)
            ms.append((time.perf_counter() - t0) * 1e3)
            assert nonce is not None
            tried.append(k)
        out["tried_mean"] = float(np.mean(tried))
        out["chunk_log"][str(cl)] = {"ms_mean": float(np.mean(ms)), **{"ms_" + k: v for k, v in spread(ms).items()}}
    return out


def proof_eval_child(lib_path, which, steps, mask):
    """runs in a process of its own; prints one JSON line"""
    bench = ctypes.CDLL(lib_path)
    ms = (ctypes.c_double * (2 * steps))()
    if which == "grinding":
        nonces = (ctypes.c_uint32 * steps)()
        rc = bench.zkhip_bench_lpc_proof_eval_grinding(0, ctypes.c_size_t(20), ctypes.c_size_t(16), ctypes.c_size_t(1), steps, ctypes.c_uint32(mask), ms, nonces)
    else:
        rounds = ctypes.c_uint64()
        rc = bench.zkhip_bench_lpc_proof_eval(0, ctypes.c_size_t(20), ctypes.c_size_t(16), ctypes.c_size_t(1), steps, 8, ms, ctypes.byref(rounds))
    assert rc == 0
    pe = list(ms)[1::2]
    print(json.dumps({"proof_eval_ms": pe, "proof_eval_ms_warm": spread(pe[1:]), "commit_ms_warm": spread(list(ms)[0::2][1:])}))


def proof_eval(lib_path, which, steps, mask=0):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib_path, which, str(steps), str(mask)], check=True, capture_output=True, text=True,
                         timeout=300).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        proof_eval_child(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--parent-lib", default=None, help="libzkhip_bench.so of a build of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pow_bench.json"))
    args = ap.parse_args()
    import bench_merkle

    zk = bench_merkle.load_pkg()
    ctx = zk.Context(0)
    res = {"what": "FRI proof of work (SHA2-256 transcript) searched on the device: zkhip_pow_grind against the reference's loop on one host thread"}
    res["kernel"] = kernel_rate(ctx, args.runs)
    print("kernel", json.dumps(res["kernel"]), flush=True)
    res["cpu"] = cpu_rate()
    res["gpu_over_one_host_thread"] = res["kernel"]["candidates_per_s"]["median"] / res["cpu"]["candidates_per_s"]["median"]
    print("cpu", json.dumps(res["cpu"]), "ratio", res["gpu_over_one_host_thread"], flush=True)
    leaf = bench_merkle.kernels(ctx, 21, 16, 1, 6)["leaf_kernel_compressions_per_s"]
    res["sanity"] = {"merkle_leaf_kernel_compressions_per_s": leaf, "half_of_it": leaf / 2,
                     "kernel_over_half": res["kernel"]["candidates_per_s"]["median"] / (leaf / 2)}
    print("sanity", json.dumps(res["sanity"]), flush=True)
    res["latency"] = {str(bits): latency(ctx, bits, (16, 20, 24), n) for bits, n in ((16, 16), (20, 16), (24, 8))}
    for cl in ("16", "20", "24"):
        res["latency"]["mean_16_plus_20_bit_ms_chunk_log_" + cl] = sum(res["latency"][b]["chunk_log"][cl]["ms_mean"] for b in ("16", "20"))
    print("latency", json.dumps(res["latency"]), flush=True)
    ctx.close()
    lib = os.path.join(ROOT, "crypto3-zk_amd", "libzkhip_bench.so")
    pe = {"instance": "16 x 2^20 rows -> domain 2^21, two opening points, one fold per round down to 16 points",
          "device_builder_sha256_transcript": {"grinding_off": proof_eval(lib, "grinding", args.steps, 0), "grinding_16_bit": proof_eval(lib, "grinding", args.steps, 0xFFFF),
                                               "grinding_20_bit": proof_eval(lib, "grinding", args.steps, 0xFFFFF)},
          "streaming_builder_scripted_transcript": {"this_tree": proof_eval(lib, "plain", args.steps)}}
    if args.parent_lib:
        pe["streaming_builder_scripted_transcript"]["parent_commit"] = proof_eval(os.path.abspath(args.parent_lib), "plain", args.steps)
        pe["streaming_builder_scripted_transcript"]["this_tree_again"] = proof_eval(lib, "plain", args.steps)
    res["proof_eval"] = pe
    print("proof_eval", json.dumps(pe), flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
