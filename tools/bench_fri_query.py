#!/usr/bin/env python3
"""Whole LPC opening proofs at size (run on the GPU box): writes profiles/fri_query_bench.json.
The README's LPC instance -- 16 x 2^20 rows -> domain 2^21, device tree builder, SHA2-256 transcript, one fold per round down to 16 points --
with `lambda` queries (default 40):
  * lpc_commitment_scheme_hip::proof_eval alone, proof_eval_full (proof_eval + the query phase on the device), and the query phase by part:
    re-extension of the committed batch from its resident coefficient forms, the value gathers (zkhip_fri_query_dev), the paths
    (zkhip_merkle_paths_multi), the host part (domain indices, limb conversion, the final polynomial at +-x^2); host wall times, medians over
    the warm runs, per-kernel HIP events off;
  * the kernels one query phase launched, by name and count, from the library's profiler in the last run (kept out of the medians);
  * next to it the path a caller of proof_eval alone takes for the same answers: download of every round polynomial
    (fri_round_polynomial(i)) and of every coefficient form (coefficients(batch, i)), and the evaluation of every committed polynomial at
    the 2 lambda query points on the host -- all polynomials on 16 threads, and `--one-thread-polys` of them on one thread (scaled to all 16
    in the summary: the whole of it takes about a minute).  Measured once.
python3 tools/bench_fri_query.py [--steps 7] [--lam 40] [--one-thread-polys 2] [--out profiles/fri_query_bench.json]"""
import argparse
import ctypes
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_N, COLS, EXPAND = 20, 16, 1


def median(v):
    return float(np.median(np.asarray(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7, help="runs; the first is the warm-up, the last has the profiler on: the medians are over the others")
    ap.add_argument("--lam", type=int, default=40)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--one-thread-polys", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri_query_bench.json"))
    args = ap.parse_args()
    bench = ctypes.CDLL(os.path.join(ROOT, "crypto3-zk_amd", "libzkhip_bench.so"))
    ms = (ctypes.c_double * (7 * args.steps))()
    caller = (ctypes.c_double * 4)()
    dump = ctypes.create_string_buffer(1 << 16)
    verified = ctypes.c_int()
    sz = ctypes.c_size_t
    rc = bench.zkhip_bench_lpc_query_phase(0, sz(LOG_N), sz(COLS), sz(EXPAND), args.steps, sz(args.lam), ctypes.c_uint(args.threads), sz(args.one_thread_polys), ms,
                                           caller, dump, sz(len(dump)), ctypes.byref(verified))
    assert rc == 0, rc
    rows = np.array(list(ms)).reshape(args.steps, 7)
    assert args.steps >= 3
    warm = rows[1:-1]
    names = ["proof_eval_ms", "proof_eval_full_ms", "query_phase_ms", "reextension_ms", "gathers_ms", "paths_ms", "host_part_ms"]
    launches = {}
    for line in dump.value.decode().splitlines():
        name, t, cnt = line.rsplit(" ", 2)
        launches[name] = {"count": int(cnt), "ms": float(t)}
    scale = COLS / args.one_thread_polys if args.one_thread_polys else None
    res = {
        "what": "whole LPC opening proofs: proof_eval_full (query phase on the device) against proof_eval plus the caller's host query phase",
        "instance": f"{COLS} x 2^{LOG_N} rows -> domain 2^{LOG_N + EXPAND}, step list all ones down to 16 points, lambda {args.lam}, device tree builder, "
                    "SHA2-256 transcript, BLS12-381 Fr",
        "runs": args.steps, "runs_in_the_medians": len(warm), "verify_eval_accepts": bool(verified.value),
        "all_runs_ms": {n: [float(x) for x in rows[:, k]] for k, n in enumerate(names)},
        "median_warm_ms": {n: median(warm[:, k]) for k, n in enumerate(names)},
        "query_phase_launches": launches,
        "caller_path_of_the_parent": {
            "what": "what a caller of proof_eval alone does for the same answers; a path of the parent commit, measured here once",
            "download_round_polynomials_ms": caller[0], "download_coefficient_forms_ms": caller[1],
            "host_evaluation_one_thread_ms": caller[2], "host_evaluation_one_thread_polynomials": args.one_thread_polys,
            "host_evaluation_one_thread_scaled_to_all_ms": caller[2] * scale if scale else None,
            "host_evaluation_threads": args.threads, "host_evaluation_threads_ms": caller[3],
            "field_multiplications": COLS * 2 * args.lam << LOG_N,
        },
    }
    m = res["median_warm_ms"]
    res["reextension_share_of_query_phase"] = m["reextension_ms"] / m["query_phase_ms"] if m["query_phase_ms"] else None
    c = res["caller_path_of_the_parent"]
    c["total_with_threads_ms"] = c["download_round_polynomials_ms"] + c["download_coefficient_forms_ms"] + c["host_evaluation_threads_ms"]
    print(json.dumps(res["median_warm_ms"]), json.dumps(c), json.dumps(launches), flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
