#!/usr/bin/env python3
"""Per-point scalar multiplication over resident bases (run on the GPU box): writes profiles/scale_bench.json.
  * zkhip_bases_scale_dev (scalars resident on the device) and zkhip_bases_scale_geometric (coeff ratio^i, built on the device) on G1 of
    BLS12-381, BN254 and Pallas at 2^12, 2^16 and 2^20 points and on G2 of BLS12-381 at 2^12 and 2^16, interleaved in one process: wall time
    of the call (it returns with the stream drained), the per-kernel HIP event sums, and their split into records (scale_records_*), ladder
    (bases_scale_pass) and normalisation (ec_ntt_store_affine);
  * next to them the only device route there was before, and only for ONE scalar: zkhip_bases_fold of the same points with `lo` at
    infinity (a spread of the points behind as many rows of infinity) -- against zkhip_bases_scale_geometric with ratio = 1 and the same
    scalar as coeff.  The two results are compared point for point first;
  * the loop the reference runs on one host thread (naive_batch_exp: one double-and-add per point): the oracle's naive multiexp on ONE thread
    over a prefix of at most 2^12 of the points, SCALED LINEARLY to the size (`host_loop_scaled_ms`; `host_prefix` says from how many points).
Every figure: one warm-up, then `--runs` timed runs (tools/bench_pasta.py: timed); median, min and max.
python3 tools/bench_scale.py [--runs 10] [--out profiles/scale_bench.json] [--logs 12 16 20] [--g2-logs 12 16]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from bench_pasta import NAMES, limbs, random_scalars, timed  # noqa: E402

RECORDS, LADDER, NORMALISATION = "scale_records", "bases_scale_pass", "ec_ntt_store_affine"
PREFIXES = [RECORDS, LADDER, NORMALISATION, "ipa_bases_fold"]
HOST_PREFIX = 1 << 12


def host_loop_ms(cp, curve, group, pts, inf, scalars):
    """the oracle's naive multiexp (a double-and-add per point) on one thread over the prefix, in ms"""
    k = min(HOST_PREFIX, len(scalars))
    threads = cp.num_threads()
    cp.set_threads(1)
    try:
        t0 = time.perf_counter()
        cp.msm(curve, group, pts[:k], scalars[:k], inf=inf[:k], naive=True)
        return (time.perf_counter() - t0) * 1e3, k
    finally:
        cp.set_threads(threads)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--logs", type=int, nargs="+", default=[12, 16, 20])
    ap.add_argument("--g2-logs", type=int, nargs="+", default=[12, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale_bench.json"))
    args = ap.parse_args()
    import bench_merkle
    import cport as cp

    zk = bench_merkle.load_pkg()
    ctx = zk.Context(0)
    res = {"what": "zkhip_bases_scale_dev / zkhip_bases_scale_geometric: per-kernel HIP event sums and host wall time, ms; "
                   "host_loop_scaled_ms is a one-thread measurement over host_prefix points scaled linearly to n", "runs": args.runs}
    shapes = [(c, zk.G1, l) for l in args.logs for c in (0, 1, 2)] + [(0, zk.G2, l) for l in args.g2_logs]
    for curve, group, log_n in shapes:
        n = 1 << log_n
        key = "%s_g%d_2^%d" % (NAMES[curve], group, log_n)
        src = ctx.bases_from_scalars(curve, group, random_scalars(30 + curve, n))
        s = random_scalars(40 + curve, n)
        d_s = ctx.malloc(32 * n)
        ctx.h2d(d_s, s)
        ratio, coeff, one = s[1], s[2], limbs(1)
        subjects = {"device_scalars": lambda: ctx.bases_scale_dev(src, 0, n, d_s).free(),
                    "geometric": lambda: ctx.bases_scale_geometric(src, 0, n, ratio, coeff).free(),
                    "one_scalar": lambda: ctx.bases_scale_geometric(src, 0, n, one, coeff).free()}
        padded = None
        if group == zk.G1:
            padded = src.spread(2 * n, first=n)    # rows [0, n): infinity (`lo`), rows [n, 2n): the points (`hi`)
            a, b = ctx.bases_scale_geometric(src, 0, n, one, coeff), ctx.bases_fold(padded, 0, n, n, coeff)
            (pa, ia), (pb, ib) = a.download(), b.download()
            assert (ia == ib).all() and (pa == pb).all(), "scale and fold disagree"
            a.free()
            b.free()
            subjects["fold_one_scalar"] = lambda: ctx.bases_fold(padded, 0, n, n, coeff).free()
        r = timed(ctx, args.runs, subjects, PREFIXES)
        for name in ("device_scalars", "geometric", "one_scalar"):
            r[name]["split_ms"] = {"records": r[name][RECORDS]["median"], "ladder": r[name][LADDER]["median"], "normalisation": r[name][NORMALISATION]["median"]}
            r[name]["ns_per_point"] = r[name]["total_ms"]["median"] * 1e6 / n
        pts, inf = src.download(0, min(n, HOST_PREFIX))
        host_ms, k = host_loop_ms(cp, curve, group, pts, inf, s)
        r["host_prefix"] = k
        r["host_loop_scaled_ms"] = host_ms * n / k
        r["ratios"] = {"host_loop_scaled_over_device_scalars_wall": r["host_loop_scaled_ms"] / r["device_scalars"]["wall_ms"]["median"],
                       "host_loop_scaled_over_geometric_wall": r["host_loop_scaled_ms"] / r["geometric"]["wall_ms"]["median"]}
        if padded is not None:
            r["fold_one_scalar"]["ns_per_point"] = r["fold_one_scalar"]["total_ms"]["median"] * 1e6 / n
            r["ratios"]["one_scalar_over_fold_kernels"] = r["one_scalar"]["total_ms"]["median"] / r["fold_one_scalar"]["total_ms"]["median"]
            r["ratios"]["one_scalar_over_fold_wall"] = r["one_scalar"]["wall_ms"]["median"] / r["fold_one_scalar"]["wall_ms"]["median"]
            padded.free()
        res[key] = r
        print(key, json.dumps(r), flush=True)
        ctx.free(d_s)
        src.free()
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
