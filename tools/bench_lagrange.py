#!/usr/bin/env python3
"""The Lagrange-basis SRS on the device (run on the GPU box): writes profiles/lagrange_bench.json.
  * zkhip_bases_lagrange at 2^12 and 2^16 points for Pallas and Vesta next to BN254 (the nearest counterpart by field width), interleaved in
    one process: wall time of the call (it returns with the stream drained), the per-kernel HIP event sums, and their split into the stage
    network (records, multiplication passes, butterflies, the affine load), the output normalisation (ec_ntt_store_affine) and the
    window tables (bases_precompute);
  * the A/B that chose the ladder: the same constructor over the GLV split (33 windows of 4 doublings + 2 additions) against the plain
    65-window ladder (4 + 1), Pallas and Vesta at 2^16, interleaved; the two results are compared point for point first;
  * a column of 2^16 evaluations committed through the Lagrange bases (upload + one MSM: commitment_evaluations) against the inverse NTT
    and the MSM over g (what `commitment` needs when the column is held as evaluations).
Every figure: one warm-up, then `--runs` timed runs (tools/bench_pasta.py: timed); median, min and max.
python3 tools/bench_lagrange.py [--runs 10] [--out profiles/lagrange_bench.json] [--logs 12 16]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_pasta import NAMES, P, Q, limbs, random_scalars, timed  # noqa: E402

BN_R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
FR = {1: (BN_R, 5), 2: (Q, 5), 3: (P, 5)}  # scalar field and its multiplicative generator
NETWORK = ["ec_ntt_setup", "ec_ntt_records", "ec_ntt_load_affine", "ec_ntt_mul_pass", "ec_ntt_butterflies"]
PREFIXES = NETWORK + ["ec_ntt_store_affine", "bases_precompute"]


def root(curve, log_m):
    r, g = FR[curve]
    return limbs(pow(g, (r - 1) >> log_m, r))


def split(res):
    """stage network / output normalisation / window tables from the per-prefix medians"""
    for d in res.values():
        d["stage_network_ms"] = sum(d[p]["median"] for p in NETWORK)
        d["normalisation_ms"] = d["ec_ntt_store_affine"]["median"]
        d["window_tables_ms"] = d["bases_precompute"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--logs", type=int, nargs="+", default=[12, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lagrange_bench.json"))
    args = ap.parse_args()
    import bench_merkle

    zk = bench_merkle.load_pkg()
    ctx = zk.Context(0)
    top = max(args.logs)
    res = {"what": "zkhip_bases_lagrange: per-kernel HIP event sums and host wall time, ms", "runs": args.runs}
    srs = {c: ctx.bases_from_scalars(c, zk.G1, random_scalars(10 + c, 1 << top)) for c in (1, 2, 3)}

    def plain(c, log_m):
        h = ctypes.c_void_p()
        ctx._check(ctx.lib.zkhip_bench_bases_lagrange_plain(ctx.h, srs[c].h, ctypes.c_size_t(0), ctypes.c_size_t(log_m),
                                                            root(c, log_m).ctypes.data_as(ctypes.c_void_p), ctypes.byref(h)), "zkhip_bench_bases_lagrange_plain")
        return zk.zkhip.Bases(ctx, h, c, zk.G1, 1 << log_m)

    # ---- the constructor, three curves side by side
    for log_m in args.logs:
        subjects = {NAMES[c]: (lambda c=c: ctx.bases_lagrange(srs[c], 0, log_m, root(c, log_m)).free()) for c in (1, 2, 3)}
        key = "bases_lagrange_2^%d" % log_m
        res[key] = split(timed(ctx, args.runs, subjects, PREFIXES))
        res[key]["ratios"] = {NAMES[c] + "_over_bn254": res[key][NAMES[c]]["total_ms"]["median"] / res[key]["bn254"]["total_ms"]["median"] for c in (2, 3)}
        print(key, json.dumps(res[key]), flush=True)

    # ---- GLV against the plain ladder
    subjects = {}
    for c in (2, 3):
        a, b = ctx.bases_lagrange(srs[c], 0, top, root(c, top)), plain(c, top)
        (pa, ia), (pb, ib) = a.download(), b.download()
        assert (ia == ib).all() and (pa == pb).all(), "the two ladders disagree"
        a.free()
        b.free()
        subjects[NAMES[c] + "_glv"] = lambda c=c: ctx.bases_lagrange(srs[c], 0, top, root(c, top)).free()
        subjects[NAMES[c] + "_plain"] = lambda c=c: plain(c, top).free()
    ab = timed(ctx, args.runs, subjects, ["ec_ntt_mul_pass", "ec_ntt_records"])
    ab["ratios"] = {}
    for c in (2, 3):
        g, p = ab[NAMES[c] + "_glv"], ab[NAMES[c] + "_plain"]
        ab["ratios"][NAMES[c]] = {"mul_pass_glv_over_plain": g["ec_ntt_mul_pass"]["median"] / p["ec_ntt_mul_pass"]["median"],
                                  "total_glv_over_plain": g["total_ms"]["median"] / p["total_ms"]["median"],
                                  "wall_glv_over_plain": g["wall_ms"]["median"] / p["wall_ms"]["median"]}
    ab["group_operations_glv_over_plain"] = 33 * 6 / (65 * 5)
    res["glv_ab_2^%d" % top] = ab
    print("glv_ab", json.dumps(ab), flush=True)

    # ---- a column held as evaluations: one MSM over the Lagrange bases against inverse NTT + MSM over g
    m = 1 << top
    evals = np.random.default_rng(20).integers(0, 1 << 63, size=(m, 4), dtype=np.uint64) << np.uint64(1)
    evals[:, 3] >>= np.uint64(2)  # below 2^254 < r of both curves and as wide as r: both paths multiply by full-width scalars
    d_e, d_o = ctx.malloc(m * 32), ctx.malloc(512)
    col = {}
    for c in (2, 3):
        lag = ctx.bases_lagrange(srs[c], 0, top, root(c, top))

        def by_evals(lag=lag):
            ctx.h2d(d_e, evals)
            ctx.msm_dev(lag, d_e, d_o)

        def by_coeffs(c=c):
            ctx.h2d(d_e, evals)
            ctx.ntt_dev(c, d_e, top, 1, root(c, top), inverse=True)
            ctx.msm_dev(srs[c], d_e, d_o)

        out = np.zeros((2, 12), dtype=np.uint64)
        by_evals()
        ctx.d2h(out[0], d_o)
        by_coeffs()
        ctx.d2h(out[1], d_o)
        ja, jb = ctx.jacobian_to_affine(c, zk.G1, out[0].reshape(3, 4)), ctx.jacobian_to_affine(c, zk.G1, out[1].reshape(3, 4))
        assert ja[1] == jb[1] and (ja[0] == jb[0]).all(), "the two commitments differ"
        r = timed(ctx, args.runs, {"evaluations": by_evals, "coefficients": by_coeffs}, ["msm", "ntt"])
        r["wall_evaluations_over_coefficients"] = r["evaluations"]["wall_ms"]["median"] / r["coefficients"]["wall_ms"]["median"]
        col[NAMES[c]] = r
        lag.free()
    res["column_commit_2^%d" % top] = col
    print("column_commit", json.dumps(col), flush=True)
    ctx.free(d_e)
    ctx.free(d_o)
    for b in srs.values():
        b.free()
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
