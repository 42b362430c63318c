#!/usr/bin/env python3
"""The inner-product-argument commitment (kimchi_pedersen) on the GPU box: writes profiles/ipa_bench.json.
Pallas and Vesta at 2^16 and 2^20 generators; the device call sequence of crypto3-zk_amd/include/nil/crypto3/zk/hip/kimchi_pedersen.hpp
restated over the C ABI, with the challenges given (no sponge, no group map: they are the caller's and cost what the caller's cost):
  * commitment of one full-length polynomial (one MSM over the resident, tabled g);
  * proof_eval, split by the per-kernel HIP events (zkhip_profile_get) into MSMs, generator folds, inner products and the rest (vector folds,
    the accumulation of a, b's powers, the sums of L and R), and the host's share: wall time (events off) minus the event sum -- the gaps,
    the per-round download of L and R, the drained stream behind every fold;
  * next to it the sum of the SAME-SIZE LONE MSMs the opening contains (two per round over the round's own generators, events of
    zkhip_msm_dev alone), so that what the folds add is visible;
  * verify_eval's device part: zkhip_fr_challenge_products_dev, the scaling, the MSM over [g ..., h] and the small MSM over 2 log n + 6 points.
Every figure: one warm-up, then `--runs` runs; median, min and max.
python3 tools/bench_ipa.py [--runs 5] [--logs 16,20] [--out profiles/ipa_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_pasta import NAMES, P, Q, limbs, random_scalars, spread  # noqa: E402

FR = {2: Q, 3: P}
ONE, ZERO = limbs(1), limbs(0)


def groups(dump):
    out = {"msm_ms": 0.0, "fold_ms": 0.0, "inner_product_ms": 0.0, "other_ms": 0.0}
    for name, (ms, _) in dump.items():
        key = "msm_ms" if name.startswith("msm") else "fold_ms" if name == "ipa_bases_fold" else "inner_product_ms" if name.startswith("ipa_inner_product") else "other_ms"
        out[key] += ms
    out["device_ms"] = sum(out.values())
    return out


class Opening:
    def __init__(self, zk, ctx, curve, log_n):
        self.zk, self.ctx, self.curve, self.log_n, self.n = zk, ctx, curve, log_n, 1 << log_n
        n, r = self.n, FR[curve]
        self.srs = ctx.bases_from_scalars(curve, zk.G1, random_scalars(10 + curve, n + 1))      # [g ..., h], window tables
        hu = random_scalars(20 + curve, 32)
        hu[2:] = 0
        self.hu = ctx.bases_from_scalars(curve, zk.G1, hu)                                       # [h, u, infinity x 30]: 32 points get window tables, as in the shim
        self.small = ctx.bases_from_scalars(curve, zk.G1, random_scalars(30 + curve, 2 * log_n + 6))
        self.d_poly, self.d_a, self.d_b, self.d_s = (ctx.malloc(n * 32) for _ in range(4))
        self.d_scalars = ctx.malloc((n + 1) * 32)
        self.d_sc, self.d_jac = ctx.malloc(4 * 32), ctx.malloc(6 * 96)
        ctx.h2d(self.d_poly, random_scalars(40 + curve, n))
        ctx.h2d(self.d_sc, random_scalars(41 + curve, 4))
        rng = np.random.default_rng(50 + curve)
        self.chals = [int(rng.integers(1, 1 << 62)) << 180 | int(rng.integers(1, 1 << 62)) for _ in range(log_n)]
        self.invs = [pow(c, r - 2, r) for c in self.chals]
        self.point = random_scalars(42 + curve, 1)
        self.small_scalars = random_scalars(43 + curve, 2 * log_n + 6)
        self.lr = np.zeros(24, dtype=np.uint64)

    def commitment(self):
        self.ctx.msm_dev(self.srs, self.d_poly, self.d_jac, 0, self.n)

    def proof_eval(self, keep=None):
        ctx, c, n = self.ctx, self.curve, self.n
        a, b, sc, jac = self.d_a, self.d_b, self.d_sc, self.d_jac
        ctx.poly_lincomb_dev(c, [self.d_poly], [n], ONE.reshape(1, 4), 1, a, n, False)
        ctx.fr_powers_lincomb_dev(c, self.point, ONE.reshape(1, 4), b, n)
        ctx.fr_inner_product_dev(c, a, b, n, sc)
        g, half = self.srs, n
        for ch, ci in zip(self.chals, self.invs):
            half >>= 1
            ctx.fr_inner_product_dev(c, a + 32 * half, b, half, sc + 32)
            ctx.fr_inner_product_dev(c, a, b + 32 * half, half, sc + 96)
            ctx.msm_batch_dev([g, self.hu, g, self.hu], [a + 32 * half, sc, a, sc + 64], [jac, jac + 96, jac + 192, jac + 288], [0, 0, half, 0], [half, 2, half, 2])
            ctx.jacobian_sum_dev(c, self.zk.G1, jac, 2, jac + 384)
            ctx.jacobian_sum_dev(c, self.zk.G1, jac + 192, 2, jac + 480)
            ctx.d2h(self.lr, jac + 384)                                  # L and R go to the sponge: the round's one wait
            ctx.fr_vec_affine_dev(c, a + 32 * half, a, limbs(ci), ONE, ZERO, a, half)
            ctx.fr_vec_affine_dev(c, b + 32 * half, b, limbs(ch), ONE, ZERO, b, half)
            nxt = ctx.bases_fold(g, 0, half, half, limbs(ch))
            if keep is not None:
                keep.append((g, half))
            elif g is not self.srs:
                g.free()
            g = nxt
        if keep is None and g is not self.srs:
            g.free()
        elif keep is not None:
            keep.append((g, 0))

    def lone_msms(self, rounds):
        """the opening's own MSMs, alone: per round <g_low, a_high> and <g_high, a_low> over that round's generators"""
        for g, half in rounds:
            if half:
                self.ctx.msm_dev(g, self.d_a + 32 * half, self.d_jac, 0, half)
                self.ctx.msm_dev(g, self.d_a, self.d_jac, half, half)

    def verify_eval(self):
        ctx, c, n = self.ctx, self.curve, self.n
        ctx.fr_challenge_products_dev(c, np.stack([limbs(x) for x in self.chals]), self.d_s)
        ctx.fr_vec_affine_dev(c, self.d_s, 0, limbs(self.invs[0]), None, ZERO, self.d_scalars, n)
        ctx.msm_dev(self.srs, self.d_scalars, self.d_jac, 0, n + 1)
        ctx.msm(self.small, self.small_scalars)

    def close(self):
        for b in (self.srs, self.hu, self.small):
            b.free()
        for d in (self.d_poly, self.d_a, self.d_b, self.d_s, self.d_scalars, self.d_sc, self.d_jac):
            self.ctx.free(d)


def measure(ctx, runs, fn):
    fn()
    ctx.sync()
    wall, parts = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        wall.append((time.perf_counter() - t0) * 1e3)
    ctx.profile(True)
    for _ in range(runs):
        ctx.profile_reset()
        fn()
        ctx.sync()
        parts.append(groups(ctx.profile_dump()))
    ctx.profile(False)
    out = {k: spread([p[k] for p in parts]) for k in parts[0]}
    out["wall_ms"] = spread(wall)
    # what the host adds on top of the kernels; the two medians come from different runs (events off / on), so a small negative value means "nothing"
    out["wall_minus_device_ms"] = out["wall_ms"]["median"] - out["device_ms"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--logs", default="16,20")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ipa_bench.json"))
    args = ap.parse_args()
    import bench_merkle

    zk = bench_merkle.load_pkg()
    ctx = zk.Context(0)
    res = {"what": "kimchi_pedersen over the C ABI: per-kernel HIP event sums and wall time, ms; challenges given, no sponge", "runs": args.runs, "sizes": {}}
    for log_n in [int(x) for x in args.logs.split(",")]:
        for curve in (2, 3):
            o = Opening(zk, ctx, curve, log_n)
            rounds = []
            o.proof_eval(keep=rounds)                     # the generators of every round, kept for the lone MSMs
            entry = {"commitment": measure(ctx, args.runs, o.commitment), "proof_eval": measure(ctx, args.runs, o.proof_eval),
                     "lone_msms_of_the_opening": measure(ctx, args.runs, lambda: o.lone_msms(rounds)), "verify_eval": measure(ctx, args.runs, o.verify_eval)}
            pe, lone = entry["proof_eval"], entry["lone_msms_of_the_opening"]
            entry["fold_share_of_device_time"] = pe["fold_ms"]["median"] / pe["device_ms"]["median"]
            entry["fold_over_opening_msms"] = pe["fold_ms"]["median"] / pe["msm_ms"]["median"]
            entry["fold_over_lone_msms"] = pe["fold_ms"]["median"] / lone["device_ms"]["median"]
            for g, half in rounds:
                if g is not o.srs:
                    g.free()
            o.close()
            res["sizes"][f"{NAMES[curve]}_2p{log_n}"] = entry
            print(NAMES[curve], log_n, json.dumps(entry), flush=True)
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
