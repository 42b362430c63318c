"""Cases and checks for the shared inversion over parked points (csrc/curve.hpp: xyzz_park, xyzz_parked_to_affine) as arith_ops.h's
parked_affine runs it: entry k is the madd chain over pts[0..k], all entries are parked and normalised with ONE inversion.  Used by the
host suites (zkt_parked_affine) and the device ones (zkd_parked_affine, zkdp_parked_affine)."""
import ctypes

import numpy as np

from util import pt_from_limbs, pts_arr


def cases(G, base):
    """(points, infinity flags, negation flags) per case, from four distinct finite points: nothing; one entry, finite and infinite; nine
    entries (more than one chunk of 8); an infinite entry first, in the middle (P, -P, Q), last, two adjacent, every entry infinite; and
    P, P for the doubling inside the chain"""
    Pt, Q, R, S = base
    return [
        ([], [], []),
        ([Pt], [0], [0]),
        ([Pt], [1], [0]),
        ([Pt, Q, R, S, Pt, Q, R, S, Pt], [0] * 9, [0, 0, 1, 0, 0, 0, 0, 1, 0]),
        ([Pt, Q, R], [1, 0, 0], [0] * 3),
        ([Pt, Pt, Q], [0] * 3, [0, 1, 0]),
        ([Pt, Q, G.add(Pt, Q)], [0] * 3, [0, 0, 1]),
        ([Pt, Pt, R, Q, S], [0, 0, 1, 0, 0], [0, 1, 0, 0, 0]),
        ([Pt, Q, R], [1, 1, 1], [0] * 3),
        ([Pt, Pt, Q], [0] * 3, [0] * 3),
    ]


def prefixes(G, pts, infs, negs):
    """the partial sums in big integers (None: infinity)"""
    out, acc = [], None
    for Pt, i, n in zip(pts, infs, negs):
        if not i:
            acc = G.add(acc, G.neg(Pt) if n else Pt)
        out.append(acc)
    return out


def run(fn, field, curve, group, pts, infs, negs, layout):
    """one call of a zk?_parked_affine entry: (n rows of canonical x | y as u32, n infinity flags)"""
    n = len(pts)
    arr = np.ascontiguousarray(pts_arr(curve, group, pts).view(np.uint32).reshape(n, -1)) if n else np.zeros((1, 1), dtype=np.uint32)
    width = arr.shape[1] if n else 1
    out = np.full((max(n, 1), width), 0xA5A5A5A5, dtype=np.uint32)
    oinf = np.full(max(n, 1), 7, dtype=np.uint8)
    infa, nega = np.array(infs + [0], dtype=np.uint8), np.array(negs + [0], dtype=np.uint8)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert fn(field, P(arr), P(infa), P(nega), ctypes.c_size_t(n), layout, P(out), P(oinf)) == 0
    return out[:n], oinf[:n]


def check(fn, field, curve, group, G, base):
    """every prefix of every case against the big-integer sums, in both layouts, which must agree limb for limb; returns the outputs"""
    results = []
    for pts, infs, negs in cases(G, base):
        exp = prefixes(G, pts, infs, negs)
        out, oinf = run(fn, field, curve, group, pts, infs, negs, 0)
        out1, oinf1 = run(fn, field, curve, group, pts, infs, negs, 1)
        assert (out == out1).all() and (oinf == oinf1).all(), (field, len(pts), infs, negs)
        for k, e in enumerate(exp):
            assert int(oinf[k]) == (1 if e is None else 0), (field, k, infs, negs)
            assert pt_from_limbs(curve, group, np.ascontiguousarray(out[k]).view(np.uint64), int(oinf[k])) == e, (field, k, infs, negs)
        results.append((out, oinf))
    return results
