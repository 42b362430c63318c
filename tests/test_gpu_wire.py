"""Proving-key points from their wire form (zkhip_bases_upload_compressed): the device decodes the ZCash compressed
BLS12-381 encodings the reference's serializers emit (g16/marshalling.hpp:111-112, 178-201).  Checked against the
reference's own literal vectors (AGG:932-1010, tests/golden/ref_kat.json), against the oracle on random points of
both signs incl. infinity, and on malformed input; and an MSM over a key loaded this way.

Below those: the encodings random keys never produce, built by tests/wire_cases.py and judged by its definition-level model (which takes
no square root: x as encoded, y^2 = x^3 + b, the flag names the larger of {y, -y}) -- every special valid class alone, all of them side by
side in the lanes of one workgroup, every refusal class with the count zkhip_last_error promises, and a wire-loaded key under the pairing
kernel.  tests/test_host_wire.py holds the oracle to the same model on the CPU."""
import contextlib
import json
import os

import numpy as np
import pytest

import cport as cp
import pyoracle as po
import wire_cases as wc
from test_pairing_ref import load_kat
from util import limbs, pt_from_limbs, pt_limbs

pytestmark = pytest.mark.gpu
KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_kat.json")))["serialisation_test"]


def _points(b, group):
    pts, inf = b.download()
    return [pt_from_limbs(0, group, pts[i], inf[i]) for i in range(len(inf))]


def test_reference_serialisation_vectors_on_device(ctx):
    g1 = (int(KAT["g1"][0], 16), int(KAT["g1"][1], 16))
    b = ctx.upload_bases_compressed(0, 1, bytes(KAT["g1_bytes"]), 1)
    assert _points(b, 1) == [g1]
    b.free()
    g2 = tuple((int(c[0], 16), int(c[1], 16)) for c in KAT["g2"])
    b = ctx.upload_bases_compressed(0, 2, bytes(KAT["g2_bytes"]), 1)
    assert _points(b, 2) == [g2]
    b.free()


@pytest.mark.parametrize("group,n", [(1, 300), (2, 120)])
def test_compressed_round_trip_and_msm(ctx, group, n):
    G = po.BLS12_381.g1 if group == 1 else po.BLS12_381.g2
    ks = cp.random_fr(0, 91, n)
    pts, inf = cp.batch_mul(0, group, ks)
    P = [pt_from_limbs(0, group, pts[i], inf[i]) for i in range(n)]
    P[3] = None          # infinity
    P[5] = G.neg(P[4])   # both roots of one x
    P[7] = G.gen
    blob = b"".join(po.bls12_381_compress(group, p) for p in P)
    assert {bool(c[0] & 0x20) for c in (blob[i * 48 * group:(i + 1) * 48 * group] for i in range(n))} == {True, False}
    b = ctx.upload_bases_compressed(0, group, blob, n)
    assert _points(b, group) == P
    # the loaded key behaves like an uploaded one
    sc = cp.random_fr(0, 92, n)
    ref = ctx.upload_bases(0, group, np.stack([pt_limbs(0, group, p) for p in P]), np.array([p is None for p in P], dtype=np.uint8))
    a1, i1 = ctx.msm_affine(b, sc)
    a2, i2 = ctx.msm_affine(ref, sc)
    assert i1 == i2 and (a1 == a2).all()  # (Jacobian representatives may differ: compared in affine)
    b.free()
    ref.free()
    empty = ctx.upload_bases_compressed(0, group, b"", 0)
    empty.free()


@pytest.mark.parametrize("group", [1, 2])
def test_malformed_encodings_are_rejected(ctx, zk, group):
    G = po.BLS12_381.g1 if group == 1 else po.BLS12_381.g2
    good = po.bls12_381_compress(group, G.mul(G.gen, 77))
    p = po.BLS12_381.p
    # an x that is not on the curve (searched with the oracle)
    x = 5
    while True:
        cand = (bytes(47) + bytes([x])) if group == 1 else (bytes(95) + bytes([x]))
        cand = bytes([cand[0] | 0x80]) + cand[1:]
        try:
            po.bls12_381_decompress(group, cand)
            x += 1
        except ValueError:
            break
    bad = [
        bytes([good[0] & 0x7F]) + good[1:],                                   # compression flag missing
        bytes([0xC0]) + bytes(48 * group - 2) + bytes([1]),                       # infinity with a non-zero body
        bytes([0x9F]) + bytes([255]) * 47 + (good[48:] if group == 2 else b""),      # x >= p
        cand,                                                                 # not on the curve
    ]
    for enc in bad:
        assert len(enc) == 48 * group
        with pytest.raises(zk.ZkhipError):
            ctx.upload_bases_compressed(0, group, good + enc, 2)
    with pytest.raises(zk.ZkhipError):
        ctx.upload_bases_compressed(1, group, good, 1)  # BN254: no pinned wire format
    # 64 encodings, one flag byte corrupted: refused as invalid, twice; then the context loads the intact key and computes with it
    n = 64
    pts, inf = cp.batch_mul(0, group, cp.random_fr(0, 93, n))
    blob = b"".join(po.bls12_381_compress(group, pt_from_limbs(0, group, pts[i], inf[i])) for i in range(n))
    at = 17 * 48 * group
    broken = blob[:at] + bytes([blob[at] & 0x7F]) + blob[at + 1:]
    for _ in range(2):
        with pytest.raises(zk.ZkhipError, match="invalid argument"):
            ctx.upload_bases_compressed(0, group, broken, n)
    b = ctx.upload_bases_compressed(0, group, blob, n)
    sc = cp.random_fr(0, 94, n)
    aff, is_inf = ctx.msm_affine(b, sc)
    exp, einf = cp.msm(0, group, pts, sc, chunks=2)
    assert is_inf == einf and (aff == exp).all()
    b.free()


# ---- the branches random keys never take (tests/wire_cases.py)
@contextlib.contextmanager
def _no_tables(ctx):
    """only the decode is under test: no window tables over points outside the r-subgroup"""
    was = ctx.get_option("msm_precompute")
    ctx.set_option("msm_precompute", 0)
    try:
        yield
    finally:
        ctx.set_option("msm_precompute", was)


def _decode(ctx, group, encs):
    with _no_tables(ctx):
        b = ctx.upload_bases_compressed(0, group, b"".join(encs), len(encs))
    try:
        return _points(b, group)
    finally:
        b.free()


def _last_error(ctx):
    return ctx.lib.zkhip_last_error(ctx.h).decode()


@pytest.mark.parametrize("group", [1, 2])
def test_every_special_valid_class_alone(ctx, group):
    for name, encs in wc.valid_classes(group).items():
        assert name == "infinity" or {wc.classify(group, e)[2] for e in encs} == {True, False}, name
        for enc in encs:
            (pt,) = _decode(ctx, group, [enc])
            wc.check_decoded(group, enc, pt)
            assert po.bls12_381_compress(group, pt) == enc, name
            # the shape of y says which arm produced it: the generic arm cannot stand in for these
            if name == "a1 == 0, a0 a square":
                assert pt[1][1] == 0 and pt[1][0] != 0
            if name == "a1 == 0, a0 a non-square":
                assert pt[1][0] == 0 and pt[1][1] != 0
            if name == "boundary y":
                assert pt[1][1] == ((wc.P + 1) // 2 if wc.classify(group, enc)[2] else (wc.P - 1) // 2)


@pytest.mark.parametrize("group", [1, 2])
def test_all_classes_side_by_side_in_one_workgroup(ctx, group):
    """n = 130: two full 64-lane workgroups and a tail of two, neighbouring lanes on different paths through the nested conditionals"""
    encs, tags = wc.mixed_batch(group, 130)
    pts = _decode(ctx, group, encs)
    assert len(pts) == 130
    for i, (enc, pt) in enumerate(zip(encs, pts)):
        assert (pt is None) == (tags[i] == "infinity"), i
        wc.check_decoded(group, enc, pt)


@pytest.mark.parametrize("group", [1, 2])
def test_every_refusal_is_counted(ctx, zk, group):
    n = 70
    raw, inf = cp.batch_mul(0, group, cp.random_fr(0, 96, n))
    good_pts = [pt_from_limbs(0, group, raw[i], inf[i]) for i in range(n)]
    good = [po.bls12_381_compress(group, p) for p in good_pts]
    bad = wc.refusals(group)
    assert {reason for _, reason in bad} >= {"compression flag missing", "infinity with other bits set", "x not on the curve"} and len(bad) <= n - 4

    def refused(encs, k):
        with pytest.raises(zk.ZkhipError, match="invalid argument"):
            ctx.upload_bases_compressed(0, group, b"".join(encs), len(encs))
        assert _last_error(ctx).startswith("%d point encoding(s) rejected" % k), _last_error(ctx)

    def intact_loads():
        b = ctx.upload_bases_compressed(0, group, b"".join(good), n)
        try:
            assert _points(b, group) == good_pts
        finally:
            b.free()

    # one bad encoding: at the first and last lane of the first workgroup, the first lane of the second, the last of the tail
    for at, (enc, _) in zip((0, 63, 64, 69), bad[::len(bad) // 4]):
        refused(good[:at] + [enc] + good[at + 1:], 1)
        intact_loads()
    # the full list, those four positions among them
    where = [0, 63, 64, 69] + [2 + 2 * j for j in range(len(bad) - 4)]
    assert len(set(where)) == len(bad) and max(where) < n
    blob = list(good)
    for at, (enc, _) in zip(where, bad):
        blob[at] = enc
    assert sum(wc.verdict(group, e) not in ("inf", "point") for e in blob) == len(bad)
    refused(blob, len(bad))
    intact_loads()
    # each class alone next to one good encoding: none hides behind another
    for enc, reason in bad:
        refused([good[0], enc], 1)
        refused([enc, good[0]], 1)
    refused([bad[0][0], bad[-1][0]], 2)
    intact_loads()


def test_a_key_loaded_from_the_wire_feeds_the_pairing_kernel(ctx):
    """the reference's kzg_ipp2 single commitment (tests/golden/ref_ipp2_kat.json) over a and v1 loaded from their compressed form"""
    a, _, v1, _, _, _, exp = load_kat()
    pa = ctx.upload_bases_compressed(0, 1, b"".join(po.bls12_381_compress(1, p) for p in a), len(a))
    pv = ctx.upload_bases_compressed(0, 2, b"".join(po.bls12_381_compress(2, q) for q in v1), len(v1))
    try:
        assert _points(pa, 1) == a and _points(pv, 2) == v1
        out = ctx.pairing_products([(pa, 0, pv, 0, len(a), 0)], 1)[0]
        assert [po.from_limbs(out[k * 6:(k + 1) * 6]) for k in range(12)] == exp["single_first"]
    finally:
        pa.free(), pv.free()
