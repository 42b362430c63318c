"""zkhip_groth16_verify_batch on the GPU (include/zkhip.h, "Groth16 verification"; csrc/groth16_verify.hip): per proof
ok = well_formed && final_exponentiation(miller(A, B) miller(-acc, gamma) miller(-C, delta)) == alpha_beta.

Checked against the reference's eight bellperson proofs (tests/golden/ref_groth16_verify_kat.json), against the model of
tests/groth16_verify_ref.py on synthetic keys (the compared value of ANY proof scalars is one exponentiation of e(G1, G2) there), and
against the host twin bit for bit.  Sizes: 1, 63, 64, 65 around the 64-lane workgroup (one proof per lane), 130 (three workgroups, the last
with two live lanes); the accumulation takes its inputs one after another without chunks, so the input counts 0, 1 and 11 are its shapes."""
import ctypes
import random

import numpy as np
import pytest

import groth16_verify_ref as gr
import pairing_ref as pr
from test_gpu_pairing import BLS, G1, G2, INVALID, RANGE, fq_limbs, fr_arr, gt_ints, upload_g1, upload_g2
from test_host_groth16_verify import host_verify
from test_host_pairing import SO

pytestmark = pytest.mark.gpu

R, P = gr.R, gr.P
g1 = gr.G1


def upload_key(ctx, alpha_beta, gamma, delta, ic):
    g2l = lambda q: fq_limbs(q[0][0]) + fq_limbs(q[0][1]) + fq_limbs(q[1][0]) + fq_limbs(q[1][1])
    abc = np.array([fq_limbs(p[0]) + fq_limbs(p[1]) if p is not None else [0] * 12 for p in ic], dtype=np.uint64)
    return ctx.groth16_vk_upload(np.array([l for v in alpha_beta for l in fq_limbs(v)], dtype=np.uint64), np.array(g2l(gamma), dtype=np.uint64),
                                 np.array(g2l(delta), dtype=np.uint64), abc, np.array([p is None for p in ic], dtype=np.uint8))


def inputs_arr(rows):
    return fr_arr([x for row in rows for x in row]).reshape(len(rows), -1, 4)


class Batch:
    """n proofs of `key` from scalars (a zero scalar is the point at infinity), resident as three bases objects"""

    def __init__(self, ctx, key, scalars, xs):
        self.key, self.scalars, self.xs = key, scalars, xs
        self.a = ctx.bases_from_scalars(BLS, G1, fr_arr([s[0] for s in scalars]))
        self.b = ctx.bases_from_scalars(BLS, G2, fr_arr([s[1] for s in scalars]))
        self.c = ctx.bases_from_scalars(BLS, G1, fr_arr([s[2] for s in scalars]))

    def free(self):
        self.a.free(), self.b.free(), self.c.free()

    def check(self, ctx, vk, idx_gt, offset=0, n=None, n_inputs=None):
        """verify proofs offset .. offset + n; ok against the model everywhere, the compared value at the indices idx_gt (relative to offset)"""
        n = len(self.scalars) - offset if n is None else n
        rows = [x if n_inputs is None else x[:n_inputs] for x in self.xs[offset:offset + n]]
        ok, gt = ctx.groth16_verify(vk, self.a, self.b, self.c, inputs_arr(rows), offset=offset, n=n, want_gt=True)
        exp = [int(self.key.accepts(s, x)) for s, x in zip(self.scalars[offset:offset + n], rows)]
        assert list(ok) == exp
        for i in idx_gt:
            assert gt_ints(gt[i]) == self.key.expected_gt(self.scalars[offset + i], rows[i]), i
        return exp


def make_batch(ctx, key, n, seed, bad=(), n_inputs=None):
    rnd = random.Random(seed)
    l = key.l if n_inputs is None else n_inputs
    xs = [[rnd.randrange(R) for _ in range(l)] for _ in range(n)]
    scalars = [key.prove(x) for x in xs]
    for i in bad:
        a, b, c = scalars[i]
        scalars[i] = (a, b, (c + 1 + i) % R)
    return Batch(ctx, key, scalars, xs)


@pytest.fixture(scope="module")
def key11(ctx):
    key = gr.Key(100, 11)
    vk = upload_key(ctx, key.alpha_beta(), *key.points())
    assert vk.n_inputs == 11
    yield key, vk
    vk.free()


BAD = (0, 62, 63, 64, 129)  # index 0, 63, 64 and n - 1 of every prefix n in 1, 63, 64, 65, 130


@pytest.fixture(scope="module")
def batch130(ctx, key11):
    bt = make_batch(ctx, key11[0], 130, 101, bad=BAD)
    yield bt
    bt.free()


@pytest.fixture(scope="module")
def kat(ctx):
    k = gr.load_kat()
    k["vk"] = upload_key(ctx, k["alpha_beta"], k["gamma"], k["delta"], k["ic"])
    yield k
    k["vk"].free()


def kat_verify(ctx, kat, proofs, xs):
    a, b, c = upload_g1(ctx, [p[0] for p in proofs]), upload_g2(ctx, [p[1] for p in proofs]), upload_g1(ctx, [p[2] for p in proofs])
    try:
        ok, gt = ctx.groth16_verify(kat["vk"], a, b, c, inputs_arr(xs), want_gt=True)
    finally:
        a.free(), b.free(), c.free()
    return list(ok), [gt_ints(g) for g in gt]


def test_the_eight_reference_proofs_in_one_call(ctx, kat):
    ok, gt = kat_verify(ctx, kat, kat["proofs"], kat["statements"])
    assert ok == [1] * 8
    assert all(g == kat["alpha_beta"] for g in gt)


def test_perturbed_reference_proofs_are_rejected(ctx, kat):
    (a0, b0, c0), (a1, b1, c1) = kat["proofs"][:2]
    st = kat["statements"][0]
    changed = st[:10] + [st[10] + 1]
    ok, gt = kat_verify(ctx, kat, [(a1, b0, c0), (a0, b1, c0), (a0, b0, c1), (a0, b0, c0), (a0, b0, c0)], [st, st, st, changed, st])
    assert ok == [0, 0, 0, 0, 1]
    assert all(g != kat["alpha_beta"] for g in gt[:4]) and gt[4] == kat["alpha_beta"]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_batch_sizes(ctx, key11, batch130, n):
    rejected = [i for i in BAD if i < n and i in (0, 63, 64, n - 1)]
    accepted = [i for i in range(n) if i not in BAD][:2]
    exp = batch130.check(ctx, key11[1], rejected + accepted, n=n)
    assert [i for i, v in enumerate(exp) if not v] == [i for i in BAD if i < n]


@pytest.mark.parametrize("l", [0, 1, 11])
def test_input_counts(ctx, key11, l):
    key = gr.Key(110 + l, l) if l != 11 else key11[0]
    vk = upload_key(ctx, key.alpha_beta(), *key.points()) if l != 11 else key11[1]
    bt = make_batch(ctx, key, 3, 120 + l, bad=(1,))
    try:
        assert vk.n_inputs == l
        assert bt.check(ctx, vk, (0, 1)) == [1, 0, 1]
    finally:
        bt.free()
        if l != 11:
            vk.free()


def test_fewer_inputs_than_the_key_has(ctx, key11):
    """n_inputs = 4 of 11 and n_inputs = 0: the missing inputs are zero, so proofs made for the padded statement are accepted, and the same
    proofs are rejected under all eleven inputs of another statement"""
    key, vk = key11
    for k in (4, 0):
        bt = make_batch(ctx, key, 3, 130 + k, bad=(2,), n_inputs=k)
        try:
            assert bt.check(ctx, vk, (0, 2)) == [1, 1, 0]
            full = [x + [0] * (11 - k) for x in bt.xs]
            assert list(ctx.groth16_verify(vk, bt.a, bt.b, bt.c, inputs_arr(full))) == [1, 1, 0]
            full[0][10] = 1
            assert list(ctx.groth16_verify(vk, bt.a, bt.b, bt.c, inputs_arr(full))) == [0, 1, 0]
        finally:
            bt.free()


def test_edge_scalars_and_acc_at_infinity(ctx):
    """input scalars 0, 1 and r - 1, 2^256 - 1 (not canonical: every window digit maximal, taken mod r by the group), and
    x_1 = -u_0 / u_1 with x_2 = 0, where acc is the point at infinity and its pair contributes one"""
    key = gr.Key(140, 2)
    vk = upload_key(ctx, key.alpha_beta(), *key.points())
    x_inf = (-key.u[0]) * pow(key.u[1], -1, R) % R
    xs = [[0, 0], [1, 1], [R - 1, R - 1], [(1 << 256) - 1, 1], [x_inf, 0], [x_inf, 0]]
    assert key.s(xs[4]) == 0
    scalars = [key.prove(x) for x in xs]
    scalars[5] = (scalars[5][0], scalars[5][1], (scalars[5][2] + 1) % R)
    bt = Batch(ctx, key, scalars, xs)
    try:
        assert bt.check(ctx, vk, range(6)) == [1, 1, 1, 1, 1, 0]
    finally:
        bt.free(), vk.free()


def test_points_at_infinity(ctx, key11):
    """A, B or C at infinity (a zero scalar): the pair contributes one and the value is still the model's"""
    key, vk = key11
    rnd = random.Random(150)
    xs = [[rnd.randrange(R) for _ in range(11)] for _ in range(5)]
    a, b, c = key.prove(xs[0])
    # with a = 0 the proof c = (-alpha beta - s gamma) / delta is accepted: e(A, B) = 1 there
    c4 = (-key.alpha * key.beta - key.s(xs[4]) * key.gamma) * pow(key.delta, -1, R) % R
    bt = Batch(ctx, key, [(0, b, c), (a, 0, c), (a, b, 0), (0, 0, 0), (0, b, c4)], xs)
    try:
        assert bt.check(ctx, vk, range(5)) == [0, 0, 0, 0, 1]
    finally:
        bt.free()


def test_malformed_points_are_rejected_alone(ctx, key11, batch130):
    """y + 1 in place of y, uploaded as host points, for A, B and C in turn: ok = 0 for that proof only, whatever the value is"""
    key, vk = key11
    n, first = 5, 1  # proofs 1 .. 5 of the batch: all accepted
    (A, _), (B, _), (C, _) = batch130.a.download(first, n), batch130.b.download(first, n), batch130.c.download(first, n)
    bump = lambda row, at: row.__setitem__(slice(at, at + 6), fq_limbs((sum(int(x) << (64 * i) for i, x in enumerate(row[at:at + 6])) + 1) % P))
    bump(A[0], 6), bump(B[2], 12), bump(C[4], 6)
    a, b, c = ctx.upload_bases(BLS, G1, A), ctx.upload_bases(BLS, G2, B), ctx.upload_bases(BLS, G1, C)
    try:
        assert list(ctx.groth16_verify(vk, a, b, c, inputs_arr(batch130.xs[first:first + n]))) == [0, 1, 0, 1, 0]
    finally:
        a.free(), b.free(), c.free()


def test_offsets_into_longer_objects(ctx, key11, batch130):
    assert batch130.check(ctx, key11[1], (0, 1, 4), offset=60, n=7) == [1, 1, 0, 0, 0, 1, 1]
    assert batch130.check(ctx, key11[1], (0,), offset=129, n=1) == [0]
    assert list(ctx.groth16_verify(key11[1], batch130.a, batch130.b, batch130.c, np.zeros((0, 0, 4), dtype=np.uint64), offset=130, n=0)) == []


def test_the_launch_count_does_not_depend_on_n(ctx, key11, batch130):
    counts = []
    ctx.profile(True)
    try:
        for n in (1, 130):
            ctx.profile_reset()
            batch130.check(ctx, key11[1], (), n=n)
            counts.append(ctx.profile_get("")[1])
    finally:
        ctx.profile(False)
    assert counts[0] == counts[1] == 3


def test_equals_the_host_twin_bit_for_bit(ctx, key11, batch130):
    key, vk = key11
    n = 65
    xs = batch130.xs[:n]
    ok, gt = ctx.groth16_verify(vk, batch130.a, batch130.b, batch130.c, inputs_arr(xs), n=n, want_gt=True)
    ints = lambda row, k: tuple(sum(int(x) << (64 * i) for i, x in enumerate(row[j * 6:(j + 1) * 6])) for j in range(k))
    A = [ints(r, 2) for r in batch130.a.download(0, n)[0]]
    B = [(lambda c: ((c[0], c[1]), (c[2], c[3])))(ints(r, 4)) for r in batch130.b.download(0, n)[0]]
    C = [ints(r, 2) for r in batch130.c.download(0, n)[0]]
    hok, hgt, _ = host_verify(ctypes.CDLL(SO), key.alpha_beta(), *key.points(), list(zip(A, B, C)), xs)
    assert hok == list(ok) and hgt == [gt_ints(g) for g in gt]


def test_refusals(zk, ctx, key11, batch130):
    """every error row of the header that one device can show (a key of another context's device needs two), before anything is launched: the
    profiler has counted no launch and the context works afterwards"""
    key, vk = key11
    bt = batch130
    pn = ctx.bases_from_scalars(1, G1, fr_arr([1, 2]))  # BN254
    L, h, z = ctx.lib, ctx.h, ctypes.c_size_t
    inp = inputs_arr(bt.xs[:4])
    ip = inp.ctypes.data_as(ctypes.c_void_p)
    ok = np.zeros(4, dtype=np.uint8)
    op = ok.ctypes.data_as(ctypes.c_void_p)
    V, A, B, C = vk.h, bt.a.h, bt.b.h, bt.c.h
    call = lambda ch, v, a, b, c, off, n, i, ni, o: L.zkhip_groth16_verify_batch(ch, v, a, b, c, z(off), z(n), i, z(ni), o, None)
    ab = np.array([l for v in key.alpha_beta() for l in fq_limbs(v)], dtype=np.uint64)
    q = np.zeros(24, dtype=np.uint64)
    abc = np.zeros((2, 12), dtype=np.uint64)
    out = ctypes.c_void_p()
    P_ = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    upload = lambda ch, curve, x, g, d, pts, n, o: L.zkhip_groth16_vk_upload(ch, curve, x, g, d, pts, None, z(n), o)
    rows = [
        ("null ctx", INVALID, lambda: call(None, V, A, B, C, 0, 4, ip, 11, op)),
        ("null vk", INVALID, lambda: call(h, None, A, B, C, 0, 4, ip, 11, op)),
        ("null a", INVALID, lambda: call(h, V, None, B, C, 0, 4, ip, 11, op)),
        ("null b", INVALID, lambda: call(h, V, A, None, C, 0, 4, ip, 11, op)),
        ("null c", INVALID, lambda: call(h, V, A, B, None, 0, 4, ip, 11, op)),
        ("null ok", INVALID, lambda: call(h, V, A, B, C, 0, 4, ip, 11, None)),
        ("null inputs", INVALID, lambda: call(h, V, A, B, C, 0, 4, None, 11, op)),
        ("G2 bases in the A slot", INVALID, lambda: call(h, V, B, B, C, 0, 4, ip, 11, op)),
        ("G1 bases in the B slot", INVALID, lambda: call(h, V, A, A, C, 0, 4, ip, 11, op)),
        ("G2 bases in the C slot", INVALID, lambda: call(h, V, A, B, B, 0, 4, ip, 11, op)),
        ("bases of another curve", INVALID, lambda: call(h, V, pn.h, B, C, 0, 2, ip, 11, op)),
        ("range one past the size", RANGE, lambda: call(h, V, A, B, C, 127, 4, ip, 11, op)),
        ("offset past the size", RANGE, lambda: call(h, V, A, B, C, 131, 0, ip, 11, op)),
        ("n wraps", RANGE, lambda: call(h, V, A, B, C, 2, (1 << 64) - 1, ip, 11, op)),
        ("more inputs than the key has", RANGE, lambda: call(h, V, A, B, C, 0, 4, ip, 12, op)),
        ("upload: BN254", INVALID, lambda: upload(h, 1, P_(ab), P_(q), P_(q), P_(abc), 2, ctypes.byref(out))),
        ("upload: Pallas", INVALID, lambda: upload(h, 2, P_(ab), P_(q), P_(q), P_(abc), 2, ctypes.byref(out))),
        ("upload: null ctx", INVALID, lambda: upload(None, BLS, P_(ab), P_(q), P_(q), P_(abc), 2, ctypes.byref(out))),
        ("upload: unknown curve", INVALID, lambda: upload(h, 7, P_(ab), P_(q), P_(q), P_(abc), 2, ctypes.byref(out))),
        ("upload: null delta", INVALID, lambda: upload(h, BLS, P_(ab), P_(q), None, P_(abc), 2, ctypes.byref(out))),
        ("upload: null points with n_abc > 0", INVALID, lambda: upload(h, BLS, P_(ab), P_(q), P_(q), None, 2, ctypes.byref(out))),
        ("upload: one input more than the limit", RANGE, lambda: upload(h, BLS, P_(ab), P_(q), P_(q), P_(abc), (1 << 15) + 2, ctypes.byref(out))),
        ("upload: null alpha_beta", INVALID, lambda: upload(h, BLS, None, P_(q), P_(q), P_(abc), 2, ctypes.byref(out))),
        ("upload: null gamma", INVALID, lambda: upload(h, BLS, P_(ab), None, P_(q), P_(abc), 2, ctypes.byref(out))),
        ("upload: null out", INVALID, lambda: upload(h, BLS, P_(ab), P_(q), P_(q), P_(abc), 2, None)),
        ("upload: n_abc = 0", RANGE, lambda: upload(h, BLS, P_(ab), P_(q), P_(q), P_(abc), 0, ctypes.byref(out))),
        ("n = 0", 0, lambda: call(h, V, A, B, C, 130, 0, None, 0, op)),
    ]
    try:
        L.zkhip_profile_enable(h, 1)
        L.zkhip_profile_reset(h)
        for name, code, fn in rows:
            assert fn() == code, name
        assert out.value is None
        ms, launches = ctypes.c_double(), ctypes.c_uint64()
        assert L.zkhip_profile_get(h, b"", ctypes.byref(ms), ctypes.byref(launches)) == 0 and launches.value == 0
        L.zkhip_profile_enable(h, 0)
        assert bt.check(ctx, vk, (0, 1), n=4) == [0, 1, 1, 1]
    finally:
        L.zkhip_profile_enable(h, 0)
        pn.free()
