"""zkhip_fri_query_dev and zkhip_merkle_paths_multi (crypto3-zk_amd/csrc/merkle.hip) through the Python view: the answers against a Python
restatement of calculate_s over the uploaded arrays (fri_query_ref) and against the oracle's leaf layout (cport.fri_leaves), the paths against
zkhip_merkle_paths per tree and against hashlib (merkle_ref).  Every comparison is bit-exact."""
import ctypes
import random

import numpy as np
import pytest

import cport as cp
import fri_query_ref as fq
import merkle_ref as mr
from util import CURVES, limbs

pytestmark = pytest.mark.gpu

INVALID, RANGE = -2, -5


class _Dev:
    """device blocks of one test, freed on exit"""

    def __init__(self, ctx):
        self.ctx, self.blocks = ctx, []

    def __enter__(self):
        return self

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.ctx.malloc(max(1, arr.nbytes))
        self.blocks.append(p)
        self.ctx.h2d(p, arr)
        return p

    def __exit__(self, *exc):
        for p in self.blocks:
            self.ctx.free(p)


def _edge_mix(curve, seed, n):
    """n elements: random ones with 0, 1, r - 1 and all-ones limbs strewn in (the gather must not care what a value is)"""
    a = cp.random_fr(curve, seed, n).reshape(n, 4)
    edge = [limbs(0, 4), limbs(1, 4), limbs(CURVES[curve].r - 1, 4), np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)]
    for k in range(0, n, 5):
        a[k] = edge[(k // 5) % 4]
    return a


def _polys(seed, batch, log_d):
    return _edge_mix(seed & 1, seed, batch << log_d).reshape(batch, 1 << log_d, 4)


def _check_set(polys, step, xs, got):
    """one set's answers: the restated walk, and the oracle's leaf -- a permutation of leaf x mod (D >> step), its order when x is below"""
    batch, D = polys.shape[0], polys.shape[1]
    assert got.shape == (len(xs), batch, 1 << (step - 1), 2, 4)
    assert np.array_equal(got, fq.expected_answers(polys, step, xs))
    leaves = cp.fri_leaves(list(polys), step).reshape(D >> step, batch, 1 << (step - 1), 2, 4)
    for k, x in enumerate(xs):
        x = int(x) % D
        leaf = leaves[x % (D >> step)]
        assert np.array_equal(fq.leaf_order(got[k], x, D, step), leaf), (step, x)
        if x < D >> step:
            assert np.array_equal(got[k], leaf), (step, x)


@pytest.mark.parametrize("log_d,steps,batch", [(1, [1], 1), (3, [3], 1), (5, [1, 2, 3, 4], 3)])
def test_fri_query_every_x(ctx, log_d, steps, batch):
    """the pair wrap at D/2 (D = 2), one leaf holding the whole domain (step = log_domain), the offset walk and the min / max order"""
    polys = _polys(6100 + log_d, batch, log_d)
    xs = np.arange(1 << log_d, dtype=np.uint64)
    with _Dev(ctx) as dev:
        d = dev.upload(polys)
        for step in steps:
            (got,) = ctx.fri_query([(d, log_d, batch, step)], xs)
            _check_set(polys, step, xs, got)


def test_fri_query_many_workgroups_and_repeats(ctx):
    """log_domain 12, step 2, batch 7, 257 queries with repeats: 7196 output elements, more than one workgroup"""
    log_d, batch, step = 12, 7, 2
    polys = _polys(6200, batch, log_d)
    rng = random.Random(12)
    xs = [0, (1 << log_d) - 1, 5, 5, 5] + [rng.randrange(1 << log_d) for _ in range(252)]
    assert len(xs) == 257
    with _Dev(ctx) as dev:
        (got,) = ctx.fri_query([(dev.upload(polys), log_d, batch, step)], xs)
    _check_set(polys, step, np.array(xs, dtype=np.uint64), got)


def test_fri_query_three_sets_in_one_call(ctx):
    """(log_domain, batch, step) = (10, 4, 1), (9, 1, 2), (7, 1, 1), indices up to 2^10 - 1: every set reduces the index by its own domain, and
    the call equals three single calls over the indices reduced by hand"""
    shapes = [(10, 4, 1), (9, 1, 2), (7, 1, 1)]
    rng = random.Random(3)
    xs = np.array([1023, 0, 512, 511, 128, 127] + [rng.randrange(1024) for _ in range(30)], dtype=np.uint64)
    data = [_polys(6300 + k, b, ld) for k, (ld, b, s) in enumerate(shapes)]
    with _Dev(ctx) as dev:
        sets = [(dev.upload(p), ld, b, s) for p, (ld, b, s) in zip(data, shapes)]
        got = ctx.fri_query(sets, xs)
        singles = [ctx.fri_query([st], xs % np.uint64(1 << st[1]))[0] for st in sets]
    assert len(got) == 3
    for p, (ld, b, s), g, one in zip(data, shapes, got, singles):
        _check_set(p, s, xs, g)
        assert np.array_equal(g, one)


def test_fri_query_offsets_past_64_mb(ctx):
    """log_domain 21, batch 2, step 1: the second polynomial starts 64 MB into the set, the last index reads its last element"""
    log_d, batch = 21, 2
    D = 1 << log_d
    polys = cp.random_fr(0, 6400, batch * D).reshape(batch, D, 4)
    rng = random.Random(21)
    xs = np.array([D - 1, 0, D // 2, D // 2 - 1] + [rng.randrange(D) for _ in range(60)], dtype=np.uint64)
    with _Dev(ctx) as dev:
        (got,) = ctx.fri_query([(dev.upload(polys), log_d, batch, 1)], xs)
    assert got.shape == (64, batch, 1, 2, 4)
    assert np.array_equal(got, fq.expected_answers(polys, 1, xs))


def test_fri_query_return_codes(ctx, zk):
    lib, h = ctx.lib, ctx.h
    sz, vp = ctypes.c_size_t, ctypes.c_void_p
    FriQuerySet = zk.zkhip.FriQuerySet
    polys = _polys(6500, 2, 3)
    want = fq.expected_answers(polys, 2, [5])
    idx = np.array([5], dtype=np.uint64)
    out = np.zeros((1, 2, 2, 2, 4), dtype=np.uint64)
    with _Dev(ctx) as dev:
        d = dev.upload(polys)

        def call(sets, n_sets, indices, count, o, handle=h):
            table = (FriQuerySet * max(1, len(sets)))(*[FriQuerySet(*s) for s in sets]) if sets is not None else None
            return lib.zkhip_fri_query_dev(handle, table, sz(n_sets), indices.ctypes.data_as(vp) if indices is not None else None, sz(count),
                                           o.ctypes.data_as(vp) if o is not None else None)

        good = [(d, 3, 2, 2)]
        cases = [
            (call(good, 1, idx, 0, out), 0),                       # nothing to do
            (call(good, 0, idx, 1, out), 0),
            (call(None, 0, None, 0, None), 0),
            (call(good, 1, idx, 1, out, handle=None), INVALID),    # null pointers
            (call(None, 1, idx, 1, out), INVALID),
            (call(good, 1, None, 1, out), INVALID),
            (call(good, 1, idx, 1, None), INVALID),
            (call([(None, 3, 2, 2)], 1, idx, 1, out), INVALID),
            (call([(d, 3, 0, 2)], 1, idx, 1, out), INVALID),       # batch 0
            (call([(d, 3, 2, 0)], 1, idx, 1, out), RANGE),         # step 0
            (call([(d, 3, 2, 4)], 1, idx, 1, out), RANGE),         # step > log_domain
            (call([(d, 33, 2, 1)], 1, idx, 1, out), RANGE),
            (call(good, 1, np.array([8], dtype=np.uint64), 1, out), RANGE),    # an index equal to D
            (call([(d, 32, 2, 32)], 1, idx, 1 << 31, out), RANGE),  # 2^31 queries x 2^33 elements: the product wraps 64 bits; refused before an index is read
            (call(good + [(d, 2, 1, 1)], 2, np.array([7, 8], dtype=np.uint64), 2, np.zeros((64, 4), dtype=np.uint64)), RANGE),
        ]
        for k, (rc, expect) in enumerate(cases):
            assert rc == expect, (k, rc)
        assert not out.any()                                        # nothing was written by any of them
        assert call(good, 1, idx, 1, out) == 0 and np.array_equal(out, want)    # the context still answers


def _tree_of(ctx, dev, seed, log_l, per_leaf):
    L = 1 << log_l
    leaves = _edge_mix(0, seed, L * per_leaf)
    return ctx.merkle_build(dev.upload(leaves), L, per_leaf), mr.tree(leaves, L)


def test_merkle_paths_multi_equals_single_trees(ctx):
    """trees of 1, 2 and 2^9 leaves in one call: tree-major, byte for byte zkhip_merkle_paths per tree over the reduced indices, and the
    siblings hashlib's digest array holds; the one-leaf tree contributes nothing"""
    rng = random.Random(9)
    xs = np.array([0, 511, 511, 1, 256] + [rng.randrange(512) for _ in range(28)], dtype=np.uint64)
    with _Dev(ctx) as dev:
        built = [_tree_of(ctx, dev, 6600 + k, log_l, per) for k, (log_l, per) in enumerate([(0, 3), (1, 2), (9, 5)])]
        trees = [t for t, _ in built]
        got = ctx.merkle_paths_multi(trees, xs)
        assert [g.shape for g in got] == [(len(xs), 0, 32), (len(xs), 1, 32), (len(xs), 9, 32)]
        for (t, digests), g in zip(built, got):
            reduced = xs % np.uint64(t.leaves)
            assert np.array_equal(g, t.paths(reduced))
            for k, i in enumerate(reduced):
                assert np.array_equal(g[k], mr.path_from_digests(digests, t.leaves, int(i)))
        # return codes: null pointers are invalid, an empty call is fine and writes nothing
        lib, h, vp, sz = ctx.lib, ctx.h, ctypes.c_void_p, ctypes.c_size_t
        handles = (vp * 3)(*[t.h for t in trees])
        buf = np.zeros(len(xs) * 10 * 32, dtype=np.uint8)
        P = lambda a: a.ctypes.data_as(vp)
        assert lib.zkhip_merkle_paths_multi(h, handles, sz(3), P(xs), sz(0), P(buf)) == 0
        assert lib.zkhip_merkle_paths_multi(h, handles, sz(0), P(xs), sz(len(xs)), P(buf)) == 0
        assert not buf.any()
        assert lib.zkhip_merkle_paths_multi(None, handles, sz(3), P(xs), sz(len(xs)), P(buf)) == INVALID
        assert lib.zkhip_merkle_paths_multi(h, None, sz(3), P(xs), sz(len(xs)), P(buf)) == INVALID
        assert lib.zkhip_merkle_paths_multi(h, (vp * 3)(trees[0].h, None, trees[2].h), sz(3), P(xs), sz(len(xs)), P(buf)) == INVALID
        assert lib.zkhip_merkle_paths_multi(h, handles, sz(3), None, sz(len(xs)), P(buf)) == INVALID
        assert lib.zkhip_merkle_paths_multi(h, handles, sz(3), P(xs), sz(len(xs)), None) == INVALID
        assert not buf.any()
        assert np.array_equal(ctx.merkle_paths_multi(trees, xs)[2], got[2])
        for t in trees:
            t.free()


def test_answers_hash_to_the_leaf_the_path_opens(ctx):
    """the two entries tied up: for a tree from zkhip_merkle_build_fri_dev (log_domain 8, batch 3, step 2) the answered values, put into
    leaf order and hashed, lead along the answered path to the root -- for every x"""
    log_d, batch, step = 8, 3, 2
    D = 1 << log_d
    polys = _polys(6700, batch, log_d)
    xs = np.arange(D, dtype=np.uint64)
    with _Dev(ctx) as dev:
        d = dev.upload(polys)
        t = ctx.merkle_build_fri(d, log_d, batch, step)
        (values,) = ctx.fri_query([(d, log_d, batch, step)], xs)
        (paths,) = ctx.merkle_paths_multi([t], xs)
        root = t.root()
        t.free()
    for x in range(D):
        leaf = x % (D >> step)
        assert mr.root_from_path(mr.element_bytes(fq.leaf_order(values[x], x, D, step)), leaf, paths[x]) == root, x
