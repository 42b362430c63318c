"""The context itself (csrc/ctx.hpp, csrc/options.hpp): the options surface of zkhip_set_option / zkhip_get_option / ZKHIP_OPTIONS, the
life cycle of everything a context and a device group own -- created, used and destroyed several times over, with results that never
change --, and entry points that fail half-way and must leave the context usable."""
import ctypes

import numpy as np
import pytest

import cport as cp
import pyoracle as po
from util import CURVES, fr_arr, fr_ints, limbs, qap_domains

pytestmark = pytest.mark.gpu

# the defaults, as literals (csrc/ctx.hpp declares them; nothing here is read from the library)
DEFAULTS = {
    "msm_window_bits": 0, "msm_segment_log": -1, "msm_sets": 0, "msm_tail_quads": 1, "msm_tail_fold": 16, "msm_fold_run": 0,
    "msm_tail_fold_g2": 1, "msm_share_sort": 1, "ec_ntt_table_lanes": 0, "msm_sort_tile_log": 14, "ntt_radix_log": 8, "ntt_tile_log": 3,
    "ntt_pair": 1, "poly_coset_extend": 1, "msm_precompute": 1, "msm_precompute_min": 32, "msm_shard_world": 1, "msm_shard_rank": 0,
    "msm_graphs": 0, "alloc_cache_mb": 16384, "stream_priority": 0,
}
# the options that are stored as given (truncated to int)
PLAIN = ["msm_window_bits", "msm_segment_log", "msm_sets", "msm_tail_quads", "msm_tail_fold", "msm_fold_run", "msm_tail_fold_g2", "msm_share_sort",
         "msm_sort_tile_log", "ntt_radix_log", "ntt_tile_log", "ntt_pair", "msm_precompute", "msm_precompute_min", "msm_graphs"]
INVALID, RANGE = "invalid argument", "size or offset out of range"


def test_option_defaults_round_trips_and_quirks(zk, monkeypatch):
    monkeypatch.delenv("ZKHIP_OPTIONS", raising=False)
    assert len(DEFAULTS) == 21
    c = zk.Context(0)
    try:
        for name, value in DEFAULTS.items():
            assert c.get_option(name) == value, name
        for k, name in enumerate(PLAIN):
            value = DEFAULTS[name] + 3 + k
            c.set_option(name, value)
            assert c.get_option(name) == value, name
        for name in PLAIN:    # nothing else moved
            c.set_option(name, DEFAULTS[name])
        for name, value in DEFAULTS.items():
            assert c.get_option(name) == value, name
        c.set_option("msm_sets", (1 << 32) + 7)    # truncated to int
        assert c.get_option("msm_sets") == 7
        c.set_option("msm_sets", 0)
        c.set_option("poly_coset_extend", 5)
        assert c.get_option("poly_coset_extend") == 1
        c.set_option("poly_coset_extend", 0)
        assert c.get_option("poly_coset_extend") == 0
        c.set_option("ec_ntt_table_lanes", -1)
        assert c.get_option("ec_ntt_table_lanes") == 0
        c.set_option("ec_ntt_table_lanes", 1 << 30)
        assert c.get_option("ec_ntt_table_lanes") == 1 << 24
        c.set_option("ec_ntt_table_lanes", 4096)
        assert c.get_option("ec_ntt_table_lanes") == 4096
        for bad in (0, 65):
            with pytest.raises(zk.ZkhipError, match=RANGE):
                c.set_option("msm_shard_world", bad)
        assert c.get_option("msm_shard_world") == 1
        c.set_option("msm_shard_world", 4)
        c.set_option("msm_shard_rank", 3)
        assert (c.get_option("msm_shard_world"), c.get_option("msm_shard_rank")) == (4, 3)
        for bad in (4, -1):
            with pytest.raises(zk.ZkhipError, match=RANGE):
                c.set_option("msm_shard_rank", bad)
        c.set_option("msm_shard_world", 2)
        assert (c.get_option("msm_shard_world"), c.get_option("msm_shard_rank")) == (2, 0)
        c.set_option("msm_shard_world", 1)
        with pytest.raises(zk.ZkhipError, match=RANGE):
            c.set_option("alloc_cache_mb", -1)
        assert c.get_option("alloc_cache_mb") == 16384
        p = c.malloc(1 << 20)    # a block enters the cache, a smaller cap sends it back
        c.free(p)
        c.set_option("alloc_cache_mb", 0)
        assert c.get_option("alloc_cache_mb") == 0
        c.set_option("alloc_cache_mb", 64)
        assert c.get_option("alloc_cache_mb") == 64
        c.set_option("stream_priority", -1)    # the context's own stream is recreated; the context keeps working
        assert c.get_option("stream_priority") == -1
        w = limbs(po.BLS12_381.root_of_unity(4), 4)
        a = cp.random_fr(0, 3, 16).reshape(1, 16, 4)
        assert (c.ntt(0, a, 4, w) == cp.ntt(0, a, 4, w)).all()
        c.set_option("stream_priority", 0)
        for name in ("bogus", "", "msm_sets ", "opt_msm_sets"):
            with pytest.raises(zk.ZkhipError, match=INVALID):
                c.set_option(name, 1)
            with pytest.raises(zk.ZkhipError, match=INVALID):
                c.get_option(name)
    finally:
        c.close()


def test_options_from_the_environment(zk, monkeypatch):
    monkeypatch.setenv("ZKHIP_OPTIONS", "ntt_pair=0,bogus=1,msm_sets=2")
    c = zk.Context(0)
    try:
        assert c.get_option("ntt_pair") == 0 and c.get_option("msm_sets") == 2
        for name, value in DEFAULTS.items():
            if name not in ("ntt_pair", "msm_sets"):
                assert c.get_option(name) == value, name
    finally:
        c.close()
    monkeypatch.setenv("ZKHIP_OPTIONS", ",=4,ntt_pair,msm_shard_world=99,,msm_tail_fold=0")    # malformed and refused entries are skipped
    c = zk.Context(0)
    try:
        assert c.get_option("msm_tail_fold") == 0
        for name, value in DEFAULTS.items():
            if name != "msm_tail_fold":
                assert c.get_option(name) == value, name
    finally:
        c.close()


N_PTS = 64


@pytest.fixture(scope="module")
def small():
    """64 BLS12-381 G1 points and scalars, a 2^4 vector and a step-domain vector, with the oracle's results (computed once)"""
    C = po.BLS12_381
    pts, inf = cp.batch_mul(0, 1, cp.random_fr(0, 71, N_PTS))
    sc = cp.random_fr(0, 72, N_PTS)
    msm = cp.msm(0, 1, pts, sc, chunks=2)
    w = limbs(C.root_of_unity(4), 4)
    a = cp.random_fr(0, 73, 16).reshape(1, 16, 4)
    return dict(pts=pts, inf=inf, sc=sc, msm=msm, w=w, a=a, ntt=cp.ntt(0, a, 4, w))


def test_context_and_group_life_cycle(zk, small):
    """Everything a context owns is created, used and released, four times over: the staging buffer of host scalars, window tables and the
    workspace (zkhip_msm), NTT tables, the domain scratch and a domain table (a step domain), the ordering event (zkhip_stream_wait), the
    profiler's events.  Then a captured graph that goes with its context, and a group of two members over the peer and the staged
    transport.  Every result equals the oracle's, every round."""
    dom, zd = qap_domains(zk, 0, 20)
    assert dom.kind == zk.zkhip.DOMAIN_STEP
    v = cp.random_fr(0, 74, dom.m).reshape(1, dom.m, 4)
    want_fft = cp.domain_fft(0, dom.kind, v[0], limbs(dom.omega, 4), limbs(dom.shift, 4))
    want_aff, want_inf = small["msm"]
    for rnd in range(4):
        c, other = zk.Context(0), zk.Context(0)
        c.profile(True)
        b = c.upload_bases(0, 1, small["pts"], small["inf"])
        jac = c.msm(b, small["sc"])
        assert (c.ntt(0, small["a"], 4, small["w"]) == small["ntt"]).all(), rnd
        assert (c.domain_fft(0, zd, v)[0] == want_fft).all(), rnd
        assert c.lib.zkhip_stream_wait(c.h, other.h) == 0 and c.lib.zkhip_stream_wait(other.h, c.h) == 0
        aff, inf = c.jacobian_to_affine(0, 1, jac)
        assert inf == want_inf and (aff == want_aff).all(), rnd
        assert c.profile_get("")[1] > 0
        b.free()
        c.close()
        other.close()
    # a graph is captured at the third identical call, replayed at the fourth and destroyed with the context
    c = zk.Context(0)
    c.set_option("msm_graphs", 1)
    b = c.upload_bases(0, 1, small["pts"], small["inf"])
    d_s, d_o = c.malloc(N_PTS * 32), c.malloc(3 * 48)
    c.h2d(d_s, small["sc"])
    for k in range(4):
        c.h2d(d_o, np.zeros(18, dtype=np.uint64))
        c.msm_dev(b, d_s, d_o)
        jac = np.zeros((3, 6), dtype=np.uint64)
        c.d2h(jac, d_o)
        aff, inf = c.jacobian_to_affine(0, 1, jac)
        assert inf == want_inf and (aff == want_aff).all(), k
    b.free()
    c.close()
    for transport in (zk.zkhip.GROUP_PEER, zk.zkhip.GROUP_STAGED):
        g = zk.DeviceGroup([0, 0])
        g.set_transport(transport)
        gb = g.upload_bases(0, 1, small["pts"], small["inf"])
        aff, inf = g.msm_affine(gb, small["sc"])
        assert g.transport() == transport and inf == want_inf and (aff == want_aff).all(), transport
        gb.free()
        g.close()


def test_r1cs_upload_out_of_range_leaves_the_context_usable(zk, ctx):
    curve, M, n = 0, 16, 2
    C = CURVES[curve]
    g16 = cp.Groth16(curve, M, n, seed=3)
    a, b, c = g16.csr(0), g16.csr(1), g16.csr(2)
    col = np.array(b[1], dtype=np.uint32)
    col[len(col) // 2] = g16.N + 1    # one column index beyond the variables
    for _ in range(2):
        with pytest.raises(zk.ZkhipError, match=RANGE):
            ctx.upload_r1cs(curve, g16.M, g16.n, g16.N, a, (b[0], col, b[2]), c)
    r1cs = ctx.upload_r1cs(curve, g16.M, g16.n, g16.N, a, b, c)
    dom, zd = qap_domains(zk, curve, M + n + 1)
    assert (r1cs.kind, r1cs.m) == (dom.kind, dom.m)
    w, gen = limbs(dom.omega, 4), limbs(C.fr_generator, 4)
    if dom.kind != 0:
        g16.set_domain(dom.kind, dom.m, w)
    z = np.concatenate([np.array([[1, 0, 0, 0]], dtype=np.uint64), g16.assignment()])
    assert (ctx.groth16_witness_h(r1cs, z, w, gen) == g16.witness_map(w, gen)).all()
    r1cs.free()


def test_bases_spread_out_of_range_leaves_the_context_usable(zk, ctx):
    curve, group, n, first = 1, 1, 1 << 13, 11
    tail = ctx.bases_from_scalars(curve, group, cp.random_fr(curve, 23, n - first))
    for _ in range(2):
        with pytest.raises(zk.ZkhipError, match=RANGE):
            tail.spread(n, first=first + 1)    # first + its size > n_total
    # a row list whose last row lies beyond the end is found by the kernel, after the object was allocated: the call builds the object (without
    # that point), the sticky status word reports the row, and the object is released like any other
    rows = np.arange(first, n, dtype=np.uint32)
    rows[-1] = n
    d_rows = ctx.malloc(rows.nbytes)
    ctx.h2d(d_rows, rows)
    flawed = tail.spread(n, d_rows=d_rows)
    with pytest.raises(zk.ZkhipError, match=RANGE):
        ctx.device_status()
    assert ctx.device_status() == 0
    flawed.free()
    ctx.free(d_rows)
    spread = tail.spread(n, first=first)
    sc = cp.random_fr(curve, 24, n)
    aff, inf = ctx.msm_affine(spread, sc)
    aff_t, inf_t = ctx.msm_affine(tail, np.ascontiguousarray(sc[first:]))
    pts, _ = tail.download()
    exp, einf = cp.msm(curve, group, pts, np.ascontiguousarray(sc[first:]), chunks=2)
    assert inf == inf_t == einf and (aff == exp).all() and (aff_t == exp).all()
    spread.free()
    tail.free()


# ---- per-call host tables (csrc/ctx.hpp: ws_upload) and the entry preamble (ZK_ARGS / ZK_ENTER) ----------------------------------------
def _dev(ctx, vals):
    d = ctx.malloc(len(vals) * 32)
    ctx.h2d(d, fr_arr(vals))
    return d


def _back(ctx, d, n):
    out = np.zeros((n, 4), dtype=np.uint64)
    ctx.d2h(out, d)
    return fr_ints(out)


@pytest.mark.parametrize("curve", [0, 1])
def test_back_to_back_pointer_tables(ctx, curve):
    """fr_vec_prod with table A (3 inputs), at once again with table B (2 other inputs), then poly_lincomb (2 polynomials, 2 taps): no
    synchronisation in between, every result against big integers.  The second table must not reach the first call's kernel."""
    r, n = CURVES[curve].r, 1 << 10
    v = [fr_ints(cp.random_fr(curve, 900 + i, n)) for i in range(5)]
    d = [_dev(ctx, x) for x in v]
    d_a, d_b, d_acc = ctx.malloc(n * 32), ctx.malloc(n * 32), ctx.malloc((n + 1) * 32)
    cs = [[po.SplitMix64(910 + 2 * i + t).next_mod(r) for t in range(2)] for i in range(2)]
    ctx.fr_vec_prod_dev(curve, d[:3], d_a, n)
    ctx.fr_vec_prod_dev(curve, d[3:], d_b, n)
    ctx.poly_lincomb_dev(curve, [d[0], d[4]], [n, n], fr_arr([x for c in cs for x in c]), 2, d_acc, n + 1, False)
    assert _back(ctx, d_a, n) == [a * b % r * c % r for a, b, c in zip(v[0], v[1], v[2])]
    assert _back(ctx, d_b, n) == [a * b % r for a, b in zip(v[3], v[4])]
    exp = [0] * (n + 1)
    for p, c in zip((v[0], v[4]), cs):
        for t in range(2):
            for j, x in enumerate(p):
                exp[j + t] = (exp[j + t] + c[t] * x) % r
    assert _back(ctx, d_acc, n + 1) == exp
    for p in d + [d_a, d_b, d_acc]:
        ctx.free(p)


def _vp(p):
    return ctypes.c_void_p(p)


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_callers_arrays_die_on_return(zk, ctx):
    """perm_factor_products (k = 2, n = 2^10) and gate_eval (log_size 6): the host-side argument arrays are overwritten as soon as the call
    has returned, before anything is downloaded"""
    curve, k, n = 0, 2, 1 << 10
    r = CURVES[curve].r
    v = [fr_ints(cp.random_fr(curve, 930 + i, n)) for i in range(3 * k)]
    d = [_dev(ctx, x) for x in v]
    d_g, d_h = ctx.malloc(n * 32), ctx.malloc(n * 32)
    beta, gamma = po.SplitMix64(940).next_mod(r), po.SplitMix64(941).next_mod(r)

    def call_and_scribble():
        tabs = [(ctypes.c_void_p * k)(*d[i * k:(i + 1) * k]) for i in range(3)]
        b, g = limbs(beta, 4), limbs(gamma, 4)
        rc = ctx.lib.zkhip_perm_factor_products_dev(ctx.h, curve, ctypes.c_size_t(k), *tabs, ctypes.c_size_t(n), _hp(b), _hp(g), _vp(d_g), _vp(d_h))
        for t in tabs:
            ctypes.memset(t, 0x5a, ctypes.sizeof(t))
        b[:] = 0
        g[:] = 0
        return rc

    assert call_and_scribble() == 0
    cols, sid, ssig = v[:k], v[k:2 * k], v[2 * k:]
    want = lambda s: [(cols[0][j] + beta * s[0][j] + gamma) * (cols[1][j] + beta * s[1][j] + gamma) % r for j in range(n)]
    assert _back(ctx, d_g, n) == want(sid) and _back(ctx, d_h, n) == want(ssig)

    # the smallest program of test_gate_eval_flat_program's kind: one gate with a selector, two terms, rotations of both signs
    log_size, size = 6, 64
    c0 = po.SplitMix64(950).next_mod(r)
    keep = [np.array([0, 2], dtype=np.uint32), np.array([2], dtype=np.uint32), np.array([1], dtype=np.int32), np.array([0, 2, 3], dtype=np.uint32),
            np.array([0, 1, 1], dtype=np.uint32), np.array([0, 1, -1], dtype=np.int32), fr_arr([c0, r - 1])]
    prog = zk.zkhip.GateProgram(1, 2, 3, 3, *[_hp(a) for a in keep])
    slots = (ctypes.c_void_p * 3)(*d[:3])
    d_out = ctx.malloc(size * 32)
    rc = ctx.lib.zkhip_gate_eval_dev(ctx.h, curve, ctypes.byref(prog), slots, ctypes.c_size_t(log_size), None, 0, _vp(d_out))
    for a in keep:
        a[...] = 0x33
    ctypes.memset(slots, 0x5a, ctypes.sizeof(slots))
    ctypes.memset(ctypes.byref(prog), 0, ctypes.sizeof(prog))
    assert rc == 0
    x = [c[:size] for c in v[:3]]
    assert _back(ctx, d_out, size) == [(c0 * x[0][j] * x[1][(j + 1) % size] - x[1][(j - 1) % size]) * x[2][(j + 1) % size] % r for j in range(size)]
    for p in d + [d_g, d_h, d_out]:
        ctx.free(p)


def _preamble_calls(zk, c, curve, d, zero):
    """(name, call) for every entry point that takes a curve id; zero: an empty call with null buffers, else a small well-formed one over d"""
    L, h, z = c.lib, c.h, ctypes.c_size_t
    one = limbs(1, 4)
    w4 = limbs(CURVES[0].root_of_unity(4), 4)
    dom = zk.zkhip.Domain.make(zk.zkhip.DOMAIN_BASIC, 16, w4)
    p = None if zero else _vp(d)
    cnt = z(0 if zero else 16)
    tab = (ctypes.c_void_p * 1)(None if zero else d)
    lens = (ctypes.c_size_t * 1)(16)
    out = np.zeros(64, dtype=np.uint64)
    rp = np.zeros(2, dtype=np.uint32)
    prog = zk.zkhip.GateProgram(0, 0, 0, 0, *([None] * 7))
    hdl = ctypes.c_void_p()
    calls = [
        ("fr_vec_op", lambda: L.zkhip_fr_vec_op_dev(h, curve, 0, p, p, p, cnt)),
        ("fr_vec_affine", lambda: L.zkhip_fr_vec_affine_dev(h, curve, p, None, _hp(one), None, _hp(one), p, cnt)),
        ("fr_vec_mul_div", lambda: L.zkhip_fr_vec_mul_div_dev(h, curve, p, p, p, p, cnt)),
        ("fr_vec_prod", lambda: L.zkhip_fr_vec_prod_dev(h, curve, z(1), tab, p, cnt)),
        ("poly_eval", lambda: L.zkhip_poly_eval_dev(h, curve, p, z(16), z(16), z(0 if zero else 1), _hp(one), z(1), _hp(out))),
        ("poly_div_linear", lambda: L.zkhip_poly_div_linear_dev(h, curve, p, cnt, _hp(one), p, _hp(out))),
        ("poly_div_vanishing", lambda: L.zkhip_poly_div_vanishing_dev(h, curve, p, cnt, z(4), p, None)),
        ("poly_lincomb", lambda: L.zkhip_poly_lincomb_dev(h, curve, z(1), tab, lens, _hp(one), z(1), p, cnt, 0)),
        ("poly_resize", lambda: L.zkhip_poly_resize_dev(h, curve, p, z(4), z(0 if zero else 1), _hp(w4), p, z(4), _hp(w4))),
        ("perm_grand_product", lambda: L.zkhip_perm_grand_product_dev(h, curve, z(1), tab, tab, tab, cnt, _hp(one), _hp(one), None, None, p)),
        ("perm_factor_products", lambda: L.zkhip_perm_factor_products_dev(h, curve, z(1), tab, tab, tab, cnt, _hp(one), _hp(one), p, p)),
        ("lookup_grand_product", lambda: L.zkhip_lookup_grand_product_dev(h, curve, z(1), tab, z(1), tab, z(2), (ctypes.c_void_p * 2)(*([None] * 2 if zero else [d, d])),
                                                                          cnt, z(0 if zero else 8), _hp(one), _hp(one), p)),
        ("domain_fft", lambda: L.zkhip_domain_fft_dev(h, curve, ctypes.byref(dom), p, z(0 if zero else 1), 0, None)),
    ]
    if not zero:    # these have no empty form: a call with an unknown curve only
        calls += [
            ("fri_fold", lambda: L.zkhip_fri_fold_dev(h, curve, p, z(4), _hp(one), _hp(w4), p)),
            ("gate_eval", lambda: L.zkhip_gate_eval_dev(h, curve, ctypes.byref(prog), None, z(4), None, 0, p)),
            ("domain_lagrange", lambda: L.zkhip_domain_lagrange_dev(h, curve, ctypes.byref(dom), _hp(one), p)),
            ("ntt_dev", lambda: L.zkhip_ntt_dev(h, curve, p, z(4), z(1), _hp(w4), 0, None)),
            ("ntt", lambda: L.zkhip_ntt(h, curve, _hp(out), z(4), z(1), _hp(w4), 0, None)),
            ("ec_ntt", lambda: L.zkhip_ec_ntt_dev(h, curve, 1, p, z(2), _hp(w4), 0)),
            ("jacobian_sum", lambda: L.zkhip_jacobian_sum_dev(h, curve, 1, p, z(1), p)),
            ("jacobian_to_affine", lambda: L.zkhip_jacobian_to_affine(h, curve, 1, _hp(out), _hp(out), _hp(out))),
            ("bases_upload", lambda: L.zkhip_bases_upload(h, curve, 1, _hp(out), None, z(1), ctypes.byref(hdl))),
            ("bases_upload_compressed", lambda: L.zkhip_bases_upload_compressed(h, curve, 1, _hp(out), z(1), ctypes.byref(hdl))),
            ("bases_from_scalars", lambda: L.zkhip_bases_from_scalars(h, curve, 1, None, _hp(out), z(1), ctypes.byref(hdl))),
            ("r1cs_upload", lambda: L.zkhip_r1cs_upload(h, curve, z(1), z(0), z(1), _hp(rp), None, None, _hp(rp), None, None, _hp(rp), None, None, ctypes.byref(hdl))),
        ]
    return calls


@pytest.mark.parametrize("zero", [False, True], ids=["unknown_curve", "empty_call"])
def test_entry_preamble(zk, zero):
    """Every entry point that takes a curve id refuses curve = 7 (ZKHIP_ERR_INVALID = -2); an empty call -- count, n or batch 0, null
    buffers -- returns ZKHIP_OK.  Neither launches a kernel: the profiler, which records every launch, has counted none."""
    c = zk.Context(0)
    try:
        d = c.malloc(1 << 16)
        c.h2d(d, np.zeros(1 << 13, dtype=np.uint64))
        c.profile(True)
        for name, call in _preamble_calls(zk, c, 0 if zero else 7, d, zero):
            assert call() == (0 if zero else -2), name
        assert c.profile_get("")[1] == 0
        c.profile(False)
        w = limbs(po.BLS12_381.root_of_unity(4), 4)    # and the context works afterwards
        a = cp.random_fr(0, 3, 16).reshape(1, 16, 4)
        assert (c.ntt(0, a, 4, w) == cp.ntt(0, a, 4, w)).all()
    finally:
        c.close()
