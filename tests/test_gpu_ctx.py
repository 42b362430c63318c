"""The context itself (csrc/ctx.hpp, csrc/options.hpp): the options surface of zkhip_set_option / zkhip_get_option / ZKHIP_OPTIONS, the
life cycle of everything a context and a device group own -- created, used and destroyed several times over, with results that never
change --, and entry points that fail half-way and must leave the context usable."""
import numpy as np
import pytest

import cport as cp
import pyoracle as po
from util import CURVES, limbs, qap_domains

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
