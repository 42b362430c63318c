"""Operand generators for the arithmetic core (crypto3-zk_amd/csrc/fu.hpp, fu2_pair.hpp, msm_recode.hpp) at the edges of its written
contract, and the ctypes glue for the raw-limb entries zkt_fu_raw (host twin) and zkd_fu_raw (device).

Every generator asserts the precondition it claims to test, so an out-of-contract case can neither pass nor fail by accident.
Op numbers are those of csrc/arith_ops.h."""
import ctypes
import random

import numpy as np

import pyoracle as po

B = 29
MASK = (1 << B) - 1
# lazy 29-bit-limb types (hosttest.hip / arith_ops.h ids): modulus, limbs L, saturated words NL, largest spread K of field_consts.hpp
TYPES = {6: (po.BLS12_381.p, 14, 12, 128), 7: (po.BN254.p, 10, 8, 128), 8: (po.BLS12_381.r, 9, 8, 64), 9: (po.BN254.r, 9, 8, 128)}
OP_MUL, OP_SQR, OP_MUL2, OP_ADD, OP_COND_SUB, OP_CANON, OP_IS_ZERO, OP_INV, OP_INV_GCD, OP_PACK, OP_UNPACK = range(11)
# the element layer of the scalar-field kernels (fu.hpp: fu_mulm .. fu_load8); OP_IO8 and OP_POW_WIDE exist for the 8-word types only
OP_MULM, OP_ADDM, OP_FROM_MONT, OP_POW, OP_POW_ONTO, OP_IO8, OP_POW_WIDE = range(30, 37)
OP_REDUCE_SMALL = 37  # fu_reduce_small: the 9-limb scalar types only
# exponents of the 64-bit powers: 0 .. 3, 2^k and 2^k - 1 around the word boundary and at the top bit, all ones
POW_EXPONENTS = [0, 1, 2, 3] + [x for k in (31, 32, 33, 63) for x in (1 << k, (1 << k) - 1)] + [(1 << 64) - 1]


def op_sub(k):
    return 20 + k.bit_length() - 1


def spreads(t):
    return [1 << j for j in range(1, TYPES[t][3].bit_length())]


def split(x, L):
    """normalised limbs: lower limbs < 2^29, the top limb holds the rest"""
    assert x >= 0
    v = [(x >> (B * i)) & MASK for i in range(L - 1)] + [x >> (B * (L - 1))]
    assert v[-1] < 1 << 32
    return v


def value(v):
    return sum(int(x) << (B * i) for i, x in enumerate(v))


def normalised(v):
    return all(x <= MASK for x in v[:-1])


def denorm(v, i):
    """move 2^29 from limb i + 1 into limb i (value unchanged); keeps every limb < 2^30"""
    v = list(v)
    assert v[i + 1] >= 1 and v[i] + (1 << B) < 1 << 30
    v[i] += 1 << B
    v[i + 1] -= 1
    return v


def denorm_all(v):
    """every lower limb raised by 2^29 where it can be: the most carries any one input can hold under limbs < 2^30"""
    for i in range(len(v) - 2, -1, -1):
        if v[i + 1] >= 1 and v[i] + (1 << B) < 1 << 30:
            v = denorm(v, i)
    return v


def rp(t):
    p, L = TYPES[t][0], TYPES[t][1]
    return (1 << (B * L)) * p


def canonical_edges(t):
    """0, 1, 2, p-1, p-2, (p +- 1)/2, R mod p, R^2 mod p, 2^k mod p and p - 2^k at k = 29 i - 1, 29 i, 32 i"""
    p, L = TYPES[t][0], TYPES[t][1]
    R = 1 << (B * L)
    vals = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, R % p, R * R % p]
    for i in range(1, L + 1):
        for k in (B * i - 1, B * i, 32 * i):
            if k < p.bit_length():
                vals += [(1 << k) % p, p - (1 << k)]
    out = sorted(set(vals))
    assert all(0 <= x < p for x in out)
    return out


def mul_ok(t, a, b):
    """fu_mul / fu_canon / fu_inv operand contract: limbs < 2^30 on both inputs, a b < R p"""
    L = TYPES[t][1]
    assert len(a) == len(b) == L and all(0 <= x < 1 << 30 for x in a + b), (a, b)
    assert value(a) * value(b) < rp(t), (t, value(a), value(b))
    return a, b


def accumulator_pairs(t):
    """b: every limb but the top at 2^30 - 1; a: built greedily from the top limb down to (R p - 1) // b with limbs < 2^30 -- the
    products that fill the column accumulator the most under a b < R p (both orders)"""
    L = TYPES[t][1]
    out = []
    for top in (0, 1, 3):
        b = [(1 << 30) - 1] * (L - 1) + [top]
        budget = (rp(t) - 1) // value(b)
        a, rest = [0] * L, budget
        for i in range(L - 1, -1, -1):
            a[i] = min((1 << 30) - 1, rest >> (B * i))
            rest -= a[i] << (B * i)
        out += [mul_ok(t, a, b), mul_ok(t, b, a)]
    return out


def mul_cases(t, rng):
    p, L = TYPES[t][0], TYPES[t][1]
    R = 1 << (B * L)
    edges = canonical_edges(t)
    cases = [mul_ok(t, split(x, L), split(y, L)) for x in edges[:12] for y in (0, 1, p - 1, R % p)]
    cases += accumulator_pairs(t)
    # non-normalised operands below 2p (what a sum of two products holds before a carry pass is skipped), and at the bound's edge:
    # the largest a with a * a < R p, every lower limb denormalised
    big = _isqrt(rp(t) - 1)
    for x in [2 * p - 1, p + 1, big, big - 1] + [rng.randrange(2 * p) for _ in range(6)]:
        y = rng.randrange(2 * p)
        ax, ay = denorm_all(split(x, L)), split(y, L)
        if value(ax) * value(ay) < rp(t):
            cases.append(mul_ok(t, ax, ay))
        if value(ax) ** 2 < rp(t):
            cases.append(mul_ok(t, ax, denorm_all(split(x, L))))
        for i in range(L - 1):
            if split(x, L)[i + 1] >= 1 and value(ax) * value(ay) < rp(t):
                cases.append(mul_ok(t, denorm(split(x, L), i), ay))
    # large products: a b just below R p
    for _ in range(6):
        a = rng.randrange(p, R)
        b = (rp(t) - 1) // a
        cases.append(mul_ok(t, split(a, L), split(b, L)))
    return cases


def _isqrt(n):
    import math
    return math.isqrt(n)


def sqr_cases(t, rng):
    """fu_sqr: normalised limbs (< 2^29 including the top limb: the doubled operand must stay < 2^30), a^2 < R p"""
    p, L = TYPES[t][0], TYPES[t][1]
    top = _isqrt(rp(t) - 1)
    vals = canonical_edges(t) + [2 * p - 1, top, top - 1]
    vals += [rng.randrange(top) for _ in range(10)]
    out = []
    for x in vals:
        a = split(x, L)
        assert all(v <= MASK for v in a) and x * x < rp(t)
        out.append(a)
    return out


def mul2_cases(t, rng):
    """fu_mul2: normalised limbs, a b + c d < R p (cases just below it, in both halves)"""
    p, L = TYPES[t][0], TYPES[t][1]
    R = 1 << (B * L)
    out = []
    for _ in range(10):
        a, b = rng.randrange(R), rng.randrange(2 * p)
        if a * b >= rp(t):
            b = (rp(t) - 1) // a
        c = rng.randrange(p, R)
        d = (rp(t) - 1 - a * b) // c
        out.append((a, b, c, d))
    out += [(0, 0, R - 1, (rp(t) - 1) // (R - 1)), (R - 1, (rp(t) - 1) // (R - 1), 0, 0), (1, 1, 1, 1), (p - 1, p - 1, p - 1, p - 1)]
    res = []
    for a, b, c, d in out:
        v = [split(x, L) for x in (a, b, c, d)]
        assert all(x < R for x in (a, b, c, d)) and all(normalised(x) and x[-1] <= MASK for x in v) and a * b + c * d < rp(t)
        res.append(v)
    return res


def add_cases(t, rng):
    """fu_add: normalised inputs; sums up to 34 p (the largest a group-law formula forms)"""
    p, L = TYPES[t][0], TYPES[t][1]
    vals = [0, 1, p - 1, 2 * p - 1, 10 * p - 1, 17 * p, 18 * p - 1]
    out = []
    for a in vals:
        for b in (0, p - 1, 16 * p, 34 * p - 1 - a if a < 34 * p else 0):
            out.append((a, b))
    out += [(rng.randrange(16 * p), rng.randrange(16 * p)) for _ in range(6)]
    res = []
    for a, b in out:
        va, vb = split(a, L), split(b, L)
        assert normalised(va) and normalised(vb) and a + b < 1 << (B * L)
        res.append((va, vb))
    return res


def sub_cases(t, k, rng):
    """fu_sub<K>: b normalised with b <= (K - 1) p (the written bound, at it and below), a normalised"""
    p, L = TYPES[t][0], TYPES[t][1]
    out = []
    for b in (0, 1, p - 1, (k - 1) * p, (k - 1) * p - 1, rng.randrange((k - 1) * p + 1)):
        for a in (0, 1, 2 * p - 1, 34 * p - 1, rng.randrange(2 * p)):
            if a + k * p >= 1 << (B * L):  # the result must stay below R (BLS12-381 r: 64 p + 34 p does not)
                continue
            va, vb = split(a, L), split(b, L)
            assert normalised(va) and normalised(vb) and b <= (k - 1) * p and a + k * p - b < 1 << (B * L)
            out.append((va, vb))
    return out


def lt2p_cases(t, rng):
    """fu_cond_sub_p / fu_is_zero_lt2p: normalised, value < 2p"""
    p, L = TYPES[t][0], TYPES[t][1]
    vals = canonical_edges(t) + [p, p + 1, 2 * p - 1, 2 * p - 2] + [rng.randrange(2 * p) for _ in range(6)]
    out = []
    for x in vals:
        v = split(x, L)
        assert normalised(v) and x < 2 * p
        out.append(v)
    return out


def canon_cases(t, rng):
    """fu_canon: any value the product contract allows against R mod p: limbs < 2^30, a (R mod p) < R p"""
    p, L = TYPES[t][0], TYPES[t][1]
    R = 1 << (B * L)
    vals = canonical_edges(t) + [2 * p - 1, 34 * p - 1, 128 * p - 1 if 128 * p < R else 2 * p, R - 1] + [rng.randrange(R) for _ in range(6)]
    out = []
    for x in vals:
        for v in (split(x, L), denorm_all(split(x, L))):
            mul_ok(t, v, split(R % p, L))
            out.append(v)
    return out


def pack_cases(t, rng):
    """fu_pack: normalised limbs, value < 2^(32 NL); fu_unpack: any NL saturated words"""
    p, L, NL = TYPES[t][0], TYPES[t][1], TYPES[t][2]
    vals = canonical_edges(t) + [(1 << (32 * NL)) - 1] + [rng.randrange(1 << (32 * NL)) for _ in range(6)]
    out = []
    for x in vals:
        v = split(x, L)
        assert normalised(v) and x < 1 << (32 * NL)
        out.append(v)
    return out


def sat_words(x, L, NL):
    """x as NL saturated u32 words, zero-padded to L words (fu_unpack's input in an L-word slot)"""
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(NL)] + [0] * (L - NL)


def inv_cases(t, rng):
    """fu_inv: 0 < a, mul contract for a a; fu_inv_gcd: canonical, 0 < a < p"""
    p, L = TYPES[t][0], TYPES[t][1]
    vals = [x for x in canonical_edges(t) if x] + [rng.randrange(1, p) for _ in range(3)]
    out = []
    for x in vals:
        v = split(x, L)
        assert 0 < x < p and normalised(v)
        out.append(v)
    return out


def addm_cases(t, rng):
    """fu_addm: normalised operands, a + b < 2p -- the canonical edges against each other and add_cases' pairs that stay below 2p"""
    p, L = TYPES[t][0], TYPES[t][1]
    edges = canonical_edges(t)
    out = [(split(x, L), split(y, L)) for x in edges for y in (0, 1, p - 1, p - x if x else 0, edges[-1])]
    out += [(a, b) for a, b in add_cases(t, rng) if value(a) + value(b) < 2 * p]
    out += [(split(2 * p - 1, L), split(0, L)), (split(p, L), split(p - 1, L))]
    assert all(normalised(a) and normalised(b) and value(a) + value(b) < 2 * p for a, b in out)
    return out


def pow_cases(t, rng):
    """fu_pow_onto(seed, base, e) -- fu_pow is the seed R mod p: the products' operand contract along the whole chain, base base < R p,
    seed base < R p and seed < R / 2 (a later power of the base is < 2p).  (seed, base) from mul_cases' pairs at the product's bounds
    and the canonical edges; every pair meets every exponent of POW_EXPONENTS once over the list"""
    p, L = TYPES[t][0], TYPES[t][1]
    R = 1 << (B * L)
    pairs = [(b, a) for a, b in mul_cases(t, rng) if value(a) ** 2 < rp(t) and value(b) < R // 2]
    edges = canonical_edges(t)
    pairs += [(split(edges[(3 * i + 1) % len(edges)], L), split(x, L)) for i, x in enumerate(edges)]
    out = []
    for i, (seed, base) in enumerate(pairs):
        mul_ok(t, base, base)
        mul_ok(t, seed, base)
        assert value(seed) < R // 2
        for j in range(3):  # three exponents per pair, walking the list
            out.append((seed, base, POW_EXPONENTS[(3 * i + j) % len(POW_EXPONENTS)]))
    return out


def reduce_small_cases(t):
    """fu_reduce_small: normalised limbs, value < 64p.  k p + d for k = 0 .. 63 and d in {-1, 0, 1, p // 2, p - 1} (both sides of every multiple of
    p the quotient estimate has to tell apart); both ends t 2^248 and (t + 1) 2^248 - 1 of every value t of the estimate's 13-bit input x >> 248
    that a value below 64p can have; 64p - 1"""
    p, L = TYPES[t][0], TYPES[t][1]
    assert L == 9 and 1 << 248 < p < 1 << 255
    vals = {k * p + d for k in range(64) for d in (-1, 0, 1, p // 2, p - 1)}
    tops = range((64 * p - 1 >> 248) + 1)
    assert tops[-1] < 1 << 13
    vals |= {x for top in tops for x in (top << 248, (top + 1 << 248) - 1)}
    vals.add(64 * p - 1)
    out = []
    for x in sorted(v for v in vals if 0 <= v < 64 * p):
        v = split(x, L)
        assert normalised(v) and v[8] >> 16 == x >> 248
        out.append(v)
    assert len(out) > 6000 and value(out[-1]) == 64 * p - 1
    return out


def exp_words(e, L):
    """an exponent as saturated u32 words in an L-word operand slot"""
    assert e < 1 << 256
    return [(e >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [0] * (L - 8)


def scalar_edges(r, c, rng):
    """0, 1, (r - 1)/2, (r + 1)/2 (the fold boundary), r - 1, r, r + 1, 2^256 - 1, every window at 2^(c-1) for c-bit windows
    (uniform and the balanced cuts), random"""
    vals = [0, 1, 2, (r - 1) // 2, (r + 1) // 2, (r + 3) // 2, r - 1, r, r + 1, 2 * r - 1, (1 << 256) - 1]
    tb = r.bit_length()
    W = (tb + c - 1) // c
    offs = [w * tb // W for w in range(W + 1)]
    half_bal = sum(1 << (offs[w] + offs[w + 1] - offs[w] - 1) for w in range(W))  # every balanced window at 2^(width-1)
    half_uni = sum(1 << (c * w + c - 1) for w in range(W)) & ((1 << 256) - 1)
    for x in (half_bal, half_uni, half_bal + 1, half_bal - 1):
        vals += [x, r - x if x < r else x]
    vals += [rng.randrange(r) for _ in range(20)]
    return [v for v in vals if 0 <= v < 1 << 256]


# ---- ctypes glue ----------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def limbs_arr(rows, L):
    a = np.zeros((max(len(rows), 1), L), dtype=np.uint32)
    for i, v in enumerate(rows):
        a[i, :len(v)] = v
    return a


def run_raw(fn, t, op, a, b=None, c=None, d=None, size_t=True):
    """a, b, c, d: lists of limb lists (missing operands: zeros); returns (status, list of L-limb lists)"""
    L = TYPES[t][1] if t in TYPES else len(a[0])
    n = len(a)
    arrs = [limbs_arr(x if x is not None else [[0] * L] * n, L) for x in (a, b, c, d)]
    out = np.zeros((max(n, 1), L), dtype=np.uint32)
    nn = ctypes.c_size_t(n) if size_t else ctypes.c_int(n)
    rc = fn(t, op, nn, *[_ptr(x) for x in arrs], _ptr(out))
    return rc, [list(map(int, row)) for row in out[:n]]


def check_raw(t, op, a, b, c, d, r, k=None):
    """oracle residue + written postcondition of one raw-limb result; returns an error string or None"""
    p, L, NL = TYPES[t][0], TYPES[t][1], TYPES[t][2]
    R = 1 << (B * L)
    Ri = pow(R, -1, p)
    va = value(a)
    got = value(r)
    if op in (OP_MUL, OP_SQR, OP_MUL2):
        prod = {OP_MUL: lambda: va * value(b), OP_SQR: lambda: va * va, OP_MUL2: lambda: va * value(b) + value(c) * value(d)}[op]()
        if got % p != prod * Ri % p:
            return "residue"
        if not (normalised(r) and got < 2 * p):
            return "postcondition: normalised, < 2p"
    elif op == OP_ADD:
        if not (got == va + value(b) and normalised(r)):
            return "exact sum"
    elif 21 <= op <= 27:
        if not (got == va + k * p - value(b) and normalised(r)):
            return "exact a + Kp - b"
    elif op == OP_COND_SUB:
        if not (got == va % p and normalised(r)):
            return "canonical"
    elif op == OP_CANON:
        if not (got == va % p and normalised(r)):
            return "canonical"
    elif op == OP_IS_ZERO:
        if r != [1 if va % p == 0 else 0] + [0] * (L - 1):
            return "zero test"
    elif op == OP_INV:
        if not (got % p == R * R * pow(va, -1, p) % p and normalised(r) and got < 2 * p):
            return "inverse"
    elif op == OP_INV_GCD:
        if not (got == R * R * pow(va, -1, p) % p and normalised(r)):
            return "inverse (canonical)"
    elif op == OP_PACK:
        if not (r[NL:] == [0] * (L - NL) and sum(x << (32 * i) for i, x in enumerate(r[:NL])) == va):
            return "pack"
    elif op == OP_UNPACK:
        x = sum(int(w) << (32 * i) for i, w in enumerate(a[:NL]))
        if r != split(x, L):
            return "unpack"
    elif op == OP_MULM:
        if not (got == va * value(b) * Ri % p and normalised(r)):
            return "canonical product"
    elif op == OP_ADDM:
        if not (got == (va + value(b)) % p and normalised(r)):
            return "canonical sum"
    elif op == OP_FROM_MONT:
        if not (got == va * Ri % p and normalised(r)):
            return "out of Montgomery form"
    elif op in (OP_POW, OP_POW_ONTO, OP_POW_WIDE):
        e = sum(int(w) << (32 * i) for i, w in enumerate(b[:8 if op == OP_POW_WIDE else 2]))
        seed = c if op == OP_POW_ONTO else split(R % p, L)
        if got % p != value(seed) * pow(va * Ri % p, e, p) % p:
            return "power residue"
        if e == 0 and list(r) != list(seed):
            return "power: e = 0 leaves the seed as it is"
        if e and not (normalised(r) and got < 2 * p):
            return "postcondition: normalised, < 2p"
    elif op == OP_REDUCE_SMALL:
        if r != split(va % p, L):
            return "canonical limbs of x mod p"
    elif op == OP_IO8:
        if list(r) != list(a):
            return "16-byte store / load round trip"
    return None


def raw_suite(t, seed=0):
    """(op, K or None, [(a, b, c, d)]) for every raw op of type t"""
    rng = random.Random(seed * 100 + t)
    L, NL = TYPES[t][1], TYPES[t][2]
    z = [0] * L
    suite = [(OP_MUL, None, [(a, b, z, z) for a, b in mul_cases(t, rng)]),
             (OP_SQR, None, [(a, z, z, z) for a in sqr_cases(t, rng)]),
             (OP_MUL2, None, [tuple(v) for v in mul2_cases(t, rng)]),
             (OP_ADD, None, [(a, b, z, z) for a, b in add_cases(t, rng)]),
             (OP_COND_SUB, None, [(a, z, z, z) for a in lt2p_cases(t, rng)]),
             (OP_IS_ZERO, None, [(a, z, z, z) for a in lt2p_cases(t, rng)]),
             (OP_CANON, None, [(a, z, z, z) for a in canon_cases(t, rng)]),
             (OP_INV, None, [(a, z, z, z) for a in inv_cases(t, rng)[:6]]),
             (OP_INV_GCD, None, [(a, z, z, z) for a in inv_cases(t, rng)]),
             (OP_PACK, None, [(a, z, z, z) for a in pack_cases(t, rng)]),
             (OP_UNPACK, None, [(sat_words(value(a), L, NL), z, z, z) for a in pack_cases(t, rng)])]
    for k in spreads(t):
        suite.append((op_sub(k), k, [(a, b, z, z) for a, b in sub_cases(t, k, rng)]))
    powers = pow_cases(t, rng)
    suite += [(OP_MULM, None, [(a, b, z, z) for a, b in mul_cases(t, rng)]),
              (OP_ADDM, None, [(a, b, z, z) for a, b in addm_cases(t, rng)]),
              (OP_FROM_MONT, None, [(a, z, z, z) for a in canon_cases(t, rng)]),
              (OP_POW, None, [(base, exp_words(e, L), z, z) for _, base, e in powers]),
              (OP_POW_ONTO, None, [(base, exp_words(e, L), seed, z) for seed, base, e in powers])]
    if L == 9:
        suite.append((OP_REDUCE_SMALL, None, [(a, z, z, z) for a in reduce_small_cases(t)]))
    if NL == 8:
        p = TYPES[t][0]
        wide = [p - 1, 0, 1, 1 << 64, (1 << 64) + 1, (1 << 256) - 1]
        suite += [(OP_IO8, None, [(a, z, z, z) for a in pack_cases(t, rng)]),
                  (OP_POW_WIDE, None, [(split(x, L), exp_words(e, L), z, z) for e in wide for x in canonical_edges(t)[:12 if e == p - 1 else 3]])]
    return suite
