"""Shared helpers for the tests: canonical-limb conversions between Python ints and numpy arrays."""
import numpy as np
import pyoracle as po

CURVES = {0: po.BLS12_381, 1: po.BN254}
FQ_LIMBS = {0: 6, 1: 4}


def limbs(v, n):
    return np.array(po.to_limbs(v, n), dtype=np.uint64)


def fr_arr(vals):
    return np.array([po.to_limbs(v, 4) for v in vals], dtype=np.uint64).reshape(len(vals), 4)


def fr_ints(arr):
    return [po.from_limbs(x) for x in np.asarray(arr).reshape(-1, 4)]


def pt_limbs(curve, group, P):
    """affine point (python) -> flat canonical limbs; None -> zeros"""
    L = FQ_LIMBS[curve]
    if P is None:
        return np.zeros(2 * L * group, dtype=np.uint64)
    if group == 1:
        return np.concatenate([limbs(P[0], L), limbs(P[1], L)])
    return np.concatenate([limbs(P[0][0], L), limbs(P[0][1], L), limbs(P[1][0], L), limbs(P[1][1], L)])


def pts_arr(curve, group, pts):
    return np.stack([pt_limbs(curve, group, P) for P in pts]) if len(pts) else np.zeros((0, 2 * FQ_LIMBS[curve] * group), dtype=np.uint64)


def pt_from_limbs(curve, group, a, inf=0):
    if inf:
        return None
    L = FQ_LIMBS[curve]
    a = np.asarray(a).reshape(-1)
    f = lambda i: po.from_limbs(a[i * L:(i + 1) * L])
    if group == 1:
        return (f(0), f(1))
    return ((f(0), f(1)), (f(2), f(3)))


def jac_to_affine_py(curve, group, jac):
    """Jacobian canonical limbs (3, coord) -> python affine point via big-int inversion (checker side)."""
    C = CURVES[curve]
    G = C.g1 if group == 1 else C.g2
    L = FQ_LIMBS[curve]
    jac = np.asarray(jac).reshape(3, -1)

    def coord(row):
        if group == 1:
            return po.from_limbs(row[:L])
        return (po.from_limbs(row[:L]), po.from_limbs(row[L:2 * L]))

    return G.to_affine((coord(jac[0]), coord(jac[1]), coord(jac[2])))


def group_of(curve, group):
    C = CURVES[curve]
    return C.g1 if group == 1 else C.g2


def qap_domains(zkmod, curve, min_size, two_adicity=None):
    """make_evaluation_domain(min_size) twice: pyoracle's EvaluationDomain and the zkhip_domain describing the same"""
    C = CURVES[curve]
    dom = po.make_evaluation_domain(C, min_size, two_adicity=two_adicity)
    zd = zkmod.zkhip.Domain.make(dom.kind, dom.m, limbs(dom.omega, 4), limbs(dom.shift, 4))
    return dom, zd


def lookup_instance(C, rng, log_n, k_in, k_val, big_inputs=()):
    """A genuine lookup instance in the shape prepare_lookup_value / prepare_lookup_input leave behind: every (theta-compressed) table
    column is zero at row 0, holds distinct non-zero values (one of them repeated in adjacent rows) in the rows after it, zero behind and
    zero from usable_rows on (the mask); every input takes table values (or zero) in the usable rows and anything behind them.  Inputs
    listed in big_inputs live on the 2n-point domain (an expression of degree > 1): f + c (X^n - 1), which reduces to f."""
    r = C.r
    n = 1 << log_n
    usable = n - 3
    values, pool = [], [0]
    for i in range(k_val):
        T = usable // 2 + i
        col = [0] * n
        prev = 0
        for j in range(1, T + 1):
            prev = prev if (j == 3 and prev) else rng.next_mod(r - 1) + 1
            col[j] = prev
            pool.append(prev)
        values.append(col)
    inputs = []
    for i in range(k_in):
        f = [pool[rng.next_mod(len(pool))] for _ in range(usable)] + [rng.next_mod(r) for _ in range(n - usable)]
        if i in big_inputs:
            big = po.dfs_resize(f, 2 * n, C.root_of_unity, r)
            c = rng.next_mod(r)
            f = [(v - 2 * c * (j & 1)) % r for j, v in enumerate(big)]
        inputs.append(f)
    return inputs, values, usable


def permutation_instance(C, rng, log_n, k, usable):
    """A genuine copy-constraint instance in placeholder's shape: the k columns are constant along the cycles of a random permutation of
    the k * usable cells of the usable rows; the rows behind them are blinding (random values, identity permutation), so the grand
    product closes AT usable: V_P[usable] = 1.  -> (columns, S_id, S_sigma)"""
    r = C.r
    n = 1 << log_n
    w, delta = C.root_of_unity(log_n), C.fr_generator
    labels = [[pow(delta, i, r) * pow(w, j, r) % r for j in range(n)] for i in range(k)]
    cells = [(i, j) for i in range(k) for j in range(usable)]
    perm = list(cells)
    for a in range(len(perm) - 1, 0, -1):            # Fisher-Yates with the test's generator
        b = rng.next_mod(a + 1)
        perm[a], perm[b] = perm[b], perm[a]
    sigma = dict(zip(cells, perm))
    val, seen = {}, set()
    for c in cells:
        if c in seen:
            continue
        v, x = rng.next_mod(r), c
        while x not in seen:
            seen.add(x)
            val[x] = v
            x = sigma[x]
    cols = [[val[(i, j)] if j < usable else rng.next_mod(r) for j in range(n)] for i in range(k)]
    S_sigma = [[labels[sigma[(i, j)][0]][sigma[(i, j)][1]] if j < usable else labels[i][j] for j in range(n)] for i in range(k)]
    return cols, labels, S_sigma


EVAL_POLYS_CASE_LOGS = (3, 3, 5, 3, 4)


def eval_polys_case(C, seed):
    """tests/cpp/eval_polys_case.hpp: five polynomials of 2^3, 2^3, 2^5, 2^3, 2^4 random evaluations, batch 0 = the first four opened at
    {a, b}, {b}, {a, b, c}, {c, a}, batch 2 = the last opened at a.  -> (evaluations as limbs, a | b | c as limbs, the expected proof.z in
    (batch, polynomial, point) order: the coefficient forms by the oracle's inverse transform, evaluated by po.poly_eval)"""
    r = C.r
    rng = po.SplitMix64(seed)
    a, b, c = (rng.next_mod(r) for _ in range(3))
    polys = [[rng.next_mod(r) for _ in range(1 << lg)] for lg in EVAL_POLYS_CASE_LOGS]
    sets = [[a, b], [b], [a, b, c], [c, a], [a]]
    want = []
    for lg, e, s in zip(EVAL_POLYS_CASE_LOGS, polys, sets):
        coeffs = po.intt(e, C.root_of_unity(lg), r)
        want += [po.poly_eval(coeffs, x, r) for x in s]
    return fr_arr([v for e in polys for v in e]), fr_arr([a, b, c]), want


def fr_vector_cases(r, n, seed):
    """tests/cpp/fr_vector_case.hpp: every member of fr_vector over vectors of n elements whose first entries are 0, 1, r - 1 (b: the same
    three rotated to 1, r - 1, 0, so that a - b runs below zero at index 0 and 1) and random ones behind, plus the cases whose sizes are
    the contract's own.  Yields (label, what, a, b, n, scalars, m, flag, want): the entry's arguments as Python integers and the expected
    output, computed here from Python integers alone."""
    rng = po.SplitMix64(seed)
    rand = lambda k: [rng.next_mod(r) for _ in range(k)]                                # noqa: E731
    nonzero = lambda k: [1 + rng.next_mod(r - 1) for _ in range(k)]                       # noqa: E731
    a = ([0, 1, r - 1] + rand(n))[:n]
    b = ([1, r - 1, 0] + rand(n))[:n]
    assert a[0] < b[0]
    yield "add", 0, a, b, n, [], 0, 0, [(x + y) % r for x, y in zip(a, b)]
    yield "sub", 1, a, b, n, [], 0, 0, [(x - y) % r for x, y in zip(a, b)]
    yield "mul", 2, a, b, n, [], 0, 0, [x * y % r for x, y in zip(a, b)]
    s = rand(3)
    yield "affine with y", 3, a, b, n, s, 0, 1, [(s[0] * x + s[1] * y + s[2]) % r for x, y in zip(a, b)]
    yield "affine without y", 3, a, b, n, s, 0, 0, [(s[0] * x + s[2]) % r for x in a]
    for c in (0, 1, r - 1):
        yield "scale by %d" % c, 4, a, [], n, [c], 0, 0, [c * x % r for x in a]
    for c, accumulate in ((s[0], 0), (s[1], 1), (r - 1, 1)):
        acc = nonzero(n + 3)
        yield "add_scaled", 6, a, acc, n, [c], n + 3, accumulate, [((acc[j] if accumulate else 0) + (c * a[j] if j < n else 0)) % r for j in range(n + 3)]
    fill = nonzero(n + 1)
    yield "copy", 9, a, fill, n, [], 0, 0, a + fill[n:]
    for length in (0, 5, 8):
        src, dst = nonzero(length), nonzero(8)
        yield "zero_padded_copy %d -> 8" % length, 5, src, dst, length, [], 8, 0, src + [0] * (8 - length)
    for log_n in (6, 3):
        v = rand(1 << log_n)
        yield "subsample 2^%d -> 2^3" % log_n, 7, v, [], log_n, [], 3, 0, v[::1 << (log_n - 3)]
    z, q = rng.next_mod(r), rand(4)
    at_root = [(-z * q[0]) % r] + [(q[k - 1] - z * q[k]) % r for k in range(1, 4)] + [q[3]]    # (X - z) q(X), degree 4
    for f in (at_root, rand(5)):
        quotient = [0] * 4
        for k in range(3, -1, -1):
            quotient[k] = (f[k + 1] + (z * quotient[k + 1] if k < 3 else 0)) % r
        remainder = (f[0] + z * quotient[0]) % r
        assert (f is at_root) == (remainder == 0) and (f is not at_root or quotient == q)
        yield "div_linear", 8, f, [], 5, [z], 0, 0, [remainder] + quotient + [remainder]


def run_fr_vector_cases(entry, curve, r, n, seed):
    """every case of fr_vector_cases through `entry` (shim_fr_vector / pasta_fr_vector of the C++ harnesses)"""
    import ctypes
    arr = lambda v: fr_arr(v) if v else np.zeros((1, 4), dtype=np.uint64)                  # noqa: E731
    for label, what, a, b, count, scalars, m, flag, want in fr_vector_cases(r, n, seed):
        out = np.full((len(want), 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        ins = [np.ascontiguousarray(arr(v)) for v in (a, b, scalars)]
        rc = entry(curve, what, *(x.ctypes.data_as(ctypes.c_void_p) for x in ins[:2]), ctypes.c_size_t(count), ins[2].ctypes.data_as(ctypes.c_void_p),
                   ctypes.c_size_t(m), flag, out.ctypes.data_as(ctypes.c_void_p))
        assert rc == 0, (label, rc)
        assert fr_ints(out) == want, label
