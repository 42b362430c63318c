"""A Python restatement of commitments::kimchi_pedersen<CurveType> (zk/commitments/polynomial/kimchi_pedersen.hpp): `commitment`
(:334-383), `proof_eval` (:385-559, the generators folded point by point), `combined_inner_product` (:561-609), `b_poly` (:611-627),
`b_poly_coefficents` (:629-643) and the verifier's equation (:645-755), over pyoracle's Group and plain integers mod r.

Everything the reference draws or squeezes is explicit here: `Draws` hands out a given list of scalars in the order the reference calls
algebra::random_element, `Transcript` is a stand-in sponge that answers challenge_fq / squeeze_challenge from a given list and records
every call with its argument, and the group map is a fixed point.  The scheme's algebra does not depend on WHICH challenges come, so a
proof made with these satisfies the verifier's equation exactly when the arithmetic is right.

Points are affine tuples, None is the point at infinity; a commitment is (unshifted list, shifted or None), its blinders likewise;
bound = -1 means "no degree bound" as in the reference (where poly_type_single::bound is a size_t, so -1 is the largest value and the
opening's `bound >= 0` branch is the only one ever taken: restated as it stands)."""
import pyoracle as po

NO_BOUND = (1 << 64) - 1  # std::size_t bound = -1


class Draws:
    """algebra::random_element<scalar_field_type>() in call order"""

    def __init__(self, values):
        self.values, self.pos = list(values), 0

    def next(self):
        v = self.values[self.pos]
        self.pos += 1
        return v


class Transcript:
    """the calls kimchi_pedersen makes on its sponge, answered from a list; log = [(name, argument or None), ...]"""

    def __init__(self, answers):
        self.answers, self.pos, self.log = list(answers), 0, []

    def _answer(self):
        v = self.answers[self.pos]
        self.pos += 1
        return v

    def absorb_fr(self, x):
        self.log.append(("absorb_fr", x))

    def absorb_g(self, P):
        self.log.append(("absorb_g", P))

    def challenge_fq(self):
        self.log.append(("challenge_fq", None))
        return self._answer()

    def squeeze_challenge(self, endo_r):
        self.log.append(("squeeze_challenge", endo_r))
        return self._answer()


def splitmix_scalars(seed, count, r):
    """`count` non-zero scalars below 2^252 (below every modulus here, so no reduction is involved) from the oracle's SplitMix64"""
    rng = po.SplitMix64(seed)
    out = []
    while len(out) < count:
        v = rng.next_mod(1 << 252)
        if v:
            out.append(v % r)
    return out


class Params:
    def __init__(self, G, r, g, h, endo_r=0, u_point=None, shift_scalar=None):
        self.G, self.r, self.g, self.h, self.endo_r = G, r, list(g), h, endo_r
        self.u_point = u_point if u_point is not None else G.mul(G.gen, 0x1234567)  # group_map.to_group: a fixed point
        self.shift_scalar = shift_scalar or (lambda x: (x + 1) % r)             # the caller's (kimchi_functions); any map serves the model

    def to_group(self, t):
        return self.u_point


def msm(G, pts, scalars):
    """multiexp over as many terms as the shorter of the two ranges holds"""
    m = min(len(pts), len(scalars))
    return po.msm_naive(G, pts[:m], scalars[:m])


def inner_product(a, b, r):
    return sum(x * y for x, y in zip(a, b)) % r


def commitment(pp, poly, bound, draws):
    """:334-383 -> ((unshifted, shifted), (unshifted blinders, shifted blinder or None))"""
    G, r, g = pp.G, pp.r, pp.g
    n = len(g)
    unshifted, left, length = [], 0, len(poly)
    while length > n:
        unshifted.append(msm(G, g, poly[left:left + n]))
        left += n
        length -= n
    if length > 0:
        unshifted.append(msm(G, g[:length], poly[left:left + length]))
    shifted = None
    if bound >= 0:
        start = bound - bound % n
        if any(c % r for c in poly) and start < len(poly):
            shifted = msm(G, g[n - bound % n:], poly[start:])
    blind_unshifted = []
    for i in range(len(unshifted)):
        w = draws.next()
        unshifted[i] = G.add(unshifted[i], G.mul(pp.h, w))
        blind_unshifted.append(w)
    w = draws.next()  # drawn whether or not a shifted part exists (:375)
    blind_shifted = None
    if shifted is not None:
        shifted = G.add(shifted, G.mul(pp.h, w))
        blind_shifted = w
    return (unshifted, shifted), (blind_unshifted, blind_shifted)


def combine_polynomials(pp, plms, polyscale):
    """the vector a (length |g|, before padding) and the blinding factor of proof_eval (:403-456); plms = [(coeffs, bound, blinders)]"""
    r, n = pp.r, len(pp.g)
    a = [0] * n
    blinding, scale = 0, 1
    for coeffs, bound, (blind_unshifted, blind_shifted) in plms:
        bnd = NO_BOUND if bound < 0 else bound
        offset, j = 0, 0
        while j < len(blind_unshifted):
            segment = coeffs[offset:min(offset + n, len(coeffs))]
            for i, c in enumerate(segment):
                a[i] = (a[i] + c * scale) % r
            blinding = (blinding + blind_unshifted[j] * scale) % r
            j += 1
            scale = scale * polyscale % r
            offset += n
            if offset > bnd:
                for i, c in enumerate(segment):
                    a[i + n - len(segment)] = (a[i + n - len(segment)] + c * scale) % r
                blinding = (blinding + (blind_shifted or 0) * scale) % r
                scale = scale * polyscale % r
    return a, blinding


def powers_lincomb(points, scales, n, r):
    """b[i] = sum_e scales[e] * points[e]^i (:460-470)"""
    b = [0] * n
    for e, s in zip(points, scales):
        spare = 1
        for i in range(n):
            b[i] = (b[i] + s * spare) % r
            spare = spare * e % r
    return b


def proof_eval(pp, plms, elm, polyscale, evalscale, sponge, draws):
    """:385-559 -> {"lr": [(L, R)], "delta", "z1", "z2", "sg"}"""
    G, r = pp.G, pp.r
    n = len(pp.g)
    p2 = 1
    while p2 < n:
        p2 <<= 1
    g = list(pp.g) + [None] * (p2 - n)
    a, blinding = combine_polynomials(pp, plms, polyscale)
    a = a + [0] * (p2 - n)
    scales, s = [], 1
    for _ in elm:
        scales.append(s)
        s = s * evalscale % r
    b = powers_lincomb(elm, scales, p2, r)
    sponge.absorb_fr(pp.shift_scalar(inner_product(a, b, r)))
    u = pp.to_group(sponge.challenge_fq())
    chals, chal_invs, blinders, lr = [], [], [], []
    while p2 > 1:
        p2 >>= 1
        g_lo, g_hi, a_lo, a_hi, b_lo, b_hi = g[:p2], g[p2:], a[:p2], a[p2:], b[:p2], b[p2:]
        rand_l, rand_r = draws.next(), draws.next()
        L = G.add(G.add(msm(G, g_lo, a_hi), G.mul(pp.h, rand_l)), G.mul(u, inner_product(a_hi, b_lo, r)))
        R = G.add(G.add(msm(G, g_hi, a_lo), G.mul(pp.h, rand_r)), G.mul(u, inner_product(a_lo, b_hi, r)))
        lr.append((L, R))
        blinders.append((rand_l, rand_r))
        sponge.absorb_g(L)
        sponge.absorb_g(R)
        c = sponge.squeeze_challenge(pp.endo_r)
        ci = pow(c, r - 2, r)
        chals.append(c)
        chal_invs.append(ci)
        a = [(hi * ci + lo) % r for hi, lo in zip(a_hi, a_lo)]
        b = [(hi * c + lo) % r for hi, lo in zip(b_hi, b_lo)]
        g = [G.add(G.mul(hi, c), lo) for hi, lo in zip(g_hi, g_lo)]
    a0, b0, g0 = a[0], b[0], g[0]
    r_prime = blinding
    for (bl, br), c, ci in zip(blinders, chals, chal_invs):
        r_prime = (r_prime + bl * ci + br * c) % r
    d, r_delta = draws.next(), draws.next()
    delta = G.add(G.mul(G.add(g0, G.mul(u, b0)), d), G.mul(pp.h, r_delta))
    sponge.absorb_g(delta)
    c = sponge.squeeze_challenge(pp.endo_r)
    return {"lr": lr, "delta": delta, "z1": (a0 * c + d) % r, "z2": (c * r_prime + r_delta) % r, "sg": g0}


def poly_eval(coeffs, x, r):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % r
    return acc


def chunk_evaluations(coeffs, n, points, r):
    """evaluation_type::evaluations of a polynomial: [point][chunk] -> chunk(point), chunks of n coefficients"""
    chunks = [coeffs[i:i + n] for i in range(0, len(coeffs), n)]
    return [[poly_eval(ch, x, r) for ch in chunks] for x in points]


def combined_inner_product(points, xi, rr, polys, g_size, r):
    """:561-609; polys = [(evaluations[point][chunk], bound or -1)]"""
    res, xi_i = 0, 1
    for evaluations, bound in polys:
        evals = [[evaluations[j][i] for j in range(len(evaluations))] for i in range(len(evaluations[0]))] if evaluations else []
        for ev in evals:
            res = (res + xi_i * poly_eval(ev, rr, r)) % r
            xi_i = xi_i * xi % r
        if bound != -1:
            last = [0] * len(points)
            if bound <= len(evals) * g_size:
                last = evals[-1]
            shifted = [pow(points[i], g_size - bound % g_size, r) * last[i] % r for i in range(len(last))]
            res = (res + xi_i * poly_eval(shifted, rr, r)) % r
            xi_i = xi_i * xi % r
    return res


def b_poly(chals, x, r):
    """:611-627"""
    k = len(chals)
    pow_twos = [x % r]
    for _ in range(1, k):
        pow_twos.append(pow_twos[-1] * pow_twos[-1] % r)
    res = 1
    for i in range(k):
        res = res * (1 + chals[i] * pow_twos[k - 1 - i]) % r
    return res


def b_poly_coefficients(chals, r):
    """:629-643"""
    rounds = len(chals)
    s = [1] * (1 << rounds)
    k, pw = 0, 1
    for i in range(1, 1 << rounds):
        if i == pw:
            k += 1
            pw <<= 1
        s[i] = s[i - (pw >> 1)] * chals[rounds - 1 - (k - 1)] % r
    return s


def verifier_terms(pp, batches, draws):
    """the points and scalars verify_eval hands to its one multiexp (:645-755).  A batch is a dict: sponge (a Transcript in the state
    the prover's had before proof_eval), evaluation = [(commit, evaluations, bound)], evaluation_points, xi, r, opening."""
    r, n = pp.r, len(pp.g)
    p2 = 1
    while p2 < n:
        p2 <<= 1
    points = [pp.h] + list(pp.g) + [None] * (p2 - n)
    scalars = [0] * (p2 + 1)
    rand_base, sg_rand_base = draws.next(), draws.next()
    rb_i, sg_i = 1, 1
    for batch in batches:
        sponge, opening = batch["sponge"], batch["opening"]
        es = [(evaluations, bound if commit[1] is not None else -1) for commit, evaluations, bound in batch["evaluation"]]
        cip = combined_inner_product(batch["evaluation_points"], batch["xi"], batch["r"], es, n, r)
        sponge.absorb_fr(pp.shift_scalar(cip))
        u = pp.to_group(sponge.challenge_fq())
        chals, chal_invs = [], []
        for L, R in opening["lr"]:
            sponge.absorb_g(L)
            sponge.absorb_g(R)
            chals.append(sponge.squeeze_challenge(pp.endo_r))
            chal_invs.append(pow(chals[-1], r - 2, r))
        sponge.absorb_g(opening["delta"])
        c = sponge.squeeze_challenge(pp.endo_r)
        scale, b0 = 1, 0
        for e in batch["evaluation_points"]:
            b0 = (b0 + scale * b_poly(chals, e, r)) % r
            scale = scale * batch["r"] % r
        s = b_poly_coefficients(chals, r)
        neg_rb = -rb_i % r
        points.append(opening["sg"])
        scalars.append((neg_rb * opening["z1"] - sg_i) % r)
        for i, v in enumerate(s):
            scalars[i + 1] = (scalars[i + 1] + v * sg_i) % r
        scalars[0] = (scalars[0] - rb_i * opening["z2"]) % r
        scalars.append(neg_rb * opening["z1"] % r * b0 % r)
        points.append(u)
        rb_c = c * rb_i % r
        for (L, R), ch, chi in zip(opening["lr"], chals, chal_invs):
            points += [L, R]
            scalars += [rb_c * chi % r, rb_c * ch % r]
        xi_i = 1
        for commit, _, bound in batch["evaluation"]:
            for comm in commit[0]:
                scalars.append(rb_c * xi_i % r)
                points.append(comm)
                xi_i = xi_i * batch["xi"] % r
            if bound >= 0 and commit[1] is not None:
                scalars.append(rb_c * xi_i % r)
                points.append(commit[1])
                xi_i = xi_i * batch["xi"] % r
        scalars.append(rb_c * cip % r)
        points.append(u)
        scalars.append(rb_i)
        points.append(opening["delta"])
        rb_i = rb_i * rand_base % r
        sg_i = sg_i * sg_rand_base % r
    return points, scalars


def verify_eval(pp, batches, draws):
    points, scalars = verifier_terms(pp, batches, draws)
    return msm(pp.G, points, scalars) is None
