"""A definition-level model of the compressed BLS12-381 point encoding (include/zkhip.h, "the WIRE form"; csrc/wire.hip; the ZCash
convention) and constructors for the encodings that uniformly random keys never produce.

The model extracts no square root.  `classify` reads the flag bits and the range of x, `on_curve` decides by Euler's criterion whether
x^3 + b is a square, and `check_decoded` takes a decoded point and verifies the three facts that determine it: its x is the encoded x,
y^2 = x^3 + b, and the 0x20 flag says whether y is the larger of {y, -y}.  An x has at most two y, so nothing else is left to choose --
and neither the kernel's nor pyoracle's "complex method" (with its a1 == 0 arms and its choice between (a0 + s)/2 and (a0 - s)/2) is
restated here.  Square roots are taken in the constructors only (to FIND an x with a wanted property; p = 3 mod 4), and every constructor
asserts the property it claims to deliver, so a case can neither pass nor fail by accident.

Fq2 = Fq[u]/(u^2 + 1); an element is the tuple (c0, c1); a G2 x travels as x.c1 then x.c0.  A point is (x, y) or None (infinity), as in
pyoracle."""
import pyoracle as po

P = po.BLS12_381.p
HALF = (P - 1) // 2
assert P % 4 == 3 and P % 3 == 1


# ---- Fq2 in big integers
def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_pow(a, e):
    r = (1, 0)
    for bit in bin(e)[2:]:
        r = f2_mul(r, r)
        if bit == "1":
            r = f2_mul(r, a)
    return r


def f2_neg(a):
    return ((-a[0]) % P, (-a[1]) % P)


def rhs(group, x):
    """x^3 + b: b = 4 on G1, 4 (1 + u) on G2"""
    if group == 1:
        return (x * x * x + 4) % P
    c = f2_mul(f2_mul(x, x), x)
    return ((c[0] + 4) % P, (c[1] + 4) % P)


def is_square_fq(a):
    return a % P == 0 or pow(a, HALF, P) == 1


# ---- the model
def classify(group, enc):
    """("inf",), ("point", x, larger_flag) or ("bad", reason) from the bits alone; whether x is on the curve is on_curve's question"""
    assert len(enc) == 48 * group
    if not enc[0] & 0x80:
        return ("bad", "compression flag missing")
    if enc[0] & 0x40:
        if enc[0] != 0xC0 or any(enc[1:]):
            return ("bad", "infinity with other bits set")
        return ("inf",)
    first = int.from_bytes(bytes([enc[0] & 0x1F]) + enc[1:48], "big")
    if first >= P:
        return ("bad", "x >= p" if group == 1 else "x.c1 >= p")
    if group == 1:
        return ("point", first, bool(enc[0] & 0x20))
    second = int.from_bytes(enc[48:], "big")  # no flags here: a set top bit is part of the number
    if second >= P:
        return ("bad", "x.c0 >= p")
    return ("point", (second, first), bool(enc[0] & 0x20))


def on_curve(group, x):
    """is x^3 + b a square?  Euler's criterion; in Fq2 an element is a square iff its norm is one in Fq"""
    a = rhs(group, x)
    if group == 1:
        return is_square_fq(a)
    return is_square_fq(a[0] * a[0] + a[1] * a[1])


def verdict(group, enc):
    """"inf", "point" or the reason a decoder must refuse enc"""
    c = classify(group, enc)
    if c[0] == "point" and not on_curve(group, c[1]):
        return "x not on the curve"
    return c[1] if c[0] == "bad" else c[0]


def check_decoded(group, enc, point):
    """`point` is what a decoder returned for the valid encoding enc"""
    c = classify(group, enc)
    assert c[0] != "bad", c
    if c[0] == "inf":
        assert point is None
        return
    assert on_curve(group, c[1])
    assert point is not None
    x, y = point
    assert x == c[1]
    if group == 1:
        assert 0 <= y < P and y * y % P == rhs(1, x)
        assert c[2] == (y > (P - y) % P)
    else:
        assert 0 <= y[0] < P and 0 <= y[1] < P and f2_mul(y, y) == rhs(2, x)
        n = f2_neg(y)
        assert c[2] == ((y[1], y[0]) > (n[1], n[0]))


def encode(group, x, larger):
    body = x.to_bytes(48, "big") if group == 1 else x[1].to_bytes(48, "big") + x[0].to_bytes(48, "big")
    assert body[0] < 0x20
    enc = bytes([body[0] | 0x80 | (0x20 if larger else 0)]) + body[1:]
    assert classify(group, enc) == ("point", x, bool(larger))
    return enc


INFINITY = {1: bytes([0xC0]) + bytes(47), 2: bytes([0xC0]) + bytes(95)}


def both_flags(group, x):
    assert on_curve(group, x)
    return [encode(group, x, False), encode(group, x, True)]


# ---- constructors (square roots from here on, to find inputs only)
def _sqrt_fq(a):
    r = pow(a, (P + 1) // 4, P)
    assert r * r % P == a % P
    return r


def g2_imaginary_part_vanishes(count=2):
    """-> (xs with a0 a square, xs with a0 a non-square), `count` of each, a = x^3 + 4 (1 + u) having a1 == 0.
    Im(x^3) = 3 x0^2 x1 - x1^3, so for x1 = 2, 3, ... take x0 = sqrt((x1^3 - 4) / (3 x1)) when it exists.  a is in Fq then, and every
    element of Fq is a square in Fq2: y = (sqrt(a0), 0) if a0 is a square, else (0, sqrt(-a0)).  All these x are on the curve (outside
    the r-subgroup; the decoder makes no subgroup check)."""
    square, non_square = [], []
    x1 = 2
    while len(square) < count or len(non_square) < count:
        v = (x1 ** 3 - 4) * pow(3 * x1, -1, P) % P
        if is_square_fq(v):
            x = (_sqrt_fq(v), x1)
            a = rhs(2, x)
            assert a[1] == 0 and a[0] != 0 and on_curve(2, x)
            into = square if is_square_fq(a[0]) else non_square
            if len(into) < count:
                into.append(x)
        x1 += 1
        assert x1 < 200
    return square, non_square


def g2_boundary_y():
    """-> (x, y) with y.c1 == (p - 1)/2 exactly, so that -y has c1 == (p + 1)/2: the two sides of the comparison's boundary.
    For y0 = 0, 1, ... c = (y0 + h u)^2 - 4 (1 + u) must be a cube: c^((p^2 - 1)/3) == 1.  p^2 - 1 = 9 t with 3 not dividing t; a cube
    root is c^e zeta with e = 1/3 mod t and zeta one of the nine 9th roots of unity.

    There is no such case with y.c1 == 0 and y.c0 == (p - 1)/2 (h^2 - 4 - 4u is not a cube in Fq2), and no G1 point with y == (p - 1)/2
    (h^2 - 4 is not a cubic residue mod p): both asserted here, so nobody needs to look for them again."""
    h = HALF
    assert pow((h * h - 4) % P, (P - 1) // 3, P) != 1
    assert f2_pow(((h * h - 4) % P, P - 4), (P * P - 1) // 3) != (1, 0)
    t = (P * P - 1) // 9
    assert 9 * t == P * P - 1 and t % 3 != 0
    e = pow(3, -1, t)
    z = (1, 1)
    while True:  # a primitive 9th root of unity
        zeta = f2_pow(z, t)
        if f2_pow(zeta, 3) != (1, 0):
            break
        z = (z[0], z[1] + 1)
    for y0 in range(64):
        y = (y0, h)
        yy = f2_mul(y, y)
        c = ((yy[0] - 4) % P, (yy[1] - 4) % P)
        if f2_pow(c, (P * P - 1) // 3) != (1, 0):
            continue
        x = f2_pow(c, e)
        for _ in range(9):
            if f2_mul(f2_mul(x, x), x) == c:
                assert rhs(2, x) == yy and on_curve(2, x) and y[1] == (P - 1) // 2 and f2_neg(y)[1] == (P + 1) // 2
                return x, y
            x = f2_mul(x, zeta)
    raise AssertionError("no boundary point found")


# leading-zero bytes and an all-but-a-few-bits-set field through the byte -> limb conversion
SMALL_LARGE_ON = {1: [0, P - 3], 2: [(2, 0), (0, 1), (1, 1), (P - 1, 0), (P - 1, P - 1)]}
SMALL_LARGE_OFF = {1: [1, 2, P - 1, P - 2], 2: [(0, 0), (1, 0), (0, 2), (0, P - 1), (P - 1, 1)]}


def small_large_x(group):
    """-> (xs on the curve, xs off it)"""
    on, off = SMALL_LARGE_ON[group], SMALL_LARGE_OFF[group]
    assert all(on_curve(group, x) for x in on) and not any(on_curve(group, x) for x in off)
    if group == 1:
        assert rhs(1, 0) == 4  # x = 0: y = 2 and p - 2
    return on, off


def g2_generic_arm(x):
    """which of (a0 + s)/2, (a0 - s)/2 is the square, s = norm^((p + 1)/4) as the kernel takes it: 1 or 2.  Only ever used to assert
    that a batch holds both; never to compute an expectation."""
    a = rhs(2, x)
    assert a[1] != 0 and on_curve(2, x)
    s = _sqrt_fq(a[0] * a[0] + a[1] * a[1])
    inv2 = pow(2, -1, P)
    first, second = is_square_fq((a[0] + s) * inv2), is_square_fq((a[0] - s) * inv2)
    assert first != second  # their product is -(a1/2)^2, a non-residue
    return 1 if first else 2


def subgroup_points(group, count, first=2):
    """k G for k = first, first + 1, ..."""
    G = po.BLS12_381.g1 if group == 1 else po.BLS12_381.g2
    out, acc = [], G.mul(G.gen, first)
    for _ in range(count):
        out.append(acc)
        acc = G.add(acc, G.gen)
    return out


def g2_generic_by_arm(count):
    """-> (xs of subgroup points taking the first arm, xs taking the second), `count` of each"""
    arms = {1: [], 2: []}
    k = 2
    G = po.BLS12_381.g2
    acc = G.mul(G.gen, k)
    while len(arms[1]) < count or len(arms[2]) < count:
        into = arms[g2_generic_arm(acc[0])]
        if len(into) < count:
            into.append(acc[0])
        acc = G.add(acc, G.gen)
        k += 1
        assert k < 64 * count
    return arms[1], arms[2]


def valid_classes(group):
    """{class name: [encodings]} -- every special valid class with both flag values (infinity has none); the classes a group does not
    have (G1: no imaginary part, no boundary y) are absent"""
    G = po.BLS12_381.g1 if group == 1 else po.BLS12_381.g2
    on, _ = small_large_x(group)
    cls = {}
    if group == 1:
        cls["generic"] = [e for pt in subgroup_points(1, 6) for e in both_flags(1, pt[0])]
    else:
        first, second = g2_generic_by_arm(3)
        cls["generic, first arm"] = [e for x in first for e in both_flags(2, x)]
        cls["generic, second arm"] = [e for x in second for e in both_flags(2, x)]
        square, non_square = g2_imaginary_part_vanishes()
        cls["a1 == 0, a0 a square"] = [e for x in square for e in both_flags(2, x)]
        cls["a1 == 0, a0 a non-square"] = [e for x in non_square for e in both_flags(2, x)]
        cls["boundary y"] = both_flags(2, g2_boundary_y()[0])
    cls["small or large x"] = [e for x in on for e in both_flags(group, x)]
    cls["infinity"] = [INFINITY[group]]
    cls["generator"] = both_flags(group, G.gen[0])
    for name, encs in cls.items():
        assert all(verdict(group, e) == ("inf" if name == "infinity" else "point") for e in encs), name
    return cls


def mixed_batch(group, n=130):
    """-> (encodings, class name of each): round-robin over the classes, each class cycling through its encodings, so every run of
    len(classes) consecutive encodings holds every class (G2: 8 in every 8; G1 has 4 classes: 4 in every 4)"""
    cls = valid_classes(group)
    names = list(cls)
    encs, tags = [], []
    for i in range(n):
        name = names[i % len(names)]
        encs.append(cls[name][(i // len(names)) % len(cls[name])])
        tags.append(name)
    for i in range(n - 7):
        assert len(set(tags[i:i + 8])) >= 4
    for name in names:
        at = [i for i in range(n) if tags[i] == name]
        assert len(at) >= 6, name
        if name != "infinity":
            assert {classify(group, encs[i])[2] for i in at} == {True, False}, name
    return encs, tags


def refusals(group):
    """[(encoding, the model's reason)]: every refusal class of the contract"""
    G = po.BLS12_381.g1 if group == 1 else po.BLS12_381.g2
    good = encode(group, G.mul(G.gen, 77)[0], True)
    tail = good[48:]  # G2: an intact x.c0
    zeros = bytes(48 * group - 1)
    _, off = small_large_x(group)

    def with_byte(enc, at, value):
        return enc[:at] + bytes([value]) + enc[at + 1:]

    out = [
        (with_byte(good, 0, good[0] & 0x7F), "compression flag missing"),
        (bytes(48 * group), "compression flag missing"),
        (bytes([0xC0]) + zeros[:-1] + bytes([1]), "infinity with other bits set"),
        (bytes([0xE0]) + zeros, "infinity with other bits set"),  # infinity and the sign flag
        (bytes([0xC1]) + zeros, "infinity with other bits set"),  # only the low five bits of byte 0
        (bytes([0xD0]) + zeros, "infinity with other bits set"),
        (bytes([0x80 | (P >> 376)]) + P.to_bytes(48, "big")[1:] + tail, "x >= p" if group == 1 else "x.c1 >= p"),  # p exactly
        (bytes([0x9F]) + bytes([255]) * 47 + tail, "x >= p" if group == 1 else "x.c1 >= p"),  # 2^381 - 1
    ]
    if group == 2:
        out += [
            (bytes([0xC0]) + bytes(47) + bytes([1]) + bytes(47), "infinity with other bits set"),  # bits in the second half only
            (bytes([0xC0]) + bytes(47) + bytes([0x80]) + bytes(47), "infinity with other bits set"),
            (good[:48] + P.to_bytes(48, "big"), "x.c0 >= p"),  # p exactly
            (good[:48] + bytes([0x1F]) + bytes([255]) * 47, "x.c0 >= p"),  # 2^381 - 1
        ]
        out += [(with_byte(good, 48, good[48] | bit), "x.c0 >= p") for bit in (0x80, 0x40, 0x20)]  # flag bits where no flags live
    out += [(encode(group, x, larger), "x not on the curve") for x in off for larger in (False, True)]
    for enc, reason in out:
        assert len(enc) == 48 * group and verdict(group, enc) == reason, (enc.hex(), reason, verdict(group, enc))
    return out
