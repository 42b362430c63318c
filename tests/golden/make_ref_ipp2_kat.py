#!/usr/bin/env python3
"""Extract the reference's known-answer DATA of the inner pairing product commitments (integer
literals only) into ref_ipp2_kat.json.

Run where the reference tree is at hand (its path is the argument); the resulting JSON is committed and is all that travels.
Source (data literals, no code):
  test/systems/ppzksnark/r1cs_gg_ppzksnark/r1cs_gg_ppzksnark_aggregation_conformity.cpp
    bls381_commitment_test, up to the key-compression part: n = 10, the key scalars u and v, ten G1
    points a and ten G2 points b (affine, z = 1), and the four expected Fq12 values of
    kzg_ipp2::single(vkey, a) and kzg_ipp2::pair(vkey, wkey, a, b), each as 12 Fq integers in the
    order of the constructor fq12(fq6(fq2, fq2, fq2), fq6(fq2, fq2, fq2)).
"""
import json
import os
import re
import sys

if len(sys.argv) != 2:
    sys.exit("usage: make_ref_ipp2_kat.py <path of the reference tree>")
REF = sys.argv[1]
AGG = os.path.join(REF, "test/systems/ppzksnark/r1cs_gg_ppzksnark/r1cs_gg_ppzksnark_aggregation_conformity.cpp")


def hexes(text, suffix):
    return [int(h, 16) for h in re.findall(r"0x([0-9a-fA-F]+)_cppui_modular" + suffix, text)]


def main():
    text = open(AGG).read()
    i = text.index("BOOST_AUTO_TEST_CASE(bls381_commitment_test)")
    j = text.index("scalar_field_value_type c(", i)  # the key-compression vectors follow; not used here
    blk = text[i:j]
    fr = hexes(blk, "255")
    fq = hexes(blk, "381")
    n = 10
    # order in the file: a (n x 2), c1.first, c1.second (12 each), b (n x 4), c2.first, c2.second
    assert len(fr) == 2 and len(fq) == 2 * n + 24 + 4 * n + 24, (len(fr), len(fq))
    a = fq[: 2 * n]
    c1 = fq[2 * n: 2 * n + 24]
    b = fq[2 * n + 24: 6 * n + 24]
    c2 = fq[6 * n + 24:]
    out = {
        "source": "NilFoundation/crypto3-zk test vectors (bellperson-derived), literals only",
        "n": n,
        "u": hex(fr[0]),
        "v": hex(fr[1]),
        # G1 points as [x, y]
        "a": [[hex(a[2 * k]), hex(a[2 * k + 1])] for k in range(n)],
        # G2 points as [[x.c0, x.c1], [y.c0, y.c1]]
        "b": [[[hex(b[4 * k]), hex(b[4 * k + 1])], [hex(b[4 * k + 2]), hex(b[4 * k + 3])]] for k in range(n)],
        "single_first": [hex(x) for x in c1[:12]],
        "single_second": [hex(x) for x in c1[12:]],
        "pair_first": [hex(x) for x in c2[:12]],
        "pair_second": [hex(x) for x in c2[12:]],
    }
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_ipp2_kat.json")
    json.dump(out, open(dst, "w"), indent=1)
    print("wrote", dst)


if __name__ == "__main__":
    main()
