#!/usr/bin/env python3
"""Extract the reference's known-answer DATA of Groth16 verification (integer literals only) into
ref_groth16_verify_kat.json.

Run where the reference tree is at hand (its path is the argument); the resulting JSON is committed and is all that travels.
Source (data literals, no code):
  test/systems/ppzksnark/r1cs_gg_ppzksnark/r1cs_gg_ppzksnark_aggregation_conformity.cpp
    bls381_verification, from `fq12_value_type vk_alpha_g1_beta_g2` to `statements`: the Fq12 value alpha_g1_beta_g2
    (12 Fq integers in the order of the constructor fq12(fq6(fq2, fq2, fq2), fq6(fq2, fq2, fq2))), gamma_g2 and
    delta_g2 (affine, z = 1), the twelve vk_ic points, and eight bellperson proofs (A in G1, B in G2, C in G1), each
    followed by its statement of eleven public inputs: 108 Fq and 88 Fr values.
"""
import json
import os
import re
import sys

if len(sys.argv) != 2:
    sys.exit("usage: make_ref_groth16_verify_kat.py <path of the reference tree>")
REF = sys.argv[1]
AGG = os.path.join(REF, "test/systems/ppzksnark/r1cs_gg_ppzksnark/r1cs_gg_ppzksnark_aggregation_conformity.cpp")
N_PROOFS, N_IC, N_INPUTS = 8, 12, 11


def hexes(text, suffix):
    return [int(h, 16) for h in re.findall(r"0x([0-9a-fA-F]+)_cppui_modular" + suffix, text)]


def g2(v):
    return [[hex(v[0]), hex(v[1])], [hex(v[2]), hex(v[3])]]


def main():
    text = open(AGG).read()
    i = text.index("BOOST_AUTO_TEST_CASE(bls381_verification)")
    i = text.index("fq12_value_type vk_alpha_g1_beta_g2", i)
    j = text.index("statements {", i)
    blk = text[i:j]
    fq, fr = hexes(blk, "381"), hexes(blk, "255")
    assert len(fq) == 12 + 4 + 4 + 2 * N_IC + 8 * N_PROOFS == 108 and len(fr) == N_PROOFS * N_INPUTS == 88, (len(fq), len(fr))
    ic = fq[20:20 + 2 * N_IC]
    pf = fq[20 + 2 * N_IC:]
    out = {
        "source": "NilFoundation/crypto3-zk test vectors (bellperson-derived), literals only",
        "alpha_g1_beta_g2": [hex(x) for x in fq[:12]],
        # G2 points as [[x.c0, x.c1], [y.c0, y.c1]], G1 points as [x, y]
        "gamma_g2": g2(fq[12:16]),
        "delta_g2": g2(fq[16:20]),
        "ic": [[hex(ic[2 * k]), hex(ic[2 * k + 1])] for k in range(N_IC)],
        "proofs": [{"a": [hex(p[0]), hex(p[1])], "b": g2(p[2:6]), "c": [hex(p[6]), hex(p[7])]} for p in (pf[8 * k:8 * k + 8] for k in range(N_PROOFS))],
        "statements": [[hex(x) for x in fr[N_INPUTS * k:N_INPUTS * (k + 1)]] for k in range(N_PROOFS)],
    }
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_groth16_verify_kat.json")
    json.dump(out, open(dst, "w"), indent=1)
    print("wrote", dst)


if __name__ == "__main__":
    main()
