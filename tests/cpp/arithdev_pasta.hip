// Device test library of the arithmetic core for the Pasta fields: the kernels, launch helpers and build flags are arithdev.hip's own
// (included as it stands, so the two libraries cannot drift apart); this file only adds the entries for the new type ids of
// csrc/hosttest.hip -- 16 Pallas Fq, 17 Vesta Fq (L = 10), 18 Pallas Fr, 19 Vesta Fr (L = 9) -- and the curve ids 2 / 3 of the recoding.
// tests/test_gpu_pasta.py compares them limb for limb with the CPU twin and both against the oracle.
#include "arithdev.hip"

extern "C" {

// raw Fu limbs, op table and layout as zkt_fu_raw (arith_ops.h)
int zkdp_fu_raw(int type, int op, int n, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *out) {
    switch (type) {
        case 16: return fu_raw<PallasFqU>(op, n, a, b, c, d, out);
        case 17: return fu_raw<VestaFqU>(op, n, a, b, c, d, out);
        case 18: return fu_raw<PallasFrU>(op, n, a, b, c, d, out);
        case 19: return fu_raw<VestaFrU>(op, n, a, b, c, d, out);
        default: return -1;
    }
}

// zkt_field_op's table on n cases of canonical u32 limbs
int zkdp_field_op(int field, int op, int n, const uint32_t *a, const uint32_t *b, uint32_t *out) {
    switch (field) {
        case 16: return field_op_dev<pallas_fqu>(op, n, a, b, out);
        case 17: return field_op_dev<vesta_fqu>(op, n, a, b, out);
        case 18: return field_op_dev<pallas_fru>(op, n, a, b, out);
        case 19: return field_op_dev<vesta_fru>(op, n, a, b, out);
        default: return -1;
    }
}

// n scalars (8 u32 each) -> digits, RECODE_STRIDE int32 per scalar; curve 2 Pallas (scalars mod q), 3 Vesta (scalars mod p)
int zkdp_recode_folded(int curve, int c, int n, const uint32_t *scalars, int32_t *digits) {
    if ((curve != 2 && curve != 3) || c < 2 || c > 21 || n < 0) return -1;
    const int tb = 255, W = msm_windows(tb, c);
    if (W > 128) return -1;
    const MsmWindows win = msm_make_windows(tb, W);
    Dev m;
    const uint32_t *ds = m.in(scalars, (size_t)n * 32);
    int32_t *dd = m.out(digits, (size_t)n * RECODE_STRIDE * 4);
    if (m.err == hipSuccess && n) {
        if (curve == 2) hipLaunchKernelGGL(k_recode<PallasFr>, dim3(blocks(n)), dim3(64), 0, 0, n, ds, win, dd);
        else hipLaunchKernelGGL(k_recode<VestaFr>, dim3(blocks(n)), dim3(64), 0, 0, n, ds, win, dd);
    }
    return m.finish();
}

// zkt_point_chain's modes 0 - 4 for the two coordinate fields (one lane)
int zkdp_point_chain(int field, const uint32_t *pts, const uint8_t *inf, const uint8_t *neg, size_t n, int mode, uint32_t k, uint32_t *out,
                     uint8_t *out_inf) {
    if (mode < 0 || mode > 4) return -1;
    switch (field) {
        case 16: return chain<pallas_fqu>(pts, inf, neg, n, mode, k, out, out_inf);
        case 17: return chain<vesta_fqu>(pts, inf, neg, n, mode, k, out, out_inf);
        default: return -1;
    }
}

// zkt_parked_affine for the two coordinate fields (one lane, n <= 16)
int zkdp_parked_affine(int field, const uint32_t *pts, const uint8_t *inf, const uint8_t *neg, size_t n, int layout, uint32_t *out, uint8_t *out_inf) {
    switch (field) {
        case 16: return parked<pallas_fqu>(pts, inf, neg, n, layout, out, out_inf);
        case 17: return parked<vesta_fqu>(pts, inf, neg, n, layout, out, out_inf);
        default: return -1;
    }
}

}  // extern "C"
