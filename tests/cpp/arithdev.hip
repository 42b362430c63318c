// Device test library: the arithmetic core as the kernels run it (inline-asm Montgomery products, -O3, gfx950; neither ZK_NO_ASM_MUL
// nor ZK_NOINLINE_MUL; the G2 lane-pair products inlined as csrc/msm_bls_g2.hip builds them), on host arrays of n cases.  Every entry
// copies its inputs in, runs one launch, synchronises, copies the results back and returns the HIP status (-1 for an id or op it does
// not know).  The op tables are csrc/arith_ops.h, shared with the CPU twin csrc/hosttest.hip; tests/test_gpu_arith.py compares the two
// limb for limb and both against the oracle.
#define ZK_PAIR_INLINE 1
#include <hip/hip_runtime.h>

#include "arith_ops.h"
#include "fu2_pair.hpp"
#include "msm_recode.hpp"

using namespace zkhip;
using namespace zkhip::arith;

namespace {

constexpr int RECODE_STRIDE = 130;  // per scalar: digits [0, W), [128] = W, [129] = carry out of the top window (must be 0)

struct Dev {  // device copies of the host arrays of one call
    void *p[8] = {};
    size_t sz[8] = {};
    const void *host[8] = {};
    int k = 0;
    hipError_t err = hipSuccess;
    template <class T>
    T *in(const T *h, size_t bytes) {  // no host array (or 0 bytes): a zeroed allocation
        void *d = nullptr;
        if (err == hipSuccess) err = hipMalloc(&d, bytes ? bytes : 16);
        if (err == hipSuccess) err = h && bytes ? hipMemcpy(d, h, bytes, hipMemcpyHostToDevice) : hipMemset(d, 0, bytes ? bytes : 16);
        p[k] = d, sz[k] = bytes, host[k] = nullptr, ++k;
        return (T *)d;
    }
    template <class T>
    T *out(T *h, size_t bytes) {
        void *d = nullptr;
        if (err == hipSuccess) err = hipMalloc(&d, bytes ? bytes : 16);
        if (err == hipSuccess) err = hipMemset(d, 0, bytes ? bytes : 16);
        p[k] = d, sz[k] = bytes, host[k] = h, ++k;
        return (T *)d;
    }
    int finish() {  // after the launch: synchronise, copy the outputs back, free
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
        for (int i = 0; i < k; ++i)
            if (err == hipSuccess && host[i] && sz[i]) err = hipMemcpy((void *)host[i], p[i], sz[i], hipMemcpyDeviceToHost);
        for (int i = 0; i < k; ++i)
            if (p[i]) (void)hipFree(p[i]);
        return (int)err;
    }
};

inline unsigned blocks(size_t threads) { return (unsigned)((threads + 63) / 64); }

template <class U>
__global__ void k_fu_raw(int op, int n, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t o = (size_t)i * U::L;
    fu_raw_one<U>(op, a + o, b + o, c + o, d + o, out + o);
}

template <class U>
int fu_raw(int op, int n, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *out) {
    if (!fu_raw_valid<U>(op) || n < 0) return -1;
    const size_t bytes = (size_t)n * U::L * 4;
    Dev m;
    const uint32_t *da = m.in(a, bytes), *db = m.in(b, bytes), *dc = m.in(c, bytes), *dd = m.in(d, bytes);
    uint32_t *dout = m.out(out, bytes);
    if (m.err == hipSuccess && n) hipLaunchKernelGGL(k_fu_raw<U>, dim3(blocks(n)), dim3(64), 0, 0, op, n, da, db, dc, dd, dout);
    return m.finish();
}

template <class F>
__global__ void k_field_op(int op, int n, const uint32_t *a, const uint32_t *b, uint32_t *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int CW = FieldOps<F>::CANON_WORDS;
    field_op<F>(op, a + (size_t)i * CW, b + (size_t)i * CW, out + (size_t)i * CW);
}

template <class F>
int field_op_dev(int op, int n, const uint32_t *a, const uint32_t *b, uint32_t *out) {
    if (!field_op_valid(op) || n < 0) return -1;
    const size_t bytes = (size_t)n * FieldOps<F>::CANON_WORDS * 4;
    Dev m;
    const uint32_t *da = m.in(a, bytes), *db = m.in(b, bytes);
    uint32_t *dout = m.out(out, bytes);
    if (m.err == hipSuccess && n) hipLaunchKernelGGL(k_field_op<F>, dim3(blocks(n)), dim3(64), 0, 0, op, n, da, db, dout);
    return m.finish();
}

// ---- FieldOps<Fu2h> on lane pairs ------------------------------------------------------------------------------------------
// One Fq2 case per lane pair; operands and results are 2 L raw limbs per case (c0 | c1).  op: 0 mul(a, b), 1 sqr(a), 2 add(a, b),
// 3 sub<K1>(a, b), 4 sub<K2>, 5 sub<K3>, 6 mul_sub<K1>(a, b, c, d), 7 is_zero(a), 8 is_zero_product(a), 9 is_exact_zero(a)
// (bool ops: each lane writes the pair's verdict into limb 0 of its own half), 10 to_canonical(a) (2 NL saturated words),
// 11 store(a) then load back through the device-buffer layout (c0 | c1, SL words each).
template <class U>
__global__ void k_fu2h(int op, int n, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *buf, uint32_t *out) {
    typedef Fu2h<U> F;
    typedef FieldOps<F> O;
    constexpr int L = U::L;
    const int t = blockIdx.x * blockDim.x + threadIdx.x, j = t >> 1;  // blockDim is even: both lanes of a pair share the bound check
    if (j >= n) return;
    const size_t o = (size_t)j * 2 * L + (F::odd() ? L : 0);
    F x, y, z, w, r = F::zero();
    for (int i = 0; i < L; ++i) x.v.v[i] = a[o + i], y.v.v[i] = b[o + i], z.v.v[i] = c[o + i], w.v.v[i] = d[o + i];
    switch (op) {
        case 0: r = O::mul(x, y); break;
        case 1: r = O::sqr(x); break;
        case 2: r = O::add(x, y); break;
        case 3: r = O::template sub<O::K1>(x, y); break;
        case 4: r = O::template sub<O::K2>(x, y); break;
        case 5: r = O::template sub<O::K3>(x, y); break;
        case 6: r = O::template mul_sub<O::K1>(x, y, z, w); break;
        case 7: r.v.v[0] = O::is_zero(x) ? 1u : 0u; break;
        case 8: r.v.v[0] = O::is_zero_product(x) ? 1u : 0u; break;
        case 9: r.v.v[0] = O::is_exact_zero(x) ? 1u : 0u; break;
        case 10: O::to_canonical(out + (size_t)j * 2 * L, x); return;
        case 11: {
            uint32_t *p = buf + (size_t)j * O::WORDS;
            O::store(p, x);
            r = O::load(p);
            break;
        }
        default: break;
    }
    for (int i = 0; i < L; ++i) out[o + i] = r.v.v[i];
}

template <class U>
int fu2h(int op, int n, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *out) {
    if (op < 0 || op > 11 || n < 0) return -1;
    const size_t bytes = (size_t)n * 2 * U::L * 4;
    Dev m;
    const uint32_t *da = m.in(a, bytes), *db = m.in(b, bytes), *dc = m.in(c, bytes), *dd = m.in(d, bytes);
    uint32_t *dbuf = m.in<uint32_t>(nullptr, (size_t)n * 2 * U::SL * 4);
    uint32_t *dout = m.out(out, bytes);
    if (m.err == hipSuccess && n) hipLaunchKernelGGL(k_fu2h<U>, dim3(blocks(2 * (size_t)n)), dim3(64), 0, 0, op, n, da, db, dc, dd, dbuf, dout);
    return m.finish();
}

// ---- recoding: msm_fold_scalar + msm_recode as msm_digits_only runs them --------------------------------------------------
template <class FR>
__global__ void k_recode(int n, const uint32_t *scalars, MsmWindows win, int32_t *digits) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t s[8];
    const bool flip = msm_fold_scalar<FR>(scalars + (size_t)i * 8, s);
    int32_t *dg = digits + (size_t)i * RECODE_STRIDE;
    uint32_t carry = 0;
    for (int w = 0; w < win.W; ++w) {
        const uint32_t d = msm_recode(s, win.off(w), win.width(w), carry);
        int32_t v = 0;
        if (d != DIG_NONE) {
            const int32_t mag = (int32_t)(d & 0x7FFFFFFFu) + 1;
            v = (d >> 31) ? -mag : mag;
        }
        dg[w] = flip ? -v : v;
    }
    dg[128] = win.W;
    dg[129] = (int32_t)carry;
}

// ---- madd chains ----------------------------------------------------------------------------------------------------------
template <class F>
__global__ void k_chain(const uint32_t *pts, const uint8_t *inf, const uint8_t *neg, size_t n, int mode, uint32_t k, uint32_t *out, uint8_t *out_inf) {
    if (blockIdx.x == 0 && threadIdx.x == 0) point_chain<F>(pts, inf, neg, n, mode, k, out, out_inf);
}

// the bucket kernel's G2 accumulation: one lane pair runs the madd chain over Fu2h (each lane converts its own component of every
// affine input), stores the XYZZ sum in the device-buffer layout; one lane then reads it back as single-lane Fu2 and normalises it
template <class U>
__global__ void k_chain_pair(const uint32_t *pts, const uint8_t *inf, const uint8_t *neg, size_t n, uint32_t *xyzz) {
    typedef Fu2h<U> F;
    constexpr int NL = U::NL;
    if (blockIdx.x != 0 || threadIdx.x >= 2) return;
    const int half = F::odd() ? NL : 0;
    XYZZ<F> acc = XYZZ<F>::infinity();
    for (size_t i = 0; i < n; ++i) {
        const uint32_t *p = pts + i * 4 * NL;
        Affine<F> q = inf[i] ? Affine<F>::infinity() : Affine<F> {{fu_from_canonical<U>(p + half)}, {fu_from_canonical<U>(p + 2 * NL + half)}};
        acc = xyzz_madd(acc, q, neg[i] != 0);
    }
    xyzz_store<F>(xyzz, acc);
}
template <class U>
__global__ void k_chain_pair_out(const uint32_t *xyzz, uint32_t *out, uint8_t *out_inf) {
    if (blockIdx.x == 0 && threadIdx.x == 0) store_aff<Fu2<U>>(out, out_inf, xyzz_load<Fu2<U>>(xyzz));
}

template <class F>
int chain(const uint32_t *pts, const uint8_t *inf, const uint8_t *neg, size_t n, int mode, uint32_t k, uint32_t *out, uint8_t *out_inf) {
    constexpr int CW = FieldOps<F>::CANON_WORDS;
    Dev m;
    const uint32_t *dp = m.in(pts, n * 2 * CW * 4);
    const uint8_t *di = m.in(inf, n), *dn = m.in(neg, n);
    uint32_t *dout = m.out(out, (size_t)(mode == 3 ? 3 : 2) * CW * 4);
    uint8_t *dinf = m.out(out_inf, 1);
    if (m.err == hipSuccess) hipLaunchKernelGGL(k_chain<F>, dim3(1), dim3(64), 0, 0, dp, di, dn, n, mode, k, dout, dinf);
    return m.finish();
}

// ---- the shared inversion over parked points (arith_ops.h: parked_affine), one lane ---------------------------------------------------
template <class F>
__global__ void k_parked(const uint32_t *pts, const uint8_t *inf, const uint8_t *neg, size_t n, int layout, uint32_t *work, uint32_t *out, uint8_t *out_inf) {
    if (blockIdx.x == 0 && threadIdx.x == 0) parked_affine<F>(pts, inf, neg, n, layout, work, out, out_inf);
}

template <class F>
int parked(const uint32_t *pts, const uint8_t *inf, const uint8_t *neg, size_t n, int layout, uint32_t *out, uint8_t *out_inf) {
    constexpr int CW = FieldOps<F>::CANON_WORDS;
    if (n > 16 || (layout != 0 && layout != 1)) return -1;
    Dev m;
    const uint32_t *dp = m.in(pts, n * 2 * CW * 4);
    const uint8_t *di = m.in(inf, n), *dn = m.in(neg, n);
    uint32_t *dw = m.in<uint32_t>(nullptr, 7 * n * FieldOps<F>::WORDS * 4);
    uint32_t *dout = m.out(out, n * 2 * CW * 4);
    uint8_t *dinf = m.out(out_inf, n);
    if (m.err == hipSuccess && n) hipLaunchKernelGGL(k_parked<F>, dim3(1), dim3(64), 0, 0, dp, di, dn, n, layout, dw, dout, dinf);
    return m.finish();
}

template <class U>
int chain_pair(const uint32_t *pts, const uint8_t *inf, const uint8_t *neg, size_t n, uint32_t *out, uint8_t *out_inf) {
    Dev m;
    const uint32_t *dp = m.in(pts, n * 4 * U::NL * 4);
    const uint8_t *di = m.in(inf, n), *dn = m.in(neg, n);
    uint32_t *dx = m.in<uint32_t>(nullptr, 4 * 2 * U::SL * 4);
    uint32_t *dout = m.out(out, 4 * U::NL * 4);
    uint8_t *dinf = m.out(out_inf, 1);
    if (m.err == hipSuccess) hipLaunchKernelGGL(k_chain_pair<U>, dim3(1), dim3(64), 0, 0, dp, di, dn, n, dx);
    if (m.err == hipSuccess) m.err = hipGetLastError();
    if (m.err == hipSuccess) hipLaunchKernelGGL(k_chain_pair_out<U>, dim3(1), dim3(64), 0, 0, dx, dout, dinf);
    return m.finish();
}

}  // namespace

extern "C" {

// raw Fu limbs: type 6 BLS Fq, 7 BN Fq, 8 BLS Fr, 9 BN Fr; op table and layout as zkt_fu_raw (arith_ops.h)
int zkd_fu_raw(int type, int op, int n, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *out) {
    switch (type) {
        case 6: return fu_raw<BlsFqU>(op, n, a, b, c, d, out);
        case 7: return fu_raw<BnFqU>(op, n, a, b, c, d, out);
        case 8: return fu_raw<BlsFrU>(op, n, a, b, c, d, out);
        case 9: return fu_raw<BnFrU>(op, n, a, b, c, d, out);
        default: return -1;
    }
}

// zkt_field_op's table on n cases of canonical u32 limbs, lazy fields 6 - 11 (10 / 11: single-lane Fu2)
int zkd_field_op(int field, int op, int n, const uint32_t *a, const uint32_t *b, uint32_t *out) {
    switch (field) {
        case 6: return field_op_dev<bls_fqu>(op, n, a, b, out);
        case 7: return field_op_dev<bn_fqu>(op, n, a, b, out);
        case 8: return field_op_dev<bls_fru>(op, n, a, b, out);
        case 9: return field_op_dev<bn_fru>(op, n, a, b, out);
        case 10: return field_op_dev<bls_fqu2>(op, n, a, b, out);
        case 11: return field_op_dev<bn_fqu2>(op, n, a, b, out);
        default: return -1;
    }
}

// FieldOps<Fu2h> over lane pairs (see k_fu2h); curve 0 BLS12-381, 1 BN254
int zkd_fu2h(int curve, int op, int n, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *out) {
    if (curve == 0) return fu2h<BlsFqU>(op, n, a, b, c, d, out);
    if (curve == 1) return fu2h<BnFqU>(op, n, a, b, c, d, out);
    return -1;
}

// n scalars (8 u32 each) -> digits, RECODE_STRIDE int32 per scalar; the windows zkt_recode_folded uses for (curve, c)
int zkd_recode_folded(int curve, int c, int n, const uint32_t *scalars, int32_t *digits) {
    if ((curve != 0 && curve != 1) || c < 2 || c > 21 || n < 0) return -1;
    const int tb = curve == 0 ? 255 : 254, W = msm_windows(tb, c);
    if (W > 128) return -1;
    const MsmWindows win = msm_make_windows(tb, W);
    Dev m;
    const uint32_t *ds = m.in(scalars, (size_t)n * 32);
    int32_t *dd = m.out(digits, (size_t)n * RECODE_STRIDE * 4);
    if (m.err == hipSuccess && n) {
        if (curve == 0) hipLaunchKernelGGL(k_recode<BlsFr>, dim3(blocks(n)), dim3(64), 0, 0, n, ds, win, dd);
        else hipLaunchKernelGGL(k_recode<BnFr>, dim3(blocks(n)), dim3(64), 0, 0, n, ds, win, dd);
    }
    return m.finish();
}

// zkt_point_chain's modes 0 - 4 for the lazy coordinate fields 6, 7, 10, 11 (one lane), and mode 5 for 10 / 11: the madd chain over
// Fu2h lane pairs, as the G2 bucket kernel accumulates (the result as mode 0's)
int zkd_point_chain(int field, const uint32_t *pts, const uint8_t *inf, const uint8_t *neg, size_t n, int mode, uint32_t k, uint32_t *out,
                    uint8_t *out_inf) {
    if (mode < 0 || mode > 5) return -1;
    if (mode == 5) {
        if (field == 10) return chain_pair<BlsFqU>(pts, inf, neg, n, out, out_inf);
        if (field == 11) return chain_pair<BnFqU>(pts, inf, neg, n, out, out_inf);
        return -1;
    }
    switch (field) {
        case 6: return chain<bls_fqu>(pts, inf, neg, n, mode, k, out, out_inf);
        case 7: return chain<bn_fqu>(pts, inf, neg, n, mode, k, out, out_inf);
        case 10: return chain<bls_fqu2>(pts, inf, neg, n, mode, k, out, out_inf);
        case 11: return chain<bn_fqu2>(pts, inf, neg, n, mode, k, out, out_inf);
        default: return -1;
    }
}

// zkt_parked_affine for the lazy coordinate fields 6, 7, 10, 11 (one lane, n <= 16)
int zkd_parked_affine(int field, const uint32_t *pts, const uint8_t *inf, const uint8_t *neg, size_t n, int layout, uint32_t *out, uint8_t *out_inf) {
    switch (field) {
        case 6: return parked<bls_fqu>(pts, inf, neg, n, layout, out, out_inf);
        case 7: return parked<bn_fqu>(pts, inf, neg, n, layout, out, out_inf);
        case 10: return parked<bls_fqu2>(pts, inf, neg, n, layout, out, out_inf);
        case 11: return parked<bn_fqu2>(pts, inf, neg, n, layout, out, out_inf);
        default: return -1;
    }
}

}  // extern "C"
