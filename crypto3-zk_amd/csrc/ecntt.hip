// Radix-2 (inverse) DFT over GROUP ELEMENTS: out[j] = sum_i omega^(i j) P_i  (inverse: omega^-1 and a final 1/m).
//
// This is evaluation_domain<Fr, G>::evaluate_all_lagrange_polynomials(powers_begin, powers_end) as the powers-of-tau
// result uses it (zk/commitments/detail/polynomial/powers_of_tau/result.hpp:81-94): with P_i = tau^i G the inverse
// transform yields L_j(tau) G for every Lagrange basis polynomial of the domain.  Setup-side
// work: every butterfly multiplies a point by a full-width twiddle, m/2 log2 m of them.
//
// Shape (round 3; round 2 ran one plain double-and-add per butterfly -- 255 doublings and, because the lanes of a wave hold
// DIFFERENT twiddles, an addition at every bit: ~1.6 M instructions per lane):
//   * a stage is a MULTIPLICATION pass (one lane per point that takes a twiddle) and a cheap butterfly pass (u + v, u - v);
//   * the multiplication is a FIXED 4-bit signed-window ladder -- every lane adds at the same 1-in-4 positions, so divergence costs
//     nothing: the lane's multiples P .. 8P (4 doublings + 3 additions) go to a table in HBM (the lane's own 8 x 4 coordinates,
//     contiguous), the twiddle is recoded once per table entry into nibbles in [-8, 7];
//   * on G1 the twiddle is split with the curve's endomorphism phi(x, y) = (beta x, y) = lambda P (GLV): k = k1 + k2 lambda with
//     |k1|, |k2| < 2^129, decomposed on the device when the twiddle records are built, so the ladder is 33 windows of 4 doublings +
//     2 additions (from the table of P and the table of phi(P): the same entries with X multiplied by beta) instead of 65 windows of
//     4 + 1: ~0.6 M instructions per lane; G2 takes the 65-window ladder (~2 x fewer additions than round 2);
//   * the 1/m of the inverse transform is folded into the LAST stage (u / m + (w^k / m) v: its own record table) -- m
//     multiplications in one parallel pass instead of m / 2 in the stage and m more afterwards.
//
// Boundary forms, one pair of load / store kernels each around the same stage network:
//   zkhip_ec_ntt_dev       canonical Jacobian points (X, Y, Z; Z = 0 for infinity), as zkhip_msm_dev returns them, in place;
//   zkhip_bases_lagrange   (zkhip.hip; zk_bases_lagrange below) the affine points of a bases object in, always the inverse transform, affine
//                          points into a new bases object out: one inversion per lane over a chunk of points (Montgomery's trick).
//                          kimchi_pedersen::params_type::add_lagrange_basis (kimchi_pedersen.hpp:92-105), G1 of all four curve ids.
//
// The same ladder WITHOUT the network -- out[i] = s_i P_i, a different scalar per resident point (zkhip_bases_scale_dev / zkhip_bases_scale_geometric;
// zk_bases_scale below): the contribution to a powers-of-tau accumulator (powers_of_tau/accumulator.hpp:89-121) and the delta^-1 scaling of the
// Groth16 MPC (r1cs_gg_ppzksnark_mpc/crs_operations.hpp:116-123).  Records from resident scalars or from coeff ratio^i, one bases_scale_pass
// per slice of table slots, the same affine store.
#include <algorithm>

#include "ctx.hpp"
#include "curve.hpp"
#include "glv.hpp"

using namespace zkhip;

namespace {

// The GLV constants, the split k -> (k1, k2) and the window record of a scalar (REC_WORDS words, scalar_record) are glv.hpp's (BlsGlv, BnGlv,
// PallasGlv, VestaGlv; NoGlv: the plain ladder).

// consts: [0] = effective root (omega, or omega^-1 for the inverse) canonical; [1] = 1/m canonical
template <class U>
__global__ void ec_ntt_setup(const uint32_t *__restrict__ omega_c, uint32_t log_m, int inverse, uint32_t *__restrict__ consts) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    Fu<U> w = fu_from_canonical<U>(omega_c);
    if (inverse) w = fu_inv(w);
    fu_to_canonical<U>(consts, w);
    Fu<U> two = fu_add(Fu<U>::one(), Fu<U>::one()), mm = Fu<U>::one();
    for (uint32_t i = 0; i < log_m; ++i) mm = fu_mul_call(mm, two);
    fu_to_canonical<U>(consts + U::NL, fu_inv(mm));
}

// rec[j] = the window record of w^(e0 + j) (times `scale` when given) for j < count: square-and-multiply over the bits of the exponent
// (e0 + j < 2^32; w^0 = 1 whatever w is, zero included), then the GLV split (G1) and the signed-nibble recoding.  The twiddles of the group
// DFT (e0 = 0) and the geometric scalars coeff ratio^(e0 + j) of zkhip_bases_scale_geometric.
template <class U, class G>
__global__ __launch_bounds__(256) void ec_ntt_records(const uint32_t *__restrict__ consts, const uint32_t *__restrict__ scale_c, uint32_t e0, uint32_t count,
                                                       uint32_t *__restrict__ rec) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    Fu<U> pw = fu_from_canonical<U>(consts), acc = Fu<U>::one();
    for (uint32_t e = e0 + j; e; e >>= 1) {
        if (e & 1) acc = fu_mul_call(acc, pw);
        pw = fu_mul_call(pw, pw);
    }
    if (scale_c) acc = fu_mul_call(acc, fu_from_canonical<U>(scale_c));
    uint32_t k[8];
    fu_to_canonical<U>(k, acc);
    scalar_record<G>(rec + (size_t)j * REC_WORDS, k);
}

// rec[j] = the window record of the resident scalar j (8 canonical words; a value that is not below r is taken mod r, as the MSM takes it)
template <class U, class G>
__global__ __launch_bounds__(256) void scale_records_from_scalars(const uint32_t *__restrict__ scalars, uint32_t count, uint32_t *__restrict__ rec) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    uint32_t k[8];
    fu_pack<U>(k, fu_reduce(fu_load8<U>(scalars, j)));
    scalar_record<G>(rec + (size_t)j * REC_WORDS, k);
}

// canonical Jacobian -> device XYZZ at the bit-reversed position
template <class F>
__global__ __launch_bounds__(64) void ec_ntt_load(const uint32_t *__restrict__ jac, uint32_t log_m, uint32_t *__restrict__ pts) {
    typedef FieldOps<F> O;
    constexpr int CW = O::CANON_WORDS, NL = O::WORDS;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, m = 1u << log_m;
    if (i >= m) return;
    const uint32_t *p = jac + (size_t)i * 3 * CW;
    Jacobian<F> j = {O::from_canonical(p), O::from_canonical(p + CW), O::from_canonical(p + 2 * CW)};
    const uint32_t r = log_m ? (__brev(i) >> (32 - log_m)) : 0;
    xyzz_store<F>(pts + (size_t)r * (4 * NL), xyzz_from_jacobian(j));
}

template <class F>
ZK_D XYZZ<F> xyzz_dbl4(XYZZ<F> a) {
    a = xyzz_dbl(a);
    a = xyzz_dbl(a);
    a = xyzz_dbl(a);
    return xyzz_dbl(a);
}

// The fixed 4-bit signed-window ladder of one lane: out <- rec P for a finite point P and a window record (glv.hpp: scalar_record).  T: the lane's table,
// 8 * HALVES points of the launch's table slots -- e P for e = 1 .. 8 (and phi(e P) behind them); every entry is re-read from memory where it is
// needed again.  The body of both multiplication kernels below.
template <class F, class G>
ZK_D void ec_ladder(const XYZZ<F> &p, const uint32_t *rec, uint32_t *T, uint32_t *out) {
    typedef FieldOps<F> O;
    constexpr int NL = O::WORDS, PW = 4 * NL, HALVES = G::ENABLED ? 2 : 1, NW = G::ENABLED ? 33 : 65;
    auto entry = [&](int e) { return T + (size_t)(e - 1) * PW; };
    {
        xyzz_store<F>(entry(1), p);
        XYZZ<F> e2 = xyzz_dbl(p);
        xyzz_store<F>(entry(2), e2);
        xyzz_store<F>(entry(3), xyzz_add(e2, p));
        e2 = xyzz_dbl(e2);
        xyzz_store<F>(entry(4), e2);
        xyzz_store<F>(entry(5), xyzz_add(e2, p));
        xyzz_store<F>(entry(8), xyzz_dbl(e2));
        e2 = xyzz_dbl(xyzz_load<F>(entry(3)));
        xyzz_store<F>(entry(6), e2);
        xyzz_store<F>(entry(7), xyzz_add(e2, p));
    }
    if constexpr (G::ENABLED) {
        static_assert(G::BETA_WORDS == O::CANON_WORDS, "beta is an element of this coordinate field");
        uint32_t bc[O::CANON_WORDS];
        for (int i = 0; i < O::CANON_WORDS; ++i) bc[i] = G::beta(i);
        const F beta = O::from_canonical(bc);
        for (int e = 1; e <= 8; ++e) {
            XYZZ<F> q = xyzz_load<F>(entry(e));
            q.X = O::mul(q.X, beta);
            xyzz_store<F>(entry(8 + e), q);
        }
    }
    const uint32_t signs = rec[10];
    XYZZ<F> acc = XYZZ<F>::infinity();
    for (int w = NW - 1; w >= 0; --w) {
        acc = xyzz_dbl4(acc);
#pragma unroll 1
        for (int h = 0; h < HALVES; ++h) {
            const int d = (int)(((rec[h * 5 + (w >> 3)] >> ((w & 7) * 4)) & 15u) ^ 8u) - 8;
            if (d != 0) {
                XYZZ<F> e = xyzz_load<F>(entry(8 * h + (d < 0 ? -d : d)));
                if ((d < 0) != (((signs >> h) & 1u) != 0)) e.Y = O::template sub<O::K2>(F::zero(), e.Y);
                acc = xyzz_add(acc, e);
            }
        }
    }
    xyzz_store<F>(out, acc);
}

// The multiplication pass.  mode 0: stage s (1-based) of the decimation-in-time network, lane t = butterfly t multiplies its lower
// input v by w^(k stride) (k = 0: nothing to do); mode 1: the last stage of the INVERSE transform, lane t = point t, upper inputs take
// 1/m, lower inputs w^k / m.  Lanes first .. first + gridDim.x * 64 of `total`; `tbl` holds 8 * HALVES points per lane of the launch.
template <class F, class G>
__global__ __launch_bounds__(64, G::ENABLED ? 2 : 1) void ec_ntt_mul_pass(uint32_t *__restrict__ pts, const uint32_t *__restrict__ rec_stage, const uint32_t *__restrict__ rec_last,
                                                      const uint32_t *__restrict__ rec_minv, uint32_t log_m, uint32_t s, int mode, uint32_t first,
                                                      uint32_t total, uint32_t *__restrict__ tbl) {
    constexpr int NL = FieldOps<F>::WORDS, PW = 4 * NL, HALVES = G::ENABLED ? 2 : 1;
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x, t = first + slot;
    if (t >= total) return;
    const uint32_t half = 1u << (s - 1);
    uint32_t j;
    const uint32_t *rec;
    if (mode == 0) {
        const uint32_t k = t & (half - 1);
        if (k == 0) return;
        j = ((t >> (s - 1)) << s) + k + half;
        rec = rec_stage + (size_t)(k << (log_m - s)) * REC_WORDS;
    } else {
        j = t;
        rec = (t & half) ? rec_last + (size_t)(t & (half - 1)) * REC_WORDS : rec_minv;
    }
    uint32_t *pj = pts + (size_t)j * PW;
    const XYZZ<F> p = xyzz_load<F>(pj);
    if (p.is_inf()) return;
    ec_ladder<F, G>(p, rec, tbl + (size_t)slot * (8 * HALVES) * PW, pj);
}

// out[i] = s_i P_i over the affine rows of a bases object (zkhip_bases_scale_*): lane `slot` of a launch takes point first + slot of `total`, reads
// it from `aff` (internal form, 2 coordinates), runs the ladder over record first + slot and leaves the XYZZ product at pts[first + slot].  A
// point at infinity gives infinity without a ladder; a zero scalar's record is all zero nibbles and leaves the accumulator where it starts.
template <class F, class G>
__global__ __launch_bounds__(64, G::ENABLED ? 2 : 1) void bases_scale_pass(const uint32_t *__restrict__ aff, const uint32_t *__restrict__ rec, uint32_t first,
                                                                          uint32_t total, uint32_t *__restrict__ pts, uint32_t *__restrict__ tbl) {
    constexpr int NL = FieldOps<F>::WORDS, PW = 4 * NL, HALVES = G::ENABLED ? 2 : 1;
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x, i = first + slot;
    if (i >= total) return;
    const XYZZ<F> p = XYZZ<F>::from_affine(affine_load<F>(aff + (size_t)i * (2 * NL)));
    uint32_t *pi = pts + (size_t)i * PW;
    if (p.is_inf()) {
        xyzz_store<F>(pi, XYZZ<F>::infinity());
        return;
    }
    ec_ladder<F, G>(p, rec + (size_t)i * REC_WORDS, tbl + (size_t)slot * (8 * HALVES) * PW, pi);
}

// the butterflies of stage s: (u, v) at distance 2^(s-1) -> (u + v, u - v)
template <class F>
__global__ __launch_bounds__(64) void ec_ntt_butterflies(uint32_t *__restrict__ pts, uint32_t log_m, uint32_t s) {
    typedef FieldOps<F> O;
    constexpr int NL = O::WORDS;
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x, m = 1u << log_m;
    if (b >= m / 2) return;
    const uint32_t half = 1u << (s - 1), k = b & (half - 1), i = ((b >> (s - 1)) << s) + k, j = i + half;
    XYZZ<F> u = xyzz_load<F>(pts + (size_t)i * (4 * NL)), v = xyzz_load<F>(pts + (size_t)j * (4 * NL));
    xyzz_store<F>(pts + (size_t)i * (4 * NL), xyzz_add(u, v));
    if (!v.is_inf()) v.Y = O::template sub<O::K2>(F::zero(), v.Y);
    xyzz_store<F>(pts + (size_t)j * (4 * NL), xyzz_add(u, v));
}

// device XYZZ -> canonical Jacobian
template <class F>
__global__ __launch_bounds__(64) void ec_ntt_store(const uint32_t *__restrict__ pts, uint32_t m, uint32_t *__restrict__ jac) {
    typedef FieldOps<F> O;
    constexpr int CW = O::CANON_WORDS, NL = O::WORDS;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    Jacobian<F> j = xyzz_to_jacobian(xyzz_load<F>(pts + (size_t)i * (4 * NL)));
    uint32_t *o = jac + (size_t)i * 3 * CW;
    O::to_canonical(o, j.X);
    O::to_canonical(o + CW, j.Y);
    O::to_canonical(o + 2 * CW, j.Z);
}

// ---- the boundary of zkhip_bases_lagrange: the affine rows of a bases object (internal form, 2 coordinates each), no canonical round trip
// affine -> device XYZZ at the bit-reversed position
template <class F>
__global__ __launch_bounds__(64) void ec_ntt_load_affine(const uint32_t *__restrict__ aff, uint32_t log_m, uint32_t *__restrict__ pts) {
    constexpr int NL = FieldOps<F>::WORDS;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, m = 1u << log_m;
    if (i >= m) return;
    const uint32_t r = log_m ? (__brev(i) >> (32 - log_m)) : 0;
    xyzz_store<F>(pts + (size_t)r * (4 * NL), XYZZ<F>::from_affine(affine_load<F>(aff + (size_t)i * (2 * NL))));
}

// device XYZZ -> affine.  A lane takes `chunk` consecutive points (affine_chunk): the running product of their denominators ZZ ZZZ goes to `pre`
// (one field element per point), ONE inversion serves the chunk (Montgomery's trick), points at infinity are skipped.  The walk is curve.hpp's
// xyzz_parked_to_affine spelled out: through the helper the kernel measured slower (EXPERIMENTS 22).
template <class F>
__global__ __launch_bounds__(64) void ec_ntt_store_affine(const uint32_t *__restrict__ pts, uint32_t m, uint32_t chunk, uint32_t *__restrict__ aff,
                                                          uint32_t *__restrict__ pre_buf) {
    typedef FieldOps<F> O;
    constexpr int NL = O::WORDS;
    const size_t first = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * chunk;
    if (first >= m) return;
    const uint32_t cnt = m - first < chunk ? (uint32_t)(m - first) : chunk;
    F pre = F::one();
    for (uint32_t k = 0; k < cnt; ++k) {
        const size_t i = first + k;
        const XYZZ<F> q = xyzz_load<F>(pts + i * (4 * NL));
        if (!q.is_inf()) pre = O::mul(pre, O::mul(q.ZZ, q.ZZZ));
        O::store(pre_buf + i * NL, pre);
    }
    F inv = O::inv(pre);
    for (uint32_t k = cnt; k-- > 0;) {
        const size_t i = first + k;
        const XYZZ<F> q = xyzz_load<F>(pts + i * (4 * NL));
        if (q.is_inf()) {
            affine_store<F>(aff + i * (2 * NL), Affine<F>::infinity());
            continue;
        }
        const F before = k > 0 ? O::load(pre_buf + (i - 1) * NL) : F::one();
        const F dinv = O::mul(inv, before);
        inv = O::mul(inv, O::mul(q.ZZ, q.ZZZ));
        const Affine<F> a = {O::mul(q.X, O::mul(dinv, q.ZZZ)), O::mul(q.Y, O::mul(dinv, q.ZZ))};
        affine_store<F>(aff + i * (2 * NL), a);
    }
}

// table slots: the lanes of one multiplication launch over `lanes` points (<= 1 GiB of tables, or "ec_ntt_table_lanes"; a pass over more lanes
// runs in several launches)
inline uint32_t ec_table_slots(const zkhip_ctx *ctx, size_t lanes, size_t slot_bytes) {
    const size_t slot_cap = ctx->opt_ec_ntt_table_lanes ? (((size_t)ctx->opt_ec_ntt_table_lanes + 63) & ~(size_t)63) : ((size_t)1 << 30) / slot_bytes / 64 * 64;
    return (uint32_t)std::max<size_t>(64, std::min<size_t>((lanes + 63) & ~(size_t)63, slot_cap));
}

struct EcNttBuffers {  // sizes in u32 words
    size_t pts_words, rec_words, tbl_words, aux_words;
    uint32_t *pts, *rec, *rec_last, *consts, *tbl, *aux;
    template <class Arena>
    void layout(Arena &a) {
        a.take(pts, pts_words);
        a.take(rec, rec_words);
        a.take(rec_last, rec_words);
        a.take(consts, 128);
        a.take(tbl, tbl_words);
        a.take(aux, aux_words);
    }
};
// The stage network between a load and a store stage: load(pts) enqueues the kernel that fills the 2^log_m XYZZ points (bit-reversed),
// store(pts, aux) the one that takes them away (natural order); aux: `aux_words` words of the workspace for the store stage.
template <class F, class U, class G, class Load, class Store>
int ec_ntt_run(zkhip_ctx *ctx, size_t log_m, const uint64_t *omega, int inverse, size_t aux_words, Load load, Store store) {
    constexpr int NL = FieldOps<F>::WORDS, PW = 4 * NL, HALVES = G::ENABLED ? 2 : 1;
    const uint32_t m = 1u << log_m, ntw = std::max<uint32_t>(1, m / 2);
    const size_t slot_bytes = (size_t)8 * HALVES * PW * 4;
    const uint32_t slots = ec_table_slots(ctx, m, slot_bytes);
    EcNttBuffers w = {(size_t)m * PW, (size_t)ntw * REC_WORDS, (size_t)slots * slot_bytes / 4, aux_words};
    ZK_TRY(ws_place(ctx, w));
    uint32_t *pts = w.pts, *rec = w.rec, *rec_last = w.rec_last, *consts = w.consts, *tbl = w.tbl;
    uint32_t *d_w = consts + 32, *d_one = consts + 48, *rec_minv = consts + 64;
    uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    ZK_TRY(ws_upload(ctx, d_w, omega, 32));
    ZK_LAUNCH(ctx, "ec_ntt_setup", ec_ntt_setup<U>, dim3(1), dim3(64), 0, d_w, (uint32_t)log_m, inverse, consts);
    ZK_LAUNCH(ctx, "ec_ntt_records", (ec_ntt_records<U, G>), grid_1d(ntw), dim3(256), 0, consts, (const uint32_t *)nullptr, 0u, ntw, rec);
    if (inverse && log_m > 0) {
        ZK_TRY(ws_upload(ctx, d_one, one, 32));
        ZK_LAUNCH(ctx, "ec_ntt_records", (ec_ntt_records<U, G>), grid_1d(ntw), dim3(256), 0, consts, consts + U::NL, 0u, ntw, rec_last);
        ZK_LAUNCH(ctx, "ec_ntt_records", (ec_ntt_records<U, G>), dim3(1), dim3(256), 0, d_one, consts + U::NL, 0u, 1u, rec_minv);
    }
    ZK_TRY(load(pts));
    for (uint32_t s = 1; s <= log_m; ++s) {
        const int mode = (inverse && s == log_m) ? 1 : 0;
        const uint32_t total = mode ? m : m / 2;
        if (mode == 1 || s > 1)  // stage 1 has no twiddle but 1
            for (uint32_t first = 0; first < total; first += slots) {
                const uint32_t lanes = std::min(slots, total - first);
                ZK_LAUNCH(ctx, "ec_ntt_mul_pass", (ec_ntt_mul_pass<F, G>), grid_1d(lanes, 64), dim3(64), 0, pts, rec, rec_last, rec_minv, (uint32_t)log_m, s,
                          mode, first, total, tbl);
            }
        ZK_LAUNCH(ctx, "ec_ntt_butterflies", ec_ntt_butterflies<F>, grid_1d(m / 2, 64), dim3(64), 0, pts, (uint32_t)log_m, s);
    }
    return store(pts, w.aux);
}

template <class F, class U, class G>
int ec_ntt_t(zkhip_ctx *ctx, uint32_t *d_jac, size_t log_m, const uint64_t *omega, int inverse) {
    const uint32_t m = 1u << log_m;
    return ec_ntt_run<F, U, G>(
        ctx, log_m, omega, inverse, 0,
        [&](uint32_t *pts) -> int {
            ZK_LAUNCH(ctx, "ec_ntt_load", ec_ntt_load<F>, grid_1d(m, 64), dim3(64), 0, d_jac, (uint32_t)log_m, pts);
            return ZKHIP_OK;
        },
        [&](uint32_t *pts, uint32_t *) -> int {
            ZK_LAUNCH(ctx, "ec_ntt_store", ec_ntt_store<F>, grid_1d(m, 64), dim3(64), 0, pts, m, d_jac);
            return ZKHIP_OK;
        });
}

// slot 0 of dst <- the inverse transform of src's rows offset .. offset + 2^log_m
template <class F, class U, class G>
int bases_lagrange_t(zkhip_ctx *ctx, const zkhip_bases *src, size_t offset, size_t log_m, const uint64_t *omega, zkhip_bases *dst) {
    constexpr int NL = FieldOps<F>::WORDS;
    const uint32_t m = 1u << log_m, chunk = affine_chunk(m);
    const uint32_t *in = src->d + offset * src->stride_u32;  // slot 0: the points themselves, whatever tables the object carries
    return ec_ntt_run<F, U, G>(
        ctx, log_m, omega, 1, (size_t)m * NL,
        [&](uint32_t *pts) -> int {
            ZK_LAUNCH(ctx, "ec_ntt_load_affine", ec_ntt_load_affine<F>, grid_1d(m, 64), dim3(64), 0, in, (uint32_t)log_m, pts);
            return ZKHIP_OK;
        },
        [&](uint32_t *pts, uint32_t *pre) -> int {
            ZK_LAUNCH(ctx, "ec_ntt_store_affine", ec_ntt_store_affine<F>, grid_1d((m + chunk - 1) / chunk, 64), dim3(64), 0, pts, m, chunk, dst->d.p, pre);
            return ZKHIP_OK;
        });
}

// ---- zkhip_bases_scale_dev / zkhip_bases_scale_geometric: slot 0 of dst <- s_i * (row offset + i of src), i < n
struct ScaleBuffers {  // sizes in u32 words
    size_t pts_words, rec_words, tbl_words, pre_words;
    uint32_t *pts, *rec, *consts, *tbl, *pre;
    template <class Arena>
    void layout(Arena &a) {
        a.take(pts, pts_words);
        a.take(rec, rec_words);
        a.take(consts, 32);
        a.take(tbl, tbl_words);
        a.take(pre, pre_words);
    }
};
// The records come from d_scalars (n resident 8-word scalars) or, when that is null, are those of coeff ratio^(e0 + i) (coeff nullable: 1).
template <class F, class U, class G>
int bases_scale_t(zkhip_ctx *ctx, const zkhip_bases *src, size_t offset, size_t n, const uint32_t *d_scalars, const uint64_t *ratio, const uint64_t *coeff,
                  uint32_t e0, zkhip_bases *dst) {
    constexpr int NL = FieldOps<F>::WORDS, PW = 4 * NL, HALVES = G::ENABLED ? 2 : 1;
    const uint32_t total = (uint32_t)n, chunk = affine_chunk(n);
    const size_t slot_bytes = (size_t)8 * HALVES * PW * 4;
    const uint32_t slots = ec_table_slots(ctx, n, slot_bytes);
    ScaleBuffers w = {n * PW, n * REC_WORDS, (size_t)slots * slot_bytes / 4, n * NL};
    ZK_TRY(ws_place(ctx, w));
    if (d_scalars) {
        ZK_LAUNCH(ctx, "scale_records_from_scalars", (scale_records_from_scalars<U, G>), grid_1d(n), dim3(256), 0, d_scalars, total, w.rec);
    } else {
        ZK_TRY(ws_upload(ctx, w.consts, ratio, 32));
        if (coeff) ZK_TRY(ws_upload(ctx, w.consts + 8, coeff, 32));
        ZK_LAUNCH(ctx, "scale_records_geometric", (ec_ntt_records<U, G>), grid_1d(n), dim3(256), 0, w.consts, coeff ? w.consts + 8 : (const uint32_t *)nullptr, e0,
                  total, w.rec);
    }
    const uint32_t *in = src->d + offset * src->stride_u32;  // slot 0: the points themselves, whatever tables the object carries
    for (uint32_t first = 0; first < total; first += slots) {
        const uint32_t lanes = std::min(slots, total - first);
        ZK_LAUNCH(ctx, "bases_scale_pass", (bases_scale_pass<F, G>), grid_1d(lanes, 64), dim3(64), 0, in, w.rec, first, total, w.pts, w.tbl);
    }
    ZK_LAUNCH(ctx, "ec_ntt_store_affine", ec_ntt_store_affine<F>, grid_1d((n + chunk - 1) / chunk, 64), dim3(64), 0, w.pts, total, chunk, dst->d.p, w.pre);
    return ZKHIP_OK;
}

}  // namespace

int zk_bases_scale(zkhip_ctx *ctx, const zkhip_bases *src, size_t offset, size_t n, const uint32_t *d_scalars, const uint64_t *ratio, const uint64_t *coeff,
                   uint32_t e0, zkhip_bases *dst) {
    if (dst->n != n || dst->stride_u32 != src->stride_u32 || dst->group != src->group) return ZKHIP_ERR_INVALID;
    if (src->group == GROUP_G1)
        return g1_dispatch(src->curve, [&](auto c) -> int {
            using C = decltype(c);
            return bases_scale_t<typename C::F, typename C::U, typename C::Glv>(ctx, src, offset, n, d_scalars, ratio, coeff, e0, dst);
        });
    if (src->curve == CURVE_BLS12_381) return bases_scale_t<CurveTraits<CURVE_BLS12_381, GROUP_G2>::F, BlsFrU, NoGlv>(ctx, src, offset, n, d_scalars, ratio, coeff, e0, dst);
    if (src->curve == CURVE_BN254) return bases_scale_t<CurveTraits<CURVE_BN254, GROUP_G2>::F, BnFrU, NoGlv>(ctx, src, offset, n, d_scalars, ratio, coeff, e0, dst);
    return ZKHIP_ERR_INVALID;
}

int zk_bases_lagrange(zkhip_ctx *ctx, const zkhip_bases *src, size_t offset, size_t log_m, const uint64_t *omega, bool glv, zkhip_bases *dst) {
    if (src->group != GROUP_G1 || dst->n != (size_t)1 << log_m || dst->stride_u32 != src->stride_u32) return ZKHIP_ERR_INVALID;
    return g1_dispatch(src->curve, [&](auto c) -> int {
        using C = decltype(c);
        if (glv) return bases_lagrange_t<typename C::F, typename C::U, typename C::Glv>(ctx, src, offset, log_m, omega, dst);
        // the plain ladder is kept for the two curves it was measured on (tools/bench_lagrange.py)
        if constexpr (C::ID == CURVE_PALLAS || C::ID == CURVE_VESTA) return bases_lagrange_t<typename C::F, typename C::U, NoGlv>(ctx, src, offset, log_m, omega, dst);
        return ZKHIP_ERR_INVALID;
    });
}

extern "C" int zkhip_ec_ntt_dev(zkhip_ctx *ctx, int curve, int group, void *d_jacobian, size_t log_m, const uint64_t *omega, int inverse) {
    // The pairing curves only.  (Pallas and Vesta have their GLV constants too -- glv.hpp -- and their group DFT is zkhip_bases_lagrange, over
    // bases objects; this entry point keeps to the curves whose powers-of-tau ceremony it serves.)
    ZK_ARGS_PAIRING(ctx, curve);
    if (!d_jacobian || !omega) return ZKHIP_ERR_INVALID;
    if (log_m > 26) return ZKHIP_ERR_RANGE;
    ZK_ENTER(ctx);
    uint32_t *d = (uint32_t *)d_jacobian;
    if (group == GROUP_G1)
        return g1_dispatch(curve, [&](auto c) -> int {
            using C = decltype(c);
            if constexpr (C::ID == CURVE_BLS12_381 || C::ID == CURVE_BN254) return ec_ntt_t<typename C::F, typename C::U, typename C::Glv>(ctx, d, log_m, omega, inverse);
            return ZKHIP_ERR_INVALID;
        });
    if (curve == CURVE_BLS12_381 && group == GROUP_G2) return ec_ntt_t<CurveTraits<CURVE_BLS12_381, GROUP_G2>::F, BlsFrU, NoGlv>(ctx, d, log_m, omega, inverse);
    if (curve == CURVE_BN254 && group == GROUP_G2) return ec_ntt_t<CurveTraits<CURVE_BN254, GROUP_G2>::F, BnFrU, NoGlv>(ctx, d, log_m, omega, inverse);
    return ZKHIP_ERR_INVALID;
}

