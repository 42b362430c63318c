/* zkhip -- C ABI of the MI355X-native MSM / NTT proving backend for NilFoundation/crypto3-zk.
 *
 * The reference is a header-only C++ template library with no FFI; its hot path leaves the repository at
 * the calls listed below (all into crypto3-algebra / crypto3-math).  Every entry point here states the
 * reference interface it replaces; INTEGRATION.md shows the C++ shim a crypto3-zk maintainer adds on top.
 *
 * Conventions
 *   - Plain C, caller owns every host buffer, nothing throws; return 0 on success, negative zkhip_status
 *     otherwise (the reference asserts, compiled out in release: prover.hpp:77,88-89; kzg.hpp:145,413).
 *   - Field elements cross the boundary as CANONICAL (non-Montgomery) little-endian 64-bit limbs:
 *       Fr (every curve) 4 limbs; BLS12-381 Fq 6 limbs; BN254, Pallas and Vesta Fq 4 limbs; Fq2 = c0 limbs then c1 limbs.
 *     G1 affine = x | y; G2 affine = x.c0 | x.c1 | y.c0 | y.c1.  Infinity travels as a separate flag.
 *     The reference's in-memory representation lives in crypto3-multiprecision (not observable from the
 *     zk tree), so the shim converts through canonical integers and never memcpy's reference objects.
 *   - Group results are returned as Jacobian (X, Y, Z) with x = X/Z^2, y = Y/Z^3 and Z = 0 for infinity,
 *     the 3-coordinate shape of the reference's G::value_type; compare in affine.
 *   - omega and the coset generator are ARGUMENTS (arithmetic_params<F> lives in crypto3-algebra).
 *   - One context per GPU per process (one process per GPU); a context is not thread-safe.  A caller that wants SEVERAL GPUs behind
 *     one call -- the shape of the reference, whose parallelism sits inside process() / commit() -- takes a device group
 *     (zkhip_group_init below): one context per GPU, the exchange inside the library.  The shim drives member 0 from the caller's
 *     thread and members 1..N-1 from host threads of its own (a caller's thread-local state does not reach them).
 *   - The library has no CPU fallback: without a usable HIP device every call fails with
 *     ZKHIP_ERR_NO_DEVICE.
 */
#ifndef ZKHIP_H
#define ZKHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zkhip_ctx zkhip_ctx;
typedef struct zkhip_bases zkhip_bases;

/* A curve id names a GROUP and ITS SCALAR FIELD -- for the Pasta cycle this is easy to get backwards:
 *     p = 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001   Pallas base field  = Vesta scalar field
 *     q = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001   Pallas scalar field = Vesta base field
 *   ZKHIP_PALLAS: points of y^2 = x^3 + 5 over F_p (generator (p - 1, 2)); its "Fr" -- scalars, NTT, polynomial and argument kernels -- is F_q.
 *   ZKHIP_VESTA:  points of y^2 = x^3 + 5 over F_q (generator (q - 1, 2)); its "Fr" is F_p.
 * A placeholder proof over pallas::base_field_type (= F_p) therefore runs under ZKHIP_VESTA.
 * Both have 4-limb Fq and Fr, G1 only (ZKHIP_G2 with either id is ZKHIP_ERR_INVALID), two-adicity 32.  The entry points that need a
 * pairing-friendly curve -- zkhip_r1cs_* / zkhip_groth16_*, zkhip_bases_upload_compressed (the wire format) and zkhip_ec_ntt_dev (the
 * powers-of-tau transform; their group DFT is zkhip_bases_lagrange, over bases objects) -- answer ZKHIP_ERR_INVALID for them. */
enum zkhip_curve { ZKHIP_BLS12_381 = 0, ZKHIP_BN254 = 1, ZKHIP_PALLAS = 2, ZKHIP_VESTA = 3 };
enum zkhip_group { ZKHIP_G1 = 1, ZKHIP_G2 = 2 };
enum zkhip_status {
    ZKHIP_OK = 0,
    ZKHIP_ERR_NO_DEVICE = -1,
    ZKHIP_ERR_INVALID = -2,
    ZKHIP_ERR_HIP = -3,
    ZKHIP_ERR_OOM = -4,
    ZKHIP_ERR_RANGE = -5,
    ZKHIP_ERR_NOT_FOUND = -6 /* a bounded search ended without a result (zkhip_pow_grind) */
};

/* ---- context -------------------------------------------------------------------------------- */
int zkhip_init(int device_id, zkhip_ctx **out);
void zkhip_destroy(zkhip_ctx *ctx);
const char *zkhip_strerror(int status);
const char *zkhip_last_error(const zkhip_ctx *ctx); /* HIP error text of the last ZKHIP_ERR_HIP */
/* All work is enqueued on this stream (default: a stream the context creates). */
int zkhip_set_stream(zkhip_ctx *ctx, void *hip_stream);
/* Two contexts on one GPU are two in-order streams (each with its own workspace).  zkhip_stream_wait(waiter, signal):
 * everything enqueued on `waiter` after this call runs after everything enqueued on `signal` before it (an event;
 * the host does not block).  The Groth16 shim runs the G2 multiexp of the B query on a second context this way, so
 * that its latency-bound reduction tail overlaps the G1 multiexps (prover.hpp:116-139 are independent). */
int zkhip_stream_wait(zkhip_ctx *waiter, zkhip_ctx *signal);
int zkhip_device(const zkhip_ctx *ctx);
int zkhip_sync(zkhip_ctx *ctx);
/* Sticky error flags raised by kernels since the last call (bit 0: a gather index out of range, bit 1: the MSM's
 * large-bucket plan overflowed its capacity, bit 2: zkhip_lookup_sort_dev met a looked-up value that is in no table, bit 3: its
 * emitted sequence does not fit the sorted vectors).  Synchronises the stream, clears the flags; returns ZKHIP_ERR_RANGE if
 * any was set (the results computed meanwhile are then not to be used).  The shims call it once per proof. */
int zkhip_device_status(zkhip_ctx *ctx, uint32_t *flags /* nullable */);
/* Tunables: "msm_window_bits" (0 = auto), "msm_sets" (bucket sets with window tables, 0 = auto), "msm_segment_log" (tail: 2^k buckets
 * per lane, < 0 = auto), "msm_tail_quads" (1: the tail of bucket sets up to 2^18 runs the group law over lane quads and level 2 of a lone MSM's two-level tail runs it with one point per wave, 2 or any other non-zero value: the quads alone -- a smaller setting than 1, kept as a value of this option until the option table may grow a row --, 0: pairs everywhere), "msm_tail_fold" (k > 0: the bucket reduction of table-backed sets of >= 2^k buckets is two-level -- row and column sums of the bucket index, then the old tail over 2 sets of ~sqrt(B) buckets; 0: off; default 16), "msm_fold_run" (buckets a lane of that kernel sums before the workgroup trees, 0 = auto), "msm_tail_fold_g2" (1: G2 sets too), "msm_share_sort" (1: consecutive members of zkhip_msm_batch_dev with the same scalars pointer, range and
 * table geometry share one digit extraction / sort / large-bucket plan; 0: every member sorts), "msm_sort_tile_log" (14: the MSM has the GPU to itself; 13: tiles of half that size, two workgroups per CU; 12: kernels of another context run alongside and
 * the sort's LDS tiles must fit next to them), "ntt_radix_log", "ntt_tile_log", "poly_coset_extend" (1: zkhip_poly_resize_dev grows n -> K n, K <= 16, by n-point transforms over the K - 1 new cosets; 0: one K n-point transform), "ec_ntt_table_lanes" (zkhip_ec_ntt_dev: points multiplied per launch = per-lane window tables held at
 * once; 0 = as many as fit 1 GiB), "msm_precompute" / "msm_precompute_min" (window
 * tables at upload), "msm_graphs" (HIP-graph replay of repeated MSM calls; off), "msm_shard_rank" / "msm_shard_world" (window
 * partition over GPUs: bases uploaded from now on hold the tables of windows {w : w mod world == rank} only, and an MSM over them
 * yields the partial sum of those windows). */
int zkhip_set_option(zkhip_ctx *ctx, const char *name, int64_t value);
/* "stream_priority" (value < 0: highest, > 0: lowest, 0: default) recreates the context's own stream with that scheduling priority:
 * of two contexts on one GPU the higher one's workgroups are dispatched first (set it before any work is enqueued). */
int zkhip_get_option(const zkhip_ctx *ctx, const char *name, int64_t *value);

/* ---- device memory (plumbing for callers that keep vectors resident) --------------------------
 * zkhip_free synchronises the device the block lives on and keeps the block for the next zkhip_malloc of its size class (option
 * "alloc_cache_mb": megabytes kept per context, default 16384, 0 = hand every block back at once); the cache is emptied at
 * zkhip_destroy and when the driver runs out of memory.
 * OWNERSHIP: a block belongs to the context it was allocated through, whichever context it is freed through (the free settles it with
 * its owner).  zkhip_destroy returns the CACHED blocks to the driver and leaves the blocks the caller still holds alone: they lose
 * their owner, stay valid, and a later zkhip_free through any live context hands them to hipFree.  A caller that wants its memory
 * back must therefore zkhip_free every block BEFORE (or after) destroying the context -- destroy does not reclaim live blocks
 * (the shim's shared_ptr handles may outlive their context and must not dangle). */
int zkhip_malloc(zkhip_ctx *ctx, size_t bytes, void **dptr);
int zkhip_free(zkhip_ctx *ctx, void *dptr);
int zkhip_memcpy_h2d(zkhip_ctx *ctx, void *dst, const void *src, size_t bytes);
int zkhip_memcpy_d2h(zkhip_ctx *ctx, void *dst, const void *src, size_t bytes);
/* enqueue only (no synchronisation): for pinned host buffers, ordered with the kernels on the context's stream */
int zkhip_memcpy_h2d_async(zkhip_ctx *ctx, void *dst, const void *src, size_t bytes);
/* the way back, enqueue only: `dst` must be page-locked (zkhip_host_alloc) and is valid after the next zkhip_sync.  The LPC shim
 * streams a precommitment's leaves to the caller's hash in slices this way: slice k + 1 is in flight while slice k is absorbed. */
int zkhip_memcpy_d2h_async(zkhip_ctx *ctx, void *dst, const void *src, size_t bytes);
/* page-locked host memory: H2D / D2H at link speed instead of through a staging copy */
/* device-to-device copy in stream order (no synchronisation) */
int zkhip_memcpy_d2d_async(zkhip_ctx *ctx, void *dst, const void *src, size_t bytes);
/* the strided form, same device, stream order: `rows` rows of `width` bytes, row r from src + r * src_pitch to dst + r * dst_pitch
 * (width <= both pitches; the two regions must not overlap).  What the LPC shim over a device group packs a member's share of the
 * evaluations with: the 2^fri_step segments of every polynomial that one leaf owner's leaves are made of (hip/lpc.hpp). */
int zkhip_memcpy_2d_d2d_async(zkhip_ctx *ctx, void *dst, size_t dst_pitch, const void *src, size_t src_pitch, size_t width, size_t rows);
int zkhip_host_alloc(zkhip_ctx *ctx, size_t bytes, void **hptr);
int zkhip_host_free(zkhip_ctx *ctx, void *hptr);

/* ---- resident bases: proving-key queries / SRS ------------------------------------------------
 * Replaces the `bases_begin, bases_end` iterator pair of algebra::multiexp at
 *   r1cs_gg_ppzksnark/prover.hpp:108-139 (A_query, B_query, H_query, L_query; layout proving_key.hpp:43-56)
 *   commitments/polynomial/kzg.hpp:143-148, 409-435 (params.commitment_key)
 * Upload once, reuse for every proof.
 * ZKHIP_PALLAS / ZKHIP_VESTA: a coordinate that is not below the base-field modulus (their 4 limbs can hold one) is ZKHIP_ERR_INVALID. */
int zkhip_bases_upload(zkhip_ctx *ctx, int curve, int group, const uint64_t *affine_xy, const uint8_t *is_infinity /* nullable */,
                       size_t n, zkhip_bases **out);
/* out[i] = scalars[i] * base (base == NULL: the standard generator), computed on the device and left
 * resident.  Replaces algebra::batch_exp / kc_batch_exp (generator.hpp:187-214,
 * knowledge_commitment_multiexp.hpp:143-208) and structured_generators_scalar_power (ipp2/srs.hpp:44-56). */
/* The same from the WIRE form of a proving key (g16/marshalling.hpp:111-112, 178-201): n compressed
 * BLS12-381 points, 48 bytes each for G1, 96 for G2 (big-endian x, G2: x.c1 then x.c0; byte 0 carries the flags
 * 0x80 compressed, 0x40 infinity, 0x20 larger y) -- the encoding pinned by the vectors of
 * r1cs_gg_ppzksnark_aggregation_conformity.cpp:932-1010.  Decoded on the device (one square root per point).
 * ZKHIP_ERR_INVALID if any encoding is malformed or not on the curve (zkhip_last_error says how many). */
int zkhip_bases_upload_compressed(zkhip_ctx *ctx, int curve, int group, const uint8_t *octets, size_t n, zkhip_bases **out);
int zkhip_bases_from_scalars(zkhip_ctx *ctx, int curve, int group, const uint64_t *base_affine_xy /* nullable */,
                             const uint64_t *scalars, size_t n, zkhip_bases **out);
/* A bases object of n_total points holding src's points at the rows d_rows[j] (a DEVICE array of src's size; NULL: the consecutive rows
 * first + j) and the point at infinity everywhere else, with its own window tables.  What it is for: queries of one proof that are
 * multiplied by the same assignment vector -- A_query, the B query's G1 half (sparse: its index list is d_rows), L_query (the auxiliary
 * part: first = n + 1) -- laid out over the SAME rows share one digit extraction and sort in zkhip_msm_batch_dev ("msm_share_sort").
 * d_rows must be STRICTLY INCREASING; a row beyond n_total or a repeated / out-of-order row raises the gather flag of
 * zkhip_device_status (a repeated row would overwrite a point). */
int zkhip_bases_spread(zkhip_ctx *ctx, const zkhip_bases *src, const uint32_t *d_rows /* nullable */, size_t first, size_t n_total,
                       zkhip_bases **out);
int zkhip_bases_download(zkhip_ctx *ctx, const zkhip_bases *b, size_t offset, size_t n, uint64_t *affine_xy, uint8_t *is_infinity);
size_t zkhip_bases_size(const zkhip_bases *b);
void zkhip_bases_free(zkhip_ctx *ctx, zkhip_bases *b);

/* ---- MSM ---------------------------------------------------------------------------------------
 * sum_{i<n} scalars[i] * bases[offset + i].
 * Replaces algebra::multiexp<multiexp_method_BDLO12>(b0, b1, s0, s1, chunks) and
 * multiexp_with_mixed_addition (prover.hpp:108-139, kzg.hpp:143-148,409-435,505-508,
 * knowledge_commitment_multiexp.hpp:107).  `chunks` has no counterpart: the device splits the work itself.
 * out_jacobian: 3 * (coordinate limbs) u64, canonical X | Y | Z of the group element; WHICH projective representative comes out is
 * not fixed (the order of additions inside a bucket follows the sort's atomics): compare points after zkhip_jacobian_to_affine,
 * as the reference's own operator== normalises before comparing.
 * The context keeps the device copy of the scalars (32 n bytes, grow-only, freed by zkhip_destroy): a prover's repeated calls neither allocate nor free, and
 * replay their launch sequence as a HIP graph. */
int zkhip_msm(zkhip_ctx *ctx, const zkhip_bases *bases, size_t offset, size_t n, const uint64_t *scalars /* host, n x 4 */,
              uint64_t *out_jacobian /* host */);
/* Same, scalars and result resident in device memory; asynchronous on the context's stream. */
int zkhip_msm_dev(zkhip_ctx *ctx, const zkhip_bases *bases, size_t offset, size_t n, const void *d_scalars, void *d_out_jacobian);
/* `count` MSMs whose results are needed together (the queries of one Groth16 proof, the columns of a KZG batch):
 * same semantics as `count` calls of zkhip_msm_dev, but the latency-bound bucket reductions of all of them run as
 * one launch when the bases share group and window size (otherwise the calls simply run one after the other). */
int zkhip_msm_batch_dev(zkhip_ctx *ctx, size_t count, const zkhip_bases *const *bases, const size_t *offsets, const size_t *ns,
                        const void *const *d_scalars, void *const *d_out_jacobian);
/* d_out = sum of `count` Jacobian points (canonical, 3 coordinates each) resident in device memory: the
 * fold of per-GPU partial MSM results after the all-gather (RCCL has no elliptic-curve reduction). */
int zkhip_jacobian_sum_dev(zkhip_ctx *ctx, int curve, int group, const void *d_points, size_t count, void *d_out_jacobian);
/* Jacobian -> affine on the device (one inversion); is_infinity receives 0/1. */
int zkhip_jacobian_to_affine(zkhip_ctx *ctx, int curve, int group, const uint64_t *jacobian, uint64_t *affine_xy, uint8_t *is_infinity);

/* ---- NTT ---------------------------------------------------------------------------------------
 * In-place radix-2 transform of `batch` vectors of m = 2^log_m Fr elements, natural order in and out:
 *   forward:  [coset != NULL: v[j] *= coset^j;]  out[i] = sum_j v[j] omega^(ij)
 *   inverse:  out[j] = (1/m) sum_i v[i] omega^(-ij);  [coset != NULL: out[j] *= coset^(-j)]
 * Replaces evaluation_domain<F>::fft / inverse_fft and math::multiply_by_coset
 * (reductions/r1cs_to_qap.hpp:250-315; column_polynomial.hpp:53; the polynomial_dfs::coefficients /
 * resize calls of kzg.hpp:431 and basic_fri.hpp:452-455). */
int zkhip_ntt(zkhip_ctx *ctx, int curve, uint64_t *data /* host, batch x m x 4 */, size_t log_m, size_t batch,
              const uint64_t *omega /* 4 limbs */, int inverse, const uint64_t *coset_gen /* nullable, 4 limbs */);
int zkhip_ntt_dev(zkhip_ctx *ctx, int curve, void *d_data, size_t log_m, size_t batch, const uint64_t *omega, int inverse,
                  const uint64_t *coset_gen);

/* ---- evaluation domains ------------------------------------------------------------------------------
 * What math::make_evaluation_domain<Fr>(min_size) returns (reductions/r1cs_to_qap.hpp:138-139, 229-230 call it with
 * num_constraints + num_inputs + 1, which is rarely a power of two).  crypto3-math is not part of the reference tree; the
 * family and the selection order are those of its libfqfft lineage: basic_radix2 (m = 2^k), extended_radix2
 * (m = 2^(s+1), s the field's two-adicity) and step_radix2 (m = 2^k + 2^j), tried at min_size and then at
 * big + rounded_small.  The point sets, in get_domain_element order:
 *   basic     omega^i, i < m                                    omega = primitive m-th root of unity
 *   extended  omega^i, then shift omega^i, i < m/2              omega = primitive (m/2)-th root
 *   step      omega^(2i), i < big, then omega (omega^(2 big/small))^i, i < small
 *                                                               omega = primitive (2 big)-th root (the domain's `omega` member)
 * The roots are ARGUMENTS like everywhere in this ABI (arithmetic_params<F> lives in crypto3-algebra); a root of the
 * wrong order is refused (ZKHIP_ERR_INVALID). */
enum zkhip_domain_kind { ZKHIP_DOMAIN_BASIC_RADIX2 = 0, ZKHIP_DOMAIN_EXTENDED_RADIX2 = 1, ZKHIP_DOMAIN_STEP_RADIX2 = 2 };
typedef struct zkhip_domain {
    int32_t kind;      /* zkhip_domain_kind */
    uint32_t reserved; /* 0 */
    uint64_t m;        /* number of points */
    uint64_t omega[4]; /* see above */
    uint64_t shift[4]; /* extended: detail::coset_shift<F>() (= multiplicative_generator^2); ignored otherwise */
} zkhip_domain;
/* (kind, m) make_evaluation_domain(min_size) picks over the curve's scalar field (two-adicity 32 for BLS12-381, Pallas and Vesta, 28 for BN254).
 * ZKHIP_ERR_RANGE when only a geometric / arithmetic sequence domain would do (beyond 2^(s+1) points: out of scope). */
int zkhip_domain_choice(int curve, size_t min_size, int *kind, size_t *m);
/* evaluation_domain::evaluate_all_lagrange_polynomials(t) (reductions/r1cs_to_qap.hpp:152-153, the key generator's QAP evaluation
 * at the trapdoor): d_out[i] = L_i(t) for every point of the domain, in get_domain_element order (m canonical Fr elements,
 * device), by the closed forms of the three radix-2 kinds with one batched inversion per 16 points.  ZKHIP_ERR_INVALID when t lies
 * in the domain (the closed forms do not cover it; a trapdoor must not lie there anyway). */
int zkhip_domain_lagrange_dev(zkhip_ctx *ctx, int curve, const zkhip_domain *dom, const uint64_t *t, void *d_out);
/* evaluation_domain<F>::fft / inverse_fft over any of the three domains, in place on `batch` vectors of dom->m Fr elements:
 *   forward:  [coset != NULL: v[j] *= coset^j;]  out[i] = sum_j v[j] x_i^j        (x_i = get_domain_element(i))
 *   inverse:  the interpolation;  [coset != NULL: out[j] *= coset^(-j)]
 * For the basic kind this is zkhip_ntt_dev. */
int zkhip_domain_fft_dev(zkhip_ctx *ctx, int curve, const zkhip_domain *dom, void *d_data, size_t batch, int inverse, const uint64_t *coset_gen);

/* ---- Groth16 witness map ------------------------------------------------------------------------
 * Resident R1CS in CSR form (three matrices A, B, C; column 0 is the constant 1, column j >= 1 is variable
 * j - 1; coefficients canonical Fr, 4 limbs each).  Replaces the constraint_system member of the proving key
 * (r1cs_gg_ppzksnark/proving_key.hpp:56; r1cs.hpp:61-64,125-133) as consumed by
 * reductions::r1cs_to_qap<F>::witness_map (reductions/r1cs_to_qap.hpp:219-325). */
typedef struct zkhip_r1cs zkhip_r1cs;
int zkhip_r1cs_upload(zkhip_ctx *ctx, int curve, size_t num_constraints, size_t num_inputs, size_t num_variables, const uint32_t *rowptr_a,
                      const uint32_t *col_a, const uint64_t *coeff_a, const uint32_t *rowptr_b, const uint32_t *col_b, const uint64_t *coeff_b,
                      const uint32_t *rowptr_c, const uint32_t *col_c, const uint64_t *coeff_c, zkhip_r1cs **out);
void zkhip_r1cs_free(zkhip_ctx *ctx, zkhip_r1cs *r);
/* The evaluation domain the witness map reduces over.  After upload it is (kind, m) = what
 * make_evaluation_domain(num_constraints + num_inputs + 1) picks (r1cs_to_qap.hpp:229-230; zkhip_domain_choice) -- a step
 * radix-2 domain for most instances.  zkhip_r1cs_set_domain installs another kind / size (m >= num_constraints + num_inputs + 1),
 * e.g. the basic domain of the next power of two for a key that was generated over that one; only kind and m are read
 * (the roots come with every witness-map call). */
int zkhip_r1cs_set_domain(zkhip_r1cs *r, int kind, size_t m);
size_t zkhip_r1cs_domain_size(const zkhip_r1cs *r);
int zkhip_r1cs_domain_kind(const zkhip_r1cs *r);
size_t zkhip_groth16_scratch_bytes(const zkhip_r1cs *r);
/* coefficients_for_H of witness_map with d1 = d2 = d3 = 0 (as prover.hpp:79-83 calls it): m + 1 Fr elements
 * written to d_h.  d_assignment = (1, primary_input, auxiliary_input), num_variables + 1 elements, device
 * resident; omega = the `omega` of the constraint system's evaluation domain (see zkhip_domain: the primitive m-th root for the
 * basic kind, the primitive (2 big)-th root for the step kind); coset_gen = the field's multiplicative generator
 * (arithmetic_params<F>::multiplicative_generator).  3 sparse mat-vecs, 7 transforms and one fused pointwise pass, all on
 * the context's stream; the result feeds zkhip_msm_dev directly.  An extended radix-2 domain also needs its shift: use
 * zkhip_groth16_witness_h_domain_dev, which takes the whole domain description (its kind and m must match the constraint
 * system's). */
int zkhip_groth16_witness_h_dev(zkhip_ctx *ctx, const zkhip_r1cs *r, const void *d_assignment, const uint64_t *omega,
                                const uint64_t *coset_gen, void *d_h, void *d_scratch);
int zkhip_groth16_witness_h_domain_dev(zkhip_ctx *ctx, const zkhip_r1cs *r, const void *d_assignment, const zkhip_domain *dom,
                                       const uint64_t *coset_gen, void *d_h, void *d_scratch);

/* d_dst[j] = d_src[d_indices[j]] on Fr elements (u32 indices): gathers the scalars of a sparse query, i.e. the
 * `*(scalar_start + scalar_position)` walk over vec.indices of kc_multiexp_with_mixed_addition
 * (knowledge_commitment_multiexp.hpp:66-100).  Zero and one scalars need no peeling on the device. */
/* d_src holds src_count elements; an index >= src_count (malformed key) gathers the zero scalar and raises the sticky
 * device status (zkhip_device_status). */
int zkhip_fr_gather_dev(zkhip_ctx *ctx, const void *d_src, size_t src_count, const void *d_indices, size_t count, void *d_dst);

/* ---- LPC / FRI polynomial helpers on top of the NTT -------------------------------------------------
 * polynomial_dfs::resize as precommit<FRI> applies it to every committed polynomial
 * (commitments/detail/polynomial/basic_fri.hpp:452-455): `batch` vectors of 2^log_n evaluations at d_in
 * (CONSUMED: left holding the coefficients) -> 2^log_out evaluations each at d_out.  omega_n / omega_out are the
 * primitive roots of the two domains.  Any pair of primitive roots is accepted; when they are NESTED (omega_out^(2^(log_out - log_n))
 * == omega_n, as roots drawn from one generator are) and the growth is at most 16-fold, only the new cosets are evaluated ("poly_coset_extend"). */
int zkhip_poly_resize_dev(zkhip_ctx *ctx, int curve, void *d_in, size_t log_n, size_t batch, const uint64_t *omega_n, void *d_out,
                          size_t log_out, const uint64_t *omega_out);
/* log_out < log_n (a SMALLER domain, for a polynomial whose degree fits it): d_out receives every 2^(log_n - log_out)-th
 * evaluation, d_in is left untouched.
 * math::polynomial_shift(f, shift, domain_size) on the evaluation vector (ph/permutation_argument.hpp:148,
 * lookup_argument.hpp:232): d_out[i] = d_in[(i + rotation) mod 2^log_size], rotation = shift * (size / domain_size), may be
 * negative; d_out must not alias d_in. */
int zkhip_poly_shift_dev(zkhip_ctx *ctx, const void *d_in, size_t log_size, int64_t rotation, void *d_out);
/* d_out[i] = prod_k d_in[k][i], i < n: the pointwise core of math::polynomial_product (ph/permutation_argument.hpp:148,
 * gates_argument.hpp:117) once every factor sits on the product's domain (zkhip_poly_resize_dev); d_in is a HOST array of
 * `count` device pointers, d_out may be one of them. */
int zkhip_fr_vec_prod_dev(zkhip_ctx *ctx, int curve, size_t count, const void *const *d_in, void *d_out, size_t n);

/* detail::fold_polynomial, DFS form (commitments/detail/polynomial/fold_polynomial.hpp:68-93):
 * d_out[i] = 1/2 [(1 + alpha omega^-i) d_f[i] + (1 - alpha omega^-i) d_f[i + size/2]], i < size/2 = 2^(log_size-1). */
int zkhip_fri_fold_dev(zkhip_ctx *ctx, int curve, const void *d_f, size_t log_size, const uint64_t *alpha, const uint64_t *omega, void *d_out);

/* The leaf layout precommit<FRI> feeds to the Merkle tree (basic_fri.hpp:456-492, FRI::m = 2): `batch` vectors of
 * 2^log_domain evaluations at d_polys -> d_out, 2^log_domain / 2^fri_step leaves of batch * 2^fri_step elements each:
 * leaf x = for every polynomial, the pairs (f[s_i], f[s_i + D/2]) in the reference's coset order.  Hashing is
 * the caller's, or zkhip_merkle_build_fri_dev's below. */
int zkhip_fri_leaves_dev(zkhip_ctx *ctx, const void *d_polys, size_t log_domain, size_t batch, size_t fri_step, void *d_out);

/* ---- Merkle trees (SHA2-256) of the LPC / FRI commitments, built and kept on the device ----------------------------
 * The tree precommit<FRI> builds with make_merkle_tree<Hash, 2> over the leaves above (basic_fri.hpp:375-409, 461-496), for
 * Hash = hashes::sha2<256>.  THE CONTRACT (crypto3's containers::merkle_tree was not at hand when this was written, so the
 * layout below is stated here and checked against an independent SHA2-256, not pinned to a reference vector):
 *   element bytes   a field element is 32 bytes: the BIG-ENDIAN encoding of its canonical integer (marshalling's
 *                   field_element with option::big_endian, basic_fri.hpp:96-97), for both curves' Fr;
 *   leaf digest     SHA2-256 of the leaf's elements concatenated in leaf order (the order zkhip_fri_leaves_dev writes);
 *   inner node      SHA2-256(left digest || right digest), 64 bytes;
 *   shape           arity 2, L leaves, L a power of two >= 1; with one leaf the root is that leaf's digest;
 *   digest array    (2L - 1) x 32 bytes: the leaf digests at [0, L), the next level at [L, L + L/2), ..., the root last.
 * A tree stays resident (64 MB at 2^20 leaves) until zkhip_merkle_free.  `hash` selects the hash function: only
 * ZKHIP_HASH_SHA2_256 exists.
 * Errors: unknown hash, null pointers, a leaf count that is not a power of two, no elements per leaf -> ZKHIP_ERR_INVALID;
 * a leaf index >= L, fri_step outside zkhip_fri_leaves_dev's range -> ZKHIP_ERR_RANGE; allocation failure -> ZKHIP_ERR_OOM. */
#define ZKHIP_HASH_SHA2_256 0
typedef struct zkhip_merkle zkhip_merkle;
/* over a leaf layout on the device: n_leaves leaves of elements_per_leaf elements each */
int zkhip_merkle_build_dev(zkhip_ctx *ctx, int hash, const void *d_leaves, size_t n_leaves, size_t elements_per_leaf, zkhip_merkle **out);
/* over the leaves zkhip_fri_leaves_dev would write for the same arguments, hashed straight from the evaluations at d_polys
 * (the leaf layout is never materialised); byte for byte the tree of zkhip_fri_leaves_dev + zkhip_merkle_build_dev */
int zkhip_merkle_build_fri_dev(zkhip_ctx *ctx, int hash, const void *d_polys, size_t log_domain, size_t batch, size_t fri_step, zkhip_merkle **out);
size_t zkhip_merkle_leaves(const zkhip_merkle *t);
size_t zkhip_merkle_depth(const zkhip_merkle *t); /* log2(L): the length of a path */
int zkhip_merkle_root(zkhip_ctx *ctx, const zkhip_merkle *t, uint8_t out[32]);
int zkhip_merkle_digests(zkhip_ctx *ctx, const zkhip_merkle *t, uint8_t *out /* host, (2L - 1) x 32 */);
/* the authentication paths of `count` leaves: per index the `depth` sibling digests from the leaf level up, gathered on the
 * device and fetched in one copy */
int zkhip_merkle_paths(zkhip_ctx *ctx, const zkhip_merkle *t, const uint64_t *leaf_indices /* host */, size_t count,
                       uint8_t *out /* host, count x depth x 32 */);
void zkhip_merkle_free(zkhip_ctx *ctx, zkhip_merkle *t);

/* ---- The FRI query phase's answers (basic_fri.hpp:747-930), read from what is resident --------------------------------
 * Both entries take the queries' domain indices on the host and return the answers on the host; each is ONE launch and ONE
 * device-to-host copy, synchronised: the answers are in `out` when the call returns.  Neither takes a curve id: both gather
 * canonical 32-byte values and compute nothing.
 *
 * zkhip_fri_query_dev: a SET is `batch` vectors of D = 2^log_domain canonical 4-limb elements at d_polys, laid out as
 * zkhip_fri_leaves_dev takes them.  For query q the set uses x = x_indices[q] mod D; its answer for (q, polynomial p) is the
 * 2^(fri_step - 1) pairs calculate_s walks from x (basic_fri.hpp:585-614): s_0 = x, then for the offsets D/4, D/8, ...
 * s_i = (offset + s_j) mod D over the already placed j, each pair being (f[min(s_i, s_i + D/2 mod D)], f[max(...)]) -- the
 * ind0 / ind1 rule of :815-818 and :892-895.  As a set of values that is leaf (x mod (D >> fri_step)) of zkhip_fri_leaves_dev,
 * and in that leaf's own order when x < (D >> fri_step).
 *   out        set-major: set t holds [q][p][i][2] elements of 4 u64 limbs, at element offset count * sum_{u<t} batch_u 2^(fri_step_u);
 *   errors     (all before anything is launched) a null ctx, or with work to do a null sets / x_indices / out / d_polys or
 *              batch == 0 -> ZKHIP_ERR_INVALID; fri_step < 1, fri_step > log_domain, log_domain > 32, batch >= 2^31, count >= 2^32 or
 *              an index >= 2^(the largest log_domain among the sets) -> ZKHIP_ERR_RANGE;
 *   count == 0 or n_sets == 0: ZKHIP_OK, nothing launched. */
typedef struct { const void *d_polys; size_t log_domain; size_t batch; size_t fri_step; } zkhip_fri_query_set;
int zkhip_fri_query_dev(zkhip_ctx *ctx, const zkhip_fri_query_set *sets, size_t n_sets,
                        const uint64_t *x_indices /* host */, size_t count, uint64_t *out /* host */);
/* zkhip_merkle_paths over several trees of the context at once: tree t answers leaf x_indices[q] mod leaves(t) -- the reduction
 * get_folded_index makes per round (basic_fri.hpp:857-860, 868-874).
 *   out        tree-major: [t][q][depth_t][32], byte for byte what zkhip_merkle_paths writes per tree for the reduced indices; a
 *              one-leaf tree contributes no bytes;
 *   errors     a null ctx, trees or tree, or with digests to write a null x_indices / out -> ZKHIP_ERR_INVALID;
 *              count >= 2^32 -> ZKHIP_ERR_RANGE;   count == 0 or n_trees == 0: ZKHIP_OK, nothing launched. */
int zkhip_merkle_paths_multi(zkhip_ctx *ctx, const zkhip_merkle *const *trees, size_t n_trees,
                             const uint64_t *x_indices /* host */, size_t count, uint8_t *out /* host */);

/* ---- Proof of work (FRI grinding) over the SHA2-256 sequential transcript, searched on the device ---------------------
 * proof_of_work<hashes::sha2<256>, std::uint32_t>::generate (commitments/detail/polynomial/proof_of_work.hpp:47-68), which
 * proof_eval<FRI> calls between its commit and query phases when fri_params.use_grinding is set (basic_fri.hpp:743-745), over
 * transcript::fiat_shamir_heuristic_sequential<sha2<256>> (zk/transcript/fiat_shamir.hpp:134-199).  THE CONTRACT (as for the
 * Merkle trees: crypto3-hash and crypto3-marshalling were not at hand, and the reference's own test only checks verify() after a
 * random start, so the bytes below are stated here and checked against an independent SHA2-256, not pinned to a crypto3 vector):
 *   transcript     its state is one 32-byte digest; absorbing bytes makes it SHA256(state || bytes); int_challenge<uint32_t>
 *                  makes it SHA256(state) and returns the low 32 bits of the state's BIG-ENDIAN integer (its bytes 28..31, big-endian);
 *   nonce bytes    a nonce n is absorbed as its four bytes, most significant first (proof_of_work.hpp:54-57);
 *   candidate      candidate(state, n) = the low 32 bits of the big-endian integer of SHA256(SHA256(state || be32(n)));
 *   acceptance     n is accepted when (candidate(state, n) & mask) == 0;
 *   search order   start, start + 1, start + 2, ... (mod 2^32): the reference's loop from its (there random) first value.
 * zkhip_pow_grind returns the FIRST accepted nonce in that order: the smallest offset k < max_tries with start + k accepted --
 * exactly what the reference's loop returns for the same start, whichever lane of the device finds a hit first.
 *   max_tries      offsets to try, at most 2^32 (0: the whole 2^32 space);
 *   chunk_log      the search runs in launches of 2^chunk_log consecutive offsets, the host looking for a hit between them
 *                  (8..32; 0: the library's default) -- the result does not depend on it;
 *   *nonce         the accepted nonce;  *tried (nullable): k + 1 on success, max_tries (2^32 for 0) when nothing was found.
 * Returns ZKHIP_ERR_NOT_FOUND when no offset below max_tries is accepted.  Errors, before anything is launched: a null ctx /
 * state / nonce or a hash other than ZKHIP_HASH_SHA2_256 -> ZKHIP_ERR_INVALID; chunk_log outside [8, 32] (0 aside) or
 * max_tries > 2^32 -> ZKHIP_ERR_RANGE. */
int zkhip_pow_grind(zkhip_ctx *ctx, int hash, const uint8_t state[32], uint32_t start, uint32_t mask, uint64_t max_tries, size_t chunk_log,
                    uint32_t *nonce, uint64_t *tried);
/* SHA2-256 of `len` bytes on the HOST, over the same core as the device's (needs no context and no GPU): what the shim's
 * transcript (hip/transcript.hpp) hashes with.  ZKHIP_ERR_INVALID for a null `out`, or a null `msg` with len > 0. */
int zkhip_sha256_host(const uint8_t *msg, size_t len, uint8_t out[32]);

/* ---- DFT over group elements -------------------------------------------------------------------------------
 * evaluation_domain<Fr, G>::evaluate_all_lagrange_polynomials(powers_begin, powers_end) as the powers-of-tau result uses
 * it (commitments/detail/polynomial/powers_of_tau/result.hpp:81-94): with P_i = tau^i G the INVERSE transform gives
 * L_j(tau) G for every Lagrange polynomial of the 2^log_m-point domain.  d_jacobian: 2^log_m canonical Jacobian points
 * (3 coordinates each, Z = 0 for infinity -- the form zkhip_msm_dev writes), transformed in place:
 * out[j] = sum_i omega^(i j) P_i, or with inverse != 0: (1/m) sum_i omega^(-i j) P_i. */
int zkhip_ec_ntt_dev(zkhip_ctx *ctx, int curve, int group, void *d_jacobian, size_t log_m, const uint64_t *omega, int inverse);

/* ---- coefficient-form polynomial arithmetic (KZG opening proofs, polynomial_dfs pointwise operators) -------
 * All vectors are canonical Fr elements (4 limbs) resident on the device.
 *
 * polynomial_dfs::operator+= / -= / *= on equal domains (ph/gates_argument.hpp:119-121,
 * ph/permutation_argument.hpp:148-167): d_out[i] = d_a[i] op d_b[i], op 0 add, 1 sub, 2 mul; in place allowed. */
int zkhip_fr_vec_op_dev(zkhip_ctx *ctx, int curve, int op, const void *d_a, const void *d_b, void *d_out, size_t count);
/* d_out[i] = a d_x[i] + b d_y[i] + c (d_y and b nullable together; a, b, c canonical Fr on the host; in place allowed): the linear
 * factors the arguments multiply up -- (1 + beta)(gamma + input), (1 + beta) gamma + value + beta value(omega X)
 * (ph/lookup_argument.hpp:313, 329, 361), mask = 1 - q_last - q_blind (:161-162) -- in one pass each. */
int zkhip_fr_vec_affine_dev(zkhip_ctx *ctx, int curve, const void *d_x, const void *d_y, const uint64_t *a, const uint64_t *b, const uint64_t *c, void *d_out,
                            size_t count);
/* d_out[j] = d_a[j] d_b[j] / d_c[j] for j < count (in place allowed; entries from `count` on are not touched): the intermediate
 * polynomials of the multi-part permutation / lookup arguments, current[j] = previous[j] g[j] / h[j] over the usable rows
 * (ph/permutation_argument.hpp:196-198, lookup_argument.hpp:264-266) -- rows in chunks of 8 that share one inversion; a zero
 * denominator zeroes its chunk. */
int zkhip_fr_vec_mul_div_dev(zkhip_ctx *ctx, int curve, const void *d_a, const void *d_b, const void *d_c, void *d_out, size_t count);
/* polynomial::evaluate for `batch` polynomials (n coefficients each, `stride` elements apart) at `npoints` points
 * given on the host (eval_polys, batched_commitment.hpp:168-183): out[b * npoints + p] = poly_b(points[p]), host. */
int zkhip_poly_eval_dev(zkhip_ctx *ctx, int curve, const void *d_polys, size_t n, size_t stride, size_t batch, const uint64_t *points,
                        size_t npoints, uint64_t *out);
/* Division by (X - z), the step `f /= V`, `L /= theta_2_vanish` of kzg_v2.hpp:267, 289 performs once per root:
 * d_out[0] = f(z) (the remainder), d_out[1 .. n) = the quotient's n - 1 coefficients.  d_out may equal d_f.
 * `remainder` (nullable, host) receives f(z); passing it synchronises the stream. */
int zkhip_poly_div_linear_dev(zkhip_ctx *ctx, int curve, const void *d_f, size_t n, const uint64_t *z, void *d_out, uint64_t *remainder);
/* Exact division by the vanishing polynomial X^n - 1 of the basic n-point domain, in coefficient form: placeholder's
 * `T_consolidated = F_consolidated_normal / common_data.Z` (ph/prover.hpp:273-275).  d_f: len coefficients; d_quot receives the
 * len - n coefficients of the quotient (nothing when len <= n); d_quot must not overlap d_f.  nonzero_remainders (nullable, host;
 * passing it synchronises the stream) receives the number of non-zero coefficients of the remainder -- 0 for the exact division
 * a satisfied circuit gives. */
int zkhip_poly_div_vanishing_dev(zkhip_ctx *ctx, int curve, const void *d_f, size_t len, size_t n, void *d_quot, uint64_t *nonzero_remainders);
/* The grand product of placeholder's permutation argument (ph/permutation_argument.hpp:103-136): over n rows and k permuted columns
 *   g_i = column_i + beta S_id_i + gamma,  h_i = column_i + beta S_sigma_i + gamma   (pointwise),
 *   V_P[0] = 1,  V_P[j] = V_P[j - 1] prod_i g_i[j - 1] / prod_i h_i[j - 1].
 * d_cols / d_sid / d_ssigma: HOST arrays of k device pointers to n canonical Fr each; d_g / d_h (nullable): k x n outputs, vector i at
 * element offset i n (the g_v / h_v the argument multiplies up afterwards); d_vp: n outputs.  The reference pays one inversion per row
 * in a serial loop; here rows are taken in chunks that share an inversion and the prefix product is a three-level scan. */
int zkhip_perm_grand_product_dev(zkhip_ctx *ctx, int curve, size_t k, const void *const *d_cols, const void *const *d_sid, const void *const *d_ssigma,
                                 size_t n, const uint64_t *beta, const uint64_t *gamma, void *d_g, void *d_h, void *d_vp);
/* The g and h polynomials of the same argument (ph/permutation_argument.hpp:140-160: polynomial_product(g_v), polynomial_product(h_v)) from vectors on
 * ANY domain: d_g[j] = prod_i (column_i[j] + beta S_id_i[j] + gamma), d_h[j] likewise over S_sigma, j < n.  With the columns and the (cached)
 * permutation polynomials extended to the products' domain this is ONE pass instead of 2 k extensions, 2 k linear passes and two k-way products. */
int zkhip_perm_factor_products_dev(zkhip_ctx *ctx, int curve, size_t k, const void *const *d_cols, const void *const *d_sid, const void *const *d_ssigma, size_t n,
                                   const uint64_t *beta, const uint64_t *gamma, void *d_g, void *d_h);
/* V_L of placeholder's lookup argument (ph/lookup_argument.hpp:375-409, `compute_V_L`), the same scan over other rows:
 *   V_L[0] = 1,  V_L[k] = V_L[k - 1] g(k - 1) / h(k - 1) for 1 <= k <= usable_rows,  V_L[k] = 0 behind,
 *   g(j) = (1 + beta)^k_in prod_i (gamma + input_i[j]) prod_i ((1 + beta) gamma + value_i[j] + beta value_i[j + 1]),
 *   h(j) = prod_i ((1 + beta) gamma + sorted_i[j] + beta sorted_i[j + 1]).
 * d_input / d_value / d_sorted: HOST arrays of device pointers to n canonical Fr each (the REDUCED vectors: on the basic domain);
 * usable_rows < n (ZKHIP_ERR_RANGE otherwise); d_vl: n outputs. */
int zkhip_lookup_grand_product_dev(zkhip_ctx *ctx, int curve, size_t k_in, const void *const *d_input, size_t k_val, const void *const *d_value, size_t k_sorted,
                                   const void *const *d_sorted, size_t n, size_t usable_rows, const uint64_t *beta, const uint64_t *gamma, void *d_vl);
/* sort_polynomials of placeholder's lookup argument (ph/lookup_argument.hpp:565-638; called at :188 between the reduction of the
 * lookup inputs / values to the basic domain and `commit(LOOKUP_BATCH)`).  Over the first usable_rows entries of every vector: the
 * values of the table columns in their order (columns one after the other), every maximal run of one value replaced by as many copies
 * as the value occurs among ALL table entries and inputs -- a run of zeros by a single zero, a trailing run of zeros by nothing, and one
 * zero in front when the first value is non-zero (the reference's walk starts from a virtual zero) --, dealt over the k_in + k_val
 * output vectors, usable_rows entries each; entry usable_rows of every vector but the last repeats the head of the next; all other
 * entries are zero.  d_input / d_value / d_sorted: HOST arrays of device pointers to n canonical Fr each (the REDUCED vectors);
 * usable_rows < n.  Equality is equality of the canonical limbs.  The reference counts with an unordered_map and emits in one serial
 * walk; here: run detection + u32 scans, an open-addressing hash table over the run heads, one atomic per input, a binary search per
 * output entry.  A looked-up value that is in no table (the reference's BOOST_ASSERT, :583) raises bit 2 of the sticky status word and
 * is otherwise ignored; more emitted entries than the vectors hold (a table whose equal values are not adjacent, :559-564) raise bit 3
 * and the excess is dropped. */
int zkhip_lookup_sort_dev(zkhip_ctx *ctx, size_t k_in, const void *const *d_input, size_t k_val, const void *const *d_value, size_t n, size_t usable_rows,
                          void *const *d_sorted);
/* d_acc[j] (+)= sum_i sum_{t < taps} coeffs[i * taps + t] * poly_i[j - t] for j < acc_len (poly_i is zero outside
 * [0, lens[i])): the accumulation `f += theta_i * (f_i - U) * diffpoly` (kzg_v2.hpp:258-263) for every committed
 * polynomial in ONE pass (coeffs[i] = theta_i * diffpoly_i, a few taps), and `L += ...` (:281-288) with taps = 1.
 * d_polys / lens / coeffs are host arrays (device pointers, element counts, canonical Fr); accumulate = 0
 * overwrites d_acc. */
int zkhip_poly_lincomb_dev(zkhip_ctx *ctx, int curve, size_t count, const void *const *d_polys, const size_t *lens, const uint64_t *coeffs,
                           size_t taps, void *d_acc, size_t acc_len, int accumulate);

/* ---- inner-product argument: what kimchi_pedersen needs beyond the MSM (zk/commitments/polynomial/kimchi_pedersen.hpp) ----------
 * The Pedersen / inner-product-argument commitment of the pairing-less curves rests on multiexp more than any other scheme: one MSM per
 * chunk to commit (:334-383), 2 log n half-size MSMs, 2 log n inner products and 3 log n vector folds to open (:385-559), one MSM over the
 * whole SRS to verify (:645-755).  The MSMs run over sub-ranges of resident bases (zkhip_msm_dev / zkhip_msm_batch_dev), the folds of the
 * scalar vectors are zkhip_fr_vec_affine_dev, `a` is accumulated by zkhip_poly_lincomb_dev, L and R are completed by a two-point MSM and
 * zkhip_jacobian_sum_dev; the four entry points below are the rest.  Conventions: G1 of every curve id; scalars are canonical Fr
 * elements (4 limbs), vectors of them resident on the device; everything is asynchronous on the context's stream except
 * zkhip_bases_fold, which like every constructor of bases returns with the stream drained.  ZKHIP_ERR_INVALID: a null pointer, an
 * unknown curve id, bases of ZKHIP_G2, a scalar that is not below r; ZKHIP_ERR_RANGE: a range beyond an object's size, a size
 * beyond the stated limit.
 *
 * The generator fold g = g_high * u + g_low (`compress_function_u`, :524-534): a NEW bases object of `half` points,
 *     out[i] = c * b[offset_hi + i] + b[offset_lo + i],   i < half < 2^31,
 * one variable-base scalar multiplication and one mixed addition per point (points at infinity, c = 0, c * hi = +-lo included).  The two
 * ranges may overlap or coincide; b is left as it is (only its points are read: whatever window tables it has play no part).  `out`
 * holds the points alone, affine, and carries NO window tables whatever its size -- it feeds two MSMs and the next fold, and tables
 * would cost more than they save; an MSM over it combines the windows by the Horner pass.  Free it with zkhip_bases_free. */
int zkhip_bases_fold(zkhip_ctx *ctx, const zkhip_bases *b, size_t offset_lo, size_t offset_hi, size_t half, const uint64_t *c /* 4 limbs */,
                     zkhip_bases **out);
/* ---- a different scalar per resident point: the powers-of-tau contribution and the Groth16 MPC phase 2 ----
 * powers_of_tau_accumulator::transform (commitments/detail/polynomial/powers_of_tau/accumulator.hpp:89-121: naive_batch_exp /
 * naive_batch_exp_with_coeff over tau_powers_g1, tau_powers_g2, alpha_tau_powers_g1, beta_tau_powers_g1 with the exponents tau^i,
 * alpha tau^i, beta tau^i) and the delta^-1 scaling of H_query / L_query in r1cs_gg_ppzksnark's mpc contribution
 * (crs_operations.hpp:116-123) are one operation: a NEW bases object of n points,
 *     out[i] = s_i * b[offset + i],   0 < n < 2^31,
 * one variable-base scalar multiplication per point (a fixed 4-bit signed-window ladder over a per-point table; on G1 the scalar is
 * split by the curve's endomorphism, GLV).  G1 of every curve id, G2 of ZKHIP_BLS12_381 and ZKHIP_BN254 (a bases object of ZKHIP_G2 with
 * a Pasta id cannot be built: ZKHIP_ERR_INVALID).  b is left as it is and only its points are read, whatever window tables it carries.  A
 * point at infinity or a scalar of zero gives the point at infinity.  `out` holds affine points in the internal form and, as for
 * zkhip_bases_fold, carries NO window tables -- a ceremony's output is downloaded or scaled again, and tables would cost more than they
 * save -- unless ZKHIP_SCALE_TABLES is set in `flags`: then it carries them exactly as a zkhip_bases_upload of the same points would
 * under the context's current "msm_precompute" / "msm_window_bits" options.  Like every constructor of bases both calls return with the
 * stream drained; free with zkhip_bases_free.  "ec_ntt_table_lanes" applies as for zkhip_ec_ntt_dev: a range of more points than one
 * launch holds tables for runs as several launches, with the same result.
 *   zkhip_bases_scale_dev        s_i = the i-th of n scalars resident on the device (4 limbs each, 16-byte aligned).  A scalar that is not
 *                                below r is taken mod r, exactly as zkhip_msm_dev takes it (the reference's field type cannot hold one).
 *   zkhip_bases_scale_geometric  s_i = coeff * ratio^(first_exponent + i), ratio and coeff on the host (4 limbs, canonical; coeff NULL: 1),
 *                                first_exponent + n <= 2^32.  ratio^0 = 1 also for ratio = 0, as the reference's running product has it.
 *                                ratio = 1 is the one-scalar case (every point times coeff: delta^-1).
 * Errors, before anything is launched, with *out = null: a null ctx / b / out / d_scalars / ratio, an unknown curve or an unknown bit of
 * `flags` -> ZKHIP_ERR_INVALID; ratio or coeff not below r -> ZKHIP_ERR_INVALID; n = 0, n >= 2^31, offset + n > zkhip_bases_size(b) or
 * first_exponent + n > 2^32 -> ZKHIP_ERR_RANGE. */
enum zkhip_scale_flags { ZKHIP_SCALE_TABLES = 1 };
int zkhip_bases_scale_dev(zkhip_ctx *ctx, const zkhip_bases *b, size_t offset, size_t n, const void *d_scalars /* device, n x 4 canonical */, int flags,
                          zkhip_bases **out);
int zkhip_bases_scale_geometric(zkhip_ctx *ctx, const zkhip_bases *b, size_t offset, size_t n, const uint64_t *ratio /* 4 limbs */,
                                const uint64_t *coeff /* nullable = 1 */, uint64_t first_exponent, int flags, zkhip_bases **out);
/* kimchi_pedersen::params_type::add_lagrange_basis (kimchi_pedersen.hpp:92-105): a NEW bases object of m = 2^log_m points,
 *     out[j] = (1/m) sum_{i<m} omega^(-i j) b[offset + i]
 * omega = the primitive m-th root of unity of the curve's scalar field (canonical, 4 limbs): the inverse DFT over group elements of a
 * range of the SRS, so that the MSM of a column's EVALUATIONS over `out` is the commitment of the column (no inverse NTT).  G1 of every
 * curve id (0-3; the twiddles are split by the curve's endomorphism, GLV, on all four); bases of ZKHIP_G2 are ZKHIP_ERR_INVALID as for
 * zkhip_bases_fold.  b is left as it is and only its points are read, whatever window tables it carries; points at infinity among the
 * inputs are ordinary.  `out` holds affine points in the internal form and, unlike the output of zkhip_bases_fold, carries window tables
 * exactly as a zkhip_bases_upload of the same points would under the context's current "msm_precompute" / "msm_window_bits" options: it
 * is built once and multiplied against many times.  Like every constructor of bases it returns with the stream drained; free with
 * zkhip_bases_free.  log_m = 0: out[0] = b[offset].  "ec_ntt_table_lanes" applies as for zkhip_ec_ntt_dev.
 * Errors, before anything is launched, with *out = null: a null ctx / b / omega / out or an unknown curve -> ZKHIP_ERR_INVALID; omega not
 * below r, or not of order exactly 2^log_m (omega^m = 1, and omega^(m/2) = -1 for m > 1) -> ZKHIP_ERR_INVALID; log_m > 26 or
 * offset + m > zkhip_bases_size(b) -> ZKHIP_ERR_RANGE. */
int zkhip_bases_lagrange(zkhip_ctx *ctx, const zkhip_bases *b, size_t offset, size_t log_m, const uint64_t *omega /* 4 limbs */, zkhip_bases **out);
/* d_out[0] = sum_{i < n} d_a[i] d_b[i] (algebra::inner_product, :472-475, :500-506), one canonical Fr element on the device; n < 2^39,
 * n = 0 gives zero.  The additions form a fixed tree (per wave, per workgroup, one last workgroup; no atomics). */
int zkhip_fr_inner_product_dev(zkhip_ctx *ctx, int curve, const void *d_a, const void *d_b, size_t n, void *d_out);
/* d_out[i] = sum_{e < npoints} scales[e] * points[e]^i for i < n: the vector b of proof_eval (:460-470: scales[e] = evalscale^e).
 * points / scales: host, canonical Fr; npoints < 65536 (0: the zero vector), n < 2^39. */
int zkhip_fr_powers_lincomb_dev(zkhip_ctx *ctx, int curve, const uint64_t *points, const uint64_t *scales, size_t npoints, void *d_out, size_t n);
/* d_out[i] = prod over the set bits t of i of chals[rounds - 1 - t], i < 2^rounds: b_poly_coefficents (:629-643), the vector s of
 * verify_eval.  chals: host, canonical Fr (nullable when rounds = 0: d_out[0] = 1); rounds <= 31. */
int zkhip_fr_challenge_products_dev(zkhip_ctx *ctx, int curve, const uint64_t *chals, size_t rounds, void *d_out);

/* ---- pairing products: the commitments and GIPA rounds of Groth16 aggregation (SnarkPack / TIPP-MIPP) --------------------------
 * kzg_ipp2::pair and ::single (zk/commitments/polynomial/kzg_ipp2.hpp:216-283) and the z / t / u values of every GIPA round
 * (systems/ppzksnark/r1cs_gg_ppzksnark/ipp2/prover.hpp:360-381, 584-593) are inner pairing products over vectors the device already
 * holds as bases objects:
 *     out_gt[k] = final_exponentiation( prod over the terms t with t.out == k of prod_{i < t.n} miller(g1[t.g1_offset + i], g2[t.g2_offset + i]) ),
 * k < n_out.  `pair` is one call with four terms and two outputs, `single` one with two terms and two outputs, ip_ab one term.
 * Conventions:
 *   - ZKHIP_BLS12_381 ONLY.  ZKHIP_BN254 and the Pasta ids are ZKHIP_ERR_INVALID: BN254's optimal ate pairing needs a different Miller
 *     loop (the parameter 6x + 2 and two Frobenius-twisted additions at its end), and the reference holds no vector to pin one to; the
 *     Pasta curves have no pairing.
 *   - The pairing is the ate pairing over |x| = 0xd201000000010000 (conjugated: x is negative) and final_exponentiation raises to
 *     3 (p^12 - 1) / r: the x-chain formulas compute the hard part to that fixed multiple, and it is the power the reference's vectors
 *     (r1cs_gg_ppzksnark_aggregation_conformity.cpp, bls381_commitment_test) hold.  Bilinearity and non-degeneracy are unaffected.
 *   - out_gt: HOST, n_out x 72 u64: an Fq12 value as 12 canonical Fq values of 6 limbs in the order of the reference's constructor
 *     fq12(fq6(fq2, fq2, fq2), fq6(fq2, fq2, fq2)), c0 before c1 at every level.
 *   - A pair whose G1 or G2 point is the point at infinity contributes one; an output that no term names, or whose pairs are all such,
 *     is one.  Points are taken as members of the order-r subgroups, as every constructor of bases delivers them.
 *   - Only the points of the bases objects are read; their window tables play no part.  A term may start anywhere inside its objects,
 *     several terms may feed one output, and terms may share objects.
 *   - Terms are meant to be few and long (a commitment has two or four, a GIPA round a handful): every workgroup finds its term by a
 *     linear walk of the term table, so a call with many small terms pays O(n_terms) per 64 pairs.
 *   - The Miller loops and the products run on the device in a fixed order without atomics; the final exponentiation of the n_out
 *     results runs on the host (~10^4 dependent Fq products each).  The call returns with the stream drained.
 * Errors, before anything is launched: a null ctx / out_gt / terms (with n_terms > 0) / g1 / g2, an unknown or unsupported curve, bases
 * of the wrong group or another curve -> ZKHIP_ERR_INVALID; g1_offset + n or g2_offset + n beyond the object's size, out >= n_out,
 * n_out = 0, or 2^37 pairs or more in all -> ZKHIP_ERR_RANGE. */
typedef struct zkhip_pairing_term {
    const zkhip_bases *g1; size_t g1_offset;   /* ZKHIP_G1 bases */
    const zkhip_bases *g2; size_t g2_offset;   /* ZKHIP_G2 bases */
    size_t n;                                  /* pairs of this term */
    uint32_t out;                              /* which output the term is multiplied into */
} zkhip_pairing_term;
int zkhip_pairing_products(zkhip_ctx *ctx, int curve, const zkhip_pairing_term *terms, size_t n_terms, size_t n_out, uint64_t *out_gt);

/* ---- Groth16 verification: batches of proofs against one key, up to and including the final exponentiation --------------------
 * Per proof, r1cs_gg_ppzksnark_verifier_weak_input_consistency::process of the reference
 * (systems/ppzksnark/r1cs_gg_ppzksnark/verifier.hpp:150-186):
 *     acc = abc[0] + sum_{j < n_inputs} x_j abc[j + 1]
 *     ok  = well_formed && final_exponentiation(miller(A, B) miller(-acc, gamma) miller(-C, delta)) == alpha_beta
 * The reference divides by double_miller_loop(acc, gamma, C, delta) before its final exponentiation; negating the G1 points instead
 * differs from that by factors of proper subfields only, which the final exponentiation removes, and an element of GT has one
 * canonical form: the compared value is the reference's bit for bit.
 * Conventions:
 *   - ZKHIP_BLS12_381 ONLY; ZKHIP_BN254 and the Pasta ids are ZKHIP_ERR_INVALID, for the reasons zkhip_pairing_products gives.  The
 *     pairing, the power 3 (p^12 - 1) / r and the layout of a GT value (72 u64) are zkhip_pairing_products'.
 *   - A key is uploaded once (zkhip_groth16_vk_upload) and holds, on the device: alpha_beta, the 68 prepared line triples of gamma and
 *     of delta each (19584 bytes per point), abc[0], and per input a fixed-base table of 4-bit windows: 64 windows x 15 affine points =
 *     92160 bytes per input.  A proof's accumulation is at most 64 mixed additions per input (one per non-zero nibble of x_j) and no
 *     doubling.  A key takes at most ZKHIP_GROTH16_VK_MAX_INPUTS = 2^15 inputs (2.8 GiB of tables); the tables are computed on one
 *     host thread at upload, about a millisecond per input.
 *   - alpha_beta: 72 u64, canonical, the order zkhip_pairing_products writes.  gamma_g2 / delta_g2: affine, 24 u64 each, not at
 *     infinity.  gamma_abc_xy: n_abc >= 1 affine G1 points of 12 u64: gamma_ABC_g1.first, then .rest; gamma_abc_inf nullable.
 *   - Proofs offset .. offset + n of three resident bases objects (a: ZKHIP_G1, b: ZKHIP_G2, c: ZKHIP_G1), so proofs can come from host
 *     points, from scalars, or from the wire decoder.  Only the points are read; window tables play no part.
 *   - inputs: HOST, n x n_inputs x 4 u64, canonical; n_inputs <= zkhip_groth16_vk_inputs(vk): missing inputs are zero (weak input
 *     consistency).  ok: HOST, n bytes, 1 = accepted.  out_gt: nullable, HOST, n x 72 u64: the value that was compared with alpha_beta.
 *   - well_formed is the reference's proof.is_well_formed(): A, B and C lie on their curves (or are at infinity).  The call checks it
 *     itself, whatever constructor made the bases.  A pair with a point at infinity contributes one; acc may be at infinity.
 *   - Membership of the order-r subgroups is not checked, as in the reference: for an on-curve point outside its subgroup ok (and
 *     out_gt) are unspecified.  No input makes the call fault: the Miller formulas have no divisions.
 *   - A rejected proof is not an error: the call returns ZKHIP_OK.  Three launches whatever n is; nothing proportional to n runs on
 *     the host but the copies of inputs, ok and out_gt.  The call returns with the stream drained.
 * Errors, before anything is launched:
 *   ZKHIP_ERR_INVALID   a null ctx / vk / a / b / c / ok; inputs null with n_inputs > 0; a bases object of the wrong group or of another
 *                       curve; a vk of another context's device.  Upload: a null ctx / alpha_beta / gamma_g2 / delta_g2 / out, a null
 *                       gamma_abc_xy with n_abc > 0, a curve other than ZKHIP_BLS12_381.
 *   ZKHIP_ERR_RANGE     offset + n beyond any of the three objects; n_inputs above the key's.  Upload: n_abc = 0 or more than
 *                       ZKHIP_GROTH16_VK_MAX_INPUTS inputs.
 *   ZKHIP_ERR_OOM       Upload: no host or device memory for the tables.
 *   n = 0 is ZKHIP_OK with nothing launched. */
#define ZKHIP_GROTH16_VK_MAX_INPUTS 32768
typedef struct zkhip_groth16_vk zkhip_groth16_vk;
int zkhip_groth16_vk_upload(zkhip_ctx *ctx, int curve, const uint64_t *alpha_beta, const uint64_t *gamma_g2, const uint64_t *delta_g2,
                            const uint64_t *gamma_abc_xy, const uint8_t *gamma_abc_inf /* nullable */, size_t n_abc, zkhip_groth16_vk **out);
size_t zkhip_groth16_vk_inputs(const zkhip_groth16_vk *vk);  /* n_abc - 1 */
void zkhip_groth16_vk_free(zkhip_ctx *ctx, zkhip_groth16_vk *vk);
int zkhip_groth16_verify_batch(zkhip_ctx *ctx, const zkhip_groth16_vk *vk, const zkhip_bases *a, const zkhip_bases *b, const zkhip_bases *c,
                               size_t offset, size_t n, const uint64_t *inputs, size_t n_inputs, uint8_t *ok, uint64_t *out_gt /* nullable */);

/* ---- the gate argument's sum over a flat program -------------------------------------------------------------------------
 * placeholder's gates argument (ph/gates_argument.hpp:93-121, 203-216) computes, on the extended domain of 2^log_size points,
 *     F = mask * sum_gates selector_g * sum_constraints theta^k * constraint(columns, rotated).
 * Which monomials a constraint is made of is decided by the reference's symbolic machinery (math::expression and its visitors: the
 * caller's, SURVEY section 2 out of scope); once flattened it is a PROGRAM over column slots, evaluated here in ONE launch, a lane per row:
 *   d_out[j] = [d_mask[j] *] ( [d_out[j] +] sum_g [slot_{sel_g}[j + rs_g] *] sum_{t in gate g} coeff_t prod_{f in term t} slot_{s_f}[(j + r_f) mod 2^log_size] )
 * -- rotations are index arithmetic on the extended domain (a rotation by k rows of the ORIGINAL n-row domain is k * 2^log_size / n here;
 * no math::polynomial_shift copies), every distinct column is read where it lies, selector and mask are multiplied in the same pass.
 * The expressions of prepare_lookup_input (ph/lookup_argument.hpp:435-496) are the same program without selectors and mask.
 * All arrays of the program are HOST memory; d_slots is a host array of n_slots device pointers to 2^log_size canonical Fr each.
 * accumulate != 0 adds to what d_out holds (a program evaluated in pieces: the mask then belongs to the LAST piece).
 * A malformed program (ranges out of order, a slot that does not exist) is refused with ZKHIP_ERR_INVALID / ZKHIP_ERR_RANGE. */
#define ZKHIP_GATE_NO_SELECTOR 0xFFFFFFFFu
typedef struct zkhip_gate_program {
    uint32_t n_gates, n_terms, n_factors, n_slots;
    const uint32_t *gate_terms;        /* n_gates + 1: gate g owns terms [gate_terms[g], gate_terms[g + 1]) */
    const uint32_t *gate_selector;     /* n_gates: slot of the gate's selector, or ZKHIP_GATE_NO_SELECTOR */
    const int32_t *gate_selector_rot;  /* n_gates: its rotation, in rows of THIS domain */
    const uint32_t *term_factors;      /* n_terms + 1: term t owns factors [term_factors[t], term_factors[t + 1]) (none: the constant coeff_t) */
    const uint32_t *factor_slot;       /* n_factors */
    const int32_t *factor_rot;         /* n_factors: rows of THIS domain, may be negative */
    const uint64_t *term_coeff;        /* n_terms x 4 limbs, canonical */
} zkhip_gate_program;
int zkhip_gate_eval_dev(zkhip_ctx *ctx, int curve, const zkhip_gate_program *prog, const void *const *d_slots, size_t log_size, const void *d_mask /* nullable */,
                        int accumulate, void *d_out);

/* ---- device group: N GPUs behind ONE caller ---------------------------------------------------------------------
 * The reference hides all of its parallelism INSIDE the call: r1cs_gg_ppzksnark_prover::process splits every multiexp into
 * `chunks = omp_get_max_threads()` pieces (r1cs_gg_ppzksnark/prover.hpp:94-99, 108-139) and kzg_commitment_scheme_v2::commit loops
 * over the batch (commitments/polynomial/kzg_v2.hpp:208-226) -- the caller sees one call and one result.  A group is the same for
 * GPUs: one zkhip_ctx per entry of device_ids (SURVEY 8b sketched this as `zkhip_init(const int *device_ids, int n_dev, ...)`),
 * every entry point asynchronous on its member's stream, with the one exchange the path has -- the partial sums of a sharded
 * multiexp, <= 864 bytes per member for a Groth16 proof -- INSIDE the library.  The shim's group paths (device_group::for_each_member)
 * drive member 0 from the caller's thread and members 1..N-1 from host threads of their own: a caller's thread-local state does not
 * reach them.
 * device_ids may name a device more than once (several members on one GPU: a 1-GPU box, tests).
 * Members are ordinary contexts (zkhip_group_ctx): every other entry point of this header works on them; they are destroyed with
 * the group.  A group is not thread-safe. */
typedef struct zkhip_device_group zkhip_device_group;
int zkhip_group_init(const int *device_ids, int n_dev, zkhip_device_group **out);
void zkhip_group_destroy(zkhip_device_group *g);
int zkhip_group_size(const zkhip_device_group *g);
zkhip_ctx *zkhip_group_ctx(const zkhip_device_group *g, int member);
const char *zkhip_group_last_error(const zkhip_device_group *g);
/* How the exchanges travel.
 *   ZKHIP_GROUP_RCCL    one single-process RCCL communicator per member (ncclCommInitAll) and a grouped ncclAllGather on the members'
 *                       streams over xGMI; librccl.so is loaded on first use (dlopen), so a single-GPU caller never pays for it.
 *                       Needs pairwise distinct devices (RCCL refuses two ranks on one GPU): ZKHIP_ERR_INVALID otherwise.
 *   ZKHIP_GROUP_PEER    stream-ordered peer copies (hipMemcpyPeerAsync behind an event per source stream -- the same call between members
 *                       that share a GPU, so a one-GPU box exercises what a multi-GPU box runs).  No host synchronisation.
 *   ZKHIP_GROUP_STAGED  through one page-locked host buffer: D2H on every member, a host synchronisation, H2D -- also between members
 *                       that share a GPU (one code path on every box).  The fallback that works wherever HIP works.
 *   ZKHIP_GROUP_AUTO    (default) RCCL when the group has more than one member on pairwise distinct devices and librccl loads,
 *                       PEER otherwise.
 * zkhip_group_transport returns what AUTO resolved to (RCCL is tried at the first exchange). */
enum zkhip_group_transport_kind { ZKHIP_GROUP_AUTO = 0, ZKHIP_GROUP_RCCL = 1, ZKHIP_GROUP_PEER = 2, ZKHIP_GROUP_STAGED = 3 };
int zkhip_group_set_transport(zkhip_device_group *g, int transport);
int zkhip_group_transport(const zkhip_device_group *g);
/* All-gather in stream order: the `bytes` bytes at d_send[k] (member k's device memory) arrive at d_recv[j] + k * bytes for every
 * member j whose d_recv[j] is not NULL (a NULL entry: that member receives nothing -- the one-host-thread caller usually needs the
 * result on member 0 only).  d_send / d_recv: HOST arrays of zkhip_group_size device pointers.  Ordered after everything enqueued
 * on the members' streams so far; with RCCL / PEER nothing blocks the host.  This is the exchange SURVEY 8e names (ncclAllGather
 * of 144- / 288-byte Jacobian partial sums + a local fold: RCCL has no elliptic-curve reduction). */
int zkhip_group_all_gather(zkhip_device_group *g, const void *const *d_send, void *const *d_recv, size_t bytes);
/* d_dst (member dst) <- d_src (member src), `bytes` bytes, ordered after src's stream so far, enqueued on dst's stream.  The source
 * must stay untouched until dst's stream has passed the copy (zkhip_sync on dst, or a later exchange). */
int zkhip_group_copy(zkhip_device_group *g, int dst_member, void *d_dst, int src_member, const void *d_src, size_t bytes);
int zkhip_group_sync(zkhip_device_group *g); /* every member's stream has drained */
/* Resident bases cut by POINT RANGE over the members: member k holds points [k n / N, (k + 1) n / N) (balanced; the
 * first n mod N members hold one more) with their own window tables.  Same arguments as zkhip_bases_upload. */
typedef struct zkhip_group_bases zkhip_group_bases;
int zkhip_group_bases_upload(zkhip_device_group *g, int curve, int group, const uint64_t *affine_xy, const uint8_t *is_infinity /* nullable */, size_t n,
                             zkhip_group_bases **out);
int zkhip_group_bases_from_scalars(zkhip_device_group *g, int curve, int group, const uint64_t *base_affine_xy /* nullable */, const uint64_t *scalars, size_t n,
                                   zkhip_group_bases **out);
void zkhip_group_bases_free(zkhip_device_group *g, zkhip_group_bases *b);
size_t zkhip_group_bases_size(const zkhip_group_bases *b);
/* member k's slice as an ordinary bases object (owned by the group object); *first receives the index of its first point */
const zkhip_bases *zkhip_group_bases_member(const zkhip_group_bases *b, int member, size_t *first /* nullable */);
/* zkhip_msm over the group: algebra::multiexp<BDLO12>(b0, b1, s0, s1, chunks) with the chunks on N GPUs (prover.hpp:94-99 chooses
 * chunks = omp_get_max_threads(); here a chunk is a member's point range).  Every member receives its slice of the scalars and
 * runs the whole pipeline over its points; the partial sums are all-gathered to member 0, folded there
 * (zkhip_jacobian_sum_dev) and returned.  Same result as zkhip_msm over one device (compare in affine). */
int zkhip_group_msm(zkhip_device_group *g, const zkhip_group_bases *bases, size_t offset, size_t n, const uint64_t *scalars /* host, n x 4 */,
                    uint64_t *out_jacobian /* host */);
/* zkhip_ntt with the batch dealt over the members in contiguous ranges ("partition by polynomial, no collective"):
 * member k transforms vectors [k batch / N, (k + 1) batch / N).  Bit-identical to zkhip_ntt. */
int zkhip_group_ntt(zkhip_device_group *g, int curve, uint64_t *data /* host, batch x m x 4 */, size_t log_m, size_t batch, const uint64_t *omega, int inverse,
                    const uint64_t *coset_gen /* nullable */);

/* ---- profiling (HIP events on the context's stream around every kernel launch) ------------------ */
int zkhip_profile_enable(zkhip_ctx *ctx, int on);
int zkhip_profile_reset(zkhip_ctx *ctx);
/* Only kernels whose name starts with `prefix` are timed from now on (NULL / "": all): keeps a timed region's event traffic to
 * the one kernel whose duration is wanted. */
int zkhip_profile_filter(zkhip_ctx *ctx, const char *prefix);
/* Total milliseconds and launch count recorded for kernels whose name starts with `prefix`. */
int zkhip_profile_get(zkhip_ctx *ctx, const char *prefix, double *total_ms, uint64_t *launches);
/* Writes "name total_ms launches\n" lines; returns bytes needed. */
size_t zkhip_profile_dump(zkhip_ctx *ctx, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* ZKHIP_H */
