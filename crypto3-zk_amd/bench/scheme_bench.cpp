// Commitment-scheme throughput drivers for bench.py / tools: BASELINE config 5's commitment leg and the LPC commit THROUGH THE
// SHIM CLASSES, with the columns starting in host memory as placeholder hands them over (upload included).
// Host compiler only; part of libzkhip_bench.so.
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <array>
#include <map>
#include <memory>
#include <thread>
#include <vector>

#include <nil/crypto3/zk/hip/kzg_v2.hpp>
#include <nil/crypto3/zk/hip/lpc.hpp>
#include <nil/crypto3/zk/hip/merkle.hpp>
#include <nil/crypto3/zk/hip/placeholder_lookup.hpp>
#include <nil/crypto3/zk/hip/placeholder_permutation.hpp>
#include <nil/crypto3/zk/hip/placeholder_quotient.hpp>
#include <nil/crypto3/zk/hip/transcript.hpp>

using namespace nil::crypto3::zk::hip;

namespace {
typedef bls12_381 C;
typedef curve_adapter<C> A;
typedef A::scalar_value_type Fr;

struct counting_transcript {
    std::vector<Fr> challenges;
    std::size_t next = 0;
    template <typename T>
    void operator()(const T &) { }
    Fr challenge() { return challenges.at(next++ % challenges.size()); }
};

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

/// 7^((r - 1) / 2^l) by square-and-multiply on the host: the primitive 2^l-th root of BLS12-381 Fr the tests use
Fr bls_root(std::size_t l) {
    const uint64_t rm1[4] = {0xffffffff00000000ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
    uint64_t e[4] = {rm1[0], rm1[1], rm1[2], rm1[3]};
    for (std::size_t k = 0; k < l; ++k) {
        for (int i = 0; i < 3; ++i) e[i] = (e[i] >> 1) | (e[i + 1] << 63);
        e[3] >>= 1;
    }
    Fr r = Fr::one(), b(7);
    for (int i = 255; i >= 0; --i) {
        r = r * r;
        if ((e[i >> 6] >> (i & 63)) & 1) r = r * b;
    }
    return r;
}

/// A stand-in for the caller's Merkle hash in the streaming shape (hip/lpc.hpp): every slice is folded (XOR of the low limbs) by
/// `threads` host threads while the next slice crosses PCIe -- the memory traffic of a hash without its arithmetic.
struct fold_tree {
    uint64_t r = 0;
    uint64_t root() const { return r; }
};
/// The fold is POSITION-WEIGHTED (round 6; it used to be an XOR, which any permutation of the leaves passes): with the leaves' limbs as one
/// sequence w_0, w_1, ... of u64 words, r = sum_k (k + 1) w_k mod 2^64 -- so bench.py can hold it against the same sum over the ORACLE's
/// leaf layout (the checker's restatement of basic_fri.hpp:456-492 over its own extension of the same polynomials) and a misplaced leaf shows.
struct streaming_fold_builder {
    unsigned threads = 8;
    fold_tree t;
    void begin(std::size_t, std::size_t) { t = fold_tree(); }
    void absorb(const Fr *leaves, std::size_t first, std::size_t count) {
        const unsigned threads = count >= ((std::size_t)1 << 16) ? this->threads : 1;    // the late FRI rounds are a few leaves: no thread is worth starting
        std::vector<uint64_t> part(threads, 0);
        std::vector<std::thread> th;
        for (unsigned k = 0; k < threads; ++k)
            th.emplace_back([&, k]() {
                uint64_t x = 0;
                for (std::size_t i = count * k / threads; i < count * (k + 1) / threads; ++i)
                    for (int j = 0; j < 4; ++j) x += (uint64_t)(4 * (first + i) + j + 1) * leaves[i].limbs[j];
                part[k] = x;
            });
        for (auto &w : th) w.join();
        for (uint64_t x : part) t.r += x;
    }
    fold_tree finish() { return t; }
};
struct vector_fold_builder {    // round 2's shape: the leaves materialised in a std::vector
    fold_tree operator()(const std::vector<Fr> &leaves, std::size_t) const {
        fold_tree t;
        for (std::size_t i = 0; i < leaves.size(); ++i)
            for (int j = 0; j < 4; ++j) t.r += (uint64_t)(4 * i + j + 1) * leaves[i].limbs[j];
        return t;
    }
};
}    // namespace

namespace {

struct splitmix {
    uint64_t seed;
    uint64_t operator()() {
        uint64_t z = (seed += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    Fr nonzero() {
        uint64_t w[4] = {(*this)() | 1, (*this)(), (*this)(), (*this)() & 0x0fffffffffffffffull};
        return A::scalar_from_limbs(w);
    }
};

/// a genuine lookup instance (see zkhip_bench_lookup): table columns, inputs drawn from them, `sorted` as sort_polynomials (:565-638) builds it
void build_lookup_instance(splitmix &sm, size_t n, size_t usable, size_t k_in, size_t k_val, std::vector<polynomial_dfs<C>> &value, std::vector<polynomial_dfs<C>> &input,
                           std::vector<polynomial_dfs<C>> &sorted) {
    const size_t total = k_in + k_val, T = usable / 2;
    value.assign(k_val, {});
    input.assign(k_in, {});
    sorted.assign(total, {});
    std::vector<Fr> pool(1, Fr::zero());
    for (auto &p : value) {
        p.values.assign(n, Fr::zero());
        for (size_t j = 1; j <= T; ++j) pool.push_back(p.values[j] = sm.nonzero());
    }
    std::vector<uint32_t> looked_up(pool.size(), 0);
    for (auto &p : input) {
        p.values.resize(n);
        for (size_t j = 0; j < n; ++j) {
            if (j < usable) {
                const size_t idx = sm() % pool.size();
                ++looked_up[idx];
                p.values[j] = pool[idx];
            } else {
                p.values[j] = sm.nonzero();
            }
        }
    }
    // sort_polynomials: a zero at every 0 -> non-zero step of the table walk, then every value as often as it occurs in table + inputs
    std::vector<Fr> flat;
    size_t idx = 1;
    for (size_t c = 0; c < k_val; ++c) {
        flat.push_back(Fr::zero());
        for (size_t j = 1; j <= T; ++j, ++idx) flat.insert(flat.end(), 1 + looked_up[idx], pool[idx]);
    }
    if (flat.size() > total * usable) throw std::runtime_error("lookup bench: instance does not fit");
    for (auto &p : sorted) p.values.assign(n, Fr::zero());
    for (size_t i = 0; i < flat.size(); ++i) sorted[i / usable].values[i % usable] = flat[i];
    for (size_t i = 0; i + 1 < total; ++i) sorted[i].values[usable] = sorted[i + 1].values[0];
}

/// a genuine copy-constraint instance in placeholder's shape: k columns constant along the cycles of a random permutation of the k * usable cells of
/// the usable rows, blinding rows (random values, identity permutation) behind; S_id[i][j] = delta^i omega^j
void build_permutation_instance(splitmix &sm, size_t log_n, size_t usable, size_t k, std::vector<polynomial_dfs<C>> &cols, std::vector<polynomial_dfs<C>> &sid,
                                std::vector<polynomial_dfs<C>> &ssig) {
    const size_t n = (size_t)1 << log_n, cells = k * usable;
    cols.assign(k, {});
    sid.assign(k, {});
    ssig.assign(k, {});
    const Fr w = bls_root(log_n), delta(7);
    Fr di = Fr::one();
    for (size_t i = 0; i < k; ++i, di = di * delta) {
        sid[i].values.resize(n);
        Fr x = di;
        for (size_t j = 0; j < n; ++j, x = x * w) sid[i].values[j] = x;
    }
    std::vector<uint32_t> perm(cells);
    for (size_t c = 0; c < cells; ++c) perm[c] = (uint32_t)c;
    for (size_t a = cells - 1; a > 0; --a) std::swap(perm[a], perm[sm() % (a + 1)]);
    std::vector<uint8_t> seen(cells, 0);
    for (size_t i = 0; i < k; ++i) {
        cols[i].values.resize(n);
        ssig[i].values.resize(n);
    }
    auto col_of = [usable](size_t c) { return c / usable; };
    auto row_of = [usable](size_t c) { return c % usable; };
    for (size_t c = 0; c < cells; ++c) {
        if (seen[c]) continue;
        const Fr v = sm.nonzero();
        for (size_t x = c; !seen[x]; x = perm[x]) {
            seen[x] = 1;
            cols[col_of(x)].values[row_of(x)] = v;
        }
    }
    for (size_t c = 0; c < cells; ++c) ssig[col_of(c)].values[row_of(c)] = sid[col_of(perm[c])].values[row_of(perm[c])];
    for (size_t i = 0; i < k; ++i)
        for (size_t j = usable; j < n; ++j) {
            cols[i].values[j] = sm.nonzero();
            ssig[i].values[j] = sid[i].values[j];
        }
}

}    // namespace

extern "C" {

/* 50 (cols) polynomial_dfs of 2^log_n rows in HOST memory (evals: cols x n x 4 canonical limbs, row-major per column) ->
 * kzg_commitment_scheme_v2_hip::append_to_batch + commit + proof_eval at two points, `steps` times on fresh scheme objects.
 * mode 0: append_to_batch(const &) (the reference's copy), 1: handed over (&&), 2: lent (std::cref).
 * ms: steps x {append, commit, proof_eval}.  out_commitments: cols x 12 u64 affine limbs of the last commit. */
int zkhip_bench_kzg_scheme(int device, size_t log_n, size_t cols, int steps, int mode, size_t upload_chunk, const uint64_t *evals, double *ms,
                           uint64_t *out_commitments) {
    try {
        const size_t n = (size_t)1 << log_n;
        context ctx(device);
        std::vector<Fr> pw(n);
        Fr x = Fr::one(), alpha(7);
        for (size_t i = 0; i < n; ++i) pw[i] = x, x = x * alpha;
        kzg_params_hip<C> params(ctx, device_bases<C, ZKHIP_G1>::from_scalars(ctx, pw.begin(), pw.end()));
        std::vector<Fr>().swap(pw);
        std::vector<polynomial_dfs<C>> master(cols);
        for (size_t c = 0; c < cols; ++c) {
            master[c].values.resize(n);
            std::memcpy(master[c].values.data(), evals + 4 * c * n, n * 32);
        }
        for (int rep = 0; rep < steps; ++rep) {
            kzg_commitment_scheme_v2_hip<C, counting_transcript> scheme(params, bls_root);
            scheme.upload_chunk = upload_chunk;
            std::vector<polynomial_dfs<C>> handed;
            if (mode == 1) handed = master;    // the copy a caller that hands its columns over never makes is outside the timing
            auto t0 = std::chrono::steady_clock::now();
            if (mode == 0) scheme.append_to_batch(0, master);
            else if (mode == 1) scheme.append_to_batch(0, std::move(handed));
            else {
                std::vector<std::reference_wrapper<const polynomial_dfs<C>>> lent(master.begin(), master.end());
                scheme.append_to_batch(0, lent);
            }
            ms[3 * rep] = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            auto commits = scheme.commit(0);
            ms[3 * rep + 1] = ms_since(t0);
            scheme.append_eval_point(0, Fr(1234567));
            scheme.append_eval_point(0, Fr(7654321));
            counting_transcript tr;
            tr.challenges = {Fr(12345), Fr(54321)};
            t0 = std::chrono::steady_clock::now();
            auto proof = scheme.proof_eval(tr);
            ms[3 * rep + 2] = ms_since(t0);
            (void)proof;
            if (out_commitments && rep == steps - 1)
                for (size_t c = 0; c < cols; ++c) commits[c].to_affine(out_commitments + 12 * c);
        }
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "zkhip_bench_kzg_scheme: %s\n", e.what());
        return -1;
    }
}

/* The same through a scheme over a DEVICE GROUP (kzg_params_group_hip: the key replicated on every member, commit(batch) dealing the columns,
 * the coefficient forms gathered on member 0 for proof_eval): `n_dev` members of THIS process, columns lent.  ms: steps x {commit, proof_eval}. */
int zkhip_bench_kzg_scheme_group(const int *devices, int n_dev, size_t log_n, size_t cols, int steps, const uint64_t *evals, double *ms,
                                 uint64_t *out_commitments) {
    try {
        const size_t n = (size_t)1 << log_n;
        device_group grp(std::vector<int>(devices, devices + n_dev));
        kzg_params_group_hip<C> params(grp, n, Fr(7));
        std::vector<polynomial_dfs<C>> master(cols);
        for (size_t c = 0; c < cols; ++c) {
            master[c].values.resize(n);
            std::memcpy(master[c].values.data(), evals + 4 * c * n, n * 32);
        }
        for (int rep = 0; rep < steps; ++rep) {
            kzg_commitment_scheme_v2_hip<C, counting_transcript> scheme(params, bls_root);
            std::vector<std::reference_wrapper<const polynomial_dfs<C>>> lent(master.begin(), master.end());
            scheme.append_to_batch(0, lent);
            auto t0 = std::chrono::steady_clock::now();
            auto commits = scheme.commit(0);
            ms[2 * rep] = ms_since(t0);
            scheme.append_eval_point(0, Fr(1234567));
            scheme.append_eval_point(0, Fr(7654321));
            counting_transcript tr;
            tr.challenges = {Fr(12345), Fr(54321)};
            t0 = std::chrono::steady_clock::now();
            auto proof = scheme.proof_eval(tr);
            ms[2 * rep + 1] = ms_since(t0);
            (void)proof;
            if (out_commitments && rep == steps - 1)
                for (size_t c = 0; c < cols; ++c) commits[c].to_affine(out_commitments + 12 * c);
        }
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "zkhip_bench_kzg_scheme_group: %s\n", e.what());
        return -1;
    }
}

/* `cols` polynomial_dfs of 2^log_n rows in host memory -> lpc_commitment_scheme_hip::append_to_batch (lent) + commit over
 * D[0] = 2^(log_n + expand): upload, inverse NTTs, extension, coset-ordered leaf layout, and the leaves to the caller's tree
 * builder.  streaming != 0: the streaming builder shape (slices absorbed by `threads` host threads while the next slice is in
 * flight); 0: round 2's std::vector shape.  ms: `steps` commit times; *root: the fold of the last one. */
int zkhip_bench_lpc_scheme(int device, size_t log_n, size_t cols, size_t expand, int steps, int streaming, unsigned threads, double *ms, uint64_t *root) {
    try {
        const size_t n = (size_t)1 << log_n;
        context ctx(device);
        fri_params_hip<C> params;
        params.log_domain = log_n + expand;
        params.step_list.assign(log_n + expand - 4, 1);    // fold down to 16 points, one step per round
        params.root_of_unity = bls_root;
        uint64_t seed = 5;
        auto sm = [&seed]() {
            uint64_t z = (seed += 0x9E3779B97F4A7C15ull);
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            return z ^ (z >> 31);
        };
        std::vector<polynomial_dfs<C>> polys(cols);
        for (auto &p : polys) {
            p.values.resize(n);
            for (auto &v : p.values) {
                uint64_t w[4] = {sm(), sm(), sm(), sm() & 0x0fffffffffffffffull};
                v = A::scalar_from_limbs(w);
            }
        }
        std::vector<std::reference_wrapper<const polynomial_dfs<C>>> lent(polys.begin(), polys.end());
        uint64_t r = 0;
        if (streaming) {
            streaming_fold_builder b;
            b.threads = threads ? threads : 8;
            lpc_commitment_scheme_hip<C, counting_transcript, streaming_fold_builder> scheme(ctx, params, b);    // ONE object: its page-locked buffers are reused
            for (int rep = 0; rep < steps; ++rep) {
                auto t0 = std::chrono::steady_clock::now();
                scheme.append_to_batch(rep, lent);
                r = scheme.commit(rep);
                ms[rep] = ms_since(t0);
            }
        } else {
            lpc_commitment_scheme_hip<C, counting_transcript, vector_fold_builder> scheme(ctx, params, vector_fold_builder());
            for (int rep = 0; rep < steps; ++rep) {
                auto t0 = std::chrono::steady_clock::now();
                scheme.append_to_batch(rep, lent);
                r = scheme.commit(rep);
                ms[rep] = ms_since(t0);
            }
        }
        if (root) *root = r;
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "zkhip_bench_lpc_scheme: %s\n", e.what());
        return -1;
    }
}

/* The same commit (same seeded polynomials, same parameters) with the DEVICE tree builder (hip/merkle.hpp): the SHA2-256 Merkle tree is built on the
 * GPU straight from the extension -- no leaf layout, no leaf over PCIe -- and commit returns its root.  ms: `steps` commit times; root: the last one. */
int zkhip_bench_lpc_scheme_device(int device, size_t log_n, size_t cols, size_t expand, int steps, double *ms, uint8_t *root) {
    try {
        const size_t n = (size_t)1 << log_n;
        context ctx(device);
        fri_params_hip<C> params;
        params.log_domain = log_n + expand;
        params.step_list.assign(log_n + expand - 4, 1);
        params.root_of_unity = bls_root;
        uint64_t seed = 5;
        auto sm = [&seed]() {
            uint64_t z = (seed += 0x9E3779B97F4A7C15ull);
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            return z ^ (z >> 31);
        };
        std::vector<polynomial_dfs<C>> polys(cols);
        for (auto &p : polys) {
            p.values.resize(n);
            for (auto &v : p.values) {
                uint64_t w[4] = {sm(), sm(), sm(), sm() & 0x0fffffffffffffffull};
                v = A::scalar_from_limbs(w);
            }
        }
        std::vector<std::reference_wrapper<const polynomial_dfs<C>>> lent(polys.begin(), polys.end());
        lpc_commitment_scheme_hip<C, counting_transcript, device_merkle_builder<>> scheme(ctx, params, device_merkle_builder<>());
        for (int rep = 0; rep < steps; ++rep) {
            auto t0 = std::chrono::steady_clock::now();
            scheme.append_to_batch(rep, lent);
            const auto r = scheme.commit(rep);
            ms[rep] = ms_since(t0);
            if (root) std::memcpy(root, r.data(), 32);
        }
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "zkhip_bench_lpc_scheme_device: %s\n", e.what());
        return -1;
    }
}

/* The same commit through a scheme over a DEVICE GROUP (hip/lpc.hpp commit_group: polynomials dealt, segments pushed to the leaf owners, each
 * owner's leaves over its own link), streaming builder, the same seeded polynomials: the fold must equal zkhip_bench_lpc_scheme's. */
int zkhip_bench_lpc_scheme_group(const int *devices, int n_dev, size_t log_n, size_t cols, size_t expand, int steps, unsigned threads, double *ms, uint64_t *root,
                                 uint64_t *owners) {
    try {
        const size_t n = (size_t)1 << log_n;
        device_group grp(std::vector<int>(devices, devices + n_dev));
        fri_params_hip<C> params;
        params.log_domain = log_n + expand;
        params.step_list.assign(log_n + expand - 4, 1);
        params.root_of_unity = bls_root;
        uint64_t seed = 5;
        auto sm = [&seed]() {
            uint64_t z = (seed += 0x9E3779B97F4A7C15ull);
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            return z ^ (z >> 31);
        };
        std::vector<polynomial_dfs<C>> polys(cols);
        for (auto &p : polys) {
            p.values.resize(n);
            for (auto &v : p.values) {
                uint64_t w[4] = {sm(), sm(), sm(), sm() & 0x0fffffffffffffffull};
                v = A::scalar_from_limbs(w);
            }
        }
        std::vector<std::reference_wrapper<const polynomial_dfs<C>>> lent(polys.begin(), polys.end());
        streaming_fold_builder b;
        b.threads = threads ? threads : 8;
        lpc_commitment_scheme_hip<C, counting_transcript, streaming_fold_builder> scheme(grp, params, b);
        uint64_t r = 0;
        for (int rep = 0; rep < steps; ++rep) {
            auto t0 = std::chrono::steady_clock::now();
            scheme.append_to_batch(rep, lent);
            r = scheme.commit(rep);
            ms[rep] = ms_since(t0);
        }
        if (root) *root = r;
        if (owners) *owners = scheme.last_leaf_owners();
        return scheme.group_commits() == (std::size_t)steps || n_dev == 1 ? 0 : -2;
    } catch (const std::exception &e) {
        fprintf(stderr, "zkhip_bench_lpc_scheme_group: %s\n", e.what());
        return -1;
    }
}

/* lpc_commitment_scheme_hip::proof_eval at size (lpc.hpp:113-200 up to and including the FRI commit phase, basic_fri.hpp:705-742): `cols`
 * polynomials of 2^log_n rows committed over D[0] = 2^(log_n + expand) (as zkhip_bench_lpc_scheme, streaming builder), every polynomial opened at
 * two points (y, y omega -- what placeholder asks of a witness column with a rotation); then proof_eval: the evaluations (block Horner over the
 * resident coefficients), the combined quotient, its extension to D[0] and the leaves of every FRI round -- one fold per round down to 16 points --
 * handed to the caller's tree builder.  ms: steps x {commit, proof_eval}.  *rounds: FRI rounds of the last proof. */
int zkhip_bench_lpc_proof_eval(int device, size_t log_n, size_t cols, size_t expand, int steps, unsigned threads, double *ms, uint64_t *rounds) {
    try {
        const size_t n = (size_t)1 << log_n;
        context ctx(device);
        fri_params_hip<C> params;
        params.log_domain = log_n + expand;
        params.step_list.assign(log_n + expand - 4, 1);
        params.root_of_unity = bls_root;
        splitmix sm {15};
        std::vector<polynomial_dfs<C>> polys(cols);
        for (auto &p : polys) {
            p.values.resize(n);
            for (auto &v : p.values) v = sm.nonzero();
        }
        std::vector<std::reference_wrapper<const polynomial_dfs<C>>> lent(polys.begin(), polys.end());
        streaming_fold_builder b;
        b.threads = threads ? threads : 8;
        const Fr y = sm.nonzero(), w = bls_root(log_n);
        for (int rep = 0; rep < steps; ++rep) {
            lpc_commitment_scheme_hip<C, counting_transcript, streaming_fold_builder> scheme(ctx, params, b);
            auto t0 = std::chrono::steady_clock::now();
            scheme.append_to_batch(0, lent);
            (void)scheme.commit(0);
            ms[2 * rep] = ms_since(t0);
            scheme.append_eval_point(0, y);
            scheme.append_eval_point(0, y * w);
            counting_transcript tr;
            for (int i = 0; i < 64; ++i) tr.challenges.push_back(sm.nonzero());
            t0 = std::chrono::steady_clock::now();
            auto proof = scheme.proof_eval(tr);
            ms[2 * rep + 1] = ms_since(t0);
            if (rounds) *rounds = proof.fri_proof.fri_roots.size();
        }
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "zkhip_bench_lpc_proof_eval: %s\n", e.what());
        return -1;
    }
}

/* The same proof_eval with the DEVICE tree builder and the SHA2-256 sequential transcript (hip/transcript.hpp), without grinding (mask == 0:
 * use_grinding stays false) and with it (fri_params.use_grinding, grinding_parameter = mask; basic_fri.hpp:743-745: the proof of work searched
 * on the device, hip/proof_of_work.hpp).  ms: steps x {commit, proof_eval}.  nonces: steps proof-of-work values (the search starts at
 * std::rand(), so the work per proof varies as it does for the reference). */
int zkhip_bench_lpc_proof_eval_grinding(int device, size_t log_n, size_t cols, size_t expand, int steps, uint32_t mask, double *ms, uint32_t *nonces) {
    try {
        const size_t n = (size_t)1 << log_n;
        context ctx(device);
        fri_params_hip<C> params;
        params.log_domain = log_n + expand;
        params.step_list.assign(log_n + expand - 4, 1);
        params.root_of_unity = bls_root;
        params.use_grinding = mask != 0;
        if (mask) params.grinding_parameter = mask;
        splitmix sm {15};
        std::vector<polynomial_dfs<C>> polys(cols);
        for (auto &p : polys) {
            p.values.resize(n);
            for (auto &v : p.values) v = sm.nonzero();
        }
        std::vector<std::reference_wrapper<const polynomial_dfs<C>>> lent(polys.begin(), polys.end());
        const Fr y = sm.nonzero(), w = bls_root(log_n);
        for (int rep = 0; rep < steps; ++rep) {
            lpc_commitment_scheme_hip<C, sha256_transcript<C>, device_merkle_builder<>> scheme(ctx, params, device_merkle_builder<>());
            auto t0 = std::chrono::steady_clock::now();
            scheme.append_to_batch(0, lent);
            (void)scheme.commit(0);
            ms[2 * rep] = ms_since(t0);
            scheme.append_eval_point(0, y);
            scheme.append_eval_point(0, y * w);
            sha256_transcript<C> tr;
            t0 = std::chrono::steady_clock::now();
            auto proof = scheme.proof_eval(tr);
            ms[2 * rep + 1] = ms_since(t0);
            if (nonces) nonces[rep] = proof.fri_proof.proof_of_work;
        }
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "zkhip_bench_lpc_proof_eval_grinding: %s\n", e.what());
        return -1;
    }
}

/* Whole opening proofs (hip/lpc.hpp: proof_eval_full = proof_eval + query_phase) on the instance above, device tree builder, SHA2-256 transcript,
 * `lambda` queries, next to the path a caller of proof_eval alone has to take for the same answers: download every round polynomial
 * (fri_round_polynomial) and every coefficient form (coefficients), evaluate every committed polynomial at the 2 lambda query points on the host.
 *   ms       steps x {proof_eval alone, proof_eval_full, query_phase alone -- timed by part: re-extension, gathers, paths, host part}  (7 per step);
 *   caller   {download ms of the round polynomials, download ms of the coefficient forms, host evaluation ms of `eval_polys` of the cols
 *            polynomials on ONE thread, host evaluation ms of all cols polynomials on `threads` threads}, measured once (eval_polys 0: the
 *            one-thread figure is skipped);
 *   launches (nullable, cap bytes) the profiler's dump -- "name ms count" lines -- of the kernels the LAST step's query_phase launched (that step
 *            runs with the per-kernel events on: keep it out of a median);
 *   *verified: verify_eval accepted the last proof. */
int zkhip_bench_lpc_query_phase(int device, size_t log_n, size_t cols, size_t expand, int steps, size_t lambda, unsigned threads, size_t eval_polys, double *ms,
                                double *caller, char *launches, size_t cap, int *verified) {
    try {
        typedef lpc_commitment_scheme_hip<C, sha256_transcript<C>, device_merkle_builder<>> base_type;
        struct scheme_type : base_type {    // the scheme with its query-phase stopwatch in reach
            using base_type::base_type;
            void time_query_phase(bool on) { this->_time_query_phase = on; }
            const typename base_type::query_phase_times &last_query_times() const { return this->_last_query_times; }
        };
        const size_t n = (size_t)1 << log_n;
        context ctx(device);
        fri_params_hip<C> params;
        params.max_degree = n - 1;
        params.log_domain = log_n + expand;
        params.step_list.assign(log_n + expand - 4, 1);
        params.root_of_unity = bls_root;
        params.lambda = lambda;
        splitmix sm {15};
        std::vector<polynomial_dfs<C>> polys(cols);
        for (auto &p : polys) {
            p.values.resize(n);
            for (auto &v : p.values) v = sm.nonzero();
        }
        std::vector<std::reference_wrapper<const polynomial_dfs<C>>> lent(polys.begin(), polys.end());
        const Fr y = sm.nonzero(), w = bls_root(log_n);
        scheme_type scheme(ctx, params, device_merkle_builder<>());
        scheme.append_to_batch(0, lent);
        const auto root = scheme.commit(0);
        scheme.append_eval_point(0, y);
        scheme.append_eval_point(0, y * w);
        scheme_type::proof_type proof;
        for (int rep = 0; rep < steps; ++rep) {
            double *out = ms + 7 * rep;
            {
                sha256_transcript<C> tr;
                const auto t0 = std::chrono::steady_clock::now();
                proof = scheme.proof_eval(tr);
                out[0] = ms_since(t0);
            }
            {
                sha256_transcript<C> tr;
                const auto t0 = std::chrono::steady_clock::now();
                proof = scheme.proof_eval_full(tr);
                out[1] = ms_since(t0);
            }
            {
                sha256_transcript<C> tr;
                proof = scheme.proof_eval(tr);
                ctx.sync();
                scheme.time_query_phase(true);
                const bool profile = launches && rep == steps - 1;
                if (profile) {
                    check(zkhip_profile_enable(ctx.get(), 1), "zkhip_profile_enable", ctx.get());
                    check(zkhip_profile_reset(ctx.get()), "zkhip_profile_reset", ctx.get());
                }
                const auto t0 = std::chrono::steady_clock::now();
                scheme.query_phase(tr, proof);
                out[2] = ms_since(t0);
                if (profile) {
                    zkhip_profile_dump(ctx.get(), launches, cap);
                    check(zkhip_profile_enable(ctx.get(), 0), "zkhip_profile_enable", ctx.get());
                }
                scheme.time_query_phase(false);
                out[3] = scheme.last_query_times().reextend_ms;
                out[4] = scheme.last_query_times().gather_ms;
                out[5] = scheme.last_query_times().paths_ms;
                out[6] = scheme.last_query_times().host_ms;
            }
        }
        {
            sha256_transcript<C> tr;
            std::map<std::size_t, scheme_type::commitment_type> commitments;
            commitments[0] = root;
            *verified = scheme.verify_eval(proof, commitments, tr) ? 1 : 0;
        }
        /* the caller's path: everything the query phase reads, brought to the host, and the evaluations at the query points */
        auto t0 = std::chrono::steady_clock::now();
        std::size_t sink = 0;
        for (std::size_t i = 1; i < params.step_list.size(); ++i) sink += scheme.fri_round_polynomial(i).values.size();
        caller[0] = ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        std::vector<std::vector<Fr>> coeffs(cols);
        for (std::size_t p = 0; p < cols; ++p) coeffs[p] = scheme.coefficients(0, p);
        caller[1] = ms_since(t0);
        std::vector<Fr> at(2 * lambda);
        for (auto &x : at) x = sm.nonzero();
        std::vector<Fr> values(cols * at.size());
        auto evaluate = [&](std::size_t lo, std::size_t hi) {    // math::polynomial::evaluate: Horner, (polynomial, point) pairs [lo, hi)
            for (std::size_t k = lo; k < hi; ++k) {
                const std::vector<Fr> &c = coeffs[k / at.size()];
                const Fr &x = at[k % at.size()];
                Fr acc = Fr::zero();
                for (std::size_t j = c.size(); j-- > 0;) acc = acc * x + c[j];
                values[k] = acc;
            }
        };
        caller[2] = 0;
        if (eval_polys) {
            t0 = std::chrono::steady_clock::now();
            evaluate(0, std::min(eval_polys, cols) * at.size());
            caller[2] = ms_since(t0);
        }
        t0 = std::chrono::steady_clock::now();
        {
            std::vector<std::thread> th;
            const std::size_t total = values.size();
            for (unsigned k = 0; k < threads; ++k) th.emplace_back(evaluate, total * k / threads, total * (k + 1) / threads);
            for (auto &t : th) t.join();
        }
        caller[3] = ms_since(t0);
        if (sink == 0 || values.empty()) return -2;
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "zkhip_bench_lpc_query_phase: %s\n", e.what());
        return -1;
    }
}

/* placeholder's quotient chain at size (hip/placeholder_quotient.hpp; prover.hpp:220-277, 314-317, gates_argument.hpp:203-216), every
 * column RESIDENT: a gate theta * q * w0 * w1(next row) * w2 over the 4n-point extended domain (4 resizes + one 4-way product + the
 * mask), a second part w1 * w2 - w3 over 2n points, F_consolidated = alpha_0 G + alpha_1 F1, its coefficients, the division by
 * X^n - 1, the split into 4 parts of n coefficients, from_coefficients, and commit(QUOTIENT_BATCH) through the KZG scheme class from
 * the resident parts.  ms: steps x {gate argument, second part, quotient_polynomial, split + from_coefficients, commit}.
 * *verified: T(y) (y^n - 1) == alpha_0 G(y) + alpha_1 F1(y) at a random y (evaluations from the coefficient forms) and every
 * commitment == part_k(alpha) G1. */
int zkhip_bench_quotient(int device, size_t log_n, int steps, double *ms, int *verified) {
    try {
        typedef placeholder_quotient_hip<C> Q;
        typedef device_polynomial_dfs<C> dfs;
        const size_t n = (size_t)1 << log_n;
        context ctx(device);
        uint64_t seed = 77;
        auto sm = [&seed]() {
            uint64_t z = (seed += 0x9E3779B97F4A7C15ull);
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            return z ^ (z >> 31);
        };
        auto rnd = [&]() {
            uint64_t w[4] = {sm(), sm(), sm(), sm() & 0x0fffffffffffffffull};
            return A::scalar_from_limbs(w);
        };
        std::vector<polynomial_dfs<C>> h(6);
        for (auto &p : h) p.values.resize(n);
        for (size_t i = 0; i < n; ++i) {
            const bool on = (i & 1) == 0;
            h[4].values[i] = on ? rnd() : Fr::zero();            // selector
            h[0].values[i] = on ? Fr::zero() : rnd();            // the gate holds on every selected row
            h[1].values[i] = rnd();
            h[2].values[i] = rnd();
            h[5].values[i] = Fr::one();                          // mask
        }
        for (size_t i = 0; i < n; ++i) h[3].values[i] = h[1].values[i] * h[2].values[i];
        std::vector<dfs> col;
        for (size_t c = 0; c < 6; ++c) col.emplace_back(ctx, h[c], c == 5 ? 0 : n - 1);
        col[4].enable_extension_cache();    // the selector and the mask are preprocessed: their extensions are kept across proofs
        col[5].enable_extension_cache();
        std::vector<polynomial_dfs<C>>().swap(h);
        std::vector<Fr> pw(n);
        Fr x = Fr::one(), alpha(7);
        for (size_t i = 0; i < n; ++i) pw[i] = x, x = x * alpha;
        kzg_params_hip<C> params(ctx, device_bases<C, ZKHIP_G1>::from_scalars(ctx, pw.begin(), pw.end()));
        std::vector<Fr>().swap(pw);
        const Fr theta = rnd(), a0 = rnd(), a1 = rnd();
        typename Q::device_coefficients T;
        std::vector<dfs> parts;
        std::vector<A::g1_value_type> commits;
        std::unique_ptr<dfs> Gk, F1k;
        for (int rep = 0; rep < steps; ++rep) {
            auto t0 = std::chrono::steady_clock::now();
            gate_product_hip<C> g;
            g.factors = {&col[4], &col[0], &col[1], &col[2]};
            g.rotations = {0, 0, 1, 0};
            g.coefficient = theta;
            dfs G = Q::gate_argument(ctx, {g}, col[5], 4 * n, bls_root);
            ms[5 * rep] = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            dfs F1 = polynomial_product<C>({col[1], col[2]}, bls_root);
            dfs w3 = col[3];
            w3.resize(2 * n, bls_root);
            F1 -= w3;
            ctx.sync();
            ms[5 * rep + 1] = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            T = Q::quotient_polynomial(ctx, {G, F1}, {a0, a1}, n, bls_root);
            ms[5 * rep + 2] = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            /* round 5: the parts stay in coefficient form on their way into the scheme (T_splitted_dfs has no other consumer, prover.hpp:199-202,
               314-317): no from_coefficients here, no coefficients() inside commit */
            auto cparts = Q::quotient_polynomial_split_coefficients(ctx, T, n, 4, n);
            ctx.sync();
            ms[5 * rep + 3] = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            kzg_commitment_scheme_v2_hip<C, counting_transcript> scheme(params, bls_root);
            scheme.append_to_batch(3, cparts);    // QUOTIENT_BATCH (proof.hpp:40)
            commits = scheme.commit(3);
            ms[5 * rep + 4] = ms_since(t0);
            if (rep == steps - 1) {
                Gk.reset(new dfs(G));
                F1k.reset(new dfs(F1));
            }
        }
        if (verified) {
            const Fr y = rnd();
            uint64_t yl[4], v[4];
            A::scalar_to_limbs(y, yl);
            auto eval = [&](const void *d, size_t len) {
                check(zkhip_poly_eval_dev(ctx.get(), A::id, d, len, len, 1, yl, 1, v), "zkhip_poly_eval_dev", ctx.get());
                return A::scalar_from_limbs(v);
            };
            auto gc = Gk->coefficients(bls_root), fc = F1k->coefficients(bls_root);
            Fr yn = y;
            for (size_t k = 0; k < log_n; ++k) yn = yn * yn;
            bool ok = eval(T.data.get(), T.size) * (yn - Fr::one()) == a0 * eval(gc.get(), Gk->size()) + a1 * eval(fc.get(), F1k->size());
            uint64_t al[4];
            A::scalar_to_limbs(alpha, al);
            for (size_t k = 0; k < 4 && ok; ++k) {
                const size_t lo = k * n, len = lo < T.size ? std::min(n, T.size - lo) : 0;
                Fr e = Fr::zero();
                if (len) {
                    check(zkhip_poly_eval_dev(ctx.get(), A::id, T.at(lo), len, len, 1, al, 1, v), "zkhip_poly_eval_dev", ctx.get());
                    e = A::scalar_from_limbs(v);
                }
                std::vector<Fr> one = {e};
                ok = commits[k] == device_bases<C, ZKHIP_G1>::from_scalars(ctx, one.begin(), one.end()).at(0);
            }
            *verified = ok ? 1 : 0;
        }
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "zkhip_bench_quotient: %s\n", e.what());
        return -1;
    }
}

/* The gate argument of a circuit with MANY gates (VERDICT r5 missing #2: the quotient leg's one four-factor gate hides what per-term launches
 * cost): n_gates gates, each a (preprocessed, cached) selector times a sum of 3 products of 2 - 4 witness columns with rotations from
 * {0, +1, -1} -- 3 - 5 factors per product with the selector -- over n_wit witness columns of 2^log_n rows, on the 8 n-point extended domain
 * (n * 2^ceil(log2(5 + 1)), gates_argument.hpp:149-150), masked.  ms: steps x {fused: one launch over the flat program; per_term: round 5's
 * two launches per product}, both INCLUDING the extensions of the witness columns (the selectors' and the mask's extensions are cached:
 * preprocessed).  info: {products, distinct columns, distinct (column, rotation) pairs, gate_eval kernel ms of the last fused run}.
 * *verified: both evaluations bit-equal, and F(y) == mask(y) sum_g sel_g(y) sum_t c_t prod_f col_f(omega^rot y) at a random y with every
 * polynomial evaluated from its COEFFICIENT form (independent of the extension, the rotations' index arithmetic and the program). */
int zkhip_bench_gate_argument(int device, size_t log_n, size_t n_gates, size_t n_wit, int steps, double *ms, double *info, int *verified) {
    try {
        typedef placeholder_quotient_hip<C> Q;
        typedef device_polynomial_dfs<C> dfs;
        const size_t n = (size_t)1 << log_n, ext = 8 * n;
        context ctx(device);
        /* the per-term path holds one extension per distinct (column, rotation) pair (99 x 268 MB): both paths get a block cache that keeps
           their buffers across repetitions, so that neither is timed through the driver's allocator (hundreds of ms when it has to scavenge) */
        ctx.set_option("alloc_cache_mb", 96 * 1024);
        uint64_t seed = 4242;
        auto sm = [&seed]() {
            uint64_t z = (seed += 0x9E3779B97F4A7C15ull);
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            return z ^ (z >> 31);
        };
        auto rnd = [&]() {
            uint64_t w[4] = {sm(), sm(), sm(), sm() & 0x0fffffffffffffffull};
            return A::scalar_from_limbs(w);
        };
        /* columns are generated ON the device (a host vector of 2^20 field values per column would take minutes to fill for 56 columns):
           column c = the inverse transform of nothing in particular -- its rows are c-dependent multiples of the powers of a random base */
        std::vector<dfs> sel, wit;
        auto fill = [&](std::vector<dfs> &out, size_t count) {
            polynomial_dfs<C> h;
            h.values.resize(n);
            for (size_t c = 0; c < count; ++c) {
                const Fr base = rnd();
                Fr x = rnd();
                for (size_t i = 0; i < n; ++i) h.values[i] = x, x = x * base;
                out.emplace_back(ctx, h, n - 1);
            }
        };
        fill(sel, n_gates);
        fill(wit, n_wit);
        polynomial_dfs<C> hm;
        hm.values.assign(n, Fr::one());
        for (size_t i = n - 8; i < n; ++i) hm.values[i] = Fr::zero();
        dfs mask(ctx, hm, n - 1);
        for (auto &s : sel) s.enable_extension_cache();
        mask.enable_extension_cache();
        std::vector<gate_product_hip<C>> products;
        const int rots[3] = {0, 1, -1};
        std::vector<std::pair<const dfs *, int>> pairs;
        for (size_t g = 0; g < n_gates; ++g)
            for (int t = 0; t < 3; ++t) {
                gate_product_hip<C> p;
                p.factors.push_back(&sel[g]);
                p.rotations.push_back(0);
                const size_t k = 2 + (sm() % 3);    // 2 - 4 witness factors
                for (size_t f = 0; f < k; ++f) {
                    p.factors.push_back(&wit[sm() % n_wit]);
                    p.rotations.push_back(rots[sm() % 3]);
                }
                p.coefficient = rnd();
                for (size_t f = 0; f < p.factors.size(); ++f) {
                    const std::pair<const dfs *, int> key(p.factors[f], p.rotations[f]);
                    if (std::find(pairs.begin(), pairs.end(), key) == pairs.end()) pairs.push_back(key);
                }
                products.push_back(std::move(p));
            }
        info[0] = (double)products.size();
        info[1] = (double)(n_gates + n_wit);
        info[2] = (double)pairs.size();
        std::unique_ptr<dfs> fused, per_term;
        for (int rep = 0; rep < steps; ++rep) {
            auto t0 = std::chrono::steady_clock::now();
            dfs F = Q::gate_argument(ctx, products, mask, ext, bls_root);
            ctx.sync();
            ms[2 * rep] = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            dfs P = Q::gate_argument_per_term(ctx, products, mask, ext, bls_root);
            ctx.sync();
            ms[2 * rep + 1] = ms_since(t0);
            if (rep == steps - 1) {
                fused.reset(new dfs(F));
                per_term.reset(new dfs(P));
            }
        }
        /* the kernel alone: one more fused run with HIP events around its launches */
        zkhip_profile_reset(ctx.get());
        zkhip_profile_enable(ctx.get(), 1);
        (void)Q::gate_argument(ctx, products, mask, ext, bls_root);
        zkhip_profile_enable(ctx.get(), 0);
        double kms = 0;
        uint64_t kc = 0;
        zkhip_profile_get(ctx.get(), "gate_eval", &kms, &kc);
        info[3] = kms;
        if (verified) {
            std::vector<uint64_t> a(4 * ext), b(4 * ext);
            ctx.d2h(a.data(), fused->data(), ext * 32);
            ctx.d2h(b.data(), per_term->data(), ext * 32);
            bool ok = a == b && fused->degree() == per_term->degree();
            std::vector<uint64_t>().swap(a);
            std::vector<uint64_t>().swap(b);
            const Fr y = rnd(), w = bls_root(log_n), wi = w.inversed();
            const Fr pts[3] = {y, y * w, y * wi};    // rotation 0, +1, -1
            uint64_t pl[12], v[12];
            for (int i = 0; i < 3; ++i) A::scalar_to_limbs(pts[i], pl + 4 * i);
            auto evals_of = [&](const dfs &p) {    // p at y, omega y, omega^-1 y from its coefficients
                auto c = p.coefficients(bls_root);
                check(zkhip_poly_eval_dev(ctx.get(), A::id, c.get(), p.size(), p.size(), 1, pl, 3, v), "zkhip_poly_eval_dev", ctx.get());
                return std::array<Fr, 3> {A::scalar_from_limbs(v), A::scalar_from_limbs(v + 4), A::scalar_from_limbs(v + 8)};
            };
            std::map<const dfs *, std::array<Fr, 3>> at;
            for (const auto &s : sel) at[&s] = evals_of(s);
            for (const auto &c : wit) at[&c] = evals_of(c);
            Fr total = Fr::zero();
            for (const auto &p : products) {
                Fr t = p.coefficient;
                for (size_t f = 0; f < p.factors.size(); ++f) t = t * at[p.factors[f]][p.rotations[f] == 0 ? 0 : (p.rotations[f] == 1 ? 1 : 2)];
                total = total + t;
            }
            total = total * evals_of(mask)[0];
            ok = ok && evals_of(*fused)[0] == total;
            *verified = ok ? 1 : 0;
        }
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "zkhip_bench_gate_argument: %s\n", e.what());
        return -1;
    }
}

/* placeholder's permutation argument at size (hip/placeholder_permutation.hpp; permutation_argument.hpp:70-224): k permuted columns of
 * 2^log_n rows, resident.  ms: steps x {grand product (g_v, h_v, V_P: zkhip_perm_grand_product_dev), whole prove_eval}.
 * *verified: V_P[0] = 1 and V_P[j + 1] prod_i h_i[j] == V_P[j] prod_i g_i[j] at 64 sampled rows (host arithmetic over downloaded rows), and
 * F_1(y) == (1 - q_last(y) - q_blind(y)) (V_P(omega y) h(y) - V_P(y) g(y)) at a random y, every polynomial evaluated from its coefficient form. */
int zkhip_bench_permutation(int device, size_t log_n, size_t k, int steps, double *ms, int *verified) {
    try {
        typedef placeholder_permutation_hip<C> PA;
        typedef device_polynomial_dfs<C> dfs;
        const size_t n = (size_t)1 << log_n;
        context ctx(device);
        uint64_t seed = 99;
        auto sm = [&seed]() {
            uint64_t z = (seed += 0x9E3779B97F4A7C15ull);
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            return z ^ (z >> 31);
        };
        auto rnd = [&]() {
            uint64_t w[4] = {sm(), sm(), sm(), sm() & 0x0fffffffffffffffull};
            return A::scalar_from_limbs(w);
        };
        std::vector<polynomial_dfs<C>> h(3 * k + 3);
        for (auto &p : h) {
            p.values.resize(n);
            for (auto &v : p.values) v = rnd();
        }
        for (size_t j = 0; j < n; ++j) {    // q_last, q_blind, lagrange_0 as placeholder shapes them
            h[3 * k].values[j] = j == n - 4 ? Fr::one() : Fr::zero();
            h[3 * k + 1].values[j] = j > n - 4 ? Fr::one() : Fr::zero();
            h[3 * k + 2].values[j] = j == 0 ? Fr::one() : Fr::zero();
        }
        std::vector<dfs> all;
        for (auto &p : h) all.emplace_back(ctx, p, n - 1);
        /* the preprocessed polynomials (S_id, S_sigma, q_last, q_blind, lagrange_0) are the same in every proof: the key holder keeps their extensions
           (device_polynomial_dfs::enable_extension_cache); the witness columns are not cached across proofs */
        for (size_t i = k; i < all.size(); ++i) all[i].enable_extension_cache();
        std::vector<dfs> cols(all.begin(), all.begin() + k), sid(all.begin() + k, all.begin() + 2 * k), ssig(all.begin() + 2 * k, all.begin() + 3 * k);
        const Fr beta = rnd(), gamma = rnd();
        std::unique_ptr<PA::prover_result_type> last;
        for (int rep = 0; rep < steps; ++rep) {
            /* the grand product alone */
            auto d_g = ctx.alloc(k * n * 32), d_h = ctx.alloc(k * n * 32), d_v = ctx.alloc(n * 32);
            std::vector<const void *> pc, pi, ps;
            for (size_t i = 0; i < k; ++i) pc.push_back(cols[i].data()), pi.push_back(sid[i].data()), ps.push_back(ssig[i].data());
            uint64_t bl[4], gl[4];
            A::scalar_to_limbs(beta, bl);
            A::scalar_to_limbs(gamma, gl);
            ctx.sync();
            auto t0 = std::chrono::steady_clock::now();
            check(zkhip_perm_grand_product_dev(ctx.get(), A::id, k, pc.data(), pi.data(), ps.data(), n, bl, gl, d_g.get(), d_h.get(), d_v.get()),
                  "zkhip_perm_grand_product_dev", ctx.get());
            ctx.sync();
            ms[2 * rep] = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            last.reset(new PA::prover_result_type(PA::prove_eval(ctx, cols, sid, ssig, all[3 * k], all[3 * k + 1], all[3 * k + 2], beta, gamma, bls_root)));
            ms[2 * rep + 1] = ms_since(t0);
        }
        if (verified) {
            bool ok = true;
            std::vector<uint64_t> vp(4 * n);
            ctx.d2h(vp.data(), last->permutation_polynomial_dfs.data(), n * 32);
            ok = A::scalar_from_limbs(vp.data()) == Fr::one();
            for (int t = 0; t < 64 && ok; ++t) {
                const size_t j = sm() % (n - 1);
                Fr nom = Fr::one(), den = Fr::one();
                for (size_t i = 0; i < k; ++i) {
                    nom = nom * (h[i].values[j] + beta * h[k + i].values[j] + gamma);
                    den = den * (h[i].values[j] + beta * h[2 * k + i].values[j] + gamma);
                }
                ok = A::scalar_from_limbs(&vp[4 * (j + 1)]) * den == A::scalar_from_limbs(&vp[4 * j]) * nom;
            }
            /* F_1 at a random point */
            const Fr y = rnd();
            uint64_t yl[4], v[4];
            auto eval_at = [&](const dfs &p, const Fr &x) {
                A::scalar_to_limbs(x, yl);
                auto c = p.coefficients(bls_root);
                check(zkhip_poly_eval_dev(ctx.get(), A::id, c.get(), p.size(), p.size(), 1, yl, 1, v), "zkhip_poly_eval_dev", ctx.get());
                return A::scalar_from_limbs(v);
            };
            Fr gy = Fr::one(), hy = Fr::one();
            for (size_t i = 0; i < k; ++i) {
                const Fr c = eval_at(cols[i], y);
                gy = gy * (c + beta * eval_at(sid[i], y) + gamma);
                hy = hy * (c + beta * eval_at(ssig[i], y) + gamma);
            }
            const dfs &VP = last->permutation_polynomial_dfs;
            const Fr lhs = eval_at(last->F_dfs[1], y);
            const Fr rhs = (Fr::one() - eval_at(all[3 * k], y) - eval_at(all[3 * k + 1], y)) * (eval_at(VP, y * bls_root(log_n)) * hy - eval_at(VP, y) * gy);
            ok = ok && lhs == rhs;
            *verified = ok ? 1 : 0;
        }
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "zkhip_bench_permutation: %s\n", e.what());
        return -1;
    }
}

/* placeholder's lookup argument, prover side, from the sorted vectors on (hip/placeholder_lookup.hpp; lookup_argument.hpp:153-296): k_in inputs drawn
 * from k_val table columns of 2^log_n rows, resident.  A GENUINE instance: table column i is zero at row 0, holds usable_rows / 2 distinct non-zero values
 * behind it and zeros after them; the inputs take table values (or zero) in the usable rows; `sorted` is built on the host as sort_polynomials (:565-638)
 * builds it -- as the EXPECTATION: the timed argument sorts on the device (LA::sort_polynomials) and its vectors must equal the host's entry by entry.
 * ms: steps x {sort_polynomials, V_L alone (zkhip_lookup_grand_product_dev), the whole argument = sort + prove_eval}.
 * *verified: V_L[0] = 1, V_L[usable_rows] = 1 -- the product over all rows closes: the reference's own BOOST_CHECK (:217) --, zeros behind it, the
 * recurrence at 64 sampled rows (host arithmetic), and F_2(y) == ((q_last + q_blind)(y) - 1)(V_L(y) g(y) - V_L(omega y) h(y)) at a random y, every
 * polynomial evaluated from its coefficient form. */
int zkhip_bench_lookup(int device, size_t log_n, size_t k_in, size_t k_val, int steps, double *ms, int *verified) {
    try {
        typedef placeholder_lookup_hip<C> LA;
        typedef device_polynomial_dfs<C> dfs;
        const size_t n = (size_t)1 << log_n, usable = n - 4, total = k_in + k_val, T = usable / 2;
        context ctx(device);
        uint64_t seed = 777;
        auto sm = [&seed]() {
            uint64_t z = (seed += 0x9E3779B97F4A7C15ull);
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            return z ^ (z >> 31);
        };
        auto rnd = [&]() {
            uint64_t w[4] = {sm() | 1, sm(), sm(), sm() & 0x0fffffffffffffffull};    // never zero
            return A::scalar_from_limbs(w);
        };
        std::vector<polynomial_dfs<C>> value, input, sorted;
        splitmix gen {seed};
        build_lookup_instance(gen, n, usable, k_in, k_val, value, input, sorted);
        seed = gen.seed;
        polynomial_dfs<C> hq_last, hq_blind, hl0;
        hq_last.values.assign(n, Fr::zero());
        hq_blind.values.assign(n, Fr::zero());
        hl0.values.assign(n, Fr::zero());
        hq_last.values[usable] = Fr::one();
        for (size_t j = usable + 1; j < n; ++j) hq_blind.values[j] = Fr::one();
        hl0.values[0] = Fr::one();
        std::vector<dfs> d_in, d_val, d_sorted;
        for (auto &p : input) d_in.emplace_back(ctx, p, n - 1);
        for (auto &p : value) d_val.emplace_back(ctx, p, n - 1);
        for (auto &p : sorted) d_sorted.emplace_back(ctx, p, n - 1);
        dfs q_last(ctx, hq_last, n - 1), q_blind(ctx, hq_blind, n - 1), lagrange_0(ctx, hl0, n - 1);
        for (dfs *p : {&q_last, &q_blind, &lagrange_0}) p->enable_extension_cache();    // preprocessed: their extensions are the same in every proof
        const Fr beta = rnd(), gamma = rnd();
        std::vector<Fr> alphas;
        for (size_t i = 0; i + 1 < total; ++i) alphas.push_back(rnd());
        std::unique_ptr<LA::prover_result_type> last;
        bool sort_ok = true;
        for (int rep = 0; rep < steps; ++rep) {
            ctx.sync();
            auto t0 = std::chrono::steady_clock::now();
            /* sort_polynomials on the device (lookup_argument.hpp:187-189); its result replaces the host-built vectors from here on */
            std::vector<dfs> dev_sorted = LA::sort_polynomials(ctx, d_in, d_val, n, usable);
            ctx.sync();
            ms[3 * rep] = ms_since(t0);
            if (rep == 0 && verified) {    // every entry of every sorted vector against the host's construction (from the draw counts, no map)
                std::vector<uint64_t> got(4 * n);
                for (size_t i = 0; i < total && sort_ok; ++i) {
                    ctx.d2h(got.data(), dev_sorted[i].data(), n * 32);
                    uint64_t want[4];
                    for (size_t j = 0; j < n && sort_ok; ++j) {
                        A::scalar_to_limbs(sorted[i].values[j], want);
                        sort_ok = std::memcmp(want, &got[4 * j], 32) == 0;
                    }
                }
                sort_ok = sort_ok && ctx.device_status() == 0;
            }
            for (auto &p : dev_sorted) p.set_degree(n - 1);
            t0 = std::chrono::steady_clock::now();
            {
                dfs v = LA::compute_V_L(ctx, dev_sorted, d_in, d_val, beta, gamma, usable);
                ctx.sync();
            }
            ms[3 * rep + 1] = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            last.reset(new LA::prover_result_type(LA::prove_eval(ctx, d_in, d_val, dev_sorted, q_last, q_blind, lagrange_0, beta, gamma, alphas, usable, bls_root)));
            ms[3 * rep + 2] = ms_since(t0) + ms[3 * rep];    // the whole argument: sort + prove_eval from the sorted vectors on
        }
        if (verified) {
            std::vector<uint64_t> vl(4 * n);
            ctx.d2h(vl.data(), last->V_L.data(), n * 32);
            auto V = [&](size_t j) { return A::scalar_from_limbs(&vl[4 * j]); };
            bool ok = sort_ok && V(0) == Fr::one() && V(usable) == Fr::one();
            for (size_t j = usable + 1; j < n && ok; ++j) ok = V(j) == Fr::zero();
            const Fr part1 = (Fr::one() + beta) * gamma;
            for (int t = 0; t < 64 && ok; ++t) {
                const size_t j = sm() % usable;
                Fr g = Fr::one(), h = Fr::one();
                for (auto &p : input) g = g * (Fr::one() + beta) * (gamma + p.values[j]);
                for (auto &p : value) g = g * (part1 + p.values[j] + beta * p.values[j + 1]);
                for (auto &p : sorted) h = h * (part1 + p.values[j] + beta * p.values[j + 1]);
                ok = V(j + 1) * h == V(j) * g;
            }
            /* F_2 at a random point */
            const Fr y = rnd(), w = bls_root(log_n);
            uint64_t yl[4], v[4];
            auto eval_at = [&](const dfs &p, const Fr &x) {
                A::scalar_to_limbs(x, yl);
                auto c = p.coefficients(bls_root);
                check(zkhip_poly_eval_dev(ctx.get(), A::id, c.get(), p.size(), p.size(), 1, yl, 1, v), "zkhip_poly_eval_dev", ctx.get());
                return A::scalar_from_limbs(v);
            };
            Fr gy = Fr::one(), hy = Fr::one();
            for (auto &p : d_in) gy = gy * (Fr::one() + beta) * (gamma + eval_at(p, y));
            for (auto &p : d_val) gy = gy * (part1 + eval_at(p, y) + beta * eval_at(p, y * w));
            for (auto &p : d_sorted) hy = hy * (part1 + eval_at(p, y) + beta * eval_at(p, y * w));
            const Fr lhs = eval_at(last->F_dfs[2], y);
            const Fr rhs = (eval_at(q_last, y) + eval_at(q_blind, y) - Fr::one()) * (eval_at(last->V_L, y) * gy - eval_at(last->V_L, y * w) * hy);
            ok = ok && lhs == rhs;
            *verified = ok ? 1 : 0;
        }
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "zkhip_bench_lookup: %s\n", e.what());
        return -1;
    }
}

/* One placeholder-shaped prover round at BASELINE config 5's row count, the pieces composed as placeholder_prover::process strings them
 * (prover.hpp:170-218, 262-277, 220-259, 314-317) over GENUINE instances, every polynomial resident from the arguments to the commitments:
 *   permutation argument (4 permuted columns, copy constraints closed inside the usable rows) -> V_P to PERMUTATION_BATCH,
 *   lookup argument (2 inputs over 1 table column; sort_polynomials on the device -> LOOKUP_BATCH + commit, V_L -> PERMUTATION_BATCH) + commit(PERMUTATION_BATCH),
 *   gate argument q (w0 w1 - w2) masked by 1 - q_last - q_blind over the 4n-point domain,
 *   quotient of the eight constraint polynomials (domains 2n .. 8n) by X^n - 1 -- exact: every part vanishes on the rows --, split into 8 parts,
 *   commit(QUOTIENT_BATCH).
 * witness_cols > 0: the round is preceded by commit(VARIABLE_VALUES_BATCH) of that many resident witness columns (prover.hpp:130-142) and followed by the
 * opening proof of everything committed (prover.hpp:363-410: the witness columns at y and y omega, V_P and V_L at y and y omega, the sorted vectors at y,
 * y omega and y omega^usable, the quotient parts at y) -- BASELINE config 5's proof shape, device side, in one figure.
 * ms: steps x {witness commit, permutation, lookup (with its LOOKUP_BATCH commit), PERMUTATION_BATCH commit, gate argument, quotient, split, QUOTIENT_BATCH commit,
 * proof_eval} (9 numbers; the first and the last are 0 when witness_cols == 0).
 * *verified: the device's sorted vectors equal the host's construction entry by entry, V_P[usable] = V_L[usable] = 1, the division left no remainder (quotient_polynomial throws otherwise) and
 * T(y) (y^n - 1) == sum_i alpha_i F_i(y) at a random y, every polynomial evaluated from its coefficient form. */
int zkhip_bench_placeholder_round(int device, size_t log_n, size_t witness_cols, int steps, double *ms, int *verified) {
    try {
        typedef placeholder_quotient_hip<C> Q;
        typedef placeholder_permutation_hip<C> PA;
        typedef placeholder_lookup_hip<C> LA;
        typedef device_polynomial_dfs<C> dfs;
        const size_t n = (size_t)1 << log_n, usable = n - 4, k = 4;
        context ctx(device);
        splitmix sm {4242};
        std::vector<polynomial_dfs<C>> h_cols, h_sid, h_ssig, h_val, h_in, h_sorted;
        build_permutation_instance(sm, log_n, usable, k, h_cols, h_sid, h_ssig);
        build_lookup_instance(sm, n, usable, 2, 1, h_val, h_in, h_sorted);
        polynomial_dfs<C> hq, hw0, hw1, hw2, hq_last, hq_blind, hl0;
        for (auto *p : {&hq, &hw0, &hw1, &hw2, &hq_last, &hq_blind, &hl0}) p->values.assign(n, Fr::zero());
        for (size_t j = 0; j < n; ++j) {
            hq.values[j] = (j % 3 == 0 && j < usable) ? Fr::one() : Fr::zero();
            hw0.values[j] = sm.nonzero();
            hw1.values[j] = sm.nonzero();
            hw2.values[j] = hq.values[j] == Fr::one() ? hw0.values[j] * hw1.values[j] : sm.nonzero();
        }
        hq_last.values[usable] = Fr::one();
        for (size_t j = usable + 1; j < n; ++j) hq_blind.values[j] = Fr::one();
        hl0.values[0] = Fr::one();
        auto up = [&](std::vector<polynomial_dfs<C>> &v) {
            std::vector<dfs> out;
            for (auto &p : v) out.emplace_back(ctx, p, n - 1);
            std::vector<polynomial_dfs<C>>().swap(v);
            return out;
        };
        std::vector<dfs> cols = up(h_cols), sid = up(h_sid), ssig = up(h_ssig), l_val = up(h_val), l_in = up(h_in), sorted = up(h_sorted);
        dfs q(ctx, hq, n - 1), w0(ctx, hw0, n - 1), w1(ctx, hw1, n - 1), w2(ctx, hw2, n - 1), q_last(ctx, hq_last, n - 1), q_blind(ctx, hq_blind, n - 1),
            lagrange_0(ctx, hl0, n - 1);
        /* preprocessed polynomials: their extensions are kept across proofs (the key holder's side of device_polynomial_dfs::enable_extension_cache) */
        for (auto *v : {&sid, &ssig})
            for (auto &p : *v) p.enable_extension_cache();
        for (dfs *p : {&q, &q_last, &q_blind, &lagrange_0}) p->enable_extension_cache();
        dfs mask = placeholder_lookup_hip<C>::affine(q_last, &q_blind, Fr::zero() - Fr::one(), Fr::zero() - Fr::one(), Fr::one());    // 1 - q_last - q_blind: preprocessed too
        mask.enable_extension_cache();
        std::vector<Fr> pw(n);
        Fr x = Fr::one(), alpha(7);
        for (size_t i = 0; i < n; ++i) pw[i] = x, x = x * alpha;
        kzg_params_hip<C> params(ctx, device_bases<C, ZKHIP_G1>::from_scalars(ctx, pw.begin(), pw.end()));
        std::vector<Fr>().swap(pw);
        std::vector<dfs> witness;    // resident witness columns: a few distinct random ones, uploaded in turn (the values do not change the work)
        if (witness_cols) {
            std::vector<polynomial_dfs<C>> h(std::min<size_t>(witness_cols, 5));
            for (auto &p : h) {
                p.values.resize(n);
                for (auto &v : p.values) v = sm.nonzero();
            }
            for (size_t c = 0; c < witness_cols; ++c) witness.emplace_back(ctx, h[c % h.size()], n - 1);
        }
        const Fr bp = sm.nonzero(), gp = sm.nonzero(), bl = sm.nonzero(), gl = sm.nonzero();
        const std::vector<Fr> l_alphas = {sm.nonzero(), sm.nonzero()};
        std::vector<Fr> alphas;
        for (int i = 0; i < 8; ++i) alphas.push_back(sm.nonzero());
        std::vector<dfs> F;
        typename Q::device_coefficients T;
        std::unique_ptr<PA::prover_result_type> perm;
        std::unique_ptr<LA::prover_result_type> look;
        constexpr std::size_t VARIABLE_VALUES_BATCH = 1, PERMUTATION_BATCH = 2, QUOTIENT_BATCH = 3, LOOKUP_BATCH = 4;
        bool sort_ok = true;
        for (int rep = 0; rep < steps; ++rep) {
            double *t = ms + 9 * rep + 1;
            kzg_commitment_scheme_v2_hip<C, counting_transcript> scheme(params, bls_root);
            ctx.sync();
            auto t0 = std::chrono::steady_clock::now();
            t[-1] = 0;
            if (witness_cols) {
                scheme.append_to_batch(VARIABLE_VALUES_BATCH, witness);
                if (scheme.commit(VARIABLE_VALUES_BATCH).size() != witness_cols) throw std::runtime_error("placeholder round: witness batch");
                t[-1] = ms_since(t0);
                t0 = std::chrono::steady_clock::now();
            }
            perm.reset(new PA::prover_result_type(PA::prove_eval(ctx, cols, sid, ssig, q_last, q_blind, lagrange_0, bp, gp, bls_root)));
            scheme.append_to_batch(PERMUTATION_BATCH, perm->permutation_polynomial_dfs);
            t[0] = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            /* lookup_argument.hpp:187-196: sort_polynomials ON THE DEVICE (round 4 uploaded a host-built `sorted`), LOOKUP_BATCH, commit */
            std::vector<dfs> dev_sorted = LA::sort_polynomials(ctx, l_in, l_val, n, usable);
            for (auto &p : dev_sorted) p.set_degree(n - 1);
            if (rep == 0 && verified) {    // against the host's construction of the same vectors (from the draw counts)
                std::vector<uint64_t> a(4 * n), b(4 * n);
                for (size_t i = 0; i < sorted.size(); ++i) {
                    ctx.d2h(a.data(), dev_sorted[i].data(), n * 32);
                    ctx.d2h(b.data(), sorted[i].data(), n * 32);
                    sort_ok = sort_ok && a == b;
                }
                sort_ok = sort_ok && ctx.device_status() == 0;
            }
            scheme.append_to_batch(LOOKUP_BATCH, dev_sorted);
            auto lookup_commit = scheme.commit(LOOKUP_BATCH);
            look.reset(new LA::prover_result_type(LA::prove_eval(ctx, l_in, l_val, dev_sorted, q_last, q_blind, lagrange_0, bl, gl, l_alphas, usable, bls_root)));
            scheme.append_to_batch(PERMUTATION_BATCH, look->V_L);
            t[1] = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            auto perm_commit = scheme.commit(PERMUTATION_BATCH);
            t[2] = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            gate_product_hip<C> g1, g2;
            g1.factors = {&q, &w0, &w1};
            g1.rotations = {0, 0, 0};
            g1.coefficient = Fr::one();
            g2.factors = {&q, &w2};
            g2.rotations = {0, 0};
            g2.coefficient = Fr::zero() - Fr::one();
            dfs G = Q::gate_argument(ctx, {g1, g2}, mask, 4 * n, bls_root);
            ctx.sync();
            t[3] = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            F = {perm->F_dfs[0], perm->F_dfs[1], perm->F_dfs[2], look->F_dfs[0], look->F_dfs[1], look->F_dfs[2], look->F_dfs[3], G};
            T = Q::quotient_polynomial(ctx, F, alphas, n, bls_root);
            t[4] = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            auto parts = Q::quotient_polynomial_split_coefficients(ctx, T, n, 8, n);    // coefficient form straight into the scheme (see zkhip_bench_quotient)
            ctx.sync();
            t[5] = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            scheme.append_to_batch(QUOTIENT_BATCH, parts);
            auto t_commit = scheme.commit(QUOTIENT_BATCH);
            t[6] = ms_since(t0);
            if (lookup_commit.size() != 3 || perm_commit.size() != 2 || t_commit.size() != 8) throw std::runtime_error("placeholder round: batch sizes");
            t[7] = 0;
            if (witness_cols) {    // the evaluation points of prover.hpp:363-410, then the opening proof of all four batches
                const Fr y = sm.nonzero(), w = bls_root(log_n);
                Fr wu = Fr::one();
                {    // omega^usable by square and multiply
                    Fr acc = Fr::one(), sq = w;
                    for (size_t e = usable; e; e >>= 1) {
                        if (e & 1) acc = acc * sq;
                        sq = sq * sq;
                    }
                    wu = acc;
                }
                scheme.append_eval_point(VARIABLE_VALUES_BATCH, y);
                for (size_t c = 0; c < witness_cols; c += 2) scheme.append_eval_point(VARIABLE_VALUES_BATCH, c, y * w);    // every other column has a rotation
                scheme.append_eval_points(PERMUTATION_BATCH, {y, y * w});
                scheme.append_eval_points(LOOKUP_BATCH, {y, y * w, y * wu});
                scheme.append_eval_point(QUOTIENT_BATCH, y);
                counting_transcript tr;
                tr.challenges = {sm.nonzero(), sm.nonzero()};
                t0 = std::chrono::steady_clock::now();
                auto proof = scheme.proof_eval(tr);
                t[7] = ms_since(t0);
                (void)proof;
            }
        }
        if (verified) {
            uint64_t one_at[4];
            auto at_row = [&](const dfs &p, size_t row) {
                ctx.d2h(one_at, static_cast<const char *>(p.data()) + 32 * row, 32);
                return A::scalar_from_limbs(one_at);
            };
            bool ok = sort_ok && at_row(perm->permutation_polynomial_dfs, usable) == Fr::one() && at_row(look->V_L, usable) == Fr::one();
            const Fr y = sm.nonzero();
            uint64_t yl[4], v[4];
            A::scalar_to_limbs(y, yl);
            auto eval = [&](const void *d, size_t len) {
                check(zkhip_poly_eval_dev(ctx.get(), A::id, d, len, len, 1, yl, 1, v), "zkhip_poly_eval_dev", ctx.get());
                return A::scalar_from_limbs(v);
            };
            Fr rhs = Fr::zero();
            for (size_t i = 0; i < F.size(); ++i) {
                auto c = F[i].coefficients(bls_root);
                rhs = rhs + alphas[i] * eval(c.get(), F[i].size());
            }
            Fr yn = y;
            for (size_t b = 0; b < log_n; ++b) yn = yn * yn;
            ok = ok && eval(T.data.get(), T.size) * (yn - Fr::one()) == rhs;
            *verified = ok ? 1 : 0;
        }
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "zkhip_bench_placeholder_round: %s\n", e.what());
        return -1;
    }
}

}    // extern "C"
