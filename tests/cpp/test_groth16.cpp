// R1cs and Groth16Prover (include/pairing_amd.hpp): the evaluation and k proofs
// through the C++ classes, compared word for word with what the caller expects.
//
// usage: test_groth16 DATA_FILE
// DATA_FILE, all u64 unless said: n_rows, n_vars, n_public, log_n, h_len, k;
// alpha_g1, beta_g1, delta_g1 (pa_g1_affine), beta_g2, delta_g2 (pa_g2_affine);
// a_query, b_g1_query (n_vars pa_g1_affine), b_g2_query (n_vars pa_g2_affine),
// l_query (n_vars - n_public), h_query (h_len); for A, B, C: nnz, row_ptr
// (n_rows + 1), col (nnz, one u64 each), val (nnz pa_fr); witness (k n_vars
// pa_fr), r, s (k pa_fr); expected a, b, c (k 2^log_n pa_fr each); expected
// proofs (k pa_groth16_proof).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <vector>

#include "pairing_amd.hpp"

using namespace pairing_amd;

static int g_failures = 0;
#define EXPECT(c)                                                      \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("  %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            g_failures++;                                              \
        }                                                              \
    } while (0)

template <class T>
static void read_rows(std::ifstream& f, std::vector<T>& v, size_t n) {
    v.resize(n);
    if (n) f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(sizeof(T) * n));
    if (!f) throw std::runtime_error("short data file");
}

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0);
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s DATA_FILE\n", argv[0]);
        return 2;
    }
    try {
        static_assert(sizeof(pa_groth16_proof) == 51 * 8, "a proof is 51 words");
        std::ifstream f(argv[1], std::ios::binary);
        uint64_t head[6];
        f.read(reinterpret_cast<char*>(head), sizeof head);
        const size_t n_rows = head[0], n_vars = head[1], n_public = head[2], h_len = head[4], k = head[5];
        const unsigned log_n = (unsigned)head[3];
        pa_groth16_key key;
        std::memset(&key, 0, sizeof key);
        f.read(reinterpret_cast<char*>(&key.alpha_g1), sizeof(pa_g1_affine));
        f.read(reinterpret_cast<char*>(&key.beta_g1), sizeof(pa_g1_affine));
        f.read(reinterpret_cast<char*>(&key.delta_g1), sizeof(pa_g1_affine));
        f.read(reinterpret_cast<char*>(&key.beta_g2), sizeof(pa_g2_affine));
        f.read(reinterpret_cast<char*>(&key.delta_g2), sizeof(pa_g2_affine));
        std::vector<pa_g1_affine> aq, b1q, lq, hq;
        std::vector<pa_g2_affine> b2q;
        read_rows(f, aq, n_vars);
        read_rows(f, b1q, n_vars);
        read_rows(f, b2q, n_vars);
        read_rows(f, lq, n_vars - n_public);
        read_rows(f, hq, h_len);
        key.n_vars = n_vars;
        key.n_public = n_public;
        key.a_query = aq.data();
        key.b_g1_query = b1q.data();
        key.b_g2_query = b2q.data();
        key.l_query = lq.data();
        key.h_query = hq.data();
        key.h_len = h_len;
        R1cs::Csr m[3];
        for (auto& x : m) {
            uint64_t nnz = 0;
            f.read(reinterpret_cast<char*>(&nnz), 8);
            std::vector<uint64_t> col64;
            read_rows(f, x.row_ptr, n_rows + 1);
            read_rows(f, col64, nnz);
            read_rows(f, x.val, nnz);
            x.col.assign(col64.begin(), col64.end());
        }
        std::vector<pa_fr> w, r, s, ea, eb, ec;
        std::vector<pa_groth16_proof> want;
        read_rows(f, w, k * n_vars);
        read_rows(f, r, k);
        read_rows(f, s, k);
        read_rows(f, ea, k << log_n);
        read_rows(f, eb, k << log_n);
        read_rows(f, ec, k << log_n);
        read_rows(f, want, k);

        const R1cs sysm(m[0], m[1], m[2], n_rows, n_vars);
        EXPECT(sysm.rows() == n_rows && sysm.cols() == n_vars);
        const R1cs::Evals e = sysm.eval(w, k, log_n);
        EXPECT(same(e.a, ea) && same(e.b, eb) && same(e.c, ec));
        std::printf("%s  R1cs::eval\n", g_failures ? "FAIL" : "ok  ");

        Groth16Prover prover(key, sysm, log_n);
        EXPECT(prover.in_subgroup());
        const std::vector<pa_groth16_proof> got = prover.prove(w, r, s, k);
        EXPECT(same(got, want));
        Groth16Prover moved(std::move(prover));
        EXPECT(prover.get() == nullptr && same(moved.prove(w, r, s, k), want));
        EXPECT(moved.prove({}, {}, {}, 0).empty());
        bool threw = false;
        try {
            (void)moved.prove(w, r, s, k + 1);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        EXPECT(threw);
        threw = false;
        try {
            m[0].row_ptr[0] = 1;   // refused by the library: PA_ERR_INVALID_ARGUMENT
            const R1cs bad(m[0], m[1], m[2], n_rows, n_vars);
        } catch (const std::exception&) {
            threw = true;
        }
        EXPECT(threw);
        std::printf("%s  Groth16Prover::prove\n", g_failures ? "FAIL" : "ok  ");
    } catch (const std::exception& e) {
        std::printf("FAIL  exception: %s\n", e.what());
        return 1;
    }
    return g_failures ? 1 : 0;
}
