// Groth16Circuit and generate_parameters (include/pairing_amd.hpp): the named
// vectors of the result and its key() / vkey() views, compared word for word
// with what the caller expects.
//
// usage: test_groth16_setup DATA_FILE
// DATA_FILE, u64 unless said: n_rows, n_vars, n_public, log_n; for each of A, B,
// C: nnz, row_ptr (n_rows + 1), col (nnz u32), val (nnz pa_fr, Montgomery); g1
// (pa_g1_affine), g2 (pa_g2_affine); the trapdoor (5 pa_fr); expected g1_out
// (3 n_vars + 2^log_n + 2 pa_g1_affine), expected g2_out (n_vars + 3 pa_g2_affine).
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
static bool same(const T* a, const T* b, size_t n) {
    return n == 0 || std::memcmp(a, b, sizeof(T) * n) == 0;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s DATA_FILE\n", argv[0]);
        return 2;
    }
    try {
        static_assert(sizeof(pa_groth16_trapdoor) == 160, "five Fr rows");
        std::ifstream f(argv[1], std::ios::binary);
        uint64_t head[4];
        f.read(reinterpret_cast<char*>(head), sizeof head);
        const size_t n_rows = head[0], n_vars = head[1], n_public = head[2];
        const unsigned log_n = (unsigned)head[3];
        R1cs::Csr m[3];
        for (int i = 0; i < 3; i++) {
            std::vector<uint64_t> nnz;
            read_rows(f, nnz, 1);
            read_rows(f, m[i].row_ptr, n_rows + 1);
            read_rows(f, m[i].col, nnz[0]);
            read_rows(f, m[i].val, nnz[0]);
        }
        std::vector<pa_g1_affine> g1, want1;
        std::vector<pa_g2_affine> g2, want2;
        std::vector<pa_groth16_trapdoor> td;
        read_rows(f, g1, 1);
        read_rows(f, g2, 1);
        read_rows(f, td, 1);
        const pa_groth16_generate_layout o = pa_groth16_generate_offsets(n_vars, n_public, log_n);
        EXPECT(o.g1_len == 3 * n_vars + ((size_t)1 << log_n) + 2 && o.g2_len == n_vars + 3);
        read_rows(f, want1, o.g1_len);
        read_rows(f, want2, o.g2_len);

        Groth16Circuit circuit(m[0], m[1], m[2], n_rows, n_vars, n_public);
        EXPECT(circuit.rows() == n_rows && circuit.cols() == n_vars && circuit.n_public() == n_public);
        Groth16Circuit moved(std::move(circuit));
        EXPECT(circuit.get() == nullptr && moved.cols() == n_vars);
        FrNttDomain domain(log_n);
        const Groth16Params p = generate_parameters(moved, domain, g1[0], g2[0], td[0]);
        EXPECT(p.a_query.size() == n_vars && same(p.a_query.data(), &want1[o.a_query], n_vars));
        EXPECT(p.b_g1_query.size() == n_vars && same(p.b_g1_query.data(), &want1[o.b_g1_query], n_vars));
        EXPECT(p.ic.size() == n_public && same(p.ic.data(), &want1[o.ic], n_public));
        EXPECT(p.l_query.size() == n_vars - n_public && same(p.l_query.data(), &want1[o.l_query], n_vars - n_public));
        EXPECT(p.h_query.size() == o.h_len && same(p.h_query.data(), &want1[o.h_query], o.h_len));
        EXPECT(same(&p.alpha_g1, &want1[o.alpha_g1], 1) && same(&p.beta_g1, &want1[o.beta_g1], 1) &&
               same(&p.delta_g1, &want1[o.delta_g1], 1));
        EXPECT(p.b_g2_query.size() == n_vars && same(p.b_g2_query.data(), &want2[o.b_g2_query], n_vars));
        EXPECT(same(&p.beta_g2, &want2[o.beta_g2], 1) && same(&p.gamma_g2, &want2[o.gamma_g2], 1) &&
               same(&p.delta_g2, &want2[o.delta_g2], 1));
        std::printf("%s  generate_parameters\n", g_failures ? "FAIL" : "ok  ");

        const pa_groth16_key k = p.key();
        EXPECT(k.n_vars == n_vars && k.n_public == n_public && k.h_len == o.h_len);
        EXPECT(k.a_query == p.a_query.data() && k.b_g1_query == p.b_g1_query.data() &&
               k.b_g2_query == p.b_g2_query.data() && k.l_query == p.l_query.data() && k.h_query == p.h_query.data());
        EXPECT(same(&k.alpha_g1, &want1[o.alpha_g1], 1) && same(&k.beta_g1, &want1[o.beta_g1], 1) &&
               same(&k.delta_g1, &want1[o.delta_g1], 1) && same(&k.beta_g2, &want2[o.beta_g2], 1) &&
               same(&k.delta_g2, &want2[o.delta_g2], 1));
        const pa_groth16_vkey v = p.vkey();
        EXPECT(v.n_public == n_public && v.ic == p.ic.data());
        EXPECT(same(&v.alpha_g1, &want1[o.alpha_g1], 1) && same(&v.beta_g2, &want2[o.beta_g2], 1) &&
               same(&v.gamma_g2, &want2[o.gamma_g2], 1) && same(&v.delta_g2, &want2[o.delta_g2], 1));
        // the views are what the prover and the verifier take
        R1cs system(m[0], m[1], m[2], n_rows, n_vars);
        const Groth16Prover prover(k, system, log_n);
        const Groth16Verifier verifier_(v);
        EXPECT(prover.in_subgroup() && verifier_.n_public() == n_public);
        std::printf("%s  Groth16Params::key / vkey\n", g_failures ? "FAIL" : "ok  ");

        bool threw = false;
        try {
            pa_groth16_trapdoor bad = td[0];
            std::memset(&bad.delta, 0, sizeof bad.delta);   // refused by the library: PA_ERR_INVALID_ARGUMENT
            (void)generate_parameters(moved, domain, g1[0], g2[0], bad);
        } catch (const std::exception&) {
            threw = true;
        }
        EXPECT(threw);
        threw = false;
        try {
            const Groth16Circuit bad(m[0], m[1], m[2], n_rows, n_vars, n_vars + 1);
        } catch (const std::exception&) {
            threw = true;
        }
        EXPECT(threw);
        std::printf("%s  errors\n", g_failures ? "FAIL" : "ok  ");
    } catch (const std::exception& e) {
        std::printf("FAIL  exception: %s\n", e.what());
        return 1;
    }
    return g_failures ? 1 : 0;
}
