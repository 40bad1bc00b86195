// Groth16Verifier (include/pairing_amd.hpp): k proofs through verify(),
// verify_encoded() and input_sum(), compared word for word with what the caller
// expects.
//
// usage: test_groth16_verify DATA_FILE
// DATA_FILE, u64 unless said: n_public, k; alpha_g1 (pa_g1_affine), beta_g2,
// gamma_g2, delta_g2 (pa_g2_affine); ic (n_public pa_g1_affine); proofs (k
// pa_groth16_proof); inputs (k (n_public - 1) pa_fr, Montgomery); expected gt (k
// pa_fq12); expected sums (k pa_g1_affine); then bytes: expected valid (k), the
// encoded proofs (192 k), expected status (3 k).
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
        static_assert(sizeof(pa_groth16_vkey) == sizeof(pa_g1_affine) + 3 * sizeof(pa_g2_affine) + 16, "key layout");
        static_assert(PA_GROTH16_ENCODED_PROOF_BYTES == 192, "A, B and C compressed");
        std::ifstream f(argv[1], std::ios::binary);
        uint64_t head[2];
        f.read(reinterpret_cast<char*>(head), sizeof head);
        const size_t n_public = head[0], k = head[1];
        pa_groth16_vkey key;
        std::memset(&key, 0, sizeof key);
        f.read(reinterpret_cast<char*>(&key.alpha_g1), sizeof(pa_g1_affine));
        f.read(reinterpret_cast<char*>(&key.beta_g2), sizeof(pa_g2_affine));
        f.read(reinterpret_cast<char*>(&key.gamma_g2), sizeof(pa_g2_affine));
        f.read(reinterpret_cast<char*>(&key.delta_g2), sizeof(pa_g2_affine));
        std::vector<pa_g1_affine> ic, want_sums;
        std::vector<pa_groth16_proof> proofs;
        std::vector<pa_fr> inputs;
        std::vector<pa_fq12> want_gt;
        std::vector<uint8_t> want_valid, enc, want_status;
        read_rows(f, ic, n_public);
        read_rows(f, proofs, k);
        read_rows(f, inputs, k * (n_public - 1));
        read_rows(f, want_gt, k);
        read_rows(f, want_sums, k);
        read_rows(f, want_valid, k);
        read_rows(f, enc, k * PA_GROTH16_ENCODED_PROOF_BYTES);
        read_rows(f, want_status, 3 * k);
        key.ic = ic.data();
        key.n_public = n_public;

        Groth16Verifier v = verifier(key);
        EXPECT(v.n_public() == n_public && v.n_inputs() == n_public - 1);
        EXPECT(same(v.input_sum(inputs, k), want_sums));
        std::printf("%s  Groth16Verifier::input_sum\n", g_failures ? "FAIL" : "ok  ");

        std::vector<pa_fq12> gt;
        EXPECT(same(v.verify(proofs, inputs, k, true, &gt), want_valid));
        EXPECT(same(gt, want_gt));
        Groth16Verifier moved(std::move(v));
        EXPECT(v.get() == nullptr && same(moved.verify(proofs, inputs, k), want_valid));
        EXPECT(moved.verify({}, {}, 0).empty());
        bool threw = false;
        try {
            (void)moved.verify(proofs, inputs, k + 1);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        EXPECT(threw);
        std::printf("%s  Groth16Verifier::verify\n", g_failures ? "FAIL" : "ok  ");

        gt.clear();
        const Groth16Verifier::EncodedResult r = moved.verify_encoded(enc, inputs, k, true, &gt);
        EXPECT(same(r.status, want_status));
        for (size_t j = 0; j < k; j++) {
            const bool decoded = !r.status[3 * j] && !r.status[3 * j + 1] && !r.status[3 * j + 2];
            EXPECT(r.valid[j] == (decoded ? want_valid[j] : 0));
            if (decoded) EXPECT(std::memcmp(&gt[j], &want_gt[j], sizeof(pa_fq12)) == 0);
        }
        threw = false;
        try {
            key.n_public = 0;   // refused by the library: PA_ERR_INVALID_ARGUMENT
            const Groth16Verifier bad(key);
        } catch (const std::exception&) {
            threw = true;
        }
        EXPECT(threw);
        std::printf("%s  Groth16Verifier::verify_encoded\n", g_failures ? "FAIL" : "ok  ");
    } catch (const std::exception& e) {
        std::printf("FAIL  exception: %s\n", e.what());
        return 1;
    }
    return g_failures ? 1 : 0;
}
