// Groth16Verifier's aggregate check (include/pairing_amd.hpp): k proofs through
// verify_aggregate(), aggregate_points() and verify_aggregate_encoded(), and
// g1_multiexp_u128(), compared word for word with what the caller expects.
//
// usage: test_groth16_aggregate DATA_FILE
// DATA_FILE, u64 unless said: n_public, k; alpha_g1 (pa_g1_affine), beta_g2,
// gamma_g2, delta_g2 (pa_g2_affine); ic (n_public pa_g1_affine); two batches of
// proofs (k pa_groth16_proof each: all valid, one spoiled); inputs (k
// (n_public - 1) pa_fr, Montgomery); z (2 k); the spoiled batch's expected gt (1
// pa_fq12) and points (k + 3 pa_g1_affine); then bytes: the valid batch encoded
// with one record spoiled on the wire (192 k), expected status (3 k).
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
        std::vector<pa_g1_affine> ic, want_points;
        std::vector<pa_groth16_proof> good, bad;
        std::vector<pa_fr> inputs;
        std::vector<uint64_t> z;
        std::vector<pa_fq12> want_gt;
        std::vector<uint8_t> enc, want_status;
        read_rows(f, ic, n_public);
        read_rows(f, good, k);
        read_rows(f, bad, k);
        read_rows(f, inputs, k * (n_public - 1));
        read_rows(f, z, 2 * k);
        read_rows(f, want_gt, 1);
        read_rows(f, want_points, k + 3);
        read_rows(f, enc, k * PA_GROTH16_ENCODED_PROOF_BYTES);
        read_rows(f, want_status, 3 * k);
        key.ic = ic.data();
        key.n_public = n_public;

        const Groth16Verifier v = verifier(key);
        pa_fq12 gt, one;
        std::memset(&one, 0, sizeof one);
        EXPECT(v.verify_aggregate({}, {}, {}, 0, true, &one));   // the empty product
        EXPECT(v.verify_aggregate(good, inputs, z, k, true, &gt));
        EXPECT(std::memcmp(&gt, &one, sizeof gt) == 0);
        EXPECT(!v.verify_aggregate(bad, inputs, z, k, true, &gt));
        EXPECT(std::memcmp(&gt, want_gt.data(), sizeof gt) == 0);
        EXPECT(!v.verify_aggregate(bad, inputs, z, k));
        bool threw = false;
        try {
            (void)v.verify_aggregate(good, inputs, std::vector<uint64_t>(2 * k + 1), k);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        EXPECT(threw);
        std::printf("%s  Groth16Verifier::verify_aggregate\n", g_failures ? "FAIL" : "ok  ");

        EXPECT(same(v.aggregate_points(bad, inputs, z, k), want_points));
        std::vector<pa_g1_affine> c(k);
        for (size_t j = 0; j < k; j++) c[j] = bad[j].c;
        const pa_g1 sum = g1_multiexp_u128(c, z);
        pa_g1_affine aff;
        check(pa_g1_into_affine_batch(&sum, &aff, 1), "into_affine");
        aff.infinity = aff.infinity ? 1 : 0;
        EXPECT(std::memcmp(&aff, &want_points[k + 1], sizeof(pa_fq) * 2) == 0 &&
               aff.infinity == want_points[k + 1].infinity);
        std::printf("%s  Groth16Verifier::aggregate_points\n", g_failures ? "FAIL" : "ok  ");

        const Groth16Verifier::AggregateEncodedResult r = v.verify_aggregate_encoded(enc, inputs, z, k);
        EXPECT(!r.valid && same(r.status, want_status));
        std::printf("%s  Groth16Verifier::verify_aggregate_encoded\n", g_failures ? "FAIL" : "ok  ");
    } catch (const std::exception& e) {
        std::printf("FAIL  exception: %s\n", e.what());
        return 1;
    }
    return g_failures ? 1 : 0;
}
