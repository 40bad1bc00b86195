// G2MsmBases (include/pairing_amd.hpp): prepare, multiexp and multiexp_batch
// in both scalar forms, against the C entry pa_g2_multiexp_prepared_batch and
// G2::multiexp over the same bases.
//
// usage: test_msm_g2 DATA_FILE OUT_FILE
// DATA_FILE: u64 m, u64 k, m pa_g2_affine records, k * m pa_fr_repr rows below r,
// the same k * m rows as Montgomery pa_fr.  OUT_FILE receives the k pa_g2
// results of the mirror's batch, then the pa_g2 of multiexp over the first
// vector, for the caller to compare with its own sums.
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

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s DATA_FILE OUT_FILE\n", argv[0]);
        return 2;
    }
    try {
        std::ifstream f(argv[1], std::ios::binary);
        uint64_t m = 0, k = 0;
        f.read(reinterpret_cast<char*>(&m), 8);
        f.read(reinterpret_cast<char*>(&k), 8);
        std::vector<G2Affine> bases;
        std::vector<FrRepr> s;
        std::vector<pa_fr> mont;
        read_rows(f, bases, m);
        read_rows(f, s, m * k);
        read_rows(f, mont, m * k);

        const G2MsmBases prepared(bases);
        EXPECT(prepared.size() == m && prepared.in_subgroup());
        const std::vector<G2> got = prepared.multiexp_batch(s, k);
        EXPECT(got.size() == k);

        // the C entry over the same rows: the same job, the same words
        std::vector<pa_g2> raw(k);
        EXPECT(pa_g2_multiexp_prepared_batch(prepared.get(), s.data(), m, k, PA_MSM_SCALARS_REPR, raw.data()) == PA_OK);
        for (size_t j = 0; j < k; j++) EXPECT(std::memcmp(&raw[j], &got[j].v, sizeof(pa_g2)) == 0);

        // each row is the single-vector multiexp's point
        for (size_t j = 0; j < k; j++) {
            const std::vector<FrRepr> one(s.begin() + (std::ptrdiff_t)(j * m), s.begin() + (std::ptrdiff_t)((j + 1) * m));
            EXPECT(got[j] == prepared.multiexp(one));
        }

        // the first vector: the plain multiexp's point, and a move keeps the object usable
        const std::vector<FrRepr> first(s.begin(), s.begin() + (std::ptrdiff_t)m);
        const G2 single = prepared.multiexp(first);
        EXPECT(single == G2::multiexp(bases, first));
        {
            G2MsmBases other(bases);
            G2MsmBases moved(std::move(other));
            EXPECT(other.get() == nullptr && moved.size() == m);
            EXPECT(moved.multiexp(first) == single);
        }

        // the Montgomery overload digests into the same scalars
        const std::vector<G2> gm = prepared.multiexp_batch(mont, k);
        EXPECT(gm.size() == k);
        for (size_t j = 0; j < k && j < gm.size(); j++) EXPECT(std::memcmp(&gm[j].v, &got[j].v, sizeof(pa_g2)) == 0);

        // no vectors: nothing; rows that are not k equal vectors: rejected by the mirror
        EXPECT(prepared.multiexp_batch(std::vector<FrRepr>(), 0).empty());
        bool threw = false;
        try {
            (void)prepared.multiexp_batch(std::vector<FrRepr>(s.begin(), s.begin() + 4), 3);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        EXPECT(threw);

        std::ofstream o(argv[2], std::ios::binary);
        o.write(reinterpret_cast<const char*>(got.data()), (std::streamsize)(sizeof(G2) * got.size()));
        o.write(reinterpret_cast<const char*>(&single), (std::streamsize)sizeof(G2));
        if (!o) throw std::runtime_error("cannot write the results");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    std::printf("%s G2MsmBases\n", g_failures ? "FAIL" : "ok  ");
    return g_failures ? 1 : 0;
}
