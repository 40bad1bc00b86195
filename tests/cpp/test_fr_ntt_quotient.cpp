// pairing_amd::FrNttDomain::quotient (include/pairing_amd.hpp) against the
// quotient the Python test computed with the oracle, bit for bit, plus the
// wrapper's own rules (lengths that differ, a row count that is no multiple of
// the domain, an empty batch) and the composition of the wrapper's transforms.
//   data file: u64 log_n, u64 batch, then five arrays of batch * 2^log_n rows
//   of 4 x u64: a, b, c, the quotient h, and (g^n - 1)^-1 repeated in every row.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <vector>

#include "pairing_amd.hpp"

static bool same(const std::vector<pa_fr>& a, const std::vector<pa_fr>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(pa_fr)) == 0);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    uint64_t log_n = 0, batch = 0;
    f.read(reinterpret_cast<char*>(&log_n), 8);
    f.read(reinterpret_cast<char*>(&batch), 8);
    const size_t rows = (size_t)batch << log_n;
    std::vector<pa_fr> v[5];
    for (auto& a : v) {
        a.resize(rows);
        f.read(reinterpret_cast<char*>(a.data()), rows * sizeof(pa_fr));
    }
    if (!f) return 2;
    int failed = 0;
    auto expect = [&](bool ok, const char* what) {
        std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
        if (!ok) failed++;
    };
    pairing_amd::FrNttDomain dom((unsigned)log_n);
    const std::vector<pa_fr> h = dom.quotient(v[0], v[1], v[2]);
    expect(same(h, v[3]), "quotient");
    expect(h.size() == rows, "rows of the result");
    // the same from the wrapper's transforms and the C entries for the pointwise step
    {
        const std::vector<pa_fr> ea = dom.coset_fft(dom.ifft(v[0])), eb = dom.coset_fft(dom.ifft(v[1])),
                                 ec = dom.coset_fft(dom.ifft(v[2]));
        std::vector<pa_fr> t(rows);
        bool ok = pa_fr_mul_batch(ea.data(), eb.data(), t.data(), rows) == 0 &&
                  pa_fr_sub_batch(t.data(), ec.data(), t.data(), rows) == 0 &&
                  pa_fr_mul_batch(t.data(), v[4].data(), t.data(), rows) == 0;
        expect(ok && same(dom.icoset_fft(t), h), "equals the composition of the transforms");
    }
    expect(dom.quotient(std::vector<pa_fr>(), std::vector<pa_fr>(), std::vector<pa_fr>()).empty(), "empty batch");
    bool threw = false;
    try {
        (void)dom.quotient(v[0], std::vector<pa_fr>(rows - 1), v[2]);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    expect(threw, "lengths that differ");
    threw = false;
    try {
        const std::vector<pa_fr> odd(rows + 1);
        (void)dom.quotient(odd, odd, odd);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    expect(threw || log_n == 0, "rows that are no multiple of the domain");
    return failed ? 1 : 0;
}
