// pairing_amd::FrNttDomain (include/pairing_amd.hpp) against transforms the
// Python test computed with the oracle: fft / ifft / coset_fft / icoset_fft of
// `batch` polynomials, bit for bit, plus the wrapper's own rules (move-only
// ownership, a row count that is no multiple of the domain).
//   data file: u64 log_n, u64 batch, then five arrays of batch * 2^log_n rows
//   of 4 x u64: the input and its four transforms in the order above.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <utility>
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
    pairing_amd::FrNttDomain first((unsigned)log_n);
    pairing_amd::FrNttDomain dom(std::move(first));   // the moved-from object frees nothing
    expect(first.get() == nullptr && dom.get() != nullptr, "move construction");
    expect(dom.log_n() == log_n && dom.size() == (size_t)1 << log_n, "log_n / size");
    expect(same(dom.fft(v[0]), v[1]), "fft");
    expect(same(dom.ifft(v[0]), v[2]), "ifft");
    expect(same(dom.coset_fft(v[0]), v[3]), "coset_fft");
    expect(same(dom.icoset_fft(v[0]), v[4]), "icoset_fft");
    expect(same(dom.ifft(dom.fft(v[0])), v[0]), "ifft(fft(a)) == a");
    expect(dom.fft(std::vector<pa_fr>()).empty(), "empty batch");
    bool threw = false;
    try {
        (void)dom.fft(std::vector<pa_fr>(rows + 1));
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    expect(threw || log_n == 0, "rows that are no multiple of the domain");
    threw = false;
    try {
        pairing_amd::FrNttDomain too_big(PA_NTT_MAX_LOG_N + 1);
    } catch (const pairing_amd::Error&) {
        threw = true;
    }
    expect(threw, "log_n above the maximum");
    return failed ? 1 : 0;
}
