// The G1 endomorphism's scalar split, shared by the fixed-base GLV comb
// (kernels_curve.hip, k_g1_glv_mul) and the MSM over prepared bases
// (kernels_msm.hip, k_msm_digits_glv).
//
// phi(x, y) = (beta x, y) acts on G1 as multiplication by -x^2 (x the BLS
// parameter), so with s = q x^2 + rem as integers, for any 256-bit s,
//   s P = rem P + q (x^2 P) = rem P + q psi(P),  psi(x, y) = (beta x, -y).
#pragma once
#include "fq.h"

namespace pa {

constexpr uint64_t kGlvX2Lo = 0x0000000100000000ull, kGlvX2Hi = 0xac45a4010001a402ull;   // x^2 = 0xd201000000010000^2
// the Barrett constant m = floor(2^256 / x^2), little-endian words
constexpr uint64_t kGlvBarrett[3] = {0x63f6e522f6cfee2eull, 0x7c6becf1e01faaddull, 1};

// s = q x^2 + rem for a 256-bit s (Barrett, HAC 14.42 without the final
// corrections): q = floor(floor(s / 2^127) m / 2^129), m = floor(2^256 / x^2),
// never above floor(s / x^2), so rem = s - q x^2 is in [0, 2 x^2) < 2^129
// (one correction short at most) and q < 2^129: 17 signed base-256 digits
// each, or ceil(130 / c) signed c-bit digits (the spare bit 129 takes the
// last carry).
PA_DEV void glv_split(const uint64_t s[4], uint64_t rem[3], uint64_t q[3]) {
    constexpr uint64_t m[3] = {kGlvBarrett[0], kGlvBarrett[1], kGlvBarrett[2]};
    const uint64_t t[3] = {(s[1] >> 63) | (s[2] << 1), (s[2] >> 63) | (s[3] << 1), s[3] >> 63};
    uint64_t pr[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const unsigned __int128 v = (unsigned __int128)t[i] * m[j] + pr[i + j] + c;
            pr[i + j] = (uint64_t)v;
            c = (uint64_t)(v >> 64);
        }
        pr[i + 3] = c;
    }
    q[0] = (pr[2] >> 1) | (pr[3] << 63);
    q[1] = (pr[3] >> 1) | (pr[4] << 63);
    q[2] = (pr[4] >> 1) | (pr[5] << 63);
    // q x^2 mod 2^192
    const unsigned __int128 a0 = (unsigned __int128)q[0] * kGlvX2Lo;
    const unsigned __int128 a1 = (unsigned __int128)q[0] * kGlvX2Hi + (uint64_t)(a0 >> 64);
    const unsigned __int128 b1 = (unsigned __int128)q[1] * kGlvX2Lo + (uint64_t)a1;
    const uint64_t w0 = (uint64_t)a0, w1 = (uint64_t)b1;
    const uint64_t w2 = (uint64_t)(a1 >> 64) + (uint64_t)(b1 >> 64) + q[1] * kGlvX2Hi + q[2] * kGlvX2Lo;
    unsigned __int128 d = (unsigned __int128)s[0] - w0;
    rem[0] = (uint64_t)d;
    d = (unsigned __int128)s[1] - w1 - (uint64_t)((d >> 64) & 1);
    rem[1] = (uint64_t)d;
    rem[2] = s[2] - w2 - (uint64_t)((d >> 64) & 1);
}

}  // namespace pa
