// The fixed-base comb table of G1 (kernels_curve.hip builds it, launch_g1_comb_table): its
// shape and the step that adds one table entry, shared by the GLV multiply and
// the Groth16 verifier's public-input sum over several tables
// (kernels_groth16_verify.hip); k_g1_comb_mul keeps its own inlined copy of the
// same step.
#pragma once
#include "curve_fl.h"

namespace pa {

constexpr int kCombWindows = 33;      // 8-bit digits of a 255-bit scalar + final carry
constexpr int kCombEntries = 128;     // |d| in 1..128
constexpr int kG1Jac = Grp<1>::JW;    // u64 words per Jacobian G1
constexpr uint32_t kFlInfinity = 0xffffffffu;  // table entry marker: no lazy limb has all 32 bits set
constexpr int kFlPair = 14;           // u64 words per table entry: x, y as 14 x 28-bit limbs (lazy core)
// rows of the GLV form: 17 windows of each half (kernels_curve.hip); a table always has room for them
constexpr int kGlvWindows = 17;
constexpr int kTableRows = 2 * kGlvWindows;   // >= kCombWindows
static_assert(kTableRows >= kCombWindows, "table rows");

// acc += sign(d) T[row][|d|] (d != 0; `flip` negates once more)
PA_DEV void comb_add_entry(FlJac& acc, bool& untouched, bool& changed, const uint64_t* table_fl, int row, int d,
                           bool flip) {
    const int ad = d < 0 ? -d : d;
    const uint2* src = reinterpret_cast<const uint2*>(table_fl + (size_t)kFlPair * (row * kCombEntries + ad - 1));
    F<1> tx, ty;
#pragma unroll
    for (int k = 0; k < 7; k++) {
        const uint2 a = src[k], b = src[7 + k];
        tx.w[2 * k] = a.x;
        tx.w[2 * k + 1] = a.y;
        ty.w[2 * k] = b.x;
        ty.w[2 * k + 1] = b.y;
    }
    if (tx.w[0] != kFlInfinity) {  // adding the identity is add_assign_mixed's no-op
        const F<2> oy = ((d < 0) != flip) ? neg(ty) : relax<2>(ty);
        fl_jac_add_mixed(acc, untouched, tx, oy);
        changed = true;
    }
}

// acc = s T's base over the table's 33 comb rows (s: an FrRepr's four words, any value below 2^256): signed 8-bit
// digits, at most 33 mixed additions, no doubling.  `untouched` stays true when nothing was added (the result
// is the reference's zero()).
PA_DEV void comb_mul_repr(FlJac& acc, bool& untouched, const uint64_t* table_fl, const uint64_t (&s)[4]) {
    acc = FlJac::zero();
    untouched = true;
    bool changed = false;
    int carry = 0;
#pragma unroll 1
    for (int win = 0; win < kCombWindows; win++) {
        int d = carry;
        if (win < 32) d += (int)((s[win >> 3] >> (8 * (win & 7))) & 0xff);
        carry = d > 128 ? 1 : 0;
        if (d > 128) d -= 256;
        if (d != 0) comb_add_entry(acc, untouched, changed, table_fl, win, d, false);
    }
}

}  // namespace pa
