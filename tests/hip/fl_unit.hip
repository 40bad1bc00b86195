// Test-only code object (built into pairing_amd/lib/test/fl_unit.hsaco, never
// loaded by the product): the hand-written lazy layer -- fl.h, tower_fl.h,
// curve_fl.h, curve_fl2.h, pairing_fl.h -- one routine per launch, one case
// per lane, on RAW operands (no fl_load), so that limb-maximal, value-maximal
// and non-canonical operands reach every routine (tests/test_fl_unit.py).
//   in  [case][24][16] u32: operand slots, 14 limbs + 2 pads each
//   out [case][16][16] u32: result slots: 14 limbs, pad 14 = the static bound U
//                           of the result TYPE (bound_of), pad 15 = a flag
//                           (ok / is_zero / untouched) where the op has one;
//                           an ABI result is 12 words + 4 zero pads
// `op` picks the routine and `p` its instantiation (bounds) or runtime
// argument (Frobenius power); both are launch-uniform.  An (op, p) the switch
// does not know leaves the output untouched (bound 0), which the test rejects.
#include "../../pairing_amd/csrc/pairing_fl.h"
#include "../../pairing_amd/csrc/curve_fl2.h"

using namespace pa;

namespace {

constexpr int IN_WORDS = 24 * 16, OUT_WORDS = 16 * 16;

template <int U>
constexpr uint32_t bound_of(const F<U>&) { return U; }

template <int U>
PA_DEV F<U> ld(const uint32_t* x, int s) {
    F<U> r;
    for (int i = 0; i < 14; i++) r.w[i] = x[16 * s + i];
    return r;
}
template <int U>
PA_DEV F2<U> ld2(const uint32_t* x, int s) { return {ld<U>(x, s), ld<U>(x, s + 1)}; }
template <int U>
PA_DEV F6<U> ld6(const uint32_t* x, int s) { return {ld2<U>(x, s), ld2<U>(x, s + 2), ld2<U>(x, s + 4)}; }
template <int U>
PA_DEV F12<U> ld12(const uint32_t* x, int s) { return {ld6<U>(x, s), ld6<U>(x, s + 6)}; }

template <int U>
PA_DEV void st(uint32_t* y, int s, const F<U>& v, uint32_t flag = 0) {
    for (int i = 0; i < 14; i++) y[16 * s + i] = v.w[i];
    y[16 * s + 14] = bound_of(v);
    y[16 * s + 15] = flag;
}
template <int U>
PA_DEV void st2(uint32_t* y, int s, const F2<U>& v, uint32_t flag = 0) {
    st(y, s, v.c0, flag);
    st(y, s + 1, v.c1, flag);
}
template <int U>
PA_DEV void st6(uint32_t* y, int s, const F6<U>& v, uint32_t flag = 0) {
    st2(y, s, v.c0, flag);
    st2(y, s + 2, v.c1, flag);
    st2(y, s + 4, v.c2, flag);
}
template <int U>
PA_DEV void st12(uint32_t* y, int s, const F12<U>& v, uint32_t flag = 0) {
    st6(y, s, v.c0, flag);
    st6(y, s + 6, v.c1, flag);
}
PA_DEV void st_abi(uint32_t* y, int s, const Fq& v) {
    for (int j = 0; j < 12; j++) y[16 * s + j] = v.w[j];
    for (int j = 12; j < 16; j++) y[16 * s + j] = 0;
}
PA_DEV Fq ld_abi(const uint32_t* x, int s) {
    Fq r;
    for (int j = 0; j < 12; j++) r.w[j] = x[16 * s + j];
    return r;
}

}  // namespace

#define CASE(P, ...) case P: { __VA_ARGS__; } break

// ---------------------------------------------------------------- fl.h ----
//  op 0 add   p: 0 (1,1)  1 (8,8)  2 (15,1)  3 (3,4)            a, b -> r
//     1 dbl   p = A in {1, 8}
//     2 sub<1, B>              p = B in 1..12
//     3 sub<16 - subcu(B), B>  p = B in 1..12   (result bound exactly 16)
//     4 neg<B>                 p = B in 1..13
//     5 red<U>                 p = U in {1, 2, 3, 4, 6, 8, 12, 16}
//     6 mul   p: 0 (1,1)  1 (1,16)  2 (16,1)  3 (4,4)  4 (2,8)
//     7 sqr<A>                 p = A in 1..3
//     8 sop   p: 0 (1,1,1,1)  1 (4,4,1,1)  2 (8,2,1,1)  3 (3,3,2,4)   a, b, c, d
//     9 fl_canon
//    10 fl_split (in: 12 words) -> slot 0, fl_pack of that -> slot 1 (words)
//    11 fl_pack_canon -> words
//    12 fl_from_abi (in: 12 words)
//    13 fl_to_abi<U>  -> words       p = U as op 5
//    14 fl_is_zero<U> -> flag        p = U as op 5
//    15 fl_store<U>   -> 6 u64       p = U as op 5
//    16 fl_inv -> r, flag = ok
//    17 fl_pack (in: raw F<1> limbs) -> words
extern "C" __global__ void __launch_bounds__(64) fl_unit_base(const uint32_t* __restrict__ in,
                                                              uint32_t* __restrict__ out, uint32_t n, uint32_t op,
                                                              uint32_t p) {
    const uint32_t item = blockIdx.x * 64 + threadIdx.x;
    if (item >= n) return;
    const uint32_t* x = in + (size_t)item * IN_WORDS;
    uint32_t* y = out + (size_t)item * OUT_WORDS;
#define SUB1(B) CASE(B, st(y, 0, sub(ld<1>(x, 0), ld<B>(x, 1))))
#define SUBX(B) CASE(B, st(y, 0, sub(ld<16 - subcu(B)>(x, 0), ld<B>(x, 1))))
#define NEG(B) CASE(B, st(y, 0, neg(ld<B>(x, 0))))
#define RED(U) CASE(U, st(y, 0, red(ld<U>(x, 0))))
#define TOABI(U) CASE(U, st_abi(y, 0, fl_to_abi(ld<U>(x, 0))))
#define ISZERO(U) CASE(U, st(y, 0, ld<U>(x, 0), fl_is_zero(ld<U>(x, 0)) ? 1u : 0u))
#define STORE(U) CASE(U, fl_store(reinterpret_cast<uint64_t*>(y), ld<U>(x, 0)); for (int j = 12; j < 16; j++) y[j] = 0)
    switch (op) {
        case 0:
            switch (p) {
                CASE(0, st(y, 0, add(ld<1>(x, 0), ld<1>(x, 1))));
                CASE(1, st(y, 0, add(ld<8>(x, 0), ld<8>(x, 1))));
                CASE(2, st(y, 0, add(ld<15>(x, 0), ld<1>(x, 1))));
                CASE(3, st(y, 0, add(ld<3>(x, 0), ld<4>(x, 1))));
            }
            break;
        case 1:
            switch (p) {
                CASE(1, st(y, 0, dbl(ld<1>(x, 0))));
                CASE(8, st(y, 0, dbl(ld<8>(x, 0))));
            }
            break;
        case 2:
            switch (p) { SUB1(1); SUB1(2); SUB1(3); SUB1(4); SUB1(5); SUB1(6); SUB1(7); SUB1(8); SUB1(9); SUB1(10); SUB1(11); SUB1(12); }
            break;
        case 3:
            switch (p) { SUBX(1); SUBX(2); SUBX(3); SUBX(4); SUBX(5); SUBX(6); SUBX(7); SUBX(8); SUBX(9); SUBX(10); SUBX(11); SUBX(12); }
            break;
        case 4:
            switch (p) { NEG(1); NEG(2); NEG(3); NEG(4); NEG(5); NEG(6); NEG(7); NEG(8); NEG(9); NEG(10); NEG(11); NEG(12); NEG(13); }
            break;
        case 5:
            switch (p) { RED(1); RED(2); RED(3); RED(4); RED(6); RED(8); RED(12); RED(16); }
            break;
        case 6:
            switch (p) {
                CASE(0, st(y, 0, mul(ld<1>(x, 0), ld<1>(x, 1))));
                CASE(1, st(y, 0, mul(ld<1>(x, 0), ld<16>(x, 1))));
                CASE(2, st(y, 0, mul(ld<16>(x, 0), ld<1>(x, 1))));
                CASE(3, st(y, 0, mul(ld<4>(x, 0), ld<4>(x, 1))));
                CASE(4, st(y, 0, mul(ld<2>(x, 0), ld<8>(x, 1))));
            }
            break;
        case 7:
            switch (p) {
                CASE(1, st(y, 0, sqr(ld<1>(x, 0))));
                CASE(2, st(y, 0, sqr(ld<2>(x, 0))));
                CASE(3, st(y, 0, sqr(ld<3>(x, 0))));
            }
            break;
        case 8:
            switch (p) {
                CASE(0, st(y, 0, sop(ld<1>(x, 0), ld<1>(x, 1), ld<1>(x, 2), ld<1>(x, 3))));
                CASE(1, st(y, 0, sop(ld<4>(x, 0), ld<4>(x, 1), ld<1>(x, 2), ld<1>(x, 3))));
                CASE(2, st(y, 0, sop(ld<8>(x, 0), ld<2>(x, 1), ld<1>(x, 2), ld<1>(x, 3))));
                CASE(3, st(y, 0, sop(ld<3>(x, 0), ld<3>(x, 1), ld<2>(x, 2), ld<4>(x, 3))));
            }
            break;
        case 9:
            st(y, 0, fl_canon(ld<1>(x, 0)));
            break;
        case 10: {
            const F<1> s = fl_split(ld_abi(x, 0));
            st(y, 0, s);
            st_abi(y, 1, fl_pack(s));
        } break;
        case 11:
            st_abi(y, 0, fl_pack_canon(ld<1>(x, 0)));
            break;
        case 12:
            st(y, 0, fl_from_abi(ld_abi(x, 0)));
            break;
        case 13:
            switch (p) { TOABI(1); TOABI(2); TOABI(3); TOABI(4); TOABI(6); TOABI(8); TOABI(12); TOABI(16); }
            break;
        case 14:
            switch (p) { ISZERO(1); ISZERO(2); ISZERO(3); ISZERO(4); ISZERO(6); ISZERO(8); ISZERO(12); ISZERO(16); }
            break;
        case 15:
            switch (p) { STORE(1); STORE(2); STORE(3); STORE(4); STORE(6); STORE(8); STORE(12); STORE(16); }
            break;
        case 16: {
            bool ok;
            const F<1> r = fl_inv(ld<1>(x, 0), ok);
            st(y, 0, r, ok ? 1u : 0u);
        } break;
        case 17:
            st_abi(y, 0, fl_pack(ld<1>(x, 0)));
            break;
    }
}

// ----------------------------------------------------------- tower_fl.h ----
//  Fq2 = 2 slots (c0, c1), Fq6 = 6, Fq12 = 12, operands back to back.
//  op 0 F2 mul  p: 0 (1,1) 1 (1,2) 2 (2,1) 3 (2,2) 4 (4,1) 5 (1,4) 6 (3,1)   (both neg branches)
//     1 F2 sqr<A>       p = A in {1, 2}   (mul form, sop form)
//     2 mul_xi<U>       p = U in {1, 2, 4}
//     3 F2 conj<U>      p = U in {1, 2}
//     4 mul_by_fq       p: 0 (1,1)  1 (4,4)        a (2 slots), b (1 slot)
//     5 F6 mul          p: 0 (1,1) 1 (1,2) 2 (2,1) 3 (2,2)
//     6 mul_by_1        p: 0 (1,1) 1 (1,2)         a, c1
//     7 mul_by_01       p: 0 (1,1,1) 1 (1,1,2)     a, c0, c1
//     8 mul_v<U>        p = U in {1, 2}
//     9 F6 frobenius    p = power
//    10 F12 mul   11 F12 sqr   12 mul_by_014 (a, c0, c1, c4)   13 F12 frobenius (p = power)
//    14 F12 conj  15 fq4_sqr (a, b -> r0, r1)   16 cyclotomic_sqr
//    17 F2 inverse  18 F6 inverse  19 F12 inverse   (flag = ok)
extern "C" __global__ void __launch_bounds__(64) fl_unit_tower(const uint32_t* __restrict__ in,
                                                               uint32_t* __restrict__ out, uint32_t n, uint32_t op,
                                                               uint32_t p) {
    const uint32_t item = blockIdx.x * 64 + threadIdx.x;
    if (item >= n) return;
    const uint32_t* x = in + (size_t)item * IN_WORDS;
    uint32_t* y = out + (size_t)item * OUT_WORDS;
    switch (op) {
        case 0:
            switch (p) {
                CASE(0, st2(y, 0, mul(ld2<1>(x, 0), ld2<1>(x, 2))));
                CASE(1, st2(y, 0, mul(ld2<1>(x, 0), ld2<2>(x, 2))));
                CASE(2, st2(y, 0, mul(ld2<2>(x, 0), ld2<1>(x, 2))));
                CASE(3, st2(y, 0, mul(ld2<2>(x, 0), ld2<2>(x, 2))));
                CASE(4, st2(y, 0, mul(ld2<4>(x, 0), ld2<1>(x, 2))));
                CASE(5, st2(y, 0, mul(ld2<1>(x, 0), ld2<4>(x, 2))));
                CASE(6, st2(y, 0, mul(ld2<3>(x, 0), ld2<1>(x, 2))));
            }
            break;
        case 1:
            switch (p) {
                CASE(1, st2(y, 0, sqr(ld2<1>(x, 0))));
                CASE(2, st2(y, 0, sqr(ld2<2>(x, 0))));
            }
            break;
        case 2:
            switch (p) {
                CASE(1, st2(y, 0, mul_xi(ld2<1>(x, 0))));
                CASE(2, st2(y, 0, mul_xi(ld2<2>(x, 0))));
                CASE(4, st2(y, 0, mul_xi(ld2<4>(x, 0))));
            }
            break;
        case 3:
            switch (p) {
                CASE(1, st2(y, 0, conj(ld2<1>(x, 0))));
                CASE(2, st2(y, 0, conj(ld2<2>(x, 0))));
            }
            break;
        case 4:
            switch (p) {
                CASE(0, st2(y, 0, mul_by_fq(ld2<1>(x, 0), ld<1>(x, 2))));
                CASE(1, st2(y, 0, mul_by_fq(ld2<4>(x, 0), ld<4>(x, 2))));
            }
            break;
        case 5:
            switch (p) {
                CASE(0, st6(y, 0, mul(ld6<1>(x, 0), ld6<1>(x, 6))));
                CASE(1, st6(y, 0, mul(ld6<1>(x, 0), ld6<2>(x, 6))));
                CASE(2, st6(y, 0, mul(ld6<2>(x, 0), ld6<1>(x, 6))));
                CASE(3, st6(y, 0, mul(ld6<2>(x, 0), ld6<2>(x, 6))));
            }
            break;
        case 6:
            switch (p) {
                CASE(0, st6(y, 0, mul_by_1(ld6<1>(x, 0), ld2<1>(x, 6))));
                CASE(1, st6(y, 0, mul_by_1(ld6<1>(x, 0), ld2<2>(x, 6))));
            }
            break;
        case 7:
            switch (p) {
                CASE(0, st6(y, 0, mul_by_01(ld6<1>(x, 0), ld2<1>(x, 6), ld2<1>(x, 8))));
                CASE(1, st6(y, 0, mul_by_01(ld6<1>(x, 0), ld2<1>(x, 6), ld2<2>(x, 8))));
            }
            break;
        case 8:
            switch (p) {
                CASE(1, st6(y, 0, mul_v(ld6<1>(x, 0))));
                CASE(2, st6(y, 0, mul_v(ld6<2>(x, 0))));
            }
            break;
        case 9:
            st6(y, 0, frobenius(ld6<1>(x, 0), (int)p));
            break;
        case 10:
            st12(y, 0, mul(ld12<1>(x, 0), ld12<1>(x, 12)));
            break;
        case 11:
            st12(y, 0, sqr(ld12<1>(x, 0)));
            break;
        case 12:
            st12(y, 0, mul_by_014(ld12<1>(x, 0), ld2<1>(x, 12), ld2<1>(x, 14), ld2<1>(x, 16)));
            break;
        case 13:
            st12(y, 0, frobenius(ld12<1>(x, 0), (int)p));
            break;
        case 14:
            st12(y, 0, conj(ld12<1>(x, 0)));
            break;
        case 15: {
            F2<1> r0, r1;
            fq4_sqr(r0, r1, ld2<1>(x, 0), ld2<1>(x, 2));
            st2(y, 0, r0);
            st2(y, 2, r1);
        } break;
        case 16:
            st12(y, 0, cyclotomic_sqr(ld12<1>(x, 0)));
            break;
        case 17: {
            bool ok;
            const F2<1> r = inverse(ld2<1>(x, 0), ok);
            st2(y, 0, r, ok ? 1u : 0u);
        } break;
        case 18: {
            bool ok;
            const F6<1> r = inverse(ld6<1>(x, 0), ok);
            st6(y, 0, r, ok ? 1u : 0u);
        } break;
        case 19: {
            bool ok;
            const F12<1> r = inverse(ld12<1>(x, 0), ok);
            st12(y, 0, r, ok ? 1u : 0u);
        } break;
    }
}

// ------------------------------------------------ curve_fl.h, curve_fl2.h ----
//  op 0 fl_jac_double      s (3 slots)
//     1 fl_jac_add_mixed   s, ox (F<1>), oy (F<2>), word 0 of slot 5 = untouched; flag = untouched after
//     2 fl_jac_add         s, o
//     3 fl_jac_double      s (6 slots), over Fq2
//     4 fl_jac_add_mixed   s, ox (2 slots), oy (F2<2>), word 0 of slot 10 = untouched
//     5 fl_jac_add         s, o
//  (the quad forms fl_jac_add_q / fl_jac_double_q: fl_unit_curve_quad below)
extern "C" __global__ void __launch_bounds__(64) fl_unit_curve(const uint32_t* __restrict__ in,
                                                               uint32_t* __restrict__ out, uint32_t n, uint32_t op,
                                                               uint32_t p) {
    const uint32_t item = blockIdx.x * 64 + threadIdx.x;
    if (item >= n) return;
    const uint32_t* x = in + (size_t)item * IN_WORDS;
    uint32_t* y = out + (size_t)item * OUT_WORDS;
    (void)p;
    if (op <= 2) {
        FlJac s = {ld<1>(x, 0), ld<1>(x, 1), ld<1>(x, 2)};
        uint32_t flag = 0;
        if (op == 0) {
            fl_jac_double(s);
        } else if (op == 1) {
            bool untouched = x[16 * 5] != 0;
            fl_jac_add_mixed(s, untouched, ld<1>(x, 3), ld<2>(x, 4));
            flag = untouched ? 1u : 0u;
        } else {
            const FlJac o = {ld<1>(x, 3), ld<1>(x, 4), ld<1>(x, 5)};
            fl_jac_add(s, o);
        }
        st(y, 0, s.x, flag);
        st(y, 1, s.y, flag);
        st(y, 2, s.z, flag);
    } else if (op <= 5) {
        FlJac2 s = {ld2<1>(x, 0), ld2<1>(x, 2), ld2<1>(x, 4)};
        uint32_t flag = 0;
        if (op == 3) {
            fl_jac_double(s);
        } else if (op == 4) {
            bool untouched = x[16 * 10] != 0;
            fl_jac_add_mixed(s, untouched, ld2<1>(x, 6), ld2<2>(x, 8));
            flag = untouched ? 1u : 0u;
        } else {
            const FlJac2 o = {ld2<1>(x, 6), ld2<1>(x, 8), ld2<1>(x, 10)};
            fl_jac_add(s, o);
        }
        st2(y, 0, s.x, flag);
        st2(y, 2, s.y, flag);
        st2(y, 4, s.z, flag);
    }
}

// ---- curve_fl.h, four lanes per point (a quad: lanes 4k..4k+3) ----
//  One case per quad; every lane of the quad loads both points and writes its
//  own copy of the result to slots 3 q .. 3 q + 2 (all four must hold the sum).
//  op 0 fl_jac_add_q  s, o      1 fl_jac_double_q  s
extern "C" __global__ void __launch_bounds__(64) fl_unit_curve_quad(const uint32_t* __restrict__ in,
                                                                    uint32_t* __restrict__ out, uint32_t n, uint32_t op,
                                                                    uint32_t p) {
    const uint32_t item = blockIdx.x * 16 + (threadIdx.x >> 2);
    const int q = threadIdx.x & 3;
    if (item >= n) return;   // whole quads leave together
    const uint32_t* x = in + (size_t)item * IN_WORDS;
    uint32_t* y = out + (size_t)item * OUT_WORDS;
    (void)p;
    FlJac s = {ld<1>(x, 0), ld<1>(x, 1), ld<1>(x, 2)};
    if (op == 0) {
        const FlJac o = {ld<1>(x, 3), ld<1>(x, 4), ld<1>(x, 5)};
        fl_jac_add_q(s, o, q);
    } else if (op == 1) {
        fl_jac_double_q(s, q);
    } else {
        return;
    }
    st(y, 3 * q, s.x);
    st(y, 3 * q + 1, s.y);
    st(y, 3 * q + 2, s.z);
}

// ---------------------------------------------------------- pairing_fl.h ----
//  op 0 dbl_step_fl  r (6 slots)              -> r' (slots 0..5), line c0, c1, c2 (slots 6..11)
//     1 add_step_fl  r, qx, qy (2 slots each) -> the same layout
//     2 ell_fl       f (12 slots), the line record's 36 u64 from slot 12 on, kx (slot 17), ky (slot 18)
extern "C" __global__ void __launch_bounds__(64) fl_unit_pairing(const uint32_t* __restrict__ in,
                                                                 uint32_t* __restrict__ out, uint32_t n, uint32_t op,
                                                                 uint32_t p) {
    const uint32_t item = blockIdx.x * 64 + threadIdx.x;
    if (item >= n) return;
    const uint32_t* x = in + (size_t)item * IN_WORDS;
    uint32_t* y = out + (size_t)item * OUT_WORDS;
    (void)p;
    if (op <= 1) {
        G2JacFl r = {ld2<1>(x, 0), ld2<1>(x, 2), ld2<1>(x, 4)};
        const LineFl c = op == 0 ? dbl_step_fl(r) : add_step_fl(r, ld2<1>(x, 6), ld2<1>(x, 8));
        st2(y, 0, r.x);
        st2(y, 2, r.y);
        st2(y, 4, r.z);
        st2(y, 6, c.c0);
        st2(y, 8, c.c1);
        st2(y, 10, c.c2);
    } else if (op == 2) {
        const uint64_t* rec = reinterpret_cast<const uint64_t*>(x + 16 * 12);
        st12(y, 0, ell_fl(ld12<1>(x, 0), rec, ld<1>(x, 17), ld<1>(x, 18)));
    }
}
