// Test-only code object (tests/test_pairing_domain.py): the pairing-only Miller
// loops' fix-up (pairing_amd/csrc/pairing_fl.h pairing_ml_fixup_lane, the body
// of kernels_pairing.hip k_pairing_ml_fixup) on its own, one pair per lane.
//
//   pairing_fixup_unit_on_curve  flags[i] = g2_on_curve_fl(Q_i), whatever the
//                                infinity words say
//   pairing_fixup_unit_run       the library kernel's body; wrote[i] = whether
//                                lane i overwrote out[i]
#include "../../pairing_amd/csrc/pairing_fl.h"

using namespace pa;

extern "C" __global__ void __launch_bounds__(64) pairing_fixup_unit_on_curve(const uint64_t* __restrict__ q_aff,
                                                                             uint8_t* __restrict__ flags,
                                                                             uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t* qq = q_aff + 25 * (size_t)i;
    flags[i] = g2_on_curve_fl(load2(qq), load2(qq + 12)) ? 1 : 0;
}

extern "C" __global__ void __launch_bounds__(64) pairing_fixup_unit_run(const uint64_t* __restrict__ p_aff,
                                                                        const uint64_t* __restrict__ q_aff,
                                                                        uint64_t* __restrict__ out,
                                                                        uint8_t* __restrict__ wrote, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    wrote[i] = pairing_ml_fixup_lane(p_aff, q_aff, out, i) ? 1 : 0;
}
