// How thinly store policy 4 samples a hot FFM row's accumulator adds (kernels.hip, "store policy"): one example in 2^e adds 2^e times its g^2, and e
// grows with the row's HEAT -- how far its accumulators are beyond the optimizer's initial value.  One add carries 2^e g^2 onto an accumulator of size
// heat, so the hotter the row the coarser the quantum it can take: at the hot-row threshold theta the base exponent (3) gives 8 g^2 / theta; from
// 8 theta on 16 g^2 / (8 theta), from 16 theta 32 g^2 / (16 theta), from 32 theta 64 g^2 / (32 theta): never more than a quarter of that.
// Plain functions of values every wave can read, the same on the host and on the device.  tests/test_hot_tiers_cpu.py compiles this header into a
// stand-alone program.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FW_HT_HD __host__ __device__
#else
#define FW_HT_HD
#endif

namespace fwgpu {

constexpr uint32_t kHotTiers = 3;          // levels above the hot-row threshold; the exponent takes one step at each
constexpr uint32_t kHotTierFirst = 8;      // the first level, in units of theta; each further one is twice the one before (8, 16, 32 theta)
constexpr uint32_t kAccSampleLog2Max = 6;  // one example in 64 at the most (the draw has 23 bits; KernelParams::acc_sample_log2 is clamped to the same)

// The sampling exponent of a hot row: the launch's base exponent plus one for every tier level the row is beyond, clamped to 0 .. 6.
FW_HT_HD inline uint32_t hot_row_sample_log2(uint32_t base_log2, uint32_t tiers_beyond) {
    const uint32_t e = base_log2 + (tiers_beyond < kHotTiers ? tiers_beyond : kHotTiers);
    return e < kAccSampleLog2Max ? e : kAccSampleLog2Max;
}

// Level t (0 .. kHotTiers - 1) as the kernels compare it: an ACCUMULATOR value, the optimizer's initial value folded in exactly as KernelParams::acc_hot_theta
// has it.  Tiers off: no accumulator is beyond +infinity, so every hot row keeps the base exponent.
FW_HT_HD inline float hot_tier_level(float theta, float initial_acc, uint32_t t, bool tiers_on) {
    return tiers_on ? theta * (float)(kHotTierFirst << t) + initial_acc : __builtin_inff();
}

// The levels an accumulator is beyond ("beyond" as for the threshold itself: strictly greater; a NaN is beyond nothing).
FW_HT_HD inline uint32_t hot_tiers_beyond(float acc, float l0, float l1, float l2) { return (acc > l0 ? 1u : 0u) + (acc > l1 ? 1u : 0u) + (acc > l2 ? 1u : 0u); }

}  // namespace fwgpu
