// How the config-C learn kernel (fw_example_kernel_r, single-chunk rows with rows kept from the gather) spreads an example's rows over the waves of
// its workgroup.  A plain integer function of values every wave can read, the same on the host and on the device.
// tests/test_wave_balance_cpu.py compiles this header into a stand-alone program.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FW_WB_HD __host__ __device__
#else
#define FW_WB_HD
#endif

namespace fwgpu {

// The wave that owns the non-empty field [a, b) of an example of nf features: the one whose share [w nf / nw, (w + 1) nf / nw) holds the field's
// MIDDLE, so that a range boundary falls on the field start nearest to w nf / nw.  Monotone in the field (fields are in buffer order), so a wave's
// fields are neighbours and its range is one interval; (a + b) / 2 < nf, so the owner is below nw.
FW_WB_HD inline uint32_t wave_of_field(uint32_t a, uint32_t b, uint32_t nw, uint32_t nf) {
    const uint32_t o = ((a + b) * nw) / (2u * nf);
    return o < nw ? o : nw - 1u;
}

}  // namespace fwgpu
