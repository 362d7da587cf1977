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

// ---- ranges that may end INSIDE a field (FW_SPLIT_FIELDS, profiles/r08_field_split.txt)
// Wave w's range starts at row floor(w nf / nw): every wave then holds floor(nf / nw) or ceil(nf / nw) rows.  The part of a cut field that falls
// into the second wave is that wave's LEAD: the first rows of its range, which it adds to the field's sum only after the first wave has flushed its part
// (a second pass of the gather), so the sum keeps its buffer order.  Two conditions keep that second pass one step deep and inside the register-kept rows:
//   (a) a field lies in at most two waves' ranges,   (b) a lead is at most lead_max rows.
// A cut that would break either falls back to the nearest boundary of its field, which is wave_of_field's rule.

// Examples too short for a split to pay (and all the small ones of the reference scenarios) keep wave_of_field's ranges throughout: what a split saves is
// rows re-read by the update, i.e. rows beyond the 20 + 3 a wave keeps from the gather.  Under wave_of_field the longest range of an example is about its
// share plus most of a field (+4.5 rows at config C's fields), so below a share of 16 rows no wave re-reads one and a split would only add its second pass.
constexpr uint32_t kSplitMinShare = 16;
FW_WB_HD inline bool split_fields_on(uint32_t nw, uint32_t nf) { return nf >= kSplitMinShare * nw; }

// The first row of wave w's range (0 < w < nw), given the non-empty field [a, b) that holds row floor(w nf / nw).  Where split_fields_on(nw, nf).
// The result is a (the field goes to wave w whole), b (to the wave before), or floor(w nf / nw) strictly inside: the field is split, its lead is b - result.
FW_WB_HD inline uint32_t split_cut(uint32_t a, uint32_t b, uint32_t w, uint32_t nw, uint32_t nf, uint32_t lead_max) {
    const uint32_t c = (w * nf) / nw;
    if (c == a) return a;  // the target is a field boundary as it is
    // (a): neither neighbour's target lies inside this field too (prev == a is that wave's clean cut; for w + 1 == nw, next == nf >= b)
    const uint32_t prev = ((w - 1u) * nf) / nw, next = ((w + 1u) * nf) / nw;
    if (prev <= a && next >= b && b - c <= lead_max) return c;
    return (a + b) * nw >= 2u * nf * w ? a : b;  // the field's owner under wave_of_field is >= w: it starts wave w's range; else it ends the range before
}

}  // namespace fwgpu
