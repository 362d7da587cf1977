// Device helpers shared by the HIP translation units (kernels.hip, sparse.hip, requests.hip, requests_head.hip, head_packed.hip).
#pragma once
#include <math.h>

#include "fwgpu_internal.h"

namespace fwgpu {

// ---- optimizer steps (optimizer.rs).  acc chain is kept free of FMA contraction so that, given the same
// gradient, acc (and hence the integer LUT key) is bit-identical to the reference.
template <int OPT>
__device__ __forceinline__ float opt_step(float grad, float &acc, float rate, float minus_power_t, const float *lut) {
    if (OPT == FWGPU_OPT_SGD) {
        return grad * rate;  // optimizer.rs:36-38
    } else if (OPT == FWGPU_OPT_ADAGRAD_FLEX) {  // optimizer.rs:76-88
        float na = __fadd_rn(acc, __fmul_rn(grad, grad));
        acc = na;
        float u = __fmul_rn(__fmul_rn(grad, rate), powf(na, minus_power_t));
        return (isnan(u) || isinf(u)) ? 0.0f : u;
    } else {  // optimizer.rs:147-156
        float na = __fadd_rn(acc, __fmul_rn(grad, grad));
        acc = na;
        // (a diverged model can put a NaN with the sign bit set here, whose key would index past the 2048-entry table: the
        // reference's bounds check panics at that point, optimizer.rs:152; this stays inside the table and goes on with NaNs)
        uint32_t key = (__float_as_uint(na) >> (31 - kLutBits)) & (uint32_t)(kLutSize - 1);
        return __fmul_rn(grad, lut[key]);
    }
}

// ---- what the example kernels and the serving kernels must agree on: each helper below is the ONE statement of a rounding or an order that the tests
// compare per float against the oracle.  All are forced inline; the build has no contraction (-ffp-contract=off), so every multiply and add below is
// rounded on its own.  A site that keeps an open-coded copy names the helper it mirrors: there the inlined helper changed the kernel's ISA.

// packed FFM rows (fwgpu_model_load_packed): the table holds the quantised inference file's f16 BUCKET NUMBERS, two bytes per weight, and a gather turns
// each into the weight the host's dequantize_ffm (model_file.cpp, quantization.rs:82-98) would have stored: w = min + f32(bucket) * increment -- the
// conversion is exact, then ONE multiply and ONE add, unfused (bit-identical for every f16 pattern).
__device__ __forceinline__ float packed_weight(uint32_t bucket16, float increment, float mn) {
    const _Float16 h = __builtin_bit_cast(_Float16, (unsigned short)bucket16);
    return __fadd_rn(mn, __fmul_rn((float)h, increment));
}
// four consecutive buckets (8 bytes, lowest address first) -> the lane's four weights of a row
__device__ __forceinline__ float4 packed_weights4(uint2 raw, float increment, float mn) {
    return make_float4(packed_weight(raw.x & 0xffffu, increment, mn), packed_weight(raw.x >> 16, increment, mn),
                       packed_weight(raw.y & 0xffffu, increment, mn), packed_weight(raw.y >> 16, increment, mn));
}

// ((a.x b.x + a.y b.y) + a.z b.z) + a.w b.w, every operation rounded
__device__ __forceinline__ float dot4(const float4 &a, const float4 &b) {
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y)), __fmul_rn(a.z, b.z)), __fmul_rn(a.w, b.w));
}

// LDS accesses of OTHER lanes of this wave ordered against this lane's, wave-wide: release, wave barrier, acquire (no workgroup barrier)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// every lane gets the sum of all 64: the butterfly v += shuffle_xor(v, m), m = 32, 16, 8, 4, 2, 1, each add rounded
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ float logistic(float t) { return 1.0f / (1.0f + expf(-t)); }  // block_loss_functions.rs:15-17

// logit -> prediction (block_loss_functions.rs:105-153): NaN -> logistic(0), below -50 -> logistic(-50), above 50 -> logistic(50), in that order
__device__ __forceinline__ float clipped_prediction(float logit) {
    if (isnan(logit)) return logistic(0.0f);
    if (logit < -50.0f) return logistic(-50.0f);
    if (logit > 50.0f) return logistic(50.0f);
    return logistic(logit);
}

// triangle slot t = i (i + 1) / 2 + j, j <= i  ->  {i, j}: a float guess of i, corrected in integers both ways (exact for every t)
__device__ __forceinline__ uint2 tri_slot(uint32_t t) {
    uint32_t i = (uint32_t)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    while (i * (i + 1) / 2 > t) --i;
    return make_uint2(i, t - i * (i + 1) / 2);
}

// The entries arrive ordered by field: the end of the run [pos, end) of field f = fld[pos], 64 field bytes per look (one ballot each; wave-uniform)
__device__ __forceinline__ uint32_t field_run_end(const uint8_t *fld, uint32_t pos, uint32_t stop, uint32_t lane) {
    const uint32_t f = fld[pos];
    uint32_t end = pos + 1;
    while (end < stop) {
        const uint32_t i = end + lane;
        const unsigned long long same = __ballot(i < stop && fld[i] == f);
        const uint32_t cnt = ~same ? (uint32_t)__builtin_ctzll(~same) : 64u;
        end += cnt;
        if (cnt < 64u) break;
    }
    return end;
}

// The combo slots of the head's input, x[c] = sum of w v over the LR entries [l0, l1) of combo c in BUFFER ORDER (no entry: 0), by one wave: lane l
// owns combo cb + l; the products of 64 entries at a time are formed once and handed round by shuffles
__device__ __forceinline__ void head_combo_slots(float *x, uint32_t C, const float *lr, const uint32_t *lr_hash, const float *lr_val, const uint16_t *lr_combo,
                                                 uint32_t l0, uint32_t l1, uint32_t lane) {
    for (uint32_t cb = 0; cb < C; cb += 64u) {
        float acc = 0.0f;
        for (uint32_t b0 = l0; b0 < l1; b0 += 64u) {
            const uint32_t i = b0 + lane, nb = l1 - b0 < 64u ? l1 - b0 : 64u;
            const float prod = i < l1 ? __fmul_rn(lr[2ull * lr_hash[i]], lr_val[i]) : 0.0f;
            const uint32_t combo = i < l1 ? (uint32_t)lr_combo[i] : 0xffffffffu;
            for (uint32_t j = 0; j < nb; ++j) {
                const float pj = __shfl(prod, (int)j, 64);
                const uint32_t cj = (uint32_t)__shfl((int)combo, (int)j, 64);
                if (cj == cb + lane) acc = __fadd_rn(acc, pj);
            }
        }
        if (cb + lane < C) x[cb + lane] = acc;
    }
}
// {label, importance} of example ex where head_step reads them (one thread)
__device__ __forceinline__ void store_label_importance(float *yi, const float *label, const float *importance, uint32_t ex) {
    yi[2 * (size_t)ex] = label[ex];
    yi[2 * (size_t)ex + 1] = importance[ex];
}

}  // namespace fwgpu
