// The reference's FFM weight quantiser (quantization.rs:18-80) on the device: a trained regressor's f32 weight table becomes the inference file's
// block -- 8-byte header {f32 increment, f32 min}, then one f16 bucket number per weight -- without the table crossing to the host.
//
// CONTRACT: the bytes are those of the host quantiser (model_file.cpp quantize_ffm, fwgpu_quantize_ffm_weights) on the same weights.
//   statistics pass  min and max of exactly n weights (the table's 64 padding floats are not part of it), and a flag when a weight is not finite.
//                    Min and max do not depend on the order of reduction, so any tree gives the host's two floats.  (The reference's sampled mean
//                    only feeds a log line and is not computed.)
//   header           formed ON THE HOST from the two reduced floats by quantize_header, the statements quantize_ffm itself runs.
//   bucket pass      f16(roundf((w - min) / increment)): IEEE subtraction and division (the build has no fast-math and no contraction), roundf
//                    half away from zero, the conversion to f16 round-to-nearest-even with overflow to infinity (v_cvt_f16_f32 under the default
//                    rounding mode: what f32_to_f16 in model_file.cpp and the reference's `half` crate do).
// HOST ROUTE: whenever the flag is set or the header's increment is 0 or not finite -- a constant table, a NaN or an infinite weight, a maximum
//   that rounds onto the minimum -- the callers do not run the bucket pass and quantise on the host as before (regressor.cpp quantize_on_device),
//   so those results are the host's by construction, NaN payloads included.
// OUTSIDE THE CONTRACT: a table whose extreme value is a zero present with both signs.  fmin(+0, -0) is unspecified on the host, so the sign of
//   the header's min (and of nothing else) may differ there.
//
// All kernels stream: 16-byte loads, four weights per lane, a grid capped at kQuantGridCap workgroups that strides over the rest.
#include <math.h>

#include <algorithm>

#include "fwgpu_internal.h"

namespace fwgpu {

static constexpr uint32_t kQuantThreads = 256;
static_assert(kQuantWsWords >= 3 * (kQuantGridCap + 1), "statistics workspace: three words per workgroup and the result");

static uint32_t quant_grid(uint64_t groups) {
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((groups + kQuantThreads - 1) / kQuantThreads, 1), kQuantGridCap);
}

__device__ __forceinline__ void stats_take(float v, float &mn, float &mx, uint32_t &bad) {
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
    bad |= (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
}

// min / max / flag of the workgroup's lanes -> out[0..2] (min bits, max bits, flag), written by thread 0
__device__ __forceinline__ void stats_reduce_store(float mn, float mx, uint32_t bad, uint32_t *out) {
    __shared__ float s_mn[kQuantThreads / 64], s_mx[kQuantThreads / 64];
    __shared__ uint32_t s_bad[kQuantThreads / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        bad |= __shfl_xor(bad, o, 64);
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_mn[wave] = mn;
        s_mx[wave] = mx;
        s_bad[wave] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (uint32_t w = 1; w < kQuantThreads / 64; w++) {
            mn = fminf(mn, s_mn[w]);
            mx = fmaxf(mx, s_mx[w]);
            bad |= s_bad[w];
        }
        out[0] = __float_as_uint(mn);
        out[1] = __float_as_uint(mx);
        out[2] = bad;
    }
}

// ws[3 * (1 + blockIdx.x) ..]: this workgroup's partial result
__global__ __launch_bounds__(kQuantThreads) void quant_stats_kernel(const float *__restrict__ w, unsigned long long n, uint32_t *__restrict__ ws) {
    const unsigned long long n4 = n >> 2, stride = (unsigned long long)gridDim.x * kQuantThreads;
    float mn = INFINITY, mx = -INFINITY;  // (min(inf, x) = x for every finite x: the host's start from w[0] gives the same)
    uint32_t bad = 0;
    const float4 *w4 = reinterpret_cast<const float4 *>(w);
    for (unsigned long long i = (unsigned long long)blockIdx.x * kQuantThreads + threadIdx.x; i < n4; i += stride) {
        const float4 v = w4[i];
        stats_take(v.x, mn, mx, bad);
        stats_take(v.y, mn, mx, bad);
        stats_take(v.z, mn, mx, bad);
        stats_take(v.w, mn, mx, bad);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) stats_take(w[n4 * 4 + threadIdx.x], mn, mx, bad);  // the tail of an n that is no multiple of 4
    stats_reduce_store(mn, mx, bad, ws + 3 * (1 + blockIdx.x));
}

// one workgroup: the partial results -> ws[0..2]
__global__ __launch_bounds__(kQuantThreads) void quant_stats_final_kernel(uint32_t *__restrict__ ws, uint32_t n_parts) {
    float mn = INFINITY, mx = -INFINITY;
    uint32_t bad = 0;
    for (uint32_t i = threadIdx.x; i < n_parts; i += kQuantThreads) {
        mn = fminf(mn, __uint_as_float(ws[3 * (1 + i)]));
        mx = fmaxf(mx, __uint_as_float(ws[3 * (1 + i) + 1]));
        bad |= ws[3 * (1 + i) + 2];
    }
    stats_reduce_store(mn, mx, bad, ws);
}

hipError_t launch_quant_stats(const float *w, uint64_t n, uint32_t *ws, hipStream_t stream) {
    if (!n) return hipErrorInvalidValue;
    const uint32_t grid = quant_grid(n >> 2);
    hipLaunchKernelGGL(quant_stats_kernel, dim3(grid), dim3(kQuantThreads), 0, stream, w, (unsigned long long)n, ws);
    hipLaunchKernelGGL(quant_stats_final_kernel, dim3(1), dim3(kQuantThreads), 0, stream, ws, grid);
    return hipGetLastError();
}

__device__ __forceinline__ uint32_t quant_bucket(float w, float mn, float inc) {
    const _Float16 h = (_Float16)roundf((w - mn) / inc);
    return (uint32_t)__builtin_bit_cast(unsigned short, h);
}

__global__ __launch_bounds__(kQuantThreads) void quant_bucket_kernel(const float *__restrict__ w, unsigned long long n, float inc, float mn,
                                                                    uint16_t *__restrict__ q) {
    const unsigned long long n4 = n >> 2, stride = (unsigned long long)gridDim.x * kQuantThreads;
    const float4 *w4 = reinterpret_cast<const float4 *>(w);
    uint2 *q4 = reinterpret_cast<uint2 *>(q);
    for (unsigned long long i = (unsigned long long)blockIdx.x * kQuantThreads + threadIdx.x; i < n4; i += stride) {
        const float4 v = w4[i];
        uint2 o;
        o.x = quant_bucket(v.x, mn, inc) | (quant_bucket(v.y, mn, inc) << 16);
        o.y = quant_bucket(v.z, mn, inc) | (quant_bucket(v.w, mn, inc) << 16);
        q4[i] = o;  // four buckets, one 8-byte store
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) q[n4 * 4 + threadIdx.x] = (uint16_t)quant_bucket(w[n4 * 4 + threadIdx.x], mn, inc);
}

hipError_t launch_quant_buckets(const float *w, uint64_t n, float increment, float mn, uint16_t *q, hipStream_t stream) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(quant_bucket_kernel, dim3(quant_grid(n >> 2)), dim3(kQuantThreads), 0, stream, w, (unsigned long long)n, increment, mn, q);
    return hipGetLastError();
}

// LR table {w, acc} pairs -> w alone (to_weights_only, model_file.cpp): four entries per lane, two 16-byte loads and one 16-byte store
__global__ __launch_bounds__(kQuantThreads) void lr_weights_kernel(const float *__restrict__ pairs, unsigned long long n, float *__restrict__ w) {
    const unsigned long long n4 = n >> 2, stride = (unsigned long long)gridDim.x * kQuantThreads;
    const float4 *p4 = reinterpret_cast<const float4 *>(pairs);
    float4 *w4 = reinterpret_cast<float4 *>(w);
    for (unsigned long long i = (unsigned long long)blockIdx.x * kQuantThreads + threadIdx.x; i < n4; i += stride) {
        const float4 a = p4[2 * i], b = p4[2 * i + 1];
        w4[i] = float4{a.x, a.z, b.x, b.z};
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) w[n4 * 4 + threadIdx.x] = pairs[2 * (n4 * 4 + threadIdx.x)];
}

hipError_t launch_lr_weights(const float *pairs, uint64_t n_entries, float *w, hipStream_t stream) {
    if (!n_entries) return hipSuccess;
    hipLaunchKernelGGL(lr_weights_kernel, dim3(quant_grid(n_entries >> 2)), dim3(kQuantThreads), 0, stream, pairs, (unsigned long long)n_entries, w);
    return hipGetLastError();
}

// ... and -> {w, 0} pairs, the LR table of an immutable regressor (create_packed): two entries per lane, 16 bytes in, 16 bytes out
__global__ __launch_bounds__(kQuantThreads) void lr_weights_pairs_kernel(const float *__restrict__ pairs, unsigned long long n, float *__restrict__ dst) {
    const unsigned long long n2 = n >> 1, stride = (unsigned long long)gridDim.x * kQuantThreads;
    const float4 *p4 = reinterpret_cast<const float4 *>(pairs);
    float4 *d4 = reinterpret_cast<float4 *>(dst);
    for (unsigned long long i = (unsigned long long)blockIdx.x * kQuantThreads + threadIdx.x; i < n2; i += stride) {
        const float4 a = p4[i];
        d4[i] = float4{a.x, 0.0f, a.z, 0.0f};
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) {
        dst[2 * (n - 1)] = pairs[2 * (n - 1)];
        dst[2 * (n - 1) + 1] = 0.0f;
    }
}

hipError_t launch_lr_weights_pairs(const float *pairs, uint64_t n_entries, float *dst_pairs, hipStream_t stream) {
    if (!n_entries) return hipSuccess;
    hipLaunchKernelGGL(lr_weights_pairs_kernel, dim3(quant_grid(n_entries >> 1)), dim3(kQuantThreads), 0, stream, pairs, (unsigned long long)n_entries,
                       dst_pairs);
    return hipGetLastError();
}

}  // namespace fwgpu
