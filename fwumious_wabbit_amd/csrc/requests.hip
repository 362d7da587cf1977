// Candidates of MANY requests in one predict-only launch, each against its own context cache (fwgpu_batch_set_caches; DESIGN.md "Requests").
//
// The cached routes of kernels.hip run the whole-example kernel per candidate: the F x R table T starts from the cache, the candidate's few rows are
// added and all F (F - 1) / 2 pair dots are formed again.  Here the reference's forward_with_cache result (block_ffm.rs:442-782) is regrouped so that a
// candidate pays for its own features only.  With A[f] the R-vector of field f's sum in the row's layout, S = A over the cached features (the cache's
// d_T, in which (S[z][f], z = 0..F-1) is the contiguous row d_T[f R .. f R + R)), D = A over the features the filter leaves, C the fields that have one:
//
//     logit = sum_lr w v + base(S) + sum_{f in C} <D[f], d_T[f R ..)> + sum_{f<z in C} <D[f][z], D[z][f]> + sum_{f in C} 0.5 (|D[f][f]|^2 - sum_i v_i^2 |w_i[f]|^2)
//     base(S) = sum_{f<z} <S[f][z], S[z][f]> + 0.5 sum_f (|S[f][f]|^2 - dcf[f])
//
// requests_base_kernel     one workgroup per cache of the set: base(S) -> base[cache].  It runs at the head of EVERY launch, on the launch's stream, so a
//                          cache that fwgpu_setup_cache refilled between two launches needs no invalidation.
// requests_predict_kernel  one wavefront per candidate, no workgroup barrier.  A lane holds 16 bytes of a row per chunk of 256 floats: e0 = (chunk * 64 +
//                          lane) * 4, z = e0 / k (k % 4 == 0: the four floats face one field).  The entries arrive ordered by field; the current field's
//                          D[f] is summed in registers in buffer order (block_ffm.rs:205), chunk by chunk, four rows in flight.  When a chunk of a field
//                          is complete the lane multiplies it into the cache row, into the own-slot term (z == f) or into the parked D[z][f] of an earlier
//                          gathered field z, and parks it in the wave's LDS slice.  Slices are handed out in field order, so the slice of field z is the
//                          number of gathered fields below z: a population count over a 256-bit wave-uniform mask, no table.  The per-lane partial sums
//                          are reduced once per candidate by a butterfly; there are no atomics: two launches give the same bits.
// LDS per wave: min(F, the batch's largest FFM entry count) * R floats.  The waves per workgroup are chosen on the host (requests_launch_shape).
//
// PACKED TABLES (fwgpu_packed_enable_caches).  requests_predict_kernel is a template over the table's storage: PK = true reads a lane's four weights
// as ONE 8-byte load of four f16 bucket numbers (rows start on a multiple of 4 buckets) and converts them as kernels.hip packed_weight does, bit for
// bit: f16 -> f32 exactly, then one multiply and one add, unfused, w = min + f32(bucket) * increment, the two header words being launch constants.
// Everything behind the load is the f32 code.  requests_base_kernel reads caches only and serves both.
// packed_cache_build_kernel  fwgpu_setup_cache on such a regressor: ONE wavefront per field f, the lane map of the predict kernel (chunk c, lane l:
//                          floats e0 = (c * 64 + l) * 4 .. + 3 of a row, facing field z = e0 / k).  The context's entries arrive ordered by field; the
//                          wave finds its run [lo, lo + n) by two population counts over the field bytes.  Per chunk the lane sums w * v over the run in
//                          BUFFER ORDER from 0, every multiply and add rounded, and stores T[z R + f k + (e0 - z k) ..] -- the lane is that float4's only
//                          writer; a field without a feature stores zeros.
//                          dcf[f], THE ORDER: a lane that holds four floats of the field's own slot (z == f; k / 4 lanes, in one chunk) forms per row
//                          ss = ((w0 w0 + w1 w1) + w2 w2) + w3 w3 and adds (ss v) v to its partial sum, rows in buffer order from 0; all other lanes hold
//                          0; the 64 partial sums are then added by the butterfly v += shuffle_xor(v, m), m = 32, 16, 8, 4, 2, 1.  That is the order
//                          the example kernels leave in an f32 regressor's cache (kernels.hip, the gather's dc and wave_sum), so a packed regressor and
//                          an f32 regressor that holds the dequantised values keep the same bits.  Lane 0 stores dcf[f] and cnt[f] = n.
//                          No atomics, no LDS, no barrier: two builds give the same bits.
#include <math.h>

#include <algorithm>

#include "fwgpu_internal.h"

namespace fwgpu {

static constexpr uint32_t kReqBaseThreads = 256;
static constexpr uint32_t kReqMaxWaves = 4;            // waves (= candidates) per workgroup
static constexpr size_t kReqLdsTarget = 64 * 1024;     // ... as many as keep the workgroup at or below this, so several workgroups share a CU
static constexpr int kReqRows = 4;                     // rows of a field in flight per lane
static constexpr int kReqRowsPacked = 4;               // ... on a packed table (half the bytes per row; 4 against 8: DESIGN.md 4.8)

__device__ __forceinline__ float req_logistic(float t) { return 1.0f / (1.0f + expf(-t)); }  // block_loss_functions.rs:15-17

__device__ __forceinline__ float req_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = __fadd_rn(v, __shfl_xor(v, m, 64));
    return v;
}

// ((a.x b.x + a.y b.y) + a.z b.z) + a.w b.w, every operation rounded (the build has no contraction)
__device__ __forceinline__ float req_dot4(const float4 &a, const float4 &b) {
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y)), __fmul_rn(a.z, b.z)), __fmul_rn(a.w, b.w));
}

// kernels.hip packed_weight / packed_weights4, restated: the bucket's f16 pattern to f32 exactly, then ONE multiply and ONE add, unfused
__device__ __forceinline__ float req_packed_weight(uint32_t bucket16, float increment, float mn) {
    const _Float16 h = __builtin_bit_cast(_Float16, (unsigned short)bucket16);
    return __fadd_rn(mn, __fmul_rn((float)h, increment));
}
__device__ __forceinline__ float4 req_packed_weights4(uint2 raw, float increment, float mn) {
    return make_float4(req_packed_weight(raw.x & 0xffffu, increment, mn), req_packed_weight(raw.x >> 16, increment, mn),
                       req_packed_weight(raw.y & 0xffffu, increment, mn), req_packed_weight(raw.y >> 16, increment, mn));
}

__global__ __launch_bounds__(kReqBaseThreads) void requests_base_kernel(const RequestsParams p) {
    __shared__ float s_part[kReqBaseThreads / 64];
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    const uint32_t F = p.F, k = p.k, R = p.R;
    const float *T = p.cache_T[c];
    const float *dcf = p.cache_T[p.n_caches + c];
    float s = 0.0f;
    // T[a R + b k + kk] = S[b][a][kk]: the pair (a, b), a < b, is this float times its mirror; the diagonal half its square
    for (uint32_t idx = tid; idx < F * R; idx += kReqBaseThreads) {
        const uint32_t a = idx / R, rem = idx - a * R, b = rem / k, kk = rem - b * k;
        const float t = T[idx];
        if (a < b)
            s = __fadd_rn(s, __fmul_rn(t, T[b * R + a * k + kk]));
        else if (a == b)
            s = __fadd_rn(s, __fmul_rn(0.5f, __fmul_rn(t, t)));
    }
    for (uint32_t f = tid; f < F; f += kReqBaseThreads) s = __fadd_rn(s, __fmul_rn(-0.5f, dcf[f]));
    s = req_wave_sum(s);
    if ((tid & 63) == 0) s_part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        float t = s_part[0];
#pragma unroll
        for (uint32_t w = 1; w < kReqBaseThreads / 64; w++) t = __fadd_rn(t, s_part[w]);
        p.base[c] = t;
    }
}

// PK: the table holds f16 bucket numbers (p.ffm_q); ROWS: rows of a field in flight per lane
template <bool PK, int ROWS>
__global__ __launch_bounds__(64 * kReqMaxWaves) void requests_predict_kernel(const RequestsParams p) {
    extern __shared__ __align__(16) float req_park[];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t ex = blockIdx.x * (blockDim.x >> 6) + wave;
    if (ex >= p.n) return;  // (no barrier below: a wave without a candidate just leaves)
    const uint32_t k = p.k, R = p.R;
    float *park = req_park + (size_t)wave * p.slots * R;
    const uint32_t ci = p.cache_of[ex];
    const float *T = p.cache_T[ci];
    const uint32_t chunks = (R + 255u) >> 8;
    float part = 0.0f;
    unsigned long long g0 = 0, g1 = 0, g2 = 0, g3 = 0;  // bit f: field f has been gathered and parked (wave-uniform)
    uint32_t ns = 0;                                     // ... how many: the next free slice
    uint32_t pos = p.ffm_off[ex];
    const uint32_t stop = p.ffm_off[ex + 1];
    while (pos < stop) {
        const uint32_t f = p.ffm_fld[pos];
        uint32_t end = pos + 1;  // the field's run of entries [pos, end): 64 field bytes per look
        while (end < stop) {
            const uint32_t i = end + lane;
            const unsigned long long same = __ballot(i < stop && p.ffm_fld[i] == f);
            const uint32_t cnt = ~same ? (uint32_t)__builtin_ctzll(~same) : 64u;
            end += cnt;
            if (cnt < 64u) break;
        }
        const float *Trow = T + (size_t)f * R;
        for (uint32_t c = 0; c < chunks; ++c) {
            const uint32_t e0 = (c * 64u + lane) * 4u;
            const bool inb = e0 < R;
            const uint32_t z = inb ? e0 / k : 0u;
            const bool self = inb && z == f;
            float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float fd = 0.0f;  // sum_i v_i^2 |w_i[f]|^2, this lane's four floats of the own slot
            for (uint32_t i = pos; i < end; i += ROWS) {
                float4 r[ROWS];
                uint2 raw[PK ? ROWS : 1];  // packed rows: the buckets as loaded; converted once all loads are issued
                float v[ROWS];
#pragma unroll
                for (int u = 0; u < ROWS; ++u) {  // all loads first (an entry beyond the run reads the run's first row again and is not added)
                    const uint32_t ii = i + u < end ? i + u : pos;
                    v[u] = p.ffm_val[ii];
                    const uint32_t h = p.ffm_hash[ii];
                    if (PK)
                        raw[PK ? u : 0] = inb ? *reinterpret_cast<const uint2 *>(p.ffm_q + h + e0) : make_uint2(0u, 0u);
                    else
                        r[u] = inb ? *reinterpret_cast<const float4 *>(p.ffm_w + h + e0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
                if (PK) {
#pragma unroll
                    for (int u = 0; u < ROWS; ++u) r[u] = req_packed_weights4(raw[PK ? u : 0], p.q_increment, p.q_min);
                }
#pragma unroll
                for (int u = 0; u < ROWS; ++u) {
                    if (i + u < end) {
                        const float4 t = make_float4(__fmul_rn(r[u].x, v[u]), __fmul_rn(r[u].y, v[u]), __fmul_rn(r[u].z, v[u]), __fmul_rn(r[u].w, v[u]));
                        acc.x = __fadd_rn(acc.x, t.x);
                        acc.y = __fadd_rn(acc.y, t.y);
                        acc.z = __fadd_rn(acc.z, t.z);
                        acc.w = __fadd_rn(acc.w, t.w);
                        if (self) fd = __fadd_rn(fd, req_dot4(t, t));
                    }
                }
            }
            if (inb) {
                part = __fadd_rn(part, req_dot4(acc, *reinterpret_cast<const float4 *>(Trow + e0)));  // <D[f], d_T[f R ..)>, z == f included
                if (self) {
                    part = __fadd_rn(part, __fmul_rn(0.5f, __fsub_rn(req_dot4(acc, acc), fd)));  // (one feature: exactly 0)
                } else {
                    const uint32_t w = z >> 6;
                    const unsigned long long word = w == 0 ? g0 : w == 1 ? g1 : w == 2 ? g2 : g3;
                    if ((word >> (z & 63u)) & 1ull) {  // an earlier gathered field: <D[f][z], D[z][f]> with D[z] from its slice
                        const uint32_t slot = (w > 0 ? __popcll(g0) : 0) + (w > 1 ? __popcll(g1) : 0) + (w > 2 ? __popcll(g2) : 0) +
                                              __popcll(word & ((1ull << (z & 63u)) - 1ull));
                        part = __fadd_rn(part, req_dot4(acc, *reinterpret_cast<const float4 *>(park + (size_t)slot * R + f * k + (e0 - z * k))));
                    }
                }
                if (ns < p.slots) *reinterpret_cast<float4 *>(park + (size_t)ns * R + e0) = acc;  // (always: a candidate fills at most min(F, its entries) slices)
            }
        }
        // the slice is read by OTHER lanes of this wave when a later field completes: order the LDS accesses, wave-wide (no workgroup barrier)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const unsigned long long bit = 1ull << (f & 63u);
        const uint32_t fw = f >> 6;
        g0 |= fw == 0 ? bit : 0ull;
        g1 |= fw == 1 ? bit : 0ull;
        g2 |= fw == 2 ? bit : 0ull;
        g3 |= fw == 3 ? bit : 0ull;
        ns++;
        pos = end;
    }
    if (p.has_lr) {
        const uint32_t le = p.lr_off[ex + 1];
        for (uint32_t i = p.lr_off[ex] + lane; i < le; i += 64u) part = __fadd_rn(part, __fmul_rn(p.lr[2ull * p.lr_hash[i]], p.lr_val[i]));
    }
    const float wsum = __fadd_rn(req_wave_sum(part), p.base[ci]);
    if (lane == 0) {
        float pr;  // block_loss_functions.rs:105-153: clip +-50, NaN -> 0.5
        if (isnan(wsum))
            pr = req_logistic(0.0f);
        else if (wsum < -50.0f)
            pr = req_logistic(-50.0f);
        else if (wsum > 50.0f)
            pr = req_logistic(50.0f);
        else
            pr = req_logistic(wsum);
        p.pred[ex] = pr;
    }
}

bool requests_launch_shape(uint32_t F, uint32_t R, uint32_t max_ffm, size_t lds_limit, RequestsShape *out) {
    const uint32_t slots = std::max<uint32_t>(1, std::min<uint32_t>(F, max_ffm));
    const size_t per_wave = (size_t)slots * R * sizeof(float);
    if (per_wave > lds_limit) return false;
    uint32_t waves = (uint32_t)std::min<size_t>(kReqMaxWaves, std::max<size_t>(1, kReqLdsTarget / std::max<size_t>(per_wave, 1)));
    out->slots = slots;
    out->threads = 64 * waves;
    out->lds_bytes = per_wave * waves;
    out->chunks = (R + 255) / 256;
    return true;
}

template <bool PK, int ROWS>
static hipError_t launch_requests_as(const RequestsParams &p, const RequestsShape &shape, hipStream_t stream) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(requests_predict_kernel<PK, ROWS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shape.lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(requests_base_kernel, dim3(p.n_caches), dim3(kReqBaseThreads), 0, stream, p);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t waves = shape.threads / 64;
    hipLaunchKernelGGL((requests_predict_kernel<PK, ROWS>), dim3((p.n + waves - 1) / waves), dim3(shape.threads), shape.lds_bytes, stream, p);
    return hipGetLastError();
}

// p.ffm_q != NULL: the packed table.  rows: 0 = the storage's default depth (kReqRows / kReqRowsPacked), 4 or 8 = that depth on the packed table
// (fwgpu_debug_requests_time: the A/B of the two depths)
hipError_t launch_requests(const RequestsParams &p, const RequestsShape &shape, hipStream_t stream, int rows) {
    if (!p.ffm_q) return launch_requests_as<false, kReqRows>(p, shape, stream);
    if (rows == 0) rows = kReqRowsPacked;
    if (rows == 4) return launch_requests_as<true, 4>(p, shape, stream);
    if (rows == 8) return launch_requests_as<true, 8>(p, shape, stream);
    return hipErrorInvalidValue;
}

// fwgpu_setup_cache on a packed regressor with caches enabled: the header comment of this file states the sums' order
__global__ __launch_bounds__(64) void packed_cache_build_kernel(const PackedCacheBuild p) {
    const uint32_t f = blockIdx.x, lane = threadIdx.x;
    const uint32_t k = p.k, R = p.R;
    // the field's run of entries [lo, lo + n): the entries are ordered by field
    uint32_t lo = 0, n = 0;
    for (uint32_t i0 = 0; i0 < p.n; i0 += 64u) {
        const uint32_t i = i0 + lane;
        const uint32_t fl = i < p.n ? (uint32_t)p.ffm_fld[i] : 0xffffffffu;
        lo += (uint32_t)__popcll(__ballot(fl < f));
        n += (uint32_t)__popcll(__ballot(fl == f));
    }
    const uint32_t chunks = (R + 255u) >> 8;
    float dc = 0.0f;
    for (uint32_t c = 0; c < chunks; ++c) {
        const uint32_t e0 = (c * 64u + lane) * 4u;
        if (e0 >= R) continue;  // (no barrier and no ballot below)
        const uint32_t z = e0 / k;
        const bool self = z == f;
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (uint32_t i = lo; i < lo + n; i += kReqRows) {
            uint2 raw[kReqRows];
            float v[kReqRows];
#pragma unroll
            for (int u = 0; u < kReqRows; ++u) {  // (an entry beyond the run reads the run's first row again and is not added)
                const uint32_t ii = i + u < lo + n ? i + u : lo;
                v[u] = p.ffm_val[ii];
                raw[u] = *reinterpret_cast<const uint2 *>(p.ffm_q + p.ffm_hash[ii] + e0);
            }
#pragma unroll
            for (int u = 0; u < kReqRows; ++u) {
                if (i + u < lo + n) {
                    const float4 w = req_packed_weights4(raw[u], p.q_increment, p.q_min);
                    acc.x = __fadd_rn(acc.x, __fmul_rn(w.x, v[u]));
                    acc.y = __fadd_rn(acc.y, __fmul_rn(w.y, v[u]));
                    acc.z = __fadd_rn(acc.z, __fmul_rn(w.z, v[u]));
                    acc.w = __fadd_rn(acc.w, __fmul_rn(w.w, v[u]));
                    if (self) {
                        const float ss = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w.x, w.x), __fmul_rn(w.y, w.y)), __fmul_rn(w.z, w.z)), __fmul_rn(w.w, w.w));
                        dc = __fadd_rn(dc, __fmul_rn(__fmul_rn(ss, v[u]), v[u]));
                    }
                }
            }
        }
        *reinterpret_cast<float4 *>(p.T + (size_t)z * R + f * k + (e0 - z * k)) = acc;
    }
    dc = req_wave_sum(dc);  // (every lane of the wave is here: the loop above has no early exit)
    if (lane == 0) {
        p.dcf[f] = dc;
        p.cnt[f] = n;
    }
}

hipError_t launch_packed_cache_build(const PackedCacheBuild &p, hipStream_t stream) {
    hipLaunchKernelGGL(packed_cache_build_kernel, dim3(p.F), dim3(64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace fwgpu
