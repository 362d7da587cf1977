// The head's inputs of a whole predict-only batch on a PACKED table (fwgpu_model_load_packed_head of a model with a deep head; DESIGN.md 4.8 "Deep heads").
//
// x = [C per-combo LR sums | NT = F (F + 1) / 2 triangle slots], slot t = i (i + 1) / 2 + j, j <= i -- the x of kernels.hip's emit_x branch (its formulas: the
// top of requests_head.hip; t -> (i, j): tri_slot).  With S_f the R-vector of field f's sum of v * row over the example's entries of field f (S_f[z] its k floats facing z):
//
//     (i, j), j < i:  <S_i[j], S_j[i]>
//     (f, f):         +0.0 when field f has at most one entry, else 0.5 (|S_f[f]|^2 - sum_entries v^2 |w[f]|^2)
//     combo c:        sum of w v over the example's LR entries of combo c, in buffer order (no entry: 0)
//
// packed_head_inputs_kernel  one workgroup of 256 threads per example; the grid strides over the batch, so n = 1 and n = 100 000 run the same code.
//   GATHER   Waves own fields: wave w takes f = w, w + 4, ... -- an assignment that depends on F alone.  For a field it owns the wave looks at the
//            example's field bytes 64 at a time (one ballot per look: the entries of the field in buffer order, wherever they lie -- one run, several
//            runs, none) and takes them four at a time.  The lane map is that of requests.hip: lane l of chunk c holds the four weights at
//            e0 = (c * 64 + l) * 4, facing field z = e0 / k, ONE 8-byte load of four f16 buckets predicated on e0 < R (rows start on multiples of 4
//            buckets: the launch refuses an entry batch that is not aligned so).  All loads of the four rows are issued, then converted --
//            packed_weights4: f16 -> f32 exactly, one multiply, one add, unfused -- and v * w is added into one (R <= 256) or two
//            (R <= 512) float4 per lane in entry order.  The lanes of the own slot (z == f) also add sum (v w)^2 over their four floats.  The wave
//            stores S_f ONCE into LDS (zeros where the field has no entry), the own-slot lanes their partial self terms, lane 0 the entry count.
//            No atomics, no two waves on one row: the bits of x do not depend on scheduling.
//   COMBOS   the last wave (it owns the fewest fields), head_combo_slots: one lane per combo, the products of 64 entries at a time handed
//            round in buffer order.
//   TRIANGLE after ONE workgroup barrier thread t owns slots t, t + 256, ...: its k-long dot from LDS, kk in order, every operation rounded (the build
//            has no contraction); the diagonal by the counts; the store to xbuf[ex X + C + t] is coalesced as it is, so no triangle row is kept
//            in LDS.  A second barrier ends the example: the next one's gather overwrites S.
// LDS LAYOUT, a deviation from rows of R floats.  Neighbouring threads of the triangle read S_i[j] with j ascending (stride: one slot) and S_j[i]
//   with j ascending (stride: one row), 16 bytes per read.  At config E (k = 16, R = 480) both strides are multiples of 64 bytes and a plain layout
//   would send a whole wave's reads to one or two groups of four banks.  So a slot is padded to ks floats and a row to RP floats with ks / 4 and
//   RP / 4 ODD: an odd multiple of four banks visits every group of four banks before it repeats, whatever power of two the bank count is.  The
//   choice is by this reasoning, not by a measurement.  Config E: ks = 20, RP = 604, 30 rows = 72.5 KB (57.6 KB unpadded), + 0.6 KB of self terms and
//   counts: two workgroups still share a CU's 160 KiB.  A shape whose S does not fit the CU's LDS is refused at the launch (packed_head_launch_shape).
// Matrix instructions do not fit here: the kernel is a gather bound by the bucket bytes and its reductions are k-long dots.  The layers then take x
// through head.hip's MFMA GEMMs or head_fused.hip (launch.cpp run_batch_packed_head).
#include <math.h>

#include <algorithm>

#include "fwgpu_device.h"

namespace fwgpu {

static constexpr uint32_t kPhThreads = 256;
static constexpr uint32_t kPhWaves = kPhThreads / 64;
static constexpr int kPhRows = 4;           // rows of a field in flight per lane
static constexpr uint32_t kPhMaxPerCu = 8;  // workgroups per CU the grid is sized for (32 waves), where the LDS lets them in

// CH: chunks of 256 floats per row (1: R <= 256, 2: R <= 512)
template <int CH>
__global__ __launch_bounds__(kPhThreads) void packed_head_inputs_kernel(const PackedHeadParams p) {
    extern __shared__ __align__(16) float ph_lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t F = p.F, k = p.k, R = p.R, q4 = k >> 2, ks = p.ks, RP = p.RP;
    float *S = ph_lds;                                                    // [F * RP] row f: S_f, slot z at z * ks
    float *dself = S + (size_t)F * RP;                                    // [R / 4] field f's sum (v w)^2, one partial per lane of its own slot
    uint32_t *cnt = reinterpret_cast<uint32_t *>(dself + (R >> 2));       // [F] entries per field
    uint32_t e0[CH], so[CH];  // the lane's four floats of a row, and where they lie in a padded LDS row
    bool inb[CH];
    uint32_t zf[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        e0[c] = ((uint32_t)c * 64u + lane) * 4u;
        inb[c] = e0[c] < R;
        zf[c] = inb[c] ? e0[c] / k : 0xffffffffu;
        so[c] = inb[c] ? zf[c] * ks + (e0[c] - zf[c] * k) : 0u;
    }
    for (uint32_t ex = blockIdx.x; ex < p.n; ex += gridDim.x) {
        const uint32_t pos = p.ffm_off[ex], stop = p.ffm_off[ex + 1];
        for (uint32_t f = wave; f < F; f += kPhWaves) {
            float4 acc[CH];
            float fd[CH];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                acc[c] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                fd[c] = 0.0f;
            }
            uint32_t nf = 0;
            for (uint32_t base = pos; base < stop; base += 64u) {
                const uint32_t i = base + lane;
                unsigned long long mask = __ballot(i < stop && p.ffm_fld[i] == f);  // (wave-uniform: so is everything that steers the loops below)
                nf += (uint32_t)__popcll(mask);
                while (mask) {
                    uint32_t ii[kPhRows];
                    int live = 0;
#pragma unroll
                    for (int u = 0; u < kPhRows; ++u) {  // the next four entries of the field (beyond the last: the first again, loaded and not added)
                        if (mask) {
                            ii[u] = base + (uint32_t)__builtin_ctzll(mask);
                            mask &= mask - 1ull;
                            ++live;
                        } else {
                            ii[u] = ii[0];
                        }
                    }
                    uint2 raw[CH][kPhRows];
                    float v[kPhRows];
#pragma unroll
                    for (int u = 0; u < kPhRows; ++u) {  // all loads first
                        v[u] = p.ffm_val[ii[u]];
                        const uint32_t h = p.ffm_hash[ii[u]];
#pragma unroll
                        for (int c = 0; c < CH; ++c)
                            raw[c][u] = inb[c] ? *reinterpret_cast<const uint2 *>(p.ffm_q + h + e0[c]) : make_uint2(0u, 0u);
                    }
#pragma unroll
                    for (int u = 0; u < kPhRows; ++u) {
                        if (u < live) {
#pragma unroll
                            for (int c = 0; c < CH; ++c) {
                                const float4 w = packed_weights4(raw[c][u], p.q_increment, p.q_min);
                                const float4 t = make_float4(__fmul_rn(w.x, v[u]), __fmul_rn(w.y, v[u]), __fmul_rn(w.z, v[u]), __fmul_rn(w.w, v[u]));
                                acc[c].x = __fadd_rn(acc[c].x, t.x);
                                acc[c].y = __fadd_rn(acc[c].y, t.y);
                                acc[c].z = __fadd_rn(acc[c].z, t.z);
                                acc[c].w = __fadd_rn(acc[c].w, t.w);
                                if (zf[c] == f)
                                    fd[c] = __fadd_rn(fd[c], dot4(t, t));
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                if (inb[c]) {
                    *reinterpret_cast<float4 *>(S + (size_t)f * RP + so[c]) = acc[c];
                    if (zf[c] == f) dself[e0[c] >> 2] = fd[c];  // (e0 / 4 = f k / 4 + the lane's place in the slot)
                }
            }
            if (lane == 0) cnt[f] = nf;
        }
        float *x = p.xbuf + (size_t)ex * p.X;
        if (wave == kPhWaves - 1) {
            head_combo_slots(x, p.C, p.lr, p.lr_hash, p.lr_val, p.lr_combo, p.lr_off[ex], p.has_lr ? p.lr_off[ex + 1] : p.lr_off[ex], lane);
        }
        if (tid == 0) store_label_importance(p.yi, p.label, p.importance, ex);
        __syncthreads();  // every S row, self term and count of this example is in LDS
        for (uint32_t t = tid; t < p.NT; t += kPhThreads) {
            const uint2 ij = tri_slot(t);
            const uint32_t i = ij.x, j = ij.y;
            const float4 *a = reinterpret_cast<const float4 *>(S + (size_t)i * RP + j * ks);  // S_i[j]
            const float4 *b = reinterpret_cast<const float4 *>(S + (size_t)j * RP + i * ks);  // S_j[i]
            float d = 0.0f;
            for (uint32_t q = 0; q < q4; ++q) {
                const float4 va = a[q], vb = b[q];
                d = __fadd_rn(d, __fmul_rn(va.x, vb.x));
                d = __fadd_rn(d, __fmul_rn(va.y, vb.y));
                d = __fadd_rn(d, __fmul_rn(va.z, vb.z));
                d = __fadd_rn(d, __fmul_rn(va.w, vb.w));
            }
            if (i == j) {
                float s = 0.0f;
                for (uint32_t q = 0; q < q4; ++q) s = __fadd_rn(s, dself[i * q4 + q]);
                d = cnt[i] <= 1u ? 0.0f : __fmul_rn(0.5f, __fsub_rn(d, s));
            }
            x[p.C + t] = d;
        }
        __syncthreads();  // (the next example's gather overwrites S)
    }
}

// slot and row strides in floats, both a multiple of 4 with an odd quarter (this file's header: LDS LAYOUT)
bool packed_head_launch_shape(uint32_t F, uint32_t k, uint32_t n, uint32_t num_cus, size_t lds_limit, PackedHeadShape *out) {
    const uint32_t R = F * k;
    if (!F || !k || k % 4 || R > 512) return false;
    const uint32_t ks = (k / 4) % 2 ? k : k + 4;
    const uint32_t RP = (F * ks / 4) % 2 ? F * ks : F * ks + 4;
    const size_t lds = ((size_t)F * RP + R / 4 + F) * sizeof(float);
    if (lds > lds_limit) return false;
    const uint32_t per_cu = (uint32_t)std::min<size_t>(kPhMaxPerCu, lds_limit / lds);
    out->ks = ks;
    out->RP = RP;
    out->lds_bytes = lds;
    out->threads = kPhThreads;
    out->chunks = (R + 255) / 256;
    out->grid = std::max<uint32_t>(1, std::min<uint32_t>(n, num_cus * per_cu));
    return true;
}

template <int CH>
static hipError_t launch_packed_head_as(const PackedHeadParams &p, const PackedHeadShape &shape, hipStream_t stream) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(packed_head_inputs_kernel<CH>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shape.lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((packed_head_inputs_kernel<CH>), dim3(shape.grid), dim3(shape.threads), shape.lds_bytes, stream, p);
    return hipGetLastError();
}

hipError_t launch_packed_head_inputs(const PackedHeadParams &p, const PackedHeadShape &shape, hipStream_t stream) {
    if (p.ks != shape.ks || p.RP != shape.RP || !p.n) return hipErrorInvalidValue;
    return shape.chunks == 1 ? launch_packed_head_as<1>(p, shape, stream) : launch_packed_head_as<2>(p, shape, stream);
}

}  // namespace fwgpu
