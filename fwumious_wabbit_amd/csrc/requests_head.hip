// Candidates of MANY requests in one predict-only launch on a model with a DEEP HEAD (fwgpu_enable_head_requests, on packed weights fwgpu_packed_enable_head_requests; DESIGN.md 4.8 "Deep heads").
//
// requests.hip gives a candidate the SUM of its pair terms; the head wants them one by one: x = [C per-combo LR sums | NT = F (F + 1) / 2 triangle
// slots], slot t = i (i + 1) / 2 + j, j <= i -- the x of kernels.hip's emit_x branch.  With S the cached field sums (d_T[f R .. f R + R) is
// (S[z][f], z = 0 .. F - 1)), D the sums over the candidate's own (filtered) features, G the fields it gathers, cnt_c / dcf_c the cache's counts and
// self terms, n_f / fd_f the candidate's:
//
//     (i, j), j < i:  <S_i[j], S_j[i]> + [i in G] <D_i[j], S_j[i]> + [j in G] <D_j[i], S_i[j]> + [i, j in G] <D_i[j], D_j[i]>
//     (f, f):         +0.0 when cnt_c[f] + n_f <= 1, else 0.5 (|S_f[f] + D_f[f]|^2 - (dcf_c[f] + fd_f))
//     combo c:        sum of w v over the candidate's LR entries of combo c, in buffer order (no entry: 0)
//
// requests_head_base_kernel  one workgroup per cache of the set, at the head of EVERY launch on the launch's stream (a cache refilled between two
//                          launches needs no invalidation): the cache's NT-float triangle row from S alone, the diagonal as a candidate that does not
//                          touch the field sees it.  One thread owns a slot, kk in order; no atomics.
// requests_head_kernel     one wavefront per candidate, no workgroup barrier, the lane map of requests_predict_kernel: a lane holds 16 bytes of a row
//                          per chunk of 256 floats, e0 = (chunk * 64 + lane) * 4, z = e0 / k; ROWS rows in flight; D[f] parked in the wave's LDS slices,
//                          the slice of z a population count.  New: the candidate's triangle row lives in the wave's LDS and starts as a copy of its
//                          cache's base row.  Per gathered field f and chunk, a lane's dot4 of pair (f, z) is the cross term with the cache row plus,
//                          where z was gathered earlier, the term with the parked D[z][f]; on the own slot (z == f) it is |S_f[f] + D_f[f]|^2 - fd_f
//                          over the lane's four floats.  The k / 4 lanes of slot z (3, 5, ... too) are added IN LANE ORDER by shuffles, and the slot's
//                          leader lane -- the first lane of the slot, or lane 0 of a chunk that begins inside it -- adds the result into the LDS row:
//                          a slot that lies across the chunk edge is added in chunk order.  The diagonal slot is set to -dcf_c[f] before the field's
//                          chunks and halved (or zeroed, by the counts) after them.  At the end the wave stores the row coalesced to
//                          xbuf[ex X + C ..), forms the combo slots (one lane per combo; the products are fetched 64 entries at a time and handed
//                          round in buffer order) and writes {label, importance} for head_step.  No atomics anywhere: two launches, both modes,
//                          grouped or interleaved candidates give the same bits of x.
// LDS per wave: min(F, the batch's largest FFM entry count) * R + NT floats; all waves' slices first (16-byte aligned), their rows behind them.
// The layers then take x through head.hip's MFMA GEMMs or head_fused.hip (launch.cpp run_batch_head_requests).
//
// PACKED TABLES (fwgpu_packed_enable_head_requests on a regressor of fwgpu_model_load_packed_head).  requests_head_kernel is a template over the table's
// storage, as requests_predict_kernel is: PK = true reads a lane's four weights of a row as ONE 8-byte load of four f16 bucket numbers from
// p.q.ffm_q + h + e0 (rows start on a multiple of 4 buckets), issues the loads of all ROWS rows in flight first and then converts them by
// packed_weights4 (fwgpu_device.h): f16 -> f32 exactly, one multiply, one add, unfused.  Every statement behind the conversion is the f32 statement in
// the f32 order, so x has the bits the f32 kernel forms on a table that holds the dequantised values.  The cached sums stay f32: T, dcf and cnt come
// from packed_cache_build_kernel (requests.hip) in the layout requests_head_base_kernel reads, and that kernel serves both storages as it is.
// A row that crosses the chunk edge inside a slot (30 x 12) never reaches the packed form: such a shape is refused when the packed table is loaded;
// the chunk-order add above is there for f32 tables.  Rows in flight on a packed table: 4, the depth the headless packed kernel kept over 8
// (fwgpu_debug_requests_time takes 4 or 8 for the A/B; scripts/bench_serving_packed_head_requests.py records both).
#include <math.h>

#include <algorithm>

#include "fwgpu_device.h"

namespace fwgpu {

static constexpr uint32_t kRhBaseThreads = 256;
static constexpr uint32_t kRhMaxWaves = 4;         // waves (= candidates) per workgroup
static constexpr size_t kRhLdsTarget = 64 * 1024;  // ... as many as keep the workgroup at or below this
static constexpr int kRhRows = 4;                  // rows of a field in flight per lane
static constexpr int kRhRowsPacked = 4;            // ... on a packed table (half the bytes per row; the depth the headless packed kernel kept over 8)

__global__ __launch_bounds__(kRhBaseThreads) void requests_head_base_kernel(const RequestsHeadParams p) {
    const uint32_t c = blockIdx.x;
    const uint32_t F = p.q.F, k = p.q.k, R = p.q.R;
    const float *T = p.q.cache_T[c];
    const float *dcf = p.q.cache_T[p.q.n_caches + c];
    const uint32_t *cnt = reinterpret_cast<const uint32_t *>(dcf + F);  // (one allocation: T, dcf, cnt -- fwgpu_setup_cache)
    float *row = p.q.base + (size_t)c * p.NT;
    for (uint32_t t = threadIdx.x; t < p.NT; t += kRhBaseThreads) {
        const uint2 ij = tri_slot(t);
        const uint32_t i = ij.x, j = ij.y;
        const float *a = T + (size_t)i * R + j * k, *b = T + (size_t)j * R + i * k;
        float d = 0.0f;
        for (uint32_t kk = 0; kk < k; ++kk) d = __fadd_rn(d, __fmul_rn(a[kk], b[kk]));
        if (i == j) d = cnt[i] <= 1u ? 0.0f : __fmul_rn(0.5f, __fsub_rn(d, dcf[i]));
        row[t] = d;
    }
}

// PK: the table holds f16 bucket numbers (p.q.ffm_q); ROWS: rows of a field in flight per lane
template <bool PK, int ROWS>
__global__ __launch_bounds__(64 * kRhMaxWaves) void requests_head_kernel(const RequestsHeadParams p) {
    extern __shared__ __align__(16) float rh_lds[];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const uint32_t ex = blockIdx.x * waves + wave;
    if (ex >= p.q.n) return;  // (no workgroup barrier below: a wave without a candidate just leaves)
    const uint32_t k = p.q.k, R = p.q.R, F = p.q.F, NT = p.NT, q4 = k >> 2;
    float *park = rh_lds + (size_t)wave * p.q.slots * R;
    float *row = rh_lds + (size_t)waves * p.q.slots * R + (size_t)wave * NT;
    const uint32_t ci = p.q.cache_of[ex];
    const float *T = p.q.cache_T[ci];
    const float *dcf = p.q.cache_T[p.q.n_caches + ci];
    const uint32_t *cnt = reinterpret_cast<const uint32_t *>(dcf + F);
    const uint32_t chunks = (R + 255u) >> 8;
    for (uint32_t t = lane; t < NT; t += 64u) row[t] = p.q.base[(size_t)ci * NT + t];
    wave_lds_sync();
    unsigned long long g0 = 0, g1 = 0, g2 = 0, g3 = 0;  // bit f: field f has been gathered and parked (wave-uniform)
    uint32_t ns = 0;                                     // ... how many: the next free slice
    uint32_t pos = p.q.ffm_off[ex];
    const uint32_t stop = p.q.ffm_off[ex + 1];
    while (pos < stop) {
        const uint32_t f = p.q.ffm_fld[pos];
        const uint32_t end = field_run_end(p.q.ffm_fld, pos, stop, lane);  // the field's run of entries [pos, end)
        const float *Trow = T + (size_t)f * R;
        const uint32_t td = f * (f + 1) / 2 + f;
        if (lane == 0) row[td] = -dcf[f];  // the diagonal anew: the chunks add |S + D|^2 - fd part by part
        wave_lds_sync();
        for (uint32_t c = 0; c < chunks; ++c) {
            const uint32_t e0 = (c * 64u + lane) * 4u;
            const bool inb = e0 < R;
            const uint32_t z = inb ? e0 / k : 0u;
            const bool self = inb && z == f;
            // (the gather loop and the gathered-fields mask of requests_predict_kernel<PK, ROWS>, word for word: see there)
            float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float fd = 0.0f;  // sum_i v_i^2 |w_i[f]|^2, this lane's four floats of the own slot
            for (uint32_t i = pos; i < end; i += ROWS) {
                float4 r[ROWS];
                uint2 raw[PK ? ROWS : 1];  // packed rows: the buckets as loaded; converted once all loads are issued
                float v[ROWS];
#pragma unroll
                for (int u = 0; u < ROWS; ++u) {  // all loads first (an entry beyond the run reads the run's first row again and is not added)
                    const uint32_t ii = i + u < end ? i + u : pos;
                    v[u] = p.q.ffm_val[ii];
                    const uint32_t h = p.q.ffm_hash[ii];
                    if (PK)
                        raw[PK ? u : 0] = inb ? *reinterpret_cast<const uint2 *>(p.q.ffm_q + h + e0) : make_uint2(0u, 0u);
                    else
                        r[u] = inb ? *reinterpret_cast<const float4 *>(p.q.ffm_w + h + e0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
                if (PK) {
#pragma unroll
                    for (int u = 0; u < ROWS; ++u) r[u] = packed_weights4(raw[PK ? u : 0], p.q.q_increment, p.q.q_min);
                }
#pragma unroll
                for (int u = 0; u < ROWS; ++u) {
                    if (i + u < end) {
                        const float4 t = make_float4(__fmul_rn(r[u].x, v[u]), __fmul_rn(r[u].y, v[u]), __fmul_rn(r[u].z, v[u]), __fmul_rn(r[u].w, v[u]));
                        acc.x = __fadd_rn(acc.x, t.x);
                        acc.y = __fadd_rn(acc.y, t.y);
                        acc.z = __fadd_rn(acc.z, t.z);
                        acc.w = __fadd_rn(acc.w, t.w);
                        if (self) fd = __fadd_rn(fd, dot4(t, t));
                    }
                }
            }
            float val = 0.0f;  // this lane's four floats of pair (f, z)
            if (inb) {
                const float4 s = *reinterpret_cast<const float4 *>(Trow + e0);  // S[z][f]
                if (self) {
                    const float4 u = make_float4(__fadd_rn(s.x, acc.x), __fadd_rn(s.y, acc.y), __fadd_rn(s.z, acc.z), __fadd_rn(s.w, acc.w));
                    val = __fsub_rn(dot4(u, u), fd);
                } else {
                    val = dot4(acc, s);  // <D[f][z], S[z][f]>
                    const uint32_t w = z >> 6;
                    const unsigned long long word = w == 0 ? g0 : w == 1 ? g1 : w == 2 ? g2 : g3;
                    if ((word >> (z & 63u)) & 1ull) {  // an earlier gathered field: <D[f][z], D[z][f]> with D[z] from its slice
                        const uint32_t slot = (w > 0 ? __popcll(g0) : 0) + (w > 1 ? __popcll(g1) : 0) + (w > 2 ? __popcll(g2) : 0) +
                                              __popcll(word & ((1ull << (z & 63u)) - 1ull));
                        val = __fadd_rn(val, dot4(acc, *reinterpret_cast<const float4 *>(park + (size_t)slot * R + f * k + (e0 - z * k))));
                    }
                }
                if (ns < p.q.slots) *reinterpret_cast<float4 *>(park + (size_t)ns * R + e0) = acc;  // (always: a candidate fills at most min(F, its entries) slices)
            }
            // the lanes of slot z in this chunk, added in lane order: lane l ends with its own value plus those of the slot's lanes behind it
            const uint32_t pin = inb ? (e0 - z * k) >> 2 : 0u;  // the lane's place among the slot's k / 4
            float sum = val;
            for (uint32_t d = 1; d < q4; ++d) {
                const float t = __shfl_down(val, d, 64);
                if (pin + d < q4 && lane + d < 64u) sum = __fadd_rn(sum, t);  // (pin + d < k / 4: lane + d is in bounds of the row and faces z too)
            }
            if (inb && (pin == 0u || lane == 0u)) {  // the slot's leader in this chunk
                const uint32_t hi = z > f ? z : f, lo = z > f ? f : z;
                float *dst = row + hi * (hi + 1) / 2 + lo;
                *dst = __fadd_rn(*dst, sum);
            }
            wave_lds_sync();  // (a slot across the chunk edge: the next chunk's lane 0 adds to what this chunk's leader left)
        }
        if (lane == 0) {
            const float d = row[td];
            row[td] = cnt[f] + (end - pos) <= 1u ? 0.0f : __fmul_rn(0.5f, d);
        }
        // the slice and the row are read by OTHER lanes of this wave when a later field completes
        wave_lds_sync();
        const unsigned long long bit = 1ull << (f & 63u);
        const uint32_t fw = f >> 6;
        g0 |= fw == 0 ? bit : 0ull;
        g1 |= fw == 1 ? bit : 0ull;
        g2 |= fw == 2 ? bit : 0ull;
        g3 |= fw == 3 ? bit : 0ull;
        ns++;
        pos = end;
    }
    float *x = p.xbuf + (size_t)ex * p.X;
    for (uint32_t t = lane; t < NT; t += 64u) x[p.C + t] = row[t];
    const uint32_t l0 = p.q.lr_off[ex], l1 = p.q.has_lr ? p.q.lr_off[ex + 1] : l0;
    // (head_combo_slots, open-coded: inlined here the helper changes this kernel's ISA)
    for (uint32_t cb = 0; cb < p.C; cb += 64u) {
        float acc = 0.0f;
        for (uint32_t b0 = l0; b0 < l1; b0 += 64u) {
            const uint32_t i = b0 + lane, nb = l1 - b0 < 64u ? l1 - b0 : 64u;
            const float prod = i < l1 ? __fmul_rn(p.q.lr[2ull * p.q.lr_hash[i]], p.q.lr_val[i]) : 0.0f;
            const uint32_t combo = i < l1 ? (uint32_t)p.lr_combo[i] : 0xffffffffu;
            for (uint32_t j = 0; j < nb; ++j) {
                const float pj = __shfl(prod, (int)j, 64);
                const uint32_t cj = (uint32_t)__shfl((int)combo, (int)j, 64);
                if (cj == cb + lane) acc = __fadd_rn(acc, pj);
            }
        }
        if (cb + lane < p.C) x[cb + lane] = acc;
    }
    if (lane == 0) store_label_importance(p.yi, p.label, p.importance, ex);
}

// the launch-shape rule of requests_launch_shape with the candidate's triangle row beside its slices
bool requests_head_launch_shape(uint32_t F, uint32_t R, uint32_t max_ffm, size_t lds_limit, RequestsShape *out) {
    const uint32_t slots = std::max<uint32_t>(1, std::min<uint32_t>(F, max_ffm));
    const size_t per_wave = ((size_t)slots * R + (size_t)F * (F + 1) / 2) * sizeof(float);
    if (per_wave > lds_limit) return false;
    const uint32_t waves = (uint32_t)std::min<size_t>(kRhMaxWaves, std::max<size_t>(1, kRhLdsTarget / per_wave));
    out->slots = slots;
    out->threads = 64 * waves;
    out->lds_bytes = per_wave * waves;
    out->chunks = (R + 255) / 256;
    return true;
}

template <bool PK, int ROWS>
static hipError_t launch_requests_head_as(const RequestsHeadParams &p, const RequestsShape &shape, hipStream_t stream) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(requests_head_kernel<PK, ROWS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shape.lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(requests_head_base_kernel, dim3(p.q.n_caches), dim3(kRhBaseThreads), 0, stream, p);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t waves = shape.threads / 64;
    hipLaunchKernelGGL((requests_head_kernel<PK, ROWS>), dim3((p.q.n + waves - 1) / waves), dim3(shape.threads), shape.lds_bytes, stream, p);
    return hipGetLastError();
}

// p.q.ffm_q != NULL: the packed table.  rows: 0 = the storage's default depth (kRhRows / kRhRowsPacked), 4 or 8 = that depth on the packed table
// (fwgpu_debug_requests_time: the A/B of the two depths)
hipError_t launch_requests_head(const RequestsHeadParams &p, const RequestsShape &shape, hipStream_t stream, int rows) {
    if (!p.q.ffm_q) return launch_requests_head_as<false, kRhRows>(p, shape, stream);
    if (rows == 0) rows = kRhRowsPacked;
    if (rows == 4) return launch_requests_head_as<true, 4>(p, shape, stream);
    if (rows == 8) return launch_requests_head_as<true, 8>(p, shape, stream);
    return hipErrorInvalidValue;
}

}  // namespace fwgpu
