// The deep head's predict-only forward for small serving batches, in ONE launch on the matrix cores (fwgpu_enable_fused_head).
//
// head.hip's GEMM route was made for training micro-batches and 32 768-row slabs: a launch per layer plus head_final_kernel, every h out to HBM and back,
// a ReLU mask per layer that a predict-only pass never reads.  A request set of tens to a few thousand candidates is launch- and round-trip-bound there.
// Here a workgroup of 512 threads (8 waves) takes a tile of 32 examples through the WHOLE head (block_neural.rs:196-222 forward, block_relu.rs:38-54,
// regressor.rs:307-319 final neuron, the sigmoid's rules) without an activation leaving the CU:
//
//   LDS     xs [Xpad / 4][32][4]           the tile's rows of x, zero-padded to Xpad = 8 ceil(X / 8) floats and beyond n
//           h0, h1 [Hpad / 4][32][4]       two ping-pong buffers for the hidden layers' outputs, Hpad = 8 ceil(widest layer / 8)
//           = 32 (Xpad + 2 Hpad) floats; config E (X = 496, 2 x 256): 32 x (496 + 512) x 4 = 126 KB -- one workgroup per CU, two waves per SIMD.
//           The layout is blocked by FOUR k: element (row, k) lives at ((k >> 2) * 32 + row) * 4 + (k & 3).  The A operand of v_mfma_f32_32x32x2_f32 wants
//           lane l to hold row l & 31; with this layout the 64 lanes of a wave read 64 CONSECUTIVE 16-byte words (ds_read_b128, no bank conflict, no
//           padding column) and each lane gets the four contiguous k it feeds to four MFMAs.
//   layer   wave w owns the 32-column output tiles w, w + 8, ... (config E: one each).  B = W_l[col, k] goes from global memory (the dense weights, a few
//           hundred KB, stay in L2) straight into registers: lane l loads the four k  8 u + 4 (l >> 5) + t  of its column as one 16-byte load -- the k order
//           of head_gemm_splitk -- three groups of eight k in flight ahead of the multiply on rotating registers.  Where in_l % 4 != 0 or the layer's
//           offset in the blob is not 16-byte aligned (shape "a": X = 29) the same loop loads its four k one by one.  Bias and ReLU / identity are applied
//           in the C/D registers (col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)) and stored into the other h buffer.  One barrier per layer.
//   final   wave w takes examples 4 w ... 4 w + 3 of the tile: lane l works for example l & 3 and walks the row's groups of four k, l >> 2, l >> 2 + 16, ...;
//           the sixteen partial sums of an example meet by shuffles.  Then head_final_kernel's sigmoid, statement by statement.
//
// No atomics, the order of every sum is fixed by (tile, wave, k): two launches give the same bits, and a row of the MFMA's A operand reaches only its own
// row of C, so a prediction does not depend on which other examples share its tile.  Exact f32 throughout (no packed fp32 operations: Makefile).
#include "fwgpu_internal.h"

namespace fwgpu {

typedef float hf16v __attribute__((ext_vector_type(16)));
typedef float hf4v __attribute__((ext_vector_type(4)));

constexpr int kHfRows = 32;    // examples per workgroup = rows of the MFMA tile
constexpr int kHfWaves = 8;
constexpr int kHfThreads = 64 * kHfWaves;

__host__ __device__ inline uint32_t hf_pad8(uint32_t v) { return (v + 7u) & ~7u; }
// float index of (row, k) in a blocked LDS buffer
__device__ __forceinline__ int hf_at(int row, int k) { return (((k >> 2) * kHfRows + row) << 2) + (k & 3); }

// One hidden layer: hout[32, out_w] = act(ain[32, in_w] . W^T + bias).  ain holds 8 ceil(in_w / 8) floats per row, zeros beyond in_w; hout gets zeros in
// the columns out_w ... 8 ceil(out_w / 8) - 1 that the next layer's A operand reads.
template <bool VEC>
__device__ __forceinline__ void hf_layer(const float *__restrict__ W, const float *__restrict__ bias, const float *ain, float *hout, int in_w, int out_w,
                                         int relu, int lane, int wave) {
    const int half = lane >> 5, ij = lane & 31;
    const int Ufull = in_w >> 3, U = (in_w + 7) >> 3, out_pad = (out_w + 7) & ~7, tiles = (out_w + 31) >> 5;
    const hf4v z4 = {0, 0, 0, 0};
    const hf4v *a4 = reinterpret_cast<const hf4v *>(ain) + half * kHfRows + ij;
    auto ld_a = [&](int u) -> hf4v { return a4[64 * min(u, U - 1)]; };  // group u of the lane's row (clamped: a pipeline's look-ahead stays inside the buffer)
    for (int ct = wave; ct < tiles; ct += kHfWaves) {
        const int col = ct * 32 + ij;
        const bool cok = col < out_w;  // (the last tile is masked: its lanes beyond the layer's width read column 0 and store zeros)
        const float *wrow = W + (size_t)(cok ? col : 0) * in_w + 4 * half;
        // a FULL group of eight k, every lane inside its row: no test, no branch, so that the loads stay in flight across the multiplies
        // (clamped to the last full group: the look-ahead past it re-reads that group and is not multiplied)
        auto ld_b = [&](int u) -> hf4v {
            const float *q = wrow + 8 * min(u, Ufull - 1);
            if (VEC) return *reinterpret_cast<const hf4v *>(q);
            hf4v v;
#pragma unroll
            for (int t = 0; t < 4; ++t) v[t] = q[t];
            return v;
        };
        hf16v acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        auto mul = [&](const hf4v &a, const hf4v &b) {
#pragma unroll
            for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[t], acc, 0, 0, 0);
        };
        // the ragged last group (in_w % 8 != 0), loaded first and multiplied last: the lane's four k one by one against the row's end
        hf4v bt = z4;
        if (in_w & 7) {
            const int kt = 8 * Ufull + 4 * half;
            if (VEC) {  // (in_w % 4 == 0: the four k are inside the row together or not at all)
                if (kt < in_w) bt = *reinterpret_cast<const hf4v *>(wrow + 8 * Ufull);
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (kt + t < in_w) bt[t] = wrow[8 * Ufull + t];
            }
        }
        if (Ufull) {
            // three groups of B in flight ahead of the one being multiplied, A one group ahead from LDS; four steps written out so that the registers
            // rotate by NAME (a copy of a register waits for its load: a loop of one step with b0 = b1 ... drains the queue every step); the scheduling
            // barriers keep each step's loads ahead of its multiplies, where the scheduler would otherwise gather them at the loop's end
            hf4v b0 = ld_b(0), b1 = ld_b(1), b2 = ld_b(2), b3;
            hf4v a0 = ld_a(0), a1, a2, a3;
            int u = 0;
            for (; u + 4 <= Ufull; u += 4) {
                b3 = ld_b(u + 3);
                a1 = ld_a(u + 1);
                mul(a0, b0);
                __builtin_amdgcn_sched_barrier(0);
                b0 = ld_b(u + 4);
                a2 = ld_a(u + 2);
                mul(a1, b1);
                __builtin_amdgcn_sched_barrier(0);
                b1 = ld_b(u + 5);
                a3 = ld_a(u + 3);
                mul(a2, b2);
                __builtin_amdgcn_sched_barrier(0);
                b2 = ld_b(u + 6);
                a0 = ld_a(u + 4);
                mul(a3, b3);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (u < Ufull) mul(a0, b0);  // (up to three full groups left, their B already here)
            if (u + 1 < Ufull) mul(ld_a(u + 1), b1);
            if (u + 2 < Ufull) mul(ld_a(u + 2), b2);
        }
        if (in_w & 7) mul(ld_a(Ufull), bt);
        if (col < out_pad) {
            const float bj = cok ? bias[col] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
                float v = acc[r] + bj;
                if (relu && v < 0.0f) v = 0.0f;  // (block_relu.rs:38-54; a NaN passes, as in head_gemm)
                hout[hf_at(row, col)] = cok ? v : 0.0f;
            }
        }
    }
}

__global__ void __launch_bounds__(kHfThreads) head_forward_fused_kernel(const float *__restrict__ x, float *__restrict__ pred, DevNN nn, uint32_t n,
                                                                        uint32_t xpad, uint32_t hpad, uint32_t vec_mask) {
    extern __shared__ __attribute__((aligned(16))) float hf_lds[];
    float *xs = hf_lds, *h0 = hf_lds + kHfRows * xpad, *h1 = h0 + kHfRows * hpad;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t row0 = blockIdx.x * kHfRows;
    const int X = (int)nn.X, L = (int)nn.n_layers;
    // ---- stage x: wave w brings rows 4 w ... 4 w + 3, sixteen lanes per row reading 64 contiguous bytes at a time
    {
        const int r = 4 * wave + (lane >> 4);
        const bool rok = row0 + r < n;
        const float *xr = x + (size_t)(rok ? row0 + r : 0) * X;
        for (int k = lane & 15; k < (int)xpad; k += 16) xs[hf_at(r, k)] = (rok && k < X) ? xr[k] : 0.0f;
    }
    __syncthreads();
    // ---- the hidden layers, h ping-pong in LDS
    const float *ain = xs;
    for (int l = 0; l < L; ++l) {
        const float *W = nn.w + nn.off[l];
        const float *bias = W + (size_t)nn.in[l] * nn.out[l];
        float *hout = (l & 1) ? h1 : h0;
        if ((vec_mask >> l) & 1u)
            hf_layer<true>(W, bias, ain, hout, (int)nn.in[l], (int)nn.out[l], (int)nn.relu[l], lane, wave);
        else
            hf_layer<false>(W, bias, ain, hout, (int)nn.in[l], (int)nn.out[l], (int)nn.relu[l], lane, wave);
        __syncthreads();
        ain = hout;
    }
    // ---- final neuron: logit = w_f . [h_last | x] + b_f (regressor.rs:307-319; topology two: h_last alone), then the sigmoid's rules
    const int e = lane & 3, j = lane >> 2, row = 4 * wave + e;
    const int wl = (int)nn.out[L - 1], topo_one = nn.topology == 1;
    const float *wf = nn.w + nn.off[L];
    const hf4v *h4 = reinterpret_cast<const hf4v *>(ain) + row, *x4 = reinterpret_cast<const hf4v *>(xs) + row;
    float dot = 0.0f;
    for (int kg = j; 4 * kg < wl; kg += 16) {
        const hf4v h = h4[kg * kHfRows];
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (4 * kg + t < wl) dot += wf[4 * kg + t] * h[t];
    }
    if (topo_one)
        for (int kg = j; 4 * kg < X; kg += 16) {
            const hf4v v = x4[kg * kHfRows];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (4 * kg + t < X) dot += wf[wl + 4 * kg + t] * v[t];
        }
#pragma unroll
    for (int m = 32; m >= 4; m >>= 1) dot += __shfl_xor(dot, m, 64);
    const float z = wf[wl + (topo_one ? X : 0)] + dot;
    float p;
    if (isnan(z)) {
        p = 1.0f / (1.0f + expf(-0.0f));
    } else if (z < -50.0f) {
        p = 1.0f / (1.0f + expf(50.0f));
    } else if (z > 50.0f) {
        p = 1.0f / (1.0f + expf(-50.0f));
    } else {
        p = 1.0f / (1.0f + expf(-z));
    }
    if (j == 0 && row0 + row < n) pred[row0 + row] = p;
}

// LDS bytes of a workgroup for the regressor's head; 0: the kernel does not serve it (no head, or a head whose tile does not fit the CU's LDS --
// the caller keeps the GEMM route)
size_t head_fused_lds_bytes(const fwgpu_regressor *r) {
    const DevNN &nn = r->nn;
    if (!nn.n_layers) return 0;
    const size_t bytes = (size_t)kHfRows * (hf_pad8(nn.X) + 2 * (size_t)hf_pad8(nn.max_out)) * sizeof(float);
    return bytes <= r->lds_per_cu ? bytes : 0;
}

// pred[0 .. n) = head(x[0 .. n)) with the regressor's dense weights as they are now.  FWGPU_ERR_RANGE: a head the kernel does not serve.
int head_forward_fused(fwgpu_regressor *r, const float *x, uint32_t n, float *d_pred, hipStream_t stream) {
    const DevNN &nn = r->nn;
    const size_t lds = head_fused_lds_bytes(r);
    if (!lds) return fail(FWGPU_ERR_RANGE, "head_forward_fused: no deep head, or a tile of 32 examples of it does not fit the LDS");
    if (!n) return FWGPU_OK;
    uint32_t vec_mask = 0;  // layers whose weight rows are read 16 bytes at a time (hipMalloc aligns the blob itself)
    for (uint32_t l = 0; l < nn.n_layers; l++)
        if (nn.in[l] % 4 == 0 && nn.off[l] % 4 == 0 && ((uintptr_t)nn.w & 15u) == 0) vec_mask |= 1u << l;
    FWGPU_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(head_forward_fused_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(head_forward_fused_kernel, dim3((n + kHfRows - 1) / kHfRows), dim3(kHfThreads), lds, stream, x, d_pred, nn, n, hf_pad8(nn.X),
                       hf_pad8(nn.max_out), vec_mask);
    FWGPU_HIP(hipGetLastError());
    return FWGPU_OK;
}

}  // namespace fwgpu

// debug (scripts/bench_head_fused.py): milliseconds per pass, by device events over `reps` passes on the null stream, of the head alone over the first n
// rows of x that the last batched head predict launch left on the device -- fused != 0: head_forward_fused_kernel, else head_step(update = false).
// The predictions of the last pass go to `pred` (n floats; may be NULL).
extern "C" int fwgpu_debug_head_forward_time(fwgpu_regressor *r, uint32_t n, int fused, uint32_t reps, float *ms_per_pass, float *pred) {
    using namespace fwgpu;
    if (!r || !ms_per_pass || !n || !reps) return fail(FWGPU_ERR_INVALID, "debug_head_forward_time: NULL argument, no rows or no passes");
    if (!r->pred_x || r->pred_n < n) return fail(FWGPU_ERR_INVALID, "debug_head_forward_time: the last batch launch left fewer than n head inputs on the device");
    FWGPU_HIP(hipSetDevice(r->device));
    fwgpu_split view;
    view.owner = r;
    view.d_x = r->pred_x;
    view.d_g = r->pred_yi;
    float *d_pred = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    auto done = [&](int code) {
        if (d_pred) (void)hipFree(d_pred);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        return code;
    };
    if (hipMalloc((void **)&d_pred, (size_t)n * sizeof(float)) != hipSuccess || hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess)
        return done(fail(FWGPU_ERR_DEVICE, "debug_head_forward_time: allocation failed"));
    auto pass = [&]() { return fused ? head_forward_fused(r, r->pred_x, n, d_pred, nullptr) : head_step(r, &view, 0, n, d_pred, /*update=*/false, nullptr); };
    if (int rc = pass()) return done(rc);  // (warm-up: code objects, the GEMM route's scratch)
    if (hipEventRecord(ev[0], nullptr) != hipSuccess) return done(fail(FWGPU_ERR_DEVICE, "debug_head_forward_time: no event"));
    for (uint32_t i = 0; i < reps; i++)
        if (int rc = pass()) return done(rc);
    if (hipEventRecord(ev[1], nullptr) != hipSuccess || hipEventSynchronize(ev[1]) != hipSuccess) return done(fail(FWGPU_ERR_DEVICE, "debug_head_forward_time: the passes failed"));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, ev[0], ev[1]) != hipSuccess) return done(fail(FWGPU_ERR_DEVICE, "debug_head_forward_time: no event time"));
    *ms_per_pass = ms / (float)reps;
    if (pred && hipMemcpy(pred, d_pred, (size_t)n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
        return done(fail(FWGPU_ERR_DEVICE, "debug_head_forward_time: read-back failed"));
    return done(FWGPU_OK);
}
