// The per-example step rule of the mini-batched deep head (fwgpu_head_set_step_rule, FWGPU_HEAD_STEP_PER_EXAMPLE).
//
// head.hip forms a micro-batch's dz_l, layer inputs and general gradients against FROZEN dense weights; its default rule then sums the weight gradients over
// the batch (dW GEMMs, column sums) and every dense weight takes ONE optimizer step.  The reference steps every dense weight once PER EXAMPLE
// (block_neural.rs:252-340, optimizer.rs): under AdaGrad the accumulator grows by sum g^2, not (sum g)^2, and a batch of n makes n steps.  This file is that
// rule on the same frozen-weight gradients: one launch applies, to every dense weight of every layer, the batch's per-example steps in example order --
//   hidden layer l, weight (j, i):  G_e = fl(dz_l[e, j] * in_l[e, i])     bias j: G_e = dz_l[e, j]         in_0 = x, in_l = h_{l-1}
//   final neuron, weight i:         G_e = fl(gvec[e] * [h_last | x][e, i])  bias:   G_e = gvec[e]           (topology two: h_last alone)
//   step (head_apply_kernel's, statement for statement):  G == 0: nothing;  acc += G^2;  w -= G * lut[bits(acc) >> 20]   (or SGD / AdagradFlex)
// It is not a matrix product: a step needs the accumulator the step before left.  So the WEIGHTS stay put and the batch streams past them:
//   * a workgroup (256 threads) owns a TJ x 64 tile of one layer's W; the lane is i -- the fast dimension of W and of in_l --, wave v owns the TJ / 4 rows
//     j0 + v TJ / 4 ..., so a lane holds TJ / 4 weights and their accumulators in VGPRs for the whole batch: loaded once, stored once;
//   * the bias is column `in` of its layer (input 1.0: fl(dz * 1) = dz), the final neuron a layer of one row whose input has two source matrices and
//     whose dz is gvec; rows and columns beyond the layer are masked by zeros in the staged operands (G == 0 steps nothing), so all of them take the same code;
//   * the operands go through LDS in chunks of 16 examples, double-buffered: chunk c + 1's global loads are issued, chunk c is stepped from LDS, then the
//     loaded registers are written to the other buffer -- one barrier per chunk.  in_s[e][i]: a wave's read of one example is 64 consecutive floats
//     (conflict-free); dz_s[e][jj]: a wave's rows of one example are one broadcast 16-byte read (two for TJ = 32).  The input rows are loaded 16 bytes per
//     thread where the segment's row lengths and bases allow, else one float per thread per row (shape a: X = 29);
//   * the step-size LUT (2048 floats) lives in LDS.  Only acc += G^2 is serial: the accumulators of four examples are formed first, their four LUT reads
//     issued together, then the four weight steps taken -- the LDS latency once per four steps;
//   * no atomics, one writer per weight: two launches give the same bits.
// Built with packed fp32 operations off (Makefile), like head_fused.hip: every product and sum here is a rounded scalar operation.
#include "fwgpu_internal.h"

namespace fwgpu {

constexpr int kSeqTI = 64;       // columns of a tile = lanes of a wave
constexpr int kSeqE = 16;        // examples per LDS chunk
constexpr int kSeqGroup = 4;     // examples whose accumulators are formed before their LUT reads are issued together
constexpr int kSeqThreads = 256;
constexpr int kSeqWaves = kSeqThreads / 64;
enum { kSeqSgd = 0, kSeqFlex = 1, kSeqLut = 2 };

typedef float f4v __attribute__((ext_vector_type(4)));

// element (e, c) of a segment's input: columns [0, w0) from src0, [w0, w0 + w1) from src1, column w0 + w1 the bias's constant 1, zeros beyond and below the batch
__device__ __forceinline__ float seq_in_elem(const HeadSeqSeg &s, uint32_t n, uint32_t e, uint32_t c) {
    if (e >= n) return 0.0f;
    if (c < s.w0) return s.src0[(size_t)e * s.w0 + c];
    if (c < s.w0 + s.w1) return s.src1[(size_t)e * s.w1 + (c - s.w0)];
    return c == s.w0 + s.w1 ? 1.0f : 0.0f;
}

template <int OPT, int TJ>
__global__ void __launch_bounds__(kSeqThreads) head_seq_kernel(const HeadSeqPlan p) {
    constexpr int JPW = TJ / kSeqWaves;             // rows of a wave = weights of a lane
    constexpr int DZ_PT = TJ * kSeqE / kSeqThreads;  // dz floats a thread stages per chunk
    static_assert(JPW % 4 == 0 && DZ_PT >= 1, "a wave reads its rows of dz as 16-byte groups");
    __shared__ __attribute__((aligned(16))) float in_s[2][kSeqE][kSeqTI];
    __shared__ __attribute__((aligned(16))) float dz_s[2][kSeqE][TJ];
    __shared__ float lut_s[OPT == kSeqLut ? kLutSize : 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- which tile
    uint32_t si = 0;
    while (si + 1 < p.n_seg && blockIdx.x >= p.seg[si + 1].tile0) ++si;
    const HeadSeqSeg &s = p.seg[si];
    const uint32_t t = blockIdx.x - s.tile0;
    const uint32_t j0 = (t / s.tiles_i) * TJ, i0 = (t % s.tiles_i) * kSeqTI;
    const uint32_t in = s.w0 + s.w1, n = p.n;
    // ---- the lane's weights and accumulators
    const uint32_t c = i0 + lane, jw = j0 + wave * JPW;
    const bool wave_on = jw < s.rows;  // (a wave whose rows all lie beyond the layer only stages: the final neuron's tiles)
    float w[JPW], a[JPW];
    size_t at[JPW];
    bool own[JPW];
#pragma unroll
    for (int q = 0; q < JPW; ++q) {
        const uint32_t j = jw + q;
        own[q] = j < s.rows && c <= in;
        at[q] = (size_t)s.off + (c < in ? (size_t)j * in + c : (size_t)in * s.rows + j);
        w[q] = own[q] ? p.w[at[q]] : 0.0f;
        a[q] = (own[q] && OPT != kSeqSgd) ? p.acc[at[q]] : 1.0f;
    }
    if (OPT == kSeqLut)
        for (uint32_t k = tid; k < (uint32_t)kLutSize; k += kSeqThreads) lut_s[k] = p.lut[k];
    // ---- staging: a chunk's 16 x 64 inputs (4 floats per thread) and 16 x TJ dz (DZ_PT per thread) through registers into LDS
    f4v rin;
    float rdz[DZ_PT];
    auto load = [&](uint32_t e0) {
        if (s.vec) {  // e = tid / 16, four consecutive columns: a group lies inside one source, starts at the bias column or lies beyond it
            const uint32_t e = e0 + (tid >> 4), c4 = i0 + (tid & 15) * 4;
            if (e < n && c4 + 3 < s.w0) rin = *reinterpret_cast<const f4v *>(s.src0 + (size_t)e * s.w0 + c4);
            else if (e < n && c4 >= s.w0 && c4 + 3 < in) rin = *reinterpret_cast<const f4v *>(s.src1 + (size_t)e * s.w1 + (c4 - s.w0));
            else {
#pragma unroll
                for (int r = 0; r < 4; ++r) rin[r] = seq_in_elem(s, n, e, c4 + r);
            }
        } else {  // e = 4 r + tid / 64, column = lane: coalesced along the row
#pragma unroll
            for (int r = 0; r < 4; ++r) rin[r] = seq_in_elem(s, n, e0 + 4 * r + wave, c);
        }
#pragma unroll
        for (int r = 0; r < DZ_PT; ++r) {
            const uint32_t ix = tid + kSeqThreads * r, e = e0 + ix / TJ, j = j0 + ix % TJ;
            rdz[r] = (e < n && j < s.rows) ? s.dz[(size_t)e * s.ld_dz + j] : 0.0f;
        }
    };
    auto store = [&](int buf) {
        if (s.vec) {
            *reinterpret_cast<f4v *>(&in_s[buf][tid >> 4][(tid & 15) * 4]) = rin;
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) in_s[buf][4 * r + wave][lane] = rin[r];
        }
#pragma unroll
        for (int r = 0; r < DZ_PT; ++r) {
            const uint32_t ix = tid + kSeqThreads * r;
            dz_s[buf][ix / TJ][ix % TJ] = rdz[r];
        }
    };
    load(0);
    store(0);
    __syncthreads();
    const uint32_t chunks = (n + kSeqE - 1) / kSeqE;
    for (uint32_t ch = 0; ch < chunks; ++ch) {
        const int buf = ch & 1;
        const bool more = ch + 1 < chunks;
        if (more) load((ch + 1) * kSeqE);
        if (wave_on) {
#pragma unroll
            for (int g0 = 0; g0 < kSeqE; g0 += kSeqGroup) {
                float xin[kSeqGroup];
                f4v d[kSeqGroup][JPW / 4];
#pragma unroll
                for (int g = 0; g < kSeqGroup; ++g) {
                    xin[g] = in_s[buf][g0 + g][lane];
#pragma unroll
                    for (int v = 0; v < JPW / 4; ++v) d[g][v] = *reinterpret_cast<const f4v *>(&dz_s[buf][g0 + g][wave * JPW + 4 * v]);
                }
#pragma unroll
                for (int q = 0; q < JPW; ++q) {
                    float G[kSeqGroup], na[kSeqGroup], upd[kSeqGroup];
#pragma unroll
                    for (int g = 0; g < kSeqGroup; ++g) {  // the serial part: the accumulator chain
                        G[g] = __fmul_rn(d[g][q >> 2][q & 3], xin[g]);
                        if (OPT != kSeqSgd) {
                            const float t2 = __fadd_rn(a[q], __fmul_rn(G[g], G[g]));
                            a[q] = G[g] != 0.0f ? t2 : a[q];
                        }
                        na[g] = a[q];
                    }
#pragma unroll
                    for (int g = 0; g < kSeqGroup; ++g) {  // the step sizes, independent of each other: the LUT reads are in flight together
                        if (OPT == kSeqSgd) {
                            upd[g] = __fmul_rn(G[g], p.rate);
                        } else if (OPT == kSeqFlex) {
                            upd[g] = __fmul_rn(__fmul_rn(G[g], p.rate), powf(na[g], p.minus_power_t));
                            if (isnan(upd[g]) || isinf(upd[g])) upd[g] = 0.0f;
                        } else {
                            upd[g] = __fmul_rn(G[g], lut_s[(__float_as_uint(na[g]) >> (31 - kLutBits)) & (uint32_t)(kLutSize - 1)]);  // (masked: see opt_step)
                        }
                    }
#pragma unroll
                    for (int g = 0; g < kSeqGroup; ++g) w[q] = G[g] != 0.0f ? __fsub_rn(w[q], upd[g]) : w[q];  // (a select: a LUT entry may be inf)
                }
            }
        }
        if (more) store(buf ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < JPW; ++q)
        if (own[q]) {
            p.w[at[q]] = w[q];
            if (OPT != kSeqSgd) p.acc[at[q]] = a[q];
        }
}

// The tiles of a step: one segment per hidden layer (dz_l against in_l) and one for the final neuron (gvec against [h_last | x]), workgroups numbered segment by segment
HeadSeqPlan head_seq_plan(const DevNN &nn, const float *x, float *const *h, float *const *dz, const float *gvec, uint32_t n, int tj) {
    HeadSeqPlan p{};
    const uint32_t L = nn.n_layers;
    auto aligned = [](const float *q, uint32_t width) { return width % 4 == 0 && ((uintptr_t)q & 15u) == 0; };
    uint32_t tile = 0;
    for (uint32_t l = 0; l <= L; l++) {
        HeadSeqSeg &s = p.seg[l];
        if (l < L) {
            s.dz = dz[l];
            s.ld_dz = s.rows = nn.out[l];
            s.src0 = l == 0 ? x : h[l - 1];
            s.w0 = nn.in[l];
        } else {
            s.dz = gvec;
            s.ld_dz = s.rows = 1;
            s.src0 = h[L - 1];
            s.w0 = nn.out[L - 1];
            if (nn.topology == 1) {
                s.src1 = x;
                s.w1 = nn.X;
            }
        }
        s.off = nn.off[l];
        s.vec = aligned(s.src0, s.w0) && (!s.w1 || aligned(s.src1, s.w1)) ? 1 : 0;
        s.tiles_i = (s.w0 + s.w1 + 1 + kSeqTI - 1) / kSeqTI;  // (+ 1: the bias column)
        s.tile0 = tile;
        tile += s.tiles_i * ((s.rows + tj - 1) / tj);
    }
    p.n_seg = L + 1;
    p.n_tiles = tile;
    p.n = n;
    p.w = nn.w;
    p.acc = nn.acc;
    p.lut = nn.lut;
    p.rate = nn.rate;
    p.minus_power_t = nn.minus_power_t;
    return p;
}

template <int TJ>
static hipError_t launch_tj(const HeadSeqPlan &p, int optimizer, hipStream_t s) {
    const dim3 grid(p.n_tiles), block(kSeqThreads);
    if (optimizer == FWGPU_OPT_SGD) hipLaunchKernelGGL((head_seq_kernel<kSeqSgd, TJ>), grid, block, 0, s, p);
    else if (optimizer == FWGPU_OPT_ADAGRAD_FLEX) hipLaunchKernelGGL((head_seq_kernel<kSeqFlex, TJ>), grid, block, 0, s, p);
    else if (optimizer == FWGPU_OPT_ADAGRAD_LUT) hipLaunchKernelGGL((head_seq_kernel<kSeqLut, TJ>), grid, block, 0, s, p);
    else return hipErrorInvalidValue;  // (no quiet fall-back: an optimizer this file does not know is an error)
    return hipGetLastError();
}

hipError_t launch_head_seq(const HeadSeqPlan &p, int optimizer, int tj, hipStream_t s) {
    if (!p.n || !p.n_tiles) return hipSuccess;
    if (tj == 16) return launch_tj<16>(p, optimizer, s);
    if (tj == 32) return launch_tj<32>(p, optimizer, s);
    return hipErrorInvalidValue;
}

}  // namespace fwgpu
