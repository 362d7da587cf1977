// The reference's weight_patcher (weight_patcher/src/main.rs) on the device: the byte diff of two inference weights sections that live in
// device memory, as the stream diff_stream.h states, and the scatter of such a stream into a packed regressor's tables.
//
// CONTRACT: the stream is that of the host codec (diff_stream.h encode) on the same bytes, byte for byte.
//
// THE DIFF is a variable-length stream compaction in three launches on one stream.  No kernel waits for another workgroup.
//   size pass   one workgroup per tile of kDiffTileBytes.  A wave owns a contiguous quarter of the tile and walks it in kDiffSteps steps of
//               64 lanes x 16 bytes (one 16-byte load of each input per lane and step).  Per tile: the number of differing bytes, the first
//               and last differing position, and the encoded size of all entries but the first, whose delta reaches into earlier tiles.
//   tile scan   one workgroup.  A lane owns a contiguous run of tiles, folds it, lane 0 chains the 1024 folds, and the lanes walk their
//               runs again: every tile gets its prev (the last differing index of the nearest earlier tile that has one, else the carried-in
//               prev_index) and, from the size of its first entry, its offset in the stream.  Positions and offsets are 64-bit.
//   emit pass   compares again (the walk of the size pass), places every lane's entries from the wave's scans and the tile's start, encodes
//               them into LDS at the stream's own 16-byte phase, and stores the tile's piece of the stream in 16-byte pieces; only the
//               piece's two ragged ends are stored byte by byte.
// Within a wave the "previous differing position before my bytes" is a ballot and one shuffle (the nearest lower lane that has a difference),
// the output offsets a 6-step shuffle scan; a step in which no lane of the wave differs -- nearly all of them between two publishes -- costs
// its two loads, a compare and the ballot.
// The tail of a section whose length is no multiple of 16 is loaded byte by byte; nothing beyond n is read.
#include <algorithm>
#include <cstring>

#include "diff_stream.h"
#include "fwgpu_internal.h"

namespace fwgpu {

static constexpr uint32_t kDiffWaves = kDiffThreads / 64;
static constexpr uint32_t kDiffStepBytes = 64 * kDiffLaneBytes;
// A tile's piece of the stream: its first entry is at most 11 bytes (a 10-byte varint and the byte), every later one has a delta below the
// tile's size, two bytes below 128 and three from there on, and the deltas sum to less than the tile's size: at most 2 bytes per tile byte.
// It is staged at the stream offset's phase within 16 bytes, so up to 15 bytes lie before it.
static constexpr uint32_t kDiffStage = ((11 + 2 * kDiffTileBytes + 15) + 15) / 16 * 16;
static_assert(kDiffTileBytes <= 16384, "deltas within a tile must fit a two-byte varint");
static_assert(kDiffLaneBytes == 16, "a lane compares one uint4 of each input per step");

__device__ __forceinline__ uint32_t dev_varint_len(unsigned long long v) { return (64 - __clzll((long long)(v | 1)) + 6) / 7; }

// 16 bytes at pos, those at or beyond n as zeros: they compare equal and are never read
__device__ __forceinline__ uint4 diff_load(const uint8_t *__restrict__ p, unsigned long long pos, unsigned long long n) {
    if (pos + kDiffLaneBytes <= n) return *reinterpret_cast<const uint4 *>(p + pos);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t i = 0; i < kDiffLaneBytes; i++)
        if (pos + i < n) w[i >> 2] |= (uint32_t)p[pos + i] << (8 * (i & 3));
    return uint4{w[0], w[1], w[2], w[3]};
}

__device__ __forceinline__ uint32_t diff_mask4(uint32_t x) {  // bit i: byte i of x is not zero
    return (uint32_t)((x & 0xffu) != 0) | ((uint32_t)((x & 0xff00u) != 0) << 1) | ((uint32_t)((x & 0xff0000u) != 0) << 2) |
           ((uint32_t)((x & 0xff000000u) != 0) << 3);
}

// What a wave knows after walking its quarter of a tile.  Positions are relative to the tile's first byte.
struct WaveWalk {
    // per lane and step
    uint32_t mask[kDiffSteps];  // bit i: byte i of the lane's 16 differs
    uint4 to[kDiffSteps];       // the second input's 16 bytes
    int32_t prev[kDiffSteps];   // the last differing position before the lane's bytes within the wave, -1: none
    uint32_t off[kDiffSteps];   // encoded bytes of the wave's entries before the lane's, the wave's first entry counted as 0 bytes
    // wave-uniform: the wave's DiffTile
    uint32_t count, rest;
    int32_t first, last;
};

__device__ __forceinline__ void wave_walk(const DiffArgs &d, unsigned long long tile_pos, uint32_t wave, uint32_t lane, WaveWalk &w) {
    int32_t carry_last = -1, first = -1;
    uint32_t carry_size = 0, cnt = 0;
#pragma unroll
    for (uint32_t s = 0; s < kDiffSteps; s++) {
        const uint32_t rel = wave * kDiffWaveBytes + s * kDiffStepBytes + lane * kDiffLaneBytes;
        const unsigned long long pos = tile_pos + rel;
        const uint4 va = diff_load(d.a, pos, d.n), vb = diff_load(d.b, pos, d.n);
        const uint32_t m = diff_mask4(va.x ^ vb.x) | (diff_mask4(va.y ^ vb.y) << 4) | (diff_mask4(va.z ^ vb.z) << 8) | (diff_mask4(va.w ^ vb.w) << 12);
        w.mask[s] = m;
        w.to[s] = vb;
        w.prev[s] = carry_last;
        w.off[s] = carry_size;
        const unsigned long long bal = __ballot(m != 0);
        if (!bal) continue;  // (wave-uniform)
        const int32_t lo = (int32_t)rel + (m ? __ffs((int)m) - 1 : 0), hi = (int32_t)rel + (m ? 31 - __clz((int)m) : 0);
        const unsigned long long below = bal & ((1ull << lane) - 1);
        const int32_t got = __shfl(hi, below ? 63 - __clzll((long long)below) : (int)lane, 64);
        const int32_t p = below ? got : carry_last;
        const uint32_t sz = m ? 2 * (__popc(m) - 1) + (p >= 0 ? dev_varint_len((unsigned long long)(lo - p)) + 1 : 0) : 0;
        uint32_t incl = sz;
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        w.prev[s] = p;
        w.off[s] = carry_size + incl - sz;
        if (carry_last < 0) first = __shfl(lo, __ffsll((unsigned long long)bal) - 1, 64);
        carry_last = __shfl(hi, 63 - __clzll((long long)bal), 64);
        carry_size += __shfl(incl, 63, 64);
        cnt += __popc(m);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    w.count = cnt;
    w.rest = carry_size;
    w.first = first;
    w.last = carry_last;
}

__global__ __launch_bounds__(kDiffThreads) void diff_size_kernel(DiffArgs d) {
    __shared__ DiffTile s_agg[kDiffWaves];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long tile = blockIdx.x;
    WaveWalk w;
    wave_walk(d, tile * kDiffTileBytes, wave, lane, w);
    if (lane == 0) s_agg[wave] = DiffTile{w.count, (uint32_t)w.first, (uint32_t)w.last, w.rest};
    __syncthreads();
    if (threadIdx.x == 0) {
        DiffTile t{0, 0, 0, 0};
        for (uint32_t i = 0; i < kDiffWaves; i++) {
            const DiffTile g = s_agg[i];
            if (!g.count) continue;
            if (!t.count) {
                t.first = g.first;
                t.rest = g.rest;
            } else {
                t.rest += g.rest + dev_varint_len(g.first - t.last) + 1;
            }
            t.last = g.last;
            t.count += g.count;
        }
        d.tiles[tile] = t;
    }
}

__global__ __launch_bounds__(kDiffScanThreads) void diff_scan_kernel(DiffArgs d) {
    __shared__ unsigned long long s_first[kDiffScanThreads], s_last[kDiffScanThreads], s_size[kDiffScanThreads], s_count[kDiffScanThreads];
    const uint32_t tid = threadIdx.x;
    const unsigned long long run = (d.n_tiles + kDiffScanThreads - 1) / kDiffScanThreads;
    const unsigned long long lo = tid * run < d.n_tiles ? tid * run : d.n_tiles, hi = lo + run < d.n_tiles ? lo + run : d.n_tiles;
    unsigned long long first = 0, last = 0, size = 0, count = 0;
    for (unsigned long long t = lo; t < hi; t++) {  // the run folded: its first and last entry, the size of all but the first
        const DiffTile g = d.tiles[t];
        if (!g.count) continue;
        const unsigned long long at = d.base_offset + t * kDiffTileBytes;
        if (!count) {
            first = at + g.first;
            size = g.rest;
        } else {
            size += dev_varint_len(at + g.first - last) + 1 + g.rest;
        }
        last = at + g.last;
        count += g.count;
    }
    s_first[tid] = first;
    s_last[tid] = last;
    s_size[tid] = size;
    s_count[tid] = count;
    __syncthreads();
    if (tid == 0) {  // the folds chained: every run's prev and offset in place of its first and size
        unsigned long long prev = d.prev_index, off = 0, cnt = 0;
        for (uint32_t i = 0; i < kDiffScanThreads; i++) {
            const unsigned long long f = s_first[i], sz = s_size[i];
            s_first[i] = prev;
            s_size[i] = off;
            if (!s_count[i]) continue;
            off += dev_varint_len(f - prev) + 1 + sz;
            prev = s_last[i];
            cnt += s_count[i];
        }
        d.totals[0] = off;
        d.totals[1] = cnt;
    }
    __syncthreads();
    unsigned long long prev = s_first[tid], off = s_size[tid];
    for (unsigned long long t = lo; t < hi; t++) {
        d.starts[t] = DiffTileStart{prev, off};
        const DiffTile g = d.tiles[t];
        if (!g.count) continue;
        const unsigned long long at = d.base_offset + t * kDiffTileBytes;
        off += dev_varint_len(at + g.first - prev) + 1 + g.rest;
        prev = at + g.last;
    }
}

__device__ __forceinline__ uint32_t diff_byte(const uint4 &v, uint32_t i) {
    const uint32_t word = i < 8 ? (i < 4 ? v.x : v.y) : (i < 12 ? v.z : v.w);
    return (word >> (8 * (i & 3))) & 0xffu;
}

__global__ __launch_bounds__(kDiffThreads) void diff_emit_kernel(DiffArgs d) {
    __shared__ DiffTile s_agg[kDiffWaves];
    __shared__ __align__(16) uint8_t s_out[kDiffStage];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long tile = blockIdx.x;
    WaveWalk w;
    wave_walk(d, tile * kDiffTileBytes, wave, lane, w);
    if (lane == 0) s_agg[wave] = DiffTile{w.count, (uint32_t)w.first, (uint32_t)w.last, w.rest};
    __syncthreads();
    // where this wave's entries begin in the tile's piece, and the entry before them
    const DiffTileStart start = d.starts[tile];
    const unsigned long long tile_at = d.base_offset + tile * kDiffTileBytes;
    unsigned long long prev = start.prev, my_prev = 0;
    uint32_t total = 0, my_base = 0, my_first_size = 0;
#pragma unroll
    for (uint32_t i = 0; i < kDiffWaves; i++) {
        const DiffTile g = s_agg[i];
        const uint32_t first_size = g.count ? dev_varint_len(tile_at + g.first - prev) + 1 : 0;
        if (i == wave) {
            my_prev = prev;
            my_base = total;
            my_first_size = first_size;
        }
        if (!g.count) continue;
        total += first_size + g.rest;
        prev = tile_at + g.last;
    }
    if (!total) return;  // (uniform: nothing differs in this tile)
    const uint32_t phase = (uint32_t)(start.out & 15);
    if (phase + total > kDiffStage || start.out + total > d.totals[0]) return;  // (uniform; the passes disagree: write nothing rather than out of bounds)
#pragma unroll
    for (uint32_t s = 0; s < kDiffSteps; s++) {
        uint32_t m = w.mask[s];
        if (!m) continue;
        const uint32_t rel = wave * kDiffWaveBytes + s * kDiffStepBytes + lane * kDiffLaneBytes;
        uint32_t bit = __ffs((int)m) - 1;
        uint32_t o = phase + my_base + w.off[s] + (w.prev[s] >= 0 ? my_first_size : 0);
        unsigned long long delta = w.prev[s] >= 0 ? (unsigned long long)((int32_t)(rel + bit) - w.prev[s]) : tile_at + rel + bit - my_prev;
        while (delta >= 0x80) {
            s_out[o++] = (uint8_t)(delta & 0x7f) | 0x80;
            delta >>= 7;
        }
        s_out[o++] = (uint8_t)delta;
        s_out[o++] = (uint8_t)diff_byte(w.to[s], bit);
        for (m &= m - 1; m; m &= m - 1) {  // the lane's further entries: deltas below 16, one byte each
            const uint32_t next = __ffs((int)m) - 1;
            s_out[o++] = (uint8_t)(next - bit);
            s_out[o++] = (uint8_t)diff_byte(w.to[s], next);
            bit = next;
        }
    }
    __syncthreads();
    // s_out[phase .. phase + total) -> out[start.out ..): LDS byte i goes to out[start.out - phase + i], so 16-byte pieces keep their alignment
    uint8_t *dst = d.out + (start.out - phase);
    const uint32_t end = phase + total;
    for (uint32_t at = threadIdx.x * 16; at < end; at += kDiffThreads * 16) {
        if (at >= phase && at + 16 <= end) {
            *reinterpret_cast<uint4 *>(dst + at) = *reinterpret_cast<const uint4 *>(s_out + at);
        } else {
            for (uint32_t i = at < phase ? phase : at; i < at + 16 && i < end; i++) dst[i] = s_out[i];
        }
    }
}

static bool diff_args_ok(const DiffArgs &d) {
    return d.n_tiles == (d.n + kDiffTileBytes - 1) / kDiffTileBytes && d.n_tiles <= 0x7fffffffull && d.prev_index <= d.base_offset && d.a && d.b &&
           d.tiles && d.starts && d.totals && (reinterpret_cast<uintptr_t>(d.a) & 15) == 0 && (reinterpret_cast<uintptr_t>(d.b) & 15) == 0;
}

hipError_t launch_diff_size(const DiffArgs &d, hipStream_t stream) {
    if (!d.n_tiles) return hipSuccess;
    if (!diff_args_ok(d)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(diff_size_kernel, dim3((uint32_t)d.n_tiles), dim3(kDiffThreads), 0, stream, d);
    return hipGetLastError();
}

hipError_t launch_diff_scan(const DiffArgs &d, hipStream_t stream) {
    if (!d.n_tiles) return hipSuccess;
    if (!diff_args_ok(d)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(diff_scan_kernel, dim3(1), dim3(kDiffScanThreads), 0, stream, d);
    return hipGetLastError();
}

hipError_t launch_diff_emit(const DiffArgs &d, hipStream_t stream) {
    if (!d.n_tiles) return hipSuccess;
    if (!diff_args_ok(d) || !d.out || (reinterpret_cast<uintptr_t>(d.out) & 15)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(diff_emit_kernel, dim3((uint32_t)d.n_tiles), dim3(kDiffThreads), 0, stream, d);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void patch_scatter_kernel(PatchArgs p) {
    const unsigned long long stride = (unsigned long long)gridDim.x * 256;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < p.n; i += stride) {
        const unsigned long long j = p.index[i];
        const uint8_t v = p.to[i];
        // bytes are stored as bytes: two entries of one word may be on different lanes
        if (j < p.lr_bytes)
            p.lr[(j >> 2) * 8 + (j & 3)] = v;  // the weight half of the {w, acc} pair
        else if (j >= p.q_at && j - p.q_at < p.q_bytes)
            p.q[j - p.q_at] = v;
    }
}

hipError_t launch_patch_scatter(const PatchArgs &p, hipStream_t stream) {
    if (!p.n) return hipSuccess;
    if (!p.index || !p.to || !p.lr || !p.q) return hipErrorInvalidValue;
    const uint32_t grid = (uint32_t)std::min<unsigned long long>((p.n + 255) / 256, 4096);
    hipLaunchKernelGGL(patch_scatter_kernel, dim3(grid), dim3(256), 0, stream, p);
    return hipGetLastError();
}

namespace {

// the device buffers of one diff: tile records, tile starts, the totals; the stream once its size is known
struct DiffRun {
    DiffArgs d{};
    void *ws = nullptr;
    uint8_t *d_out = nullptr;
    ~DiffRun() {
        (void)hipFree(ws);
        (void)hipFree(d_out);
    }
    int prepare(const uint8_t *d_a, const uint8_t *d_b, uint64_t n, uint64_t base_offset, uint64_t prev_index) {
        if (prev_index > base_offset) return fail(FWGPU_ERR_INVALID, "diff: prev_index lies beyond base_offset");
        if (base_offset > UINT64_MAX - n) return fail(FWGPU_ERR_INVALID, "diff: base_offset + n does not fit 64 bits");
        d.a = d_a;
        d.b = d_b;
        d.n = n;
        d.base_offset = base_offset;
        d.prev_index = prev_index;
        d.n_tiles = (n + kDiffTileBytes - 1) / kDiffTileBytes;
        if (!d.n_tiles) return FWGPU_OK;
        if (d.n_tiles > 0x7fffffffull) return fail(FWGPU_ERR_RANGE, "diff: more tiles than one launch's workgroups");
        const size_t bytes = 16 + d.n_tiles * (sizeof(DiffTile) + sizeof(DiffTileStart));
        if (hipMalloc(&ws, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(FWGPU_ERR_OOM, "diff: no device memory for the tile records");
        }
        d.totals = static_cast<unsigned long long *>(ws);
        d.starts = reinterpret_cast<DiffTileStart *>(static_cast<uint8_t *>(ws) + 16);
        d.tiles = reinterpret_cast<DiffTile *>(d.starts + d.n_tiles);
        return FWGPU_OK;
    }
    int alloc_out(uint64_t bytes) {
        if (hipMalloc((void **)&d_out, bytes + 16) != hipSuccess) {
            (void)hipGetLastError();
            return fail(FWGPU_ERR_OOM, "diff: no device memory for the stream");
        }
        d.out = d_out;
        return FWGPU_OK;
    }
};

// two device arrays -> the stream in host memory (two-call protocol); the current device is the arrays'
int diff_on_device(const uint8_t *d_a, const uint8_t *d_b, uint64_t n, uint64_t base_offset, uint64_t prev_index, uint8_t *out, uint64_t cap,
                   uint64_t *written, uint64_t *changed) {
    DiffRun run;
    int rc = run.prepare(d_a, d_b, n, base_offset, prev_index);
    if (rc) return rc;
    unsigned long long totals[2] = {0, 0};
    if (run.d.n_tiles) {
        FWGPU_HIP(launch_diff_size(run.d, 0));
        FWGPU_HIP(launch_diff_scan(run.d, 0));
        FWGPU_HIP(hipMemcpy(totals, run.d.totals, sizeof totals, hipMemcpyDeviceToHost));
    }
    *written = totals[0];
    if (changed) *changed = totals[1];
    if (!out || cap < totals[0]) return fail(FWGPU_ERR_RANGE, "diff: buffer too small for the stream");
    if (!totals[0]) return FWGPU_OK;
    if ((rc = run.alloc_out(totals[0]))) return rc;
    FWGPU_HIP(launch_diff_emit(run.d, 0));
    FWGPU_HIP(hipMemcpy(out, run.d_out, totals[0], hipMemcpyDeviceToHost));
    return FWGPU_OK;
}

}  // namespace
}  // namespace fwgpu

using namespace fwgpu;

extern "C" {

int fwgpu_diff_bytes(const uint8_t *a, const uint8_t *b, uint64_t n, uint64_t base_offset, uint64_t prev_index, uint8_t *out, uint64_t cap,
                     uint64_t *written, uint64_t *changed) {
    if ((n && (!a || !b)) || !written) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (prev_index > base_offset) return fail(FWGPU_ERR_INVALID, "diff_bytes: prev_index lies beyond base_offset");
    *written = diffstream::encode(a, b, n, base_offset, prev_index, out, out ? cap : 0, changed, nullptr);
    if (!out || cap < *written) return fail(FWGPU_ERR_RANGE, "diff_bytes: buffer too small for the stream");
    return FWGPU_OK;
}

int fwgpu_diff_apply_bytes(uint8_t *target, uint64_t n, uint64_t base_offset, const uint8_t *diff, uint64_t len, uint64_t *applied) {
    if ((n && !target) || (len && !diff)) return fail(FWGPU_ERR_INVALID, "NULL argument");
    const int st = diffstream::apply(target, n, base_offset, diff, len, applied);
    if (st) return fail(FWGPU_ERR_FORMAT, std::string("diff_apply_bytes: ") + diffstream::status_text(st));
    return FWGPU_OK;
}

int fwgpu_image_diff(const fwgpu_image *base, const fwgpu_image *next, uint8_t *out, uint64_t cap, uint64_t *written, uint64_t *changed) {
    if (!base || !next || !written) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (base->device != next->device) return fail(FWGPU_ERR_INVALID, "image_diff: the images are on different devices");
    if (base->header.size() != next->header.size() || base->weights_bytes != next->weights_bytes)
        return fail(FWGPU_ERR_INVALID, "image_diff: the images have different lengths");
    // the headers on the host (they are usually identical), then the weights sections on the device from where the header's stream ends
    const uint64_t hb = base->header.size();
    std::vector<uint8_t> head(2 * hb + 16);
    uint64_t head_changed = 0, last = 0;
    const uint64_t head_size = diffstream::encode(base->header.data(), next->header.data(), hb, 0, 0, head.data(), head.size(), &head_changed, &last);
    if (head_size > head.size()) return fail(FWGPU_ERR_RANGE, "image_diff: header stream");  // (at most 2 bytes per byte and one long delta)
    FWGPU_HIP(hipSetDevice(base->device));
    const bool fits = out && cap >= head_size;
    uint64_t body = 0, body_changed = 0;
    const int rc = diff_on_device(base->d_weights, next->d_weights, base->weights_bytes, hb, last, fits ? out + head_size : nullptr, fits ? cap - head_size : 0,
                                  &body, &body_changed);
    *written = head_size + body;
    if (changed) *changed = head_changed + body_changed;
    if (rc) return rc;
    memcpy(out, head.data(), head_size);
    return FWGPU_OK;
}

int fwgpu_debug_diff(int device, const uint8_t *a, const uint8_t *b, uint64_t n, uint64_t base_offset, uint64_t prev_index, uint8_t *out,
                     uint64_t cap, uint64_t *written, uint64_t *changed) {
    if ((n && (!a || !b)) || !written) return fail(FWGPU_ERR_INVALID, "NULL argument");
    FWGPU_HIP(hipSetDevice(device));
    uint8_t *d_ab = nullptr;  // both arrays in one allocation, the second on a 16-byte boundary
    const uint64_t pitch = (n + 15) / 16 * 16;
    if (n) {
        FWGPU_HIP(hipMalloc((void **)&d_ab, 2 * pitch));
        hipError_t e = hipMemcpy(d_ab, a, n, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_ab + pitch, b, n, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d_ab);
            return fail(FWGPU_ERR_DEVICE, std::string("debug_diff: ") + hipGetErrorString(e));
        }
    }
    const int rc = diff_on_device(d_ab, d_ab + pitch, n, base_offset, prev_index, out, cap, written, changed);
    (void)hipFree(d_ab);
    return rc;
}

int fwgpu_debug_diff_geometry(uint32_t *tile_bytes) {
    if (!tile_bytes) return fail(FWGPU_ERR_INVALID, "NULL argument");
    *tile_bytes = kDiffTileBytes;
    return FWGPU_OK;
}

int fwgpu_debug_diff_rates(const fwgpu_image *base, const fwgpu_image *next, float *ms4) {
    if (!base || !next || !ms4) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (base->device != next->device || base->header.size() != next->header.size() || base->weights_bytes != next->weights_bytes || !base->weights_bytes)
        return fail(FWGPU_ERR_INVALID, "debug_diff_rates: two images of one length on one device");
    FWGPU_HIP(hipSetDevice(base->device));
    FWGPU_HIP(hipDeviceSynchronize());
    DiffRun run;
    int rc = run.prepare(base->d_weights, next->d_weights, base->weights_bytes, base->header.size(), 0);
    if (rc) return rc;
    void *copy = nullptr;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    unsigned long long totals[2] = {0, 0};
    hipError_t e = hipMalloc(&copy, base->weights_bytes);
    for (int i = 0; i < 6 && e == hipSuccess; i++) e = hipEventCreate(&ev[i]);
    if (e == hipSuccess) e = hipEventRecord(ev[0], 0);
    if (e == hipSuccess) e = launch_diff_size(run.d, 0);
    if (e == hipSuccess) e = hipEventRecord(ev[1], 0);
    if (e == hipSuccess) e = launch_diff_scan(run.d, 0);
    if (e == hipSuccess) e = hipEventRecord(ev[2], 0);
    if (e == hipSuccess) e = hipMemcpy(totals, run.d.totals, sizeof totals, hipMemcpyDeviceToHost);
    if (e == hipSuccess && hipMalloc((void **)&run.d_out, totals[0] + 16) != hipSuccess) e = hipErrorOutOfMemory;
    run.d.out = run.d_out;
    if (e == hipSuccess) e = hipEventRecord(ev[3], 0);  // (the device was idle while the host read the totals)
    if (e == hipSuccess) e = launch_diff_emit(run.d, 0);
    if (e == hipSuccess) e = hipEventRecord(ev[4], 0);
    if (e == hipSuccess) e = hipMemcpyAsync(copy, base->d_weights, base->weights_bytes, hipMemcpyDeviceToDevice, 0);
    if (e == hipSuccess) e = hipEventRecord(ev[5], 0);
    if (e == hipSuccess) e = hipEventSynchronize(ev[5]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms4[0], ev[0], ev[1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms4[1], ev[1], ev[2]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms4[2], ev[3], ev[4]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms4[3], ev[4], ev[5]);
    for (int i = 0; i < 6; i++)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    (void)hipFree(copy);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(FWGPU_ERR_DEVICE, std::string("debug_diff_rates: ") + hipGetErrorString(e));
    }
    return FWGPU_OK;
}

int fwgpu_packed_apply_diff(fwgpu_regressor *r, const uint8_t *diff, uint64_t len, uint64_t *applied) {
    if (!r || (len && !diff)) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (applied) *applied = 0;
    if (!r->packed()) return fail(FWGPU_ERR_INVALID, "packed_apply_diff: the regressor's FFM weights are f32, not the file's f16 buckets: a byte diff of two inference files does not apply to it");
    if (r->file_quantized_at_load)
        return fail(FWGPU_ERR_INVALID, "packed_apply_diff: the regressor's file was quantised at load: its buckets are not the file's bytes");
    if (!r->file_header_bytes)
        return fail(FWGPU_ERR_INVALID, "packed_apply_diff: the regressor has no inference file behind it (made by fwgpu_pack_regressor: refresh it with that call; or loaded from a file that carries optimizer state)");
    // the file: header | LR weights (f32) | {increment, min} | buckets
    const uint64_t hb = r->file_header_bytes, lr_bytes = r->lr_len * 4, q_at = lr_bytes + 8, q_bytes = r->ffm_len * 2;
    const uint64_t file_bytes = hb + q_at + q_bytes;
    uint64_t entries = 0, in_header = 0;
    int st = diffstream::walk(diff, len, file_bytes, [&](uint64_t index, uint8_t) { in_header += index < hb; }, &entries);
    if (st) return fail(FWGPU_ERR_FORMAT, std::string("packed_apply_diff: ") + diffstream::status_text(st));
    if (in_header) return fail(FWGPU_ERR_INVALID, "packed_apply_diff: the model's header changed: load the file");
    if (!entries) return FWGPU_OK;
    uint8_t q_header[8];
    memcpy(q_header, &r->q_increment, 4);
    memcpy(q_header + 4, &r->q_min, 4);
    std::vector<unsigned long long> index;
    std::vector<uint8_t> to;
    index.reserve(entries);
    to.reserve(entries);
    diffstream::walk(diff, len, file_bytes, [&](uint64_t at, uint8_t v) {
        const uint64_t j = at - hb;
        if (j >= lr_bytes && j < q_at) {
            q_header[j - lr_bytes] = v;
        } else {
            index.push_back(j);
            to.push_back(v);
        }
    });
    FWGPU_HIP(hipSetDevice(r->device));
    FWGPU_HIP(hipDeviceSynchronize());
    if (!index.empty()) {
        // one allocation: the indices, then the bytes
        uint8_t *d_entries = nullptr;
        const size_t n = index.size();
        if (hipMalloc((void **)&d_entries, n * 9) != hipSuccess) {
            (void)hipGetLastError();
            return fail(FWGPU_ERR_OOM, "packed_apply_diff: no device memory for the entries");
        }
        PatchArgs p{};
        p.index = reinterpret_cast<const unsigned long long *>(d_entries);
        p.to = d_entries + n * 8;
        p.n = n;
        p.lr_bytes = lr_bytes;
        p.q_at = q_at;
        p.q_bytes = q_bytes;
        p.lr = reinterpret_cast<uint8_t *>(r->d_lr);
        p.q = reinterpret_cast<uint8_t *>(r->d_ffm_q);
        hipError_t e = hipMemcpy(d_entries, index.data(), n * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_entries + n * 8, to.data(), n, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = launch_patch_scatter(p, 0);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        (void)hipFree(d_entries);
        if (e != hipSuccess) return fail(FWGPU_ERR_DEVICE, std::string("packed_apply_diff: ") + hipGetErrorString(e));
    }
    memcpy(&r->q_increment, q_header, 4);
    memcpy(&r->q_min, q_header + 4, 4);
    r->weights_epoch++;  // (context caches set up before, fwgpu_packed_enable_caches, are stale from here on)
    if (applied) *applied = entries;
    return FWGPU_OK;
}

}  // extern "C"
