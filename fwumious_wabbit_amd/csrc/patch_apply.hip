// The reader of a byte-diff stream (diff_stream.h walk) on the device: the raw stream is uploaded, decoded by three launches on one stream and
// stored into an image's weights section, a packed regressor's tables or a pair of debug arrays.  No kernel waits for another workgroup and
// nothing is added atomically: two runs give the same bytes.
//
// CONTRACT: the status is diffstream::walk's on the same bytes, code for code, and nothing is stored unless it is kOk.
//
// WHY IT IS PARALLEL.  Call a byte a `to` byte or a varint byte.  A byte with its top bit set leaves the reader expecting a varint byte; a byte
// with its top bit clear flips what it expects.  So byte i is a `to` byte exactly when the run of top-bit-clear bytes that ends at i - 1 has
// odd length (tests/test_diff_decode_rule_cpu.py).  An entry is the varint bytes between two `to` bytes and the second of them.
//
//   summary pass  one workgroup per tile of kDecTileBytes, staged in LDS.  A lane owns a slot of 16 bytes per step (one uint4 load; the ragged
//                 tail byte by byte).  A slot that holds a top-bit-set byte fixes the reader's state behind it, so the state in front of a slot
//                 is that of the nearest lower such slot (a ballot and a shuffle within a wave, one LDS byte per wave and step across them), or
//                 the tile's own start state.  That one is unknown here -- a stream with no top bit set anywhere carries it through every tile --
//                 so the pass keeps BOTH hypotheses: per start state the number of `to` bytes, the first one's position, the bytes left
//                 pending behind the last one, the state at the tile's end, and the saturating 64-bit sum of the deltas of all entries but the
//                 tile's first, up to the first of them that is faulty, with that fault's status.
//                 The first entry is left out because where its varint starts cannot be told from a halo: in  c c c S | c t  the byte S is
//                 a `to` byte >= 128 or the first byte of a two-byte varint, by the parity of a clear run of any length in front of it.
//   tile scan     one workgroup.  A lane owns a contiguous run of tiles.  (1) The runs are folded as maps {start state} -> {end state, pending
//                 bytes} and lane 0 chains the folds, which resolves every tile's start state and the bytes of its first entry that lie in
//                 earlier tiles.  (2) The lanes walk their runs with that knowledge, decode every tile's first entry from global memory (at
//                 most 10 bytes) and sum counts and deltas; lane 0 chains those.  (3) The lanes walk once more and give every tile its first
//                 entry's ordinal and the index before it, and find the run's first fault: indices only ascend, so "some entry of this tile
//                 lies at or beyond the end" is decided by the tile's last index before its first other fault.  The first fault in tile
//                 order is the stream's; a partial entry behind the last `to` byte is judged last.
//   apply pass    launched only when the scan says kOk.  Decodes the tile again with its known start state, places every entry by two wave
//                 scans (ordinals, and deltas in 64 bits) and stores its `to` byte through a small target map.  Indices ascend strictly, so every
//                 target byte has one writer.
#include <algorithm>
#include <cstring>

#include "diff_stream.h"
#include "fwgpu_internal.h"

namespace fwgpu {

static constexpr uint32_t kDecWaves = kDecThreads / 64;
static constexpr uint32_t kDecSlots = kDecTileBytes / 16;   // slot k: the tile's bytes [16 k, 16 k + 16)
static constexpr uint32_t kDecChunks = kDecSlots / 64;      // a chunk: the 64 slots one wave walks in one step
static constexpr uint32_t kDecOpen = 2;                     // "the state in front of this slot is the tile's start state"
static constexpr uint32_t kDecNoFault = 0xffffffffu;
static constexpr uint32_t kDecPendCap = 255;                // pending bytes saturate here; from 11 on the varint is too long whatever follows
static constexpr unsigned long long kU64Max = ~0ull;
static_assert(kDecTileBytes < (1u << 28), "a fault's position and status share 32 bits");

__device__ __forceinline__ unsigned long long sat_add(unsigned long long a, unsigned long long b) { return a > kU64Max - b ? kU64Max : a + b; }

__device__ __forceinline__ uint32_t top_bits4(uint32_t x) { return ((x >> 7) & 1u) | ((x >> 14) & 2u) | ((x >> 21) & 4u) | ((x >> 28) & 8u); }

// The reader's walk over one slot: h the top bits of its n bytes, state what the reader expects in front of it (1: a `to` byte).
// Returns the mask of `to` bytes; state becomes the one behind the slot.
__device__ __forceinline__ uint32_t walk_slot(uint32_t h, uint32_t n, uint32_t &state) {
    uint32_t to = 0;
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) {
        if (i >= n) break;
        to |= state << i;
        state = ((h >> i) & 1u) ? 0u : state ^ 1u;
    }
    return to;
}

// A varint of n <= 10 bytes (read by at(i)): kOk or kVarint, the value in delta
template <class At>
__device__ __forceinline__ uint32_t read_varint(uint32_t n, At &&at, unsigned long long &delta) {
    delta = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t v = at(i) & 0x7fu;
        if (i == 9 && v > 1) return diffstream::kVarint;  // bit 63 is the last that fits
        delta |= (unsigned long long)v << (7 * i);
    }
    return diffstream::kOk;
}

// What a workgroup knows of its tile after staging it: the `to` masks of every slot under both start states
struct TileMasks {
    uint32_t len;                  // the tile's bytes
    uint32_t to[kDecSteps][2];     // per step of this lane and start state: the `to` bytes of the slot
    uint32_t first[2], last[2];    // per start state: the tile's first and last `to` position, kDecNoFault: none
    uint32_t count[2];
    uint32_t end_state[2];
};

struct DecShared {
    __align__(16) uint8_t bytes[kDecTileBytes];
    uint16_t to[2][kDecSlots];
    uint8_t chunk[kDecChunks];     // the state behind the chunk: 0, 1, or kDecOpen when no byte of it has its top bit set
    uint32_t end_state[2];
    uint32_t red_u32[kDecWaves][6];
    unsigned long long red_u64[kDecWaves][2];
    unsigned long long chunk_sum[kDecChunks];
    uint32_t chunk_cnt[kDecChunks];
};

__device__ __forceinline__ void tile_masks(const DecArgs &d, unsigned long long tile, DecShared &sh, TileMasks &m) {
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned long long tile_at = tile * kDecTileBytes;
    m.len = (uint32_t)std::min<unsigned long long>(kDecTileBytes, d.len - tile_at);
    uint32_t h[kDecSteps], nb[kDecSteps], trail[kDecSteps];
    unsigned long long bal[kDecSteps];
#pragma unroll
    for (uint32_t s = 0; s < kDecSteps; s++) {
        const uint32_t slot = s * kDecThreads + tid, rel = slot * 16;
        nb[s] = rel >= m.len ? 0 : std::min<uint32_t>(16, m.len - rel);
        uint4 v{0, 0, 0, 0};
        if (nb[s] == 16) {
            v = *reinterpret_cast<const uint4 *>(d.stream + tile_at + rel);
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (uint32_t i = 0; i < nb[s]; i++) w[i >> 2] |= (uint32_t)d.stream[tile_at + rel + i] << (8 * (i & 3));
            v = uint4{w[0], w[1], w[2], w[3]};
        }
        *reinterpret_cast<uint4 *>(sh.bytes + rel) = v;
        h[s] = top_bits4(v.x) | (top_bits4(v.y) << 4) | (top_bits4(v.z) << 8) | (top_bits4(v.w) << 12);
        // behind the slot's last top-bit-set byte the reader expects a varint byte; every clear byte after it flips that
        trail[s] = h[s] ? (nb[s] - 1 - (31 - __clz((int)h[s]))) & 1u : 0;
        bal[s] = __ballot(h[s] != 0);
        const uint32_t behind = bal[s] ? __shfl(trail[s], 63 - __clzll((long long)bal[s]), 64) : kDecOpen;
        if (lane == 0) sh.chunk[s * kDecWaves + wave] = (uint8_t)behind;
    }
    __syncthreads();
    uint32_t first[2] = {kDecNoFault, kDecNoFault}, last[2] = {0, 0}, count[2] = {0, 0};  // (last: position + 1, 0: none)
#pragma unroll
    for (uint32_t s = 0; s < kDecSteps; s++) {
        const uint32_t slot = s * kDecThreads + tid, rel = slot * 16;
        uint32_t in = kDecOpen;  // the state in front of this wave's chunk: behind the nearest lower chunk that fixes one
        for (int c = (int)(s * kDecWaves + wave) - 1; c >= 0 && in == kDecOpen; c--) in = sh.chunk[c];
        const unsigned long long below = bal[s] & ((1ull << lane) - 1);
        const uint32_t got = __shfl(trail[s], below ? 63 - __clzll((long long)below) : (int)lane, 64);
        const uint32_t front = below ? got : in;
#pragma unroll
        for (uint32_t hyp = 0; hyp < 2; hyp++) {
            uint32_t state = front == kDecOpen ? hyp : front;
            const uint32_t to = walk_slot(h[s], nb[s], state);
            m.to[s][hyp] = to;
            sh.to[hyp][slot] = (uint16_t)to;
            if (nb[s] && rel + nb[s] == m.len) sh.end_state[hyp] = state;  // (the slot that holds the tile's last byte)
            if (to) {
                first[hyp] = std::min(first[hyp], rel + (uint32_t)__ffs((int)to) - 1);
                last[hyp] = std::max(last[hyp], rel + 32 - (uint32_t)__clz((int)to));
                count[hyp] += __popc(to);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (uint32_t hyp = 0; hyp < 2; hyp++) {
            first[hyp] = std::min(first[hyp], (uint32_t)__shfl_xor(first[hyp], o, 64));
            last[hyp] = std::max(last[hyp], (uint32_t)__shfl_xor(last[hyp], o, 64));
            count[hyp] += __shfl_xor(count[hyp], o, 64);
        }
    }
    if (lane == 0)
        for (uint32_t hyp = 0; hyp < 2; hyp++) {
            sh.red_u32[wave][hyp * 3] = first[hyp];
            sh.red_u32[wave][hyp * 3 + 1] = last[hyp];
            sh.red_u32[wave][hyp * 3 + 2] = count[hyp];
        }
    __syncthreads();
    for (uint32_t hyp = 0; hyp < 2; hyp++) {
        m.first[hyp] = kDecNoFault;
        m.last[hyp] = 0;
        m.count[hyp] = 0;
        for (uint32_t w = 0; w < kDecWaves; w++) {
            m.first[hyp] = std::min(m.first[hyp], sh.red_u32[w][hyp * 3]);
            m.last[hyp] = std::max(m.last[hyp], sh.red_u32[w][hyp * 3 + 1]);
            m.count[hyp] += sh.red_u32[w][hyp * 3 + 2];
        }
        m.last[hyp] = m.last[hyp] ? m.last[hyp] - 1 : kDecNoFault;
        m.end_state[hyp] = sh.end_state[hyp];
    }
}

// Every entry whose `to` byte lies in slot `slot`, in order: visit(position in the tile, status, delta, the `to` byte).  The tile's first entry
// (position `first`) has its varint's start in the scan's hands: it is visited with is_first set and no delta.
// The varint of any other entry begins behind the previous `to` byte, which a valid entry has within 11 bytes: in this slot or the one below.
template <class Visit>
__device__ __forceinline__ void slot_entries(const DecShared &sh, uint32_t hyp, uint32_t slot, uint32_t to, uint32_t first, Visit &&visit) {
    if (!to) return;
    const uint32_t both = (slot ? (uint32_t)sh.to[hyp][slot - 1] : 0u) | (to << 16);  // bit i: the `to` flag of tile byte 16 (slot - 1) + i
    const uint32_t base = slot * 16 - 16;                                            // (never read below bit 16 when slot is 0)
    for (uint32_t m = to; m; m &= m - 1) {
        const uint32_t j = 16 + (uint32_t)__ffs((int)m) - 1, pos = base + j;
        const uint8_t byte = sh.bytes[pos];
        if (pos == first) {
            visit(pos, (uint32_t)diffstream::kOk, 0ull, byte, true);
            continue;
        }
        const uint32_t lower = both & ((1u << j) - 1);
        const uint32_t start = lower ? 32 - (uint32_t)__clz((int)lower) : 0, n = j - start;  // the varint: bits [start, j)
        unsigned long long delta = 0;
        uint32_t status = diffstream::kVarint;
        if (lower && n <= 10) {
            status = read_varint(n, [&](uint32_t i) { return (uint32_t)sh.bytes[base + start + i]; }, delta);
            if (!status && !delta) status = diffstream::kZeroDelta;  // (never the stream's first entry: that one is a tile's first)
        }
        visit(pos, status, delta, byte, false);
    }
}

__global__ __launch_bounds__(kDecThreads) void dec_summary_kernel(DecArgs d) {
    __shared__ DecShared sh;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    TileMasks m;
    tile_masks(d, blockIdx.x, sh, m);
    // per slot and start state: the deltas summed up to the slot's first fault, and that fault as (position << 3 | status)
    unsigned long long sum[kDecSteps][2];
    uint32_t fault[2] = {kDecNoFault, kDecNoFault};
#pragma unroll
    for (uint32_t s = 0; s < kDecSteps; s++)
#pragma unroll
        for (uint32_t hyp = 0; hyp < 2; hyp++) {
            unsigned long long acc = 0;
            uint32_t f = kDecNoFault;
            slot_entries(sh, hyp, s * kDecThreads + tid, m.to[s][hyp], m.first[hyp], [&](uint32_t pos, uint32_t status, unsigned long long delta, uint8_t, bool is_first) {
                if (is_first || f != kDecNoFault) return;
                if (status)
                    f = pos << 3 | status;
                else
                    acc = sat_add(acc, delta);
            });
            sum[s][hyp] = acc;
            fault[hyp] = std::min(fault[hyp], f);
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        for (uint32_t hyp = 0; hyp < 2; hyp++) fault[hyp] = std::min(fault[hyp], (uint32_t)__shfl_xor(fault[hyp], o, 64));
    __syncthreads();  // (red_u32 was read by every lane in tile_masks)
    if (lane == 0) {
        sh.red_u32[wave][0] = fault[0];
        sh.red_u32[wave][1] = fault[1];
    }
    __syncthreads();
    unsigned long long total[2];
    for (uint32_t hyp = 0; hyp < 2; hyp++) {
        uint32_t f = kDecNoFault;
        for (uint32_t w = 0; w < kDecWaves; w++) f = std::min(f, sh.red_u32[w][hyp]);
        fault[hyp] = f;
        // slots that begin at or before the tile's first fault count: those before it have none of their own, the one that holds it stopped there
        const uint32_t until = f == kDecNoFault ? kDecNoFault : f >> 3;
        unsigned long long acc = 0;
#pragma unroll
        for (uint32_t s = 0; s < kDecSteps; s++)
            if ((s * kDecThreads + tid) * 16 <= until) acc = sat_add(acc, sum[s][hyp]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc = sat_add(acc, (unsigned long long)__shfl_xor((long long)acc, o, 64));
        total[hyp] = acc;
    }
    if (lane == 0) {
        sh.red_u64[wave][0] = total[0];
        sh.red_u64[wave][1] = total[1];
    }
    __syncthreads();
    if (tid < 2) {
        const uint32_t hyp = tid;
        unsigned long long acc = 0;
        for (uint32_t w = 0; w < kDecWaves; w++) acc = sat_add(acc, sh.red_u64[w][hyp]);
        DecHyp out;
        out.n_to = m.count[hyp];
        out.first_to = m.first[hyp];
        out.pend = m.count[hyp] ? m.len - 1 - m.last[hyp] : m.len;
        out.flags = (m.end_state[hyp] & 1u) | (fault[hyp] == kDecNoFault ? 0u : (fault[hyp] & 7u) << 8);
        out.rest_sum = acc;
        d.tiles[blockIdx.x].h[hyp] = out;
    }
}

__device__ __forceinline__ uint32_t pend_after(const DecHyp &h, uint32_t pend) {
    return h.n_to ? std::min(h.pend, kDecPendCap) : std::min(kDecPendCap, pend + std::min(h.pend, kDecPendCap));
}

__global__ __launch_bounds__(kDecScanThreads) void dec_scan_kernel(DecArgs d) {
    // a run's fold per start state: bit 0 the end state, bit 1 "some tile of the run has a `to` byte" (pending is then a value, else an addend)
    __shared__ uint32_t s_map[2][kDecScanThreads], s_pend[2][kDecScanThreads];
    __shared__ uint32_t s_state[kDecScanThreads], s_in_pend[kDecScanThreads], s_fault[kDecScanThreads];
    __shared__ unsigned long long s_sum[kDecScanThreads], s_cnt[kDecScanThreads];
    __shared__ uint32_t s_final[2];
    const uint32_t tid = threadIdx.x;
    const unsigned long long run = (d.n_tiles + kDecScanThreads - 1) / kDecScanThreads;
    const unsigned long long lo = tid * run < d.n_tiles ? tid * run : d.n_tiles, hi = lo + run < d.n_tiles ? lo + run : d.n_tiles;
    {
        uint32_t state[2] = {0, 1}, pend[2] = {0, 0}, has[2] = {0, 0};
        for (unsigned long long t = lo; t < hi; t++)
            for (uint32_t hyp = 0; hyp < 2; hyp++) {
                const DecHyp h = d.tiles[t].h[state[hyp]];
                pend[hyp] = pend_after(h, pend[hyp]);
                has[hyp] |= h.n_to != 0;
                state[hyp] = h.flags & 1u;
            }
        for (uint32_t hyp = 0; hyp < 2; hyp++) {
            s_map[hyp][tid] = state[hyp] | has[hyp] << 1;
            s_pend[hyp][tid] = pend[hyp];
        }
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t state = 0, pend = 0;  // the stream's start: a varint byte is expected, nothing is pending
        for (uint32_t i = 0; i < kDecScanThreads; i++) {
            s_state[i] = state;
            s_in_pend[i] = pend;
            const uint32_t map = s_map[state][i], p = s_pend[state][i];
            pend = (map & 2u) ? p : std::min(kDecPendCap, pend + p);
            state = map & 1u;
        }
        s_final[0] = state;
        s_final[1] = pend;
    }
    __syncthreads();
    {
        uint32_t state = s_state[tid], pend = s_in_pend[tid];
        unsigned long long sum = 0, cnt = 0;
        for (unsigned long long t = lo; t < hi; t++) {
            const DecHyp h = d.tiles[t].h[state];
            DecStart st{};
            st.state = state;
            st.pend = pend;
            if (h.n_to) {
                // the tile's first entry: its varint is the pending bytes and the tile's bytes in front of its `to` byte
                const unsigned long long tile_at = t * kDecTileBytes;
                const uint32_t n = pend + h.first_to;
                st.fault = diffstream::kVarint;
                if (n <= 10 && pend <= tile_at) {
                    const uint8_t *p = d.stream + (tile_at - pend);
                    st.fault = read_varint(n, [&](uint32_t i) { return (uint32_t)p[i]; }, st.first_delta);
                }
                if (!st.fault) sum = sat_add(sum, sat_add(st.first_delta, h.rest_sum));
                cnt += h.n_to;
            }
            d.starts[t] = st;
            pend = pend_after(h, pend);
            state = h.flags & 1u;
        }
        s_sum[tid] = sum;
        s_cnt[tid] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long sum = 0, cnt = 0;
        for (uint32_t i = 0; i < kDecScanThreads; i++) {
            const unsigned long long s = s_sum[i], c = s_cnt[i];
            s_sum[i] = sum;
            s_cnt[i] = cnt;
            sum = sat_add(sum, s);
            cnt += c;
        }
        d.result->entries = cnt;
    }
    __syncthreads();
    {
        unsigned long long index = s_sum[tid], ordinal = s_cnt[tid];
        uint32_t fault = diffstream::kOk;
        for (unsigned long long t = lo; t < hi; t++) {
            DecStart st = d.starts[t];
            const DecHyp h = d.tiles[t].h[st.state];
            st.base_index = index;
            st.ordinal = ordinal;
            d.starts[t] = st;
            if (!h.n_to) continue;
            const unsigned long long at_first = sat_add(index, st.first_delta), at_last = sat_add(at_first, h.rest_sum);
            if (!fault) {  // the precedence within an entry is the host's: the varint, a zero delta, the index
                if (st.fault)
                    fault = st.fault;
                else if (ordinal && !st.first_delta)
                    fault = diffstream::kZeroDelta;
                else if (at_first >= d.end || at_last >= d.end)  // (at_last: the last entry before the tile's first other fault)
                    fault = diffstream::kBeyond;
                else
                    fault = (h.flags >> 8) & 7u;
            }
            index = at_last;
            ordinal += h.n_to;
        }
        s_fault[tid] = fault;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t fault = diffstream::kOk;
        for (uint32_t i = 0; i < kDecScanThreads && !fault; i++) fault = s_fault[i];
        const uint32_t pend = s_final[1];
        if (!fault && pend)  // a partial entry behind the last `to` byte: its 10th byte may still overflow, an 11th is one too many
            fault = pend >= 11 || (pend == 10 && (d.stream[d.len - 1] & 0x7fu) > 1) ? diffstream::kVarint : diffstream::kTruncated;
        d.result->status = fault;
        d.result->final_state = s_final[0];
    }
}

// where an entry's byte goes
__device__ __forceinline__ void store_entry(const DecArgs &d, unsigned long long ordinal, unsigned long long index, uint8_t to) {
    if (index >= d.end) return;  // (the scan found none such; out of bounds is never written)
    if (d.target == kDecToArrays) {
        if (ordinal < d.cap) {
            d.out_index[ordinal] = index;
            d.out_to[ordinal] = to;
        }
        return;
    }
    if (index < d.skip_below) return;  // the file's header: the host's
    const unsigned long long j = index - d.skip_below;
    if (d.target == kDecToImage) {
        d.weights[j] = to;
    } else if (j < d.lr_bytes) {
        d.weights[(j >> 2) * 8 + (j & 3)] = to;  // the weight half of the {w, acc} pair
    } else if (j < d.lr_bytes + 8) {
        d.q_header[j - d.lr_bytes] = to;
    } else {
        d.buckets[j - d.lr_bytes - 8] = to;
    }
}

__global__ __launch_bounds__(kDecThreads) void dec_apply_kernel(DecArgs d) {
    __shared__ DecShared sh;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    TileMasks m;
    tile_masks(d, blockIdx.x, sh, m);
    const DecStart st = d.starts[blockIdx.x];
    const uint32_t hyp = st.state & 1u;
    if (!m.count[hyp]) return;  // (uniform)
    // per slot: its entries' count and summed deltas, then both as exclusive prefixes over the tile's slots
    unsigned long long sum[kDecSteps];
    uint32_t cnt[kDecSteps];
#pragma unroll
    for (uint32_t s = 0; s < kDecSteps; s++) {
        unsigned long long acc = 0;
        slot_entries(sh, hyp, s * kDecThreads + tid, m.to[s][hyp], m.first[hyp],
                     [&](uint32_t, uint32_t, unsigned long long delta, uint8_t, bool is_first) { acc += is_first ? st.first_delta : delta; });
        const uint32_t c = __popc(m.to[s][hyp]);
        unsigned long long incl = acc;
        uint32_t incl_c = c;
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const unsigned long long t = (unsigned long long)__shfl_up((long long)incl, o, 64);
            const uint32_t tc = __shfl_up(incl_c, o, 64);
            if (lane >= o) {
                incl += t;
                incl_c += tc;
            }
        }
        sum[s] = incl - acc;
        cnt[s] = incl_c - c;
        if (lane == 63) {
            sh.chunk_sum[s * kDecWaves + wave] = incl;
            sh.chunk_cnt[s * kDecWaves + wave] = incl_c;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t s = 0; s < kDecSteps; s++) {
        if (!m.to[s][hyp]) continue;
        unsigned long long index = st.base_index + sum[s], ordinal = st.ordinal + cnt[s];
        for (uint32_t c = 0; c < s * kDecWaves + wave; c++) {
            index += sh.chunk_sum[c];
            ordinal += sh.chunk_cnt[c];
        }
        slot_entries(sh, hyp, s * kDecThreads + tid, m.to[s][hyp], m.first[hyp], [&](uint32_t, uint32_t, unsigned long long delta, uint8_t to, bool is_first) {
            index += is_first ? st.first_delta : delta;
            store_entry(d, ordinal++, index, to);
        });
    }
}

static bool dec_args_ok(const DecArgs &d) {
    return d.len && d.n_tiles == (d.len + kDecTileBytes - 1) / kDecTileBytes && d.n_tiles <= 0x7fffffffull && d.stream && d.tiles && d.starts &&
           d.result && (reinterpret_cast<uintptr_t>(d.stream) & 15) == 0;
}

hipError_t launch_dec_summary(const DecArgs &d, hipStream_t stream) {
    if (!dec_args_ok(d)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_summary_kernel, dim3((uint32_t)d.n_tiles), dim3(kDecThreads), 0, stream, d);
    return hipGetLastError();
}

hipError_t launch_dec_scan(const DecArgs &d, hipStream_t stream) {
    if (!dec_args_ok(d)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_scan_kernel, dim3(1), dim3(kDecScanThreads), 0, stream, d);
    return hipGetLastError();
}

hipError_t launch_dec_apply(const DecArgs &d, hipStream_t stream) {
    if (!dec_args_ok(d)) return hipErrorInvalidValue;
    if (d.target == kDecToArrays ? (d.cap && (!d.out_index || !d.out_to)) : !d.weights) return hipErrorInvalidValue;
    if (d.target == kDecToPacked && (!d.buckets || !d.q_header)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_apply_kernel, dim3((uint32_t)d.n_tiles), dim3(kDecThreads), 0, stream, d);
    return hipGetLastError();
}

namespace {

constexpr size_t kUploadChunk = 8u << 20;  // two pinned buffers of this size carry a large stream: the host's copy of one runs beside the other's transfer

// the device side of one decode: the stream, the tile records, the result, the 8 bytes of a packed regressor's {increment, min}
struct DecodeRun {
    DecArgs d{};
    uint8_t *d_stream = nullptr, *ws = nullptr;
    PatchStaging own, *staging = &own;  // (the owner's, where the patched object keeps one)
    ~DecodeRun() {
        (void)hipFree(d_stream);
        (void)hipFree(ws);
    }
    int alloc(const char *who, uint64_t len, uint64_t end) {
        d.len = len;
        d.end = end;
        d.n_tiles = (len + kDecTileBytes - 1) / kDecTileBytes;
        if (d.n_tiles > 0x7fffffffull) return fail(FWGPU_ERR_RANGE, std::string(who) + ": more tiles than one launch's workgroups");
        const size_t ws_bytes = 64 + d.n_tiles * (sizeof(DecTile) + sizeof(DecStart));
        if (hipMalloc((void **)&d_stream, (len + 15) / 16 * 16) != hipSuccess || hipMalloc((void **)&ws, ws_bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(FWGPU_ERR_OOM, std::string(who) + ": no device memory for the stream");
        }
        d.stream = d_stream;
        d.result = reinterpret_cast<DecResult *>(ws);
        d.q_header = ws + 32;
        d.starts = reinterpret_cast<DecStart *>(ws + 64);
        d.tiles = reinterpret_cast<DecTile *>(d.starts + d.n_tiles);
        return FWGPU_OK;
    }
    int upload(const uint8_t *diff) {
        const uint64_t len = d.len;
        uint8_t *&pinned = staging->pinned;
        hipEvent_t *ev = staging->ev;
        if (len <= kUploadChunk) {
            FWGPU_HIP(hipMemcpy(d_stream, diff, len, hipMemcpyHostToDevice));
        } else {
            if (!pinned) FWGPU_HIP(hipHostMalloc((void **)&pinned, 2 * kUploadChunk, hipHostMallocDefault));
            for (int i = 0; i < 2; i++)
                if (!ev[i]) FWGPU_HIP(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
            uint32_t k = 0;
            for (uint64_t at = 0; at < len; at += kUploadChunk, k ^= 1) {
                const size_t n = (size_t)std::min<uint64_t>(kUploadChunk, len - at);
                if (at >= 2 * kUploadChunk) FWGPU_HIP(hipEventSynchronize(ev[k]));  // (the buffer's last transfer)
                memcpy(pinned + k * kUploadChunk, diff + at, n);
                FWGPU_HIP(hipMemcpyAsync(d_stream + at, pinned + k * kUploadChunk, n, hipMemcpyHostToDevice, 0));
                FWGPU_HIP(hipEventRecord(ev[k], 0));
            }
        }
        return FWGPU_OK;
    }
    // uploads the stream and runs the summary pass and the scan; *status: the stream's
    int decode(const char *who, const uint8_t *diff, uint64_t len, uint64_t end, uint64_t *entries, int *status) {
        int rc = alloc(who, len, end);
        if (!rc) rc = upload(diff);
        if (rc) return rc;
        FWGPU_HIP(launch_dec_summary(d, 0));
        FWGPU_HIP(launch_dec_scan(d, 0));
        DecResult res{};
        FWGPU_HIP(hipMemcpy(&res, d.result, sizeof res, hipMemcpyDeviceToHost));
        *status = (int)res.status;
        *entries = res.entries;
        return FWGPU_OK;
    }
};

}  // namespace
}  // namespace fwgpu

using namespace fwgpu;

extern "C" {

int fwgpu_image_apply_diff(fwgpu_image *img, const uint8_t *diff, uint64_t len, uint64_t *applied) {
    if (!img || (len && !diff)) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (applied) *applied = 0;
    if (!len) return FWGPU_OK;
    const uint64_t hb = img->header.size();
    if (hb > UINT64_MAX - img->weights_bytes) return fail(FWGPU_ERR_INVALID, "image_apply_diff: the image's length does not fit 64 bits");
    FWGPU_HIP(hipSetDevice(img->device));
    DecodeRun run;
    run.staging = &img->patch_staging;
    uint64_t entries = 0;
    int st = 0;
    const int rc = run.decode("image_apply_diff", diff, len, hb + img->weights_bytes, &entries, &st);
    if (rc) return rc;
    if (st) return fail(FWGPU_ERR_FORMAT, std::string("image_apply_diff: ") + diffstream::status_text(st));
    run.d.target = kDecToImage;
    run.d.skip_below = hb;
    run.d.weights = img->d_weights;
    if (img->weights_bytes) {
        FWGPU_HIP(launch_dec_apply(run.d, 0));
        FWGPU_HIP(hipDeviceSynchronize());
    }
    // the header's entries, once the device has done its part: the stream is valid and indices ascend, so a walk of its prefix that stops at the first entry behind the header finds them
    uint64_t at = 0, index = 0;
    while (at < len) {
        uint64_t delta = 0;
        for (uint32_t k = 0;; k++) {
            const uint8_t byte = diff[at++];
            delta |= (uint64_t)(byte & 0x7f) << (7 * k);
            if (!(byte & 0x80)) break;
        }
        index += delta;
        if (index >= hb) break;
        img->header[index] = diff[at++];
    }
    if (applied) *applied = entries;
    return FWGPU_OK;
}

int fwgpu_packed_apply_diff(fwgpu_regressor *r, const uint8_t *diff, uint64_t len, uint64_t *applied) {
    if (!r || (len && !diff)) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (applied) *applied = 0;
    if (!r->packed()) return fail(FWGPU_ERR_INVALID, "packed_apply_diff: the regressor's FFM weights are f32, not the file's f16 buckets: a byte diff of two inference files does not apply to it");
    if (r->nn.n_layers)
        return fail(FWGPU_ERR_INVALID, "packed_apply_diff: the regressor has a deep head, whose layers lie behind the buckets in the file: a diff is not applied to it, load the file");
    if (r->file_quantized_at_load)
        return fail(FWGPU_ERR_INVALID, "packed_apply_diff: the regressor's file was quantised at load: its buckets are not the file's bytes");
    if (!r->file_header_bytes)
        return fail(FWGPU_ERR_INVALID, "packed_apply_diff: the regressor has no inference file behind it (made by fwgpu_pack_regressor: refresh it with that call; or loaded from a file that carries optimizer state)");
    if (!len) return FWGPU_OK;
    // the file: header | LR weights (f32) | {increment, min} | buckets
    const uint64_t hb = r->file_header_bytes, lr_bytes = r->lr_len * 4, q_bytes = r->ffm_len * 2;
    FWGPU_HIP(hipSetDevice(r->device));
    FWGPU_HIP(hipDeviceSynchronize());
    DecodeRun run;
    run.staging = &r->patch_staging;
    uint64_t entries = 0;
    int st = 0;
    const int rc = run.decode("packed_apply_diff", diff, len, hb + lr_bytes + 8 + q_bytes, &entries, &st);
    if (rc) return rc;
    if (st) return fail(FWGPU_ERR_FORMAT, std::string("packed_apply_diff: ") + diffstream::status_text(st));
    // indices ascend: an entry in the header, if there is one, is the first, and its delta is its index
    uint64_t first = 0;
    for (uint32_t k = 0;; k++) {
        first |= (uint64_t)(diff[k] & 0x7f) << (7 * k);
        if (!(diff[k] & 0x80)) break;
    }
    if (first < hb) return fail(FWGPU_ERR_INVALID, "packed_apply_diff: the model's header changed: load the file");
    uint8_t q_header[8];
    memcpy(q_header, &r->q_increment, 4);
    memcpy(q_header + 4, &r->q_min, 4);
    FWGPU_HIP(hipMemcpy(run.d.q_header, q_header, 8, hipMemcpyHostToDevice));
    run.d.target = kDecToPacked;
    run.d.skip_below = hb;
    run.d.lr_bytes = lr_bytes;
    run.d.weights = reinterpret_cast<uint8_t *>(r->d_lr);
    run.d.buckets = reinterpret_cast<uint8_t *>(r->d_ffm_q);
    FWGPU_HIP(launch_dec_apply(run.d, 0));
    FWGPU_HIP(hipMemcpy(q_header, run.d.q_header, 8, hipMemcpyDeviceToHost));
    memcpy(&r->q_increment, q_header, 4);
    memcpy(&r->q_min, q_header + 4, 4);
    r->weights_epoch++;  // (context caches set up before, fwgpu_packed_enable_caches, are stale from here on)
    if (applied) *applied = entries;
    return FWGPU_OK;
}

int fwgpu_debug_diff_decode(int device, const uint8_t *diff, uint64_t len, uint64_t end, uint64_t *index, uint8_t *to, uint64_t cap, uint64_t *entries,
                            int32_t *status) {
    if ((len && !diff) || (cap && (!index || !to)) || !entries || !status) return fail(FWGPU_ERR_INVALID, "NULL argument");
    *entries = 0;
    *status = diffstream::kOk;
    if (!len) return FWGPU_OK;
    FWGPU_HIP(hipSetDevice(device));
    DecodeRun run;
    int st = 0;
    const int rc = run.decode("debug_diff_decode", diff, len, end, entries, &st);
    if (rc) return rc;
    *status = st;
    if (st) return fail(FWGPU_ERR_FORMAT, std::string("debug_diff_decode: ") + diffstream::status_text(st));
    const uint64_t n = std::min(*entries, cap);
    if (!n) return FWGPU_OK;
    uint8_t *d_out = nullptr;  // the indices, then the bytes
    if (hipMalloc((void **)&d_out, n * 9) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FWGPU_ERR_OOM, "debug_diff_decode: no device memory for the entries");
    }
    run.d.target = kDecToArrays;
    run.d.out_index = reinterpret_cast<unsigned long long *>(d_out);
    run.d.out_to = d_out + n * 8;
    run.d.cap = n;
    hipError_t e = launch_dec_apply(run.d, 0);
    if (e == hipSuccess) e = hipMemcpy(index, d_out, n * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(to, d_out + n * 8, n, hipMemcpyDeviceToHost);
    (void)hipFree(d_out);
    if (e != hipSuccess) return fail(FWGPU_ERR_DEVICE, std::string("debug_diff_decode: ") + hipGetErrorString(e));
    return FWGPU_OK;
}

int fwgpu_debug_decode_rates(int device, const uint8_t *diff, uint64_t len, uint64_t end, float *ms4) {
    if (!diff || !len || !ms4) return fail(FWGPU_ERR_INVALID, "NULL argument");
    FWGPU_HIP(hipSetDevice(device));
    DecodeRun run;
    int rc = run.alloc("debug_decode_rates", len, end);
    if (!rc) rc = run.upload(diff);
    if (rc) return rc;
    FWGPU_HIP(hipDeviceSynchronize());
    void *copy = nullptr;
    uint8_t *d_out = nullptr;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    DecResult res{};
    hipError_t e = hipMalloc(&copy, len);
    for (int i = 0; i < 6 && e == hipSuccess; i++) e = hipEventCreate(&ev[i]);
    if (e == hipSuccess) e = hipEventRecord(ev[0], 0);
    if (e == hipSuccess) e = launch_dec_summary(run.d, 0);
    if (e == hipSuccess) e = hipEventRecord(ev[1], 0);
    if (e == hipSuccess) e = launch_dec_scan(run.d, 0);
    if (e == hipSuccess) e = hipEventRecord(ev[2], 0);
    if (e == hipSuccess) e = hipMemcpy(&res, run.d.result, sizeof res, hipMemcpyDeviceToHost);
    const bool ok = e == hipSuccess && !res.status && res.entries;
    if (ok) e = hipMalloc((void **)&d_out, res.entries * 9);  // the apply pass stores every entry: the indices, then the bytes
    run.d.target = kDecToArrays;
    run.d.out_index = reinterpret_cast<unsigned long long *>(d_out);
    run.d.out_to = d_out + res.entries * 8;
    run.d.cap = res.entries;
    if (e == hipSuccess) e = hipEventRecord(ev[3], 0);  // (the device was idle while the host read the result)
    if (ok && e == hipSuccess) e = launch_dec_apply(run.d, 0);
    if (e == hipSuccess) e = hipEventRecord(ev[4], 0);
    if (e == hipSuccess) e = hipMemcpyAsync(copy, run.d_stream, len, hipMemcpyDeviceToDevice, 0);
    if (e == hipSuccess) e = hipEventRecord(ev[5], 0);
    if (e == hipSuccess) e = hipEventSynchronize(ev[5]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms4[0], ev[0], ev[1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms4[1], ev[1], ev[2]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms4[2], ev[3], ev[4]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms4[3], ev[4], ev[5]);
    for (int i = 0; i < 6; i++)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    (void)hipFree(copy);
    (void)hipFree(d_out);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(FWGPU_ERR_DEVICE, std::string("debug_decode_rates: ") + hipGetErrorString(e));
    }
    if (res.status) return fail(FWGPU_ERR_FORMAT, std::string("debug_decode_rates: ") + diffstream::status_text((int)res.status));
    return FWGPU_OK;
}

int fwgpu_debug_decode_geometry(uint32_t *tile_bytes) {
    if (!tile_bytes) return fail(FWGPU_ERR_INVALID, "NULL argument");
    *tile_bytes = kDecTileBytes;
    return FWGPU_OK;
}

}  // extern "C"
