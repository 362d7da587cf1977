// From the plain records of many requests' candidate lines to the entry batch of the requests kernels (requests.hip, requests_head.hip), on the device:
// fwgpu_predictor_predict_requests_text (serving.cpp).  The host route parses every line behind its predictor's context, translates the merged record
// (translate.cpp translate_record) and drops the FFM entries the predictor's cache holds (fwgpu_block_cache_filter); here the device parser has left
// every line's STAND-ALONE record, and three kernels do the rest:
//   count  one wavefront per line: which request and cache the line belongs to (binary search of its first byte in the requests' offsets), the cache's
//          record rule (context_cache.cpp block_cache_record_ok, delta form) against THAT cache, and the entries of the merged record -- a namespace
//          slot reads the candidate's word where the candidate fills it and the context's otherwise (kernels.hip slot_count / slot_get);
//   scan   one workgroup: exclusive sums of the counts (a line's rank is its example), totals, maxima, the "other route" flag and every request's
//          first line -- the one block the host reads;
//   emit   one wavefront per line: the entries in the host translator's order (the f32 sums of the requests kernels depend on it), written straight
//          into the batch's SoA arrays.  FFM: field by field, the features of the pairs the context does not cover.  LR: combo by combo, first
//          namespace most significant, hash = (hash * 16777619) ^ h, values multiplied, then the combo's weight; the constant entry last.
// Data movement: the translator's tables are packed into LDS once per workgroup (kernels.hip TrLds), every wave stages its candidate's record in LDS,
// the context's record is staged once per workgroup when all its lines share a request (lines of a request are contiguous) and read through the L2
// otherwise.  A wave finds its pairs' and combos' first entries by a wave-wide prefix scan; each lane then finds its entry's pair or combo by binary
// search and decodes that one entry (stage_example's two steps, at wave scope).  Integer and LDS work: no matrix instructions.
#include "requests_text.h"

namespace fwgpu {
namespace {

constexpr uint32_t kNotSingle = 0x80000000u, kNoFeatures = 0x80000000u, kHeaderLen = 3;  // parser.rs:13-19
constexpr uint32_t kConstantHash = 11650396u;  // feature_buffer.rs:8
constexpr uint32_t kCountCap = 1u << 20;       // entry counts saturate here (the route refuses beyond 4096)

// feature_reader! (feature_buffer.rs:47-108) on a slot word
__device__ __forceinline__ uint32_t word_count(uint32_t w) {
    if (!(w & kNotSingle)) return 1;                        // single feature, value 1.0
    return ((w & 0xffffu) - ((w >> 16) & 0x3fffu)) >> 1;   // NO_FEATURES -> 0
}
__device__ __forceinline__ void word_get(const uint32_t *rec, uint32_t w, bool is_f32, uint32_t q, uint32_t &hash, float &val) {
    if (!(w & kNotSingle)) {
        hash = w;
        val = 1.0f;
    } else {
        const uint32_t st = (w >> 16) & 0x3fffu;
        hash = rec[st + 2 * q];
        val = is_f32 ? 1.0f : __uint_as_float(rec[st + 2 * q + 1]);
    }
}
// the merged record: the candidate's word where the candidate fills the slot, the context's otherwise
struct Merged {
    const uint32_t *cand, *ctx;
    __device__ __forceinline__ uint32_t word(uint32_t ns, const uint32_t *&src) const {
        uint32_t w = cand[kHeaderLen + ns];
        src = cand;
        if (w == kNoFeatures) {
            w = ctx[kHeaderLen + ns];
            src = ctx;
        }
        return w;
    }
    __device__ __forceinline__ uint32_t count(uint32_t ns) const {
        const uint32_t *src;
        return word_count(word(ns, src));
    }
};

__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct TrLds {  // kernels.hip TrLds: the translator's tables, packed
    const uint32_t *pair;  // [n_pairs]      namespace | field << 16 | f32 << 31
    const uint32_t *coff;  // [n_combos + 1]
    const uint32_t *cm;    // [n_members]    namespace | f32 << 31
    const float *cw;       // [n_combos]
    __device__ __forceinline__ uint32_t pair_ns(uint32_t j) const { return pair[j] & 0xffffu; }
    __device__ __forceinline__ bool pair_f32(uint32_t j) const { return (pair[j] >> 31) != 0; }
    __device__ __forceinline__ uint32_t pair_field(uint32_t j) const { return (pair[j] >> 16) & 0xffu; }
    __device__ __forceinline__ uint32_t combo_ns(uint32_t m) const { return cm[m] & 0x7fffffffu; }
    __device__ __forceinline__ bool combo_f32(uint32_t m) const { return (cm[m] >> 31) != 0; }
};
__host__ __device__ inline uint32_t tr_words(const DevTranslator &t) { return t.n_pairs + (t.n_combos + 1) + t.n_members + t.n_combos; }
__host__ __device__ inline uint32_t base_words(const DevTranslator &t) { return (t.n_pairs + 1) + (t.n_combos + 1); }

// the request of a line: the last one whose text begins at or before the line's first byte (a request without text begins where the next one does)
__device__ __forceinline__ uint32_t request_of(const RtArgs &a, uint32_t line) {
    const uint32_t pos = a.lstart[line];
    uint32_t lo = 0, hi = a.n_requests;  // t_off[lo] <= pos < t_off[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.t_off[mid] <= pos) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool covered(const RtCache &c, uint32_t ns) { return ((c.cover[ns >> 5] >> (ns & 31u)) & 1u) != 0; }

// is (masked hash, field * k) a cached feature: the filter bit first, then the sorted keys
__device__ __forceinline__ bool present_hit(const RtCache &c, uint32_t masked_hash, uint32_t fk) {
    const unsigned long long key = ((unsigned long long)masked_hash << 32) | fk;
    const uint32_t b = (uint32_t)((key * 0x9e3779b97f4a7c15ULL) >> 52);
    if (!((c.present_bits[b >> 6] >> (b & 63u)) & 1ull)) return false;
    uint32_t lo = 0, hi = c.n_present;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const unsigned long long v = c.present[mid];
        if (v == key) return true;
        if (v < key) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

// EMIT == false: the count pass.  EMIT == true: the emit pass, launched only when the scan found no line for the other route.
template <bool EMIT>
__global__ __launch_bounds__(64 * kRtLines) void requests_text_kernel(RtArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const DevTranslator &t = a.tr;
    const uint32_t NP = t.n_pairs, NC = t.n_combos, NM = t.n_members;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // ---- LDS: tables | per wave {first entry of every pair, of every combo} | the context's record | per wave the candidate's record
    uint32_t *s_pair = lds, *s_coff = s_pair + NP, *s_cm = s_coff + NC + 1, *s_cw = s_cm + NM;
    uint32_t *s_base = s_cw + NC + wave * base_words(t);
    uint32_t *s_ctx = s_cw + NC + kRtLines * base_words(t);
    uint32_t *s_rec = s_ctx + kRtCtxWords + wave * kRtRecWords;
    for (uint32_t j = tid; j < NP; j += blockDim.x) s_pair[j] = t.pair_ns[j] | ((uint32_t)t.pair_field[j] << 16) | (t.pair_f32[j] ? kNotSingle : 0u);
    for (uint32_t c = tid; c <= NC; c += blockDim.x) s_coff[c] = t.combo_off[c];
    for (uint32_t m = tid; m < NM; m += blockDim.x) s_cm[m] = t.combo_ns[m] | (t.combo_f32[m] ? kNotSingle : 0u);
    for (uint32_t c = tid; c < NC; c += blockDim.x) s_cw[c] = __float_as_uint(t.combo_w[c]);
    const TrLds tr{s_pair, s_coff, s_cm, reinterpret_cast<const float *>(s_cw)};
    // ---- the workgroup's lines: one request (its context's record goes to LDS once) or several (read through the L2)
    const uint32_t line0 = blockIdx.x * kRtLines, line_last = min(line0 + kRtLines, a.nlines) - 1;
    const uint32_t r_first = request_of(a, line0), r_last = request_of(a, line_last);
    const RtCache &c_first = a.caches[a.cache_of_request[r_first]];
    const bool shared_ctx = r_first == r_last && c_first.ctx_len <= kRtCtxWords;
    if (shared_ctx)
        for (uint32_t i = tid; i < c_first.ctx_len; i += blockDim.x) s_ctx[i] = c_first.ctx_rec[i];
    __syncthreads();
    const uint32_t line = line0 + wave;
    if (line >= a.nlines) return;  // (no workgroup barrier below)
    const uint32_t req = shared_ctx ? r_first : request_of(a, line);
    const uint32_t cache_index = a.cache_of_request[req];
    const RtCache &cache = a.caches[cache_index];
    if (!EMIT && lane == 0) a.cache_of[line] = cache_index;  // (fwgpu_batch_set_caches' index array: example = line)
    const uint64_t r0 = a.rec_off[line];
    const uint32_t len = (uint32_t)(a.rec_off[line + 1] - r0);
    const uint32_t nns = a.nns;
    bool ok = (a.status[line].x & 0xffu) == 1u /* kTextDeviceOk */ && a.text[a.lstart[line]] == '|' && len >= kHeaderLen + nns && len <= kRtMaxRecord;
    if (EMIT) ok = a.counts[line].x != 0;
    if (!ok) {
        if (!EMIT && lane == 0) a.counts[line] = make_uint4(0u, 0u, 0u, req);
        return;
    }
    const uint32_t *grec = a.records + r0;
    const bool rec_in_lds = len <= kRtRecWords;
    if (rec_in_lds) {
        for (uint32_t i = lane; i < len; i += 64) s_rec[i] = grec[i];
        wave_lds_sync();
    }
    const Merged rec{rec_in_lds ? s_rec : grec, shared_ctx ? s_ctx : cache.ctx_rec};
    // ---- first entry of every uncovered (field, namespace) pair and of every LR combo: wave-wide prefix scans
    uint32_t *ffm_base = s_base, *lr_base = s_base + NP + 1;
    uint32_t n_ffm = 0, n_combo = 0;
    for (uint32_t b0 = 0; b0 < NP; b0 += 64) {
        const uint32_t j = b0 + lane;
        uint32_t cnt = 0;
        if (j < NP && !covered(cache, tr.pair_ns(j))) cnt = word_count(rec.cand[kHeaderLen + tr.pair_ns(j)]);
        const uint32_t inc = wave_scan_incl(cnt, lane);
        if (EMIT && j < NP) ffm_base[j] = min(n_ffm + inc - cnt, kCountCap);  // (the count pass needs the totals only)
        n_ffm = min(n_ffm + (uint32_t)__shfl((int)inc, 63, 64), kCountCap);
    }
    for (uint32_t b0 = 0; b0 < NC; b0 += 64) {
        const uint32_t c = b0 + lane;
        unsigned long long total = (c < NC && a.has_lr) ? 1ull : 0ull;
        if (total)
            for (uint32_t m = tr.coff[c]; m < tr.coff[c + 1]; ++m) total = min(total * rec.count(tr.combo_ns(m)), (unsigned long long)kCountCap);
        const uint32_t cnt = (uint32_t)total, inc = wave_scan_incl(min(cnt, kCountCap >> 6), lane);  // (64 capped lanes stay below 2^32)
        if (EMIT && c < NC) lr_base[c] = min(n_combo + inc - min(cnt, kCountCap >> 6), kCountCap);
        n_combo = min(n_combo + (uint32_t)__shfl((int)inc, 63, 64), kCountCap);
    }
    if (EMIT && lane == 0) {
        ffm_base[NP] = n_ffm;
        lr_base[NC] = n_combo;
    }
    const uint32_t n_lr = n_combo + ((a.has_lr && t.add_const) ? 1u : 0u);
    if (!EMIT) {
        // ---- the cache's record rule (block_cache_record_ok, delta form): no slot the context fills is filled again, every range lies in the record,
        // and no FFM feature of an uncovered pair is a cached one
        bool bad = false;
        for (uint32_t ns = lane; ns < nns; ns += 64) {
            const uint32_t w = rec.cand[kHeaderLen + ns];
            if (w == kNoFeatures) continue;
            bad = bad || covered(cache, ns);
            if (w & kNotSingle) {
                const uint32_t st = (w >> 16) & 0x3fffu, en = w & 0xffffu;
                bad = bad || en > len || en < st || st < kHeaderLen + nns || ((en - st) & 1u);
            }
        }
        if (__ballot(bad) == 0ull) {  // (ranges are sound: the features may be read)
            for (uint32_t j = lane; j < NP; j += 64) {
                const uint32_t ns = tr.pair_ns(j), fk = tr.pair_field(j) * a.ffm_k;
                if (covered(cache, ns)) continue;
                const uint32_t w = rec.cand[kHeaderLen + ns], n = word_count(w);
                for (uint32_t q = 0; q < n && !bad; q++) {
                    uint32_t h;
                    float v;
                    word_get(rec.cand, w, false, q, h, v);
                    bad = present_hit(cache, h & t.ffm_mask, fk);
                }
            }
        }
        const bool line_ok = __ballot(bad) == 0ull;
        if (lane == 0) a.counts[line] = make_uint4(line_ok ? 1u : 0u, n_lr, n_ffm, req);
        return;
    }
    // ---- emit: this line is example `line` of the batch
    wave_lds_sync();
    const uint32_t fo = a.counts[line].y, lo = a.counts[line].z;  // (the scan left the line's first entries here)
    if (lane == 0) {
        a.lr_off[line] = lo;
        a.ffm_off[line] = fo;
        if (line + 1 == a.nlines) {
            a.lr_off[line + 1] = (uint32_t)a.totals->tot_lr;
            a.ffm_off[line + 1] = (uint32_t)a.totals->tot_ffm;
        }
        a.label[line] = 0.0f;
        a.importance[line] = 1.0f;
    }
    // ffm_buffer, ordered by field (feature_buffer.rs:314-335): entry e belongs to the last pair whose first entry is <= e
    for (uint32_t e = lane; e < n_ffm; e += 64) {
        uint32_t lo_ = 0, hi_ = NP;
        while (hi_ - lo_ > 1) {
            const uint32_t mid = (lo_ + hi_) >> 1;
            if (ffm_base[mid] <= e) lo_ = mid;
            else hi_ = mid;
        }
        const uint32_t j = lo_;
        uint32_t h;
        float v;
        word_get(rec.cand, rec.cand[kHeaderLen + tr.pair_ns(j)], tr.pair_f32(j), e - ffm_base[j], h, v);
        a.ffm_hash[fo + e] = h & t.ffm_mask;
        a.ffm_val[fo + e] = v;
        a.ffm_fld[fo + e] = (uint8_t)tr.pair_field(j);
    }
    // lr_buffer (feature_buffer.rs:194-276)
    for (uint32_t e = lane; e < n_combo; e += 64) {
        uint32_t lo_ = 0, hi_ = NC;
        while (hi_ - lo_ > 1) {
            const uint32_t mid = (lo_ + hi_) >> 1;
            if (lr_base[mid] <= e) lo_ = mid;
            else hi_ = mid;
        }
        const uint32_t c = lo_;
        // digits of the entry's index within the combo, first namespace most significant (the reference's loop nesting)
        uint32_t rem = e - lr_base[c], div = lr_base[c + 1] - lr_base[c];
        uint32_t hash = 0;
        float val = 1.0f;
        for (uint32_t m = tr.coff[c]; m < tr.coff[c + 1]; ++m) {
            const uint32_t *src;
            const uint32_t w = rec.word(tr.combo_ns(m), src);
            div /= word_count(w);
            const uint32_t q = rem / div;
            rem -= q * div;
            uint32_t h;
            float v;
            word_get(src, w, tr.combo_f32(m), q, h, v);
            if (m == tr.coff[c]) {
                hash = h;
                val = v;
            } else {
                hash = (hash * 16777619u) ^ h;  // feature_buffer.rs:242-251 (wrapping)
                val = val * v;
            }
        }
        a.lr_hash[lo + e] = hash & t.lr_mask;
        a.lr_val[lo + e] = val * tr.cw[c];
        a.lr_combo[lo + e] = (uint16_t)c;
    }
    if (lane == 0 && n_lr > n_combo) {  // feature_buffer.rs:270-276
        a.lr_hash[lo + n_combo] = kConstantHash & t.lr_mask;
        a.lr_val[lo + n_combo] = 1.0f;
        a.lr_combo[lo + n_combo] = (uint16_t)NC;
    }
}

// One workgroup over all lines, a contiguous run of lines per WAVE, walked 64 lines at a time (one coalesced 1 KiB load per step): counts[i] =
// {ok, LR, FFM, request} -> {ok, first FFM entry, first LR entry, request}; the totals, the maxima, the flag; and every request's first line (the first
// line that begins at or behind the request's text).
__device__ __forceinline__ unsigned long long wave_total(unsigned long long v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__global__ __launch_bounds__(kRtScanThreads) void requests_text_scan(RtArgs a) {
    constexpr uint32_t kWaves = kRtScanThreads / 64;
    __shared__ unsigned long long s_lr[kWaves], s_ffm[kWaves];
    __shared__ uint32_t s_max_lr, s_max_ffm, s_bad;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, n = a.nlines;
    if (tid == 0) s_max_lr = s_max_ffm = s_bad = 0;
    __syncthreads();
    const uint32_t per = ((n + kWaves - 1) / kWaves + 63u) & ~63u;  // lines per wave, whole steps
    const uint32_t first = min(wave * per, n), end = min(first + per, n);
    unsigned long long lr = 0, ffm = 0;
    uint32_t mx_lr = 0, mx_ffm = 0, bad = 0;
    for (uint32_t i = first + lane; i < end; i += 64) {
        const uint4 c = a.counts[i];
        bad |= c.x == 0;
        lr += c.y;
        ffm += c.z;
        mx_lr = max(mx_lr, c.y);
        mx_ffm = max(mx_ffm, c.z);
    }
    lr = wave_total(lr);
    ffm = wave_total(ffm);
    if (lane == 0) {
        s_lr[wave] = lr;
        s_ffm[wave] = ffm;
    }
    if (mx_lr) atomicMax(&s_max_lr, mx_lr);
    if (mx_ffm) atomicMax(&s_max_ffm, mx_ffm);
    if (bad) atomicOr(&s_bad, 1u);
    __syncthreads();
    unsigned long long at_lr = 0, at_ffm = 0, tot_lr = 0, tot_ffm = 0;  // the wave's first entries; the totals
    for (uint32_t w = 0; w < kWaves; w++) {
        if (w < wave) {
            at_lr += s_lr[w];
            at_ffm += s_ffm[w];
        }
        tot_lr += s_lr[w];
        tot_ffm += s_ffm[w];
    }
    const bool fits = tot_lr <= 0xffffffffull && tot_ffm <= 0xffffffffull;
    for (uint32_t i0 = first; i0 < end && fits; i0 += 64) {  // (wave-uniform bounds: every lane takes part in the step's scans)
        const uint32_t i = i0 + lane;
        const uint4 c = i < end ? a.counts[i] : make_uint4(0u, 0u, 0u, 0u);
        const uint32_t inc_lr = wave_scan_incl(c.y, lane), inc_ffm = wave_scan_incl(c.z, lane);  // (64 counts below 2^20 each)
        if (i < end) a.counts[i] = make_uint4(c.x, (uint32_t)(at_ffm + inc_ffm - c.z), (uint32_t)(at_lr + inc_lr - c.y), c.w);
        at_lr += (uint32_t)__shfl((int)inc_lr, 63, 64);
        at_ffm += (uint32_t)__shfl((int)inc_ffm, 63, 64);
    }
    if (tid == 0) {
        RtTotals o;
        o.fallback = (s_bad || !fits) ? 1u : 0u;
        o.max_lr = s_max_lr;
        o.max_ffm = s_max_ffm;
        o.pad_ = 0;
        o.tot_lr = tot_lr;
        o.tot_ffm = tot_ffm;
        *a.totals = o;
    }
    for (uint32_t r = tid; r <= a.n_requests; r += kRtScanThreads) {
        const uint32_t pos = a.t_off[r];
        uint32_t lo = 0, hi = n;  // the first line i in [0, n] with lstart[i] >= pos (lstart[n] is the text's length)
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (a.lstart[mid] < pos) lo = mid + 1;
            else hi = mid;
        }
        a.first_line[r] = lo;
    }
}

}  // namespace

size_t requests_text_lds_bytes(const DevTranslator &t) {
    const size_t bytes = 4 * ((size_t)tr_words(t) + (size_t)kRtLines * base_words(t) + kRtCtxWords + (size_t)kRtLines * kRtRecWords);
    return bytes <= kRtLdsLimit ? bytes : 0;
}

hipError_t launch_requests_text_count(const RtArgs &a, hipStream_t stream) {
    const size_t lds = requests_text_lds_bytes(a.tr);
    if (!lds || a.nlines == 0 || a.n_requests == 0) return hipErrorInvalidValue;
    requests_text_kernel<false><<<(a.nlines + kRtLines - 1) / kRtLines, 64 * kRtLines, lds, stream>>>(a);
    requests_text_scan<<<1, kRtScanThreads, 0, stream>>>(a);
    return hipGetLastError();
}

hipError_t launch_requests_text_emit(const RtArgs &a, hipStream_t stream) {
    const size_t lds = requests_text_lds_bytes(a.tr);
    if (!lds || a.nlines == 0 || a.n_requests == 0) return hipErrorInvalidValue;
    requests_text_kernel<true><<<(a.nlines + kRtLines - 1) / kRtLines, 64 * kRtLines, lds, stream>>>(a);
    return hipGetLastError();
}

}  // namespace fwgpu
