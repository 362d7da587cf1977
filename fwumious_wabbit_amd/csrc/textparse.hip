// VW text -> u32 records on the device (parser.rs:214-461 next_vowpal_to_size, as parser.cpp's parse_head / parse_body mirror it).
//
// Line index: 16-byte loads count the '\n' bytes of every 16-byte piece, a rocPRIM scan turns the counts into ranks, a second pass
// writes line_start[rank + 1] = position + 1.
//
// Line -> record: one wavefront per line.  The line is copied to LDS with 16-byte loads (coalesced) and everything after that reads LDS.
//   1. head (label, importance, first '|'): a handful of bytes, scanned by every lane alike;
//   2. token starts (a non-space byte after a space) by ballot, compacted into an LDS list;
//   3. one lane per token: end, first ':', weight, namespace lookup (exact bytes) or murmur3 with the seed of the namespace in force -- the
//      last '|' token before it, a "last set" scan over the ballot of namespace tokens, carried from one group of 64 tokens to the next;
//   4. the layout (in-place single features, promotion, slot words) is the reference's state machine over the token list in LDS.
// The kernel never guesses: whatever is not a plain example it reproduces exactly gets NEEDS_HOST and the host parser takes the line.
// Lines up to 4 KiB run four waves to a workgroup; longer ones (to 64 KiB) are listed and taken by single-wave workgroups with a larger
// LDS image.  The same code runs twice: once for {status, length}, once -- when the host has placed the records -- to write them.
//
// Candidate mode (TextParseArgs::cand): the lines are the candidates of one context whose record the device holds.  A line that starts with
// '|' opens a namespace of its own, so the scan does not depend on the context and its record is the stand-alone one with the context's
// words 1 and 2 and NO_FEATURES in every slot whose merged form equals the context's slot word -- fwgpu_parser_parse_candidate's
// candidate-only record (parser.cpp).  With a translator (TextParseArgs::tr) the status pass also counts the line's LR and FFM entries
// (translate.cpp count_record) and, in candidate mode, decides the cache's record rule (context_cache.cpp block_cache_record_ok) exactly.
//
// Micro-batch plan (training from text, textparse.h): from a piece's status array alone, a rocPRIM select lists the NEEDS_HOST lines, a rocPRIM scan
// places every taken line's record, and one workgroup per launch window sums what the host would otherwise count from the records.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "f32_text.h"
#include "textparse.h"

namespace fwgpu {

namespace {

constexpr uint32_t kNotSingle = 1u << 31, kMask31 = ~kNotSingle, kNoFeatures = kNotSingle, kNoLabel = 0xff, kFloatOne = 0x3f800000u;
constexpr int kHeaderLen = 3;
constexpr int kShortStage = 4096, kShortTok = 512, kShortWaves = 4;
constexpr int kLongStage = 65536, kLongTok = 4096;

__device__ inline void wave_sync() {  // LDS written by some lanes of this wave, read by others
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ inline uint32_t murmur3_dev(const unsigned char *d, uint32_t len, uint32_t seed) {
    const uint32_t c1 = 0xcc9e2d51u, c2 = 0x1b873593u;
    uint32_t h1 = seed;
    const uint32_t nb = len >> 2;
    for (uint32_t i = 0; i < nb; i++) {
        uint32_t k1 = d[4 * i] | ((uint32_t)d[4 * i + 1] << 8) | ((uint32_t)d[4 * i + 2] << 16) | ((uint32_t)d[4 * i + 3] << 24);
        k1 *= c1;
        k1 = (k1 << 15) | (k1 >> 17);
        k1 *= c2;
        h1 ^= k1;
        h1 = (h1 << 13) | (h1 >> 19);
        h1 = h1 * 5 + 0xe6546b64u;
    }
    const unsigned char *t = d + 4 * nb;
    uint32_t k1 = 0;
    const uint32_t r = len & 3;
    if (r >= 3) k1 ^= (uint32_t)t[2] << 16;
    if (r >= 2) k1 ^= (uint32_t)t[1] << 8;
    if (r >= 1) {
        k1 ^= t[0];
        k1 *= c1;
        k1 = (k1 << 15) | (k1 >> 17);
        k1 *= c2;
        h1 ^= k1;
    }
    h1 ^= len;
    h1 ^= h1 >> 16;
    h1 *= 0x85ebca6bu;
    h1 ^= h1 >> 13;
    h1 *= 0xc2b2ae35u;
    h1 ^= h1 >> 16;
    return h1;
}

// fwgpu_parser::find_ns on the uploaded table: FNV-1a slot, linear probing, exact comparison of the bytes
__device__ inline int find_ns_dev(const TextNsTable &ns, const unsigned char *s, uint32_t n) {
    uint32_t h = 2166136261u;
    for (uint32_t i = 0; i < n; i++) h = (h ^ s[i]) * 16777619u;
    uint32_t slot = h & ns.mask;
    for (;;) {
        const int e = ns.slots[slot];
        if (e < 0) return -1;
        const uint32_t a = ns.name_off[e], l = ns.name_off[e + 1] - a;
        if (l == n) {
            uint32_t j = 0;
            while (j < n && ns.names[a + j] == s[j]) j++;
            if (j == n) return e;
        }
        slot = (slot + 1) & ns.mask;
    }
}

// a weight / importance / f32 value the kernel may use: in the grammar, proven, finite, not "NONE"
__device__ inline bool number_dev(const unsigned char *s, uint32_t n, uint32_t *bits) {
    if (n == 4 && s[0] == 'N' && s[1] == 'O' && s[2] == 'N' && s[3] == 'E') return false;
    const F32Text r = f32_from_text(s, n);
    *bits = r.bits;
    return r.grammar && r.proven && (r.bits & 0x7f800000u) != 0x7f800000u;
}

struct LineLds {
    unsigned char *stage;  // 16-byte aligned, STAGE + 32 bytes
    uint16_t *tok_start;
    uint8_t *tok_kind;  // 0 namespace, 1 plain feature (both weights 1), 2 weighted feature, 3 feature of an f32 namespace
    uint32_t *tok_a;    // namespace: entry; feature: hash
    uint32_t *tok_w;    // feature: bits of ns_weight * weight, or of the f32 value
    uint32_t *slots;    // [kTextMaxNamespaces]
    uint16_t *slot_run; // [kTextMaxNamespaces] first feature token of the run a filled slot holds
};

struct LineFacts {  // what the status pass reports beside the status
    uint32_t len = 0, n_lr = 0, n_ffm = 0;
    bool record_ok = false;
};

__device__ inline uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// is (hash & mask, field * k) a cached feature: fwgpu_block_cache::present is sorted
__device__ inline bool present_dev(const TextCandidate &cd, uint32_t masked_hash, uint32_t fk) {
    const uint64_t key = ((uint64_t)masked_hash << 32) | fk;
    uint32_t lo = 0, hi = cd.n_present;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const uint64_t v = cd.present[mid];
        if (v == key) return true;
        if (v < key) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

// One line by one wave.  Returns the status (wave-uniform); *facts: record length, entry counts, record rule.  WRITE: `dst` is where the record goes.
// CAND: the line is a candidate of a.cand's context.
template <int TOKCAP, bool WRITE, bool CAND>
__device__ uint32_t parse_line_wave(const TextParseArgs &a, uint32_t start, uint32_t size, const LineLds &L, uint32_t *dst, LineFacts *facts) {
    const uint32_t lane = threadIdx.x & 63u;
    const TextNsTable &ns = a.ns;
    const uint32_t rowlen = size - 1;  // "ignore last newline byte": the line's last byte only ever answers the one-past reads
    // ---- stage
    const uint32_t base = start & ~15u, o = start & 15u, nvec = (o + size + 15u) >> 4;
    const uint4 *src = reinterpret_cast<const uint4 *>(a.text + base);
    uint4 *sd = reinterpret_cast<uint4 *>(L.stage);
    for (uint32_t v = lane; v < nvec; v += 64) sd[v] = src[v];
    wave_sync();
    const unsigned char *c = L.stage + o;
    // ---- head (parser.rs:226-316)
    const unsigned char c0 = c[0];
    if (c0 != '1' && c0 != '-' && c0 != '|') return kTextNeedsHost;  // commands and errors
    if (CAND && c0 != '|') return kTextNeedsHost;  // a label, or a feature token that goes on in the context's last namespace
    const uint32_t label = c0 == '1' ? 1u : c0 == '-' ? 0u : kNoLabel;
    uint32_t imp = kFloatOne, ie = 0;
    if (c0 != '|') {
        while (ie < rowlen && c[ie] != ' ') ie++;
        while (ie < rowlen && c[ie] == ' ') ie++;
        if (c[ie] != '|') {
            const uint32_t is = ie;
            while (ie < rowlen && c[ie] != ' ') ie++;
            if (!number_dev(c + is, ie - is, &imp)) return kTextNeedsHost;
            if (__uint_as_float(imp) < 0.0f) return kTextNeedsHost;
        }
    }
    while (ie < rowlen && c[ie] != '|') ie++;
    const uint32_t pos = ie;
    // a line that ends in two spaces makes the reference scan one more, empty, token at the line's last byte
    if (rowlen >= 2 && rowlen > pos && c[rowlen - 1] == ' ' && c[rowlen - 2] == ' ') return kTextNeedsHost;
    // ---- token starts
    uint32_t ntok = 0;
    for (uint32_t k = pos; k < rowlen; k += 64) {
        const uint32_t b = k + lane;
        bool st = false;
        if (b < rowlen) st = c[b] != ' ' && (b == pos || c[b - 1] == ' ');
        const unsigned long long m = __ballot(st);
        const uint32_t idx = ntok + __popcll(m & ((1ull << lane) - 1ull));
        if (st && idx < (uint32_t)TOKCAP) L.tok_start[idx] = (uint16_t)b;
        ntok += __popcll(m);
    }
    if (ntok > (uint32_t)TOKCAP) return kTextNeedsHost;
    wave_sync();
    // ---- one lane per token
    int carry_ent = -1;
    uint32_t carry_w = kFloatOne;
    bool any_bad = false;
    for (uint32_t g = 0; g < ntok; g += 64) {
        const uint32_t t = g + lane;
        const bool valid = t < ntok;
        bool bad = false, isns = false;
        uint32_t s = 0, e = 0, ef = 0, wbits = kFloatOne;
        int ent = -1;
        if (valid) {
            s = L.tok_start[t];
            e = s;
            bool colon = false;
            while (e < rowlen && c[e] != ' ') {
                if (c[e] == ':' && !colon) colon = true, ef = e;
                e++;
            }
            if (!colon) ef = e;
            isns = c[s] == '|';
            if (ef != e && !number_dev(c + ef + 1, e - ef - 1, &wbits)) bad = true;
            if (isns) {
                ent = find_ns_dev(ns, c + s + 1, ef - s - 1);
                if (ent < 0) bad = true;  // not predeclared
            }
        }
        const unsigned long long nsmask = __ballot(valid && isns);
        const unsigned long long below = nsmask & ((2ull << lane) - 1ull);
        const int srcl = below ? 63 - __clzll((long long)below) : 0;
        const int got_ent = __shfl(ent, srcl, 64);
        const uint32_t got_w = __shfl(wbits, srcl, 64);
        const int my_ent = below ? got_ent : carry_ent;
        const uint32_t my_nsw = below ? got_w : carry_w;
        if (nsmask) {
            const int top = 63 - __clzll((long long)nsmask);
            carry_ent = __shfl(ent, top, 64);
            carry_w = __shfl(wbits, top, 64);
        }
        if (valid) {
            uint32_t kind = 0, av = (uint32_t)ent, wv = 0;
            if (!isns) {
                if (my_ent < 0) {
                    bad = true;
                } else {
                    av = murmur3_dev(c + s, ef - s, ns.seed[my_ent]) & kMask31;
                    const float nsw = __uint_as_float(my_nsw), fw = __uint_as_float(wbits);
                    const float prod = __fmul_rn(nsw, fw);
                    if (ns.f32[my_ent]) {
                        kind = 3;
                        const uint32_t fs = s + ns.skip_prefix;
                        wv = 0x7fc00000u;  // no value after the prefix: NaN
                        if (fs > ef) bad = true;
                        else if (fs != ef && !number_dev(c + fs, ef - fs, &wv)) bad = true;
                        if (prod != 1.0f) bad = true;
                    } else {
                        kind = (nsw == 1.0f && fw == 1.0f) ? 1 : 2;
                        wv = __float_as_uint(prod);
                    }
                }
            }
            L.tok_kind[t] = (uint8_t)kind;
            L.tok_a[t] = av;
            L.tok_w[t] = wv;
        }
        any_bad = any_bad || __ballot(valid && bad) != 0ull;
    }
    if (any_bad) return kTextNeedsHost;
    // ---- layout (parser.rs:318-457), every lane alike; lane 0 stores
    const uint32_t nns = ns.num_namespaces;
    for (uint32_t j = lane; j < nns; j += 64) L.slots[j] = kNoFeatures;
    wave_sync();
    uint32_t len = kHeaderLen + nns, ns_slot = 0, ns_start = 0, ns_count = 0;
    auto push = [&](uint32_t x) {
        if (WRITE && lane == 0) dst[len] = x;
        len++;
    };
    for (uint32_t t = 0; t < ntok; t++) {
        const uint32_t kind = L.tok_kind[t], av = L.tok_a[t];
        if (kind == 0) {
            ns_slot = ns.index[av];
            ns_count = 0;
            ns_start = len;
            continue;
        }
        if (ns_count == 0) L.slot_run[ns_slot] = (uint16_t)t;
        if (kind == 1 && ns_count == 0) {
            L.slots[ns_slot] = av;
        } else {
            const uint32_t cur = L.slots[ns_slot];
            if (ns_count == 1 && (cur & kNotSingle) == 0) {  // promote the in-place feature
                push(cur);
                push(kFloatOne);
            }
            push(av);
            push(L.tok_w[t]);
            L.slots[ns_slot] = kNotSingle | ((ns_start << 16) + len);
        }
        ns_count++;
    }
    if (len > 65535u) return kTextNeedsHost;  // the slot word has 16 bits for a position
    const bool count = !WRITE && a.tr.combo_off != nullptr;
    // entry counts read 14-bit start positions; in the context's record + this one a range lies ctx_len - (header + slots) further on
    if ((CAND || count) && (CAND ? a.cand.ctx_len - (kHeaderLen + nns) : 0u) + len > 16383u) return kTextNeedsHost;
    facts->len = len;
    wave_sync();
    if (CAND) {  // a single feature the context's slot already holds: "as in the context"
        for (uint32_t j = lane; j < nns; j += 64) {
            const uint32_t w = L.slots[j];
            if ((w & kNotSingle) == 0 && w == a.cand.ctx_rec[kHeaderLen + j]) L.slots[j] = kNoFeatures;
        }
        wave_sync();
    }
    if (count) {
        const TextTranslator &tr = a.tr;
        auto cnt = [&](uint32_t nsi) -> uint32_t {
            uint32_t w = L.slots[nsi];
            if (CAND && w == kNoFeatures) w = a.cand.ctx_rec[kHeaderLen + nsi];  // inherited
            if ((w & kNotSingle) == 0) return 1u;
            return ((w & 0xffffu) - ((w >> 16) & 0x3fffu)) >> 1;
        };
        constexpr unsigned long long kCap = 2000000ull;  // count_record refuses beyond 1 000 000
        unsigned long long lr = 0;
        for (uint32_t ci = lane; ci < tr.n_combos; ci += 64) {
            unsigned long long prod = 1;
            for (uint32_t m = tr.combo_off[ci]; m < tr.combo_off[ci + 1]; m++) prod = min(prod * cnt(tr.combo_ns[m]), kCap);
            lr = min(lr + prod, kCap);
        }
        uint32_t ffm = 0;
        for (uint32_t j = lane; j < tr.n_pairs; j += 64) ffm += cnt(tr.pair_ns[j]);
        const uint32_t n_lr = wave_sum((uint32_t)lr) + tr.add_const, n_ffm = wave_sum(ffm);
        if (n_lr > 1000000u || n_ffm > 1000000u) return kTextNeedsHost;
        facts->n_lr = n_lr;
        facts->n_ffm = n_ffm;
        if (CAND) {
            const TextCandidate &cd = a.cand;
            auto covered = [&](uint32_t nsi) { return nsi < cd.n_cover_slots && ((cd.cover[nsi >> 5] >> (nsi & 31u)) & 1u) != 0; };
            bool bad = false;
            for (uint32_t j = lane; j < cd.n_cover_slots; j += 64) bad = bad || (covered(j) && L.slots[j] != kNoFeatures);
            for (uint32_t j = lane; j < tr.n_pairs; j += 64) {
                const uint32_t nsi = tr.pair_ns[j], fk = tr.pair_fk[j];
                if (covered(nsi)) continue;
                const uint32_t w = L.slots[nsi];
                if ((w & kNotSingle) == 0) {
                    bad = bad || present_dev(cd, w & tr.ffm_mask, fk);
                } else if (w != kNoFeatures) {  // the run's feature tokens are the range's features, in order
                    for (uint32_t t = L.slot_run[nsi]; t < ntok && L.tok_kind[t] != 0; t++) bad = bad || present_dev(cd, L.tok_a[t] & tr.ffm_mask, fk);
                }
            }
            facts->record_ok = __ballot(bad) == 0ull;
        }
    }
    if (WRITE) {
        if (lane == 0) {
            dst[0] = len;
            dst[1] = a.set_word1 ? a.word1 : CAND ? a.cand.ctx_rec[1] : label;
            dst[2] = CAND ? a.cand.ctx_rec[2] : imp;
        }
        for (uint32_t j = lane; j < nns; j += 64) dst[kHeaderLen + j] = L.slots[j];
    }
    return kTextDeviceOk;
}

template <int STAGE, int TOKCAP>
__device__ inline LineLds carve(unsigned char *p) {
    LineLds L;
    L.stage = p;
    p += STAGE + 32;
    L.tok_a = reinterpret_cast<uint32_t *>(p);
    p += 4 * TOKCAP;
    L.tok_w = reinterpret_cast<uint32_t *>(p);
    p += 4 * TOKCAP;
    L.slots = reinterpret_cast<uint32_t *>(p);
    p += 4 * kTextMaxNamespaces;
    L.tok_start = reinterpret_cast<uint16_t *>(p);
    p += 2 * TOKCAP;
    L.slot_run = reinterpret_cast<uint16_t *>(p);
    p += 2 * kTextMaxNamespaces;
    L.tok_kind = p;
    return L;
}
template <int STAGE, int TOKCAP>
constexpr int lds_bytes() {
    return STAGE + 32 + 11 * TOKCAP + 6 * kTextMaxNamespaces;
}

// WRITE: does this line's record get written, and where
__device__ inline bool write_target(const TextParseArgs &a, uint32_t line, uint32_t **dst) {
    if (line >= a.n_used || (a.status[line].x & 0xffu) != kTextDeviceOk) return false;
    *dst = a.dst + a.dst_off[line];
    return true;
}

__device__ inline uint4 status_word(uint32_t status, const LineFacts &f) {
    if (status != kTextDeviceOk) return make_uint4(status, 0u, 0u, 0u);
    return make_uint4(status | (f.record_ok ? kTextRecordOk : 0u), f.len, f.n_lr, f.n_ffm);
}

template <bool WRITE, bool CAND>
__global__ __launch_bounds__(64 * kShortWaves) void text_parse_short(TextParseArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[kShortWaves][lds_bytes<kShortStage, kShortTok>()];
    static_assert(lds_bytes<kShortStage, kShortTok>() % 16 == 0, "wave images stay 16-byte aligned");
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t line = blockIdx.x * kShortWaves + wave;
    if (line >= a.nlines) return;
    const uint32_t start = a.lstart[line], size = a.lstart[line + 1] - start;
    uint32_t *dst = nullptr;
    if (WRITE && !write_target(a, line, &dst)) return;
    uint32_t status = kTextNeedsHost;
    LineFacts facts;
    if (ns_ok(a.ns) && size >= 1 && size <= (uint32_t)kLongStage) {
        if (size > (uint32_t)kShortStage) {  // for the single-wave workgroups
            if (lane == 0) a.long_list[atomicAdd(a.long_count, 1u)] = line;
            return;
        }
        status = parse_line_wave<kShortTok, WRITE, CAND>(a, start, size, carve<kShortStage, kShortTok>(lds[wave]), dst, &facts);
    }
    if (!WRITE && lane == 0) a.status[line] = status_word(status, facts);
}

template <bool WRITE, bool CAND>
__global__ __launch_bounds__(64) void text_parse_long(TextParseArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[lds_bytes<kLongStage, kLongTok>()];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n = *a.long_count;
    for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {
        const uint32_t line = a.long_list[k];
        const uint32_t start = a.lstart[line], size = a.lstart[line + 1] - start;
        uint32_t *dst = nullptr;
        if (WRITE && !write_target(a, line, &dst)) continue;
        LineFacts facts;
        const uint32_t status = parse_line_wave<kLongTok, WRITE, CAND>(a, start, size, carve<kLongStage, kLongTok>(lds), dst, &facts);
        if (!WRITE && lane == 0) a.status[line] = status_word(status, facts);
        wave_sync();  // the next line reuses the image
    }
}

// ---- line index
__device__ inline uint32_t newline_mask16(uint4 v, uint32_t at, uint32_t len) {  // bit j: byte at + j is a '\n' of the text
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
    for (int q = 0; q < 4; q++)
        for (int j = 0; j < 4; j++)
            if (((w[q] >> (8 * j)) & 0xffu) == '\n' && at + 4 * q + j < len) m |= 1u << (4 * q + j);
    return m;
}

__global__ void text_count_newlines(const uint4 *text, uint32_t n16, uint32_t len, uint32_t *cnt) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n16) cnt[t] = __popc(newline_mask16(text[t], 16 * t, len));
    else if (t == n16) cnt[t] = 0;
}

__global__ void text_line_starts(const uint4 *text, uint32_t n16, uint32_t len, const uint32_t *rank, int tail, uint32_t *lstart) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) {
        lstart[0] = 0;
        if (tail) lstart[rank[n16] + 1] = len;  // a last line without a newline is a line
    }
    if (t >= n16) return;
    uint32_t m = newline_mask16(text[t], 16 * t, len), r = rank[t];
    while (m) {
        const int j = __ffs(m) - 1;
        m &= m - 1;
        lstart[++r] = 16 * t + j + 1;
    }
}

// ---- micro-batch plan (textparse.h): one scan for the placement, one workgroup per launch window for its statistics
__host__ __device__ inline bool line_counts(uint32_t status_x) {
    const uint32_t s = status_x & 0xffu;
    return s == kTextDeviceOk || s == kTextHostDone;
}

struct PlanLineLen {  // record length of line i as the placement counts it; line n_take (one past) closes the scan
    const uint4 *status;
    uint32_t n_take;
    __host__ __device__ uint64_t operator()(uint32_t i) const {
        if (i >= n_take) return 0;
        const uint4 s = status[i];
        return line_counts(s.x) ? (uint64_t)s.y : 0ull;
    }
};

struct PlanNeedsHost {
    const uint4 *status;
    __host__ __device__ bool operator()(uint32_t i) const { return (status[i].x & 0xffu) == kTextNeedsHost; }
};

__global__ void text_plan_windows(const uint4 *status, uint32_t n_take, uint32_t micro_batch, TextPlanShape shape, const uint64_t *rec_off, uint64_t *win_stats) {
    __shared__ uint32_t s_max[3][4];
    __shared__ unsigned long long s_tot[2][4];
    const uint32_t w = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    uint32_t first, end;
    shape.window(w, micro_batch, n_take, &first, &end);
    uint32_t mx[3] = {0, 0, 0};
    unsigned long long tot[2] = {0, 0};
    for (uint32_t i = first + threadIdx.x; i < end; i += blockDim.x) {
        const uint4 s = status[i];
        if (!line_counts(s.x)) continue;
        mx[0] = max(mx[0], s.z);
        mx[1] = max(mx[1], s.w);
        mx[2] = max(mx[2], s.y);
        tot[0] += s.z;
        tot[1] += s.w;
    }
    for (int o = 32; o; o >>= 1) {
        for (int q = 0; q < 3; q++) mx[q] = max(mx[q], (uint32_t)__shfl_xor((int)mx[q], o, 64));
        for (int q = 0; q < 2; q++) tot[q] += __shfl_xor(tot[q], o, 64);
    }
    if (lane == 0) {
        for (int q = 0; q < 3; q++) s_max[q][wave] = mx[q];
        for (int q = 0; q < 2; q++) s_tot[q][wave] = tot[q];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (uint32_t v = 1; v < nwaves; v++) {
        for (int q = 0; q < 3; q++) mx[q] = max(mx[q], s_max[q][v]);
        for (int q = 0; q < 2; q++) tot[q] += s_tot[q][v];
    }
    uint64_t *o = win_stats + (size_t)kTextPlanStats * w;
    o[0] = end - first;
    o[1] = rec_off[end] - rec_off[first];
    o[2] = mx[0];
    o[3] = mx[1];
    o[4] = mx[2];
    o[5] = tot[0];
    o[6] = tot[1];
}

__global__ void text_plan_host_off(const uint64_t *rec_off, uint32_t n_take, const uint32_t *host_lines, uint32_t n_host, uint64_t *host_off) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_host) return;
    const uint32_t line = host_lines[j];
    host_off[j] = line < n_take ? rec_off[line] : 0ull;
}

// a launch window's offsets for a copy of its records that starts at word 0: lane i reads one entry, every lane the window's first (a broadcast)
__global__ void text_window_offsets_kernel(const uint64_t *rec_off, uint32_t n_off, uint64_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_off) out[i] = rec_off[i] - rec_off[0];
}

}  // namespace

hipError_t text_window_offsets(const uint64_t *rec_off_first, uint32_t n, uint64_t *out, hipStream_t stream) {
    const uint32_t n_off = n + 1;
    text_window_offsets_kernel<<<(n_off + 255) / 256, 256, 0, stream>>>(rec_off_first, n_off, out);
    return hipGetLastError();
}

size_t text_plan_temp_bytes(uint32_t nlines_max) {
    size_t a = 0, b = 0;
    (void)rocprim::exclusive_scan(nullptr, a, rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0), PlanLineLen{nullptr, 0}), (uint64_t *)nullptr,
                                  (uint64_t)0, (size_t)nlines_max + 1, rocprim::plus<uint64_t>(), (hipStream_t)0);
    (void)rocprim::select(nullptr, b, rocprim::counting_iterator<uint32_t>(0), rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0), PlanNeedsHost{nullptr}),
                          (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)nlines_max, (hipStream_t)0);
    return std::max<size_t>(std::max(a, b), 256);
}

hipError_t text_host_lines(const uint4 *status, uint32_t nlines, uint32_t *host_lines, uint32_t *count, void *tmp, size_t tmp_bytes, hipStream_t stream) {
    if (nlines == 0) return hipMemsetAsync(count, 0, 4, stream);
    hipError_t e = rocprim::select(tmp, tmp_bytes, rocprim::counting_iterator<uint32_t>(0),
                                   rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0), PlanNeedsHost{status}), host_lines, count, (size_t)nlines, stream);
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t text_batch_plan(const uint4 *status, uint32_t n_take, uint32_t micro_batch, uint32_t learn_before, uint64_t *rec_off, uint64_t *win_stats,
                           const uint32_t *host_lines, uint32_t n_host, uint64_t *host_off, void *tmp, size_t tmp_bytes, hipStream_t stream) {
    if (micro_batch == 0) return hipErrorInvalidValue;
    hipError_t e = rocprim::exclusive_scan(tmp, tmp_bytes, rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0), PlanLineLen{status, n_take}), rec_off,
                                           (uint64_t)0, (size_t)n_take + 1, rocprim::plus<uint64_t>(), stream);
    if (e != hipSuccess) return e;
    const TextPlanShape shape = text_plan_shape(n_take, micro_batch, learn_before);
    if (shape.n_windows) text_plan_windows<<<shape.n_windows, micro_batch <= 64 ? 64 : 256, 0, stream>>>(status, n_take, micro_batch, shape, rec_off, win_stats);
    if (n_host) text_plan_host_off<<<(n_host + 255) / 256, 256, 0, stream>>>(rec_off, n_take, host_lines, n_host, host_off);
    return hipGetLastError();
}

size_t text_scan_temp_bytes(uint32_t n16_max) {
    size_t b = 0;
    (void)rocprim::exclusive_scan(nullptr, b, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)n16_max + 1, rocprim::plus<uint32_t>(), (hipStream_t)0);
    return b;
}

hipError_t text_count_lines(const unsigned char *text, uint32_t len, uint32_t *cnt, uint32_t *rank, void *tmp, size_t tmp_bytes, hipStream_t stream) {
    const uint32_t n16 = (len + 15) / 16;
    text_count_newlines<<<(n16 + 1 + 255) / 256, 256, 0, stream>>>(reinterpret_cast<const uint4 *>(text), n16, len, cnt);
    hipError_t e = rocprim::exclusive_scan(tmp, tmp_bytes, cnt, rank, 0u, (size_t)n16 + 1, rocprim::plus<uint32_t>(), stream);
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t text_line_index(const unsigned char *text, uint32_t len, const uint32_t *rank, int tail, uint32_t *lstart, hipStream_t stream) {
    const uint32_t n16 = (len + 15) / 16;
    text_line_starts<<<(n16 + 255) / 256 + 1, 256, 0, stream>>>(reinterpret_cast<const uint4 *>(text), n16, len, rank, tail, lstart);
    return hipGetLastError();
}

hipError_t text_parse_launch(const TextParseArgs &a, bool write, hipStream_t stream) {
    if (a.nlines == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(a.long_count, 0, 4, stream);
    if (e != hipSuccess) return e;
    const uint32_t grid = (a.nlines + kShortWaves - 1) / kShortWaves;
    const bool cand = a.cand.ctx_rec != nullptr;
    if (write && cand) {
        text_parse_short<true, true><<<grid, 64 * kShortWaves, 0, stream>>>(a);
        text_parse_long<true, true><<<256, 64, 0, stream>>>(a);
    } else if (write) {
        text_parse_short<true, false><<<grid, 64 * kShortWaves, 0, stream>>>(a);
        text_parse_long<true, false><<<256, 64, 0, stream>>>(a);
    } else if (cand) {
        text_parse_short<false, true><<<grid, 64 * kShortWaves, 0, stream>>>(a);
        text_parse_long<false, true><<<256, 64, 0, stream>>>(a);
    } else {
        text_parse_short<false, false><<<grid, 64 * kShortWaves, 0, stream>>>(a);
        text_parse_long<false, false><<<256, 64, 0, stream>>>(a);
    }
    return hipGetLastError();
}

}  // namespace fwgpu
