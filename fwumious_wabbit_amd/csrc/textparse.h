// Device text route: what textparse.hip (kernels) and text_parser.cpp (host side, C ABI) share.  Not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace fwgpu {

constexpr uint32_t kTextDeviceOk = 1, kTextNeedsHost = 2;  // per-line status
constexpr uint32_t kTextHostDone = 3;  // training from text: the host parsed the line and wrote its record length and entry counts into the status entry
constexpr uint32_t kTextNoHoldout = 0xffffffffu;  // text_batch_plan's learn_before: every taken line may be learned
constexpr uint32_t kTextMaxNamespaces = 256;               // slot words a wave keeps in LDS; a larger map goes to the host whole
constexpr uint32_t kTextPad = 64;                          // readable bytes the text allocation has after its last byte

// fwgpu_parser's namespace table (parser_types.h build_ns_table) in device memory
struct TextNsTable {
    const int32_t *slots;        // [mask + 1] entry or -1
    const uint32_t *name_off;    // [n_entries + 1] into names
    const unsigned char *names;  // the vw names back to back
    const uint32_t *seed;        // murmur3(vwname, 0) per entry
    const uint32_t *index;       // namespace_index per entry
    const uint8_t *f32;          // NamespaceFormat::F32 per entry
    uint32_t mask, n_entries, num_namespaces, skip_prefix;
};
__host__ __device__ inline bool ns_ok(const TextNsTable &t) { return t.slots && t.num_namespaces <= kTextMaxNamespaces; }

// The translator as the status pass needs it for a line's entry counts (translate.cpp count_record) and for the cache's record rule
// (context_cache.cpp block_cache_record_ok): combos as CSR over namespaces, the (field, namespace) pairs in field order.  combo_off == NULL: no counts.
struct TextTranslator {
    const uint32_t *combo_off;  // [n_combos + 1]
    const uint32_t *combo_ns;
    const uint32_t *pair_ns;    // [n_pairs]; none when ffm_k == 0
    const uint32_t *pair_fk;    // field * ffm_k of each pair (an FFM entry's contra_field_index)
    uint32_t n_combos, n_pairs, add_const, ffm_mask;
};

// Candidate mode: every line is a candidate of one context, whose record the device holds (fwgpu_block_cache::d_ctx_rec).  ctx_rec == NULL: plain mode.
struct TextCandidate {
    const uint32_t *ctx_rec;  // [ctx_len]
    uint32_t ctx_len;
    const uint32_t *cover;    // bit per namespace slot below n_cover_slots: the context filled it
    uint32_t n_cover_slots;
    const uint64_t *present;  // sorted (masked hash << 32 | field * k) of the cached FFM features
    uint32_t n_present;
};

constexpr uint32_t kTextRecordOk = 1u << 8;  // in status.x beside the status: the cache's record rule holds for the line (candidate mode)

struct TextParseArgs {
    const unsigned char *text;  // 16-byte aligned, kTextPad readable bytes after the end
    const uint32_t *lstart;     // [nlines + 1]
    uint32_t nlines;
    TextNsTable ns;
    TextTranslator tr;
    TextCandidate cand;
    uint32_t set_word1, word1;  // set_word1: word 1 of every record written is word1 (serving zeroes the label)
    uint4 *status;              // [nlines] {status (| kTextRecordOk), record length, LR entries, FFM entries}: written by the status pass, read by the write pass
    // write pass: lines [0, n_used) with status DEVICE_OK go to dst + dst_off[line]
    uint32_t n_used;
    const uint64_t *dst_off;
    uint32_t *dst;
    uint32_t *long_list, *long_count;  // lines beyond the four-wave kernel's LDS image, for the single-wave one
};

size_t text_scan_temp_bytes(uint32_t n16_max);
// cnt, rank: [ceil(len / 16) + 1]; rank[ceil(len / 16)] = number of '\n' bytes
hipError_t text_count_lines(const unsigned char *text, uint32_t len, uint32_t *cnt, uint32_t *rank, void *tmp, size_t tmp_bytes, hipStream_t stream);
hipError_t text_line_index(const unsigned char *text, uint32_t len, const uint32_t *rank, int tail, uint32_t *lstart, hipStream_t stream);
hipError_t text_parse_launch(const TextParseArgs &a, bool write, hipStream_t stream);

// ---- micro-batch plan of a piece (training from text): placement, per-launch statistics and the host's lines, all from the status array.
// The first n_take lines are taken.  They are cut into launch windows of at most micro_batch lines, and no window straddles line learn_before
// (the first line that is predicted instead of learned; kTextNoHoldout: none): windows [0, n_windows_learn) cover lines [0, n_learn), the others
// the rest.  A line counts with its status entry's {length, LR entries, FFM entries} when its status is DEVICE_OK or HOST_DONE, with zeros otherwise.
struct TextPlanShape {
    uint32_t n_learn, n_windows_learn, n_windows;
    __host__ __device__ void window(uint32_t w, uint32_t micro_batch, uint32_t n_take, uint32_t *first, uint32_t *end) const {
        const bool learn = w < n_windows_learn;
        const uint64_t f = learn ? (uint64_t)w * micro_batch : n_learn + (uint64_t)(w - n_windows_learn) * micro_batch;
        const uint64_t lim = learn ? n_learn : n_take, e = f + micro_batch < lim ? f + micro_batch : lim;
        *first = (uint32_t)f;
        *end = (uint32_t)e;
    }
};
inline TextPlanShape text_plan_shape(uint32_t n_take, uint32_t micro_batch, uint32_t learn_before) {
    TextPlanShape s;
    s.n_learn = learn_before < n_take ? learn_before : n_take;
    s.n_windows_learn = (uint32_t)(((uint64_t)s.n_learn + micro_batch - 1) / micro_batch);
    s.n_windows = s.n_windows_learn + (uint32_t)(((uint64_t)(n_take - s.n_learn) + micro_batch - 1) / micro_batch);
    return s;
}
constexpr uint32_t kTextPlanStats = 7;  // per window: examples, words, max_lr, max_ffm, max_rec, tot_lr, tot_ffm (RecordStats of the window's records)
size_t text_plan_temp_bytes(uint32_t nlines_max);
// the NEEDS_HOST lines of [0, nlines), in order, and their number (device memory)
hipError_t text_host_lines(const uint4 *status, uint32_t nlines, uint32_t *host_lines, uint32_t *count, void *tmp, size_t tmp_bytes, hipStream_t stream);
// rec_off[0 .. n_take]: word offset of every taken line's record (the write pass's dst_off, the launches' rec_off) and their total;
// win_stats[kTextPlanStats * n_windows]; host_off[j] = rec_off[host_lines[j]] for the first n_host listed lines (0 for a line beyond n_take)
hipError_t text_batch_plan(const uint4 *status, uint32_t n_take, uint32_t micro_batch, uint32_t learn_before, uint64_t *rec_off, uint64_t *win_stats,
                           const uint32_t *host_lines, uint32_t n_host, uint64_t *host_off, void *tmp, size_t tmp_bytes, hipStream_t stream);
// A launch window's offsets rebased to a copy of its records alone (the delayed protocol's ring, trainer.cpp): rec_off_first = rec_off + first of the
// piece's plan, out[i] = rec_off[first + i] - rec_off[first] for i = 0 .. n (n + 1 entries; out holds at least that many)
hipError_t text_window_offsets(const uint64_t *rec_off_first, uint32_t n, uint64_t *out, hipStream_t stream);

}  // namespace fwgpu
