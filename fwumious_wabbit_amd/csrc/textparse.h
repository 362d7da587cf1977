// Device text route: what textparse.hip (kernels) and text_parser.cpp (host side, C ABI) share.  Not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace fwgpu {

constexpr uint32_t kTextDeviceOk = 1, kTextNeedsHost = 2;  // per-line status
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
// (regressor.cpp block_cache_record_ok): combos as CSR over namespaces, the (field, namespace) pairs in field order.  combo_off == NULL: no counts.
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

}  // namespace fwgpu
