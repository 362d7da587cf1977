// Many requests' candidates from their TEXT to the entry batch of the requests kernels, on the device: what requests_text.hip (kernels) and
// serving.cpp (fwgpu_predictor_predict_requests_text) share.  Not part of the C ABI.
#pragma once

#include "fwgpu_internal.h"

namespace fwgpu {

constexpr uint32_t kRtLines = 4;          // candidate lines (wavefronts) per workgroup of the count and emit kernels
constexpr uint32_t kRtRecWords = 1024;    // a wave's LDS image of its candidate's record; a longer record is read through the L2
constexpr uint32_t kRtCtxWords = 2048;    // the workgroup's LDS image of the context's record, when its lines share a request and it fits
constexpr uint32_t kRtScanThreads = 1024; // the scan kernel: one workgroup, a contiguous run of lines per wave
constexpr uint32_t kRtMaxRecord = 16383;  // a slot word has 14 bits for a range's first position (parser.rs:62-66)
constexpr size_t kRtLdsLimit = 64 * 1024; // a translator whose tables do not fit beside the images takes the host route

// One cache of the call's set as the kernels read it: what TextCandidate holds for the single-request route, per cache
struct RtCache {
    const uint32_t *ctx_rec;         // the context's own record ...
    const uint32_t *cover;           // ... and a bit per namespace slot it fills
    const uint64_t *present;         // sorted (masked hash << 32 | field * k) of the cached FFM features
    const uint64_t *present_bits;    // [64] the 4096-bit filter in front of them (context_cache.cpp present_bit)
    uint32_t ctx_len, n_present;
};

// the block the host reads back after the scan, followed by first_line[n_requests + 1]
struct RtTotals {
    uint32_t fallback;               // some line needs the other route
    uint32_t max_lr, max_ffm, pad_;
    unsigned long long tot_lr, tot_ffm;
};

struct RtArgs {
    // ---- the parse (textparse.hip, plain mode): the lines' stand-alone records
    const unsigned char *text;
    const uint32_t *lstart;          // [nlines + 1]
    const uint4 *status;             // [nlines]
    const uint32_t *records;
    const uint64_t *rec_off;         // [nlines + 1]
    uint32_t nlines, nns;            // nns: namespace slots of a record
    // ---- the requests
    const uint32_t *t_off;           // [n_requests + 1] byte offset of every request's text
    const uint32_t *cache_of_request;
    const RtCache *caches;
    uint32_t n_requests;
    DevTranslator tr;
    uint32_t ffm_k;
    int32_t has_lr;
    // ---- count pass -> scan -> emit pass
    uint4 *counts;                   // [nlines] {ok, LR entries, FFM entries, request}; after the scan {ok, first FFM entry, first LR entry, request}
    uint32_t *cache_of;              // [nlines] the cache of every line's request (the count pass writes it: fwgpu_batch_set_caches' index array)
    RtTotals *totals;
    uint32_t *first_line;            // [n_requests + 1] behind the totals
    // ---- the entry batch (fwgpu_batch): example i is line i
    uint32_t *ffm_hash, *ffm_off, *lr_hash, *lr_off;
    float *ffm_val, *lr_val, *label, *importance;
    uint8_t *ffm_fld;
    uint16_t *lr_combo;
};

// dynamic LDS of the count / emit kernels; 0: the translator's tables do not fit kRtLdsLimit
size_t requests_text_lds_bytes(const DevTranslator &t);
hipError_t launch_requests_text_count(const RtArgs &a, hipStream_t stream);  // count pass, then the scan (totals, offsets, first_line)
hipError_t launch_requests_text_emit(const RtArgs &a, hipStream_t stream);

}  // namespace fwgpu
