// The byte-diff stream of the reference's weight_patcher (weight_patcher/src/main.rs), host side.  Nothing from HIP is included here: the header
// is compiled into libfwgpu.so and, alone, into host/test_diff_stream.cpp.
//
// THE STREAM: what compare_files_and_write_diff hands to its writer, without the gzip container the tool wraps around it.  Two inputs of equal
// length; every index i with a[i] != b[i] gives one entry, in ascending order:
//     varint(i - prev)  b[i]
// prev is the index of the previous entry and starts at 0, so a difference at index 0 is encoded as delta 0.  The varint is little-endian
// base-128: 7 bits per byte, the top bit set on every byte but the last (write_varint, main.rs:260-266).
//
// THE READER IS STRICTER than recreate_file_inner in two places, and changes nothing unless the whole stream is valid:
//   - a stream that ends inside an entry, a varint longer than 10 bytes and one that overflows 64 bits are errors (the reference stops
//     silently on a truncated entry and shifts past 64 bits on a long varint);
//   - an entry at or beyond the target's end is an error, and so is a zero delta anywhere but in the first entry (the reference never
//     reaches the first and would apply the second to the same byte twice).
#pragma once

#include <stdint.h>

namespace fwgpu {
namespace diffstream {

enum Status {
    kOk = 0,
    kTruncated = 1,   // the stream ends inside a varint or before an entry's `to` byte
    kVarint = 2,      // a varint of more than 10 bytes, or one whose value does not fit 64 bits
    kBeyond = 3,      // an entry's index is at or beyond the target's end (or does not fit 64 bits)
    kZeroDelta = 4,   // a zero delta in an entry that is not the first
};

inline const char *status_text(int s) {
    switch (s) {
        case kOk: return "ok";
        case kTruncated: return "the stream ends inside an entry";
        case kVarint: return "a varint is longer than 10 bytes or overflows 64 bits";
        case kBeyond: return "an entry lies at or beyond the target's end";
        case kZeroDelta: return "a zero delta in an entry that is not the first";
    }
    return "?";
}

inline uint32_t varint_len(uint64_t v) {
    uint32_t n = 1;
    while (v >= 0x80) {
        v >>= 7;
        n++;
    }
    return n;
}

inline uint32_t put_varint(uint8_t *out, uint64_t v) {  // write_varint, main.rs:260-266
    uint32_t n = 0;
    while (v >= 0x80) {
        out[n++] = (uint8_t)(v & 0x7f) | 0x80;
        v >>= 7;
    }
    out[n++] = (uint8_t)v;
    return n;
}

// compare_files_and_write_diff (main.rs:68-130) on two arrays that stand for the bytes [base_offset, base_offset + n) of the two files; prev_index
// is the index of the last entry emitted before this range (0 at the start of a file; never above base_offset).  Returns the stream's size.  Entries
// are written while they fit `cap` (out may be NULL with cap 0): the stream is complete exactly when the returned size is <= cap.
// *changed: the number of entries; *last: the index of the last one, prev_index when there is none.
inline uint64_t encode(const uint8_t *a, const uint8_t *b, uint64_t n, uint64_t base_offset, uint64_t prev_index, uint8_t *out, uint64_t cap,
                       uint64_t *changed, uint64_t *last) {
    uint64_t size = 0, count = 0, prev = prev_index;
    for (uint64_t i = 0; i < n; i++) {
        if (a[i] == b[i]) continue;
        const uint64_t index = base_offset + i, delta = index - prev;
        const uint32_t len = varint_len(delta) + 1;
        if (out && size + len <= cap) {
            const uint32_t v = put_varint(out + size, delta);
            out[size + v] = b[i];
        }
        size += len;
        prev = index;
        count++;
    }
    if (changed) *changed = count;
    if (last) *last = prev;
    return size;
}

// read_diff_entry + read_varint (main.rs:208-246) over a whole stream, with the checks above.  end: one past the last index an entry may
// have.  visit(index, to) is called for every entry in order; nothing is called after an error, so callers that must change nothing on a bad
// stream walk twice, the first time with a visitor that does nothing.  *entries: entries seen before the error, or all of them.
template <class Visit>
inline int walk(const uint8_t *diff, uint64_t len, uint64_t end, Visit &&visit, uint64_t *entries = nullptr) {
    uint64_t at = 0, index = 0, count = 0;
    int status = kOk;
    while (at < len) {
        uint64_t delta = 0;
        uint32_t k = 0;
        for (;; k++) {
            if (at >= len) {
                status = kTruncated;
                break;
            }
            if (k == 10) {
                status = kVarint;
                break;
            }
            const uint8_t byte = diff[at++];
            if (k == 9 && (byte & 0x7f) > 1) {  // bit 63 is the last that fits
                status = kVarint;
                break;
            }
            delta |= (uint64_t)(byte & 0x7f) << (7 * k);
            if (!(byte & 0x80)) break;
        }
        if (status) break;
        if (at >= len) {
            status = kTruncated;
            break;
        }
        const uint8_t to = diff[at++];
        if (count && !delta) {
            status = kZeroDelta;
            break;
        }
        if (delta > UINT64_MAX - index || index + delta >= end) {
            status = kBeyond;
            break;
        }
        index += delta;
        visit(index, to);
        count++;
    }
    if (entries) *entries = count;
    return status;
}

// recreate_file_inner (main.rs:148-206) in place on `target`, which stands for the file's bytes [base_offset, base_offset + n).  Entries below
// base_offset are skipped.  Nothing is written unless the whole stream is valid.  *applied: entries written into the target.
inline int apply(uint8_t *target, uint64_t n, uint64_t base_offset, const uint8_t *diff, uint64_t len, uint64_t *applied) {
    if (applied) *applied = 0;
    const uint64_t end = base_offset > UINT64_MAX - n ? UINT64_MAX : base_offset + n;
    const int status = walk(diff, len, end, [](uint64_t, uint8_t) {});
    if (status) return status;
    uint64_t count = 0;
    walk(diff, len, end, [&](uint64_t index, uint8_t to) {
        if (index < base_offset) return;
        target[index - base_offset] = to;
        count++;
    });
    if (applied) *applied = count;
    return kOk;
}

}  // namespace diffstream
}  // namespace fwgpu
