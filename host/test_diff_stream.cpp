// The byte-diff stream's host codec (csrc/diff_stream.h) alone: the reference's known answers (weight_patcher/src/main.rs, its tests and
// the format) and the streams the reader must refuse.  A plain executable; nothing but the header is included.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "diff_stream.h"

using namespace fwgpu::diffstream;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

using Bytes = std::vector<uint8_t>;

static Bytes diff(const Bytes &a, const Bytes &b, uint64_t base = 0, uint64_t prev = 0, uint64_t *changed = nullptr) {
    const uint64_t need = encode(a.data(), b.data(), a.size(), base, prev, nullptr, 0, nullptr, nullptr);
    Bytes out(need);  // exactly: a write past the stream's size is the sanitizer's to find
    CHECK(encode(a.data(), b.data(), a.size(), base, prev, out.data(), out.size(), changed, nullptr) == need);
    return out;
}

static Bytes text(const char *s) { return Bytes(s, s + std::strlen(s)); }

// varint(v) as the stream encodes it: one differing byte at index v, prev 0
static Bytes varint_of(uint64_t v) {
    Bytes s = diff({1}, {2}, v, 0);
    CHECK(!s.empty() && s.back() == 2);
    s.pop_back();
    return s;
}

int main() {
    // known answers
    CHECK(varint_of(12345) == (Bytes{0xb9, 0x60}));
    CHECK(varint_of(16383) == (Bytes{0xff, 0x7f}));
    CHECK(varint_of(16384) == (Bytes{0x80, 0x80, 0x01}));
    CHECK(varint_of(2097151) == (Bytes{0xff, 0xff, 0x7f}));
    CHECK(varint_of(2097152) == (Bytes{0x80, 0x80, 0x80, 0x01}));
    CHECK(varint_of(UINT64_MAX).size() == 10);
    CHECK(diff(text("hello"), text("world")) == (Bytes{0x00, 0x77, 0x01, 0x6f, 0x01, 0x72, 0x02, 0x64}));
    CHECK(diff(text("hello world"), text("hello world")).empty());
    CHECK(diff({}, {}).empty());
    // the reference's varint round trip, through base_offset (the value is the first delta) and through prev_index (base - prev is)
    for (uint64_t v : {0ull, 1ull, 127ull, 128ull, 16383ull, 16384ull, 2097151ull, 2097152ull, (unsigned long long)UINT64_MAX}) {
        const Bytes s = varint_of(v);
        CHECK(s.size() == varint_len(v));
        uint64_t seen = 0, n = 0;
        Bytes entry = s;
        entry.push_back(7);
        CHECK(walk(entry.data(), entry.size(), UINT64_MAX, [&](uint64_t index, uint8_t to) { seen = index + (to == 7 ? 0 : 1); }, &n) ==
              (v == UINT64_MAX ? kBeyond : kOk));  // (index 2^64 - 1 is beyond every target)
        if (v != UINT64_MAX) CHECK(n == 1 && seen == v);
        if (v <= UINT64_MAX - 1000) {
            Bytes want = s;
            want.push_back(2);
            CHECK(diff({1}, {2}, v + 1000, 1000) == want);
        }
    }
    {  // prev_index: the delta is measured from it
        Bytes a(300, 0), b(300, 0);
        b[299] = 9;
        CHECK(diff(a, b, 1000, 1000 + 299 - 128) == (Bytes{0x80, 0x01, 9}));
        CHECK(diff(a, b, 1000, 0) == (Bytes{0x93, 0x0a, 9}));  // 1299 = 0x513
        uint64_t changed = 0;
        b[0] = 1;
        CHECK(diff(a, b, 0, 0, &changed) == (Bytes{0x00, 1, 0xab, 0x02, 9}) && changed == 2);  // delta 0 at index 0; 299 = 0x12b
    }
    // round trip
    {
        Bytes a(5000), b(5000);
        uint32_t x = 12345;
        for (size_t i = 0; i < a.size(); i++) {
            x = x * 1664525u + 1013904223u;
            a[i] = (uint8_t)(x >> 24);
            b[i] = (x >> 8) % 7 == 0 ? (uint8_t)(a[i] + 1 + (x >> 16) % 255) : a[i];
        }
        for (uint64_t base : {0ull, 77ull, (1ull << 32) - 100}) {
            const Bytes s = diff(a, b, base, 0);
            Bytes t = a;
            uint64_t applied = 0;
            CHECK(apply(t.data(), t.size(), base, s.data(), s.size(), &applied) == kOk);
            CHECK(t == b && applied > 500);
        }
        // entries below base_offset are skipped: the second half patched alone
        const Bytes s = diff(a, b);
        Bytes t(a.begin() + 2500, a.end());
        CHECK(apply(t.data(), t.size(), 2500, s.data(), s.size(), nullptr) == kOk);
        CHECK(t == Bytes(b.begin() + 2500, b.end()));
    }
    // bad streams: the status, and the target unchanged
    {
        const Bytes target = text("hello");
        struct Case {
            const char *name;
            Bytes stream;
            int status;
        } cases[] = {
            {"truncated varint", {0x01, 0x6f, 0x80}, kTruncated},
            {"missing `to` byte", {0x01, 0x6f, 0x02}, kTruncated},
            {"11-byte varint", {0x01, 0x6f, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x00, 0x64}, kVarint},
            {"varint beyond 64 bits", {0x01, 0x6f, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0x02, 0x64}, kVarint},
            {"index equal to n", {0x01, 0x6f, 0x04, 0x64}, kBeyond},
            {"index overflows", {0x01, 0x6f, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0x01, 0x64}, kBeyond},
            {"zero delta in a second entry", {0x01, 0x6f, 0x00, 0x64}, kZeroDelta},
        };
        for (const Case &c : cases) {
            Bytes t = target;
            uint64_t applied = 99;
            const int st = apply(t.data(), t.size(), 0, c.stream.data(), c.stream.size(), &applied);
            if (st != c.status || t != target || applied != 0) {
                std::printf("FAILED bad stream '%s': status %d (%s), want %d\n", c.name, st, status_text(st), c.status);
                failures++;
            }
        }
        Bytes t = target;  // ... while a first entry with delta 0 is the format's own
        const Bytes ok = {0x00, 0x77};
        CHECK(apply(t.data(), t.size(), 0, ok.data(), ok.size(), nullptr) == kOk && t == text("wello"));
    }
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("diff_stream: all checks passed\n");
    return 0;
}
