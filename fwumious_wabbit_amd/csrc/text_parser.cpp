// Host side of the device text route: VW text goes up in chunks cut at line breaks, textparse.hip turns the lines into the u32 records
// of parser.rs:57-74, and the lines the kernel does not take are parsed, in order, by the host parser (parser.cpp) -- so every result,
// stop and message is the host parser's.  Order of a chunk: status kernel -> {status, length} per line to the host -> host parser on
// the flagged lines, which fixes their lengths and finds the stop -> offsets -> write kernel -> host-parsed records copied in.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "f32_text.h"
#include "fwgpu_internal.h"
#include "parser_types.h"
#include "textparse.h"

namespace fwgpu {
namespace {

constexpr uint64_t kChunkBytes = 16u << 20;  // text per kernel pass (line positions are u32)
constexpr size_t kPinnedBytes = 4u << 20;    // staging piece; two of them alternate

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return FWGPU_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = bytes + bytes / 4 + 256;
        FWGPU_HIP(hipMalloc(&p, want));
        cap = want;
        return FWGPU_OK;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    template <class T>
    T *as() const { return static_cast<T *>(p); }
};

struct HostRecord {
    uint32_t line;
    uint64_t off;  // where it goes, in words from the call's first record
    std::vector<uint32_t> words;
};

struct TrainSet {  // what the launches of one piece read and write; reused when they have retired
    DevBuf records, rec_off, pred, work;
    std::vector<uint32_t> host_words;  // the host-parsed records of the piece, back to back (source of asynchronous copies: kept until the set's next piece)
    std::vector<uint4> host_status;    // ... and their status entries
};

struct LineMode {  // what the kernels get beyond the text: all zero for fwgpu_text_parser_parse_buffer
    TextTranslator tr{};
    TextCandidate cand{};
    uint32_t set_word1 = 0, word1 = 0;
};

struct TextChunk {  // one chunk of text on the device and what the host knows about its lines
    DevBuf text, cnt, rank, lstart, status, off, long_list;
    uint32_t len = 0, nlines = 0, n_used = 0;
    uint64_t first_word = 0;  // offset of the chunk's first record
    std::vector<uint4> h_status;
    std::vector<uint32_t> h_lstart;  // fetched only when a line needs the host or the call stops inside the chunk
    std::vector<uint64_t> h_off;
    std::vector<HostRecord> host_recs;
};

}  // namespace
}  // namespace fwgpu

using namespace fwgpu;

struct fwgpu_text_parser {
    fwgpu_parser *host = nullptr;  // takes the lines the kernel flags; owns the command argument
    int device = 0;
    hipStream_t stream = nullptr;
    void *ns_blob = nullptr;
    TextNsTable ns{};
    void *pinned[2] = {nullptr, nullptr};
    hipEvent_t pinned_free[2] = {nullptr, nullptr};
    uint32_t *long_count = nullptr;
    DevBuf scan_tmp, words;
    std::vector<std::unique_ptr<TextChunk>> chunks;
    std::vector<uint32_t> line_words;  // one host-parsed record
    uint64_t last_lines = 0, last_host_lines = 0;
    // candidate / counting calls: the translator and the cache's keys on the device (uploaded again only when they change), and the call's results
    LineMode mode{};
    DevBuf side;
    std::vector<unsigned char> side_host;
    std::vector<uint64_t> li_off;
    std::vector<fwgpu_candidate_info> li_info;
    size_t li_chunks = 0;
    // training from text (text_train_*): two sets of launch buffers that alternate piece by piece, the plan's scratch, what the host reads of a plan
    TrainSet train[2];
    DevBuf plan_tmp, plan_out, host_list;
    uint64_t *plan_host = nullptr;  // pinned: window statistics, then the host lines' offsets
    size_t plan_host_cap = 0;
    std::vector<uint32_t> h_host_list;
    fwgpu_translator_config train_t{};  // borrowed from text_train_begin's caller for the length of its call
    uint64_t wait_ns = 0;               // host time spent waiting for `stream` since the last call began
};

namespace fwgpu {
namespace {

struct RunResult {
    uint64_t n_records = 0, n_words = 0, consumed = 0;
    int rc = FWGPU_OK;
    size_t n_chunks = 0;
    std::vector<uint64_t> rec_off;  // filled when the caller gave none
};

// the host waits for the parser's stream; the time is kept for fwgpu_text_parser_last_wait_ns
int wait_stream(fwgpu_text_parser *tp) {
    const auto t0 = std::chrono::steady_clock::now();
    const hipError_t e = hipStreamSynchronize(tp->stream);
    tp->wait_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    if (e != hipSuccess) return fail(FWGPU_ERR_DEVICE, std::string("hipStreamSynchronize(parser stream): ") + hipGetErrorString(e));
    return FWGPU_OK;
}

int upload_text(fwgpu_text_parser *tp, TextChunk &ch, const char *text, uint32_t len) {
    int rc = ch.text.ensure((size_t)len + kTextPad + 16);
    if (rc) return rc;
    unsigned char *d = ch.text.as<unsigned char>();
    for (size_t at = 0, k = 0; at < len; at += kPinnedBytes, k ^= 1) {
        const size_t n = std::min<size_t>(kPinnedBytes, len - at);
        FWGPU_HIP(hipEventSynchronize(tp->pinned_free[k]));
        std::memcpy(tp->pinned[k], text + at, n);
        FWGPU_HIP(hipMemcpyAsync(d + at, tp->pinned[k], n, hipMemcpyHostToDevice, tp->stream));
        FWGPU_HIP(hipEventRecord(tp->pinned_free[k], tp->stream));
    }
    FWGPU_HIP(hipMemsetAsync(d + len, 0, kTextPad, tp->stream));
    ch.len = len;
    return FWGPU_OK;
}

// line index + status pass of a chunk already on the device; leaves h_status (fetch == false: the statuses stay on the device, nobody waits for the pass)
int chunk_status(fwgpu_text_parser *tp, TextChunk &ch, bool tail, bool fetch = true) {
    const uint32_t n16 = (ch.len + 15) / 16;
    int rc = ch.cnt.ensure(4 * ((size_t)n16 + 1));
    if (!rc) rc = ch.rank.ensure(4 * ((size_t)n16 + 1));
    const size_t tmp = text_scan_temp_bytes(n16);
    if (!rc) rc = tp->scan_tmp.ensure(std::max<size_t>(tmp, 256));
    if (rc) return rc;
    FWGPU_HIP(text_count_lines(ch.text.as<unsigned char>(), ch.len, ch.cnt.as<uint32_t>(), ch.rank.as<uint32_t>(), tp->scan_tmp.p, tmp, tp->stream));
    uint32_t newlines = 0;
    FWGPU_HIP(hipMemcpyAsync(&newlines, ch.rank.as<uint32_t>() + n16, 4, hipMemcpyDeviceToHost, tp->stream));
    if ((rc = wait_stream(tp))) return rc;
    ch.nlines = newlines + (tail ? 1u : 0u);
    ch.h_lstart.clear();
    ch.host_recs.clear();
    ch.n_used = 0;
    if (!(rc = ch.lstart.ensure(4 * ((size_t)ch.nlines + 2)))) rc = ch.status.ensure(16 * std::max<size_t>(ch.nlines, 1));
    if (!rc) rc = ch.off.ensure(8 * std::max<size_t>(ch.nlines, 1));
    if (!rc) rc = ch.long_list.ensure(4 * std::max<size_t>(ch.nlines, 1));
    if (rc) return rc;
    FWGPU_HIP(text_line_index(ch.text.as<unsigned char>(), ch.len, ch.rank.as<uint32_t>(), tail ? 1 : 0, ch.lstart.as<uint32_t>(), tp->stream));
    TextParseArgs a{};
    a.text = ch.text.as<unsigned char>();
    a.lstart = ch.lstart.as<uint32_t>();
    a.nlines = ch.nlines;
    a.ns = tp->ns;
    a.tr = tp->mode.tr;
    a.cand = tp->mode.cand;
    a.status = ch.status.as<uint4>();
    a.long_list = ch.long_list.as<uint32_t>();
    a.long_count = tp->long_count;
    FWGPU_HIP(text_parse_launch(a, false, tp->stream));
    if (!fetch) return FWGPU_OK;
    ch.h_status.resize(ch.nlines);
    if (ch.nlines) FWGPU_HIP(hipMemcpyAsync(ch.h_status.data(), ch.status.p, 16 * (size_t)ch.nlines, hipMemcpyDeviceToHost, tp->stream));
    FWGPU_HIP(hipStreamSynchronize(tp->stream));
    return FWGPU_OK;
}

int fetch_line_starts(fwgpu_text_parser *tp, TextChunk &ch) {
    if (!ch.h_lstart.empty()) return FWGPU_OK;
    ch.h_lstart.resize((size_t)ch.nlines + 1);
    FWGPU_HIP(hipMemcpyAsync(ch.h_lstart.data(), ch.lstart.p, 4 * ((size_t)ch.nlines + 1), hipMemcpyDeviceToHost, tp->stream));
    return wait_stream(tp);
}

// the host parser on one line, exactly as fwgpu_parser_parse_buffer meets it; the record is left in tp->line_words
int host_line(fwgpu_text_parser *tp, const char *line, uint64_t size) {
    tp->line_words.resize((size_t)size + tp->ns.num_namespaces + 16);  // a record has at most header + slots + one word per byte
    uint64_t off2[2], nr = 0, nw = 0, used = 0;
    int rc = fwgpu_parser_parse_buffer(tp->host, line, size, tp->line_words.data(), tp->line_words.size(), off2, 1, &nr, &nw, &used);
    if (rc != FWGPU_OK) return rc;
    if (nr != 1) return fail(FWGPU_ERR_RANGE, "text parser: a record larger than its line allows");
    tp->line_words.resize((size_t)nw);
    tp->last_host_lines++;
    return FWGPU_OK;
}

// write pass of a chunk: records of its DEVICE_OK lines [0, n_used) to dst + (h_off[line] - rebase)
int chunk_write(fwgpu_text_parser *tp, TextChunk &ch, uint32_t *dst, uint64_t rebase) {
    if (!ch.n_used) return FWGPU_OK;
    if (rebase)
        for (uint32_t i = 0; i < ch.n_used; i++) ch.h_off[i] -= rebase;
    FWGPU_HIP(hipMemcpyAsync(ch.off.p, ch.h_off.data(), 8 * (size_t)ch.n_used, hipMemcpyHostToDevice, tp->stream));
    TextParseArgs a{};
    a.text = ch.text.as<unsigned char>();
    a.lstart = ch.lstart.as<uint32_t>();
    a.nlines = ch.nlines;
    a.ns = tp->ns;
    a.tr = tp->mode.tr;
    a.cand = tp->mode.cand;
    a.set_word1 = tp->mode.set_word1;
    a.word1 = tp->mode.word1;
    a.status = ch.status.as<uint4>();
    a.n_used = ch.n_used;
    a.dst_off = ch.off.as<uint64_t>();
    a.dst = dst;
    a.long_list = ch.long_list.as<uint32_t>();
    a.long_count = tp->long_count;
    FWGPU_HIP(text_parse_launch(a, true, tp->stream));
    return FWGPU_OK;
}

// The walk of fwgpu_parser_parse_buffer over `text`.  keep == false: the records land in `words` (host) chunk by chunk.
// keep == true: nothing is written yet; the chunks stay on the device (tp->chunks[0 .. n_chunks)) for the caller to place.
int run(fwgpu_text_parser *tp, const char *text, uint64_t len, uint32_t *words, uint64_t words_cap, uint64_t *rec_off, uint64_t max_records,
        bool keep, RunResult &R) {
    FWGPU_HIP(hipSetDevice(tp->device));
    tp->last_lines = tp->last_host_lines = 0;
    tp->mode = LineMode();
    uint64_t pos = 0, nr = 0, nw = 0;
    bool stop = false;
    auto set_off = [&](uint64_t i, uint64_t v) {
        if (rec_off) rec_off[i] = v;
        else R.rec_off.push_back(v);
    };
    set_off(0, 0);
    while (pos < len && nr < max_records && !stop) {
        uint64_t cut = std::min<uint64_t>(len - pos, kChunkBytes);
        if (pos + cut < len) {  // cut at the last line break of the window
            const void *nl = memrchr(text + pos, '\n', cut);
            if (!nl) {  // one line longer than a chunk: the host's
                const char *e = static_cast<const char *>(std::memchr(text + pos + cut, '\n', len - pos - cut));
                const uint64_t size = e ? (uint64_t)(e - (text + pos)) + 1 : len - pos;
                tp->last_lines++;
                const int rc = host_line(tp, text + pos, size);
                if (rc != FWGPU_OK) {
                    R.rc = rc;
                    break;
                }
                if (nw + tp->line_words.size() > words_cap) break;
                if (keep) {
                    if (R.n_chunks == tp->chunks.size()) tp->chunks.emplace_back(new TextChunk());
                    TextChunk &ch = *tp->chunks[R.n_chunks++];
                    ch.nlines = ch.n_used = ch.len = 0;
                    ch.host_recs.clear();
                    ch.host_recs.push_back({0, nw, tp->line_words});
                } else {
                    std::memcpy(words + nw, tp->line_words.data(), tp->line_words.size() * 4);
                }
                nw += tp->line_words.size();
                set_off(++nr, nw);
                pos += size;
                continue;
            }
            cut = (uint64_t)(static_cast<const char *>(nl) - (text + pos)) + 1;
        }
        const size_t ci = keep ? R.n_chunks : 0;
        if (ci == tp->chunks.size()) tp->chunks.emplace_back(new TextChunk());
        TextChunk &ch = *tp->chunks[ci];
        if (keep) R.n_chunks++;
        int rc = upload_text(tp, ch, text + pos, (uint32_t)cut);
        if (!rc) rc = chunk_status(tp, ch, text[pos + cut - 1] != '\n');
        if (rc) return rc;
        ch.first_word = nw;
        ch.h_off.resize(ch.nlines);
        uint32_t i = 0;
        for (; i < ch.nlines; i++) {
            if (nr == max_records) break;
            uint64_t reclen = ch.h_status[i].y;
            tp->last_lines++;
            if ((ch.h_status[i].x & 0xffu) != kTextDeviceOk) {
                if ((rc = fetch_line_starts(tp, ch))) return rc;
                rc = host_line(tp, text + pos + ch.h_lstart[i], ch.h_lstart[i + 1] - ch.h_lstart[i]);
                if (rc != FWGPU_OK) {
                    R.rc = rc;  // a command, or an error with the host parser's message
                    stop = true;
                    break;
                }
                reclen = tp->line_words.size();
                if (nw + reclen > words_cap) {
                    tp->last_lines--;
                    tp->last_host_lines--;
                    break;
                }
                ch.host_recs.push_back({i, nw, tp->line_words});
            } else if (nw + reclen > words_cap) {
                tp->last_lines--;
                break;
            }
            ch.h_off[i] = nw;
            nw += reclen;
            set_off(++nr, nw);
        }
        ch.n_used = i;
        if (i < ch.nlines) {  // stopped inside the chunk
            stop = true;
            if ((rc = fetch_line_starts(tp, ch))) return rc;
            pos += ch.h_lstart[i];
        } else {
            pos += cut;
        }
        if (!keep && nw > ch.first_word) {
            const uint64_t nwc = nw - ch.first_word;
            if ((rc = tp->words.ensure(4 * (size_t)nwc))) return rc;
            if ((rc = chunk_write(tp, ch, tp->words.as<uint32_t>(), ch.first_word))) return rc;
            FWGPU_HIP(hipMemcpyAsync(words + ch.first_word, tp->words.p, 4 * (size_t)nwc, hipMemcpyDeviceToHost, tp->stream));
            FWGPU_HIP(hipStreamSynchronize(tp->stream));
            for (const HostRecord &h : ch.host_recs) std::memcpy(words + h.off, h.words.data(), h.words.size() * 4);
        }
    }
    R.n_records = nr;
    R.n_words = nw;
    R.consumed = pos;
    return FWGPU_OK;
}


// ---- every line of a text: a request's candidates, or whole lines, with the per-line facts serving needs

// the translator's CSR arrays and the cache's keys, as the kernels read them; kept on the device between calls that bring the same ones
int upload_side(fwgpu_text_parser *tp, const fwgpu_translator_config *t, const fwgpu_block_cache *cache) {
    const uint32_t nns = tp->ns.num_namespaces;
    const uint32_t ncm = t->n_combos ? t->combo_off[t->n_combos] : 0;
    const uint32_t npr = (t->ffm_k && t->n_fields) ? t->field_off[t->n_fields] : 0;
    for (uint32_t m = 0; m < ncm; m++)
        if (t->combo_ns[m] >= nns) return fail(FWGPU_ERR_INVALID, "translator: a combo names a namespace the map does not have");
    for (uint32_t m = 0; m < npr; m++)
        if (t->field_ns[m] >= nns) return fail(FWGPU_ERR_INVALID, "translator: a field names a namespace the map does not have");
    const size_t np = cache ? cache->present.size() : 0;
    auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
    size_t q = 0;
    const size_t q_coff = q; q = up(q + 4 * ((size_t)t->n_combos + 1));
    const size_t q_cns = q; q = up(q + 4 * (size_t)ncm);
    const size_t q_pns = q; q = up(q + 4 * (size_t)npr);
    const size_t q_pfk = q; q = up(q + 4 * (size_t)npr);
    const size_t q_pres = q; q = up(q + 8 * np);
    std::vector<unsigned char> blob(std::max<size_t>(q, 16), 0);
    if (t->n_combos) std::memcpy(blob.data() + q_coff, t->combo_off, 4 * ((size_t)t->n_combos + 1));
    if (ncm) std::memcpy(blob.data() + q_cns, t->combo_ns, 4 * (size_t)ncm);
    if (npr) {
        std::memcpy(blob.data() + q_pns, t->field_ns, 4 * (size_t)npr);
        uint32_t *fk = reinterpret_cast<uint32_t *>(blob.data() + q_pfk);
        for (uint32_t f = 0; f < t->n_fields; f++)
            for (uint32_t m = t->field_off[f]; m < t->field_off[f + 1]; m++) fk[m] = f * t->ffm_k;
    }
    if (np) std::memcpy(blob.data() + q_pres, cache->present.data(), 8 * np);
    if (blob != tp->side_host || !tp->side.p) {
        int rc = tp->side.ensure(blob.size());
        if (rc) return rc;
        FWGPU_HIP(hipMemcpy(tp->side.p, blob.data(), blob.size(), hipMemcpyHostToDevice));  // (no pass of an earlier call is in flight)
        tp->side_host = blob;
    }
    const unsigned char *b = tp->side.as<unsigned char>();
    LineMode &lm = tp->mode;
    lm.tr.combo_off = reinterpret_cast<const uint32_t *>(b + q_coff);
    lm.tr.combo_ns = reinterpret_cast<const uint32_t *>(b + q_cns);
    lm.tr.pair_ns = reinterpret_cast<const uint32_t *>(b + q_pns);
    lm.tr.pair_fk = reinterpret_cast<const uint32_t *>(b + q_pfk);
    lm.tr.n_combos = t->n_combos;
    lm.tr.n_pairs = npr;
    lm.tr.add_const = t->add_constant_feature ? 1 : 0;
    lm.tr.ffm_mask = ffm_hash_mask(t->ffm_bit_precision, t->ffm_k);
    if (cache) {
        lm.cand.ctx_rec = cache->d_ctx_rec;
        lm.cand.ctx_len = (uint32_t)cache->ctx_rec.size();
        lm.cand.cover = cache->d_cover;
        lm.cand.n_cover_slots = (uint32_t)cache->ctx_slots.size();
        lm.cand.present = reinterpret_cast<const uint64_t *>(b + q_pres);
        lm.cand.n_present = (uint32_t)np;
    }
    return FWGPU_OK;
}

// one line by the host parser, with the host twins of the kernel's per-line facts; the record (none for an error) is left in tp->line_words
void host_fact_line(fwgpu_text_parser *tp, const fwgpu_parse_prefix *px, const fwgpu_block_cache *cache, const fwgpu_translator_config *t,
                    const char *line, uint64_t size, fwgpu_candidate_info *info) {
    const size_t ctx_len = cache ? cache->ctx_rec.size() : 0;
    tp->line_words.resize((size_t)size + ctx_len + tp->ns.num_namespaces + 16);  // header + slots + one word per byte, behind the context's words when merged
    uint32_t nw = 0;
    int is_delta = 0;
    const int rc = px ? fwgpu_parser_parse_candidate(tp->host, px, line, size, tp->line_words.data(), (uint32_t)tp->line_words.size(), &nw, &is_delta)
                      : fwgpu_parser_parse_line(tp->host, line, size, tp->line_words.data(), (uint32_t)tp->line_words.size(), &nw);
    *info = fwgpu_candidate_info{};
    info->code = rc;
    info->by_host = 1;
    tp->last_host_lines++;
    if (rc != FWGPU_OK) nw = 0;
    tp->line_words.resize(nw);
    if (!nw) return;
    info->is_delta = is_delta ? 1 : 0;
    uint32_t *rec = tp->line_words.data();
    if (tp->mode.set_word1) rec[1] = tp->mode.word1;
    uint32_t n_lr = 0, n_ffm = 0;
    const bool counted = count_record(t, rec, nw, is_delta ? cache->ctx_rec.data() : nullptr, is_delta ? (uint32_t)ctx_len : 0, &n_lr, &n_ffm) == FWGPU_OK;
    info->n_lr = counted ? n_lr : 0;
    info->n_ffm = counted ? n_ffm : 0;
    info->record_ok = counted && (!px || block_cache_record_ok(cache, t, rec, nw, is_delta != 0)) ? 1 : 0;
}

// Status passes over every line of `text`, piece by piece (pieces are cut at line breaks and stay on the device: tp->chunks[0 .. li_chunks)).
// px != NULL: the lines are candidates of the context `px` and `cache` hold.  Leaves tp->li_off (n_lines + 1 word offsets) and tp->li_info.
int scan_lines(fwgpu_text_parser *tp, const fwgpu_parse_prefix *px, const fwgpu_block_cache *cache, const fwgpu_translator_config *t, const char *text,
               uint64_t len, uint64_t piece_bytes) {
    tp->last_lines = tp->last_host_lines = 0;
    tp->li_off.assign(1, 0);
    tp->li_info.clear();
    tp->li_chunks = 0;
    piece_bytes = std::min<uint64_t>(std::max<uint64_t>(piece_bytes, 1), kChunkBytes);
    uint64_t pos = 0, nw = 0;
    auto next_chunk = [&]() -> TextChunk & {
        if (tp->li_chunks == tp->chunks.size()) tp->chunks.emplace_back(new TextChunk());
        TextChunk &ch = *tp->chunks[tp->li_chunks++];
        ch.nlines = ch.n_used = ch.len = 0;
        ch.host_recs.clear();
        ch.h_lstart.clear();
        return ch;
    };
    fwgpu_candidate_info info;
    auto host_line_at = [&](TextChunk &ch, uint32_t i, const char *line, uint64_t size) {
        host_fact_line(tp, px, cache, t, line, size, &info);
        if (!tp->line_words.empty()) ch.host_recs.push_back({i, nw, tp->line_words});
        return (uint64_t)tp->line_words.size();
    };
    while (pos < len) {
        uint64_t cut = std::min<uint64_t>(len - pos, piece_bytes);
        if (pos + cut < len) {
            const void *nl = memrchr(text + pos, '\n', cut);
            if (!nl) {  // one line longer than a piece: the host's
                const char *e = static_cast<const char *>(std::memchr(text + pos + cut, '\n', len - pos - cut));
                const uint64_t size = e ? (uint64_t)(e - (text + pos)) + 1 : len - pos;
                nw += host_line_at(next_chunk(), 0, text + pos, size);
                tp->li_info.push_back(info);
                tp->li_off.push_back(nw);
                tp->last_lines++;
                pos += size;
                continue;
            }
            cut = (uint64_t)(static_cast<const char *>(nl) - (text + pos)) + 1;
        }
        TextChunk &ch = next_chunk();
        int rc = upload_text(tp, ch, text + pos, (uint32_t)cut);
        if (!rc) rc = chunk_status(tp, ch, text[pos + cut - 1] != '\n');
        if (rc) return rc;
        ch.first_word = nw;
        ch.h_off.resize(ch.nlines);
        for (uint32_t i = 0; i < ch.nlines; i++) {
            const uint4 st = ch.h_status[i];
            ch.h_off[i] = nw;
            if ((st.x & 0xffu) == kTextDeviceOk) {
                info = fwgpu_candidate_info{};
                info.code = FWGPU_OK;
                info.is_delta = px ? 1 : 0;
                info.record_ok = (!px || (st.x & kTextRecordOk)) ? 1 : 0;
                info.n_lr = st.z;
                info.n_ffm = st.w;
                nw += st.y;
            } else {
                if ((rc = fetch_line_starts(tp, ch))) return rc;
                nw += host_line_at(ch, i, text + pos + ch.h_lstart[i], ch.h_lstart[i + 1] - ch.h_lstart[i]);
            }
            tp->li_info.push_back(info);
            tp->li_off.push_back(nw);
        }
        tp->last_lines += ch.nlines;
        ch.n_used = ch.nlines;
        pos += cut;
    }
    return FWGPU_OK;
}

}  // namespace

int text_lines_scan(fwgpu_text_parser *tp, const fwgpu_parse_prefix *px, const fwgpu_block_cache *cache, const fwgpu_translator_config *t, const char *text,
                    uint64_t len, uint64_t piece_bytes, bool zero_word1, TextLines *out) {
    if (!tp || !t || !out || (!text && len) || (px && !cache)) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (px) {
        if (!cache->d_cover) return fail(FWGPU_ERR_INVALID, "candidates from text: the cache does not know its context's record (fwgpu_block_cache_cover_record)");
        if (cache->owner->device != tp->device) return fail(FWGPU_ERR_INVALID, "candidates from text: parser and cache are on different devices");
        if (!fwgpu_parse_prefix_is_record(px, cache->ctx_rec.data(), (uint32_t)cache->ctx_rec.size()) ||
            cache->ctx_rec.size() < 3 + (size_t)tp->ns.num_namespaces)
            return fail(FWGPU_ERR_INVALID, "candidates from text: the prefix is not the record of the cache's context (fwgpu_parse_prefix_is_record)");
    }
    FWGPU_HIP(hipSetDevice(tp->device));
    tp->mode = LineMode();
    int rc = upload_side(tp, t, px ? cache : nullptr);
    if (rc) return rc;
    tp->mode.set_word1 = zero_word1 ? 1 : 0;
    rc = scan_lines(tp, px, cache, t, text ? text : "", len, piece_bytes ? piece_bytes : kChunkBytes);
    if (rc) return rc;
    out->info = tp->li_info.data();
    out->rec_off = tp->li_off.data();
    out->n_lines = tp->li_info.size();
    out->n_words = tp->li_off.back();
    return FWGPU_OK;
}

int text_lines_place(fwgpu_text_parser *tp, uint32_t *d_records) {
    FWGPU_HIP(hipSetDevice(tp->device));
    for (size_t c = 0; c < tp->li_chunks; c++) {
        TextChunk &ch = *tp->chunks[c];
        int rc = chunk_write(tp, ch, d_records, 0);
        if (rc) return rc;
        for (const HostRecord &h : ch.host_recs)
            FWGPU_HIP(hipMemcpyAsync(d_records + h.off, h.words.data(), h.words.size() * 4, hipMemcpyHostToDevice, tp->stream));
    }
    FWGPU_HIP(hipStreamSynchronize(tp->stream));
    return FWGPU_OK;
}

// ---- training from text (trainer.cpp fwgpu_trainer_digest_text_device): a piece of text -> records, offsets and launch statistics in one of the
// parser's two sets of device buffers.  Status pass, then the host parses exactly the lines the kernel listed as NEEDS_HOST and writes their
// {HOST_DONE, length, LR entries, FFM entries} into the status array, then text_batch_plan places every record and sums every launch window, then
// the write pass and the copies of the host's records.  The host reads a line count, the number of host lines and a few words per window.
int text_train_begin(fwgpu_text_parser *tp, const fwgpu_translator_config *t, int device) {
    if (!tp || !t) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (tp->device != device) return fail(FWGPU_ERR_INVALID, "training from text: parser and regressor are on different devices");
    FWGPU_HIP(hipSetDevice(tp->device));
    tp->last_lines = tp->last_host_lines = 0;
    tp->wait_ns = 0;
    tp->mode = LineMode();
    tp->train_t = *t;
    return upload_side(tp, t, nullptr);
}

hipStream_t text_train_stream(fwgpu_text_parser *tp) { return tp->stream; }
int text_train_wait(fwgpu_text_parser *tp) { return wait_stream(tp); }

int text_train_piece(fwgpu_text_parser *tp, const char *text, uint64_t len, int set, uint32_t micro_batch, uint32_t learn_before, TextTrainPiece *out) {
    *out = TextTrainPiece();
    if (len == 0) return FWGPU_OK;
    if (tp->chunks.empty()) tp->chunks.emplace_back(new TextChunk());
    TextChunk &ch = *tp->chunks[0];
    TrainSet &S = tp->train[set];
    S.host_words.clear();
    S.host_status.clear();
    const bool device_scan = len <= kChunkBytes;  // (the caller cuts at line breaks: anything longer is ONE line, the host's)
    int rc = FWGPU_OK;
    uint32_t n_host = 0;
    uint32_t *d_count = tp->long_count + 4;
    if (device_scan) {
        if ((rc = upload_text(tp, ch, text, (uint32_t)len))) return rc;
        if ((rc = chunk_status(tp, ch, text[len - 1] != '\n', /*fetch=*/false))) return rc;
        const size_t tmp = text_plan_temp_bytes(ch.nlines);
        if ((rc = tp->plan_tmp.ensure(tmp))) return rc;
        if ((rc = tp->host_list.ensure(4 * std::max<size_t>(ch.nlines, 1)))) return rc;
        FWGPU_HIP(text_host_lines(ch.status.as<uint4>(), ch.nlines, tp->host_list.as<uint32_t>(), d_count, tp->plan_tmp.p, tmp, tp->stream));
        FWGPU_HIP(hipMemcpyAsync(&n_host, d_count, 4, hipMemcpyDeviceToHost, tp->stream));
        if ((rc = wait_stream(tp))) return rc;
        if (n_host > ch.nlines) return fail(FWGPU_ERR_DEVICE, "training from text: more host lines than lines");
        tp->h_host_list.resize(n_host);
        if (n_host) {
            FWGPU_HIP(hipMemcpyAsync(tp->h_host_list.data(), tp->host_list.p, 4 * (size_t)n_host, hipMemcpyDeviceToHost, tp->stream));
            if ((rc = fetch_line_starts(tp, ch))) return rc;  // (waits for the list too)
        }
    } else {
        ch.len = 0;
        ch.nlines = n_host = 1;
        ch.n_used = 0;
        ch.host_recs.clear();
        ch.h_lstart.assign({0u, 0u});
        if ((rc = ch.status.ensure(16))) return rc;
        if ((rc = tp->host_list.ensure(4))) return rc;
        if ((rc = tp->plan_tmp.ensure(text_plan_temp_bytes(1)))) return rc;
        FWGPU_HIP(hipMemsetAsync(tp->host_list.p, 0, 4, tp->stream));
        tp->h_host_list.assign(1, 0u);
    }
    const uint32_t nlines = ch.nlines;
    uint32_t n_take = nlines;
    // ---- the host's lines, in order; the first that is no example ends the take
    struct Placed { uint32_t line; uint64_t at, n; };  // in S.host_words
    std::vector<Placed> placed;
    for (uint32_t j = 0; j < n_host; j++) {
        const uint32_t i = tp->h_host_list[j];
        const char *line = device_scan ? text + ch.h_lstart[i] : text;
        const uint64_t size = device_scan ? ch.h_lstart[i + 1] - ch.h_lstart[i] : len;
        rc = host_line(tp, line, size);
        if (rc != FWGPU_OK) {
            out->stop = rc;
            out->stop_msg = fwgpu_last_error();
            n_take = i;
            n_host = j;
            break;
        }
        uint32_t n_lr = 0, n_ffm = 0;
        if ((rc = count_record(&tp->train_t, tp->line_words.data(), (uint32_t)tp->line_words.size(), &n_lr, &n_ffm))) return rc;
        placed.push_back({i, S.host_words.size(), tp->line_words.size()});
        S.host_words.insert(S.host_words.end(), tp->line_words.begin(), tp->line_words.end());
        S.host_status.push_back(make_uint4(kTextHostDone, (uint32_t)tp->line_words.size(), n_lr, n_ffm));
    }
    for (uint32_t j = 0; j < n_host; j++)
        FWGPU_HIP(hipMemcpyAsync(ch.status.as<uint4>() + placed[j].line, &S.host_status[j], 16, hipMemcpyHostToDevice, tp->stream));
    tp->last_lines += n_take + (out->stop != FWGPU_OK ? 1 : 0);
    out->n_lines = nlines;
    out->n_take = n_take;
    out->consumed = n_take < nlines ? ch.h_lstart[n_take] : len;
    if (n_take == 0) return FWGPU_OK;
    // ---- the plan
    const TextPlanShape shape = text_plan_shape(n_take, micro_batch, learn_before);
    const size_t n_out = (size_t)kTextPlanStats * shape.n_windows + n_host;
    if ((rc = S.rec_off.ensure(8 * ((size_t)n_take + 1)))) return rc;
    if ((rc = tp->plan_out.ensure(8 * n_out))) return rc;
    if (tp->plan_host_cap < n_out) {
        if (tp->plan_host) (void)hipHostFree(tp->plan_host);
        tp->plan_host = nullptr;
        tp->plan_host_cap = 0;
        FWGPU_HIP(hipHostMalloc((void **)&tp->plan_host, 8 * (n_out * 2 + 64), hipHostMallocDefault));
        tp->plan_host_cap = n_out * 2 + 64;
    }
    uint64_t *d_stats = tp->plan_out.as<uint64_t>(), *d_host_off = d_stats + (size_t)kTextPlanStats * shape.n_windows;
    FWGPU_HIP(text_batch_plan(ch.status.as<uint4>(), n_take, micro_batch, learn_before, S.rec_off.as<uint64_t>(), d_stats, tp->host_list.as<uint32_t>(), n_host,
                              d_host_off, tp->plan_tmp.p, tp->plan_tmp.cap, tp->stream));
    FWGPU_HIP(hipMemcpyAsync(tp->plan_host, d_stats, 8 * n_out, hipMemcpyDeviceToHost, tp->stream));
    if ((rc = wait_stream(tp))) return rc;
    uint64_t n_words = 0;
    for (uint32_t w = 0; w < shape.n_windows; w++) n_words += tp->plan_host[(size_t)kTextPlanStats * w + 1];
    // ---- placement
    if ((rc = S.records.ensure(4 * std::max<uint64_t>(n_words, 1)))) return rc;
    if ((rc = S.pred.ensure(4 * (size_t)n_take))) return rc;
    if ((rc = S.work.ensure(4 * (size_t)kTextTrainWorkStride * shape.n_windows))) return rc;
    if (device_scan) {
        TextParseArgs a{};
        a.text = ch.text.as<unsigned char>();
        a.lstart = ch.lstart.as<uint32_t>();
        a.nlines = nlines;
        a.ns = tp->ns;
        a.tr = tp->mode.tr;
        a.status = ch.status.as<uint4>();
        a.n_used = n_take;
        a.dst_off = S.rec_off.as<uint64_t>();
        a.dst = S.records.as<uint32_t>();
        a.long_list = ch.long_list.as<uint32_t>();
        a.long_count = tp->long_count;
        FWGPU_HIP(text_parse_launch(a, true, tp->stream));
    }
    const uint64_t *host_off = tp->plan_host + (size_t)kTextPlanStats * shape.n_windows;
    for (uint32_t j = 0; j < n_host; j++) {
        if (host_off[j] + placed[j].n > n_words) return fail(FWGPU_ERR_DEVICE, "training from text: a host line's record lies outside the piece's records");
        FWGPU_HIP(hipMemcpyAsync(S.records.as<uint32_t>() + host_off[j], S.host_words.data() + placed[j].at, 4 * (size_t)placed[j].n, hipMemcpyHostToDevice, tp->stream));
    }
    out->n_learn = shape.n_learn;
    out->n_windows_learn = shape.n_windows_learn;
    out->n_windows = shape.n_windows;
    out->n_words = n_words;
    out->win_stats = tp->plan_host;
    out->d_records = S.records.as<uint32_t>();
    out->d_rec_off = S.rec_off.as<uint64_t>();
    out->d_pred = S.pred.as<float>();
    out->d_work = S.work.as<uint32_t>();
    return FWGPU_OK;
}

}  // namespace fwgpu

extern "C" {

// VowpalParser::new (parser.rs:78-105) for the device route: the vw map's name table, seeds, indices and formats go up once
int fwgpu_text_parser_create(const fwgpu_vwmap *vw, int device, fwgpu_text_parser **out) {
    if (!vw || !out) return fail(FWGPU_ERR_INVALID, "NULL argument");
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
        return fail(FWGPU_ERR_DEVICE, "fwgpu_text_parser_create: no such HIP device");
    std::unique_ptr<fwgpu_text_parser, void (*)(fwgpu_text_parser *)> tp(new fwgpu_text_parser(), fwgpu_text_parser_free);
    tp->device = device;
    int rc = fwgpu_parser_create(vw, &tp->host);
    if (rc) return rc;
    FWGPU_HIP(hipSetDevice(device));
    FWGPU_HIP(hipStreamCreateWithFlags(&tp->stream, hipStreamNonBlocking));
    for (int k = 0; k < 2; k++) {
        FWGPU_HIP(hipHostMalloc(&tp->pinned[k], kPinnedBytes, hipHostMallocDefault));
        FWGPU_HIP(hipEventCreateWithFlags(&tp->pinned_free[k], hipEventDisableTiming));
    }
    FWGPU_HIP(hipMalloc((void **)&tp->long_count, 64));
    const fwgpu_parser &hp = *tp->host;
    const size_t ne = hp.vw_copy.entries.size(), ns = hp.ns_table.size();
    std::vector<uint32_t> name_off(ne + 1, 0), seed(ne), index(ne);
    std::vector<uint8_t> f32(ne);
    std::string names;
    for (size_t i = 0; i < ne; i++) {
        names += hp.vw_copy.entries[i].vwname;
        name_off[i + 1] = (uint32_t)names.size();
        seed[i] = hp.seed[i];
        index[i] = hp.vw_copy.entries[i].index;
        f32[i] = hp.vw_copy.entries[i].f32;
    }
    auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
    size_t q = 0;
    const size_t q_slots = q; q = up(q + 4 * ns);
    const size_t q_off = q; q = up(q + 4 * (ne + 1));
    const size_t q_seed = q; q = up(q + 4 * ne);
    const size_t q_index = q; q = up(q + 4 * ne);
    const size_t q_f32 = q; q = up(q + ne);
    const size_t q_names = q; q = up(q + names.size());
    std::vector<unsigned char> blob(std::max<size_t>(q, 16), 0);
    std::memcpy(blob.data() + q_slots, hp.ns_table.data(), 4 * ns);
    std::memcpy(blob.data() + q_off, name_off.data(), 4 * (ne + 1));
    if (ne) {
        std::memcpy(blob.data() + q_seed, seed.data(), 4 * ne);
        std::memcpy(blob.data() + q_index, index.data(), 4 * ne);
        std::memcpy(blob.data() + q_f32, f32.data(), ne);
        std::memcpy(blob.data() + q_names, names.data(), names.size());
    }
    FWGPU_HIP(hipMalloc(&tp->ns_blob, blob.size()));
    FWGPU_HIP(hipMemcpy(tp->ns_blob, blob.data(), blob.size(), hipMemcpyHostToDevice));
    const unsigned char *b = static_cast<const unsigned char *>(tp->ns_blob);
    tp->ns.slots = reinterpret_cast<const int32_t *>(b + q_slots);
    tp->ns.name_off = reinterpret_cast<const uint32_t *>(b + q_off);
    tp->ns.seed = reinterpret_cast<const uint32_t *>(b + q_seed);
    tp->ns.index = reinterpret_cast<const uint32_t *>(b + q_index);
    tp->ns.f32 = b + q_f32;
    tp->ns.names = b + q_names;
    tp->ns.mask = hp.ns_mask;
    tp->ns.n_entries = (uint32_t)ne;
    tp->ns.num_namespaces = hp.vw_copy.num_namespaces;
    tp->ns.skip_prefix = hp.vw_copy.skip_prefix;
    *out = tp.release();
    return FWGPU_OK;
}

void fwgpu_text_parser_free(fwgpu_text_parser *tp) {
    if (!tp) return;
    (void)hipSetDevice(tp->device);
    if (tp->stream) (void)hipStreamSynchronize(tp->stream);
    tp->chunks.clear();
    for (int k = 0; k < 2; k++) {
        if (tp->pinned[k]) (void)hipHostFree(tp->pinned[k]);
        if (tp->pinned_free[k]) (void)hipEventDestroy(tp->pinned_free[k]);
    }
    if (tp->long_count) (void)hipFree(tp->long_count);
    if (tp->plan_host) (void)hipHostFree(tp->plan_host);
    if (tp->ns_blob) (void)hipFree(tp->ns_blob);
    if (tp->stream) (void)hipStreamDestroy(tp->stream);
    if (tp->host) fwgpu_parser_free(tp->host);
    delete tp;
}

// fwgpu_parser_parse_buffer (parser.rs:166-176 over many lines) with the scan of parser.rs:214-461 done by the device
int fwgpu_text_parser_parse_buffer(fwgpu_text_parser *tp, const char *text, uint64_t len, uint32_t *words, uint64_t words_cap, uint64_t *rec_off,
                                   uint64_t max_records, uint64_t *n_records, uint64_t *n_words, uint64_t *consumed) {
    if (!tp || !text || !words || !rec_off || !n_records || !n_words || !consumed) return fail(FWGPU_ERR_INVALID, "NULL argument");
    RunResult R;
    int rc = run(tp, text, len, words, words_cap, rec_off, max_records, false, R);
    if (rc) return rc;
    *n_records = R.n_records;
    *n_words = R.n_words;
    *consumed = R.consumed;
    return R.rc;
}

// Every line of `text` as a candidate of the context that `px` scanned and `cache` holds: fwgpu_parser_parse_candidate line by line, with the scan of
// the lines that start with '|' done by the device, and per line the entry counts and the cache's record rule (include/fwgpu.h).
int fwgpu_text_parser_parse_candidates(fwgpu_text_parser *tp, const fwgpu_parse_prefix *px, const fwgpu_block_cache *cache,
                                       const fwgpu_translator_config *t, const char *text, uint64_t len, uint64_t max_lines, uint32_t *words,
                                       uint64_t words_cap, uint64_t *rec_off, fwgpu_candidate_info *info, uint64_t *n_lines, uint64_t *n_words) {
    if (!tp || !px || !cache || !t || (!text && len) || (!words && words_cap) || !rec_off || (!info && max_lines) || !n_lines || !n_words)
        return fail(FWGPU_ERR_INVALID, "NULL argument");
    *n_lines = *n_words = 0;
    rec_off[0] = 0;
    TextLines tl;
    int rc = text_lines_scan(tp, px, cache, t, text, len, 0, false, &tl);
    if (rc) return rc;
    if (tl.n_lines > max_lines) return fail(FWGPU_ERR_RANGE, "parse_candidates: more lines than max_lines");
    if (tl.n_words > words_cap) return fail(FWGPU_ERR_RANGE, "parse_candidates: record buffer too small");
    if (tl.n_words) {
        if ((rc = tp->words.ensure(4 * (size_t)tl.n_words))) return rc;
        if ((rc = text_lines_place(tp, tp->words.as<uint32_t>()))) return rc;
        FWGPU_HIP(hipMemcpy(words, tp->words.p, 4 * (size_t)tl.n_words, hipMemcpyDeviceToHost));
    }
    std::memcpy(rec_off, tl.rec_off, 8 * ((size_t)tl.n_lines + 1));
    if (tl.n_lines) std::memcpy(info, tl.info, sizeof(fwgpu_candidate_info) * (size_t)tl.n_lines);
    *n_lines = tl.n_lines;
    *n_words = tl.n_words;
    return FWGPU_OK;
}

int fwgpu_text_parser_last_lines(const fwgpu_text_parser *tp, uint64_t *lines, uint64_t *host_lines) {
    if (!tp) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (lines) *lines = tp->last_lines;
    if (host_lines) *host_lines = tp->last_host_lines;
    return FWGPU_OK;
}

int fwgpu_text_parser_last_wait_ns(const fwgpu_text_parser *tp, uint64_t *ns) {
    if (!tp || !ns) return fail(FWGPU_ERR_INVALID, "NULL argument");
    *ns = tp->wait_ns;
    return FWGPU_OK;
}

// text_batch_plan (textparse.hip) on host arrays, for tests against a plain restatement
int fwgpu_debug_text_plan(const uint32_t *status4, uint32_t nlines, uint32_t n_take, uint32_t micro_batch, uint32_t learn_before_holdout, uint64_t *dst_off,
                          uint64_t *rec_off, uint32_t *n_windows, uint64_t *window_stats, uint32_t *host_lines, uint32_t *n_host_lines, void *stream_) {
    if ((nlines && !status4) || !rec_off || !n_windows || !n_host_lines || (nlines && !host_lines) || (n_take && !dst_off))
        return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (n_take > nlines || micro_batch == 0) return fail(FWGPU_ERR_INVALID, "text_plan: n_take > nlines or micro_batch == 0");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const TextPlanShape shape = text_plan_shape(n_take, micro_batch, learn_before_holdout);
    if (shape.n_windows && !window_stats) return fail(FWGPU_ERR_INVALID, "NULL argument");
    DevBuf d_status, d_off, d_stats, d_list, d_count, d_host_off, tmp;
    int rc = d_status.ensure(16 * std::max<size_t>(nlines, 1));
    if (!rc) rc = d_off.ensure(8 * ((size_t)n_take + 1));
    if (!rc) rc = d_stats.ensure(8 * kTextPlanStats * std::max<size_t>(shape.n_windows, 1));
    if (!rc) rc = d_list.ensure(4 * std::max<size_t>(nlines, 1));
    if (!rc) rc = d_host_off.ensure(8 * std::max<size_t>(nlines, 1));
    if (!rc) rc = d_count.ensure(4);
    if (!rc) rc = tmp.ensure(text_plan_temp_bytes(nlines));
    if (rc) return rc;
    if (nlines) FWGPU_HIP(hipMemcpyAsync(d_status.p, status4, 16 * (size_t)nlines, hipMemcpyHostToDevice, stream));
    FWGPU_HIP(text_host_lines(d_status.as<uint4>(), nlines, d_list.as<uint32_t>(), d_count.as<uint32_t>(), tmp.p, tmp.cap, stream));
    uint32_t n_host = 0;
    FWGPU_HIP(hipMemcpyAsync(&n_host, d_count.p, 4, hipMemcpyDeviceToHost, stream));
    FWGPU_HIP(hipStreamSynchronize(stream));
    if (n_host > nlines) return fail(FWGPU_ERR_DEVICE, "text_plan: more host lines than lines");
    FWGPU_HIP(text_batch_plan(d_status.as<uint4>(), n_take, micro_batch, learn_before_holdout, d_off.as<uint64_t>(), d_stats.as<uint64_t>(), d_list.as<uint32_t>(), n_host,
                              d_host_off.as<uint64_t>(), tmp.p, tmp.cap, stream));
    FWGPU_HIP(hipMemcpyAsync(rec_off, d_off.p, 8 * ((size_t)n_take + 1), hipMemcpyDeviceToHost, stream));
    if (shape.n_windows) FWGPU_HIP(hipMemcpyAsync(window_stats, d_stats.p, 8 * (size_t)kTextPlanStats * shape.n_windows, hipMemcpyDeviceToHost, stream));
    if (n_host) FWGPU_HIP(hipMemcpyAsync(host_lines, d_list.p, 4 * (size_t)n_host, hipMemcpyDeviceToHost, stream));
    FWGPU_HIP(hipStreamSynchronize(stream));
    if (n_take) std::memcpy(dst_off, rec_off, 8 * (size_t)n_take);
    *n_windows = shape.n_windows;
    *n_host_lines = n_host;
    return FWGPU_OK;
}

// the file name of the last hogwild_load line (parser.rs:149-164), as fwgpu_parser_command_argument
const char *fwgpu_text_parser_command_argument(const fwgpu_text_parser *tp) { return tp ? fwgpu_parser_command_argument(tp->host) : ""; }

// fwgpu_record_batch_create over the records of `text`, which never come to the host as input: the write kernel puts them into the batch.
// Stops as fwgpu_parser_parse_buffer stops; a line that is not an example ends the batch before it, and is reported (return code, message,
// command argument) by the call that finds it first, with no batch.
int fwgpu_record_batch_from_text(fwgpu_regressor *r, const fwgpu_translator_config *t, fwgpu_text_parser *tp, const char *text, uint64_t len,
                                 uint64_t max_records, fwgpu_batch **out, uint64_t *n_records, uint64_t *consumed) {
    if (!r || !t || !tp || !out || !n_records || !consumed || (!text && len)) return fail(FWGPU_ERR_INVALID, "NULL argument");
    *out = nullptr;
    *n_records = *consumed = 0;
    if (r->device != tp->device) return fail(FWGPU_ERR_INVALID, "fwgpu_record_batch_from_text: parser and regressor are on different devices");
    RunResult R;
    int rc = run(tp, text ? text : "", len, nullptr, ~0ull, nullptr, std::min<uint64_t>(max_records, 0xffffffffull), true, R);
    if (rc) return rc;
    if (R.rc != FWGPU_OK && R.n_records == 0) return R.rc;
    const uint32_t n = (uint32_t)R.n_records;
    fwgpu_batch *b = nullptr;
    rc = record_batch_alloc(r, t, std::max<uint32_t>(n, 1), std::max<uint64_t>(R.n_words, 1), &b);
    if (rc) return rc;
    std::vector<uint32_t> back((size_t)R.n_words);
    auto place = [&]() -> int {
        for (size_t c = 0; c < R.n_chunks; c++) {
            TextChunk &ch = *tp->chunks[c];
            int rc2 = chunk_write(tp, ch, b->records, 0);
            if (rc2) return rc2;
            for (const HostRecord &h : ch.host_recs)
                FWGPU_HIP(hipMemcpyAsync(b->records + h.off, h.words.data(), h.words.size() * 4, hipMemcpyHostToDevice, tp->stream));
        }
        FWGPU_HIP(hipMemcpyAsync(b->rec_off, R.rec_off.data(), 8 * ((size_t)n + 1), hipMemcpyHostToDevice, tp->stream));
        // RecordStats and the oversize host copy come from a read-back of the placed records through count_records
        if (!back.empty()) FWGPU_HIP(hipMemcpyAsync(back.data(), b->records, 4 * back.size(), hipMemcpyDeviceToHost, tp->stream));
        FWGPU_HIP(hipStreamSynchronize(tp->stream));
        return FWGPU_OK;
    };
    rc = place();
    RecordStats st;
    if (rc == FWGPU_OK) rc = count_records(t, back.data(), R.rec_off.data(), n, &st);
    if (rc == FWGPU_OK) {  // as record_batch_upload leaves a batch
        b->n = n;
        b->n_lr = st.tot_lr;
        b->n_ffm = st.tot_ffm;
        b->n_words = R.n_words;
        b->max_lr = r->cfg.wiring == FWGPU_WIRING_FFM_ONLY ? 0 : st.max_lr;
        b->max_ffm = st.max_ffm;
        b->max_rec = st.max_rec;
        b->aligned4 = true;
        rc = record_batch_host_copy_if_oversize(r, t, b, back.data(), R.rec_off.data(), n);
    }
    if (rc) {
        fwgpu_batch_free(b);
        return rc;
    }
    *out = b;
    *n_records = n;
    *consumed = R.consumed;
    return FWGPU_OK;
}

// the device's number conversion (f32_text.h), compiled for the host: FWGPU_ERR_PARSE when `s` is not in parse_f32_rust's grammar
int fwgpu_f32_from_text(const char *s, uint64_t len, float *out, int *proven) {
    if ((!s && len) || !out || !proven) return fail(FWGPU_ERR_INVALID, "NULL argument");
    const F32Text r = f32_from_text(reinterpret_cast<const unsigned char *>(s), (size_t)len);
    *proven = r.proven ? 1 : 0;
    std::memcpy(out, &r.bits, 4);
    if (!r.grammar) return fail(FWGPU_ERR_PARSE, "not an f32: " + std::string(s ? s : "", (size_t)len));
    return FWGPU_OK;
}

}  // extern "C"
