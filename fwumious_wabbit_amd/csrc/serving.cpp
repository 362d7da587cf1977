// The reference's serving FFI, same symbols and signatures (lib.rs:150-234): new_fw_predictor_prototype, clone_lite,
// fw_predict, fw_predict_with_cache, fw_setup_cache, free_predictor -- a binary that links libfw.so can link this library
// instead.  Each call parses the VW text, translates the record and runs the example kernel on the device.
//
// Context cache (lib.rs:88-148, block_ffm.rs:442-782, block_lr.rs:165-255): fw_setup_cache scans the context line once
// (fwgpu_parse_prefix: a request's scan resumes at the context's last token boundary instead of going over the context's text
// again, and gives the very record next_vowpal_with_cache builds from context + candidate, parser.rs:195-211), translates it
// and has the device compute its features' field sums once (fwgpu_setup_cache).  fw_predict_with_cache translates the request's
// record on the host and ships only the entries that are not in the cache.  fwgpu_predictor_predict_batch sends all candidates
// of a request in one launch, as records: the kernel's own translation leaves out the namespaces the cache covers
// (fwgpu_block_cache_cover_record); a request in which some candidate names a context namespace again, or carries a feature
// equal to a cached one, takes the entry route (host translation + fwgpu_block_cache_filter), which is the reference's rule
// for those.  Models with a deep head are served through the cache like any other (block_neural.rs:355, block_misc.rs:847, block_relu.rs:123: every block
// behind the FFM block inherits forward_with_cache): the cache also keeps how many features it holds per field, which is what the head's input diagonal
// needs (kernels.hip nn_forward), a request of 256 candidates or more takes the batched head route (launch.cpp run_batch_head_predict), a smaller one
// the per-example kernel.  Predictors created with --packed_weights keep the uncached route (whole line scored), which gives the same result --
// unless the command also holds --packed_context_cache: the model's regressor then gets fwgpu_packed_enable_caches, fw_setup_cache builds the
// device cache from the packed table (no record cover: every cached call takes the ENTRY route), and fw_predict_with_cache,
// fwgpu_predictor_predict_batch(with_cache) and fwgpu_predictor_predict_requests score the filtered candidate against it on the requests kernels.
// fwgpu_predictor_apply_diff makes every such cache stale (the regressor's weights epoch); a predictor rebuilds its cache from the context's entries
// it keeps before its next cached call, under the model's mutex.
//
// fwgpu_predictor_predict_text takes a request as one text, a candidate per line, and keeps the host out of the scan: the device parser
// (textparse.hip, candidate mode) turns every line that starts with '|' into the candidate-only record fwgpu_parser_parse_candidate defines,
// counts its entries and decides the cache's record rule; its write pass puts the records straight into the shared record batch, and the one
// launch fwgpu_predictor_predict_batch makes follows.  Lines the kernel does not take are parsed here and copied in.  A request in which some
// line's record breaks the record rule or cannot be split off the context, a predictor without a device cache (packed weights, FFM-less models,
// no fw_setup_cache yet) or with a context that is not its own record, and FWGPU_SERVING_HOST_PARSE=1 take fwgpu_predictor_predict_batch on
// the split lines instead (fwgpu_predictor_last_text_route: fell_back).  FWGPU_SERVING_TEXT_PIECE=<bytes>: text per parser pass.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "fw_ffi.h"
#include "fwgpu_internal.h"

using namespace fwgpu;

namespace {

struct SharedModel {  // what clone_lite shares: the immutable regressor and the descriptions it was built from
    fwgpu_regressor *re = nullptr;
    fwgpu_vwmap *vw = nullptr;
    fwgpu_model_instance *mi = nullptr;
    fwgpu_translator_config tr{};
    std::mutex mu;  // the regressor's single-example staging buffers are shared
    fwgpu_batch *batch = nullptr;  // device buffers of fwgpu_predictor_predict_batch, grown on demand and reused
    fwgpu_batch *one = nullptr;    // single requests: a host-mapped batch (no copy calls, no memset: launch + one synchronisation)
    fwgpu_text_parser *tp = nullptr;  // fwgpu_predictor_predict_text: the device parser, made by the first call, used under mu
    fwgpu_batch *requests = nullptr;  // fwgpu_predictor_predict_requests: its entry batch, grown on demand and reused (n_cap examples)
    ~SharedModel() {
        if (tp) fwgpu_text_parser_free(tp);
        if (requests) fwgpu_batch_free(requests);
        if (batch) fwgpu_batch_free(batch);
        if (one) fwgpu_batch_free(one);
        if (re) fwgpu_free(re);
        if (vw) fwgpu_vwmap_free(vw);
        if (mi) fwgpu_mi_free(mi);
    }
};

// shellwords::split (lib.rs:161): whitespace separated words, '...' and "..." quoting, backslash escapes
std::vector<std::string> shell_split(const char *s) {
    std::vector<std::string> out;
    std::string cur;
    bool in_word = false;
    char quote = 0;
    for (const char *p = s; *p; ++p) {
        const char c = *p;
        if (quote) {
            if (c == quote) quote = 0;
            else if (c == '\\' && quote == '"' && p[1]) cur += *++p;
            else cur += c;
        } else if (c == '\'' || c == '"') {
            quote = c;
            in_word = true;
        } else if (c == '\\' && p[1]) {
            cur += *++p;
            in_word = true;
        } else if (c == ' ' || c == '\t' || c == '\n') {
            if (in_word) out.push_back(cur);
            cur.clear();
            in_word = false;
        } else {
            cur += c;
            in_word = true;
        }
    }
    if (in_word) out.push_back(cur);
    return out;
}

}  // namespace

// one parser thread's share of a batched request (kept between requests: no fresh pages to fault in, no parser to build)
struct Part {
    std::vector<uint32_t> words;
    std::vector<uint64_t> len;
    std::vector<uint32_t> slot;
    // entry route: translated on the host, filtered (forward_with_cache gathers only what features_present lacks)
    HostBatch hb;
    bool hb_ok = true;
    RecordStats stats;  // record route: what record_batch_upload would otherwise count again, serially
    bool stats_ok = true;
    bool entry_route = false;  // some candidate of this slice is not covered record-wise (fwgpu_block_cache_record_ok)
    fwgpu_parser *parser = nullptr;  // VowpalParser is not thread safe (clone_lite's reason): one per thread
    std::vector<uint32_t> rec;
    void reset() {
        words.clear();
        len.clear();
        slot.clear();
        hb.clear();
        hb_ok = stats_ok = true;
        entry_route = false;
        stats = RecordStats();
    }
    ~Part() {
        if (parser) fwgpu_parser_free(parser);
    }
};

struct FfiPredictor {
    std::shared_ptr<SharedModel> model;
    std::vector<std::unique_ptr<Part>> parts;
    Workers workers;  // the parser threads of batched requests, kept between requests: starting 31 threads costs more than scanning a 20 000-candidate request on them takes
    fwgpu_parser *parser = nullptr;
    std::string cached_text;  // PredictorCache.input_buffer_size bytes of the context line (lib.rs:64-67)
    fwgpu_parse_prefix *prefix = nullptr;  // the same bytes, scanned
    bool has_cache = false;
    bool delta_ok = false;  // the scanned context is the context's own record: requests can travel as candidate-only records
    fwgpu_block_cache *cache = nullptr;  // PredictorCache.blocks: the context's field sums, on the device
    std::vector<uint32_t> record;
    std::vector<fwgpu_lr_entry> lr;
    std::vector<fwgpu_ffm_entry> ffm;
    std::vector<fwgpu_lr_entry> ctx_lr;    // --packed_context_cache: the context's entries as fw_setup_cache translated them: what a stale cache
    std::vector<fwgpu_ffm_entry> ctx_ffm;  // is rebuilt from (lr / ffm above are scratch of every request)
    uint64_t text_lines = 0, text_host_lines = 0;  // fwgpu_predictor_last_text_route
    int text_fell_back = 0;
    ~FfiPredictor() {
        if (prefix) fwgpu_parse_prefix_free(prefix);
        if (parser) fwgpu_parser_free(parser);
        if (cache) fwgpu_block_cache_free(cache);
    }
};

namespace {

constexpr float kEofErrorCode = -1.0f, kExceptionErrorCode = -1.0f;  // lib.rs:47-48

// --packed_context_cache, under the model's mutex: a cache set up before the last hot patch (fwgpu_predictor_apply_diff) is rebuilt from the
// context's entries, so that no cached call is served from -- or refused for -- sums of weights that no longer exist
int refresh_stale_cache(FfiPredictor *p) {
    SharedModel &m = *p->model;
    if (!p->cache || !m.re->packed() || p->cache->epoch == m.re->weights_epoch) return FWGPU_OK;
    return fwgpu_setup_cache(m.re, p->ctx_lr.data(), (uint32_t)p->ctx_lr.size(), p->ctx_ffm.data(), (uint32_t)p->ctx_ffm.size(), &p->cache);
}

// parse -> translate -> predict (lib.rs:70-86).  The record goes to the device as it is (one small copy) and is translated
// in the example kernel's stage phase, like every other record batch; fwgpu_predictor_predict_batch is the same path with n > 1.
float predict_line(FfiPredictor *p, const char *prefix, size_t prefix_len, const char *text, size_t len) {
    uint32_t n_words = 0;
    p->record.resize(std::max<size_t>(p->record.size(), 4096));
    int rc;
    for (;;) {
        rc = prefix && p->prefix
                 ? fwgpu_parser_parse_after_prefix(p->parser, p->prefix, text, len, p->record.data(), (uint32_t)p->record.size(), &n_words)
                 : fwgpu_parser_parse_with_prefix(p->parser, prefix, prefix_len, text, len, p->record.data(), (uint32_t)p->record.size(), &n_words);
        if (rc == FWGPU_ERR_RANGE && p->record.size() < (1u << 24)) {
            p->record.resize(p->record.size() * 4);
            continue;
        }
        break;
    }
    if (rc != FWGPU_OK) return kExceptionErrorCode;  // parse errors and commands alike ("Reading result ... returns error")
    if (n_words == 0) return kEofErrorCode;
    p->record[1] = 0;  // no label in a request (NO_LABEL = 0xff); the prediction does not depend on it
    SharedModel &m = *p->model;
    std::lock_guard<std::mutex> g(m.mu);
    if (prefix && p->cache) {  // predict_with_cache (lib.rs:88-108): translate, then only the uncached features are gathered
        float label, imp, out = 0.0f;
        if (translate_record(&m.tr, p->record.data(), n_words, p->lr, p->ffm, &label, &imp) != FWGPU_OK) return kExceptionErrorCode;
        if (refresh_stale_cache(p) != FWGPU_OK) return kExceptionErrorCode;
        if (fwgpu_predict_with_cache(m.re, p->cache, p->lr.data(), (uint32_t)p->lr.size(), p->ffm.data(), (uint32_t)p->ffm.size(), &out) != FWGPU_OK)
            return kExceptionErrorCode;
        return out;
    }
    // The request goes into host memory the device has mapped; the kernel reads it over PCIe in its stage phase and writes the
    // prediction back the same way.  Per call: one kernel launch and one synchronisation (before: two copies in, a memset, the
    // launch, a copy out and the synchronisation).
    if (!m.one || m.one->words_cap < n_words) {
        if (m.one) fwgpu_batch_free(m.one);
        m.one = nullptr;
        if (record_batch_alloc(m.re, &m.tr, 1, std::max<uint64_t>(2 * (uint64_t)n_words, 1 << 14), &m.one, /*host_mapped=*/true) != FWGPU_OK)
            return kExceptionErrorCode;
    }
    fwgpu_batch *b = m.one;
    uint32_t c_lr = 0, c_ffm = 0;
    if (count_record(&m.tr, p->record.data(), n_words, &c_lr, &c_ffm) != FWGPU_OK) return kExceptionErrorCode;  // validates the record
    std::memcpy(b->h_records, p->record.data(), (size_t)n_words * 4);
    b->h_rec_off[0] = 0;
    b->h_rec_off[1] = n_words;
    b->n = 1;
    b->n_lr = c_lr;
    b->n_ffm = c_ffm;
    b->n_words = n_words;
    b->max_lr = m.re->cfg.wiring == FWGPU_WIRING_FFM_ONLY ? 0 : c_lr;
    b->max_ffm = c_ffm;
    b->max_rec = n_words;
    b->aligned4 = true;
    b->h_pred[0] = kExceptionErrorCode;  // (a launch that processed nothing must not return the previous request's answer)
    if (fwgpu_learn_batch(m.re, b, FWGPU_MODE_SEQUENTIAL, /*update=*/0, nullptr) != FWGPU_OK) return kExceptionErrorCode;
    if (hipStreamSynchronize(nullptr) != hipSuccess) return kExceptionErrorCode;
    return b->h_pred[0];
}

}  // namespace

extern "C" {

FfiPredictor *new_fw_predictor_prototype(const char *command) {  // lib.rs:150-185
    if (!command) {
        set_error("new_fw_predictor_prototype: NULL command");
        return nullptr;
    }
    const std::vector<std::string> words = shell_split(command);
    std::string weights;
    int device = 0;
    for (size_t i = 0; i + 1 < words.size(); i++) {
        if (words[i] == "-i" || words[i] == "--initial_regressor") weights = words[i + 1];
        if (words[i] == "--device") device = std::atoi(words[i + 1].c_str());  // ours: which GPU serves
    }
    bool packed = false, packed_caches = false;
    for (const auto &w : words) {
        if (w.rfind("--initial_regressor=", 0) == 0) weights = w.substr(std::strlen("--initial_regressor="));
        if (w == "--packed_weights") packed = true;  // ours: the FFM weights stay f16 buckets on the device (fwgpu_model_load_packed)
        if (w == "--packed_context_cache") packed_caches = true;  // ours: ... and context caches are built from them (fwgpu_packed_enable_caches)
    }
    if (packed_caches && !packed) {
        set_error("--packed_context_cache is valid only together with --packed_weights (an f32 predictor keeps its context cache without it)");
        return nullptr;
    }
    if (weights.empty()) {
        set_error("Cannot resolve input weights file name");  // the reference panics here (lib.rs:164-167)
        return nullptr;
    }
    auto model = std::make_shared<SharedModel>();
    if ((packed ? fwgpu_model_load_packed(weights.c_str(), device, &model->vw, &model->mi, &model->re)
                : fwgpu_model_load(weights.c_str(), device, /*immutable=*/1, &model->vw, &model->mi, &model->re)) != FWGPU_OK)
        return nullptr;
    if (packed_caches && fwgpu_packed_enable_caches(model->re) != FWGPU_OK) return nullptr;
    if (fwgpu_mi_configs(model->mi, device, nullptr, &model->tr, nullptr) != FWGPU_OK) return nullptr;
    auto p = std::make_unique<FfiPredictor>();
    p->model = model;
    if (fwgpu_parser_create(model->vw, &p->parser) != FWGPU_OK) return nullptr;
    return p.release();
}

FfiPredictor *clone_lite(FfiPredictor *prototype) {  // lib.rs:187-205: cheap copy, one per thread, shared weights
    if (!prototype) return nullptr;
    auto p = std::make_unique<FfiPredictor>();
    p->model = prototype->model;
    if (fwgpu_parser_create(p->model->vw, &p->parser) != FWGPU_OK) return nullptr;
    return p.release();
}

float fw_predict(FfiPredictor *ptr, const char *input_buffer) {  // lib.rs:207-212
    if (!ptr || !input_buffer) return kExceptionErrorCode;
    return predict_line(ptr, nullptr, 0, input_buffer, std::strlen(input_buffer));
}

float fw_setup_cache(FfiPredictor *ptr, const char *input_buffer) {  // lib.rs:224-232, 110-147
    if (!ptr || !input_buffer) return kExceptionErrorCode;
    size_t len = std::strlen(input_buffer);
    // the context line must itself parse (next_vowpal_with_size), and an empty one is EOF
    uint32_t n_words = 0;
    const int rc = fwgpu_parser_parse_line(ptr->parser, input_buffer, len, nullptr, 0, &n_words);
    if (rc != FWGPU_OK) return kExceptionErrorCode;
    if (n_words == 0) return kEofErrorCode;
    ptr->record.resize(std::max<size_t>(ptr->record.size(), (size_t)n_words));
    if (fwgpu_parser_parse_line(ptr->parser, input_buffer, len, ptr->record.data(), (uint32_t)ptr->record.size(), &n_words) != FWGPU_OK)
        return kExceptionErrorCode;
    if (len && input_buffer[len - 1] == '\n') len -= 1;  // "ignore last newline byte" (parser.rs:184-193)
    ptr->cached_text.assign(input_buffer, len);
    ptr->has_cache = true;
    ptr->delta_ok = false;
    if (ptr->prefix) fwgpu_parse_prefix_free(ptr->prefix);
    ptr->prefix = nullptr;
    if (fwgpu_parse_prefix_create(ptr->parser, ptr->cached_text.data(), ptr->cached_text.size(), &ptr->prefix) != FWGPU_OK) return kExceptionErrorCode;
    SharedModel &m = *ptr->model;
    // (a packed regressor keeps no device-side context cache: the whole context + candidate record is scored -- unless --packed_context_cache)
    if (m.re->cfg.ffm_k != 0 && m.re->packed() && m.re->packed_caches) {
        // the cache from the packed table; no record cover (record batches with a cache are not served on packed weights): delta_ok stays false
        float label, imp;
        std::lock_guard<std::mutex> g(m.mu);
        if (translate_record(&m.tr, ptr->record.data(), n_words, ptr->ctx_lr, ptr->ctx_ffm, &label, &imp) != FWGPU_OK) return kExceptionErrorCode;
        if (fwgpu_setup_cache(m.re, ptr->ctx_lr.data(), (uint32_t)ptr->ctx_lr.size(), ptr->ctx_ffm.data(), (uint32_t)ptr->ctx_ffm.size(), &ptr->cache) != FWGPU_OK)
            return kExceptionErrorCode;
    } else if (m.re->cfg.ffm_k != 0 && !m.re->packed()) {
        // translate_and_filter(buffer, 0, Some(Primitive)) + Regressor::setup_cache (lib.rs:133-146); every namespace this
        // library accepts is primitive (transformed namespaces are refused when the model is loaded)
        float label, imp;
        std::lock_guard<std::mutex> g(m.mu);
        if (translate_record(&m.tr, ptr->record.data(), n_words, ptr->lr, ptr->ffm, &label, &imp) != FWGPU_OK) return kExceptionErrorCode;
        if (fwgpu_setup_cache(m.re, ptr->lr.data(), (uint32_t)ptr->lr.size(), ptr->ffm.data(), (uint32_t)ptr->ffm.size(), &ptr->cache) != FWGPU_OK)
            return kExceptionErrorCode;
        if (fwgpu_block_cache_cover_record(ptr->cache, &m.tr, ptr->record.data(), n_words) != FWGPU_OK) return kExceptionErrorCode;
        ptr->delta_ok = fwgpu_parse_prefix_is_record(ptr->prefix, ptr->record.data(), n_words) != 0;
    }
    return 0.0f;
}

float fw_predict_with_cache(FfiPredictor *ptr, const char *input_buffer) {  // lib.rs:214-222, 88-108
    if (!ptr || !input_buffer) return kExceptionErrorCode;
    return predict_line(ptr, ptr->cached_text.data(), ptr->cached_text.size(), input_buffer, std::strlen(input_buffer));
}

void free_predictor(FfiPredictor *ptr) { delete ptr; }  // lib.rs:234-236

// All candidates of a request in one launch.  inputs[i] is what fw_predict (with_cache == 0) or fw_predict_with_cache
// (with_cache != 0) would be given; out[i] what it would return (-1.0 for a line that does not parse).
int fwgpu_predictor_predict_batch(FfiPredictor *ptr, const char *const *inputs, uint32_t n, int with_cache, float *out) {
    if (!ptr || (!inputs && n) || (!out && n)) return fail(FWGPU_ERR_INVALID, "NULL argument");
    SharedModel &m = *ptr->model;
    // parse on a few host threads (each with its own parser: VowpalParser is not thread safe, clone_lite's reason)
    // (FWGPU_SERVING_THREADS overrides; by default one thread per 128 lines, up to the cores there are and at most 32)
    unsigned T = 1;
    if (n >= 256) {
        const char *env = std::getenv("FWGPU_SERVING_THREADS");
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        T = env && std::atoi(env) > 0 ? (unsigned)std::atoi(env) : std::min<unsigned>(std::min<unsigned>(32, hw), std::max<unsigned>(1, n / 128));
        T = std::min<unsigned>(T, 64);
    }
    const bool cached = with_cache && ptr->cache;  // candidates reduced to the entries the context cache does not cover
    // records + the kernel's own translation, unless a candidate turns out to need the entry route (FWGPU_SERVING_ENTRY_ROUTE=1 forces that one)
    // (--packed_context_cache: the entry route always -- a packed regressor's cache knows no record)
    bool by_record = cached && !m.re->packed() && !std::getenv("FWGPU_SERVING_ENTRY_ROUTE");
    // ... and of those records only what the candidate adds to the context's record, which the device already holds
    // (FWGPU_SERVING_MERGED_RECORDS=1: whole context + candidate records instead)
    const bool delta_wanted = ptr->delta_ok && !std::getenv("FWGPU_SERVING_MERGED_RECORDS");
    bool delta = false;
    const bool timing = std::getenv("FWGPU_SERVING_TIMING") != nullptr;
    const auto t_begin = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (timing)
            std::fprintf(stderr, "[predict_batch] %-10s %.3f ms since entry\n", what,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
    };
    while (ptr->parts.size() < T) ptr->parts.push_back(std::make_unique<Part>());
    std::vector<Part *> parts(T);
    for (unsigned k = 0; k < T; k++) parts[k] = ptr->parts[k].get();
    for (uint32_t i = 0; i < n; i++) out[i] = kExceptionErrorCode;  // a worker that cannot start leaves its slice marked
    auto work = [&](unsigned k) {
        Part &pt = *parts[k];
        pt.reset();
        if (!pt.parser && fwgpu_parser_create(m.vw, &pt.parser) != FWGPU_OK) return;
        fwgpu_parser *parser = pt.parser;
        std::vector<uint32_t> &rec = pt.rec;
        if (rec.size() < 4096) rec.resize(4096);
        std::vector<fwgpu_lr_entry> t_lr;
        std::vector<fwgpu_ffm_entry> t_ffm;
        const uint32_t a = (uint32_t)((uint64_t)n * k / T), e = (uint32_t)((uint64_t)n * (k + 1) / T);
        for (uint32_t i = a; i < e; i++) {
            out[i] = kExceptionErrorCode;
            if (!inputs[i]) continue;
            uint32_t nw = 0;
            int rc;
            int is_delta = 0;
            for (;;) {
                rc = delta ? fwgpu_parser_parse_candidate(parser, ptr->prefix, inputs[i], std::strlen(inputs[i]), rec.data(), (uint32_t)rec.size(), &nw, &is_delta)
                     : with_cache && ptr->prefix
                         ? fwgpu_parser_parse_after_prefix(parser, ptr->prefix, inputs[i], std::strlen(inputs[i]), rec.data(), (uint32_t)rec.size(), &nw)
                         : fwgpu_parser_parse_with_prefix(parser, with_cache ? ptr->cached_text.data() : nullptr,
                                                          with_cache ? ptr->cached_text.size() : 0, inputs[i], std::strlen(inputs[i]),
                                                          rec.data(), (uint32_t)rec.size(), &nw);
                if (rc == FWGPU_ERR_RANGE && rec.size() < (1u << 24)) {
                    rec.resize(rec.size() * 4);
                    continue;
                }
                break;
            }
            if (rc != FWGPU_OK || nw == 0) {
                if (rc == FWGPU_OK) out[i] = kEofErrorCode;
                continue;
            }
            rec[1] = 0;  // a request carries no label (NO_LABEL = 0xff); the prediction does not depend on it
            if (by_record && ((delta && !is_delta) || !block_cache_record_ok(ptr->cache, &m.tr, rec.data(), nw, delta))) {
                pt.entry_route = true;
                break;  // the whole request goes again, by entries
            }
            if (cached && !by_record) {
                float label, imp;
                if (translate_record(&m.tr, rec.data(), nw, t_lr, t_ffm, &label, &imp) != FWGPU_OK) continue;
                uint32_t kept = 0;
                if (fwgpu_block_cache_filter(ptr->cache, t_ffm.data(), (uint32_t)t_ffm.size(), t_ffm.data(), &kept) != FWGPU_OK) continue;
                if (append_example(m.re, pt.hb, t_lr.data(), (uint32_t)t_lr.size(), t_ffm.data(), kept, 0.0f, 1.0f) != FWGPU_OK) {
                    pt.hb_ok = false;
                    continue;
                }
                pt.slot.push_back(i);
                continue;
            }
            uint32_t c_lr = 0, c_ffm = 0;
            const uint32_t ctx_len = delta ? (uint32_t)ptr->cache->ctx_rec.size() : 0;
            if (count_record(&m.tr, rec.data(), nw, delta ? ptr->cache->ctx_rec.data() : nullptr, ctx_len, &c_lr, &c_ffm) != FWGPU_OK) {
                if (delta) {
                    pt.entry_route = true;
                    break;
                }
                pt.stats_ok = false;  // (the upload validates again and reports)
            } else {
                pt.stats.max_lr = std::max(pt.stats.max_lr, c_lr);
                pt.stats.max_ffm = std::max(pt.stats.max_ffm, c_ffm);
                pt.stats.max_rec = std::max(pt.stats.max_rec, nw + ctx_len);  // (LDS holds the context's record behind the candidate's)
                pt.stats.tot_lr += c_lr;
                pt.stats.tot_ffm += c_ffm;
            }
            pt.words.insert(pt.words.end(), rec.begin(), rec.begin() + nw);
            pt.len.push_back(nw);
            pt.slot.push_back(i);
        }
    };
    for (;;) {
        delta = by_record && delta_wanted;
        ptr->workers.run(T, work);
        bool again = false;
        for (const Part *pt : parts) again = again || pt->entry_route;
        if (!again) break;
        by_record = false;
    }
    lap("parsed");
    std::vector<uint64_t> off(1, 0);
    std::vector<uint32_t> slot;  // which input each record belongs to
    RecordStats stats;
    bool stats_ok = true;
    std::vector<size_t> wbase(parts.size() + 1, 0);
    for (size_t q = 0; q < parts.size(); q++) {
        const Part &pt = *parts[q];
        wbase[q + 1] = wbase[q] + pt.words.size();
        for (uint64_t l : pt.len) off.push_back(off.back() + l);
        slot.insert(slot.end(), pt.slot.begin(), pt.slot.end());
        stats.merge(pt.stats);
        stats_ok = stats_ok && pt.stats_ok;
    }
    const size_t total_words = wbase[parts.size()];
    lap("merged");
    if (slot.empty()) return FWGPU_OK;
    std::lock_guard<std::mutex> g(m.mu);
    const uint32_t nrec = (uint32_t)slot.size();
    if (cached && !by_record) {  // one entry batch, every example starting from the cached field sums
        HostBatch hb;
        hb.clear();
        {   // the parts' SoA arrays land in one host batch at their offsets (copied by one thread per part), example offsets rebased
            const size_t P = parts.size();
            std::vector<size_t> fb(P + 1, 0), lb(P + 1, 0), eb_(P + 1, 0);
            for (size_t q = 0; q < P; q++) {
                if (!parts[q]->hb_ok) return fail(FWGPU_ERR_RANGE, "predict_batch: a candidate's entries were refused (see append_example)");
                fb[q + 1] = fb[q] + parts[q]->hb.ffm_hash.size();
                lb[q + 1] = lb[q] + parts[q]->hb.lr_hash.size();
                eb_[q + 1] = eb_[q] + parts[q]->hb.label.size();
            }
            hb.ffm_hash.resize(fb[P]);
            hb.ffm_val.resize(fb[P]);
            hb.ffm_fld.resize(fb[P]);
            hb.lr_hash.resize(lb[P]);
            hb.lr_val.resize(lb[P]);
            hb.lr_combo.resize(lb[P]);
            hb.label.resize(eb_[P]);
            hb.importance.resize(eb_[P]);
            hb.ffm_off.resize(eb_[P] + 1);
            hb.lr_off.resize(eb_[P] + 1);
            hb.ffm_off[0] = hb.lr_off[0] = 0;
            auto put = [&](size_t q) {
                const HostBatch &src = parts[q]->hb;
                auto cp = [](auto &dst, size_t at, const auto &from) {
                    if (!from.empty()) std::memcpy(dst.data() + at, from.data(), from.size() * sizeof(from[0]));
                };
                cp(hb.ffm_hash, fb[q], src.ffm_hash);
                cp(hb.ffm_val, fb[q], src.ffm_val);
                cp(hb.ffm_fld, fb[q], src.ffm_fld);
                cp(hb.lr_hash, lb[q], src.lr_hash);
                cp(hb.lr_val, lb[q], src.lr_val);
                cp(hb.lr_combo, lb[q], src.lr_combo);
                cp(hb.label, eb_[q], src.label);
                cp(hb.importance, eb_[q], src.importance);
                for (size_t j = 1; j < src.ffm_off.size(); j++) hb.ffm_off[eb_[q] + j] = src.ffm_off[j] + (uint32_t)fb[q];
                for (size_t j = 1; j < src.lr_off.size(); j++) hb.lr_off[eb_[q] + j] = src.lr_off[j] + (uint32_t)lb[q];
            };
            ptr->workers.run((unsigned)P, [&](unsigned q) { put(q); });
            for (const Part *pt : parts) {
                hb.max_lr = std::max(hb.max_lr, pt->hb.max_lr);
                hb.max_ffm = std::max(hb.max_ffm, pt->hb.max_ffm);
                hb.aligned4 = hb.aligned4 && pt->hb.aligned4;
            }
        }
        lap("batched");
        fwgpu_batch *eb = nullptr;
        int rc0 = batch_alloc(m.re, nrec, hb.lr_hash.size(), hb.ffm_hash.size(), &eb);
        if (rc0 != FWGPU_OK) return rc0;
        rc0 = batch_upload(eb, hb, 0);
        if (rc0 == FWGPU_OK) rc0 = refresh_stale_cache(ptr);
        if (rc0 == FWGPU_OK) rc0 = fwgpu_batch_set_cache(eb, ptr->cache);
        if (rc0 == FWGPU_OK) rc0 = fwgpu_learn_batch(m.re, eb, FWGPU_MODE_HOGWILD, /*update=*/0, nullptr);
        std::vector<float> preds(nrec);
        if (rc0 == FWGPU_OK) rc0 = fwgpu_batch_predictions(eb, preds.data(), nrec, nullptr);
        fwgpu_batch_free(eb);
        if (rc0 != FWGPU_OK) return rc0;
        for (size_t j = 0; j < slot.size(); j++) out[slot[j]] = preds[j];
        lap("predicted");
        return FWGPU_OK;
    }
    if (!m.batch || m.batch->n_cap < nrec || m.batch->words_cap < total_words) {
        if (m.batch) fwgpu_batch_free(m.batch);
        m.batch = nullptr;
        int rc0 = record_batch_alloc(m.re, &m.tr, std::max<uint32_t>(nrec * 2, 256), std::max<uint64_t>(total_words * 2, 1 << 16), &m.batch);
        if (rc0 != FWGPU_OK) return rc0;
    }
    fwgpu_batch *b = m.batch;
    int rc = FWGPU_OK;
    if (stats_ok) {
        // every thread's records go to the device from where the thread left them (no merged host copy); the threads
        // counted and validated their records as they parsed (what record_batch_upload would do again, serially)
        for (size_t q = 0; q < parts.size() && rc == FWGPU_OK; q++)
            if (!parts[q]->words.empty() &&
                hipMemcpyAsync(b->records + wbase[q], parts[q]->words.data(), parts[q]->words.size() * 4, hipMemcpyHostToDevice, nullptr) != hipSuccess)
                rc = fail(FWGPU_ERR_DEVICE, "predict_batch: copy to the device failed");
        if (rc == FWGPU_OK && hipMemcpyAsync(b->rec_off, off.data(), ((size_t)nrec + 1) * 8, hipMemcpyHostToDevice, nullptr) != hipSuccess)
            rc = fail(FWGPU_ERR_DEVICE, "predict_batch: copy to the device failed");
        b->n = nrec;
        b->n_lr = stats.tot_lr;
        b->n_ffm = stats.tot_ffm;
        b->n_words = total_words;
        b->max_lr = m.re->cfg.wiring == FWGPU_WIRING_FFM_ONLY ? 0 : stats.max_lr;
        b->max_ffm = stats.max_ffm;
        b->max_rec = stats.max_rec;
        b->aligned4 = true;
    } else {  // some record did not validate: one host copy, and record_batch_upload says which and why
        std::vector<uint32_t> words(total_words);
        for (size_t q = 0; q < parts.size(); q++)
            if (!parts[q]->words.empty()) std::memcpy(words.data() + wbase[q], parts[q]->words.data(), parts[q]->words.size() * 4);
        rc = record_batch_upload(b, &m.tr, words.data(), off.data(), nrec, 0, nullptr);
    }
    if (rc != FWGPU_OK) return rc;
    lap("uploaded");
    if (by_record) rc = fwgpu_batch_set_cache(b, ptr->cache);  // the kernel's translation leaves the covered namespaces out
    b->delta_records = delta;
    if (rc == FWGPU_OK) rc = fwgpu_learn_batch(m.re, b, FWGPU_MODE_HOGWILD, /*update=*/0, nullptr);
    std::vector<float> preds(slot.size());
    if (rc == FWGPU_OK) rc = fwgpu_batch_predictions(b, preds.data(), (uint32_t)preds.size(), nullptr);
    (void)fwgpu_batch_set_cache(b, nullptr);
    b->delta_records = false;
    if (rc != FWGPU_OK) return rc;
    for (size_t j = 0; j < slot.size(); j++) out[slot[j]] = preds[j];
    lap("predicted");
    return FWGPU_OK;
}

// fwgpu_predictor_predict_text by the existing route: the lines, each with its newline, through fwgpu_predictor_predict_batch
static int predict_text_by_lines(FfiPredictor *p, const char *text, uint64_t len, int with_cache, float *out, uint64_t cap, uint64_t *n) {
    std::vector<std::string> lines;
    for (uint64_t pos = 0; pos < len;) {
        const char *e = static_cast<const char *>(std::memchr(text + pos, '\n', len - pos));
        const uint64_t size = e ? (uint64_t)(e - (text + pos)) + 1 : len - pos;
        lines.emplace_back(text + pos, size);
        if (!e) lines.back().push_back('\n');
        pos += size;
    }
    p->text_lines = p->text_host_lines = lines.size();
    p->text_fell_back = 1;
    *n = lines.size();
    if (lines.size() > cap || lines.size() > 0xffffffffull) return fail(FWGPU_ERR_RANGE, "predict_text: more lines than the output holds");
    std::vector<const char *> ptrs(lines.size());
    for (size_t i = 0; i < lines.size(); i++) ptrs[i] = lines[i].c_str();
    return fwgpu_predictor_predict_batch(p, ptrs.data(), (uint32_t)ptrs.size(), with_cache, out);
}

// A request as one text, one candidate per line: out[i] is what fw_predict_with_cache (with_cache != 0) or fw_predict would return for line i
// with its newline, *n the number of lines.  See the head of this file for the route.
int fwgpu_predictor_predict_text(FfiPredictor *ptr, const char *text, uint64_t len, int with_cache, float *out, uint64_t cap, uint64_t *n) {
    if (!ptr || (!text && len) || (!out && cap) || !n) return fail(FWGPU_ERR_INVALID, "NULL argument");
    *n = 0;
    ptr->text_lines = ptr->text_host_lines = 0;
    ptr->text_fell_back = 0;
    if (len == 0) return FWGPU_OK;
    SharedModel &m = *ptr->model;
    const bool cand = with_cache != 0;
    if (std::getenv("FWGPU_SERVING_HOST_PARSE") || (cand && !(ptr->cache && ptr->prefix && ptr->delta_ok)))
        return predict_text_by_lines(ptr, text, len, with_cache, out, cap, n);
    std::string owned;
    if (text[len - 1] != '\n') {  // the last line gets its newline, as every line a caller of fw_predict sends has one
        owned.assign(text, len);
        owned.push_back('\n');
        text = owned.data();
        len++;
    }
    const char *piece_env = std::getenv("FWGPU_SERVING_TEXT_PIECE");
    const uint64_t piece = piece_env && std::atoll(piece_env) > 0 ? (uint64_t)std::atoll(piece_env) : 0;
    std::unique_lock<std::mutex> g(m.mu);
    int rc = FWGPU_OK;
    if (!m.tp && (rc = fwgpu_text_parser_create(m.vw, m.re->device, &m.tp)) != FWGPU_OK) return rc;
    TextLines tl;
    if ((rc = text_lines_scan(m.tp, cand ? ptr->prefix : nullptr, cand ? ptr->cache : nullptr, &m.tr, text, len, piece, /*zero_word1=*/true, &tl)) != FWGPU_OK)
        return rc;
    uint64_t host_lines = 0;
    (void)fwgpu_text_parser_last_lines(m.tp, nullptr, &host_lines);
    const uint32_t ctx_len = cand ? (uint32_t)ptr->cache->ctx_rec.size() : 0;
    RecordStats stats;
    std::vector<uint64_t> off(1, 0);
    std::vector<uint64_t> slot;  // which line each record belongs to
    bool by_lines = false;
    for (uint64_t i = 0; i < tl.n_lines && !by_lines; i++) {
        const fwgpu_candidate_info &li = tl.info[i];
        const uint64_t nw = tl.rec_off[i + 1] - tl.rec_off[i];
        if (li.code != FWGPU_OK || nw == 0) continue;
        if (!li.record_ok || (cand && !li.is_delta)) {  // the rule fwgpu_predictor_predict_batch has: the whole request goes the other way
            by_lines = true;
            break;
        }
        stats.max_lr = std::max(stats.max_lr, li.n_lr);
        stats.max_ffm = std::max(stats.max_ffm, li.n_ffm);
        stats.max_rec = std::max(stats.max_rec, (uint32_t)nw + ctx_len);  // (LDS holds the context's record behind the candidate's)
        stats.tot_lr += li.n_lr;
        stats.tot_ffm += li.n_ffm;
        off.push_back(tl.rec_off[i + 1]);
        slot.push_back(i);
    }
    if (by_lines || tl.n_lines > 0xffffffffull) {
        g.unlock();
        return predict_text_by_lines(ptr, text, len, with_cache, out, cap, n);
    }
    *n = tl.n_lines;
    ptr->text_lines = tl.n_lines;
    ptr->text_host_lines = host_lines;
    if (tl.n_lines > cap) return fail(FWGPU_ERR_RANGE, "predict_text: more lines than the output holds");
    for (uint64_t i = 0; i < tl.n_lines; i++) out[i] = kExceptionErrorCode;
    if (slot.empty()) return FWGPU_OK;
    const uint32_t nrec = (uint32_t)slot.size();
    const uint64_t total_words = tl.n_words;
    if (!m.batch || m.batch->n_cap < nrec || m.batch->words_cap < total_words) {
        if (m.batch) fwgpu_batch_free(m.batch);
        m.batch = nullptr;
        if ((rc = record_batch_alloc(m.re, &m.tr, std::max<uint32_t>(nrec * 2, 256), std::max<uint64_t>(total_words * 2, 1 << 16), &m.batch)) != FWGPU_OK) return rc;
    }
    fwgpu_batch *b = m.batch;
    if ((rc = text_lines_place(m.tp, b->records)) != FWGPU_OK) return rc;  // write pass + the host-parsed records; the records are there on return
    if (hipMemcpyAsync(b->rec_off, off.data(), ((size_t)nrec + 1) * 8, hipMemcpyHostToDevice, nullptr) != hipSuccess)
        return fail(FWGPU_ERR_DEVICE, "predict_text: copy to the device failed");
    b->n = nrec;
    b->n_lr = stats.tot_lr;
    b->n_ffm = stats.tot_ffm;
    b->n_words = total_words;
    b->max_lr = m.re->cfg.wiring == FWGPU_WIRING_FFM_ONLY ? 0 : stats.max_lr;
    b->max_ffm = stats.max_ffm;
    b->max_rec = stats.max_rec;
    b->aligned4 = true;
    if (cand) rc = fwgpu_batch_set_cache(b, ptr->cache);
    b->delta_records = cand;
    if (rc == FWGPU_OK) rc = fwgpu_learn_batch(m.re, b, FWGPU_MODE_HOGWILD, /*update=*/0, nullptr);
    std::vector<float> preds(nrec);
    if (rc == FWGPU_OK) rc = fwgpu_batch_predictions(b, preds.data(), nrec, nullptr);
    (void)fwgpu_batch_set_cache(b, nullptr);
    b->delta_records = false;
    if (rc != FWGPU_OK) return rc;
    for (size_t j = 0; j < slot.size(); j++) out[slot[j]] = preds[j];
    return FWGPU_OK;
}

// The candidates of SEVERAL requests in one launch: predictors[r] (the prototype and clone_lite copies of one model, each after its own
// fw_setup_cache; the same one may appear twice) with its lines inputs[r][0 .. n_inputs[r]).  The existing entry route per line -- parse after the
// context's prefix, translate, filter by the cache's features -- with the requests spread over the worker pool, then ONE shared entry batch with a cache
// per example (fwgpu_batch_set_caches) and ONE launch, under the model's mutex taken once.
int fwgpu_predictor_predict_requests(FfiPredictor *const *predictors, uint32_t n_requests, const char *const *const *inputs, const uint32_t *n_inputs,
                                     float *const *out) {
    if (n_requests == 0) return FWGPU_OK;
    if (!predictors || !inputs || !n_inputs || !out) return fail(FWGPU_ERR_INVALID, "NULL argument");
    static const char *kSee = " (fwgpu_predictor_predict_batch serves this predictor, one request per call)";
    uint64_t total = 0;
    for (uint32_t r = 0; r < n_requests; r++) {
        if (!predictors[r] || (n_inputs[r] && (!inputs[r] || !out[r]))) return fail(FWGPU_ERR_INVALID, "NULL argument");
        if (predictors[r]->model != predictors[0]->model)
            return fail(FWGPU_ERR_INVALID, std::string("predict_requests: the predictors are not the prototype and clone_lite copies of ONE model") + kSee);
        total += n_inputs[r];
    }
    if (total > 0xffffffffull) return fail(FWGPU_ERR_RANGE, "predict_requests: more than 2^32 - 1 lines");
    SharedModel &m = *predictors[0]->model;
    if (m.re->packed() && !m.re->packed_caches)
        return fail(FWGPU_ERR_INVALID, std::string("predict_requests: a --packed_weights predictor keeps no device cache") + kSee);
    if (m.re->cfg.ffm_k == 0) return fail(FWGPU_ERR_INVALID, std::string("predict_requests: a model without an FFM block keeps no device cache") + kSee);
    if (m.re->nn.n_layers) return fail(FWGPU_ERR_INVALID, std::string("predict_requests: models with a deep head are not served by the requests route") + kSee);
    std::vector<const fwgpu_block_cache *> caches;  // the set: every predictor's cache once
    std::vector<uint32_t> cache_of_request(n_requests);
    for (uint32_t r = 0; r < n_requests; r++) {
        const FfiPredictor *p = predictors[r];
        if (!p->cache || !p->prefix) return fail(FWGPU_ERR_INVALID, std::string("predict_requests: a predictor has no device cache (no fw_setup_cache yet)") + kSee);
        size_t c = 0;
        while (c < caches.size() && caches[c] != p->cache) c++;
        if (c == caches.size()) caches.push_back(p->cache);
        cache_of_request[r] = (uint32_t)c;
        for (uint32_t j = 0; j < n_inputs[r]; j++) out[r][j] = kExceptionErrorCode;
    }
    if (total == 0) return FWGPU_OK;
    // the lines of all requests in equal shares per thread (FWGPU_SERVING_THREADS overrides; by default one thread per 128 lines, up to the cores there are and at most 32)
    FfiPredictor *host = predictors[0];  // its worker pool and per-thread parsers serve the call
    unsigned T = 1;
    {
        const char *env = std::getenv("FWGPU_SERVING_THREADS");
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        T = env && std::atoi(env) > 0 ? (unsigned)std::atoi(env) : std::min<unsigned>(std::min<unsigned>(32, hw), std::max<unsigned>(1, (unsigned)(total / 128)));
        T = std::min<unsigned>(T, 64);
    }
    while (host->parts.size() < T) host->parts.push_back(std::make_unique<Part>());
    std::vector<uint64_t> first(n_requests + 1, 0);  // the lines of all requests, numbered through: thread t takes an equal share of them
    for (uint32_t r = 0; r < n_requests; r++) first[r + 1] = first[r] + n_inputs[r];
    std::vector<std::vector<uint32_t>> where(T), line(T), which(T);  // per thread and kept example: its request, its line there, its cache of the set
    auto work = [&](unsigned t) {
        Part &pt = *host->parts[t];
        pt.reset();
        if (!pt.parser && fwgpu_parser_create(m.vw, &pt.parser) != FWGPU_OK) {
            pt.hb_ok = false;
            return;
        }
        std::vector<uint32_t> &rec = pt.rec;
        if (rec.size() < 4096) rec.resize(4096);
        std::vector<fwgpu_lr_entry> t_lr;
        std::vector<fwgpu_ffm_entry> t_ffm;
        const uint64_t a = total * t / T, e = total * (t + 1) / T;
        uint32_t r = (uint32_t)(std::upper_bound(first.begin(), first.end(), a) - first.begin()) - 1;
        for (uint64_t g = a; g < e; g++) {
            while (g >= first[r + 1]) r++;
            const uint32_t j = (uint32_t)(g - first[r]);
            const FfiPredictor *p = predictors[r];
            const char *text = inputs[r][j];
            if (!text) continue;
            uint32_t nw = 0;
            int rc;
            for (;;) {
                rc = fwgpu_parser_parse_after_prefix(pt.parser, p->prefix, text, std::strlen(text), rec.data(), (uint32_t)rec.size(), &nw);
                if (rc == FWGPU_ERR_RANGE && rec.size() < (1u << 24)) {
                    rec.resize(rec.size() * 4);
                    continue;
                }
                break;
            }
            if (rc != FWGPU_OK || nw == 0) {
                if (rc == FWGPU_OK) out[r][j] = kEofErrorCode;
                continue;
            }
            rec[1] = 0;  // a request carries no label
            float label, imp;
            if (translate_record(&m.tr, rec.data(), nw, t_lr, t_ffm, &label, &imp) != FWGPU_OK) continue;
            uint32_t kept = 0;
            if (fwgpu_block_cache_filter(p->cache, t_ffm.data(), (uint32_t)t_ffm.size(), t_ffm.data(), &kept) != FWGPU_OK) continue;
            if (append_example(m.re, pt.hb, t_lr.data(), (uint32_t)t_lr.size(), t_ffm.data(), kept, 0.0f, 1.0f) != FWGPU_OK) {
                pt.hb_ok = false;
                continue;
            }
            where[t].push_back(r);
            line[t].push_back(j);
            which[t].push_back(cache_of_request[r]);
        }
    };
    host->workers.run(T, work);
    // one entry batch: every thread's SoA arrays go to the device from where the thread left them, at their offsets (no merged host copy); only the
    // example offsets are rebased here
    std::vector<size_t> fb(T + 1, 0), lb(T + 1, 0);
    std::vector<uint32_t> ffm_off(1, 0), lr_off(1, 0), ex_req, ex_line, ex_cache;
    uint32_t max_lr = 0, max_ffm = 0;
    bool aligned4 = true;
    for (unsigned t = 0; t < T; t++) {
        const HostBatch &src = host->parts[t]->hb;
        if (!host->parts[t]->hb_ok) return fail(FWGPU_ERR_RANGE, "predict_requests: a candidate's entries were refused (see append_example)");
        fb[t + 1] = fb[t] + src.ffm_hash.size();
        lb[t + 1] = lb[t] + src.lr_hash.size();
        for (size_t j = 1; j < src.ffm_off.size(); j++) ffm_off.push_back(src.ffm_off[j] + (uint32_t)fb[t]);
        for (size_t j = 1; j < src.lr_off.size(); j++) lr_off.push_back(src.lr_off[j] + (uint32_t)lb[t]);
        max_lr = std::max(max_lr, src.max_lr);
        max_ffm = std::max(max_ffm, src.max_ffm);
        aligned4 = aligned4 && src.aligned4;
        ex_req.insert(ex_req.end(), where[t].begin(), where[t].end());
        ex_line.insert(ex_line.end(), line[t].begin(), line[t].end());
        ex_cache.insert(ex_cache.end(), which[t].begin(), which[t].end());
    }
    const uint32_t nrec = (uint32_t)ex_req.size();
    if (nrec == 0) return FWGPU_OK;
    if (fb[T] > 0xffffffffull || lb[T] > 0xffffffffull) return fail(FWGPU_ERR_RANGE, "predict_requests: more than 2^32 - 1 entries in one call");
    if (max_ffm > 4096 || max_lr > 4096)
        return fail(FWGPU_ERR_INVALID, std::string("predict_requests: a line has more than 4096 entries of a kind") + kSee);
    std::lock_guard<std::mutex> g(m.mu);
    int rc = FWGPU_OK;
    if (!m.requests || m.requests->n_cap < nrec || m.requests->n_lr < lb[T] || m.requests->n_ffm < fb[T]) {
        if (m.requests) fwgpu_batch_free(m.requests);
        m.requests = nullptr;
        const uint32_t cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(2ull * nrec, 256), 0xffffffffull);
        if ((rc = batch_alloc(m.re, cap, std::max<uint64_t>(2 * lb[T], 1 << 16), std::max<uint64_t>(2 * fb[T], 1 << 14), &m.requests)) != FWGPU_OK) return rc;
        m.requests->n_cap = cap;
    }
    fwgpu_batch *eb = m.requests;
    eb->n = nrec;
    auto up = [&](void *dst, const void *src, size_t bytes) {
        if (rc == FWGPU_OK && bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, nullptr) != hipSuccess)
            rc = fail(FWGPU_ERR_DEVICE, "predict_requests: copy to the device failed");
    };
    for (unsigned t = 0; t < T; t++) {  // (labels, importances and combo slots are not read by a predict-only launch of a model without a deep head)
        const HostBatch &src = host->parts[t]->hb;
        up(eb->ffm_hash + fb[t], src.ffm_hash.data(), src.ffm_hash.size() * 4);
        up(eb->ffm_val + fb[t], src.ffm_val.data(), src.ffm_val.size() * 4);
        up(eb->ffm_fld + fb[t], src.ffm_fld.data(), src.ffm_fld.size());
        up(eb->lr_hash + lb[t], src.lr_hash.data(), src.lr_hash.size() * 4);
        up(eb->lr_val + lb[t], src.lr_val.data(), src.lr_val.size() * 4);
    }
    up(eb->ffm_off, ffm_off.data(), ffm_off.size() * 4);
    up(eb->lr_off, lr_off.data(), lr_off.size() * 4);
    eb->max_lr = max_lr;
    eb->max_ffm = max_ffm;
    eb->aligned4 = aligned4;
    for (uint32_t r = 0; r < n_requests && rc == FWGPU_OK; r++) rc = refresh_stale_cache(predictors[r]);  // (--packed_context_cache: before the set is attached)
    if (rc == FWGPU_OK) rc = fwgpu_batch_set_caches(eb, caches.data(), (uint32_t)caches.size(), ex_cache.data());
    if (rc == FWGPU_OK) rc = fwgpu_learn_batch(m.re, eb, FWGPU_MODE_HOGWILD, /*update=*/0, nullptr);
    std::vector<float> preds(nrec);
    if (rc == FWGPU_OK) rc = fwgpu_batch_predictions(eb, preds.data(), nrec, nullptr);
    // (the set stays attached to this private batch until the next call replaces it: no launch happens in between, and detaching would free its table)
    if (rc != FWGPU_OK) return rc;
    for (uint32_t i = 0; i < nrec; i++) out[ex_req[i]][ex_line[i]] = preds[i];
    return FWGPU_OK;
}

int fwgpu_predictor_last_text_route(const FfiPredictor *ptr, uint64_t *lines, uint64_t *host_lines, int *fell_back) {
    if (!ptr) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (lines) *lines = ptr->text_lines;
    if (host_lines) *host_lines = ptr->text_host_lines;
    if (fell_back) *fell_back = ptr->text_fell_back;
    return FWGPU_OK;
}

// The hot patch of a --packed_weights model from a byte diff of two published files (fwgpu_packed_apply_diff), under the model's mutex.  The
// prototype and every clone_lite copy share the tables, so all of them see it.  Plain --packed_weights predictors keep no device cache, so nothing
// derived from the weights goes stale; with --packed_context_cache the patch bumps the regressor's weights epoch under this mutex, and every
// predictor of the model rebuilds its cache before its next cached call (refresh_stale_cache).
int fwgpu_predictor_apply_diff(FfiPredictor *ptr, const uint8_t *diff, uint64_t len) {
    if (!ptr || (len && !diff)) return fail(FWGPU_ERR_INVALID, "NULL argument");
    SharedModel &m = *ptr->model;
    if (!m.re->packed())
        return fail(FWGPU_ERR_INVALID, "predictor_apply_diff: the predictor was not created with --packed_weights: its f32 tables are not the file's bytes, load the file");
    std::lock_guard<std::mutex> g(m.mu);
    return fwgpu_packed_apply_diff(m.re, diff, len, nullptr);
}

}  // extern "C"
