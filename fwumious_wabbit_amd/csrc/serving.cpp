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
// the per-example kernel; with --head_requests on the command (fwgpu_enable_head_requests) fwgpu_predictor_predict_requests serves such a model too,
// through the head-input kernels of requests_head.hip; with --fused_head (fwgpu_enable_fused_head) a batch of any size takes the batched head route and
// small ones run the whole head in one launch (head_fused.hip); with --packed_weights --packed_head_requests (fwgpu_packed_enable_head_requests) a
// deep-head model on packed weights gets the same: fw_setup_cache builds the cache from the packed table, every cached call takes the ENTRY route
// through the set of one, and fwgpu_predictor_predict_requests is one launch of requests_head.hip's packed form (fwgpu_predictor_predict_text keeps
// the host-translated lines).  Predictors created with --packed_weights keep the uncached route (whole line scored), which gives the same result --
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
#include "requests_text.h"
#include "textparse.h"

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
    // fwgpu_predictor_predict_requests_text: the translator's arrays on the device (as an empty record batch holds them), what its kernels write
    // between the passes, and what every call uploads (the requests' offsets, the caches of the set); grown on demand and reused
    fwgpu_batch *rt_tr = nullptr;
    void *rt_scratch = nullptr, *rt_side = nullptr;
    size_t rt_scratch_bytes = 0, rt_side_bytes = 0;
    ~SharedModel() {
        if (rt_scratch) (void)hipFree(rt_scratch);
        if (rt_side) (void)hipFree(rt_side);
        if (rt_tr) fwgpu_batch_free(rt_tr);
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
    std::vector<uint32_t> ctx_record;      // fwgpu_predictor_predict_requests_text: the context's own record, when the scanned context is that record
    // ... and what its kernels read of this predictor's cache, as it is uploaded: present keys | 64 filter words | the record | cover bits (each part
    // 8-byte aligned; the byte offsets of the last three); built by the first text call after fw_setup_cache (rt_piece_of), empty before
    std::vector<uint64_t> rt_piece;
    size_t rt_piece_bits = 0, rt_piece_rec = 0, rt_piece_cover = 0;
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
    if (m.re->packed() && m.re->nn.n_layers) {
        // --packed_weights on a model with a deep head: the head-input kernel of the packed table takes entry batches only (head_packed.hip), so the
        // line -- with a context, the whole context + candidate line: such a predictor keeps no cache -- is translated here and goes as a batch of one
        float label, imp, out = kExceptionErrorCode;
        if (translate_record(&m.tr, p->record.data(), n_words, p->lr, p->ffm, &label, &imp) != FWGPU_OK) return kExceptionErrorCode;
        if (fwgpu_predict(m.re, p->lr.data(), (uint32_t)p->lr.size(), p->ffm.data(), (uint32_t)p->ffm.size(), &out) != FWGPU_OK) return kExceptionErrorCode;
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
    bool packed = false, packed_caches = false, head_requests = false, fused_head = false, packed_head_requests = false;
    for (const auto &w : words) {
        if (w.rfind("--initial_regressor=", 0) == 0) weights = w.substr(std::strlen("--initial_regressor="));
        if (w == "--packed_weights") packed = true;  // ours: the FFM weights stay f16 buckets on the device (fwgpu_model_load_packed)
        if (w == "--packed_context_cache") packed_caches = true;  // ours: ... and context caches are built from them (fwgpu_packed_enable_caches)
        if (w == "--head_requests") head_requests = true;  // ours: a deep-head model takes the requests route (fwgpu_enable_head_requests)
        if (w == "--fused_head") fused_head = true;  // ours: small batches run the whole head in one launch (fwgpu_enable_fused_head)
        // ours: a deep-head model on packed weights keeps context caches and takes the requests route (fwgpu_packed_enable_head_requests)
        if (w == "--packed_head_requests") packed_head_requests = true;
    }
    if (packed_caches && !packed) {
        set_error("--packed_context_cache is valid only together with --packed_weights (an f32 predictor keeps its context cache without it)");
        return nullptr;
    }
    if (packed_head_requests && !packed) {
        set_error("--packed_head_requests is valid only together with --packed_weights (on f32 weights --head_requests serves a model with a deep head)");
        return nullptr;
    }
    if (weights.empty()) {
        set_error("Cannot resolve input weights file name");  // the reference panics here (lib.rs:164-167)
        return nullptr;
    }
    if (head_requests || fused_head || packed_head_requests) {  // the file's header decides, before a device is touched
        fwgpu_model_instance *mi = nullptr;
        fwgpu_nn_config nn{};
        if (fwgpu_model_read_header(weights.c_str(), nullptr, &mi) != FWGPU_OK) return nullptr;
        const int rc = fwgpu_mi_configs(mi, device, nullptr, nullptr, &nn);
        fwgpu_mi_free(mi);
        if (rc != FWGPU_OK) return nullptr;
        if (fused_head && nn.n_layers == 0) {
            set_error(packed ? "--fused_head is not valid together with --packed_weights on a model without a deep head (a packed regressor has no head route for it)"
                             : "--fused_head is valid only on a model with a deep head");
            return nullptr;
        }
        if (head_requests && (nn.n_layers == 0 || packed)) {
            set_error(packed ? "--head_requests is not valid together with --packed_weights (a packed regressor keeps no context cache for a deep head)"
                             : "--head_requests is valid only on a model with a deep head (fwgpu_predictor_predict_requests serves a headless model without it)");
            return nullptr;
        }
        if (packed_head_requests && nn.n_layers == 0) {
            set_error("--packed_head_requests is valid only on a model with a deep head (--packed_context_cache serves a headless model on packed weights)");
            return nullptr;
        }
    }
    auto model = std::make_shared<SharedModel>();
    if ((packed ? fwgpu_model_load_packed_head(weights.c_str(), device, &model->vw, &model->mi, &model->re)
                : fwgpu_model_load(weights.c_str(), device, /*immutable=*/1, &model->vw, &model->mi, &model->re)) != FWGPU_OK)
        return nullptr;
    if (packed_caches && fwgpu_packed_enable_caches(model->re) != FWGPU_OK) return nullptr;
    if (head_requests && fwgpu_enable_head_requests(model->re) != FWGPU_OK) return nullptr;  // (a model without a head: an error, with the reason)
    if (fused_head && fwgpu_enable_fused_head(model->re) != FWGPU_OK) return nullptr;
    if (packed_head_requests && fwgpu_packed_enable_head_requests(model->re) != FWGPU_OK) return nullptr;
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
    ptr->rt_piece.clear();
    ptr->ctx_record.clear();  // (kept for every kind of cache: a packed regressor's cache knows no record of its own)
    if (fwgpu_parse_prefix_is_record(ptr->prefix, ptr->record.data(), n_words)) ptr->ctx_record.assign(ptr->record.begin(), ptr->record.begin() + n_words);
    SharedModel &m = *ptr->model;
    // (a packed regressor keeps no device-side context cache: the whole context + candidate record is scored -- unless --packed_context_cache or,
    // on a model with a deep head, --packed_head_requests)
    if (m.re->cfg.ffm_k != 0 && m.re->packed() && m.re->keeps_packed_caches()) {
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
    // --packed_weights on a model with a deep head: the head-input kernel of the packed table takes entry batches only (head_packed.hip), so every line
    // is translated here, whole, and nothing is filtered (such a predictor keeps no context cache -- with --packed_head_requests it has one, and a
    // cached call takes the entry route above: translated, filtered, the set of one)
    const bool whole_entries = m.re->packed() && m.re->nn.n_layers != 0;
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
            if ((cached && !by_record) || whole_entries) {
                float label, imp;
                if (translate_record(&m.tr, rec.data(), nw, t_lr, t_ffm, &label, &imp) != FWGPU_OK) continue;
                uint32_t kept = (uint32_t)t_ffm.size();
                if (cached && fwgpu_block_cache_filter(ptr->cache, t_ffm.data(), (uint32_t)t_ffm.size(), t_ffm.data(), &kept) != FWGPU_OK) continue;
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
    if ((cached && !by_record) || whole_entries) {  // one entry batch, every example starting from the cached field sums (whole_entries: from nothing)
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
        if (rc0 == FWGPU_OK && cached) rc0 = refresh_stale_cache(ptr);
        if (rc0 == FWGPU_OK && cached) rc0 = fwgpu_batch_set_cache(eb, ptr->cache);
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
    // (--packed_weights on a model with a deep head: entry batches only -- fwgpu_predictor_predict_batch translates the lines)
    if (std::getenv("FWGPU_SERVING_HOST_PARSE") || (cand && !(ptr->cache && ptr->prefix && ptr->delta_ok)) || (m.re->packed() && m.re->nn.n_layers))
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

// fwgpu_predictor_predict_requests_text: the refusals of fwgpu_predictor_predict_requests, with its messages, and the set (every predictor's cache once)
static int requests_set_of(FfiPredictor *const *predictors, uint32_t n_requests, std::vector<const fwgpu_block_cache *> &caches,
                           std::vector<uint32_t> &cache_of_request) {
    static const char *kSee = " (fwgpu_predictor_predict_batch serves this predictor, one request per call)";
    for (uint32_t r = 0; r < n_requests; r++) {
        if (!predictors[r]) return fail(FWGPU_ERR_INVALID, "NULL argument");
        if (predictors[r]->model != predictors[0]->model)
            return fail(FWGPU_ERR_INVALID, std::string("predict_requests: the predictors are not the prototype and clone_lite copies of ONE model") + kSee);
    }
    SharedModel &m = *predictors[0]->model;
    if (m.re->packed() && !m.re->keeps_packed_caches())
        return fail(FWGPU_ERR_INVALID, std::string("predict_requests: a --packed_weights predictor keeps no device cache") + kSee);
    if (m.re->cfg.ffm_k == 0) return fail(FWGPU_ERR_INVALID, std::string("predict_requests: a model without an FFM block keeps no device cache") + kSee);
    if (m.re->nn.n_layers && !m.re->serves_head_requests()) return fail(FWGPU_ERR_INVALID, std::string("predict_requests: models with a deep head are not served by the requests route") + kSee);
    caches.clear();
    cache_of_request.assign(n_requests, 0);
    for (uint32_t r = 0; r < n_requests; r++) {
        const FfiPredictor *p = predictors[r];
        if (!p->cache || !p->prefix) return fail(FWGPU_ERR_INVALID, std::string("predict_requests: a predictor has no device cache (no fw_setup_cache yet)") + kSee);
        size_t c = 0;
        while (c < caches.size() && caches[c] != p->cache) c++;
        if (c == caches.size()) caches.push_back(p->cache);
        cache_of_request[r] = (uint32_t)c;
    }
    return FWGPU_OK;
}
static const char *const kRequestsTooManyEntries =
    "predict_requests: a line has more than 4096 entries of a kind (fwgpu_predictor_predict_batch serves this predictor, one request per call)";

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
    if (m.re->packed() && !m.re->keeps_packed_caches())
        return fail(FWGPU_ERR_INVALID, std::string("predict_requests: a --packed_weights predictor keeps no device cache") + kSee);
    if (m.re->cfg.ffm_k == 0) return fail(FWGPU_ERR_INVALID, std::string("predict_requests: a model without an FFM block keeps no device cache") + kSee);
    if (m.re->nn.n_layers && !m.re->serves_head_requests()) return fail(FWGPU_ERR_INVALID, std::string("predict_requests: models with a deep head are not served by the requests route") + kSee);
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
    const bool head = m.re->nn.n_layers != 0;
    for (unsigned t = 0, ex0 = 0; t < T; t++) {  // (labels, importances and combo slots are not read by a predict-only launch of a model without a deep head)
        const HostBatch &src = host->parts[t]->hb;
        if (head) {  // --head_requests, --packed_head_requests: the head's input keeps one LR sum per combo slot, and head_step reads {label, importance}
            up(eb->lr_combo + lb[t], src.lr_combo.data(), src.lr_combo.size() * sizeof(uint16_t));
            up(eb->label + ex0, src.label.data(), src.label.size() * 4);
            up(eb->importance + ex0, src.importance.data(), src.importance.size() * 4);
            ex0 += (unsigned)src.label.size();
        }
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

// fwgpu_predictor_predict_requests_text by the existing route: every request's lines, each with its newline, through fwgpu_predictor_predict_requests
static int predict_requests_text_by_lines(FfiPredictor *const *predictors, uint32_t n_requests, const char *const *texts, const uint64_t *lens,
                                          float *const *out, const uint64_t *caps, uint64_t *n_lines) {
    std::vector<std::vector<std::string>> lines(n_requests);
    uint64_t total = 0;
    bool fits = true;
    for (uint32_t r = 0; r < n_requests; r++) {
        for (uint64_t pos = 0; pos < lens[r];) {
            const char *e = static_cast<const char *>(std::memchr(texts[r] + pos, '\n', lens[r] - pos));
            const uint64_t size = e ? (uint64_t)(e - (texts[r] + pos)) + 1 : lens[r] - pos;
            lines[r].emplace_back(texts[r] + pos, size);
            if (!e) lines[r].back().push_back('\n');
            pos += size;
        }
        n_lines[r] = lines[r].size();
        total += lines[r].size();
        fits = fits && lines[r].size() <= caps[r] && lines[r].size() <= 0xffffffffull;
    }
    predictors[0]->text_lines = predictors[0]->text_host_lines = total;
    predictors[0]->text_fell_back = 1;
    if (!fits) return fail(FWGPU_ERR_RANGE, "predict_requests_text: more lines than a request's output holds");
    std::vector<std::vector<const char *>> ptrs(n_requests);
    std::vector<const char *const *> inputs(n_requests);
    std::vector<uint32_t> n_inputs(n_requests);
    for (uint32_t r = 0; r < n_requests; r++) {
        for (const std::string &l : lines[r]) ptrs[r].push_back(l.c_str());
        inputs[r] = ptrs[r].data();
        n_inputs[r] = (uint32_t)ptrs[r].size();
    }
    return fwgpu_predictor_predict_requests(predictors, n_requests, inputs.data(), n_inputs.data(), out);
}

// The predictor's piece of the text call's upload, made once per fw_setup_cache.  false: the scanned context is not its own record, or the record is
// not one the kernels may read by what its slot words say (every range inside it, behind the slots, of whole {hash, value} pairs).
static bool rt_piece_of(FfiPredictor *p, uint32_t nns) {
    if (!p->rt_piece.empty()) return true;
    const std::vector<uint32_t> &rec = p->ctx_record;
    if (rec.size() < 3 + (size_t)nns || rec.size() > kRtMaxRecord) return false;
    for (uint32_t ns = 0; ns < nns; ns++) {
        const uint32_t w = rec[3 + ns], st = (w >> 16) & 0x3fffu, en = w & 0xffffu;
        if ((w & 0x80000000u) && w != 0x80000000u && !(en <= rec.size() && en >= st && st >= 3 + nns && !((en - st) & 1u))) return false;
    }
    const std::vector<uint64_t> &present = p->cache->present;
    auto up8 = [](size_t x) { return (x + 7) & ~(size_t)7; };
    p->rt_piece_bits = 8 * present.size();
    p->rt_piece_rec = p->rt_piece_bits + 8 * 64;
    p->rt_piece_cover = up8(p->rt_piece_rec + 4 * rec.size());
    p->rt_piece.assign(up8(p->rt_piece_cover + 4 * (((size_t)nns + 31) / 32)) / 8, 0);
    unsigned char *b = reinterpret_cast<unsigned char *>(p->rt_piece.data());
    if (!present.empty()) std::memcpy(b, present.data(), 8 * present.size());
    uint64_t *bits = reinterpret_cast<uint64_t *>(b + p->rt_piece_bits);
    for (uint64_t key : present) {  // (context_cache.cpp present_bit)
        const uint32_t h = (uint32_t)((key * 0x9e3779b97f4a7c15ULL) >> 52);
        bits[h >> 6] |= 1ull << (h & 63);
    }
    std::memcpy(b + p->rt_piece_rec, rec.data(), 4 * rec.size());
    uint32_t *cover = reinterpret_cast<uint32_t *>(b + p->rt_piece_cover);
    for (uint32_t ns = 0; ns < nns; ns++)
        if (rec[3 + ns] != 0x80000000u) cover[ns >> 5] |= 1u << (ns & 31);  // NO_FEATURES (parser.rs:19)
    return true;
}

// device memory kept between calls: grown (never shrunk) to `bytes`
static int rt_grow(void **p, size_t *cap, size_t bytes) {
    if (bytes <= *cap) return FWGPU_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    const size_t want = bytes + bytes / 2 + 256;
    FWGPU_HIP(hipMalloc(p, want));
    *cap = want;
    return FWGPU_OK;
}

// The candidates of SEVERAL requests from their TEXT, a candidate per line, without the host's parser, translator or filter: ONE plain pass of the
// device parser over all texts (text_lines_device), the count / scan / emit kernels of requests_text.hip -- which decide the cache's record rule per
// line against the line's OWN request's cache and write the filtered entries in the host translator's order straight into the entry batch -- and the
// ONE launch fwgpu_predictor_predict_requests makes.  The host reads one small block (totals, maxima, the flag, every request's first line) and the
// predictions.  The whole call goes through fwgpu_predictor_predict_requests on the split lines instead (fell_back) when any line is not the device
// parser's, does not start with '|', fills a namespace its context fills or repeats a cached FFM feature; when a predictor's scanned context is not its
// own record; with FWGPU_SERVING_HOST_PARSE; with a namespace map beyond the device parser's; and with more text than one parser pass takes.
int fwgpu_predictor_predict_requests_text(FfiPredictor *const *predictors, uint32_t n_requests, const char *const *texts, const uint64_t *lens,
                                          float *const *out, const uint64_t *caps, uint64_t *n_lines) {
    if (n_requests == 0) return FWGPU_OK;
    if (!predictors || !texts || !lens || !out || !caps || !n_lines) return fail(FWGPU_ERR_INVALID, "NULL argument");
    uint64_t total_len = 0;
    for (uint32_t r = 0; r < n_requests; r++) {
        if (!predictors[r] || (lens[r] && !texts[r]) || (caps[r] && !out[r])) return fail(FWGPU_ERR_INVALID, "NULL argument");
        n_lines[r] = 0;
        total_len += lens[r] + (lens[r] && texts[r][lens[r] - 1] != '\n' ? 1 : 0);
    }
    std::vector<const fwgpu_block_cache *> caches;
    std::vector<uint32_t> cache_of_request;
    if (const int rc0 = requests_set_of(predictors, n_requests, caches, cache_of_request)) return rc0;
    FfiPredictor *host = predictors[0];
    host->text_lines = host->text_host_lines = 0;
    host->text_fell_back = 0;
    if (total_len == 0) return FWGPU_OK;
    SharedModel &m = *host->model;
    auto by_lines = [&]() { return predict_requests_text_by_lines(predictors, n_requests, texts, lens, out, caps, n_lines); };
    if (std::getenv("FWGPU_SERVING_HOST_PARSE") || total_len > std::min<uint64_t>(0xffffffffull, text_device_max_bytes())) return by_lines();
    std::vector<FfiPredictor *> owner(caches.size(), nullptr);  // the predictor that holds each cache of the set (and its context's record)
    for (uint32_t r = 0; r < n_requests; r++) owner[cache_of_request[r]] = predictors[r];
    std::unique_lock<std::mutex> g(m.mu);
    int rc = FWGPU_OK;
    if (!m.tp && (rc = fwgpu_text_parser_create(m.vw, m.re->device, &m.tp)) != FWGPU_OK) return rc;
    if (!m.rt_tr && (rc = record_batch_alloc(m.re, &m.tr, 1, 16, &m.rt_tr)) != FWGPU_OK) return rc;
    const DevTranslator dtr = m.rt_tr->tr;  // (made once per model and never changed)
    const uint32_t nns = text_parser_namespaces(m.tp);
    g.unlock();  // ---- the host's share of the call needs no device and holds up no other predictor of the model
    bool served = nns <= kTextMaxNamespaces && requests_text_lds_bytes(dtr) != 0;
    for (uint32_t j = 0; served && j < dtr.n_members; j++) served = m.tr.combo_ns[j] < nns;
    for (uint32_t j = 0; served && j < dtr.n_pairs; j++) served = m.tr.field_ns[j] < nns;
    for (size_t c = 0; served && c < owner.size(); c++) served = rt_piece_of(owner[c], nns);
    if (!served) return by_lines();
    // the texts back to back, each request ending in a newline
    std::string text;
    text.reserve((size_t)total_len);
    std::vector<uint32_t> t_off(n_requests + 1, 0);
    for (uint32_t r = 0; r < n_requests; r++) {
        t_off[r] = (uint32_t)text.size();
        if (!lens[r]) continue;
        text.append(texts[r], (size_t)lens[r]);
        if (text.back() != '\n') text.push_back('\n');
    }
    t_off[n_requests] = (uint32_t)text.size();
    // what the kernels read beside the parse, one upload: the requests' offsets and caches, the descriptors of the set's caches, and every cache's piece
    // (kept by its predictor since its fw_setup_cache: present keys, filter bits, the context's record, its cover bits).  An f32 cache's own device
    // copies are not used: they cover the slots up to the last FFM namespace only, where this route's rule takes every slot the context fills, and a
    // packed regressor's cache has none
    auto up8 = [](size_t x) { return (x + 7) & ~(size_t)7; };
    size_t q = 0;
    const size_t q_toff = q; q = up8(q + 4 * ((size_t)n_requests + 1));
    const size_t q_cor = q; q = up8(q + 4 * (size_t)n_requests);
    const size_t q_desc = q; q = up8(q + sizeof(RtCache) * caches.size());
    std::vector<size_t> q_piece(caches.size());
    for (size_t c = 0; c < caches.size(); c++) {
        q_piece[c] = q;
        q += 8 * owner[c]->rt_piece.size();
    }
    std::vector<uint64_t> side((q + 7) / 8, 0);
    unsigned char *sb = reinterpret_cast<unsigned char *>(side.data());
    std::memcpy(sb + q_toff, t_off.data(), 4 * t_off.size());
    std::memcpy(sb + q_cor, cache_of_request.data(), 4 * cache_of_request.size());
    for (size_t c = 0; c < caches.size(); c++) std::memcpy(sb + q_piece[c], owner[c]->rt_piece.data(), 8 * owner[c]->rt_piece.size());
    g.lock();
    for (uint32_t r = 0; r < n_requests && rc == FWGPU_OK; r++) rc = refresh_stale_cache(predictors[r]);  // (--packed_context_cache)
    if (rc != FWGPU_OK) return rc;
    if ((rc = rt_grow(&m.rt_side, &m.rt_side_bytes, q)) != FWGPU_OK) return rc;
    const unsigned char *db = static_cast<const unsigned char *>(m.rt_side);
    for (size_t c = 0; c < caches.size(); c++) {  // (the descriptors point into the device copy)
        const FfiPredictor *o = owner[c];
        const unsigned char *piece = db + q_piece[c];
        RtCache d{};
        d.present = reinterpret_cast<const uint64_t *>(piece);
        d.present_bits = reinterpret_cast<const uint64_t *>(piece + o->rt_piece_bits);
        d.ctx_rec = reinterpret_cast<const uint32_t *>(piece + o->rt_piece_rec);
        d.cover = reinterpret_cast<const uint32_t *>(piece + o->rt_piece_cover);
        d.ctx_len = (uint32_t)o->ctx_record.size();
        d.n_present = (uint32_t)(o->rt_piece_bits / 8);
        std::memcpy(sb + q_desc + sizeof(RtCache) * c, &d, sizeof(RtCache));
    }
    // ---- one plain pass of the device parser
    TextDeviceLines dl;
    if ((rc = text_lines_device(m.tp, text.data(), (uint32_t)text.size(), &dl)) != FWGPU_OK) return rc;
    const uint32_t n = dl.nlines;
    size_t w = 0;
    const size_t w_counts = w; w = up8(w + 16 * (size_t)n);
    const size_t w_of = w; w = up8(w + 4 * (size_t)n);
    const size_t w_tot = w; w = up8(w + sizeof(RtTotals) + 4 * ((size_t)n_requests + 1));
    if ((rc = rt_grow(&m.rt_scratch, &m.rt_scratch_bytes, w)) != FWGPU_OK) return rc;
    // (`side` is pageable and local: every return between this copy and the wait for the stream below waits for it first)
    auto drained = [&](int code) {
        (void)hipStreamSynchronize(dl.stream);
        return code;
    };
    if (hipMemcpyAsync(m.rt_side, sb, q, hipMemcpyHostToDevice, dl.stream) != hipSuccess)
        return drained(fail(FWGPU_ERR_DEVICE, "predict_requests_text: copy to the device failed"));
    // ---- count pass and scan; the one block the host reads
    unsigned char *wb = static_cast<unsigned char *>(m.rt_scratch);
    RtArgs a{};
    a.text = dl.text;
    a.lstart = dl.lstart;
    a.status = dl.status;
    a.records = dl.records;
    a.rec_off = dl.rec_off;
    a.nlines = n;
    a.nns = nns;
    a.t_off = reinterpret_cast<const uint32_t *>(db + q_toff);
    a.cache_of_request = reinterpret_cast<const uint32_t *>(db + q_cor);
    a.caches = reinterpret_cast<const RtCache *>(db + q_desc);
    a.n_requests = n_requests;
    a.tr = dtr;
    a.ffm_k = m.re->cfg.ffm_k;
    a.has_lr = m.re->cfg.wiring != FWGPU_WIRING_FFM_ONLY;
    a.counts = reinterpret_cast<uint4 *>(wb + w_counts);
    a.cache_of = reinterpret_cast<uint32_t *>(wb + w_of);
    a.totals = reinterpret_cast<RtTotals *>(wb + w_tot);
    a.first_line = reinterpret_cast<uint32_t *>(wb + w_tot + sizeof(RtTotals));
    std::vector<uint64_t> block((sizeof(RtTotals) + 4 * ((size_t)n_requests + 1) + 7) / 8);
    const bool timing = std::getenv("FWGPU_SERVING_TIMING") != nullptr;  // device events around the new kernels alone, to stderr (as predict_batch's laps)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    if (timing)
        for (hipEvent_t &e : ev)
            if (hipEventCreate(&e) != hipSuccess) return drained(fail(FWGPU_ERR_DEVICE, "predict_requests_text: no event"));
    struct EventsGuard {
        hipEvent_t *ev;
        ~EventsGuard() {
            for (int i = 0; i < 4; i++)
                if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
    } events_guard{ev};
    if (n) {
        hipError_t e = timing ? hipEventRecord(ev[0], dl.stream) : hipSuccess;
        if (e == hipSuccess) e = launch_requests_text_count(a, dl.stream);
        if (e == hipSuccess && timing) e = hipEventRecord(ev[1], dl.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(block.data(), a.totals, sizeof(RtTotals) + 4 * ((size_t)n_requests + 1), hipMemcpyDeviceToHost, dl.stream);
        if (e != hipSuccess) return drained(fail(FWGPU_ERR_DEVICE, std::string("predict_requests_text: count pass: ") + hipGetErrorString(e)));
    }
    FWGPU_HIP(hipStreamSynchronize(dl.stream));
    RtTotals tot{};
    std::memcpy(&tot, block.data(), sizeof(RtTotals));
    const uint32_t *first_line = reinterpret_cast<const uint32_t *>(reinterpret_cast<const unsigned char *>(block.data()) + sizeof(RtTotals));
    if (n == 0 || tot.fallback) {
        g.unlock();
        return by_lines();
    }
    bool fits = true;
    for (uint32_t r = 0; r < n_requests; r++) {
        n_lines[r] = first_line[r + 1] - first_line[r];
        fits = fits && n_lines[r] <= caps[r];
    }
    host->text_lines = n;
    if (!fits) return fail(FWGPU_ERR_RANGE, "predict_requests_text: more lines than a request's output holds");
    if (tot.max_ffm > 4096 || tot.max_lr > 4096) return fail(FWGPU_ERR_INVALID, kRequestsTooManyEntries);
    // ---- the entry batch, filled by the emit pass; the set with the index array the count pass left; the launch of fwgpu_predictor_predict_requests
    if (!m.requests || m.requests->n_cap < n || m.requests->n_lr < tot.tot_lr || m.requests->n_ffm < tot.tot_ffm) {
        if (m.requests) fwgpu_batch_free(m.requests);
        m.requests = nullptr;
        const uint32_t cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(2ull * n, 256), 0xffffffffull);
        if ((rc = batch_alloc(m.re, cap, std::max<uint64_t>(2 * tot.tot_lr, 1 << 16), std::max<uint64_t>(2 * tot.tot_ffm, 1 << 14), &m.requests)) != FWGPU_OK) return rc;
        m.requests->n_cap = cap;
    }
    fwgpu_batch *eb = m.requests;
    eb->n = n;
    eb->max_lr = tot.max_lr;
    eb->max_ffm = tot.max_ffm;
    eb->aligned4 = (dtr.ffm_mask & 3u) == 0;  // every row starts where the translator's mask puts it
    a.ffm_hash = eb->ffm_hash;
    a.ffm_val = eb->ffm_val;
    a.ffm_fld = eb->ffm_fld;
    a.ffm_off = eb->ffm_off;
    a.lr_hash = eb->lr_hash;
    a.lr_val = eb->lr_val;
    a.lr_off = eb->lr_off;
    a.lr_combo = eb->lr_combo;
    a.label = eb->label;
    a.importance = eb->importance;
    if (timing) FWGPU_HIP(hipEventRecord(ev[2], nullptr));
    FWGPU_HIP(launch_requests_text_emit(a, nullptr));  // (the parser's stream is idle: the launch's own stream from here on)
    if (timing) FWGPU_HIP(hipEventRecord(ev[3], nullptr));
    rc = batch_set_caches_device(eb, caches.data(), (uint32_t)caches.size(), a.cache_of, nullptr);
    if (rc == FWGPU_OK) rc = fwgpu_learn_batch(m.re, eb, FWGPU_MODE_HOGWILD, /*update=*/0, nullptr);
    std::vector<float> preds(n);
    if (rc == FWGPU_OK) rc = fwgpu_batch_predictions(eb, preds.data(), n, nullptr);
    if (rc != FWGPU_OK) return rc;
    if (timing) {  // (the predictions are here: every event has passed)
        float ms_count = 0.0f, ms_emit = 0.0f;
        FWGPU_HIP(hipEventElapsedTime(&ms_count, ev[0], ev[1]));
        FWGPU_HIP(hipEventElapsedTime(&ms_emit, ev[2], ev[3]));
        std::fprintf(stderr, "[predict_requests_text] %u requests, %u lines: count + scan %.4f ms, emit %.4f ms\n", n_requests, n, ms_count, ms_emit);
    }
    for (uint32_t r = 0; r < n_requests; r++)
        if (n_lines[r]) std::memcpy(out[r], preds.data() + first_line[r], 4 * (size_t)n_lines[r]);
    return FWGPU_OK;
}

// which path and kernel the model's regressor took in its last batch launch (fwgpu_debug_last_route, fwgpu_debug_last_launch): the prototype and its
// clone_lite copies share the regressor, so this is the last launch of any of them
int fwgpu_predictor_last_launch(const FfiPredictor *ptr, int *route, int32_t *launch, uint32_t n) {
    if (!ptr || !route || (n && !launch)) return fail(FWGPU_ERR_INVALID, "NULL argument");
    const int rc = fwgpu_debug_last_route(ptr->model->re, route);
    return rc != FWGPU_OK ? rc : fwgpu_debug_last_launch(ptr->model->re, launch, n);
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
