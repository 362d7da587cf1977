// ------------------------------------------------------------------ context cache (serving)
// Regressor::setup_cache / predict_with_cache (regressor.rs:397-423) with BlockFFM's cache (block_ffm.rs:442-782): the field
// sums ("contra fields") and self-pair corrections of the context's features are computed once, on the device, and every
// candidate then gathers only the rows of the features that are NOT in `features_present`.  BlockLR's cache is inert in the
// reference (prepare_forward_cache skips every feature: `hash & IS_NOT_SINGLE_MASK == 0` always holds for a masked hash,
// block_lr.rs:236-239), so LR entries are always all read, exactly like there.
// Also here: the cache sets of the requests route (fwgpu_batch_set_caches) and a packed regressor's cache switch.  The launches are launch.cpp's.
#include <string.h>

#include <algorithm>

#include "launch.h"

namespace fwgpu {

// takes the set off the batch (hipFree waits for the launches that still read the table)
void requests_detach(fwgpu_batch *b) {
    if (b->req_dev) (void)hipFree(b->req_dev);
    b->req_dev = nullptr;
    b->req_dev_bytes = 0;
    b->req_T = nullptr;
    b->req_base = nullptr;
    b->req_of = nullptr;
    b->req_of_n = 0;
    b->req_single = false;
    b->req_caches.clear();
}

// A packed regressor's caches hold sums of the weights of ONE epoch (fwgpu_packed_apply_diff and fwgpu_pack_regressor's refresh bump it): an older
// cache is refused wherever it is attached or launched with, until fwgpu_setup_cache on its handle has refilled it.
bool cache_is_stale(const fwgpu_regressor *r, const fwgpu_block_cache *c) { return r->packed() && c->epoch != r->weights_epoch; }
const char *const kStaleCache =
    "a context cache is stale: the packed regressor's weights changed after it was set up (fwgpu_packed_apply_diff, fwgpu_pack_regressor); "
    "call fwgpu_setup_cache on the same handle";

}  // namespace fwgpu

using namespace fwgpu;

extern "C" {

static int requests_attach_single(fwgpu_batch *b, const fwgpu_block_cache *c);
static uint64_t cache_key(const fwgpu_ffm_entry &e) { return ((uint64_t)e.hash << 32) | e.contra_field_index; }  // regressor.rs:25-38

int fwgpu_setup_cache(fwgpu_regressor *r, const fwgpu_lr_entry *lr, uint32_t n_lr, const fwgpu_ffm_entry *ffm,
                      uint32_t n_ffm, fwgpu_block_cache **cache) {
    if (!r || !cache) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if ((n_lr && !lr) || (n_ffm && !ffm)) return fail(FWGPU_ERR_INVALID, "NULL entry buffer");
    if (!r->packed_caches)
        if (int rcp = refuse_packed(r, "setup_cache (a device-side context cache)")) return rcp;
    FWGPU_HIP(hipSetDevice(r->device));
    const uint32_t F = r->cfg.ffm_k ? r->cfg.ffm_num_fields : 0, R = F * r->cfg.ffm_k;
    fwgpu_block_cache *c = *cache;
    if (c && c->owner != r) return fail(FWGPU_ERR_INVALID, "cache belongs to another regressor");
    if (!c) {  // should_create (regressor.rs:415-417)
        c = new fwgpu_block_cache();
        c->owner = r;
        if (hipMalloc((void **)&c->d_T, ((size_t)F * R + 2 * (size_t)F + 4) * sizeof(float)) != hipSuccess) {
            delete c;
            return fail(FWGPU_ERR_DEVICE, "setup_cache: allocation failed");
        }
        c->d_dcf = c->d_T + (size_t)F * R;
        c->d_cnt = reinterpret_cast<uint32_t *>(c->d_dcf + F);  // (features per field: what the deep head's input diagonal asks, nn_forward)
    }
    HostBatch hb;
    hb.clear();
    float pred = 0.0f;
    int rc = append_example(r, hb, lr, n_lr, ffm, n_ffm, 0.0f, 1.0f);
    if (rc == FWGPU_OK) rc = ensure_one(r, (uint32_t)hb.lr_hash.size(), (uint32_t)hb.ffm_hash.size());
    if (rc == FWGPU_OK) rc = batch_upload(r->one, hb, 0);
    if (rc == FWGPU_OK && r->packed()) {
        // packed weights: the build kernel of requests.hip in place of the example kernel's emitting launch -- the same sums in the same order
        if (!hb.aligned4)
            rc = fail(FWGPU_ERR_INVALID, "packed regressor: an FFM entry's hash is not a multiple of 4 (rows must start where the translator's mask puts them: hash & fwgpu_ffm_hash_mask)");
        if (rc == FWGPU_OK) {
            PackedCacheBuild q{};
            q.ffm_q = r->d_ffm_q;
            q.ffm_hash = r->one->ffm_hash;
            q.ffm_val = r->one->ffm_val;
            q.ffm_fld = r->one->ffm_fld;
            q.n = (uint32_t)hb.ffm_hash.size();
            q.F = F;
            q.k = r->cfg.ffm_k;
            q.R = R;
            q.q_increment = r->q_increment;
            q.q_min = r->q_min;
            q.T = c->d_T;
            q.dcf = c->d_dcf;
            q.cnt = c->d_cnt;
            hipError_t e = launch_packed_cache_build(q, 0);
            if (e == hipSuccess) e = hipStreamSynchronize(0);
            if (e != hipSuccess) rc = fail(FWGPU_ERR_DEVICE, std::string("setup_cache (packed): ") + hipGetErrorString(e));
        }
    } else if (rc == FWGPU_OK) {
        r->one->cache = nullptr;
        r->one->emit_T = c->d_T;
        r->one->emit_dcf = c->d_dcf;
        r->one->emit_cnt = c->d_cnt;  // (a refilled cache: T, dcf and the counts are all written again by this launch)
        rc = run_batch(r, r->one, FWGPU_MODE_SEQUENTIAL, 0, 0);
        r->one->emit_T = r->one->emit_dcf = nullptr;
        r->one->emit_cnt = nullptr;
    }
    if (rc == FWGPU_OK && !r->packed() && one_prediction(r, &pred) != FWGPU_OK) rc = fail(FWGPU_ERR_DEVICE, "setup_cache: launch failed");
    if (rc != FWGPU_OK) {
        if (!*cache) {
            (void)hipFree(c->d_T);
            delete c;
        }
        return rc;
    }
    c->present.clear();
    for (uint32_t i = 0; i < (r->cfg.ffm_k ? n_ffm : 0); i++) c->present.push_back(cache_key(ffm[i]));
    std::sort(c->present.begin(), c->present.end());
    c->present.erase(std::unique(c->present.begin(), c->present.end()), c->present.end());
    c->epoch = r->weights_epoch;
    *cache = c;
    return FWGPU_OK;
}

int fwgpu_block_cache_free(fwgpu_block_cache *c) {
    if (!c) return FWGPU_OK;
    if (c->d_cover) (void)hipFree(c->d_cover);
    if (c->d_T) (void)hipFree(c->d_T);
    delete c;
    return FWGPU_OK;
}

// The FFM entries forward_with_cache still gathers: those whose (hash, contra_field_index) is not in features_present
// (block_ffm.rs:548, 600).  out may alias ffm.
int fwgpu_block_cache_filter(const fwgpu_block_cache *c, const fwgpu_ffm_entry *ffm, uint32_t n_ffm, fwgpu_ffm_entry *out, uint32_t *n_out) {
    if (!c || !n_out || (n_ffm && (!ffm || !out))) return fail(FWGPU_ERR_INVALID, "NULL argument");
    uint32_t m = 0;
    for (uint32_t i = 0; i < n_ffm; i++)
        if (!std::binary_search(c->present.begin(), c->present.end(), cache_key(ffm[i]))) out[m++] = ffm[i];
    *n_out = m;
    return FWGPU_OK;
}

int fwgpu_predict_with_cache(fwgpu_regressor *r, const fwgpu_block_cache *c, const fwgpu_lr_entry *lr, uint32_t n_lr,
                             const fwgpu_ffm_entry *ffm, uint32_t n_ffm, float *prediction) {
    if (!r || !c || !prediction) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (c->owner != r) return fail(FWGPU_ERR_INVALID, "cache belongs to another regressor");
    if ((n_lr && !lr) || (n_ffm && !ffm)) return fail(FWGPU_ERR_INVALID, "NULL entry buffer");
    if (cache_is_stale(r, c)) return fail(FWGPU_ERR_INVALID, std::string("predict_with_cache: ") + kStaleCache);
    FWGPU_HIP(hipSetDevice(r->device));
    std::vector<fwgpu_ffm_entry> rest(n_ffm);
    uint32_t m = 0;
    int rc = fwgpu_block_cache_filter(c, ffm, n_ffm, rest.data(), &m);
    if (rc) return rc;
    HostBatch hb;
    hb.clear();
    rc = append_example(r, hb, lr, n_lr, rest.data(), m, 0.0f, 1.0f);
    if (rc) return rc;
    rc = ensure_one(r, (uint32_t)hb.lr_hash.size(), (uint32_t)hb.ffm_hash.size());
    if (rc) return rc;
    rc = batch_upload(r->one, hb, 0);
    if (rc) return rc;
    if (r->packed()) {  // the set of one on the requests route; the table stays allocated for the next call, the set does not stay attached
        rc = requests_attach_single(r->one, c);
        if (rc == FWGPU_OK) rc = run_batch(r, r->one, FWGPU_MODE_SEQUENTIAL, 0, 0);
        r->one->req_caches.clear();
    } else {
        r->one->cache = c;
        rc = run_batch(r, r->one, FWGPU_MODE_SEQUENTIAL, 0, 0);
        r->one->cache = nullptr;
    }
    if (rc) return rc;
    return one_prediction(r, prediction);
}

static inline uint32_t present_bit(uint64_t key) { return (uint32_t)((key * 0x9e3779b97f4a7c15ULL) >> 52); }  // 12 bits

// Record batches with a context cache.  `record` is the context's own record (what fw_setup_cache parsed): the namespace
// slots it fills are the covered ones.  A request's record (context + candidate, parser.rs:195-211) then goes to the device
// whole, and the stage phase leaves out the FFM features of covered slots -- which are exactly the features
// fwgpu_block_cache_filter drops, PROVIDED the request passes fwgpu_block_cache_record_ok.
int fwgpu_block_cache_cover_record(fwgpu_block_cache *c, const fwgpu_translator_config *t, const uint32_t *record, uint32_t len) {
    if (!c || !t || !record) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (c->owner && c->owner->packed())
        return fail(FWGPU_ERR_INVALID, "block_cache_cover_record: a packed regressor's cache serves the entry route only (an entry batch of the buffers "
                                       "fwgpu_block_cache_filter leaves, fwgpu_batch_set_cache / fwgpu_batch_set_caches); record batches with a cache are not served");
    uint32_t nl = 0, nf = 0;
    int rc = count_record(t, record, len, &nl, &nf);
    if (rc) return rc;
    uint32_t max_ns = 0;
    for (uint32_t m = 0; m < t->field_off[t->n_fields]; m++) max_ns = std::max(max_ns, t->field_ns[m]);
    const uint32_t n_slots = std::min<uint32_t>(len > 3 ? len - 3 : 0, max_ns + 1);
    const size_t cover_words = (max_ns + 32) / 32;
    FWGPU_HIP(hipSetDevice(c->owner->device));
    if (c->d_cover && (c->cover.size() != cover_words || c->ctx_rec_cap < len)) {
        // (a refilled cache keeps its allocation when the new context fits: fw_setup_cache runs once per request)
        (void)hipFree(c->d_cover);
        c->d_cover = nullptr;
    }
    if (!c->d_cover) c->ctx_rec_cap = (size_t)len * 2;
    c->cover.assign(cover_words, 0);
    c->ctx_slots.assign(record + 3, record + 3 + n_slots);
    for (uint32_t ns = 0; ns < n_slots; ns++)
        if (record[3 + ns] != 0x80000000u) c->cover[ns >> 5] |= 1u << (ns & 31);  // NO_FEATURES (parser.rs:19)
    if (!c->d_cover) FWGPU_HIP(hipMalloc((void **)&c->d_cover, (cover_words + c->ctx_rec_cap) * 4));
    c->d_ctx_rec = c->d_cover + cover_words;
    c->ctx_rec.assign(record, record + len);
    std::vector<uint32_t> up(c->cover);
    up.insert(up.end(), record, record + len);
    FWGPU_HIP(hipMemcpy(c->d_cover, up.data(), up.size() * 4, hipMemcpyHostToDevice));
    c->present_bits.assign(64, 0);
    for (uint64_t key : c->present) {
        const uint32_t b = present_bit(key);
        c->present_bits[b >> 6] |= 1ull << (b & 63);
    }
    return FWGPU_OK;
}

// 1 when leaving out the covered slots of this request's record is what fwgpu_block_cache_filter would do with its
// translation: the request has not rewritten a covered slot (a namespace named again replaces the context's features in the
// record, parser.rs:318-326, while the cache still holds them), and none of its own FFM features equals a cached one
// (hash and field: the filter would drop it).  0: take the entry route (translate, filter) for this request.
int fwgpu_block_cache_record_ok(const fwgpu_block_cache *c, const fwgpu_translator_config *t, const uint32_t *record, uint32_t len) {
    return block_cache_record_ok(c, t, record, len, false);
}

}  // extern "C"
namespace fwgpu {
// delta: `record` holds the candidate's namespaces only (a covered slot it does not touch reads NO_FEATURES there)
int block_cache_record_ok(const fwgpu_block_cache *c, const fwgpu_translator_config *t, const uint32_t *record, uint32_t len, bool delta) {
    if (!c || !t || !record || !c->d_cover) return 0;
    const uint32_t n_slots = (uint32_t)c->ctx_slots.size();
    if (len < 3 + n_slots) return 0;
    for (uint32_t ns = 0; ns < n_slots; ns++)
        if (((c->cover[ns >> 5] >> (ns & 31)) & 1u) && record[3 + ns] != (delta ? 0x80000000u : c->ctx_slots[ns])) return 0;
    const uint32_t ffm_mask = ffm_hash_mask(t->ffm_bit_precision, t->ffm_k);
    for (uint32_t f = 0; f < t->n_fields; f++)
        for (uint32_t m = t->field_off[f]; m < t->field_off[f + 1]; m++) {
            const uint32_t ns = t->field_ns[m];
            if (3 + ns >= len) return 0;
            if (ns < n_slots && ((c->cover[ns >> 5] >> (ns & 31)) & 1u)) continue;
            const uint32_t w = record[3 + ns];
            auto hit = [&](uint32_t hash) {
                const uint64_t key = ((uint64_t)(hash & ffm_mask) << 32) | (f * t->ffm_k);
                const uint32_t b = present_bit(key);
                return ((c->present_bits[b >> 6] >> (b & 63)) & 1ull) && std::binary_search(c->present.begin(), c->present.end(), key);
            };
            if (!(w & 0x80000000u)) {
                if (hit(w)) return 0;
                continue;
            }
            const uint32_t start = (w >> 16) & 0x3fff, end = w & 0xffff;
            if (end > len || end < start) return 0;
            for (uint32_t o = start; o + 1 < end; o += 2)
                if (hit(record[o])) return 0;
        }
    return 1;
}
}  // namespace fwgpu
extern "C" {

// Predict-only launches of this batch start every example's field sums from the cache (NULL detaches it): an entry batch must
// then hold only the entries fwgpu_block_cache_filter leaves; a record batch holds whole requests that pass
// fwgpu_block_cache_record_ok, and the cache must know the context's record (fwgpu_block_cache_cover_record).
int fwgpu_batch_set_cache(fwgpu_batch *b, const fwgpu_block_cache *c) {
    if (!b) return fail(FWGPU_ERR_INVALID, "NULL batch");
    if (c && c->owner != b->owner) return fail(FWGPU_ERR_INVALID, "cache belongs to another regressor");
    if (c && b->owner && b->owner->packed()) {  // (fwgpu_packed_enable_caches: a packed regressor has no other cache) the set of ONE on the requests route
        if (b->records)
            return fail(FWGPU_ERR_INVALID, "set_cache: a packed regressor serves a cache through the entry route only: a record batch with a cache is not served "
                                           "(send an entry batch of the buffers fwgpu_block_cache_filter leaves)");
        if (const char *why = requests_refusal(b->owner, b)) return fail(FWGPU_ERR_INVALID, std::string("set_cache: ") + why);
        if (cache_is_stale(b->owner, c)) return fail(FWGPU_ERR_INVALID, std::string("set_cache: ") + kStaleCache);
        return requests_attach_single(b, c);
    }
    if (c && b->records && !c->d_cover)
        return fail(FWGPU_ERR_INVALID, "a record batch needs a context cache that knows the context's record (fwgpu_block_cache_cover_record)");
    b->cache = c;
    requests_detach(b);  // (one cache for the whole batch replaces a set, as a set replaces it)
    return FWGPU_OK;
}

// A cache PER EXAMPLE: example i of the entry batch holds all LR entries of its request and the FFM entries
// fwgpu_block_cache_filter(caches[cache_of_example[i]], ...) leaves.  Predict-only launches of the batch then take the requests route
// (requests.hip: FWGPU_ROUTE_REQUESTS).  The pointer table and the index array are copied here; the caches are referenced and must
// outlive the launches (a cache refilled by fwgpu_setup_cache on the same handle is read as refilled).  n_caches == 0 detaches.
// A refused call leaves the batch as it was.
int fwgpu_batch_set_caches(fwgpu_batch *b, const fwgpu_block_cache *const *caches, uint32_t n_caches, const uint32_t *cache_of_example) {
    if (!b) return fail(FWGPU_ERR_INVALID, "NULL batch");
    if (n_caches == 0) {
        requests_detach(b);
        return FWGPU_OK;
    }
    if (!caches || (b->n && !cache_of_example)) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (!b->owner) return fail(FWGPU_ERR_INVALID, "set_caches: the batch has no regressor");
    if (const char *why = requests_refusal(b->owner, b)) return fail(FWGPU_ERR_INVALID, std::string("set_caches: ") + why);
    for (uint32_t c = 0; c < n_caches; c++) {
        if (!caches[c]) return fail(FWGPU_ERR_INVALID, "set_caches: NULL cache");
        if (caches[c]->owner != b->owner) return fail(FWGPU_ERR_INVALID, "set_caches: a cache belongs to another regressor");
        if (cache_is_stale(b->owner, caches[c])) return fail(FWGPU_ERR_INVALID, std::string("set_caches: ") + kStaleCache);
    }
    for (uint32_t i = 0; i < b->n; i++)
        if (cache_of_example[i] >= n_caches) return fail(FWGPU_ERR_INVALID, "set_caches: cache_of_example holds an index >= n_caches");
    // one allocation: d_T of every cache, d_dcf of every cache, base [n_caches] (8-byte slots), then cache_of [n]
    const size_t table = 2 * (size_t)n_caches * sizeof(float *), base = (((size_t)n_caches * sizeof(float)) + 7) & ~(size_t)7;
    std::vector<unsigned char> host(table + base + (size_t)b->n * sizeof(uint32_t), 0);
    const float **tp = reinterpret_cast<const float **>(host.data());
    for (uint32_t c = 0; c < n_caches; c++) {
        tp[c] = caches[c]->d_T;
        tp[n_caches + c] = caches[c]->d_dcf;
    }
    if (b->n) memcpy(host.data() + table + base, cache_of_example, (size_t)b->n * sizeof(uint32_t));
    FWGPU_HIP(hipSetDevice(b->owner->device));
    // (a set that fits the allocation of the one it replaces is written over it: the call must not overlap a launch of this batch that is still in
    // flight, as with every other change of a batch's contents)
    void *dev = b->req_dev_bytes >= host.size() ? b->req_dev : nullptr;
    const bool fresh = dev == nullptr;
    if (fresh && hipMalloc(&dev, host.size()) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FWGPU_ERR_OOM, "set_caches: no device memory for the cache table");
    }
    if (hipMemcpy(dev, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess) {
        if (fresh) (void)hipFree(dev);
        return fail(FWGPU_ERR_DEVICE, "set_caches: copy to the device failed");
    }
    if (fresh) {
        requests_detach(b);
        b->req_dev_bytes = host.size();
    }
    b->cache = nullptr;
    b->req_dev = dev;
    b->req_T = reinterpret_cast<const float *const *>(dev);
    b->req_base = reinterpret_cast<float *>(static_cast<unsigned char *>(dev) + table);
    b->req_of = reinterpret_cast<uint32_t *>(static_cast<unsigned char *>(dev) + table + base);
    b->req_of_n = b->n;
    b->req_single = false;
    b->req_caches.assign(caches, caches + n_caches);
    return FWGPU_OK;
}

// ONE cache for every example of an entry batch of a packed regressor: the set of one.  The table of the call before is kept where it still says the
// same (the single-example calls attach the same cache request after request).
static int requests_attach_single(fwgpu_batch *b, const fwgpu_block_cache *c) {
    if (b->req_dev && b->req_single && b->req_of_n >= b->n && b->req_single_T == c->d_T) {
        b->req_caches.assign(1, c);
        return FWGPU_OK;
    }
    const std::vector<uint32_t> zeros(std::max<uint32_t>(b->n, 1), 0u);
    const int rc = fwgpu_batch_set_caches(b, &c, 1, zeros.data());
    if (rc != FWGPU_OK) return rc;
    b->req_single = true;
    b->req_single_T = c->d_T;
    return FWGPU_OK;
}

int fwgpu_packed_enable_caches(fwgpu_regressor *r) {
    if (!r) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (!r->packed()) return fail(FWGPU_ERR_INVALID, "packed_enable_caches: the regressor's FFM weights are f32: its context caches need no switch");
    r->packed_caches = true;
    return FWGPU_OK;
}

int fwgpu_packed_caches_state(const fwgpu_regressor *r, int *enabled, uint64_t *weights_epoch) {
    if (!r) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (enabled) *enabled = r->packed_caches ? 1 : 0;
    if (weights_epoch) *weights_epoch = r->weights_epoch;
    return FWGPU_OK;
}

int fwgpu_debug_block_cache_read(const fwgpu_block_cache *c, float *T, float *dcf, uint32_t *cnt, uint64_t *epoch) {
    if (!c || !c->owner) return fail(FWGPU_ERR_INVALID, "NULL argument");
    const fwgpu_regressor *r = c->owner;
    const size_t F = r->cfg.ffm_k ? r->cfg.ffm_num_fields : 0, R = F * r->cfg.ffm_k;
    FWGPU_HIP(hipSetDevice(r->device));
    FWGPU_HIP(hipDeviceSynchronize());
    if (T && F) FWGPU_HIP(hipMemcpy(T, c->d_T, F * R * sizeof(float), hipMemcpyDeviceToHost));
    if (dcf && F) FWGPU_HIP(hipMemcpy(dcf, c->d_dcf, F * sizeof(float), hipMemcpyDeviceToHost));
    if (cnt && F) FWGPU_HIP(hipMemcpy(cnt, c->d_cnt, F * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (epoch) *epoch = c->epoch;
    return FWGPU_OK;
}

}  // extern "C"
