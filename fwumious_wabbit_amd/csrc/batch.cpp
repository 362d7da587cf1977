// Batches: the host staging of a CSR batch (HostBatch), allocation and upload of entry and record batches, the buffers of the synchronous
// micro-batch pipeline, and the C entry points that create, free and read them.  Nothing here launches an example kernel (launch.cpp).
#include <string.h>

#include <algorithm>
#include <memory>

#include "launch.h"

namespace fwgpu {

void HostBatch::clear() {
    ffm_hash.clear();
    ffm_val.clear();
    ffm_fld.clear();
    lr_hash.clear();
    lr_val.clear();
    lr_combo.clear();
    label.clear();
    importance.clear();
    ffm_off.assign(1, 0);
    lr_off.assign(1, 0);
    max_lr = max_ffm = 0;
    aligned4 = true;
}

void HostBatch::append_slice(const HostBatch &src, uint32_t e, uint32_t f0, uint32_t f1, uint32_t l0, uint32_t l1) {
    if (ffm_off.empty()) clear();
    ffm_hash.insert(ffm_hash.end(), src.ffm_hash.begin() + f0, src.ffm_hash.begin() + f1);
    ffm_val.insert(ffm_val.end(), src.ffm_val.begin() + f0, src.ffm_val.begin() + f1);
    ffm_fld.insert(ffm_fld.end(), src.ffm_fld.begin() + f0, src.ffm_fld.begin() + f1);
    lr_hash.insert(lr_hash.end(), src.lr_hash.begin() + l0, src.lr_hash.begin() + l1);
    lr_val.insert(lr_val.end(), src.lr_val.begin() + l0, src.lr_val.begin() + l1);
    lr_combo.insert(lr_combo.end(), src.lr_combo.begin() + l0, src.lr_combo.begin() + l1);
    ffm_off.push_back((uint32_t)ffm_hash.size());
    lr_off.push_back((uint32_t)lr_hash.size());
    label.push_back(src.label[e]);
    importance.push_back(src.importance[e]);
    max_ffm = std::max(max_ffm, f1 - f0);
    max_lr = std::max(max_lr, l1 - l0);
    aligned4 = aligned4 && src.aligned4;
}

int append_example(const fwgpu_regressor *r, HostBatch &hb, const fwgpu_lr_entry *lr, uint32_t n_lr,
                   const fwgpu_ffm_entry *ffm, uint32_t n_ffm, float label, float importance) {
    if (hb.ffm_off.empty()) hb.clear();
    const uint32_t k = r->cfg.ffm_k, F = r->cfg.ffm_num_fields;
    if (k == 0) n_ffm = 0;  // no FFM block: ffm_buffer is ignored
    uint32_t prev = 0;
    for (uint32_t i = 0; i < n_ffm; i++) {
        const uint32_t cfi = ffm[i].contra_field_index;
        if (cfi % k != 0 || cfi / k >= F) return fail(FWGPU_ERR_RANGE, "ffm entry: contra_field_index is not field*k of a known field");
        if (cfi < prev) return fail(FWGPU_ERR_INVALID, "ffm entries must be ordered by field (block_ffm.rs:165-183)");
        prev = cfi;
        if ((uint64_t)ffm[i].hash + (uint64_t)F * k > r->ffm_len) return fail(FWGPU_ERR_RANGE, "ffm entry: hash outside the weight table");
        if (ffm[i].hash & 3u) hb.aligned4 = false;
        hb.ffm_hash.push_back(ffm[i].hash);
        hb.ffm_val.push_back(ffm[i].value);
        hb.ffm_fld.push_back((uint8_t)(cfi / k));
    }
    if (r->cfg.wiring == FWGPU_WIRING_FFM_ONLY) n_lr = 0;
    for (uint32_t i = 0; i < n_lr; i++) {
        if (lr[i].hash >= r->lr_len) return fail(FWGPU_ERR_RANGE, "lr entry: hash outside the weight table");
        if (lr[i].combo_index >= r->cfg.num_combos) return fail(FWGPU_ERR_RANGE, "lr entry: combo_index >= num_combos");
        hb.lr_hash.push_back(lr[i].hash);
        hb.lr_val.push_back(lr[i].value);
        hb.lr_combo.push_back((uint16_t)lr[i].combo_index);
    }
    hb.ffm_off.push_back((uint32_t)hb.ffm_hash.size());
    hb.lr_off.push_back((uint32_t)hb.lr_hash.size());
    hb.label.push_back(label);
    hb.importance.push_back(importance);
    hb.max_lr = std::max(hb.max_lr, n_lr);
    hb.max_ffm = std::max(hb.max_ffm, n_ffm);
    return FWGPU_OK;
}

static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

int batch_alloc(fwgpu_regressor *r, uint32_t n, uint64_t n_lr, uint64_t n_ffm, fwgpu_batch **out, bool host_mapped) {
    std::unique_ptr<fwgpu_batch> b(new fwgpu_batch());
    b->owner = r;
    b->n = n;
    b->n_lr = n_lr;
    b->n_ffm = n_ffm;
    size_t o = 0, off[11];
    off[0] = o; o = up256(o + 4 * n_ffm);
    off[1] = o; o = up256(o + 4 * n_ffm);
    off[2] = o; o = up256(o + n_ffm);
    off[3] = o; o = up256(o + 4 * ((size_t)n + 1));
    off[4] = o; o = up256(o + 4 * n_lr);
    off[5] = o; o = up256(o + 4 * n_lr);
    off[6] = o; o = up256(o + 4 * ((size_t)n + 1));
    off[7] = o; o = up256(o + 4 * (size_t)n);
    off[8] = o; o = up256(o + 4 * (size_t)n);
    off[9] = o; o = up256(o + 4 * (size_t)n);
    off[10] = o; o = up256(o + 2 * n_lr);
    b->dev_bytes = std::max<size_t>(o, 256);
    FWGPU_HIP(hipSetDevice(r->device));
    unsigned char *base = nullptr;
    if (host_mapped) {
        // single-example batches (fwgpu_learn / fwgpu_predict / predict_with_cache): the entries live in host memory the device
        // has mapped; the kernel's stage phase reads them over PCIe and the prediction comes back the same way -- no copy calls
        FWGPU_HIP(hipHostMalloc(&b->host_block, b->dev_bytes, hipHostMallocMapped | hipHostMallocCoherent));
        void *dv = nullptr;
        FWGPU_HIP(hipHostGetDevicePointer(&dv, b->host_block, 0));
        base = static_cast<unsigned char *>(dv);
        b->host_delta = static_cast<unsigned char *>(b->host_block) - base;
        FWGPU_HIP(hipMalloc((void **)&b->work_ring, kWorkRing * sizeof(uint32_t)));
        FWGPU_HIP(hipMemset(b->work_ring, 0, kWorkRing * sizeof(uint32_t)));
        b->work = b->work_ring;
    } else {
        FWGPU_HIP(hipMalloc(&b->dev, b->dev_bytes));
        FWGPU_HIP(hipMalloc((void **)&b->work, 64));
        base = static_cast<unsigned char *>(b->dev);
    }
    b->ffm_hash = reinterpret_cast<uint32_t *>(base + off[0]);
    b->ffm_val = reinterpret_cast<float *>(base + off[1]);
    b->ffm_fld = reinterpret_cast<uint8_t *>(base + off[2]);
    b->ffm_off = reinterpret_cast<uint32_t *>(base + off[3]);
    b->lr_hash = reinterpret_cast<uint32_t *>(base + off[4]);
    b->lr_val = reinterpret_cast<float *>(base + off[5]);
    b->lr_off = reinterpret_cast<uint32_t *>(base + off[6]);
    b->label = reinterpret_cast<float *>(base + off[7]);
    b->importance = reinterpret_cast<float *>(base + off[8]);
    b->pred = reinterpret_cast<float *>(base + off[9]);
    b->lr_combo = reinterpret_cast<uint16_t *>(base + off[10]);
    *out = b.release();
    return FWGPU_OK;
}

int mapped_batch_next_counter(fwgpu_batch *b, hipStream_t stream) {
    if (!b->work_ring) return fail(FWGPU_ERR_INVALID, "not a host-mapped batch");
    if (b->work_next == kWorkRing) {  // every counter has been used once (a 1-example launch leaves 2 in its counter)
        FWGPU_HIP(hipMemsetAsync(b->work_ring, 0, kWorkRing * sizeof(uint32_t), stream));
        b->work_next = 0;
    }
    b->work = b->work_ring + b->work_next++;
    return FWGPU_OK;
}

int record_batch_alloc(fwgpu_regressor *r, const fwgpu_translator_config *t, uint32_t n_cap, uint64_t words_cap,
                       fwgpu_batch **out, bool host_mapped) {
    int rc = check_translator(r, t);
    if (rc) return rc;
    if (t->n_fields > 255) return fail(FWGPU_ERR_INVALID, "translator: more than 255 fields");
    std::unique_ptr<fwgpu_batch> b(new fwgpu_batch());
    b->owner = r;
    b->n = 0;
    b->n_cap = n_cap;
    b->words_cap = words_cap;
    FWGPU_HIP(hipSetDevice(r->device));
    size_t o = 0;
    const size_t o_rec = o; o = up256(o + 4 * words_cap);
    const size_t o_off = o; o = up256(o + 8 * ((size_t)n_cap + 1));
    const size_t o_pred = o; o = up256(o + 4 * (size_t)n_cap);
    b->dev_bytes = std::max<size_t>(o, 256);
    unsigned char *base = nullptr;
    if (host_mapped) {
        FWGPU_HIP(hipHostMalloc(&b->host_block, b->dev_bytes, hipHostMallocMapped | hipHostMallocCoherent));
        void *dv = nullptr;
        FWGPU_HIP(hipHostGetDevicePointer(&dv, b->host_block, 0));
        base = static_cast<unsigned char *>(dv);
        unsigned char *hb = static_cast<unsigned char *>(b->host_block);
        b->h_records = reinterpret_cast<uint32_t *>(hb + o_rec);
        b->h_rec_off = reinterpret_cast<uint64_t *>(hb + o_off);
        b->h_pred = reinterpret_cast<float *>(hb + o_pred);
        FWGPU_HIP(hipMalloc((void **)&b->work_ring, kWorkRing * sizeof(uint32_t)));
        FWGPU_HIP(hipMemset(b->work_ring, 0, kWorkRing * sizeof(uint32_t)));
        b->work = b->work_ring;
    } else {
        FWGPU_HIP(hipMalloc(&b->dev, b->dev_bytes));
        FWGPU_HIP(hipMalloc((void **)&b->work, 64));
        base = static_cast<unsigned char *>(b->dev);
    }
    b->records = reinterpret_cast<uint32_t *>(base + o_rec);
    b->rec_off = reinterpret_cast<uint64_t *>(base + o_off);
    b->pred = reinterpret_cast<float *>(base + o_pred);
    // translator blob: the (field, namespace) pairs are flattened in field order
    const uint32_t ncm = t->n_combos ? t->combo_off[t->n_combos] : 0;
    const uint32_t npr = (t->ffm_k && t->n_fields) ? t->field_off[t->n_fields] : 0;
    std::vector<uint8_t> pair_field(npr);
    for (uint32_t f = 0; f < t->n_fields && t->ffm_k; f++)
        for (uint32_t m = t->field_off[f]; m < t->field_off[f + 1]; m++) pair_field[m] = (uint8_t)f;
    size_t q = 0;
    const size_t q_coff = q; q = up256(q + 4 * ((size_t)t->n_combos + 1));
    const size_t q_cns = q; q = up256(q + 4 * (size_t)ncm);
    const size_t q_cf32 = q; q = up256(q + ncm);
    const size_t q_cw = q; q = up256(q + 4 * (size_t)t->n_combos);
    const size_t q_pns = q; q = up256(q + 4 * (size_t)npr);
    const size_t q_pf32 = q; q = up256(q + npr);
    const size_t q_pfld = q; q = up256(q + npr);
    std::vector<unsigned char> blob(std::max<size_t>(q, 256), 0);
    memcpy(blob.data() + q_coff, t->combo_off, 4 * ((size_t)t->n_combos + 1));
    if (ncm) {
        memcpy(blob.data() + q_cns, t->combo_ns, 4 * (size_t)ncm);
        memcpy(blob.data() + q_cf32, t->combo_ns_f32, ncm);
    }
    if (t->n_combos) memcpy(blob.data() + q_cw, t->combo_weight, 4 * (size_t)t->n_combos);
    if (npr) {
        memcpy(blob.data() + q_pns, t->field_ns, 4 * (size_t)npr);
        memcpy(blob.data() + q_pf32, t->field_ns_f32, npr);
        memcpy(blob.data() + q_pfld, pair_field.data(), npr);
    }
    FWGPU_HIP(hipMalloc(&b->tr_dev, blob.size()));
    FWGPU_HIP(hipMemcpy(b->tr_dev, blob.data(), blob.size(), hipMemcpyHostToDevice));
    unsigned char *tb = static_cast<unsigned char *>(b->tr_dev);
    b->tr.combo_off = reinterpret_cast<const uint32_t *>(tb + q_coff);
    b->tr.combo_ns = reinterpret_cast<const uint32_t *>(tb + q_cns);
    b->tr.combo_f32 = reinterpret_cast<const uint8_t *>(tb + q_cf32);
    b->tr.combo_w = reinterpret_cast<const float *>(tb + q_cw);
    b->tr.pair_ns = reinterpret_cast<const uint32_t *>(tb + q_pns);
    b->tr.pair_f32 = reinterpret_cast<const uint8_t *>(tb + q_pf32);
    b->tr.pair_field = reinterpret_cast<const uint8_t *>(tb + q_pfld);
    b->tr.n_combos = t->n_combos;
    b->tr.n_pairs = npr;
    b->tr.n_members = ncm;
    b->tr.add_const = t->add_constant_feature ? 1 : 0;
    b->tr.lr_mask = r->lr_hash_mask;
    b->tr.ffm_mask = r->ffm_hash_mask;
    *out = b.release();
    return FWGPU_OK;
}

int count_records(const fwgpu_translator_config *t, const uint32_t *records, const uint64_t *rec_off, uint32_t n,
                  RecordStats *st) {
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t len = (uint32_t)(rec_off[i + 1] - rec_off[i]);
        uint32_t nl, nf;
        int rc = count_record(t, records + rec_off[i], len, &nl, &nf);
        if (rc) return rc;
        st->max_lr = std::max(st->max_lr, nl);
        st->max_ffm = std::max(st->max_ffm, nf);
        st->max_rec = std::max(st->max_rec, len);
        st->tot_lr += nl;
        st->tot_ffm += nf;
    }
    return FWGPU_OK;
}

int record_batch_upload(fwgpu_batch *b, const fwgpu_translator_config *t, const uint32_t *records, const uint64_t *rec_off,
                        uint32_t n, hipStream_t stream, const RecordStats *stats) {
    if (!b->records) return fail(FWGPU_ERR_INVALID, "not a record batch");
    const uint64_t words = n ? rec_off[n] - rec_off[0] : 0;
    if (n > b->n_cap || words > b->words_cap) return fail(FWGPU_ERR_RANGE, "record batch larger than its allocation");
    // validate + count on the host (slot words only, no hashing): sizes the kernel's LDS arrays
    RecordStats st;
    if (stats) {
        st = *stats;
    } else {
        int rc = count_records(t, records, rec_off, n, &st);
        if (rc) return rc;
    }
    const uint32_t max_lr = st.max_lr, max_ffm = st.max_ffm, max_rec = st.max_rec;
    const uint64_t tot_lr = st.tot_lr, tot_ffm = st.tot_ffm;
    if (n) {
        FWGPU_HIP(hipMemcpyAsync(b->records, records + rec_off[0], words * 4, hipMemcpyHostToDevice, stream));
        if (rec_off[0] == 0) {
            FWGPU_HIP(hipMemcpyAsync(b->rec_off, rec_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, stream));
        } else {
            std::vector<uint64_t> rel((size_t)n + 1);
            for (uint32_t i = 0; i <= n; i++) rel[i] = rec_off[i] - rec_off[0];
            FWGPU_HIP(hipMemcpyAsync(b->rec_off, rel.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, stream));
            FWGPU_HIP(hipStreamSynchronize(stream));
        }
    }
    b->n = n;
    b->n_lr = tot_lr;
    b->n_ffm = tot_ffm;
    b->n_words = words;
    b->max_lr = b->owner->cfg.wiring == FWGPU_WIRING_FFM_ONLY ? 0 : max_lr;
    b->max_ffm = max_ffm;
    b->max_rec = max_rec;
    b->aligned4 = true;  // hash & ffm_mask clears the low log2(next_pow2(k)) bits (feature_buffer.rs:141-148)
    return FWGPU_OK;
}

int batch_upload(fwgpu_batch *b, const HostBatch &hb, hipStream_t stream) {
    const uint32_t n = hb.size();
    if (n > b->n || hb.ffm_hash.size() > b->n_ffm || hb.lr_hash.size() > b->n_lr)
        return fail(FWGPU_ERR_RANGE, "batch_upload: host batch larger than the device allocation");
#define UP(dst, vec)                                                                                              \
    if (!(vec).empty()) {                                                                                         \
        if (b->host_block)                                                                                        \
            memcpy(reinterpret_cast<unsigned char *>(dst) + b->host_delta, (vec).data(), (vec).size() * sizeof((vec)[0])); \
        else                                                                                                      \
            FWGPU_HIP(hipMemcpyAsync((dst), (vec).data(), (vec).size() * sizeof((vec)[0]), hipMemcpyHostToDevice, stream)); \
    }
    UP(b->ffm_hash, hb.ffm_hash);
    UP(b->ffm_val, hb.ffm_val);
    UP(b->ffm_fld, hb.ffm_fld);
    UP(b->ffm_off, hb.ffm_off);
    UP(b->lr_hash, hb.lr_hash);
    UP(b->lr_val, hb.lr_val);
    UP(b->lr_combo, hb.lr_combo);
    UP(b->lr_off, hb.lr_off);
    UP(b->label, hb.label);
    UP(b->importance, hb.importance);
#undef UP
    b->max_lr = hb.max_lr;
    b->max_ffm = hb.max_ffm;
    b->aligned4 = hb.aligned4;
    return FWGPU_OK;
}

}  // namespace fwgpu

using namespace fwgpu;

extern "C" {

// ------------------------------------------------------------------ batches

int fwgpu_batch_create(fwgpu_regressor *r, const fwgpu_lr_entry *lr, const uint32_t *lr_off, const fwgpu_ffm_entry *ffm,
                       const uint32_t *ffm_off, const float *label, const float *importance, uint32_t n,
                       fwgpu_batch **out) {
    if (!r || !out || !lr_off || !ffm_off || (n && (!label || !importance)))
        return fail(FWGPU_ERR_INVALID, "fwgpu_batch_create: NULL argument");
    *out = nullptr;
    HostBatch hb;
    hb.clear();
    for (uint32_t i = 0; i < n; i++) {
        if (lr_off[i + 1] < lr_off[i] || ffm_off[i + 1] < ffm_off[i]) return fail(FWGPU_ERR_INVALID, "offsets must be non-decreasing");
        int rc = append_example(r, hb, lr ? lr + lr_off[i] : nullptr, lr_off[i + 1] - lr_off[i],
                                ffm ? ffm + ffm_off[i] : nullptr, ffm_off[i + 1] - ffm_off[i], label[i], importance[i]);
        if (rc) return rc;
    }
    fwgpu_batch *b = nullptr;
    int rc = batch_alloc(r, n, hb.lr_hash.size(), hb.ffm_hash.size(), &b);
    if (rc) return rc;
    rc = batch_upload(b, hb, 0);
    if (rc == FWGPU_OK && hipStreamSynchronize(0) != hipSuccess) rc = fail(FWGPU_ERR_DEVICE, "upload failed");
    if (rc) {
        fwgpu_batch_free(b);
        return rc;
    }
    keep_host_copy_if_oversize(b, std::move(hb));
    *out = b;
    return FWGPU_OK;
}

int fwgpu_record_batch_create(fwgpu_regressor *r, const fwgpu_translator_config *t, const uint32_t *records,
                              const uint64_t *rec_off, uint32_t n, fwgpu_batch **out) {
    if (!r || !t || !out || (n && (!records || !rec_off))) return fail(FWGPU_ERR_INVALID, "NULL argument");
    *out = nullptr;
    fwgpu_batch *b = nullptr;
    const uint64_t words = n ? rec_off[n] - rec_off[0] : 0;
    int rc = record_batch_alloc(r, t, std::max<uint32_t>(n, 1), std::max<uint64_t>(words, 1), &b);
    if (rc) return rc;
    rc = record_batch_upload(b, t, records, rec_off, n, 0);
    if (rc == FWGPU_OK && hipStreamSynchronize(0) != hipSuccess) rc = fail(FWGPU_ERR_DEVICE, "upload failed");
    if (rc == FWGPU_OK) rc = record_batch_host_copy_if_oversize(r, t, b, records, rec_off, n);
    if (rc) {
        fwgpu_batch_free(b);
        return rc;
    }
    *out = b;
    return FWGPU_OK;
}

int fwgpu_batch_free(fwgpu_batch *b) {
    if (!b) return FWGPU_OK;
    requests_detach(b);
    if (b->dev) (void)hipFree(b->dev);
    if (b->tr_dev) (void)hipFree(b->tr_dev);
    if (b->host_block) (void)hipHostFree(b->host_block);
    if (b->work_ring)
        (void)hipFree(b->work_ring);
    else if (b->work)
        (void)hipFree(b->work);
    delete b;
    return FWGPU_OK;
}

int fwgpu_batch_size(const fwgpu_batch *b, uint32_t *n, uint64_t *n_lr, uint64_t *n_ffm) {
    if (!b) return fail(FWGPU_ERR_INVALID, "NULL batch");
    if (n) *n = b->n;
    if (n_lr) *n_lr = b->n_lr;
    if (n_ffm) *n_ffm = b->n_ffm;
    return FWGPU_OK;
}

int fwgpu_batch_predictions(fwgpu_batch *b, float *host_out, uint32_t n, void *stream) {
    if (!b) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (n > b->n) return fail(FWGPU_ERR_RANGE, "n > batch size");
    if (n == 0) return FWGPU_OK;
    if (!host_out) return fail(FWGPU_ERR_INVALID, "NULL argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    FWGPU_HIP(hipMemcpyAsync(host_out, b->pred, n * sizeof(float), hipMemcpyDeviceToHost, s));
    FWGPU_HIP(hipStreamSynchronize(s));
    return FWGPU_OK;
}

int fwgpu_batch_predictions_device(fwgpu_batch *b, void **dev_ptr) {
    if (!b || !dev_ptr) return fail(FWGPU_ERR_INVALID, "NULL argument");
    *dev_ptr = b->pred;
    return FWGPU_OK;
}

// ------------------------------------------------------------------ synchronous micro-batch ("split") pipeline
// FWD (gather -> split records) -> MID (records -> prediction + general gradient) -> UPD (AdaGrad from the records): every
// example of the batch sees the weights of the batch start, like the examples in flight at once in hogwild.rs, but with a
// defined staleness (the batch).  It is what the owner-sharded multi-GPU mode (dist.cpp) and the mini-batched deep head
// (head.hip) are built from; on one GPU fwgpu_learn_batch_sync runs the three steps back to back.

int fwgpu_split_create(fwgpu_regressor *r, uint32_t n_examples, uint32_t max_ffm_per_example, fwgpu_split **out) {
    if (!r || !out || !n_examples) return fail(FWGPU_ERR_INVALID, "split_create: bad argument");
    FWGPU_HIP(hipSetDevice(r->device));
    std::unique_ptr<fwgpu_split> sp(new fwgpu_split());
    sp->owner = r;
    sp->n_cap = n_examples;
    const uint32_t F = r->cfg.ffm_k ? r->cfg.ffm_num_fields : 0, R = F * r->cfg.ffm_k;
    sp->nlr = r->nn.n_layers ? r->cfg.num_combos : 1;
    sp->split_len = split_record_len(F, R, sp->nlr);
    sp->selfw_stride = (std::max<uint32_t>(4, (max_ffm_per_example + 3) & ~3u)) * std::max<uint32_t>(1, r->cfg.ffm_k);
    const uint32_t X = r->nn.n_layers ? r->nn.X : 0;
    const size_t bytes[5] = {(size_t)n_examples * sp->split_len * 4, (size_t)n_examples * sp->selfw_stride * 4,
                             (size_t)n_examples * 2 * 4 + 64, (size_t)n_examples * X * 4, (size_t)n_examples * X * 4};
    float **ptrs[5] = {&sp->d_split, &sp->d_selfw, &sp->d_g, &sp->d_x, &sp->d_dx};
    for (int i = 0; i < 5; i++) {
        if (!bytes[i]) continue;
        if (hipMalloc((void **)ptrs[i], bytes[i]) != hipSuccess) {
            fwgpu_split_free(sp.release());
            return fail(FWGPU_ERR_DEVICE, "split_create: allocation failed");
        }
    }
    *out = sp.release();
    return FWGPU_OK;
}

int fwgpu_split_free(fwgpu_split *sp) {
    if (!sp) return FWGPU_OK;
    for (float *q : {sp->d_split, sp->d_selfw, sp->d_g, sp->d_x, sp->d_dx})
        if (q) (void)hipFree(q);
    delete sp;
    return FWGPU_OK;
}

}  // extern "C"
