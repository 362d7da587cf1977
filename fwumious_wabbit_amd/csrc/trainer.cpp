// HogwildTrainer replacement (hogwild.rs:13-103).  Records are copied as they are into a host staging buffer,
// shipped to HBM in micro-batches and translated + learned on the device (the stage phase of the example kernel is
// FeatureBufferTranslator::translate).  Two staging/device buffers alternate so that filling and uploading
// micro-batch i+1 overlaps the kernel of micro-batch i.  The host only validates slot words (count_record).
// fwgpu_trainer_digest_text_device feeds the same two slots from the device parser's buffers instead (launch_text_piece).
#include <string.h>

#include <string>

#include <algorithm>
#include <deque>
#include <memory>
#include <chrono>
#include <thread>

#include "fwgpu_internal.h"
#include "textparse.h"

using namespace fwgpu;

struct fwgpu_trainer {
    fwgpu_regressor *r = nullptr;
    uint32_t micro_batch = 0;
    // deep copy of the translator description (the caller's arrays are only borrowed for the create call)
    std::vector<uint32_t> combo_off, combo_ns, field_off, field_ns;
    std::vector<uint8_t> combo_f32, field_f32;
    std::vector<float> combo_weight;
    fwgpu_translator_config t{};
    // raw record words of the micro-batch being filled, in PINNED host memory (H2D at PCIe rate, truly asynchronous)
    uint32_t *rec[2] = {nullptr, nullptr};
    uint64_t rec_used[2] = {0, 0}, rec_cap[2] = {0, 0};
    std::vector<uint64_t> off[2];   // [n+1] word offsets
    RecordStats stats[2];           // accumulated while the records are copied in
    unsigned host_threads = 1;
    fwgpu_batch *dev[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};
    hipEvent_t uploaded[2] = {nullptr, nullptr};  // micro-batch c's records are in device buffer c (copy stream -> compute stream)
    hipStream_t copy_stream = nullptr;            // uploads run here, next to the previous micro-batch's kernel on `stream`
    bool in_flight[2] = {false, false};
    int cur = 0;
    hipStream_t stream = nullptr;
    uint64_t seen = 0;
    // hold-out / test-only protocol (main.rs:184-185, 238-241): examples numbered >= holdout_after (from 1) are predicted,
    // never learned; their predictions are kept in stream order
    uint64_t holdout_after = 0;
    bool testonly = false;
    bool slot_predict[2] = {false, false};
    uint32_t slot_n[2] = {0, 0};
    float *pred_host[2] = {nullptr, nullptr};  // pinned
    uint32_t pred_cap[2] = {0, 0};
    std::vector<float> preds;
    // chunk buffers of fwgpu_trainer_digest_cache
    std::unique_ptr<uint32_t[]> cache_words[2];
    std::unique_ptr<uint64_t[]> cache_off[2];
    uint64_t cache_off_cap = 0;
    // host threads kept between calls: staging copies of fwgpu_digest_records, parser threads of
    // fwgpu_trainer_digest_text.  Two pools: a chunk of text is parsed while the previous chunk's records are digested.
    Workers copy_pool, parse_pool;
    // device text route: the launch windows of the piece in slot c (views of the parser's buffers), and the batch that owns the translator's device arrays
    std::vector<std::unique_ptr<fwgpu_batch>> views[2];
    fwgpu_batch *text_tr = nullptr;
    // progressive / hold-out loss (fwgpu_trainer_set_metrics; metrics.hip): window 0 = off, nothing below is touched
    MetricsTable metrics;
    // delayed protocol (fwgpu_trainer_set_delay; main.rs:248-258): delay 0 = off, nothing below is touched.  A launch window's record batch stays in
    // device memory between its predict launch and its learn launch: `pending` in stream order, learned ones in `spare` for the next windows.
    struct RingBatch {
        fwgpu_batch *b = nullptr;
        hipEvent_t learned = nullptr;  // the batch's learn launch has run: it may be refilled
        uint64_t last = 0;             // stream number of the window's last example
        uint32_t n = 0;
    };
    uint64_t delay = 0, predictions_after = 0;
    std::deque<RingBatch> pending, spare;
    uint64_t learned_through = 0, pending_examples = 0, ring_bytes = 0;
};

// The delayed protocol's eligibility rule, the one copy of it: once the window that ends at example `taken_last` has been taken, a pending window that
// ends at `pending_last` is learned iff pending_last <= taken_last - delay.
static bool delay_eligible(uint64_t pending_last, uint64_t taken_last, uint64_t delay) {
    return taken_last >= delay && pending_last <= taken_last - delay;
}

static bool predict_mode(const fwgpu_trainer *tr) {  // for the NEXT example (number seen + 1)
    return tr->testonly || (tr->holdout_after && tr->seen + 1 >= tr->holdout_after);
}

// waits for slot c's launch and, if it was a predict-only one, appends its predictions (slots retire in launch order)
static int retire(fwgpu_trainer *tr, int c) {
    if (!tr->in_flight[c]) return FWGPU_OK;
    FWGPU_HIP(hipEventSynchronize(tr->done[c]));
    tr->in_flight[c] = false;
    if (tr->slot_predict[c]) tr->preds.insert(tr->preds.end(), tr->pred_host[c], tr->pred_host[c] + tr->slot_n[c]);
    tr->slot_predict[c] = false;
    return FWGPU_OK;
}

// With metrics on, the launch of `b` that is on the compute stream is followed by the metrics kernel there: the batch's predictions against the batch's own
// labels, the launch's first example being number `first_number` of the stream.  Every route leaves a prediction per example, learned or not: the example
// kernels store it before the update phase, the batched head predict writes the batch's, and the example-by-example walk copies its own into b->pred.
static int score_launch(fwgpu_trainer *tr, const fwgpu_batch *b, uint64_t first_number, bool learned) {
    if (!tr->metrics.window || !b->n) return FWGPU_OK;
    MetricsLaunch a;
    metrics_from_batch(b, 0, b->n, &a);
    a.first_number = first_number;
    a.learned_all = learned ? 1 : 0;
    return tr->metrics.score(a, tr->stream);
}

// first half of a host-fed launch: the records staged for slot c go into its device buffer (copy stream -> compute stream)
static int stage_slot(fwgpu_trainer *tr, int c, uint32_t n) {
    fwgpu_regressor *r = tr->r;
    // device buffer c may still be read by its previous kernel
    int rrc = retire(tr, c);
    if (rrc) return rrc;
    const uint64_t words = tr->rec_used[c];
    fwgpu_batch *b = tr->dev[c];
    if (!b || b->n_cap < n || b->words_cap < words) {
        if (b) fwgpu_batch_free(b);
        tr->dev[c] = nullptr;
        int rc = record_batch_alloc(r, &tr->t, std::max(n, tr->micro_batch), words * 3 / 2 + 4096, &tr->dev[c]);
        if (rc) return rc;
        b = tr->dev[c];
    }
    // The upload goes down its own stream: it overlaps the kernel of the previous micro-batch (other device buffer), and the
    // compute stream only waits for THIS buffer's copy (one stream for both cost the copy's 0.6 ms per 16 384 examples: 4.0 -> 4.6 M ex/s).
    int rc = record_batch_upload(b, &tr->t, tr->rec[c], tr->off[c].data(), n, tr->copy_stream, &tr->stats[c]);
    if (rc) return rc;
    // (a record that translates to more entries than a workgroup stages: the micro-batch is walked example by example, launch.cpp learn_one_chunked)
    if ((rc = record_batch_host_copy_if_oversize(r, &tr->t, b, tr->rec[c], tr->off[c].data(), n))) return rc;
    FWGPU_HIP(hipEventRecord(tr->uploaded[c], tr->copy_stream));
    FWGPU_HIP(hipStreamWaitEvent(tr->stream, tr->uploaded[c], 0));
    return FWGPU_OK;
}

// second half, shared by the host-fed and the device text route: slot c's launches are on the compute stream; the predictions of its n_pred
// examples that were not learned (d_pred, NULL: none) come back with them, the slot's event closes it and the other slot is the current one
// slot c's pinned prediction buffer holds n_pred floats (the slot is retired: nothing in flight writes the old one)
static int reserve_pred_host(fwgpu_trainer *tr, int c, uint32_t n_pred) {
    if (tr->pred_cap[c] >= n_pred) return FWGPU_OK;
    if (tr->pred_host[c]) (void)hipHostFree(tr->pred_host[c]);
    tr->pred_host[c] = nullptr;
    tr->pred_cap[c] = 0;
    FWGPU_HIP(hipHostMalloc((void **)&tr->pred_host[c], (size_t)std::max(n_pred, tr->micro_batch) * 4, hipHostMallocDefault));
    tr->pred_cap[c] = std::max(n_pred, tr->micro_batch);
    return FWGPU_OK;
}

// (`gathered`: the caller's launches have already left the n_pred predictions in the slot's pinned buffer, window by window)
static int close_slot(fwgpu_trainer *tr, int c, const float *d_pred, uint32_t n_pred, bool gathered = false) {
    if (gathered) d_pred = nullptr;
    if (d_pred && n_pred) {
        int rc = reserve_pred_host(tr, c, n_pred);
        if (rc) return rc;
        FWGPU_HIP(hipMemcpyAsync(tr->pred_host[c], d_pred, (size_t)n_pred * 4, hipMemcpyDeviceToHost, tr->stream));
    }
    tr->slot_predict[c] = (d_pred || gathered) && n_pred;
    tr->slot_n[c] = n_pred;
    FWGPU_HIP(hipEventRecord(tr->done[c], tr->stream));
    tr->in_flight[c] = true;
    tr->cur = c ^ 1;
    return FWGPU_OK;
}

// Staging buffer c stays untouched until its copies and kernel are done; the other buffer, now the current one, may be
// refilled once ITS previous micro-batch has completed.
static int open_slot(fwgpu_trainer *tr) {
    const int c2 = tr->cur;
    int rrc = retire(tr, c2);
    if (rrc) return rrc;
    tr->rec_used[c2] = 0;
    tr->off[c2].assign(1, 0);
    tr->stats[c2] = RecordStats();
    return FWGPU_OK;
}

// ---- delayed protocol: the ring of record batches between a window's predict launch and its learn launch
// A batch for a window of n examples / `words` record words: a learned batch that is large enough (its learn launch waited for: long past in steady
// state), else a new allocation; a learned batch that is too small makes room for it.  No allocation once the ring has reached its size.
static int ring_take(fwgpu_trainer *tr, uint32_t n, uint64_t words, fwgpu_trainer::RingBatch *out) {
    for (auto it = tr->spare.begin(); it != tr->spare.end(); ++it) {
        if (it->b->n_cap < n || it->b->words_cap < words) continue;
        *out = *it;
        tr->spare.erase(it);
        FWGPU_HIP(hipEventSynchronize(out->learned));
        return FWGPU_OK;
    }
    if (!tr->spare.empty()) {  // (none fits: the oldest one goes; hipFree waits for the device)
        tr->ring_bytes -= tr->spare.front().b->dev_bytes;
        fwgpu_batch_free(tr->spare.front().b);
        (void)hipEventDestroy(tr->spare.front().learned);
        tr->spare.pop_front();
    }
    fwgpu_trainer::RingBatch rb;
    const uint32_t n_cap = std::max(n, tr->micro_batch);
    const uint64_t words_cap = words * 3 / 2 + 4096;
    int rc = record_batch_alloc(tr->r, &tr->t, n_cap, words_cap, &rb.b);
    if (rc == FWGPU_OK && hipEventCreateWithFlags(&rb.learned, hipEventDisableTiming) != hipSuccess) {
        fwgpu_batch_free(rb.b);
        rc = fail(FWGPU_ERR_DEVICE, "hipEventCreateWithFlags");
    }
    if (rc) {
        (void)hipGetLastError();
        const std::string why = fwgpu_last_error();
        return fail(FWGPU_ERR_DEVICE, "prediction_model_delay: no device memory for a window of " + std::to_string(n_cap) + " examples / " +
                                          std::to_string(words_cap) + " record words; the ring holds " + std::to_string(tr->ring_bytes) + " bytes, " +
                                          std::to_string(tr->pending.size()) + " windows (" + std::to_string(tr->pending_examples) + " examples) pending (" + why + ")");
    }
    tr->ring_bytes += rb.b->dev_bytes;
    *out = rb;
    return FWGPU_OK;
}

// the window in `rb` (records in place, on the compute stream) ends at stream number `last`: its predict-only launch if its examples are predicted,
// scored as examples that will be learned; then it is pending
static int ring_predict_and_keep(fwgpu_trainer *tr, fwgpu_trainer::RingBatch rb, uint64_t last, bool predicted) {
    rb.n = rb.b->n;
    rb.last = last;
    tr->pending.push_back(rb);  // (first: whatever fails below, the batch is the ring's)
    tr->pending_examples += rb.n;
    if (!predicted) return FWGPU_OK;
    int rc = fwgpu_learn_batch(tr->r, rb.b, FWGPU_MODE_HOGWILD, 0, tr->stream);
    if (rc) return rc;
    return score_launch(tr, rb.b, last - rb.n + 1, true);
}

// every pending window that the window ending at `taken_last` makes eligible is learned, oldest first (not scored: an example counts once)
static int ring_learn_eligible(fwgpu_trainer *tr, uint64_t taken_last) {
    while (!tr->pending.empty() && delay_eligible(tr->pending.front().last, taken_last, tr->delay)) {
        fwgpu_trainer::RingBatch rb = tr->pending.front();
        int rc = fwgpu_learn_batch(tr->r, rb.b, FWGPU_MODE_HOGWILD, 1, tr->stream);
        if (rc) return rc;
        FWGPU_HIP(hipEventRecord(rb.learned, tr->stream));
        tr->pending.pop_front();
        tr->pending_examples -= rb.n;
        tr->learned_through = rb.last;
        tr->spare.push_back(rb);
    }
    return FWGPU_OK;
}

// flush in the delayed protocol: the staged window goes up into a ring batch, is predicted there and stays; then the windows it makes eligible are learned
static int flush_delayed(fwgpu_trainer *tr) {
    const int c = tr->cur;
    const uint32_t n = (uint32_t)(tr->off[c].size() - 1);
    fwgpu_regressor *r = tr->r;
    FWGPU_HIP(hipSetDevice(r->device));
    int rc = retire(tr, c);  // (the slot's pinned prediction buffer)
    if (rc) return rc;
    fwgpu_trainer::RingBatch rb;
    if ((rc = ring_take(tr, n, tr->rec_used[c], &rb))) {  // the window is dropped: the trainer stays usable for fwgpu_finish / fwgpu_trainer_free
        tr->seen -= n;
        tr->rec_used[c] = 0;
        tr->off[c].assign(1, 0);
        tr->stats[c] = RecordStats();
        return rc;
    }
    const uint64_t last = tr->seen;  // (`seen` already counts the staged examples)
    const bool predicted = last - n + 1 > tr->predictions_after;
    rc = record_batch_upload(rb.b, &tr->t, tr->rec[c], tr->off[c].data(), n, tr->copy_stream, &tr->stats[c]);
    // an oversize example's host copy stays with its batch: both visits take the chunked route
    if (rc == FWGPU_OK) rc = record_batch_host_copy_if_oversize(r, &tr->t, rb.b, tr->rec[c], tr->off[c].data(), n);
    if (rc == FWGPU_OK && hipEventRecord(tr->uploaded[c], tr->copy_stream) != hipSuccess) rc = fail(FWGPU_ERR_DEVICE, "hipEventRecord");
    if (rc == FWGPU_OK && hipStreamWaitEvent(tr->stream, tr->uploaded[c], 0) != hipSuccess) rc = fail(FWGPU_ERR_DEVICE, "hipStreamWaitEvent");
    if (rc) {  // (nothing reads the batch: it is a spare one again)
        (void)hipStreamSynchronize(tr->copy_stream);
        (void)hipEventRecord(rb.learned, tr->stream);
        tr->spare.push_back(rb);
        return rc;
    }
    if ((rc = ring_predict_and_keep(tr, rb, last, predicted))) return rc;
    // the staging buffer and the predictions close with the predict launch; the learn launches read ring batches only
    if ((rc = close_slot(tr, c, predicted ? rb.b->pred : nullptr, n))) return rc;
    if ((rc = ring_learn_eligible(tr, last))) return rc;
    return open_slot(tr);
}

static int flush(fwgpu_trainer *tr, bool predict = false) {
    const int c = tr->cur;
    const uint32_t n = (uint32_t)(tr->off[c].size() - 1);
    if (n == 0) return FWGPU_OK;
    if (tr->delay) return flush_delayed(tr);
    fwgpu_regressor *r = tr->r;
    FWGPU_HIP(hipSetDevice(r->device));
    int rc = stage_slot(tr, c, n);
    if (rc) return rc;
    fwgpu_batch *b = tr->dev[c];
    rc = fwgpu_learn_batch(r, b, FWGPU_MODE_HOGWILD, predict ? 0 : 1, tr->stream);
    if (rc) return rc;
    if ((rc = score_launch(tr, b, tr->seen - n + 1, !predict))) return rc;  // (`seen` already counts the staged examples)
    if ((rc = close_slot(tr, c, predict ? b->pred : nullptr, n))) return rc;
    return open_slot(tr);
}

// ---- device text route: a piece the parser has planned and placed (text_parser.cpp text_train_piece) is launched window by window from the
// parser's buffers.  A window is a non-owning record batch: rec_off + first into the piece's offsets, its own predictions and work counter.
static int launch_text_piece(fwgpu_trainer *tr, fwgpu_text_parser *tp, int c, const TextTrainPiece &P) {
    fwgpu_regressor *r = tr->r;
    if (!tr->text_tr) {  // (owns the translator's device arrays every window points at)
        int rc = record_batch_alloc(r, &tr->t, 1, 1, &tr->text_tr);
        if (rc) return rc;
    }
    // the launches wait for the parser's stream, not the host
    FWGPU_HIP(hipEventRecord(tr->uploaded[c], text_train_stream(tp)));
    FWGPU_HIP(hipStreamWaitEvent(tr->stream, tr->uploaded[c], 0));
    std::vector<std::unique_ptr<fwgpu_batch>> &views = tr->views[c];
    while (views.size() < P.n_windows) views.emplace_back(new fwgpu_batch());
    TextPlanShape shape;
    shape.n_learn = P.n_learn;
    shape.n_windows_learn = P.n_windows_learn;
    shape.n_windows = P.n_windows;
    for (uint32_t w = 0; w < P.n_windows; w++) {
        const uint64_t *st = P.win_stats + (size_t)kTextPlanStats * w;
        uint32_t first, end;
        shape.window(w, tr->micro_batch, P.n_take, &first, &end);
        if (st[0] != end - first) return fail(FWGPU_ERR_DEVICE, "training from text: the plan's windows are not the host's");
        fwgpu_batch *b = views[w].get();
        b->owner = r;
        b->n = b->n_cap = end - first;
        b->n_lr = st[5];
        b->n_ffm = st[6];
        b->n_words = b->words_cap = st[1];
        b->max_lr = r->cfg.wiring == FWGPU_WIRING_FFM_ONLY ? 0 : (uint32_t)st[2];  // as record_batch_upload leaves a batch
        b->max_ffm = (uint32_t)st[3];
        b->max_rec = (uint32_t)st[4];
        b->aligned4 = true;
        b->records = P.d_records;
        b->rec_off = P.d_rec_off + first;
        b->pred = P.d_pred + first;
        b->work = P.d_work + (size_t)kTextTrainWorkStride * w;
        b->tr = tr->text_tr->tr;
        b->host_copy.reset();
        if (record_batch_is_oversize(b)) {  // the walk of fwgpu_digest_records, from this launch's records alone
            std::vector<uint64_t> off((size_t)b->n + 1);
            std::vector<uint32_t> words((size_t)st[1]);
            int rc = text_train_wait(tp);
            if (rc) return rc;
            FWGPU_HIP(hipMemcpy(off.data(), b->rec_off, 8 * off.size(), hipMemcpyDeviceToHost));
            const uint64_t w0 = off[0];
            if (off.back() - w0 != st[1]) return fail(FWGPU_ERR_DEVICE, "training from text: a window's offsets and its word count differ");
            if (!words.empty()) FWGPU_HIP(hipMemcpy(words.data(), b->records + w0, 4 * words.size(), hipMemcpyDeviceToHost));
            for (uint64_t &o : off) o -= w0;
            if ((rc = record_batch_host_copy_if_oversize(r, &tr->t, b, words.data(), off.data(), b->n))) return rc;
        }
        int rc = fwgpu_learn_batch(r, b, FWGPU_MODE_HOGWILD, w < P.n_windows_learn ? 1 : 0, tr->stream);
        if (rc) return rc;
        if ((rc = score_launch(tr, b, tr->seen + 1 + first, w < P.n_windows_learn))) return rc;  // (`seen` counts the piece once it is launched)
    }
    const uint32_t n_pred = P.n_take - P.n_learn;
    return close_slot(tr, c, n_pred ? P.d_pred + P.n_learn : nullptr, n_pred);
}

// launch_text_piece in the delayed protocol.  The parser's buffers are reused two pieces later, so every window's records are copied device to device
// into a ring batch on the compute stream, its offsets rebased to the copy (textparse.hip text_window_offsets), and the launches read the copy.  The plan
// was cut at predictions_after: its windows [0, n_windows_learn) hold the examples that are not predicted.
static int launch_text_piece_delayed(fwgpu_trainer *tr, fwgpu_text_parser *tp, int c, const TextTrainPiece &P) {
    fwgpu_regressor *r = tr->r;
    FWGPU_HIP(hipEventRecord(tr->uploaded[c], text_train_stream(tp)));
    FWGPU_HIP(hipStreamWaitEvent(tr->stream, tr->uploaded[c], 0));
    TextPlanShape shape;
    shape.n_learn = P.n_learn;
    shape.n_windows_learn = P.n_windows_learn;
    shape.n_windows = P.n_windows;
    const uint32_t n_pred = P.n_take - P.n_learn;
    int rc = reserve_pred_host(tr, c, n_pred);
    if (rc) return rc;
    uint64_t word0 = 0;  // the piece's records lie back to back in window order (text_batch_plan: rec_off is the running sum of the lines' lengths)
    for (uint32_t w = 0; w < P.n_windows; w++) {
        const uint64_t *st = P.win_stats + (size_t)kTextPlanStats * w;
        uint32_t first, end;
        shape.window(w, tr->micro_batch, P.n_take, &first, &end);
        const uint32_t n = end - first;
        if (st[0] != n || word0 + st[1] > P.n_words) return fail(FWGPU_ERR_DEVICE, "training from text: the plan's windows are not the host's");
        fwgpu_trainer::RingBatch rb;
        if ((rc = ring_take(tr, n, st[1], &rb))) return rc;
        fwgpu_batch *b = rb.b;
        hipError_t e = st[1] ? hipMemcpyAsync(b->records, P.d_records + word0, 4 * (size_t)st[1], hipMemcpyDeviceToDevice, tr->stream) : hipSuccess;
        if (e == hipSuccess) e = text_window_offsets(P.d_rec_off + first, n, b->rec_off, tr->stream);
        if (e != hipSuccess) {
            (void)hipEventRecord(rb.learned, tr->stream);
            tr->spare.push_back(rb);
            return fail(FWGPU_ERR_DEVICE, std::string("training from text: copying a window into the delay ring: ") + hipGetErrorString(e));
        }
        word0 += st[1];
        b->n = n;
        b->n_lr = st[5];
        b->n_ffm = st[6];
        b->n_words = st[1];
        b->max_lr = r->cfg.wiring == FWGPU_WIRING_FFM_ONLY ? 0 : (uint32_t)st[2];  // as record_batch_upload leaves a batch
        b->max_ffm = (uint32_t)st[3];
        b->max_rec = (uint32_t)st[4];
        b->aligned4 = true;
        b->host_copy.reset();
        if (record_batch_is_oversize(b)) {  // the one read-back: the host's translation of the window stays with the batch for both visits
            std::vector<uint64_t> off((size_t)n + 1);
            std::vector<uint32_t> words((size_t)st[1]);
            e = hipStreamSynchronize(tr->stream);
            if (e == hipSuccess) e = hipMemcpy(off.data(), b->rec_off, 8 * off.size(), hipMemcpyDeviceToHost);
            if (e == hipSuccess && !words.empty()) e = hipMemcpy(words.data(), b->records, 4 * words.size(), hipMemcpyDeviceToHost);
            rc = e != hipSuccess ? fail(FWGPU_ERR_DEVICE, std::string("training from text: reading an oversize window back: ") + hipGetErrorString(e))
                 : off[0] != 0 || off.back() != st[1] ? fail(FWGPU_ERR_DEVICE, "training from text: a window's offsets and its word count differ")
                                                      : record_batch_host_copy_if_oversize(r, &tr->t, b, words.data(), off.data(), n);
            if (rc) {
                (void)hipEventRecord(rb.learned, tr->stream);
                tr->spare.push_back(rb);
                return rc;
            }
        }
        const uint64_t last = tr->seen + end;  // (`seen` counts the piece once it is launched)
        const bool predicted = w >= P.n_windows_learn;
        if ((rc = ring_predict_and_keep(tr, rb, last, predicted))) return rc;
        if (predicted) FWGPU_HIP(hipMemcpyAsync(tr->pred_host[c] + (first - P.n_learn), b->pred, (size_t)n * 4, hipMemcpyDeviceToHost, tr->stream));
        if ((rc = ring_learn_eligible(tr, last))) return rc;
    }
    return close_slot(tr, c, nullptr, n_pred, true);
}

extern "C" {

int fwgpu_trainer_create(fwgpu_regressor *r, const fwgpu_translator_config *t, uint32_t micro_batch, fwgpu_trainer **out) {
    if (!r || !t || !out) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (micro_batch == 0) return fail(FWGPU_ERR_INVALID, "micro_batch must be > 0");
    if (int rcp = refuse_packed(r, "trainer_create")) return rcp;
    int crc = check_translator(r, t);
    if (crc) return crc;
    std::unique_ptr<fwgpu_trainer> tr(new fwgpu_trainer());
    tr->r = r;
    tr->micro_batch = micro_batch;
    tr->combo_off.assign(t->combo_off, t->combo_off + t->n_combos + 1);
    const uint32_t ncm = t->n_combos ? t->combo_off[t->n_combos] : 0;
    tr->combo_ns.assign(t->combo_ns, t->combo_ns + ncm);
    tr->combo_f32.assign(t->combo_ns_f32, t->combo_ns_f32 + ncm);
    tr->combo_weight.assign(t->combo_weight, t->combo_weight + t->n_combos);
    tr->field_off.assign(t->field_off, t->field_off + t->n_fields + 1);
    const uint32_t nfm = t->n_fields ? t->field_off[t->n_fields] : 0;
    tr->field_ns.assign(t->field_ns, t->field_ns + nfm);
    tr->field_f32.assign(t->field_ns_f32, t->field_ns_f32 + nfm);
    tr->t = *t;
    tr->t.combo_off = tr->combo_off.data();
    tr->t.combo_ns = tr->combo_ns.data();
    tr->t.combo_ns_f32 = tr->combo_f32.data();
    tr->t.combo_weight = tr->combo_weight.data();
    tr->t.field_off = tr->field_off.data();
    tr->t.field_ns = tr->field_ns.data();
    tr->t.field_ns_f32 = tr->field_f32.data();
    tr->off[0].assign(1, 0);
    tr->off[1].assign(1, 0);
    tr->host_threads = std::max(1u, std::thread::hardware_concurrency());
    FWGPU_HIP(hipSetDevice(r->device));
    FWGPU_HIP(hipStreamCreateWithFlags(&tr->stream, hipStreamNonBlocking));
    FWGPU_HIP(hipStreamCreateWithFlags(&tr->copy_stream, hipStreamNonBlocking));
    FWGPU_HIP(hipEventCreateWithFlags(&tr->uploaded[0], hipEventDisableTiming));
    FWGPU_HIP(hipEventCreateWithFlags(&tr->uploaded[1], hipEventDisableTiming));
    FWGPU_HIP(hipEventCreateWithFlags(&tr->done[0], hipEventDisableTiming));
    FWGPU_HIP(hipEventCreateWithFlags(&tr->done[1], hipEventDisableTiming));
    *out = tr.release();
    return FWGPU_OK;
}

int fwgpu_digest_records(fwgpu_trainer *tr, const uint32_t *records, const uint64_t *rec_off, uint32_t n) {
    if (!tr || (n && (!records || !rec_off))) return fail(FWGPU_ERR_INVALID, "NULL argument");
    uint32_t i = 0;
    while (i < n) {
        const int c = tr->cur;
        const uint32_t have = (uint32_t)(tr->off[c].size() - 1);
        uint32_t take = std::min<uint32_t>(n - i, tr->micro_batch - have);
        const bool predicting = predict_mode(tr);
        if (!predicting && tr->holdout_after) {  // a micro-batch never straddles the hold-out boundary
            const uint64_t until = tr->holdout_after - 1 - tr->seen;  // examples that may still be learned (>= 1 here)
            if (take > until) take = (uint32_t)until;
        }
        if (tr->delay && tr->seen < tr->predictions_after)  // ... nor predictions_after: a window's examples are predicted, or none is
            take = (uint32_t)std::min<uint64_t>(take, tr->predictions_after - tr->seen);
        // the records are copied (main.rs:243 `Vec::from(buffer)`)
        const uint64_t w0 = rec_off[i], w1 = rec_off[i + take];
        const uint64_t base = tr->rec_used[c];
        if (base + (w1 - w0) > tr->rec_cap[c]) {
            // (pinning memory is slow, 0.3-0.5 ms per MB: grow generously, a micro-batch a few percent larger than the last must not pin again)
            const uint64_t ncap = std::max<uint64_t>((base + (w1 - w0)) * 2, 1u << 20);
            uint32_t *nbuf = nullptr;
            FWGPU_HIP(hipSetDevice(tr->r->device));
            FWGPU_HIP(hipHostMalloc((void **)&nbuf, ncap * 4, hipHostMallocDefault));
            if (base) memcpy(nbuf, tr->rec[c], base * 4);
            if (tr->rec[c]) (void)hipHostFree(tr->rec[c]);
            tr->rec[c] = nbuf;
            tr->rec_cap[c] = ncap;
        }
        // copy into the pinned staging buffer and validate/count, on a few host threads for large slices
        {
            const unsigned T = take >= 4096 ? std::min<unsigned>(tr->host_threads, 8) : 1;
            std::vector<RecordStats> st(T);
            std::vector<int> rcs(T, FWGPU_OK);
            std::vector<std::string> msgs(T);
            auto work = [&](unsigned k) {
                const uint32_t a = i + (uint32_t)((uint64_t)take * k / T), e = i + (uint32_t)((uint64_t)take * (k + 1) / T);
                memcpy(tr->rec[c] + base + (rec_off[a] - w0), records + rec_off[a], (rec_off[e] - rec_off[a]) * 4);
                rcs[k] = count_records(&tr->t, records, rec_off + a, e - a, &st[k]);
                if (rcs[k]) msgs[k] = fwgpu_last_error();
            };
            tr->copy_pool.run(T, work);
            for (unsigned k = 0; k < T; k++) {
                if (rcs[k]) return fail(rcs[k], msgs[k]);
                tr->stats[c].merge(st[k]);
            }
        }
        tr->rec_used[c] = base + (w1 - w0);
        for (uint32_t j = 1; j <= take; j++) tr->off[c].push_back(base + (rec_off[i + j] - w0));
        tr->seen += take;
        i += take;
        if (tr->off[c].size() - 1 >= tr->micro_batch || (!predicting && predict_mode(tr)) || (tr->delay && tr->seen == tr->predictions_after)) {
            int rc = flush(tr, predicting);  // the last learned example closes its micro-batch
            if (rc) return rc;
        }
    }
    return FWGPU_OK;
}

// Cache file -> trainer without leaving native code (main.rs:213-270 with a cache: get_next_record -> digest_example).
// A reader thread fills one chunk from the file while the previous chunk is copied to pinned memory and shipped.
int fwgpu_trainer_digest_cache(fwgpu_trainer *tr, fwgpu_cache *cache, uint64_t max_records, uint64_t *n_digested) {
    if (!tr || !cache) return fail(FWGPU_ERR_INVALID, "NULL argument");
    const uint64_t chunk_records = std::max<uint64_t>(4 * (uint64_t)tr->micro_batch, 65536);
    const uint64_t chunk_words = 8ull << 20;  // 32 MiB of records per chunk
    struct Chunk {
        uint32_t *words = nullptr;
        uint64_t *off = nullptr;
        uint64_t n = 0, nw = 0;
        int rc = FWGPU_OK;
        std::string msg;
    } chunks[2];
    for (int k = 0; k < 2; k++) {  // buffers live in the trainer: no per-call allocation or zero fill
        if (!tr->cache_words[k]) tr->cache_words[k].reset(new uint32_t[chunk_words]);
        if (!tr->cache_off[k] || tr->cache_off_cap < chunk_records + 1) tr->cache_off[k].reset(new uint64_t[chunk_records + 1]);
        chunks[k].words = tr->cache_words[k].get();
        chunks[k].off = tr->cache_off[k].get();
    }
    tr->cache_off_cap = chunk_records + 1;
    uint64_t left = max_records ? max_records : ~0ull, done = 0;
    auto read_chunk = [&](Chunk &c, uint64_t want) {
        c.rc = fwgpu_cache_next_records(cache, c.words, chunk_words, c.off, std::min(want, chunk_records), &c.n, &c.nw);
        if (c.rc) c.msg = fwgpu_last_error();
    };
    int cur = 0;
    read_chunk(chunks[cur], left);
    int rc = FWGPU_OK;
    while (true) {
        Chunk &c = chunks[cur];
        if (c.rc) {
            rc = fail(c.rc, c.msg);
            break;
        }
        if (c.n == 0) break;  // end of file
        left -= c.n;
        std::thread reader;
        Chunk &next = chunks[cur ^ 1];
        const bool more = left > 0;
        if (more) reader = std::thread(read_chunk, std::ref(next), left);
        uint64_t i = 0;
        while (i < c.n && rc == FWGPU_OK) {  // fwgpu_digest_records takes a 32-bit count
            const uint32_t take = (uint32_t)std::min<uint64_t>(c.n - i, 1u << 30);
            rc = fwgpu_digest_records(tr, c.words, c.off + i, take);
            i += take;
        }
        if (reader.joinable()) reader.join();
        done += c.n;
        if (rc || !more) break;
        cur ^= 1;
    }
    if (n_digested) *n_digested = done;
    return rc;
}

// Text -> trainer in native code (main.rs:213-270 without a cache, or its first pass with `-c`): the buffer is cut at line
// boundaries into one slice per host thread, every slice is parsed by its own parser clone (VowpalParser is not thread
// safe), the records are digested in the original order and, when `cache` is open for writing, appended to it.
int fwgpu_trainer_digest_text(fwgpu_trainer *tr, fwgpu_parser *parser, fwgpu_cache *cache, const char *text, uint64_t len,
                              uint32_t threads, uint64_t *n_examples, uint64_t *consumed) {
    if (!tr || !parser || (!text && len)) return fail(FWGPU_ERR_INVALID, "NULL argument");
    const unsigned T = std::max(1u, std::min<unsigned>(threads ? threads : 8, 64));
    struct Slice {
        uint64_t begin = 0, end = 0, used = 0, nr = 0, nw = 0;
        std::unique_ptr<uint32_t[]> words;  // uninitialised on purpose: zero-filling hundreds of MB costs more than parsing them
        uint64_t words_cap = 0;
        std::vector<uint64_t> off;
        int rc = FWGPU_OK;
        std::string msg;
        void grow(uint64_t cap) {
            std::unique_ptr<uint32_t[]> nb(new uint32_t[cap]);
            if (nw) memcpy(nb.get(), words.get(), nw * 4);
            words = std::move(nb);
            words_cap = cap;
        }
    };
    struct Clones {  // one parser clone per extra thread (VowpalParser is not thread safe), for the length of this call
        std::vector<fwgpu_parser *> p;
        ~Clones() {
            for (fwgpu_parser *q : p) fwgpu_parser_free(q);
        }
    } clones;
    // Two stages, pipelined over chunks of the text: chunk i+1 is parsed (T threads) while chunk i's records are digested (staging
    // copy, upload, learn launches) on a helper thread, in order.  One pass over the whole buffer (parse everything, then digest
    // everything) left the GPU idle while parsing and the parsers idle while learning: 1.3 M lines/s on 16 threads.
    auto parse_range = [&](uint64_t r_begin, uint64_t r_end, std::vector<Slice> &sl) {
    if (sl.size() != T) sl.resize(T);
    for (Slice &q : sl) {  // (the record buffers of the previous chunk are kept: first-touch page faults of 16 threads at once do not scale)
        q.begin = q.end = q.used = q.nr = q.nw = 0;
        q.rc = FWGPU_OK;
        q.msg.clear();
    }
    uint64_t pos = r_begin;
    const uint64_t rlen = r_end - r_begin;
    for (unsigned k = 0; k < T; k++) {  // slice k ends at the first line break at or after its proportional share
        sl[k].begin = pos;
        uint64_t e = k + 1 == T ? r_end : std::max<uint64_t>(pos, r_begin + rlen * (k + 1) / T);
        if (e < r_end) {
            const void *nl = memchr(text + e, '\n', r_end - e);
            e = nl ? (uint64_t)(static_cast<const char *>(nl) - text) + 1 : r_end;
        }
        sl[k].end = pos = e;
    }
    auto work = [&](unsigned k) {
        Slice &s = sl[k];
        const uint64_t n = s.end - s.begin;
        if (!n) return;
        fwgpu_parser *p = k > 0 ? clones.p[k - 1] : parser;
        uint64_t lines = 0;
        for (const char *q = text + s.begin, *e = text + s.end; q < e; lines++) {
            const void *nl = memchr(q, '\n', (size_t)(e - q));
            q = nl ? static_cast<const char *>(nl) + 1 : e;
        }
        // a feature token takes >= 2 bytes of text and <= 2 words of record; the per-line header depends on the namespace
        // map, so the buffer grows whenever a pass stops short without an error
        if (s.words_cap < n + lines * 64 + 4096) s.grow(n + lines * 64 + 4096);
        s.off.assign(lines + 1, 0);
        std::vector<uint64_t> tmp(lines + 1);
        while (s.used < n) {
            uint64_t nr = 0, nw = 0, used = 0;
            s.rc = fwgpu_parser_parse_buffer(p, text + s.begin + s.used, n - s.used, s.words.get() + s.nw, s.words_cap - s.nw,
                                             tmp.data(), lines - s.nr, &nr, &nw, &used);
            for (uint64_t j = 1; j <= nr; j++) s.off[s.nr + j] = s.nw + tmp[j];
            s.nr += nr;
            s.nw += nw;
            s.used += used;
            if (s.rc != FWGPU_OK) {
                s.msg = fwgpu_last_error();
                break;
            }
            if (s.used < n) {  // out of room (not a command, not an error): grow and go on
                if (s.words_cap > (1ull << 33)) {
                    s.rc = FWGPU_ERR_RANGE;
                    s.msg = "digest_text: a slice needs more than 32 GiB of records";
                    break;
                }
                s.grow(s.words_cap * 2);
            }
        }
    };
    tr->parse_pool.run(T, work);
    };
    for (unsigned k = 1; k < T; k++) {
        fwgpu_parser *c = nullptr;
        const int crc = fwgpu_parser_clone(parser, &c);
        if (crc) return crc;
        clones.p.push_back(c);
    }
    uint64_t done = 0, used = 0;
    // digests the slices of one chunk in order; false: stop (rc says why: an error, or a command line reached)
    auto digest_slices = [&](std::vector<Slice> &sl, int &rc, std::string &msg) -> bool {
        for (unsigned k = 0; k < T && rc == FWGPU_OK; k++) {
            Slice &s = sl[k];
            uint64_t i = 0;
            while (i < s.nr && rc == FWGPU_OK) {
                const uint32_t take = (uint32_t)std::min<uint64_t>(s.nr - i, 1u << 30);
                // offsets are relative to the slice's first word
                rc = fwgpu_digest_records(tr, s.words.get(), s.off.data() + i, take);
                i += take;
            }
            if (rc == FWGPU_OK && cache && s.nw) rc = fwgpu_cache_push_records(cache, s.words.get(), s.nw);
            if (rc != FWGPU_OK) {
                msg = fwgpu_last_error();  // (thread-local: carried back to the caller's thread)
                return false;
            }
            done += s.nr;
            used = s.begin + s.used;
            if (s.rc != FWGPU_OK) {  // a command or a bad line stopped this slice: stop here, in order
                rc = s.rc;
                msg = s.msg;
                return false;
            }
        }
        return rc == FWGPU_OK;
    };
    // chunks of about 1 MB of text per parser thread (the threads are a pool: a chunk costs no thread start), 8 to 64 MB in all
    // (FWGPU_TEXT_CHUNK_MB overrides), cut at line breaks
    uint64_t chunk_target = std::min<uint64_t>(std::max<uint64_t>((uint64_t)T * (1u << 20), 8u << 20), 64u << 20);
    if (const char *env = getenv("FWGPU_TEXT_CHUNK_MB"))
        if (atoi(env) > 0) chunk_target = (uint64_t)atoi(env) << 20;
    std::vector<Slice> cur, next;
    int rc = FWGPU_OK;
    std::string msg;
    uint64_t pos = 0;
    auto chunk_end = [&](uint64_t from) {
        uint64_t e = std::min<uint64_t>(len, from + chunk_target);
        if (e < len) {
            const void *nl = memchr(text + e, '\n', len - e);
            e = nl ? (uint64_t)(static_cast<const char *>(nl) - text) + 1 : len;
        }
        return e;
    };
    bool have = false;
    if (len) {
        const uint64_t e = chunk_end(0);
        parse_range(0, e, cur);
        pos = e;
        have = true;
    }
    const bool timing = getenv("FWGPU_TRAINER_TIMING") != nullptr;  // per chunk: parse of the next chunk / digest of this one, ms
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    while (have) {
        bool go_on = true;
        double t_digest = 0.0;
        const auto t0 = now();
        std::thread dg([&] {
            go_on = digest_slices(cur, rc, msg);
            t_digest = ms(t0, now());
        });
        bool parsed_next = false;
        if (pos < len) {
            const uint64_t e = chunk_end(pos);
            parse_range(pos, e, next);
            pos = e;
            parsed_next = true;
        }
        const double t_parse = ms(t0, now());
        dg.join();
        if (timing) fprintf(stderr, "[digest_text] chunk: parse of the next %.2f ms, digest of this one %.2f ms, both %.2f ms\n", t_parse, t_digest, ms(t0, now()));
        if (!go_on || !parsed_next) break;  // (a chunk parsed past a command line or an error is dropped: `consumed` says where to resume)
        cur.swap(next);
    }
    if (rc != FWGPU_OK && rc != FWGPU_PARSE_FLUSH && rc != FWGPU_PARSE_HOGWILD_LOAD) rc = fail(rc, msg);
    if (n_examples) *n_examples = done;
    if (consumed) *consumed = used;
    return rc;
}

// fwgpu_trainer_digest_text with the parser on the device (textparse.hip): the text goes up in pieces cut at line breaks, every piece is parsed,
// cut into micro-batches and placed by kernels on the parser's stream, and launched from there -- piece i + 1 is parsed while piece i is learned.
// The host parses only the lines the kernel leaves to it and reads a few words per launch; records come back only for a cache that is written
// and for a launch with an oversize example.
int fwgpu_trainer_digest_text_device(fwgpu_trainer *tr, fwgpu_text_parser *tp, fwgpu_cache *cache, const char *text, uint64_t len, uint64_t *n_examples,
                                     uint64_t *consumed) {
    if (n_examples) *n_examples = 0;
    if (consumed) *consumed = 0;
    if (!tr || !tp || (!text && len)) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (cache && !fwgpu_cache_is_writing(cache)) return fail(FWGPU_ERR_INVALID, "digest_text_device: the cache is not open for writing");
    fwgpu_regressor *r = tr->r;
    FWGPU_HIP(hipSetDevice(r->device));
    int rc = text_train_begin(tp, &tr->t, r->device);
    if (rc) return rc;
    // a micro-batch an earlier fwgpu_digest_records left open goes first (its examples are of one kind, as in fwgpu_finish)
    if ((rc = flush(tr, tr->testonly || (tr->holdout_after && tr->seen >= tr->holdout_after)))) return rc;
    uint64_t piece = 8u << 20;
    if (const char *env = getenv("FWGPU_TRAINER_TEXT_PIECE"))
        if (atoll(env) > 0) piece = (uint64_t)atoll(env);
    piece = std::min<uint64_t>(piece, 16u << 20);
    uint64_t pos = 0, done = 0, used = 0;
    std::vector<uint32_t> back;
    std::string msg;
    while (pos < len && rc == FWGPU_OK) {
        uint64_t cut = std::min<uint64_t>(len - pos, piece);
        if (pos + cut < len) {  // cut at the last line break of the window; a line longer than a piece is a piece
            const void *nl = memrchr(text + pos, '\n', cut);
            if (!nl) nl = memchr(text + pos + cut, '\n', len - pos - cut);
            cut = nl ? (uint64_t)(static_cast<const char *>(nl) - (text + pos)) + 1 : len - pos;
        }
        const int c = tr->cur;
        if ((rc = retire(tr, c))) return rc;  // the parser's set c was read by the piece before the last (retired when that slot was opened)
        uint32_t learn_before = kTextNoHoldout;  // lines of this piece that may still be learned: no launch straddles the hold-out boundary
        if (tr->testonly) learn_before = 0;
        else if (tr->holdout_after) learn_before = (uint32_t)std::min<uint64_t>(tr->seen + 1 >= tr->holdout_after ? 0 : tr->holdout_after - 1 - tr->seen, 0xfffffffeu);
        else if (tr->delay)  // delayed protocol: nothing is held out; the plan's cut is the one at predictions_after (lines before it are not predicted)
            learn_before = (uint32_t)std::min<uint64_t>(tr->seen >= tr->predictions_after ? 0 : tr->predictions_after - tr->seen, 0xfffffffeu);
        TextTrainPiece P;
        if ((rc = text_train_piece(tp, text + pos, cut, c, tr->micro_batch, learn_before, &P))) return rc;
        if (P.n_take) {
            if (cache) {  // the one read-back of this route: the piece's records, word for word what the host route appends
                back.resize((size_t)P.n_words);
                if ((rc = text_train_wait(tp))) return rc;
                FWGPU_HIP(hipMemcpy(back.data(), P.d_records, 4 * back.size(), hipMemcpyDeviceToHost));
                if ((rc = fwgpu_cache_push_records(cache, back.data(), P.n_words))) return rc;
            }
            if ((rc = tr->delay ? launch_text_piece_delayed(tr, tp, c, P) : launch_text_piece(tr, tp, c, P))) return rc;
            if ((rc = open_slot(tr))) return rc;  // (waits for the piece BEFORE this one, whose buffers the next piece takes)
            tr->seen += P.n_take;
            done += P.n_take;
        }
        used = pos + P.consumed;
        if (n_examples) *n_examples = done;
        if (consumed) *consumed = used;
        if (P.stop != FWGPU_OK) {
            rc = P.stop;
            msg = P.stop_msg;
        }
        pos += cut;
    }
    if (rc != FWGPU_OK && rc != FWGPU_PARSE_FLUSH && rc != FWGPU_PARSE_HOGWILD_LOAD) rc = fail(rc, msg);
    return rc;
}

int fwgpu_trainer_set_holdout(fwgpu_trainer *tr, uint64_t holdout_after, int testonly) {
    if (!tr) return fail(FWGPU_ERR_INVALID, "NULL trainer");
    if (tr->off[tr->cur].size() > 1) return fail(FWGPU_ERR_INVALID, "set the hold-out before digesting (or right after fwgpu_finish)");
    if (tr->delay && (holdout_after || testonly))
        return fail(FWGPU_ERR_INVALID, std::string("set_holdout: ") + (testonly ? "testonly" : "holdout_after") +
                                           " conflicts with prediction_model_delay (fwgpu_trainer_set_delay), whose loop holds nothing out: set one of them");
    tr->holdout_after = holdout_after;
    tr->testonly = testonly != 0;
    return FWGPU_OK;
}

int fwgpu_trainer_set_delay(fwgpu_trainer *tr, uint64_t delay, uint64_t predictions_after) {
    if (!tr) return fail(FWGPU_ERR_INVALID, "NULL trainer");
    if (tr->seen) return fail(FWGPU_ERR_INVALID, "set_delay: prediction_model_delay and predictions_after are set before the first example is digested");
    if (delay && (tr->holdout_after || tr->testonly))
        return fail(FWGPU_ERR_INVALID, std::string("set_delay: prediction_model_delay conflicts with ") + (tr->testonly ? "testonly" : "holdout_after") +
                                           " (fwgpu_trainer_set_holdout): the delayed loop holds nothing out: set one of them");
    tr->delay = delay;
    tr->predictions_after = delay ? predictions_after : 0;
    return FWGPU_OK;
}

int fwgpu_trainer_delay_state(const fwgpu_trainer *tr, uint64_t *learned_through, uint64_t *pending_examples, uint64_t *pending_windows, uint64_t *ring_bytes) {
    if (!tr) return fail(FWGPU_ERR_INVALID, "NULL trainer");
    if (learned_through) *learned_through = tr->learned_through;
    if (pending_examples) *pending_examples = tr->pending_examples;
    if (pending_windows) *pending_windows = tr->pending.size();
    if (ring_bytes) *ring_bytes = tr->ring_bytes;
    return FWGPU_OK;
}

int fwgpu_debug_delay_plan(const uint64_t *window_last, uint32_t n_windows, uint64_t delay, uint64_t *learned_through_after) {
    if (n_windows && (!window_last || !learned_through_after)) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (!delay) return fail(FWGPU_ERR_INVALID, "delay_plan: delay must be > 0 (0 is the trainer without the delayed protocol)");
    uint64_t learned = 0;
    uint32_t front = 0;  // oldest pending window
    for (uint32_t j = 0; j < n_windows; j++) {
        if (window_last[j] <= (j ? window_last[j - 1] : 0)) return fail(FWGPU_ERR_INVALID, "delay_plan: the windows' last numbers must grow, from 1");
        while (front <= j && delay_eligible(window_last[front], window_last[j], delay)) learned = window_last[front++];
        learned_through_after[j] = learned;
    }
    return FWGPU_OK;
}

int fwgpu_trainer_set_metrics(fwgpu_trainer *tr, uint64_t window) {
    if (!tr) return fail(FWGPU_ERR_INVALID, "NULL trainer");
    if (tr->seen) return fail(FWGPU_ERR_INVALID, "set the metrics window before digesting");
    tr->metrics.window = window;
    return FWGPU_OK;
}

int fwgpu_trainer_metrics(fwgpu_trainer *tr, fwgpu_metric_window *rows, uint64_t cap, uint64_t *n_rows, fwgpu_metric_total *learned,
                          fwgpu_metric_total *held_out) {
    if (!tr || !n_rows) return fail(FWGPU_ERR_INVALID, "NULL argument");
    *n_rows = tr->metrics.used;
    if (rows && cap < tr->metrics.used) return fail(FWGPU_ERR_RANGE, "buffer too small for the windows");
    FWGPU_HIP(hipSetDevice(tr->r->device));
    return tr->metrics.fetch(0, rows ? tr->metrics.used : 0, rows, learned, held_out, tr->stream);
}

int fwgpu_trainer_predictions(fwgpu_trainer *tr, float *out, uint64_t cap, uint64_t *n) {
    if (!tr || !n) return fail(FWGPU_ERR_INVALID, "NULL argument");
    *n = tr->preds.size();
    if (!out) return FWGPU_OK;
    if (cap < tr->preds.size()) return fail(FWGPU_ERR_RANGE, "buffer too small for the predictions");
    if (!tr->preds.empty()) memcpy(out, tr->preds.data(), tr->preds.size() * 4);
    return FWGPU_OK;
}

int fwgpu_finish(fwgpu_trainer *tr) {
    if (!tr) return fail(FWGPU_ERR_INVALID, "NULL trainer");
    // the open micro-batch holds examples of ONE kind; they were predicted iff the example before `seen + 1` was
    const bool last_predict = tr->testonly || (tr->holdout_after && tr->seen >= tr->holdout_after);
    int rc = flush(tr, last_predict);
    if (rc) return rc;
    FWGPU_HIP(hipSetDevice(tr->r->device));
    FWGPU_HIP(hipStreamSynchronize(tr->stream));
    // slots retire in launch order: the one launched before the current filling slot's predecessor first
    rc = retire(tr, tr->cur);
    if (rc) return rc;
    rc = retire(tr, tr->cur ^ 1);
    if (rc) return rc;
    return FWGPU_OK;
}

int fwgpu_trainer_free(fwgpu_trainer *tr) {
    if (!tr) return FWGPU_OK;
    (void)hipSetDevice(tr->r->device);
    if (tr->stream) (void)hipStreamSynchronize(tr->stream);
    if (tr->text_tr) fwgpu_batch_free(tr->text_tr);
    for (std::deque<fwgpu_trainer::RingBatch> *q : {&tr->pending, &tr->spare})  // the delay ring: pending windows are dropped unlearned, like the reference's queue
        for (fwgpu_trainer::RingBatch &rb : *q) {
            fwgpu_batch_free(rb.b);
            (void)hipEventDestroy(rb.learned);
        }
    tr->metrics.release();
    for (int i = 0; i < 2; i++) {
        if (tr->dev[i]) fwgpu_batch_free(tr->dev[i]);
        if (tr->rec[i]) (void)hipHostFree(tr->rec[i]);
        if (tr->pred_host[i]) (void)hipHostFree(tr->pred_host[i]);
        if (tr->done[i]) (void)hipEventDestroy(tr->done[i]);
    }
    if (tr->stream) (void)hipStreamDestroy(tr->stream);
    if (tr->copy_stream) (void)hipStreamDestroy(tr->copy_stream);
    for (int i = 0; i < 2; i++)
        if (tr->uploaded[i]) (void)hipEventDestroy(tr->uploaded[i]);
    delete tr;
    return FWGPU_OK;
}

int fwgpu_trainer_examples_seen(const fwgpu_trainer *tr, uint64_t *n) {
    if (!tr || !n) return fail(FWGPU_ERR_INVALID, "NULL argument");
    *n = tr->seen;
    return FWGPU_OK;
}

}  // extern "C"
