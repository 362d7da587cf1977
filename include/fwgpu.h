/*
 * fwgpu.h -- C ABI of the MI355X-native LR+FFM online learner.
 *
 * This library is a drop-in for ONE path of outbrain-inc/fwumious_wabbit: what sits behind
 * `Regressor` (src/regressor.rs:142-147) and `HogwildTrainer` (src/hogwild.rs:13-61), i.e.
 * block_lr / block_ffm / block_misc::Triangle / block_loss_functions / optimizer / hogwild.
 * Everything is plain pointers and sizes; no C++/torch types cross this boundary.
 *
 * Conventions (cf. the reference's existing predict-only C ABI, src/lib.rs:151-243):
 *  - every call returns an int status (FWGPU_OK == 0); fwgpu_last_error() gives the message of the
 *    last failure on the calling thread.  Nothing unwinds across the boundary.
 *  - the caller owns every input buffer; buffers are borrowed for the duration of the call only
 *    (fwgpu_digest_records copies the records, like main.rs:243 `Vec::from(buffer)`).
 *  - the library owns weights, optimizer state and all device scratch.
 *  - one handle == one device context.  learn/update calls on one handle are single-producer
 *    (regressor.rs:362-365: learn() is not thread-safe).
 *  - `stream` arguments are `hipStream_t` passed as void* (NULL = the null stream), so a caller that
 *    already runs on a stream (e.g. torch.cuda.current_stream().cuda_stream) can time and order the
 *    work with its own events.
 *  - there is NO CPU fallback: if no HIP device is usable fwgpu_create fails with FWGPU_ERR_DEVICE.
 */
#ifndef FWGPU_H
#define FWGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FWGPU_ABI_VERSION 1

enum {
    FWGPU_OK = 0,
    FWGPU_ERR_INVALID = 1, /* bad argument / config (the reference exits 1: main.rs:44-47) */
    FWGPU_ERR_DEVICE = 2,  /* HIP error or no device */
    FWGPU_ERR_OOM = 3,
    FWGPU_ERR_RANGE = 4,   /* buffer too small / index out of range */
    FWGPU_ERR_FORMAT = 5,  /* malformed record, weight blob, cache or model file */
    FWGPU_ERR_PARSE = 6,   /* the text parser rejected a line; fwgpu_last_error() holds the reference's message */
    FWGPU_ERR_IO = 7,      /* file could not be opened / read / written */
    FWGPU_ERR_PEER = 8,    /* multi-GPU step: ANOTHER rank of the job failed (or is gone); this rank exchanged and applied nothing in the step */
    /* not errors: commands the text parser hands back instead of a record (parser.rs:31-57) */
    FWGPU_PARSE_FLUSH = 100,
    FWGPU_PARSE_HOGWILD_LOAD = 101
};

/* model_instance.rs:24-28 `enum Optimizer` */
enum { FWGPU_OPT_SGD = 100, FWGPU_OPT_ADAGRAD_FLEX = 200, FWGPU_OPT_ADAGRAD_LUT = 300 };

/* Graph wiring.  REGRESSOR: regressor.rs:173-330 LR -> [FFM -> Triangle -> Join] -> Sigmoid.
 * FFM_ONLY: the wiring of the reference's FFM block tests (block_ffm.rs:1253-1254: FFM -> Sigmoid). */
enum { FWGPU_WIRING_REGRESSOR = 0, FWGPU_WIRING_FFM_ONLY = 1 };

/* How a batch is executed on the device.
 * SEQUENTIAL: one workgroup walks the batch in order; example i sees every update of examples <i.
 *             This is the reference's single-thread semantics (main.rs:213-270) and the parity mode.
 * HOGWILD:    all workgroups run examples concurrently against the shared tables with unsynchronised
 *             read-modify-write, the device analogue of hogwild.rs:24-103 (non-deterministic). */
enum { FWGPU_MODE_SEQUENTIAL = 0, FWGPU_MODE_HOGWILD = 1 };

/* feature_buffer.rs:10-15 `HashAndValue` */
typedef struct fwgpu_lr_entry {
    uint32_t hash;
    float value;
    uint32_t combo_index;
} fwgpu_lr_entry;

/* feature_buffer.rs:17-22 `HashAndValueAndSeq` */
typedef struct fwgpu_ffm_entry {
    uint32_t hash;
    float value;
    uint32_t contra_field_index; /* field * ffm_k */
} fwgpu_ffm_entry;

/* The ModelInstance fields the blocks on this path read (model_instance.rs:47-97;
 * block_lr.rs:53-67, block_ffm.rs:70-94, 793-822). */
typedef struct fwgpu_config {
    int32_t optimizer;        /* FWGPU_OPT_* */
    float learning_rate;      /* -l */
    float power_t;            /* --power_t */
    float init_acc_gradient;  /* --init_acc_gradient */
    uint32_t bit_precision;   /* -b : LR table has 2^b entries (block_lr.rs:67) */
    uint32_t num_combos;      /* feature_combo_descs.len() + (add_constant_feature ? 1 : 0) (block_lr.rs:53-56) */
    uint32_t ffm_k;           /* --ffm_k, 0 = no FFM block */
    uint32_t ffm_bit_precision;
    uint32_t ffm_num_fields;  /* ffm_fields.len() */
    float ffm_learning_rate, ffm_power_t, ffm_init_acc_gradient;
    float ffm_init_center, ffm_init_width, ffm_init_zero_band;
    int32_t wiring;           /* FWGPU_WIRING_* */
    int32_t device;           /* HIP device ordinal */
} fwgpu_config;

typedef struct fwgpu_regressor fwgpu_regressor; /* opaque, like lib.rs:50-53 FfiPredictor */
typedef struct fwgpu_batch fwgpu_batch;         /* opaque device-resident micro-batch */
typedef struct fwgpu_trainer fwgpu_trainer;     /* opaque record-stream trainer (HogwildTrainer role) */

const char *fwgpu_last_error(void);
int fwgpu_abi_version(void);

/* ---------------------------------------------------------------- Regressor
 * fwgpu_create        <= Regressor::new_without_weights(&ModelInstance)   regressor.rs:173-330
 *                        (tables are allocated here, zero-filled)
 * fwgpu_init_weights  <= Regressor::allocate_and_init_weights             regressor.rs:352-354
 * fwgpu_learn         <= Regressor::learn(&FeatureBuffer,&mut PortBuffer,update) -> f32   regressor.rs:356-379
 * fwgpu_predict       <= Regressor::predict(&FeatureBuffer,&mut PortBuffer) -> f32        regressor.rs:381-395
 * fwgpu_free          <= drop(Regressor)
 * The FeatureBuffer (feature_buffer.rs:24-31) is passed as its four members. ffm entries must be
 * ordered by field, as FeatureBufferTranslator produces them (block_ffm.rs:165-183 relies on it). */
int fwgpu_create(const fwgpu_config *cfg, fwgpu_regressor **out);
int fwgpu_free(fwgpu_regressor *r);
int fwgpu_init_weights(fwgpu_regressor *r);
int fwgpu_learn(fwgpu_regressor *r, const fwgpu_lr_entry *lr, uint32_t n_lr, const fwgpu_ffm_entry *ffm,
                uint32_t n_ffm, float label, float importance, int update, float *prediction);
int fwgpu_predict(fwgpu_regressor *r, const fwgpu_lr_entry *lr, uint32_t n_lr, const fwgpu_ffm_entry *ffm,
                  uint32_t n_ffm, float *prediction);

/* ---------------------------------------------------------------- serving context cache
 * fwgpu_setup_cache        <= Regressor::setup_cache(&FeatureBuffer, &mut Vec<BlockCache>, should_create)  regressor.rs:409-423
 *                             (*cache == NULL creates it; otherwise the existing cache is refilled)
 * fwgpu_predict_with_cache <= Regressor::predict_with_cache(&FeatureBuffer, &mut PortBuffer, &[BlockCache]) -> f32
 *                             regressor.rs:397-407.  fb is the FeatureBuffer of context + candidate, as the reference's
 *                             caller passes it (lib.rs:88-108).
 * The cache is BlockFFM's (block_ffm.rs:442-782): the context features' field sums and self-pair corrections, computed once
 * on the device, plus `features_present` (regressor.rs:25-38: hash + contra_field_index).  A candidate then gathers only the
 * FFM rows of the features that are not present in the cache.  BlockLR's cache never holds anything in the reference
 * (block_lr.rs:236-239 skips every masked hash), so LR entries are all read, as there.  Models with a deep head are covered (every
 * block behind the FFM block inherits forward_with_cache, block_neural.rs:355): the cache also keeps how many features it holds per
 * field, and the head's input diagonal of a field with c cached and n gathered features is what an uncached launch computes for
 * c == 0, exactly 0 for c + n <= 1, and 0.5 (|field sum|^2 - sum of the features' own squares) otherwise.  A second
 * fwgpu_setup_cache on the same handle refreshes sums and counts.  Packed regressors: refused, unless fwgpu_packed_enable_caches was called.
 * fwgpu_block_cache_filter: the FFM entries forward_with_cache still gathers (what an entry batch used with
 * fwgpu_batch_set_cache: must hold); predict-only launches of that batch then start every example from the cache. */
typedef struct fwgpu_block_cache fwgpu_block_cache;
int fwgpu_setup_cache(fwgpu_regressor *r, const fwgpu_lr_entry *lr, uint32_t n_lr, const fwgpu_ffm_entry *ffm,
                      uint32_t n_ffm, fwgpu_block_cache **cache);
int fwgpu_predict_with_cache(fwgpu_regressor *r, const fwgpu_block_cache *cache, const fwgpu_lr_entry *lr, uint32_t n_lr,
                             const fwgpu_ffm_entry *ffm, uint32_t n_ffm, float *prediction);
int fwgpu_block_cache_filter(const fwgpu_block_cache *cache, const fwgpu_ffm_entry *ffm, uint32_t n_ffm, fwgpu_ffm_entry *out,
                       uint32_t *n_out);
int fwgpu_block_cache_free(fwgpu_block_cache *cache);
/* Record batches with the cache: the context's own record marks its namespace slots as covered; the record of a request
 * (context + candidate, parser.rs:195-211) then goes to the device whole and the example kernel's translation leaves the
 * covered slots' FFM features out.  That equals fwgpu_block_cache_filter on the request's translation whenever
 * fwgpu_block_cache_record_ok returns 1 (the request has not named a covered namespace again, and none of its own features
 * has the hash and field of a cached one); a request for which it returns 0 takes the entry route. */
struct fwgpu_translator_config;
int fwgpu_block_cache_cover_record(fwgpu_block_cache *cache, const struct fwgpu_translator_config *t, const uint32_t *record, uint32_t len);
int fwgpu_block_cache_record_ok(const fwgpu_block_cache *cache, const struct fwgpu_translator_config *t, const uint32_t *record, uint32_t len);

/* ---------------------------------------------------------------- deep head (BASELINE config E)
 * fwgpu_set_nn <= the `--nn_layers / --nn N:width:W / --nn N:activation:relu / --nn N:init:hu / --nn_topology` part of
 * Regressor::new_without_weights (regressor.rs:191-320): BlockCopy -> [BlockNeuronLayer -> BlockRELU]* -> Join ->
 * single neuron (InitType::One) in front of the sigmoid.  Call after fwgpu_create and before fwgpu_init_weights.
 * Per-example semantics are the reference's (block_neural.rs:252-340: every dense weight with a non-zero upstream
 * gradient takes an AdaGrad step, neuron by neuron).
 * INIT STREAM -- PARITY UNPINNED: hidden-layer init Hu / Xavier draws from the library's own deterministic generator.  The
 * reference draws from Xoshiro256PlusPlus::seed_from_u64(..) + rand_distr::Normal (block_neural.rs:385-406; third-party crates,
 * no reference test observes a value), so a model INITIALISED here has the reference's distribution but not its numbers: it is
 * not the model `fw` would initialise from the same command line.  Cross-checks load identical weights on both sides
 * (fwgpu_table_write(FWGPU_TABLE_NN_W) or a model file); InitType::One / Zero are exact.
 * Mini-batch mode: inside fwgpu_learn_batch_sync a deep head trains mini-batched on the matrix cores (dense weights frozen per
 * batch, gradients summed, ONE optimizer step per weight and batch) -- a different algorithm from the per-example one above,
 * never chosen implicitly. */
#define FWGPU_NN_MAX_LAYERS 8
enum { FWGPU_NN_INIT_XAVIER = 0, FWGPU_NN_INIT_HU = 1, FWGPU_NN_INIT_ONE = 2, FWGPU_NN_INIT_ZERO = 3 };
typedef struct fwgpu_nn_config {
    uint32_t n_layers;                     /* hidden layers */
    uint32_t width[FWGPU_NN_MAX_LAYERS];   /* --nn N:width:W (default 20) */
    uint32_t relu[FWGPU_NN_MAX_LAYERS];    /* --nn N:activation:relu -> 1, none -> 0 */
    uint32_t init[FWGPU_NN_MAX_LAYERS];    /* --nn N:init:... (default hu) */
    uint32_t topology;                     /* 1 = "one" (default, model_instance.rs:42), 2 = "two" */
    float nn_learning_rate, nn_power_t, nn_init_acc_gradient; /* model_instance.rs:426-428 */
} fwgpu_nn_config;
int fwgpu_set_nn(fwgpu_regressor *r, const fwgpu_nn_config *nn);

/* ---------------------------------------------------------------- weight (de)serialisation
 * fwgpu_serialized_len / fwgpu_write_weights / fwgpu_read_weights
 *      <= Regressor::write_weights_to_buf / overwrite_weights_from_buf    regressor.rs:426-469
 * Blob = u64 LE total element count (sum of get_serialized_len), then per block, in order:
 *   LR : 2^b x {f32 w, f32 acc}   (SGD: {f32 w})              block_lr.rs:257-275, block_helpers.rs:17-28
 *   FFM: len x f32 w, then len x f32 acc (SGD: no acc part)   block_ffm.rs:835-863
 *   NN : per dense layer, weights then optimizer state        block_neural.rs:430-448
 * fwgpu_serialized_len returns the byte size of that blob. */
int fwgpu_serialized_len(fwgpu_regressor *r, uint64_t *n_bytes);
int fwgpu_write_weights(fwgpu_regressor *r, uint8_t *buf, uint64_t cap, uint64_t *written);
int fwgpu_read_weights(fwgpu_regressor *r, const uint8_t *buf, uint64_t len);

/* Raw table access (tests, weight patching).  which: 0 = LR table as interleaved {w,acc} floats
 * (2*2^b floats), 1 = FFM weights, 2 = FFM optimizer state (each 2^ffm_bits + F*k floats,
 * block_ffm.rs:92-94).  Offsets and counts are in floats. */
enum { FWGPU_TABLE_LR = 0, FWGPU_TABLE_FFM_W = 1, FWGPU_TABLE_FFM_ACC = 2,
       FWGPU_TABLE_NN_W = 3, FWGPU_TABLE_NN_ACC = 4 /* all dense layers back to back: hidden layers, then the final neuron */ };
int fwgpu_table_len(fwgpu_regressor *r, int which, uint64_t *n_floats);
int fwgpu_table_read(fwgpu_regressor *r, int which, uint64_t offset, uint64_t count, float *host_out);
int fwgpu_table_write(fwgpu_regressor *r, int which, uint64_t offset, uint64_t count, const float *host_in);
int fwgpu_table_fill(fwgpu_regressor *r, int which, float value);
/* Order-independent checksum of a table computed on the device: sum over i of
 * mix64(i ^ bits(table[i])) (wrapping u64). */
int fwgpu_table_checksum(fwgpu_regressor *r, int which, uint64_t *checksum);
/* Device address of a table (for zero-copy interop, e.g. wrapping it for an RCCL all-reduce). */
int fwgpu_table_device_ptr(fwgpu_regressor *r, int which, void **dev_ptr);

/* ---------------------------------------------------------------- micro-batches
 * A batch is a CSR of FeatureBuffers resident in HBM: example i owns lr[lr_off[i]..lr_off[i+1]) and
 * ffm[ffm_off[i]..ffm_off[i+1]).  label/importance per example (feature_buffer.rs:187-189).
 * fwgpu_batch_create copies host arrays to the device (synchronously, on the null stream). */
int fwgpu_batch_create(fwgpu_regressor *r, const fwgpu_lr_entry *lr, const uint32_t *lr_off,
                       const fwgpu_ffm_entry *ffm, const uint32_t *ffm_off, const float *label,
                       const float *importance, uint32_t n_examples, fwgpu_batch **out);
int fwgpu_batch_free(fwgpu_batch *b);
int fwgpu_batch_size(const fwgpu_batch *b, uint32_t *n_examples, uint64_t *n_lr, uint64_t *n_ffm);
/* Synchronous micro-batch: every example of the batch is scored with the weights of the batch start, then all updates are
 * applied (FWGPU_MODE_SEQUENTIAL: in example order; FWGPU_MODE_HOGWILD: concurrently).  This is the step the owner-sharded
 * multi-GPU mode (fwgpu_dist_*) runs across GPUs, and the mode in which a deep head trains mini-batched on the matrix cores.
 * fwgpu_split = the device buffers of one such batch (n_examples x {field sums, own slots, gradients}). */
typedef struct fwgpu_split fwgpu_split;
int fwgpu_split_create(fwgpu_regressor *r, uint32_t n_examples, uint32_t max_ffm_per_example, fwgpu_split **out);
int fwgpu_split_free(fwgpu_split *sp);
int fwgpu_learn_batch_sync(fwgpu_regressor *r, fwgpu_batch *b, fwgpu_split *sp, int mode, void *hip_stream);
/* predict-only launches of this batch start every example's field sums from this context cache (NULL detaches it); a record
 * batch needs a cache that went through fwgpu_block_cache_cover_record */
int fwgpu_batch_set_cache(fwgpu_batch *b, const fwgpu_block_cache *cache);
/* A context cache PER EXAMPLE: candidates of many requests in one launch.  `b` is an entry batch whose example i holds all LR entries
 * of its request and the FFM entries fwgpu_block_cache_filter(caches[cache_of_example[i]], ...) leaves (what an entry batch with
 * fwgpu_batch_set_cache holds, per request).  fwgpu_learn_batch(r, b, mode, update = 0, stream) then takes FWGPU_ROUTE_REQUESTS in
 * both modes (a predict-only launch has no order): the work per candidate follows the candidate's own features, not F * F * k.
 * update != 0 on such a batch is FWGPU_ERR_INVALID.  The pointer table and the index array are copied at the call; the caches are
 * referenced and must outlive the launches -- a cache refilled by fwgpu_setup_cache on the same handle is read as refilled, by the
 * next launch.  Like every change of a batch's contents, the call must not overlap a launch of the batch that is still in flight.
 * n_caches == 0 detaches; fwgpu_batch_set_cache on the same batch replaces the set, and the other way round.
 * FWGPU_ERR_INVALID, the batch left as it was: a record batch, an index >= n_caches, a cache of another regressor, a regressor with
 * a deep head or packed weights (without fwgpu_packed_enable_caches), a stale cache of a packed regressor, a batch with an oversize example, ffm_k % 4 != 0, an FFM row off the 16-byte boundary.  A launch
 * whose min(fields, largest FFM entry count of an example) * F * k floats exceed the 160 KiB LDS returns FWGPU_ERR_RANGE. */
int fwgpu_batch_set_caches(fwgpu_batch *b, const fwgpu_block_cache *const *caches, uint32_t n_caches,
                           const uint32_t *cache_of_example /* [examples of b] */);
/* Enqueue one pass over the batch on `stream`: for every example, Regressor::learn(fb, update)
 * (update=0: Regressor::predict).  Predictions land in the batch's device buffer. Asynchronous. */
int fwgpu_learn_batch(fwgpu_regressor *r, fwgpu_batch *b, int mode, int update, void *stream);
/* Copy the batch's predictions to the host (synchronises `stream`). */
int fwgpu_batch_predictions(fwgpu_batch *b, float *host_out, uint32_t n, void *stream);
/* Device pointer of the batch's prediction buffer (n_examples floats). */
int fwgpu_batch_predictions_device(fwgpu_batch *b, void **dev_ptr);

/* ---------------------------------------------------------------- record translation
 * FeatureBufferTranslator (feature_buffer.rs:33-44, 138-338) for primitive namespaces.
 * A translator describes which namespaces feed which LR combo / FFM field; namespaces are
 * identified by their index in the record (vwmap.rs:115-147). */
typedef struct fwgpu_translator_config {
    uint32_t n_combos;           /* feature_combo_descs.len() */
    const uint32_t *combo_off;   /* n_combos+1 offsets into combo_ns */
    const uint32_t *combo_ns;    /* namespace_index of each combo member */
    const uint8_t *combo_ns_f32; /* 1 if the namespace is NamespaceFormat::F32 */
    const float *combo_weight;   /* per combo */
    int32_t add_constant_feature;
    uint32_t n_fields;           /* ffm_fields.len() */
    const uint32_t *field_off;   /* n_fields+1 offsets into field_ns */
    const uint32_t *field_ns;
    const uint8_t *field_ns_f32;
    /* the ModelInstance fields FeatureBufferTranslator::new reads for its masks (feature_buffer.rs:138-148) */
    uint32_t bit_precision;
    uint32_t ffm_k;              /* 0: no ffm_buffer is produced */
    uint32_t ffm_bit_precision;
} fwgpu_translator_config;

/* lr_hash_mask / ffm_hash_mask as FeatureBufferTranslator::new computes them (feature_buffer.rs:138-148) */
uint32_t fwgpu_lr_hash_mask(uint32_t bit_precision);
uint32_t fwgpu_ffm_hash_mask(uint32_t ffm_bit_precision, uint32_t ffm_k);

/* Translate one record (parser.rs:57-74 layout) into caller-provided entry buffers (pure host code).
 * <= FeatureBufferTranslator::translate(record, example_number)   feature_buffer.rs:174-338 */
int fwgpu_translate(const fwgpu_translator_config *t, const uint32_t *record, uint32_t record_len, fwgpu_lr_entry *lr_out, uint32_t lr_cap, uint32_t *n_lr,
                    fwgpu_ffm_entry *ffm_out, uint32_t ffm_cap, uint32_t *n_ffm, float *label, float *importance);
/* Translate n back-to-back records (rec_off[i] = u32 offset of record i, n+1 entries) into a
 * device-resident batch. */
int fwgpu_batch_from_records(fwgpu_regressor *r, const fwgpu_translator_config *t, const uint32_t *records,
                             const uint64_t *rec_off, uint32_t n, fwgpu_batch **out);

/* Raw-record batch: the n records are copied to HBM as they are (4 x record_len bytes per example) and
 * FeatureBufferTranslator::translate (feature_buffer.rs:174-338) runs INSIDE the example kernel's stage phase, so the host
 * only validates the slot words.  Same results as fwgpu_batch_from_records, bit for bit. */
int fwgpu_record_batch_create(fwgpu_regressor *r, const fwgpu_translator_config *t, const uint32_t *records,
                              const uint64_t *rec_off, uint32_t n, fwgpu_batch **out);

/* ---------------------------------------------------------------- multi-GPU (replaces hogwild.rs:24-103 across GPUs)
 * One process per GPU over RCCL / xGMI.  fwgpu_dist_unique_id on one rank, the 128 bytes to every rank by any side channel
 * (the Rust caller of hogwild.rs:51-60 would use its own launcher's), then fwgpu_dist_init on every rank with its regressor
 * (every rank creates and initialises the SAME model: weight init is deterministic).
 *
 * fwgpu_dist_learn_sharded: the owner-sharded synchronous step.  Every rank owns a contiguous range of the FFM table and of
 * the LR table (fwgpu_dist_ranges) and brings a micro-batch of n records; the records are all-gathered, every rank gathers
 * the rows it owns for ALL examples, the partial field sums are reduce-scattered to the examples' home ranks, which compute
 * prediction and gradient; gradients and field sums are all-gathered and every rank applies the AdaGrad updates of the rows it
 * owns.  Semantics: fwgpu_learn_batch_sync with a micro-batch of n_ranks * n examples (every example sees the weights of the
 * step's start; per-occurrence AdaGrad on every row, as on one GPU).  Collective call: same n on every rank.
 * fwgpu_dist_gather_tables: every rank's owned range into every rank's tables (before saving or single-GPU prediction).
 * fwgpu_dist_all_reduce_sum: plain RCCL all-reduce of a device float buffer (replica mode: table deltas).
 * The fwgpu_dist_group_* functions run the same step with all ranks inside ONE process (collectives become device copies):
 * the tests and the single-box emulation of an N-GPU job use them. */
typedef struct fwgpu_dist fwgpu_dist;
typedef struct fwgpu_dist_group fwgpu_dist_group;
int fwgpu_dist_unique_id(uint8_t *id, uint64_t cap /* >= 128 */);
int fwgpu_dist_init(fwgpu_regressor *r, const uint8_t *unique_id, int rank, int n_ranks, fwgpu_dist **out);
int fwgpu_dist_free(fwgpu_dist *d);
/* FWGPU_MODE_HOGWILD (default): the examples of a phase run concurrently; FWGPU_MODE_SEQUENTIAL: in example order on one
 * workgroup (deterministic, for parity checks) */
int fwgpu_dist_set_mode(fwgpu_dist *d, int mode);
int fwgpu_dist_group_set_mode(fwgpu_dist_group *g, int mode);
/* Owner-side apply: sharded hogwild whose read-modify-writes never cross a link (what hogwild.rs:89-103 does with threads on one shared table,
 * with GPUs and owner-sharded tables): a rank FETCHES its examples' weight rows from their owners, and PUSHES one gradient row per occurrence
 * into a ring in the owner's memory; the owner runs the optimizer on its own tables.  fwgpu_dist_owner_attach maps tables and rings (rings sized
 * for steps of up to max_rows gradient rows / max_lr LR gradients per rank); fwgpu_dist_learn_owner is ONE COLLECTIVE STEP -- every rank calls
 * it, n may be 0 -- of push, count exchange, apply.  FWGPU_MODE_SEQUENTIAL with one example per step, ranks taking turns, is the sequential
 * reference.  The in-process group form takes every rank's micro-batch in one call. */
int fwgpu_dist_owner_attach(fwgpu_dist *d, uint32_t max_rows, uint32_t max_lr);
int fwgpu_dist_learn_owner(fwgpu_dist *d, const fwgpu_translator_config *t, const uint32_t *records, const uint64_t *rec_off, uint32_t n,
                           float *predictions, int update);
int fwgpu_dist_group_learn_owner(fwgpu_dist_group *g, const fwgpu_translator_config *t, const uint32_t *const *records,
                                 const uint64_t *const *rec_off, const uint32_t *n, float *const *predictions, int update);
/* STREAMING form of the owner-side apply: the owners drain their regions WHILE the sources' kernels fill them (a persistent consumer grid per owner,
 * circular regions, flow control through words the owner stores in the source's memory: no read-modify-write and no poll crosses a link), so that the
 * staleness of a gradient is the examples in flight -- as with hogwild.rs:89-103's threads -- whatever the step's size; the step-synchronous form above is
 * bounded to ~1024 global examples per step by stability.  HOGWILD only.  batches (or NULL): rank j's micro-batch already in HBM (a record batch of
 * its regressor; predictions land in the batch), else records / rec_off / n.  log2_rows / log2_lr: capacity of one (owner, source) region in gradient
 * rows / LR gradients (0: 2^15 / 2^16); consumer_workgroups: size of an owner's consumer grid (0: 48). */
int fwgpu_dist_group_learn_owner_stream(fwgpu_dist_group *g, const fwgpu_translator_config *t, const uint32_t *const *records, const uint64_t *const *rec_off,
                                        const uint32_t *n, fwgpu_batch *const *batches, float *const *predictions, int update, uint32_t log2_rows,
                                        uint32_t log2_lr, uint32_t consumer_workgroups);
/* ... and its process-per-rank form: fwgpu_dist_owner_stream_attach (collective, once) maps tables and the streaming regions of every rank;
 * fwgpu_dist_learn_owner_stream is ONE COLLECTIVE STEP (every rank calls it; n may be 0) with two small collectives (shapes, final positions). */
int fwgpu_dist_owner_stream_attach(fwgpu_dist *d, uint32_t log2_rows, uint32_t log2_lr);
int fwgpu_dist_learn_owner_stream(fwgpu_dist *d, const fwgpu_translator_config *t, const uint32_t *records, const uint64_t *rec_off, uint32_t n,
                                  float *predictions, int update, uint32_t consumer_workgroups);
int fwgpu_dist_rank(const fwgpu_dist *d, int *rank, int *n_ranks);
/* ranks of the job as the RCCL communicator itself counts them (ncclCommCount); 0 for a member of an in-process group */
int fwgpu_dist_comm_count(const fwgpu_dist *d, int *count);
int fwgpu_dist_ranges(const fwgpu_dist *d, uint32_t *ffm_lo, uint32_t *ffm_hi, uint32_t *lr_lo, uint32_t *lr_hi);
int fwgpu_dist_learn_sharded(fwgpu_dist *d, const fwgpu_translator_config *t, const uint32_t *records, const uint64_t *rec_off,
                             uint32_t n, float *predictions);
/* the same step with the rank's micro-batch already resident in HBM (a record batch): predictions land in the batch */
int fwgpu_dist_learn_sharded_batch(fwgpu_dist *d, const fwgpu_translator_config *t, fwgpu_batch *b);
int fwgpu_dist_gather_tables(fwgpu_dist *d);
int fwgpu_dist_all_reduce_sum(fwgpu_dist *d, float *device_buf, uint64_t count, void *hip_stream);
int fwgpu_dist_group_create(fwgpu_regressor *const *regressors, int n_ranks, fwgpu_dist_group **out);
int fwgpu_dist_group_free(fwgpu_dist_group *g);
int fwgpu_dist_group_learn_sharded(fwgpu_dist_group *g, const fwgpu_translator_config *t, const uint32_t *const *records,
                                   const uint64_t *const *rec_off, uint32_t n, float *const *predictions);
int fwgpu_dist_group_gather_tables(fwgpu_dist_group *g);
/* Row-sparse gradient buckets (north_star: "RCCL all-reduce of sparse gradient buckets"; replaces hogwild.rs:24-103's shared
 * table ACROSS GPUs): every rank keeps a full replica and scores its own micro-batch (any size) against it; the gradients of the
 * touched rows are summed per row on the rank (segment reduction over the sorted occurrence list), all-gathered as
 * {row hash, R-float gradient row} buckets, and every rank applies all buckets in the same order: ONE optimizer step per row and
 * global batch with the summed gradient.  Replicas that start identical stay bit-identical; there is no table exchange.
 * The update rule differs from the reference's (one step per occurrence): the oracle's fwo_learn_sparse restates it.
 * Models without a deep head.  Predictions: host buffer (may be NULL) / the batch's own. */
int fwgpu_dist_learn_sparse(fwgpu_dist *d, const fwgpu_translator_config *t, const uint32_t *records, const uint64_t *rec_off,
                            uint32_t n, float *predictions);
int fwgpu_dist_learn_sparse_batch(fwgpu_dist *d, const fwgpu_translator_config *t, fwgpu_batch *b);
/* bucket rows the rank sent in its last sparse step: FFM rows (4-byte key + R floats each) and LR entries (key + float) */
int fwgpu_dist_sparse_last_rows(const fwgpu_dist *d, uint32_t *ffm_rows, uint32_t *lr_rows);
/* in-process group: rank j brings n[j] records */
int fwgpu_dist_group_learn_sparse(fwgpu_dist_group *g, const fwgpu_translator_config *t, const uint32_t *const *records,
                                  const uint64_t *const *rec_off, const uint32_t *n, float *const *predictions);
/* Peer-sharded hogwild step (replaces hogwild.rs:24-103's shared table ACROSS GPUs with the reference's own update rule): the tables
 * are sharded by owner (rank s owns the FFM rows that START in its 1/N of 2^ffm_bits and the LR entries in its 1/N of 2^bits), every
 * rank runs the fused hogwild kernel on its own n[j] records and reaches each row IN ITS OWNER'S MEMORY -- a plain pointer on the
 * same device, a peer-mapped pointer over xGMI between the GPUs of one process.  No collective and no barrier between ranks:
 * per-occurrence AdaGrad steps, staleness = the examples in flight on all GPUs.  1, 2, 4 or 8 ranks; models without a deep head.
 * fwgpu_dist_group_set_mode(FWGPU_MODE_SEQUENTIAL): rank after rank, in example order -- the sequential reference algorithm over
 * the ranks' micro-batches in rank order (the deterministic form).  update = 0: predict only.  fwgpu_dist_group_gather_tables
 * afterwards gives every rank the whole model. */
int fwgpu_dist_group_learn_peer(fwgpu_dist_group *g, const fwgpu_translator_config *t, const uint32_t *const *records,
                                const uint64_t *const *rec_off, const uint32_t *n, float *const *predictions, int update);
/* The same mode with one PROCESS per rank (hogwild.rs:24-103 across the GPUs of a node, one process per GPU as RCCL jobs are launched):
 * fwgpu_dist_peer_attach -- collective, once -- exports this rank's tables as IPC handles (hipIpcGetMemHandle), all-gathers the handles
 * through the job's communicator and maps every other rank's tables (hipIpcOpenMemHandle: a peer GPU's memory over xGMI, or the same
 * device's when ranks share a GPU); fwgpu_dist_learn_peer then runs THIS rank's n records through the fused kernel, each row reached
 * in its owner's allocation -- not a collective, ranks run at their own pace; fwgpu_dist_barrier (collective) is where the caller
 * orders them: before fwgpu_dist_gather_tables, before a hold-out pass, or between ranks for a deterministic rank-after-rank run.
 * While the mode is on, a rank's OWNED range of the LR table lives in an allocation of its own (what the peers map: 1/N of the table --
 * hipIpcOpenMemHandle hangs on a 2 GiB allocation on ROCm 7.2); fwgpu_dist_gather_tables copies it back before it assembles the
 * tables, so fwgpu_predict / fwgpu_save on the rank's regressor see the trained LR weights only after that call. */
int fwgpu_dist_peer_attach(fwgpu_dist *d);
int fwgpu_dist_learn_peer(fwgpu_dist *d, const fwgpu_translator_config *t, const uint32_t *records, const uint64_t *rec_off, uint32_t n,
                          float *predictions, int update);
/* ... with the rank's micro-batch already in HBM (a record batch of its regressor); launched on hip_stream, or on the rank's own stream */
int fwgpu_dist_learn_peer_batch(fwgpu_dist *d, const fwgpu_translator_config *t, fwgpu_batch *b, int update, void *hip_stream);
int fwgpu_dist_barrier(fwgpu_dist *d);


/* ---------------------------------------------------------------- HogwildTrainer replacement
 * fwgpu_trainer_create  <= HogwildTrainer::new(regressor, &model_instance, num_workers)  hogwild.rs:24-49
 * fwgpu_digest_records  <= HogwildTrainer::digest_example(Vec<u32>)                      hogwild.rs:51-53
 *                          (n records per call; records are copied)
 * fwgpu_finish          <= HogwildTrainer::block_until_workers_finished                  hogwild.rs:55-60
 *                          (flushes the partial micro-batch and waits; the trainer stays usable)
 * Records are translated on the host, packed into micro-batches of `micro_batch` examples and run in
 * HOGWILD mode on an internal stream, double-buffered.  Like the reference, no predictions are
 * produced for hogwild-trained examples (main.rs:242-243). */
int fwgpu_trainer_create(fwgpu_regressor *r, const fwgpu_translator_config *t, uint32_t micro_batch,
                         fwgpu_trainer **out);
int fwgpu_digest_records(fwgpu_trainer *tr, const uint32_t *records, const uint64_t *rec_off, uint32_t n);
int fwgpu_finish(fwgpu_trainer *tr);
int fwgpu_trainer_free(fwgpu_trainer *tr);
int fwgpu_trainer_examples_seen(const fwgpu_trainer *tr, uint64_t *n);
/* The hold-out / test-only protocol of the reference's example loop (main.rs:184-185, 238-241, `--holdout_after N`, `-t`):
 * examples are numbered from 1 in the order they are digested; those numbered >= holdout_after (0 = none), or all of them
 * when testonly != 0, are predicted with update = false and never learned.  Their predictions are kept in stream order and
 * can be fetched after fwgpu_finish (out == NULL: count only).  Learned examples have no prediction here, like the
 * reference's hogwild branch (it prints 0.0, main.rs:242-243). */
int fwgpu_trainer_set_holdout(fwgpu_trainer *tr, uint64_t holdout_after, int testonly);
int fwgpu_trainer_predictions(fwgpu_trainer *tr, float *out, uint64_t cap, uint64_t *n);

/* ---------------------------------------------------------------- predicting with a model delayed by N examples
 * `--prediction_model_delay N` (cmdline.rs:284-289, main.rs:200-258): labels arrive late, so example i (from 1) is predicted by a model
 * that has learned nothing newer than example i - 1 - N.  The reference's loop for N > 0:
 *     if i > predictions_after: prediction = learn(example i, update = false)
 *     push example i;  if the queue is longer than N: pop the oldest (example i - N) and learn it
 * and at the end of input the queue is dropped: the last N examples are never learned.
 *
 * fwgpu_trainer_set_delay: delay == 0 (the default) leaves the trainer what it is without this call -- same launches, same bits;
 *   delay > 0 turns the delayed protocol on for every route (fwgpu_digest_records, _digest_cache, _digest_text, _digest_file and the
 *   device text route).  FWGPU_ERR_INVALID once examples have been digested, and together with holdout_after > 0 or testonly in either
 *   call order (fwgpu_trainer_set_holdout refuses likewise while a delay is set): the reference's command line declares that conflict
 *   and its delayed loop ignores holdout_after; this library refuses instead of ignoring.
 *
 * The window rule.  The trainer works in launch windows: a window holds at most micro_batch consecutive examples, no window straddles
 * predictions_after, fwgpu_finish closes a partial one (the device text route also closes one at the end of every piece of text).  When
 * the window that ends at example e has been taken:
 *   1. if its examples are numbered > predictions_after, a predict-only launch scores it (update = 0, FWGPU_MODE_HOGWILD, the route
 *      fwgpu_learn_batch picks);
 *   2. those predictions are appended to the list fwgpu_trainer_predictions returns, in stream order;
 *   3. its record batch joins a ring in device memory: records do not come back to the host for their second visit;
 *   4. every pending window whose LAST example is numbered <= e - delay is learned, oldest first, one learn launch each, on the same
 *      stream, and leaves the ring.
 * Nothing else learns.  Hence, for every predicted example i:
 *   - its model has learned NO example numbered above i - 1 - delay: it is never fresher than the reference's;
 *   - its model has learned every example up to i - 1 - delay - (2 * micro_batch - 2) at least;
 *   - with micro_batch == 1 the trainer IS the reference's loop.
 * After fwgpu_finish the pending windows stay pending -- at least `delay` examples are unlearned (all of them, if fewer were digested),
 * like the reference at the end of input -- and the trainer stays usable: further digests continue the same stream and the same ring.
 * fwgpu_trainer_free drops the ring.
 *
 * The ring holds about delay + 2 * micro_batch examples' records.  Learned batches are refilled, so a steady stream allocates nothing.
 * A failed allocation is FWGPU_ERR_DEVICE with the sizes in the message; that window is dropped (fwgpu_trainer_examples_seen does not
 * count it) and the trainer stays usable for fwgpu_finish / fwgpu_trainer_free.  A window with an oversize example keeps the host's
 * translation with its batch and takes the example-by-example route on both visits.
 * Metrics (fwgpu_trainer_set_metrics): a window's predict launch is scored on the LEARNED side -- progressive predictions of examples
 * that will be learned; its later learn launch is not scored (an example counts once); examples <= predictions_after are not scored.
 *
 * fwgpu_trainer_delay_state (any pointer may be NULL): the last example number learned (0: none), the examples and windows pending in
 *   the ring (an open micro-batch still on the host is not among them), and the bytes of device memory the ring's batches take.
 * fwgpu_debug_delay_plan: the eligibility rule alone, on the host: given the windows' last example numbers (growing, from 1) and a
 *   delay > 0, learned_through_after[j] = the last example number learned once window j's step is done (0: none yet). */
int fwgpu_trainer_set_delay(fwgpu_trainer *tr, uint64_t delay, uint64_t predictions_after);
int fwgpu_trainer_delay_state(const fwgpu_trainer *tr, uint64_t *learned_through, uint64_t *pending_examples, uint64_t *pending_windows,
                              uint64_t *ring_bytes);
int fwgpu_debug_delay_plan(const uint64_t *window_last, uint32_t n_windows, uint64_t delay, uint64_t *learned_through_after);

/* ---------------------------------------------------------------- progressive and hold-out loss, scored on the device
 * The reference's example loop has a prediction for every example, made BEFORE the example is learned (main.rs:246) and written out
 * (main.rs:260-268); the loss of those predictions is benchmark/calc_loss.py's.  Here a kernel (csrc/metrics.hip) scores the
 * predictions a launch left in its batch against the batch's own labels, on the device: no prediction and no label crosses to the host.
 * Per example, in f64: p = clip((double)pred, 1e-15, 1 - 1e-15), loss = label == 1 ? -log(p) : -log(1 - p).  An example whose label is
 * the parser's NO_LABEL (parser.rs:28: 0xff, 255.0f) counts in n_unlabelled; otherwise one whose prediction is not finite counts in
 * n_bad; neither enters a sum or a histogram.  Examples are numbered from 1; window w of size W covers the numbers w * W + 1 .. (w + 1) * W,
 * and every window has a learned and a held-out side.  Integer fields and histograms are exact; the f64 sums are accumulated with
 * atomic adds, so their last bits depend on the order of arrival. */
typedef struct fwgpu_metric_sums {
    uint64_t n, n_unlabelled, n_bad;       /* scored / NO_LABEL / prediction not finite */
    double sum_importance, sum_loss;       /* sum_loss: importance * loss */
    double sum_loss_plain, sum_pred, sum_label;
} fwgpu_metric_sums;
typedef struct fwgpu_metric_window {
    uint64_t first_number;                 /* the window's first stream number */
    fwgpu_metric_sums learned, held_out;
} fwgpu_metric_window;
/* hist[c * 256 + b]: scored examples of class c (1: label == 1, 0: the rest) whose raw f32 prediction falls into bin
 * b = min(255, (int)(pred * 256)) of 256 equal bins over [0, 1]: calibration and a binned AUC without a label on the host */
typedef struct fwgpu_metric_total {
    fwgpu_metric_sums sums;
    uint64_t hist[512];
} fwgpu_metric_total;
/* fwgpu_batch_metrics <= benchmark/calc_loss.py on the predictions of main.rs:246: scores the current predictions of the batch's
 *   examples first .. first + n - 1 (entry batches: the batch's label / importance arrays; record batches: the records' words 1 and 2,
 *   feature_buffer.rs:187-189) on `stream`, waits for it and returns one set of sums and, if hist512 is not NULL, that histogram.
 *   `learned` is not interpreted here.  FWGPU_ERR_RANGE: first + n beyond the batch.
 * fwgpu_trainer_set_metrics <= the progressive validation of main.rs:246, 260-268: window > 0 turns scoring on, every launch of the
 *   trainer (learn and predict-only, on every route) is followed by the metrics kernel on the trainer's stream; 0 (the default) is off.
 *   FWGPU_ERR_INVALID once examples have been digested.
 * fwgpu_trainer_metrics: after fwgpu_finish, the windows scored so far (rows == NULL: *n_rows only; cap < *n_rows: FWGPU_ERR_RANGE) and
 *   the running totals of the learned and of the held-out examples (either may be NULL).  Metrics off: no rows, zero totals. */
int fwgpu_batch_metrics(fwgpu_batch *b, uint32_t first, uint32_t n, int learned, fwgpu_metric_sums *out, uint64_t *hist512, void *stream);
int fwgpu_trainer_set_metrics(fwgpu_trainer *tr, uint64_t window);
int fwgpu_trainer_metrics(fwgpu_trainer *tr, fwgpu_metric_window *rows, uint64_t cap, uint64_t *n_rows, fwgpu_metric_total *learned,
                          fwgpu_metric_total *held_out);

/* ---------------------------------------------------------------- launch tuning (optional)
 * threads: workgroup size (multiple of 64, <=1024); workgroups_per_cu: persistent grid = CUs*this.
 * 0 keeps the default.  Does not change results in SEQUENTIAL mode. */
int fwgpu_set_launch(fwgpu_regressor *r, uint32_t threads, uint32_t workgroups_per_cu);
/* The graph wiring of a live regressor (a model file carries none: a loaded regressor starts as FWGPU_WIRING_REGRESSOR).  Takes effect at the
 * next launch; batches made before the call keep their entries. */
int fwgpu_set_wiring(fwgpu_regressor *r, int wiring);
/* HOGWILD launches process as many examples concurrently as the device holds workgroups (768 on MI355X at config C).  On a
 * small or tiny-example data set that much staleness keeps the model from learning (hogwild.rs runs 16 threads): n caps
 * the examples in flight, n = 16 is the reference's default degree of concurrency, n = 1 is its single-thread loop (one
 * workgroup walks the stream in order: identical to FWGPU_MODE_SEQUENTIAL), 0 = no cap. */
int fwgpu_set_max_in_flight(fwgpu_regressor *r, uint32_t n_examples);

/* ---------------------------------------------------------------- multi-GPU replica bookkeeping (device pointers)
 * Data-parallel replicas exchange what each changed since the last agreed snapshot (replaces hogwild.rs's shared
 * memory across GPUs; the all-reduce itself is RCCL via torch.distributed, see fwumious_wabbit_amd/dist_sync.py):
 *   fwgpu_delta_start : local_delta = table - snapshot ; summed_delta = scale * local_delta
 *                       (summed_delta is then all-reduced in place; scale = 1/world_size makes the sum the MEAN of the
 *                        replicas' deltas, which is what keeps N >= 4 replicas from diverging: scripts/replica_sim.py)
 *   fwgpu_delta_finish: snapshot += summed_delta ; table += summed_delta - local_delta
 * One fused pass each over n_floats elements, enqueued on `stream`. */
int fwgpu_delta_start(const void *table, const void *snapshot, void *local_delta, void *summed_delta, uint64_t n_floats,
                      float scale, void *stream);
int fwgpu_delta_finish(void *table, void *snapshot, const void *local_delta, const void *summed_delta, uint64_t n_floats,
                       void *stream);

/* ---------------------------------------------------------------- diagnostics
 * Cross-XCD visibility probe for the access pattern the HOGWILD mode relies on: one workgroup publishes a
 * 1 KiB payload `iters` times (sc1 or plain stores), 15 workgroups spread over the XCDs re-read it (sc1 or
 * plain loads) after a device-scope flag and count words older than the flag.  With use_sc1=1 the count must
 * be 0; with use_sc1=0 it shows the hazard the kernels avoid. */
/* Per-phase shader-clock accounting of the example kernel (debug): enable=1 allocates/zeroes 8 device counters that
 * every workgroup's thread 0 adds to: [0] stage entries, [1] field boundaries + overlap scan, [2] row gather,
 * [3] dot + LR forward + sigmoid, [4] LR update, [5] FFM update, [6] wait for the slowest wave, [7] examples.
 * out16 (may be NULL) receives the counters accumulated so far.  The stamps are compiled into -DFW_TICKS builds of kernels.hip only
 * (scripts/build_variant.sh ticks -DFW_TICKS; scripts/perf_probe.py): the shipped kernels add nothing, the counters stay 0.  Slots 12-14 (large-table kernel): every
 * wave's wait at the barrier behind the gather, its wait at the loop-top barrier, and its whole example, each summed over all waves. */
int fwgpu_debug_phase_ticks(fwgpu_regressor *r, int enable, uint64_t *out16);
/* How the FFM accumulator table was placed relative to the weight table (fwgpu_create tries a few candidate allocations for
 * tables beyond the Infinity Cache and times the update's access pattern on each pair; FWGPU_PLACEMENT=0 disables it):
 * candidates tried (1: no search), fastest and slowest pair probe in milliseconds (0 when nothing was timed). */
int fwgpu_debug_placement(const fwgpu_regressor *r, int *tries, float *ms_fastest, float *ms_slowest);
/* 0 = automatic kernel choice, 1 = force the generic kernel (v1), 2 = register-resident rows (v2) where applicable. */
int fwgpu_debug_set_kernel_version(fwgpu_regressor *r, int version);
/* Tuning switches for experiments.  option 1: value 1 = read the AdaGrad LUT from global memory instead of an LDS copy.
 * option 2: the update path of large models (k % 4 == 0, rows of at most 256 floats): 0 = float-granular row updates, rows repeated
 *   inside an example serialised on one wave (the round-1 path); 1 = automatic (default): tables beyond the Infinity Cache take the
 *   chained path (repeated rows applied by their first occurrence's wave, from registers), with whole-128-byte-line accesses only
 *   when the accumulator table could not be placed away from the weight table; 2 = chained path with whole-line accesses, always;
 *   3 = chained path with float-granular accesses, always (what large tables run when the placement search succeeded, on any table).
 * option 3: value 1 = no duplicate-row chains (A/B runs).
 * option 4: HOGWILD launches step the constant feature's LR entry (in every example, feature_buffer.rs:270-276) with atomics: the
 *   step is taken at the accumulator the example's forward pass read + its own g^2, `acc += g^2` and `w -= step` are added to the
 *   table by float atomics.  value 1 (default): both per example; value n > 1: a workgroup's WEIGHT deltas stay pending in LDS for
 *   n of its examples; 0 = plain per-example read-modify-writes, which serialise on that one entry and overwrite each other.
 *   SEQUENTIAL launches never use it.
 * option 5: store policy of the FFM row stores in HOGWILD launches of that update path: 0 = both tables device-scope write-through,
 *   1 = weight rows write-back through the XCD's L2, 2 = both tables write-back, 3 (the default since round 5) = 1 with thinned accumulator stores on hot
 *   register-kept rows (one example in eight stores eight times its g^2: DESIGN 4.2), 4 = 3 with the thinned store replaced by a thinned device-scope
 *   atomic add (one example in eight adds eight times its g^2, on every hot row of the example: nothing is lost to a concurrent writer); -1 = the build's
 *   default.  option 9: policies 3 / 4 call a row hot once its accumulators have grown by more than value / 1024 (-1 = default: 0.5); option 10: one example in
 *   2^value touches a hot row's accumulators (0..6; -1 = default: 3).  option 6: with
 *   policy 1 / 2 a workgroup writes its XCD's dirty L2 lines back every `value` of its examples (0 = only when the launch ends; -1 = the
 *   build's default: 128) -- the bound on how long a popular row can stay private to one XCD (DESIGN.md 4.2,
 *   tests/test_gpu_conservation.py).  SEQUENTIAL launches are exact under every policy.
 * option 15: store policy 4 thins a hot row's adds by the row's heat: 1 = a row whose accumulators have grown by more than 8 / 16 / 32 times option 9's threshold is touched by
 *   one example in 2^(option 10's value + 1 / 2 / 3), 64 at the most (csrc/hot_tiers.h); 0 = every hot row at option 10's exponent; -1 = default (FWGPU_ACC_TIERS).
 * option 13: rows the large-table kernel keeps from the gather (20 in registers + 3 in LDS per wave, written back as w_gather - step): 1 (default, -1) = kept; 0 = none, every row is
 *   re-read by the update (14 % slower; without the damping of rows many concurrent examples hold -- on BASELINE configs[2]'s stream the reference's own hold-out curve).
 * option 12: store policy 4 also on hot LR entries of that kernel (the weight stored alone, the accumulator by thinned atomic adds): 1 (default, -1) / 0.
 * option 11: HOGWILD launches of a model with a deep head and rows of 257..512 floats (BASELINE config E: k = 16 at 30 fields): 1 (default, -1) = the head runs
 *   as a phase of the large-table kernel, two 512-thread workgroups per CU, where they fit; 0 = always on the generic kernel (one 1024-thread workgroup per CU).
 *   SEQUENTIAL launches take the generic kernel (the parity mode) unless value 2 forces them onto the large-table kernel too (tests of that kernel's head phase).
 * option 14: predict-only HOGWILD batches of 256 or more examples of a model with a deep head: 1 (default, -1) = the batched route (the example kernel leaves every example's
 *   head input in a batch buffer, the layers run as GEMMs over slabs of examples: DESIGN.md 4.4) where the shape allows it; 0 = the per-example forward for every launch.
 *   -1 follows FWGPU_HEAD_PREDICT_PER_EXAMPLE (set: per example), a value set here overrides it.
 * option 7: value 0 = the updating launches do not prefetch the next example's record (A/B runs; default 1).
 * option 8: rows per wave, beyond the 20 kept in registers, whose gather-time weights are parked in LDS for the update phase instead of
 *   being re-read (config-C-shaped rows on the chained path): 0..3, -1 (default) = as many as still let two workgroups share a CU.
 * (The update path of option 2 = 1 / 2 keeps the first 20 rows of every wave's share of an example from the gather and writes
 *   them back as w_gather - step in HOGWILD launches: what the concurrent mode's hold-out loss rests on) */
int fwgpu_debug_set_option(fwgpu_regressor *r, int option, int value);
/* Which path the regressor's last fwgpu_learn_batch took (read-only; the single-example calls do not change it): */
#define FWGPU_ROUTE_NONE 0                 /* no batch launch yet, or an empty batch */
#define FWGPU_ROUTE_FUSED 1                /* the fused example kernel, the deep head (if any) per example inside it */
#define FWGPU_ROUTE_HEAD_BATCHED 2         /* predict-only batch of a deep head: head inputs to a batch buffer, layers as GEMMs (option 14); with or without a
                                            * context cache (fwgpu_batch_set_cache: filtered entries, records with covered slots, candidate-only records) */
#define FWGPU_ROUTE_HEAD_BATCHED_REFUSED 3 /* ... which refused the batch's shape (FWGPU_ERR_RANGE); the batch was re-run on the fused example kernel, per example */
#define FWGPU_ROUTE_PACKED 4               /* packed regressor: the packed predict kernel (or its refusal) */
#define FWGPU_ROUTE_HOST_WALK 5            /* a batch with an oversize example: walked example by example from its host copy */
#define FWGPU_ROUTE_REQUESTS 6             /* predict-only entry batch with a cache per example (fwgpu_batch_set_caches) */
int fwgpu_debug_last_route(const fwgpu_regressor *r, int *route);
/* What the regressor's last example-kernel launch ran, from its RESOLVED launch parameters (host side, read-only; every batch launch that reaches the
 * example kernel records it, the launch of a refused batch does not): the first n <= FWGPU_LAUNCH_INFO_LEN of
 *   [0] kernel family (FWGPU_KERNEL_*; -1: no launch yet)   [1] chunks per row: ceil(R / 64) on the scalar kernel, ceil(R / 256) on the 16-byte kernels
 *   [2] window (the chained whole-row update path)          [3] chain (duplicate rows chained to their first occurrence)
 *   [4] no_kept_rows (option 13 = 0)                        [5] lds_keep (rows per wave parked in LDS, after clamping)
 *   [6] threads per workgroup                               [7] LDS bytes per workgroup
 * FWGPU_KERNEL_PACKED: [0], [1] and [6] as above ([1]: ceil(R / 256), the packed kernel's one or two chunks); [2]..[5] describe update paths a
 * predict-only kernel does not have and are 0; [7] is 0 (the packed launch sizes its LDS itself, it is not reported). */
#define FWGPU_KERNEL_SCALAR 0   /* generic kernel, one float per lane (k % 4 != 0, or an entry batch with a row off a 16-byte boundary) */
#define FWGPU_KERNEL_VEC4 1     /* generic kernel, 16 bytes per lane */
#define FWGPU_KERNEL_RESIDENT 2 /* register-resident kernel (rows of up to 256 floats, or up to 512 where 256 % k == 0) */
#define FWGPU_KERNEL_PACKED 3   /* ... its predict-only instantiation on a packed table */
#define FWGPU_KERNEL_REQUESTS 4 /* the requests kernels (FWGPU_ROUTE_REQUESTS): [1] = ceil(R / 256), [6] = threads per workgroup, [7] = LDS bytes, [2]..[5] = 0 */
#define FWGPU_KERNEL_PACKED_REQUESTS 5 /* ... their instantiation on a packed table (fwgpu_packed_enable_caches); the fields as FWGPU_KERNEL_REQUESTS */
#define FWGPU_LAUNCH_INFO_LEN 8
int fwgpu_debug_last_launch(const fwgpu_regressor *r, int32_t *out, uint32_t n);
/* The head inputs x = [per-combo LR sums | triangle of the FFM pair outputs] (n examples x X floats, example-major) that the last batched head predict
 * launch left on the device: the first n_floats of them to `out`.  FWGPU_ERR_INVALID unless the last batch launch took FWGPU_ROUTE_HEAD_BATCHED,
 * FWGPU_ERR_RANGE beyond n * X.  Waits for the device. */
int fwgpu_debug_head_inputs(fwgpu_regressor *r, float *out, uint64_t n_floats);
/* an f32 as serde_json / ryu prints it in the embedded JSON documents ("0.1", "1.0", "1e-7"); NUL-terminated */
int fwgpu_debug_format_f32(float v, char *buf, uint32_t cap);
int fwgpu_debug_coherence_probe(int device, int use_sc1, uint32_t iters, uint32_t *stale_words, uint32_t *timeouts);
/* One product of the mini-batched head (head.hip) on device pointers, for tests against a plain f32 reference:
 * C[M, N] = op(A) . op(B) with A(m, k) = ta ? A[k * lda + m] : A[m * lda + k], B(k, n) = tb ? B[n * ldb + k] : B[k * ldb + n]; epilogue 0: C = acc,
 * 1: C = relu(acc + bias[n]) with the 0 / 1 mask in aux, 2: C = acc * aux[m, n], 3: C += acc.  tiled != 0 forces the LDS-tiled 64 x 64 kernel;
 * otherwise the split-K kernel runs where K % 8 == 0 and the operands allow 16-byte loads.  The three (ta, tb) pairs the head uses: (0, 1), (1, 0), (0, 0). */
int fwgpu_debug_head_gemm(const float *A, const float *B, float *C, int M, int N, int K, int lda, int ldb, int ldc, int ta, int tb, int epilogue,
                          const float *bias, float *aux, int relu, int tiled, void *stream);
/* One training (update != 0) or predict-only step of the mini-batched head (head.hip head_step) on the regressor's current dense weights, for tests
 * against a float64 reference (tests/head_ref.py head_train64): host x[n * X] and yi[2 n] ({label, importance} pairs) are copied to device buffers of
 * their own -- allocated as a micro-batch's are, so every product takes the kernel it takes in training -- the step runs, the stream is waited for,
 * and the step's buffers come back to the host: pred[n], gvec[n] (the general gradients), per layer and back to back h, mask [n * out_l]; with update
 * also dz (like h), dx[n * X] and dW[nn_len], the gradient sums in TABLE_NN_W layout as the optimizer step saw them.  An example whose general
 * gradient is 0 learns nothing: its rows of h come back as zeros after a training step.  NULL outputs are skipped; step_ms: the step's kernels
 * between two events.  The dense weights and accumulators before and after: fwgpu_table_read / fwgpu_table_write on TABLE_NN_W / TABLE_NN_ACC. */
int fwgpu_debug_head_step(fwgpu_regressor *r, const float *x, const float *yi, uint32_t n, int update, float *pred, float *gvec, float *dx,
                          float *dW, float *h, float *mask, float *dz, float *step_ms, void *stream);
/* The reduce and apply steps of the row-sparse gradient buckets (sparse.hip) on device pointers, for tests against a plain f32 restatement
 * (tests/sparse_ref.py): the calls only fill the argument structs of the multi-GPU step, allocate its scratch buffers and wait for the stream.
 * reduce: keys[n] = (hash << 32 | slot) or ~0 (padding) in any order, key_bits = 32 + bits of the largest hash; desc[slot] = {value bits, field};
 *   slot = example * max_entries + entry.  R != 0 (FFM): split[example * split_len + field * R + e], selfw[example * selfw_stride + entry * k + e % k],
 *   gbuf[example]; the 16-byte kernel runs where k % 4 == 0 and split_len % 4 == 0 (split, bk_rows 16-byte aligned).  R == 0 (LR): one float per bucket
 *   row, split / selfw unused.  Out: bk_key[rows], bk_rows[rows * max(R, 1)] on the device, *count = rows on the host.
 * apply: all_key / all_rows hold n_ranks * stride bucket rows of which rank r's first counts[r] (device) are valid; one rank's keys must be sorted by
 *   (hash, index).  R != 0: tables w / acc, k4 != 0 = the 16-byte kernel (R % 4 == 0; w, acc, all_rows and every hash on 16-byte boundaries);
 *   R == 0: w = the {w, acc} pair table, acc unused.  lut: 2048 floats on the device.
 * FWGPU_ERR_INVALID: a null pointer, k == 0 with R != 0, R % k != 0, k4 with R % 4 != 0.  Alignment and table bounds are the caller's. */
int fwgpu_debug_sparse_reduce(const void *keys, uint32_t n, int key_bits, const void *desc, uint32_t max_entries, uint32_t R, uint32_t k,
                              const float *split, uint32_t split_len, const float *selfw, uint32_t selfw_stride, const float *gbuf, uint32_t *bk_key,
                              float *bk_rows, uint32_t *count, void *stream);
int fwgpu_debug_sparse_apply(const uint32_t *all_key, const float *all_rows, const uint32_t *counts, uint32_t n_ranks, uint32_t stride, int key_bits,
                             uint32_t R, uint32_t k4, float *w, float *acc, int optimizer, float rate, float minus_power_t, const float *lut,
                             void *stream);
/* The metrics kernel (metrics.hip) alone on host arrays, for tests against a float64 restatement (tests/metrics_ref.py): pred, label,
 * importance [n] and learned [n] (0: held out) go to device buffers, the examples are numbered first_number .. first_number + n - 1
 * (first_number >= 1) and scored in launches of at most `launch` examples (0: one launch) into a window table that starts empty and grows
 * as a trainer's does.  Out: the windows from first_number's to the last example's (cap < *n_rows: FWGPU_ERR_RANGE; rows == NULL: the
 * count only) and the two totals (either may be NULL).  window == 0 is FWGPU_ERR_INVALID. */
int fwgpu_debug_metrics(const float *pred, const float *label, const float *importance, const uint8_t *learned, uint64_t first_number,
                        uint32_t n, uint64_t window, uint32_t launch, fwgpu_metric_window *rows, uint64_t cap, uint64_t *n_rows,
                        fwgpu_metric_total *learned_total, fwgpu_metric_total *held_out_total, void *stream);

/* ---------------------------------------------------------------- feed path: namespace map, VW text parser, input cache
 * (SURVEY.md 8 f1/f3).  Host-side code; none of it needs a device.
 *
 * vw_namespace_map.csv (vwmap.rs:106-151): "vwname,verbose[,f32]" per line, namespace_index = line number,
 * optional "_namespace_skip_prefix,N".  The JSON form is serde_json::to_vec_pretty(vw_source) as embedded in cache and
 * model files (persistence.rs:36-53); fwgpu_vwmap_to_json reproduces it byte for byte (buf == NULL: size query). */
typedef struct fwgpu_vwmap fwgpu_vwmap;
int fwgpu_vwmap_from_csv(const char *csv, uint64_t len, fwgpu_vwmap **out);
int fwgpu_vwmap_from_json(const char *json, uint64_t len, fwgpu_vwmap **out);
void fwgpu_vwmap_free(fwgpu_vwmap *vw);
uint32_t fwgpu_vwmap_num_namespaces(const fwgpu_vwmap *vw); /* max namespace_index + 1 (vwmap.rs:83-88) */
uint32_t fwgpu_vwmap_num_entries(const fwgpu_vwmap *vw);
int fwgpu_vwmap_to_json(const fwgpu_vwmap *vw, char *buf, uint64_t cap, uint64_t *len);
/* name -> namespace_index / format; verbose != 0 looks the verbose name up (map_verbose_to_namespace_descriptor) */
int fwgpu_vwmap_lookup(const fwgpu_vwmap *vw, const char *name, uint64_t len, int verbose, uint32_t *index,
                       uint32_t *is_f32);

/* VowpalParser (parser.rs:24-461).  fwgpu_parser_parse_line = next_vowpal_to_size on one line as read_until(b'\n')
 * delivers it (the newline, when present, is part of `line`); the record (parser.rs:57-74) is copied to `out`
 * (out == NULL: only *n_words).  len == 0 -> end of stream, *n_words = 0.  Returns FWGPU_OK, FWGPU_PARSE_FLUSH,
 * FWGPU_PARSE_HOGWILD_LOAD (file name via fwgpu_parser_command_argument) or FWGPU_ERR_PARSE with the reference's
 * message in fwgpu_last_error().  fwgpu_parser_parse_with_prefix = next_vowpal_with_cache (parser.rs:195-211): the
 * cached context bytes followed by the request's bytes.  fwgpu_parser_parse_buffer parses many lines into records laid
 * out back to back (rec_off: n_records + 1 word offsets), stopping at max_records, a full buffer, or the first line
 * that is not an example (*consumed = bytes fully parsed; the return value says why it stopped). */
typedef struct fwgpu_parser fwgpu_parser;
int fwgpu_parser_create(const fwgpu_vwmap *vw, fwgpu_parser **out);
void fwgpu_parser_free(fwgpu_parser *p);
int fwgpu_parser_parse_line(fwgpu_parser *p, const char *line, uint64_t len, uint32_t *out, uint32_t cap, uint32_t *n_words);
int fwgpu_parser_parse_with_prefix(fwgpu_parser *p, const char *prefix, uint64_t prefix_len, const char *line, uint64_t len,
                                   uint32_t *out, uint32_t cap, uint32_t *n_words);
/* The same result as fwgpu_parser_parse_with_prefix(prefix, line) for every line, without scanning the context again per
 * request (lib.rs:88-108 scans context + candidate every time): the context is scanned once up to its last token boundary,
 * requests resume there.  Contexts that cannot be resumed (fwgpu_parse_prefix_resumable == 0) take the concatenating route. */
typedef struct fwgpu_parse_prefix fwgpu_parse_prefix;
int fwgpu_parse_prefix_create(fwgpu_parser *p, const char *prefix, uint64_t len, fwgpu_parse_prefix **out);
void fwgpu_parse_prefix_free(fwgpu_parse_prefix *px);
int fwgpu_parse_prefix_resumable(const fwgpu_parse_prefix *px);
int fwgpu_parser_parse_after_prefix(fwgpu_parser *p, const fwgpu_parse_prefix *px, const char *line, uint64_t len, uint32_t *out,
                                    uint32_t cap, uint32_t *n_words);
/* Candidate-only records.  When the scanned part of the context is all of it (fwgpu_parse_prefix_is_record: its output buffer
 * equals the context's own record), fwgpu_parser_parse_candidate returns what the request ADDED to that record (*is_delta = 1):
 * header, a slot word per namespace the request filled (every other slot NO_FEATURES = "as in the context"), the request's
 * feature words.  A request that continues a namespace the context began comes back merged (*is_delta = 0). */
int fwgpu_parse_prefix_is_record(const fwgpu_parse_prefix *px, const uint32_t *record, uint32_t len);
int fwgpu_parser_parse_candidate(fwgpu_parser *p, const fwgpu_parse_prefix *px, const char *line, uint64_t len, uint32_t *out,
                                 uint32_t cap, uint32_t *n_words, int *is_delta);
const char *fwgpu_parser_command_argument(const fwgpu_parser *p);
int fwgpu_parser_parse_buffer(fwgpu_parser *p, const char *text, uint64_t len, uint32_t *words, uint64_t words_cap,
                              uint64_t *rec_off, uint64_t max_records, uint64_t *n_records, uint64_t *n_words,
                              uint64_t *consumed);

/* ---------------------------------------------------------------- VW text parsed on the device (parser.rs:214-461)
 * The scan of next_vowpal_to_size runs in HIP kernels (csrc/textparse.hip): line index, one wavefront per line, records laid out
 * word for word as the host parser lays them out.  A line that is not a plain example the kernel reproduces exactly (a command, an
 * error, NONE / inf / nan, a number it cannot prove correctly rounded, an undeclared namespace, more than 64 KiB, ...) is parsed by
 * the host parser instead, so fwgpu_text_parser_parse_buffer is fwgpu_parser_parse_buffer on every input: words, rec_off, counts,
 * consumed, return code, fwgpu_last_error() and the command argument (fwgpu_text_parser_command_argument).  The text goes up in
 * chunks cut at line breaks through pinned staging: len is not bounded.  fwgpu_text_parser_last_lines: lines the last call took, and
 * how many of them the host parsed. */
typedef struct fwgpu_text_parser fwgpu_text_parser;
int fwgpu_text_parser_create(const fwgpu_vwmap *vw, int device, fwgpu_text_parser **out);
void fwgpu_text_parser_free(fwgpu_text_parser *tp);
int fwgpu_text_parser_parse_buffer(fwgpu_text_parser *tp, const char *text, uint64_t len, uint32_t *words, uint64_t words_cap,
                                   uint64_t *rec_off, uint64_t max_records, uint64_t *n_records, uint64_t *n_words,
                                   uint64_t *consumed);
int fwgpu_text_parser_last_lines(const fwgpu_text_parser *tp, uint64_t *lines, uint64_t *host_lines);
const char *fwgpu_text_parser_command_argument(const fwgpu_text_parser *tp);
/* Every line of `text` as one candidate of a context: fwgpu_parser_parse_candidate(px, line) line by line, no line stops the walk.
 * `cache` is the context's cache (it went through fwgpu_block_cache_cover_record) and `px` the scan of the same context whose output is
 * that record (fwgpu_parse_prefix_is_record); anything else, or a parser on another device, is FWGPU_ERR_INVALID.  A line that starts
 * with '|' is scanned by the device: its candidate-only record is its stand-alone record with the context record's words 1 and 2 and
 * NO_FEATURES in every slot whose merged form equals the context's slot word.  Every other line (a feature token that goes on in the
 * context's last namespace, a label, an empty line, what the kernel leaves to the host in any mode) goes through
 * fwgpu_parser_parse_candidate.  Per line: code = that function's return code, rec_off[i] .. rec_off[i + 1] = its record in `words` (no
 * words for an error or an empty record), is_delta, n_lr / n_ffm = the entry counts of its translation on top of the context's record,
 * record_ok = fwgpu_block_cache_record_ok for the record in the form it has (0 when the record does not count), by_host = 1 when the
 * host parsed it.  FWGPU_ERR_RANGE: more than max_lines lines or more than words_cap words. */
typedef struct fwgpu_candidate_info {
    int32_t code;
    uint8_t is_delta, record_ok, by_host, pad;
    uint32_t n_lr, n_ffm;
} fwgpu_candidate_info;
int fwgpu_text_parser_parse_candidates(fwgpu_text_parser *tp, const fwgpu_parse_prefix *px, const fwgpu_block_cache *cache,
                                       const struct fwgpu_translator_config *t, const char *text, uint64_t len, uint64_t max_lines,
                                       uint32_t *words, uint64_t words_cap, uint64_t *rec_off, fwgpu_candidate_info *info,
                                       uint64_t *n_lines, uint64_t *n_words);
/* Text -> raw-record batch, as fwgpu_record_batch_create makes from the same records; the records the device parsed never leave
 * it.  Stops as fwgpu_parser_parse_buffer stops (max_records, a line that is not an example): the batch holds the examples before
 * the stop and *consumed says where to go on.  A call whose FIRST line is not an example returns that line's code (FWGPU_PARSE_FLUSH,
 * FWGPU_PARSE_HOGWILD_LOAD, FWGPU_ERR_PARSE) and no batch.  Parser and regressor must be on the same device. */
int fwgpu_record_batch_from_text(fwgpu_regressor *r, const fwgpu_translator_config *t, fwgpu_text_parser *tp, const char *text,
                                 uint64_t len, uint64_t max_records, fwgpu_batch **out, uint64_t *n_records, uint64_t *consumed);
/* The device's decimal -> f32 conversion (csrc/f32_text.h) compiled for the host.  FWGPU_ERR_PARSE: not in Rust's f32::from_str
 * grammar.  *proven != 0: *out is the correctly rounded value (strtof); otherwise the device leaves the line to the host. */
int fwgpu_f32_from_text(const char *s, uint64_t len, float *out, int *proven);

/* RecordCache (cache.rs:54-232).  fwgpu_cache_open(input, vw): if "<input>.fwcache" exists and its header ("FWCA",
 * version 11, vw_source equal to `vw`) verifies, the cache is opened for reading; otherwise "<input>.fwcache.writing" is
 * created for writing and renamed by fwgpu_cache_write_finish (cache.rs:70-131, 146-152).  Inputs whose name ends in
 * "gz" use an LZ4 frame stream (cache.rs:73).  fwgpu_cache_next_records = bulk get_next_record: whole records into
 * `words`, rec_off[0..n_records] word offsets; *n_records == 0 at end of file. */
typedef struct fwgpu_cache fwgpu_cache;
int fwgpu_cache_open(const char *input_filename, const fwgpu_vwmap *vw, fwgpu_cache **out);
int fwgpu_cache_is_reading(const fwgpu_cache *c);
int fwgpu_cache_is_writing(const fwgpu_cache *c);
int fwgpu_cache_push_records(fwgpu_cache *c, const uint32_t *words, uint64_t n_words);
int fwgpu_cache_write_finish(fwgpu_cache *c);
int fwgpu_cache_next_records(fwgpu_cache *c, uint32_t *words, uint64_t words_cap, uint64_t *rec_off, uint64_t max_records,
                             uint64_t *n_records, uint64_t *n_words);
void fwgpu_cache_free(fwgpu_cache *c);
/* The example loop over a cache file (main.rs:213-270: get_next_record -> digest_example) in native code: up to max_records
 * (0 = to the end of the file) are read, copied to pinned memory and learned; a reader thread overlaps the file with the
 * device.  Call fwgpu_finish afterwards, as after fwgpu_digest_records. */
int fwgpu_trainer_digest_cache(fwgpu_trainer *tr, fwgpu_cache *cache, uint64_t max_records, uint64_t *n_digested);
/* The same loop over VW TEXT (no cache, or the cache-writing first pass of `-c`): `text` is cut at line breaks into one
 * slice per host thread (threads == 0: 8), each parsed by a clone of `parser`; the records are learned in the original
 * order and appended to `cache` when it is non-NULL and open for writing.  Stops at the first line that is not an
 * example: the return value says why (FWGPU_PARSE_FLUSH, FWGPU_PARSE_HOGWILD_LOAD, FWGPU_ERR_PARSE), *consumed = bytes
 * fully digested, *n_examples = examples learned. */
int fwgpu_parser_clone(const fwgpu_parser *src, fwgpu_parser **out);
/* create_buffered_input (buffer_handler.rs:8-37): ".vw" plain, ".gz" gzip (several members allowed, MultiGzDecoder), ".zst"
 * zstd (libzstd.so.1 resolved at run time); any other extension is refused with the reference's message.
 * fwgpu_input_read fills `buf` with decompressed bytes, *n == 0 at the end.  fwgpu_trainer_digest_file = the example loop
 * over such a file: 64 MiB windows cut at line breaks -> fwgpu_trainer_digest_text. */
typedef struct fwgpu_input fwgpu_input;
int fwgpu_input_open(const char *filename, fwgpu_input **out);
int fwgpu_input_read(fwgpu_input *in, char *buf, uint64_t cap, uint64_t *n);
void fwgpu_input_close(fwgpu_input *in);
int fwgpu_trainer_digest_file(fwgpu_trainer *tr, fwgpu_parser *parser, fwgpu_cache *cache, const char *filename,
                              uint32_t threads, uint64_t *n_examples);
int fwgpu_trainer_digest_text(fwgpu_trainer *tr, fwgpu_parser *parser, fwgpu_cache *cache, const char *text, uint64_t len,
                              uint32_t threads, uint64_t *n_examples, uint64_t *consumed);
/* fwgpu_trainer_digest_text / _digest_file with the parser on the DEVICE (csrc/textparse.hip): same order, stops, return codes, messages,
 * *consumed, *n_examples, hold-out protocol and cache contents as the host forms; the command argument comes through
 * fwgpu_text_parser_command_argument.  The text goes up in pieces cut at line breaks (FWGPU_TRAINER_TEXT_PIECE=<bytes>, default 8 MiB); a piece
 * is parsed, cut into launches of at most micro_batch examples and placed by kernels on the parser's stream while the piece before it is learned,
 * and the host parses only the lines the kernel leaves to it (fwgpu_text_parser_last_lines).  micro_batch is a cap here: a piece's last launch,
 * and the launch before the hold-out boundary, may be shorter.  Everything parsed is launched before the call returns; fwgpu_finish waits.  A
 * micro-batch left open by fwgpu_digest_records is launched first.  Records are read back only for a cache open for writing (once per piece) and
 * for a launch that holds an oversize example.  A cache open for reading, or a parser on another device than the regressor's, is
 * FWGPU_ERR_INVALID.  The parser's buffers hold the launches' records: free it after fwgpu_finish, and use it with one trainer at a time.
 * fwgpu_text_parser_last_wait_ns: how long the host waited for the parser's stream during the last such call. */
int fwgpu_trainer_digest_text_device(fwgpu_trainer *tr, fwgpu_text_parser *tp, fwgpu_cache *cache, const char *text, uint64_t len,
                                     uint64_t *n_examples, uint64_t *consumed);
int fwgpu_trainer_digest_file_device(fwgpu_trainer *tr, fwgpu_text_parser *tp, fwgpu_cache *cache, const char *filename,
                                     uint64_t *n_examples);
int fwgpu_text_parser_last_wait_ns(const fwgpu_text_parser *tp, uint64_t *ns);
/* The micro-batch plan of that route (textparse.hip text_batch_plan) on host arrays, for tests.  status4: nlines x {status, record length, LR
 * entries, FFM entries}, status (low byte) 1 = parsed by the device, 2 = needs the host, 3 = done by the host; a line of status 2 counts with
 * zeros.  The first n_take lines are cut into windows of at most micro_batch lines, none of which straddles line learn_before_holdout
 * (0xffffffff: no boundary).  Out: dst_off[n_take] and rec_off[n_take + 1] (word offsets), *n_windows, window_stats[7 per window] = examples,
 * words, max_lr, max_ffm, max_rec, tot_lr, tot_ffm, and the status-2 lines of all nlines in order (host_lines[nlines], *n_host_lines). */
int fwgpu_debug_text_plan(const uint32_t *status4, uint32_t nlines, uint32_t n_take, uint32_t micro_batch, uint32_t learn_before_holdout,
                          uint64_t *dst_off, uint64_t *rec_off, uint32_t *n_windows, uint64_t *window_stats, uint32_t *host_lines,
                          uint32_t *n_host_lines, void *stream);

/* ---------------------------------------------------------------- model files
 * File = "FWRE", u32 version 6, u64 + JSON(vw_source), u64 + JSON(ModelInstance), weights blob (persistence.rs:17-97,
 * regressor.rs:426-469).  ModelInstance (model_instance.rs:47-97) crosses the boundary as an opaque handle made from /
 * rendered to that JSON; fwgpu_mi_to_json reproduces serde_json::to_vec_pretty (nn layer keys sorted: the reference's
 * HashMap order is arbitrary).  fwgpu_mi_configs fills the structs fwgpu_create / fwgpu_set_nn / the translator take
 * (any of the three may be NULL); their array pointers stay valid while the handle lives.  Features of ModelInstance this
 * path does not implement (transformed namespaces, nn topologies four/five, layernorm, dropout, maxnorm) are
 * rejected there, never ignored. */
typedef struct fwgpu_model_instance fwgpu_model_instance;
int fwgpu_mi_from_json(const char *json, uint64_t len, fwgpu_model_instance **out);
void fwgpu_mi_free(fwgpu_model_instance *mi);
int fwgpu_mi_to_json(const fwgpu_model_instance *mi, char *buf, uint64_t cap, uint64_t *len);
int fwgpu_mi_configs(fwgpu_model_instance *mi, int device, fwgpu_config *cfg, fwgpu_translator_config *tr,
                     fwgpu_nn_config *nn);
int fwgpu_mi_set_inference(fwgpu_model_instance *mi, int dequantize_weights); /* main.rs:141-145 */
/* save_regressor_to_filename (persistence.rs:73-89); quantize_weights: FFM weights as f16 buckets (block_ffm.rs:835-848) */
int fwgpu_model_save(const char *path, const fwgpu_vwmap *vw, const fwgpu_model_instance *mi, fwgpu_regressor *r,
                     int quantize_weights);
/* load_regressor_without_weights (persistence.rs:91-125): header only, no device */
int fwgpu_model_read_header(const char *path, fwgpu_vwmap **vw, fwgpu_model_instance **mi);
/* new_regressor_from_filename (persistence.rs:127-174).  *r == NULL: a regressor is created on `device` (immutable != 0:
 * optimizer forced to SGD, only the weights kept).  *r != NULL: hogwild_load (persistence.rs:176-187), the weights
 * are loaded into the existing regressor.  vw / mi may be NULL. */
int fwgpu_model_load(const char *path, int device, int immutable, fwgpu_vwmap **vw, fwgpu_model_instance **mi,
                     fwgpu_regressor **r);
/* fwgpu_model_load(path, device, immutable = 1, ...) whose FFM weights STAY in the quantised inference file's form in device
 * memory: one f16 bucket number per weight, w = min + f32(bucket) * increment formed inside the predict kernel (bit for bit
 * what fwgpu_dequantize_ffm_weights gives).  A file with dequantize_weights = true is uploaded as it is; any other model
 * file is quantised on the host first (what fwgpu_model_convert_inference(..., quantize_weights = 1) would have written).
 * No f32 FFM table and no accumulator table exist on the device.  The regressor PREDICTS: fwgpu_predict, fwgpu_learn /
 * fwgpu_learn_batch with update = 0 (entry and record batches, both modes), fwgpu_batch_predictions*, fwgpu_table_len,
 * fwgpu_table_read / fwgpu_table_checksum of FWGPU_TABLE_FFM_W (the dequantised values).  Everything that would write or
 * train -- update != 0, fwgpu_learn_batch_sync, fwgpu_table_write / fill / device_ptr on the FFM tables, fwgpu_read_weights,
 * fwgpu_write_weights, fwgpu_model_save, fwgpu_trainer_create, fwgpu_dist_*, hogwild_load into it -- and fwgpu_setup_cache
 * (unless fwgpu_packed_enable_caches was called, below) return FWGPU_ERR_INVALID and leave it usable.
 * Refused here with FWGPU_ERR_INVALID: models with a deep head, models without an FFM block, ffm_k % 4 != 0, rows
 * (ffm_k x fields) of more than 256 weights unless ffm_k divides 256 and the row has at most 512.  Refused at the launch:
 * entry batches with an FFM hash that is not a multiple of 4 (raw entries that did not pass fwgpu_ffm_hash_mask), examples
 * of more than 2048 FFM features. */
int fwgpu_model_load_packed(const char *path, int device, fwgpu_vwmap **vw, fwgpu_model_instance **mi, fwgpu_regressor **r);
/* How the FFM weight table lives on the device, and the bytes it occupies there */
enum { FWGPU_FFM_F32 = 0, FWGPU_FFM_F16_BUCKETS = 1 };
int fwgpu_ffm_storage(fwgpu_regressor *r, int *storage, uint64_t *table_bytes);
/* ---- context caches on a packed regressor (opt-in).  fwgpu_packed_enable_caches is a ONE-WAY switch on a packed regressor (made by
 * fwgpu_model_load_packed or fwgpu_pack_regressor, whose refresh in place keeps it); an f32 regressor is FWGPU_ERR_INVALID.  Without it every
 * call answers as above.  With it, on that regressor:
 *   fwgpu_setup_cache          builds the cache with the packed build kernel (csrc/requests.hip): T, dcf and the counts in the layout and summation
 *                              order an f32 regressor's cache has, from the values the buckets stand for
 *   fwgpu_block_cache_filter   as ever
 *   fwgpu_batch_set_cache      on an ENTRY batch: the set of one; fwgpu_batch_set_caches: a cache per example.  A predict-only launch of such a
 *                              batch takes FWGPU_ROUTE_REQUESTS with the kernel family FWGPU_KERNEL_PACKED_REQUESTS; update != 0, an oversize
 *                              example, a hash off the 4-bucket boundary (FWGPU_ERR_INVALID) and the LDS range (FWGPU_ERR_RANGE) as on f32 tables
 *   fwgpu_predict_with_cache   the same route for one example
 * Record batches with a cache stay refused: fwgpu_block_cache_cover_record and fwgpu_batch_set_cache on a record batch are FWGPU_ERR_INVALID
 * and name the entry route.
 * STALENESS.  The regressor carries a weights epoch, bumped by fwgpu_packed_apply_diff (when it applies an entry) and by fwgpu_pack_regressor's
 * refresh in place.  A cache records the epoch at fwgpu_setup_cache.  Attaching a cache of an older epoch (fwgpu_batch_set_cache(s)), launching a
 * batch that holds one, and fwgpu_predict_with_cache with one are FWGPU_ERR_INVALID ("stale"), the batch left as it was: nothing is served from
 * sums of weights that no longer exist.  fwgpu_setup_cache on the same handle refills the cache at the current epoch. */
int fwgpu_packed_enable_caches(fwgpu_regressor *r);
int fwgpu_packed_caches_state(const fwgpu_regressor *r, int *enabled, uint64_t *weights_epoch); /* either output may be NULL */
/* debug: a cache's contents as the device holds them -- T [F * F * k], dcf [F], cnt [F], the epoch it was set up at (each may be NULL).  Waits for the device. */
int fwgpu_debug_block_cache_read(const fwgpu_block_cache *cache, float *T, float *dcf, uint32_t *cnt, uint64_t *epoch);
/* debug (scripts/bench_serving_packed_requests.py): milliseconds per launch, by device events over `reps` launches on the null stream, of the
 * requests route of a batch with a set attached (base kernel + predict kernel).  rows: the packed predict kernel's rows in flight per lane, 4 or 8,
 * 0 = the default (the only value an f32 regressor takes). */
int fwgpu_debug_requests_time(fwgpu_regressor *r, fwgpu_batch *b, int rows, uint32_t reps, float *ms_per_launch);
/* ---- quantising on the device: train -> publish -> serve without the training blob crossing to the host
 * The reference's quantiser (quantization.rs:18-80) as HIP kernels (csrc/quantize.hip): a statistics pass (min, max, "a weight is not finite")
 * over exactly the table's weights, the header {increment, min} formed on the host from the two reduced floats by the host quantiser's own
 * statements, and a bucket pass f16(roundf((w - min) / increment)).
 * CONTRACT: the bytes are those of fwgpu_quantize_ffm_weights on the same weights.  HOST ROUTE: when a weight is NaN or infinite, or the
 * header's increment is 0 or not finite (a constant table, a maximum that rounds onto the minimum), the device route is not used and the
 * call quantises on the host as before (fwgpu_table_read + the host quantiser): those results are the host's by construction.
 * OUTSIDE THE CONTRACT: a table whose extreme value is a zero present with both signs (fmin(+0, -0) is unspecified on the host): the sign
 * of the header's min may differ.  FWGPU_QUANTIZE_HOST=1 in the environment forces the host route everywhere (A/B runs).
 * Every call below first waits for the regressor's outstanding launches, as fwgpu_write_weights does, and leaves the source regressor's
 * tables and its ability to train untouched. */
/* The regressor's FFM weights as the quantised block: 8-byte header, then one f16 bucket per weight (8 + 2 n bytes, n = fwgpu_table_len of
 * FWGPU_TABLE_FFM_W).  Only the buckets cross to the host.  FWGPU_ERR_INVALID for packed regressors and models without an FFM block. */
int fwgpu_quantize_ffm_table(fwgpu_regressor *r, uint8_t *out, uint64_t cap, uint64_t *written);
/* From a live training regressor, the file that fwgpu_model_save(training file) followed by fwgpu_model_convert_inference(...,
 * quantize_weights) writes (main.rs:136-148), byte for byte: the header is that of a copy of `mi` after fwgpu_mi_set_inference; LR weights
 * only (compacted on the device), FFM weights as f32 or as buckets, dense layers' weights only (small: through the host).  The
 * accumulator tables never leave the device.  All three optimizers and models with a deep head are accepted. */
int fwgpu_model_save_inference(const char *path, const fwgpu_vwmap *vw, const fwgpu_model_instance *mi, fwgpu_regressor *r,
                               int quantize_weights);
/* *out == NULL: creates, on src's device, the packed regressor fwgpu_model_load_packed would create from a file saved from src at this
 * moment -- table to table on the device, no host copy of either -- with fwgpu_model_load_packed's refusals and messages (deep head, no FFM
 * block, ffm_k % 4, row size).  *out != NULL: refreshes that packed regressor in place: buckets, the two header words the predict kernel
 * takes as launch constants, and the LR weights.  It must be a packed regressor (made here or by fwgpu_model_load_packed) of src's
 * geometry on src's device; anything else is FWGPU_ERR_INVALID and *out stays usable.  A packed src is refused.  The call waits for the
 * device; the caller must not have predict launches of *out in flight on other streams while it runs. */
int fwgpu_pack_regressor(fwgpu_regressor *src, fwgpu_regressor **out);
/* debug: the statistics and bucket kernels on a host array of any length (uploaded, quantised, 8 + 2 n bytes returned); *on_device = 0 when
 * the contract sent the array to the host route */
int fwgpu_debug_quantize(int device, const float *weights, uint64_t n, uint8_t *out, uint64_t cap, int *on_device);
/* debug (scripts/bench_publish.py): milliseconds, by device events, of the statistics kernels, the bucket kernel and a device-to-device copy
 * of the same table, on the regressor's FFM weights; nothing of the regressor changes */
int fwgpu_debug_quantize_rates(fwgpu_regressor *r, float *ms3);
/* --convert_inference_regressor (main.rs:136-148): training file -> inference file; host only */
int fwgpu_model_convert_inference(const char *in_path, const char *out_path, int quantize_weights);
/* quantization.rs:42-98: out = 8-byte header {f32 increment, f32 min} + n f16 bucket numbers (8 + 2n bytes) */
int fwgpu_quantize_ffm_weights(const float *weights, uint64_t n, uint8_t *out, uint64_t cap);
int fwgpu_dequantize_ffm_weights(const uint8_t *in, uint64_t n, float *weights);

/* ---------------------------------------------------------------- byte diffs of published inference models (weight_patcher/src/main.rs)
 * THE STREAM is what the reference's compare_files_and_write_diff hands to its writer, byte for byte, WITHOUT the gzip container the tool
 * wraps around it: for every index i with a[i] != b[i], ascending, varint(i - prev) then the byte b[i]; prev is the previous entry's index
 * and starts at 0 (a difference at index 0 is delta 0); the varint is little-endian base-128, top bit set on every byte but the last.
 * THE READER IS STRICTER than recreate_file_inner: a stream that ends inside an entry, a varint of more than 10 bytes or beyond 64 bits, an
 * entry at or beyond the target's end, and a zero delta in any entry but the first are FWGPU_ERR_FORMAT, and nothing is written unless the
 * whole stream is valid (csrc/diff_stream.h holds the codec and states the format). */
/* compare_files_and_write_diff (main.rs:68-130) on two host arrays that stand for the bytes [base_offset, base_offset + n) of two files.
 * prev_index: the index of the last entry already emitted before this range (0 at the start of a file; above base_offset is
 * FWGPU_ERR_INVALID).  Two-call protocol: out == NULL or cap too small returns FWGPU_ERR_RANGE with *written = the size needed.
 * *changed (may be NULL): the number of entries. */
int fwgpu_diff_bytes(const uint8_t *a, const uint8_t *b, uint64_t n, uint64_t base_offset, uint64_t prev_index, uint8_t *out, uint64_t cap,
                     uint64_t *written, uint64_t *changed);
/* recreate_file_inner (main.rs:148-206) in place on a host array that stands for the file's bytes [base_offset, base_offset + n).  Entries
 * below base_offset are skipped; *applied (may be NULL): entries written.  A bad stream is FWGPU_ERR_FORMAT and the target is unchanged. */
int fwgpu_diff_apply_bytes(uint8_t *target, uint64_t n, uint64_t base_offset, const uint8_t *diff, uint64_t len, uint64_t *applied);
/* An image is the file fwgpu_model_save_inference(path, vw, mi, r, quantize_weights) would write at this moment, split in two: the header
 * (write_header + the u64 element count) on the host, the weights section in ONE device allocation in file order.  It is built by the routines
 * that call uses (the LR compaction, the device quantiser with its host route, the layers' copies); the tables do not cross to the host.
 * CONTRACT: fwgpu_image_read gives exactly that file's bytes.  capture waits for the regressor's outstanding launches, leaves it and its ability
 * to train untouched, and refuses packed regressors.  fwgpu_image_load puts an existing inference file (optimizer SGD, weights only) into the
 * same form: a trainer that restarts diffs its next publish against it. */
typedef struct fwgpu_image fwgpu_image;
int fwgpu_image_capture(fwgpu_regressor *r, const fwgpu_vwmap *vw, const fwgpu_model_instance *mi, int quantize_weights, fwgpu_image **img);
int fwgpu_image_load(const char *path, int device, fwgpu_image **img);
int fwgpu_image_len(const fwgpu_image *img, uint64_t *header_bytes, uint64_t *weights_bytes);
int fwgpu_image_read(const fwgpu_image *img, uint8_t *out, uint64_t cap);  /* cap below header + weights bytes: FWGPU_ERR_RANGE */
void fwgpu_image_free(fwgpu_image *img);
/* The stream of the two whole files (compare_files_and_write_diff on them): the headers are diffed on the host, the weights sections by
 * three HIP kernels (csrc/patch.hip: size pass, tile scan, emit pass) with base_offset = header_bytes, and only the stream crosses to the
 * host.  Two-call protocol as fwgpu_diff_bytes.  *changed (may be NULL): differing bytes -- when the quantiser's rounded extremes move, nearly
 * every bucket changes and the stream approaches two bytes per file byte: ship the file instead.  Images of different lengths or on
 * different devices are FWGPU_ERR_INVALID. */
int fwgpu_image_diff(const fwgpu_image *base, const fwgpu_image *next, uint8_t *out, uint64_t cap, uint64_t *written, uint64_t *changed);
/* Patches a packed regressor in place from such a stream: afterwards it is the regressor fwgpu_model_load_packed makes from the second file.
 * r must come from fwgpu_model_load_packed on an inference file that was already quantised (dequantize_weights = true): its tables are
 * that file's bytes.  FWGPU_ERR_INVALID, with the reason: an f32 regressor, a product of fwgpu_pack_regressor (no file behind it: refresh it
 * with that call), a packed regressor whose file was quantised at load, and a stream with an entry in the file's header ("the model's header
 * changed: load the file").  A bad stream is FWGPU_ERR_FORMAT.  In all these cases r is as it was and usable.  Entries in the FFM block's 8-byte
 * header update the two launch constants; all others are scattered by one kernel, byte by byte.  The call waits for the device; the caller
 * must not have predict launches of r in flight on other streams (fwgpu_pack_regressor's refresh contract).  *applied (may be NULL): entries. */
int fwgpu_packed_apply_diff(fwgpu_regressor *r, const uint8_t *diff, uint64_t len, uint64_t *applied);
/* debug: two host arrays uploaded, the three kernels run, the stream returned (two-call protocol as fwgpu_diff_bytes) */
int fwgpu_debug_diff(int device, const uint8_t *a, const uint8_t *b, uint64_t n, uint64_t base_offset, uint64_t prev_index, uint8_t *out,
                     uint64_t cap, uint64_t *written, uint64_t *changed);
/* debug: the bytes of one tile of the kernels, so that tests can place differences on tile edges */
int fwgpu_debug_diff_geometry(uint32_t *tile_bytes);
/* debug (scripts/bench_publish_diff.py): milliseconds, by device events, of the size pass, the tile scan, the emit pass and a device-to-device
 * copy of one weights section; nothing of the images changes */
int fwgpu_debug_diff_rates(const fwgpu_image *base, const fwgpu_image *next, float *ms4);

/* ---------------------------------------------------------------- synthetic record streams
 * Generates records in the parser's output format (parser.rs:57-74) for the BASELINE.json configs:
 * n_namespaces namespaces == fields; per namespace 1+Poisson(mean_extra) features (exactly 1 when
 * mean_extra==0); ids ~ Zipf(zipf_s) over ids_per_ns; feature hash = murmur3(decimal id,
 * seed=murmur3(namespace name)) & MASK31 as the parser does (parser.rs:82-87, 382-385); a feature has
 * value 1.0 with probability 1-p_weighted else U(0.5,2); label from a fixed random teacher.
 * Two-call protocol: call with records==NULL to get the sizes, then with buffers. */
typedef struct fwgpu_synth_config {
    uint32_t n_namespaces;
    float mean_extra;
    double zipf_s;
    uint32_t ids_per_ns;
    float p_weighted;
    uint64_t seed;
} fwgpu_synth_config;
int fwgpu_synth_records(const fwgpu_synth_config *cfg, uint64_t first_example, uint32_t n, uint32_t *records,
                        uint64_t records_cap, uint64_t *rec_off, uint64_t *n_words);
uint32_t fwgpu_murmur3_32(const uint8_t *data, size_t len, uint32_t seed);

#ifdef __cplusplus
}
#endif
#endif
