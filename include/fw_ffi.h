/*
 * fw_ffi.h -- the reference's own serving FFI, exported by libfwgpu.so under the reference's names and signatures
 * (/root/reference/src/lib.rs:50-53, 150-236).  A program that links the reference's libfw (Java/JNI, C, Python ctypes)
 * links this library instead and keeps its calls: the predictions come from the MI355X example kernel.
 *
 *   lib.rs:150-185  new_fw_predictor_prototype(command)   command = the fw command line; `-i/--initial_regressor FILE` is
 *                                                         loaded as an immutable regressor (persistence.rs:127-174);
 *                                                         `--device N` (ours) picks the GPU; `--packed_weights` (ours) keeps
 *                                                         the FFM weights as the quantised file's f16 buckets on the device
 *                                                         (fwgpu_model_load_packed: half the table, same calls);
 *                                                         `--packed_context_cache` (ours, only with --packed_weights, else
 *                                                         an error) lets such a predictor keep device context caches
 *                                                         (fwgpu_packed_enable_caches): fw_setup_cache builds one from the
 *                                                         packed table, the cached calls below and
 *                                                         fwgpu_predictor_predict_requests score filtered candidates.  NULL +
 *                                                         fwgpu_last_error() on failure (the reference panics).
 *   lib.rs:187-205  clone_lite(prototype)                 cheap per-thread copy sharing the weights
 *   lib.rs:207-212  fw_predict(ptr, vw_text)              -> prediction, or -1.0 for EOF / a line that does not parse
 *   lib.rs:224-232  fw_setup_cache(ptr, context_text)     -> 0.0 (or -1.0); remembers the request's context part
 *   lib.rs:214-222  fw_predict_with_cache(ptr, text)      -> prediction for context + text
 *   lib.rs:234-236  free_predictor(ptr)
 */
#ifndef FW_FFI_H
#define FW_FFI_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct FfiPredictor FfiPredictor;

FfiPredictor *new_fw_predictor_prototype(const char *command);
FfiPredictor *clone_lite(FfiPredictor *prototype);
float fw_predict(FfiPredictor *ptr, const char *input_buffer);
float fw_predict_with_cache(FfiPredictor *ptr, const char *input_buffer);
float fw_setup_cache(FfiPredictor *ptr, const char *input_buffer);
void free_predictor(FfiPredictor *ptr);

/* Not in the reference: all candidates of one request in ONE device launch.  inputs[i] is what fw_predict
 * (with_cache == 0) or fw_predict_with_cache (with_cache != 0) would be given, out[i] what it would return. */
int fwgpu_predictor_predict_batch(FfiPredictor *ptr, const char *const *inputs, uint32_t n, int with_cache, float *out);

/* The same request as ONE text, a candidate per line (a last line may lack its newline), scanned by the device: out[i] is what
 * fw_predict_with_cache (with_cache != 0) or fw_predict would return for line i with its newline, -1.0 for a line that does not
 * parse or gives no record; *n = number of lines; FWGPU_ERR_RANGE when cap is smaller.  With a device cache whose context is its
 * own record, lines that start with '|' never reach the host parser and the records go from the parser's write pass into the
 * launch.  A request in which a candidate names a cached namespace with another feature, repeats a cached feature in an uncached
 * namespace or continues the context's last namespace takes fwgpu_predictor_predict_batch on the split lines, as do predictors
 * without a device cache (--packed_weights) and FWGPU_SERVING_HOST_PARSE=1: same numbers.  fwgpu_predictor_last_text_route: lines
 * of the last call on this predictor, how many of them the host parsed, and whether the call went through predict_batch. */
int fwgpu_predictor_predict_text(FfiPredictor *p, const char *text, uint64_t len, int with_cache, float *out, uint64_t cap, uint64_t *n);
int fwgpu_predictor_last_text_route(const FfiPredictor *p, uint64_t *lines, uint64_t *host_lines, int *fell_back);

/* The candidates of SEVERAL requests in ONE device launch.  predictors[r] are the prototype and clone_lite copies of one model, each
 * after its own fw_setup_cache (the same predictor may appear twice); inputs[r][j], j < n_inputs[r], is what
 * fw_predict_with_cache(predictors[r], .) would be given, out[r][j] what it would return, -1.0 for a line that does not parse or
 * gives no record.  Every line is parsed behind its predictor's context, translated and filtered by that predictor's cache on the
 * host's worker threads; one entry batch with a cache per example follows (fwgpu_batch_set_caches), whose kernel's work per candidate
 * follows the candidate's own features.  FWGPU_ERR_INVALID, pointing to fwgpu_predictor_predict_batch: predictors of different
 * models, a predictor without a device cache (no fw_setup_cache yet, --packed_weights without --packed_context_cache, a model without an FFM block), a model with
 * a deep head.  Concurrent callers are not coalesced: each call is one launch under the model's mutex. */
int fwgpu_predictor_predict_requests(FfiPredictor *const *predictors, uint32_t n_requests, const char *const *const *inputs,
                                     const uint32_t *n_inputs, float *const *out);

/* Not in the reference's FFI (its weight_patcher rewrites the file): patches a --packed_weights model in place from the bare byte-diff stream
 * of the file it was loaded from and the next published file (include/fwgpu.h: fwgpu_image_diff, fwgpu_diff_bytes; fwgpu_packed_apply_diff
 * states the refusals).  Runs under the model's mutex; the prototype and every clone_lite copy share the tables and see the patch.
 * Predictors without --packed_weights are FWGPU_ERR_INVALID.  A refused or malformed stream leaves the model as it was.
 * With --packed_context_cache the patch makes every context cache of the model stale (the regressor's weights epoch); each predictor, clones
 * included, rebuilds its cache from the context's entries it keeps before its next cached call, under the same mutex. */
int fwgpu_predictor_apply_diff(FfiPredictor *p, const uint8_t *diff, uint64_t len);

#ifdef __cplusplus
}
#endif
#endif
