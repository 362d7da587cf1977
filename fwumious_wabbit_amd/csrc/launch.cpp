// The launch path: every fused, packed, requests, batched-head, peer, chunked and split-phase launch is planned and issued here -- the planners
// (plan_launch, plan_head_inputs), the route of a batch (pick_route, run_batch), single-example learn / predict (regressor.rs:356-395), the oversize
// example's chunked pipeline, the split phases, and the C entry points that are only launches.  There is no CPU compute path: every learn / predict
// runs the HIP kernel.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "hot_tiers.h"
#include "launch.h"

#ifndef FWGPU_LR_THIN_DEFAULT  // store policy 4 also on hot LR entries of the large-table path (kernels.hip lr_update; DESIGN 4.2: shipped in round 6)
#define FWGPU_LR_THIN_DEFAULT 1
#endif
#ifndef FWGPU_ACC_TIERS_DEFAULT  // store policy 4: hot rows beyond 8 / 16 / 32 x the threshold sampled one in 16 / 32 / 64 (hot_tiers.h; DESIGN 4.2, profiles/hot_tiers_ab.txt)
#define FWGPU_ACC_TIERS_DEFAULT 1
#endif
namespace fwgpu {

// the kernel version a launch is planned with (KernelParams::kernel_version: 0 = auto, 1 = the generic kernel)
static int32_t kernel_version_of(const fwgpu_regressor *r, KernelChoice kernel) {
    return kernel == KernelChoice::kGeneric ? 1 : kernel == KernelChoice::kResident ? 0 : r->launch.kernel_version;
}

KernelParams make_params(const fwgpu_regressor *r, const fwgpu_batch *b, int update, KernelChoice kernel) {
    KernelParams p{};
    p.ffm_w = r->packed() ? reinterpret_cast<float *>(r->d_ffm_q) : r->d_ffm_w;  // (packed: read by launch_packed_predict's kernels only, as 2-byte buckets)
    p.ffm_acc = r->d_ffm_acc;
    p.lr = r->d_lr;
    p.lut_lr = r->d_lut_lr;
    p.lut_ffm = r->d_lut_ffm;
    p.ffm_hash = b->ffm_hash;
    p.ffm_val = b->ffm_val;
    p.ffm_fld = b->ffm_fld;
    p.ffm_off = b->ffm_off;
    p.lr_hash = b->lr_hash;
    p.lr_val = b->lr_val;
    p.lr_off = b->lr_off;
    p.lr_combo = b->lr_combo;
    p.nn = r->nn;
    p.num_combos = r->cfg.num_combos;
    p.label = b->label;
    p.importance = b->importance;
    p.pred = b->pred;
    p.n_examples = b->n;
    p.F = r->cfg.ffm_k ? r->cfg.ffm_num_fields : 0;
    p.k = r->cfg.ffm_k;
    p.R = p.F * p.k;
    p.max_ffm = std::max<uint32_t>(4, (b->max_ffm + 3) & ~3u);
    p.max_lr = std::max<uint32_t>(4, (b->max_lr + 3) & ~3u);
    p.has_lr = r->cfg.wiring == FWGPU_WIRING_REGRESSOR;
    p.update = update ? 1 : 0;
    p.aligned4 = b->aligned4 ? 1 : 0;
    // Whole-line row updates pay where partial-line writes reach HBM, i.e. when w + acc do not fit the 256 MiB Infinity
    // Cache (profiles/r02_rowceil.txt: cache-resident tables write partial lines at full rate).  Small tables also are
    // where concurrent examples would meet on a line most often, so they keep float-granular writes.
    // (launch_example_kernel keeps the flag only where the whole-line path exists.)
    p.window = r->launch.window >= 2 || (r->launch.window == 1 && r->ffm_len * 8ull > (256ull << 20)) ? 1 : 0;  // (3: the path of large tables on a table of any size, tests)
    // Whole-line accesses pay when w and acc contend for one region of the device memory (partial-line writes are what is slow
    // then: -6.5 %); with the accumulator table placed away from the weights they buy nothing (4.64 vs 4.60 M examples/s) and
    // only widen hogwild's race from the float to the line, so they are used when asked for (option 2 = 2) or when the placement
    // search found no partner that does not contend.
    p.line_pass = r->launch.window == 2 || (p.window && r->placement_contended) ? 1 : 0;
    p.no_chain = r->launch.no_chain;
    p.hot_lr_hash = 11650396u & lr_hash_mask(r->cfg.bit_precision);  // feature_buffer.rs:8, 270-276
    p.hot_lr_every = r->launch.hot_lr_every;
    {
        static const char *env = getenv("FWGPU_HOT_LR_EVERY");  // A/B runs: 0 = plain read-modify-writes
        if (env) p.hot_lr_every = (uint32_t)atoi(env);
    }
    p.k_log2 = 0xffu;
    for (uint32_t l = 0; l < 16; l++)
        if ((1u << l) == r->cfg.ffm_k) p.k_log2 = l;
    p.lr_rate = r->cfg.learning_rate;
    p.lr_minus_power_t = -r->cfg.power_t;
    p.ffm_rate = r->cfg.ffm_learning_rate;
    p.ffm_minus_power_t = -r->cfg.ffm_power_t;
    p.ticks = r->d_ticks;
    if (!update && b->cache) {  // predict_with_cache: the field sums start from the cached features' (regressor.rs:397-407)
        p.ctx_T = b->cache->d_T;
        p.ctx_dcf = b->cache->d_dcf;
        p.ctx_cnt = b->cache->d_cnt;
        if (b->records) p.ctx_cover = b->cache->d_cover;
        if (b->records && b->delta_records) {
            p.ctx_rec = b->cache->d_ctx_rec;
            p.ctx_rec_len = (uint32_t)b->cache->ctx_rec.size();
        }
    }
    if (!update) {
        p.emit_T = b->emit_T;
        p.emit_dcf = b->emit_dcf;
        p.emit_cnt = b->emit_cnt;
    }
    p.records = b->records;
    p.rec_self_len = b->rec_self_len ? 1 : 0;
    p.rec_off = b->rec_off;
    p.max_rec = (b->max_rec + 3) & ~3u;
    p.tr = b->tr;
    p.kernel_version = kernel_version_of(r, kernel);
    p.lut_global = r->launch.lut_global;
    {   // FFM row store policy of hogwild launches and its write-back interval (kernels.hip, "store policy"); -1 / ~0 = the kernels' build default
        static const char *env_pol = getenv("FWGPU_STORE_POLICY"), *env_wb = getenv("FWGPU_WB_FLUSH_EVERY"), *env_pf = getenv("FWGPU_PREFETCH");
        p.store_policy = r->launch.store_policy >= 0 ? r->launch.store_policy : (env_pol ? atoi(env_pol) : -1);
        static const char *env_th = getenv("FWGPU_ACC_HOT_THETA"), *env_sm = getenv("FWGPU_ACC_SAMPLE_LOG2");  // policy 3's two knobs (A/B runs)
        // "hot" = the row has ACCUMULATED more than theta: measured from the accumulators' initial value (AdagradFlex starts them at ffm_init_acc_gradient,
        // optimizer.rs:90-92; AdagradLUT at 0 with the initial value folded into its table, 158-161), so a row is never hot before it has been stepped
        const float theta = r->launch.acc_hot_theta >= 0.0f ? r->launch.acc_hot_theta : (env_th ? (float)atof(env_th) : 0.5f);
        p.acc_hot_theta = theta + initial_acc(r->cfg.optimizer, r->cfg.ffm_init_acc_gradient);
        const int sm = r->launch.acc_sample_log2 >= 0 ? r->launch.acc_sample_log2 : (env_sm ? atoi(env_sm) : 3);
        p.acc_sample_log2 = (uint32_t)std::min(std::max(sm, 0), 6);  // (1u << it in the kernels: one example in 1 .. 64)
        {   // the levels beyond which a hot row's adds are thinned further, as accumulator values like acc_hot_theta (A/B runs: FWGPU_ACC_TIERS=0, option 15)
            static const char *env_ti = getenv("FWGPU_ACC_TIERS");
            const bool tiers = (r->launch.acc_tiers >= 0 ? r->launch.acc_tiers : (env_ti ? atoi(env_ti) : FWGPU_ACC_TIERS_DEFAULT)) != 0;
            for (uint32_t t = 0; t < kHotTiers; ++t)
                p.acc_tier[t] = hot_tier_level(theta, initial_acc(r->cfg.optimizer, r->cfg.ffm_init_acc_gradient), t, tiers);
        }
        static const char *env_kr = getenv("FWGPU_KEPT_ROWS");
        p.no_kept_rows = (r->launch.kept_rows >= 0 ? r->launch.kept_rows == 0 : (env_kr && env_kr[0] == '0')) ? 1 : 0;
        static const char *env_lt = getenv("FWGPU_LR_THIN");
        // (an LR entry's g^2 is (g v)^2 ~ 0.1-0.25 per hit where an FFM float's is ~1e-4: the same "stepped by more than a hundred examples" reads 64 x the FFM rows' threshold here)
        static const char *env_ls = getenv("FWGPU_LR_HOT_SCALE");
        p.lr_hot_theta = theta * (env_ls ? (float)atof(env_ls) : 64.0f) + initial_acc(r->cfg.optimizer, r->cfg.init_acc_gradient);
        p.lr_thin = r->launch.lr_thin >= 0 ? r->launch.lr_thin : (env_lt ? atoi(env_lt) : FWGPU_LR_THIN_DEFAULT);
        static const char *env_tr = getenv("FWGPU_THIN_REREAD");
        p.thin_reread = env_tr ? atoi(env_tr) : 1;
        p.wb_flush_every = r->launch.wb_flush_every >= 0 ? (uint32_t)r->launch.wb_flush_every : (env_wb ? (uint32_t)atoi(env_wb) : 0xffffffffu);
        p.prefetch = (r->launch.prefetch && !(env_pf && env_pf[0] == '0')) ? 1 : 0;
        static const char *env_lk = getenv("FWGPU_LDS_KEEP");
        // rows per wave kept in LDS beyond the register-kept ones: the wish (clamped to the kernel's maximum by resolve_row_mode, to what leaves two
        // workgroups on a CU by plan_launch)
        p.lds_keep = r->launch.lds_keep >= 0 ? (uint32_t)r->launch.lds_keep : (env_lk ? (uint32_t)atoi(env_lk) : 255u);
    }
    p.work = b->work;
    p.host_cus = r->num_cus;
    p.host_wgs_cap = r->launch.workgroups_per_cu;
    p.host_grid_cap = r->launch.max_in_flight;
    return p;
}

// launch shape of a batch: workgroup size, LDS copy of the LUT or not (settles p.window / p.chain / p.lut_global)
uint32_t nn_v2_threads();  // (kernels.hip: the workgroup size the head-as-a-phase instantiation was built for)
int plan_launch(const fwgpu_regressor *r, const fwgpu_batch *b, int mode, int update, KernelChoice kernel, LaunchPlan &plan, const char **why) {
    KernelParams &p = plan.p;
    uint32_t &threads = plan.threads;
    const int32_t kernel_version = kernel_version_of(r, kernel);
    auto refuse = [why](int code, const char *reason) {
        *why = reason;
        return code;
    };
    p = make_params(r, b, update, kernel);
    p.concurrent = (mode == FWGPU_MODE_HOGWILD && p.host_grid_cap != 1 && b->n > 1) ? 1 : 0;  // (one workgroup -- in-order semantics -- otherwise)
    // SEQUENTIAL: one workgroup walks the batch.  HOGWILD: 0 = "what the device keeps resident" (launch_persistent)
    plan.grid = mode == FWGPU_MODE_SEQUENTIAL ? 1u : 0u;
    threads = r->launch.threads;
    if (mode == FWGPU_MODE_SEQUENTIAL) threads = std::max<uint32_t>(threads, 512);
    if ((uint64_t)p.max_ffm > 4ull * threads) threads = 1024;
    if ((uint64_t)p.max_ffm > 4ull * threads)
        return refuse(FWGPU_ERR_RANGE, "an example has more than 4096 FFM features");
    // Small examples (BASELINE configs[1]: 10 features, 11 LR entries): a 512-thread workgroup has eight waves for ten rows, and the rate of such a launch is (examples in
    // flight) / (an example's latency) with MORE than ~512 in flight costing both rate and loss (the hot LR entries' lines).  Two waves per example and two workgroups per CU:
    // 13.8 M examples/s at hold-out 0.59431 against 11.9 M at 0.59419 for the 512-thread shape (profiles/r06_configB_time_to_loss_table.txt).  FWGPU_SMALL_SHAPE=0: the old shape.
    {
        static const char *env_ss = getenv("FWGPU_SMALL_SHAPE");
        // (not the generic kernel forced by kernel_version 1: the peer-sharded and streaming launches size their consumer workgroups by the regressor's own workgroup size)
        if (!(env_ss && env_ss[0] == '0') && p.concurrent && update && !r->launch.threads_set && kernel_version != 1 && !p.nn.n_layers && p.max_ffm <= 32 && p.max_lr <= 64) {
            threads = 128;
            if (!p.host_grid_cap) p.host_grid_cap = 2 * r->num_cus;
        }
    }
    // Config E's concurrent launches: the deep head as a phase of the v2 kernel's two-chunk instantiation (kernels.hip fw_example_kernel_r<..., NN = true>) where TWO of its
    // 512-thread workgroups fit a CU -- the AdaGrad LUT read through L1, no record prefetch, no LDS copy of the entries' own slots -- instead of one 1024-thread workgroup
    // of the generic kernel.  In-order launches (the parity mode) and shapes that do not fit stay on the generic kernel.  fwgpu_debug_set_option(r, 11, 0) / FWGPU_NN_V2=0: off.
    {
        static const char *env_nn = getenv("FWGPU_NN_V2");
        const bool wish = r->launch.nn_v2 >= 0 ? r->launch.nn_v2 != 0 : !(env_nn && env_nn[0] == '0');
        const bool forced = r->launch.nn_v2 == 2;  // (tests: in-order launches too, whatever fits -- the head's wiring in that kernel against the oracle, per example)
        if (wish && p.nn.n_layers && update && (p.concurrent || forced) && p.window && p.k_log2 != 0xffu && p.R > 64 * 4 && (!r->launch.threads_set || r->launch.threads == nn_v2_threads()) && kernel_version != 1 && (uint64_t)p.max_ffm <= 4ull * 512) {
            KernelParams q = p;
            q.nn_v2 = 1;
            q.lut_global = 1;
            q.prefetch = 0;
            const uint32_t th_q = nn_v2_threads();
            resolve_row_mode(q, th_q);
            const size_t lds_q = example_kernel_lds_bytes(q, r->cfg.optimizer);
            if (example_kernel_is_resident(q, th_q) && q.window && (forced ? lds_q <= r->lds_per_cu : 2 * lds_q <= r->lds_per_cu)) {
                p = q;
                threads = th_q;
            }
        }
    }
    resolve_row_mode(p, threads);
    size_t lds = example_kernel_lds_bytes(p, r->cfg.optimizer);
    // rows parked in LDS by the gather (KernelParams::lds_keep): as many per wave as still let a second workgroup live on the CU
    while (p.lds_keep > 0 && 2 * lds > r->lds_per_cu) {
        p.lds_keep--;
        resolve_row_mode(p, threads);
        lds = example_kernel_lds_bytes(p, r->cfg.optimizer);
    }
    // When the LDS footprint lets only ONE workgroup live on a CU (k = 16 rows: T alone is 57.6 KB), the CU's waves have
    // to come from that workgroup: 1024 threads (measured at k = 16: 1.53 -> 1.82 M examples/s; with the deep head 0.67 -> 0.79).
    if (!r->launch.threads_set && mode == FWGPU_MODE_HOGWILD && 2 * lds > r->lds_per_cu) {
        // ... unless giving up the LDS copy of the AdaGrad LUT (8 KB) is what lets a SECOND workgroup in: two examples in
        // flight with the LUT read through L1 beat one example with the LUT in LDS (k = 16: 1.82 -> 1.93 M examples/s)
        KernelParams q = p;
        q.lut_global = 1;
        const size_t lds_nolut = example_kernel_lds_bytes(q, r->cfg.optimizer);  // (== lds where the kernel keeps the LUT in LDS regardless: lut_lds_forced)
        if (!p.lut_global && 2 * lds_nolut <= r->lds_per_cu) {
            p.lut_global = 1;
            lds = lds_nolut;
        } else if (example_kernel_is_resident(p, threads)) {
            // ... and unless the launch runs on the v2 kernel (models without a deep head): ONE 512-thread workgroup of it per CU beats one 1024-thread workgroup
            // of the generic kernel on both axes -- headless k = 16, round 5: 2.62-2.63 M examples/s and hold-out 0.653-0.655 against 2.52-2.53 M and 0.673
            // (profiles/r05_k16_threads_ab.txt)
        } else {
            threads = 1024;
            p.lds_keep = 0;
            resolve_row_mode(p, threads);
            lds = example_kernel_lds_bytes(p, r->cfg.optimizer);
        }
    }
    if (lds > r->lds_per_cu)
        return refuse(FWGPU_ERR_RANGE, "example does not fit the 160 KiB LDS (k*F^2 or features per example too large)");
    return FWGPU_OK;
}

// The FFM / LR part of a predict-only batch whose deep head runs afterwards, for the whole batch (run_batch_head_predict): plan_launch with the
// head's per-example LDS taken out of the picture.  A refusal is FWGPU_ERR_RANGE: the caller falls back to the per-example forward.
int plan_head_inputs(const fwgpu_regressor *r, const fwgpu_batch *b, LaunchPlan &plan, const char **why) {
    KernelParams &p = plan.p;
    auto refuse = [why](const char *reason) {
        *why = reason;
        return FWGPU_ERR_RANGE;
    };
    p = make_params(r, b, 0);  // (with the batch's context cache, if it has one: ctx_*)
    // candidate-only records: the stage phase puts the context's record behind the candidate's in LDS, so the batch's longest record counts both
    // (serving.cpp sizes max_rec that way; a batch that does not cannot be staged)
    if (p.ctx_rec && b->max_rec < p.ctx_rec_len) return refuse("candidate-only records: the batch's longest record does not include the context's");
    p.emit_x = 1;
    p.xbuf = r->pred_x;
    p.gbuf = r->pred_yi;
    plan.grid = 0;
    plan.threads = std::min<uint32_t>(r->launch.threads, 512);
    if ((uint64_t)p.max_ffm > 4ull * plan.threads) return refuse("an example has more than 2048 FFM features");  // (the caller falls back)
    resolve_row_mode(p, plan.threads);
    if (example_kernel_lds_bytes(p, r->cfg.optimizer) > r->lds_per_cu) return refuse("example does not fit the LDS");
    return FWGPU_OK;
}

// What fwgpu_debug_last_launch reports, in the order of its array.  launched() is the one writer of fwgpu_regressor::last_launch.
struct LaunchRecord {
    int32_t family, chunks, window, chain, no_kept_rows, lds_keep, threads, lds_bytes;
};
static void launched(fwgpu_regressor *r, const LaunchRecord &l) {
    const int32_t fields[8] = {l.family, l.chunks, l.window, l.chain, l.no_kept_rows, l.lds_keep, l.threads, l.lds_bytes};
    static_assert(sizeof(fields) == sizeof(r->last_launch), "fwgpu_debug_last_launch: FWGPU_LAUNCH_INFO_LEN fields");
    for (int i = 0; i < 8; i++) r->last_launch[i] = fields[i];
}
// ... for a launch of the example kernels: the RESOLVED parameters (after plan_launch / resolve_row_mode)
static void record_launch(fwgpu_regressor *r, const LaunchPlan &plan, bool packed, int optimizer) {
    const KernelParams &p = plan.p;
    const int family = packed ? FWGPU_KERNEL_PACKED : example_kernel_family(p, plan.threads);
    const uint32_t per_chunk = family == FWGPU_KERNEL_SCALAR ? 64u : 256u;  // floats of a row that one pass of a wave covers (1 or 4 per lane)
    LaunchRecord l{};
    l.family = family;
    l.chunks = (int32_t)((p.R + per_chunk - 1) / per_chunk);
    l.threads = (int32_t)plan.threads;
    // (the packed kernel is predict-only and sizes its LDS inside launch_packed_predict: the update path's fields and the LDS size are not reported for it)
    if (!packed) {
        l.window = p.window;
        l.chain = p.chain;
        l.no_kept_rows = p.no_kept_rows;
        l.lds_keep = (int32_t)p.lds_keep;
        l.lds_bytes = (int32_t)example_kernel_lds_bytes(p, optimizer);
    }
    launched(r, l);
}

// the launch's work counter at zero: the next counter of a host-mapped batch's ring, or a memset of the batch's own
static int fresh_work_counter(fwgpu_batch *b, KernelParams &p, hipStream_t stream) {
    if (b->work_ring) {
        int rc = mapped_batch_next_counter(b, stream);
        if (rc) return rc;
        p.work = b->work;
    } else {
        FWGPU_HIP(hipMemsetAsync(b->work, 0, sizeof(uint32_t), stream));
    }
    return FWGPU_OK;
}

static int run_batch_by_example(fwgpu_regressor *r, fwgpu_batch *b, int update, hipStream_t stream);
// predict-only launch of a packed regressor: the v2 kernel's shapes only (kernels.hip launch_packed_predict)
static int run_batch_packed(fwgpu_regressor *r, fwgpu_batch *b, int mode, int update, hipStream_t stream) {
    if (update) return refuse_packed(r, "an updating launch");
    if (b->n == 0) return FWGPU_OK;
    if (b->host_copy) return fail(FWGPU_ERR_INVALID, "packed regressor: an example of more than 4096 entries of a kind is not served");
    if (!b->aligned4)
        return fail(FWGPU_ERR_INVALID, "packed regressor: an FFM entry's hash is not a multiple of 4 (rows must start where the translator's mask puts them: hash & fwgpu_ffm_hash_mask)");
    LaunchPlan plan;
    const char *why = nullptr;
    int rc = plan_launch(r, b, mode, 0, KernelChoice::kResident, plan, &why);  // (the packed gather exists in the v2 kernel only)
    if (rc) return fail(rc, why);
    if (!example_kernel_is_resident(plan.p, plan.threads))
        return fail(FWGPU_ERR_INVALID, "packed regressor: the launch shape is not served (workgroups of at most 512 threads, at most 2048 FFM features per example)");
    if ((rc = fresh_work_counter(b, plan.p, stream))) return rc;
    record_launch(r, plan, true, FWGPU_OPT_SGD);
    FWGPU_HIP(launch_packed_predict(plan.p, r->q_increment, r->q_min, plan.grid, plan.threads, stream));
    return FWGPU_OK;
}

// Why the requests kernels (requests.hip) do not serve this regressor / batch shape, or NULL.  Asked when a set is attached and again at every launch.
const char *requests_refusal(const fwgpu_regressor *r, const fwgpu_batch *b) {
    const uint32_t k = r->cfg.ffm_k, F = r->cfg.ffm_num_fields;
    if (r->packed() && !r->packed_caches) return "a packed regressor keeps no device-side context cache";
    if (r->nn.n_layers) return "models with a deep head are not served by the requests route (fwgpu_batch_set_cache serves them)";
    if (b->records) return "a record batch is not served by the requests route (an entry batch of the filtered buffers is)";
    if (b->host_copy) return "the batch holds an oversize example (more than 4096 entries of a kind, or beyond the fused kernel's LDS)";
    if (k == 0) return "the model has no FFM block";
    if (k % 4 != 0) return "ffm_k is no multiple of 4 (the requests kernel has no one-float-per-lane form)";
    if (F > 256) return "more than 256 fields";
    if (!b->aligned4) return "an FFM entry's row does not start on a 16-byte boundary (hash & 3 != 0)";
    return nullptr;
}

// predict-only launch of an entry batch with a cache per example: base(S) of every cache of the set, then one wavefront per candidate, on `stream`
// (`rows`: the packed predict kernel's rows in flight, 0 = its default -- fwgpu_debug_requests_time)
static int run_batch_requests(fwgpu_regressor *r, fwgpu_batch *b, int update, hipStream_t stream, int rows = 0) {
    if (update) return fail(FWGPU_ERR_INVALID, "a batch with a cache per example (fwgpu_batch_set_caches) is predict-only: update must be 0");
    if (const char *why = requests_refusal(r, b)) return fail(FWGPU_ERR_INVALID, std::string("requests route: ") + why);
    for (const fwgpu_block_cache *c : b->req_caches)
        if (cache_is_stale(r, c)) return fail(FWGPU_ERR_INVALID, std::string("requests route: ") + kStaleCache);
    const uint32_t F = r->cfg.ffm_num_fields, k = r->cfg.ffm_k, R = F * k;
    RequestsShape shape;
    if (!requests_launch_shape(F, R, b->max_ffm, r->lds_per_cu, &shape))
        return fail(FWGPU_ERR_RANGE, "requests route: min(fields, the batch's largest FFM entry count) * F * k floats of one candidate do not fit the 160 KiB LDS");
    RequestsParams p{};
    p.ffm_w = r->packed() ? nullptr : r->d_ffm_w;
    p.ffm_q = r->d_ffm_q;  // (packed: 16-bit buckets and the header as it is NOW -- a refresh or a hot patch is seen by this launch)
    p.q_increment = r->q_increment;
    p.q_min = r->q_min;
    p.lr = r->d_lr;        // (a packed regressor keeps its LR weights as {w, 0} pairs: the same layout)
    p.ffm_hash = b->ffm_hash;
    p.ffm_val = b->ffm_val;
    p.ffm_fld = b->ffm_fld;
    p.ffm_off = b->ffm_off;
    p.lr_hash = b->lr_hash;
    p.lr_val = b->lr_val;
    p.lr_off = b->lr_off;
    p.pred = b->pred;
    p.cache_T = b->req_T;
    p.cache_of = b->req_of;
    p.base = b->req_base;
    p.n = b->n;
    p.n_caches = (uint32_t)b->req_caches.size();
    p.F = F;
    p.k = k;
    p.R = R;
    p.slots = shape.slots;
    p.has_lr = r->cfg.wiring == FWGPU_WIRING_REGRESSOR;
    LaunchRecord l{};
    l.family = r->packed() ? FWGPU_KERNEL_PACKED_REQUESTS : FWGPU_KERNEL_REQUESTS;
    l.chunks = (int32_t)shape.chunks;
    l.threads = (int32_t)shape.threads;
    l.lds_bytes = (int32_t)shape.lds_bytes;
    launched(r, l);
    FWGPU_HIP(launch_requests(p, shape, stream, rows));
    return FWGPU_OK;
}

// Predict-only batches of a model with a deep head (hold-out passes, serving): the weights are frozen, so nothing orders the examples and the head need
// not run per example.  The FFM / LR part runs on the v2 kernel (two workgroups per CU, no dense traffic) and leaves every example's head input x
// (regressor.rs:185-189: LR combo sums | triangle) in a batch buffer; the layers then take the batch through v_mfma_f32_32x32x2_f32 GEMMs, slab by slab
// (head.hip head_step, update = false) -- the dense weights are read once per slab instead of once per example (block_neural.rs:196-222 per example:
// 0.77 MB of weights for 1.2 MFLOP).  Same numbers as the per-example forward up to the order of the f32 sums.
static constexpr uint32_t kHeadPredictSlab = 32768;
static bool head_predict_batched(const fwgpu_regressor *r, const fwgpu_batch *b, int mode, int update) {
    static const bool env_off = getenv("FWGPU_HEAD_PREDICT_PER_EXAMPLE") != nullptr;  // A/B runs: the per-example forward for every launch
    const bool off = r->launch.head_predict >= 0 ? r->launch.head_predict == 0 : env_off;  // (fwgpu_debug_set_option 14 overrides the environment)
    if (off || update || !r->nn.n_layers || mode != FWGPU_MODE_HOGWILD || b->n < 256 || b->emit_T) return false;
    const uint32_t k = r->cfg.ffm_k, R = k * r->cfg.ffm_num_fields;
    return k && k % 4 == 0 && b->aligned4 && (R <= 256 || (R <= 512 && 256 % k == 0)) && r->launch.kernel_version != 1;
}
static int run_batch_head_predict(fwgpu_regressor *r, fwgpu_batch *b, hipStream_t stream) {
    const uint32_t X = r->nn.X;
    if (r->pred_cap < b->n) {
        FWGPU_HIP(hipStreamSynchronize(stream));
        if (r->pred_x) (void)hipFree(r->pred_x);
        if (r->pred_yi) (void)hipFree(r->pred_yi);
        r->pred_x = r->pred_yi = nullptr;
        r->pred_cap = 0;
        if (hipMalloc((void **)&r->pred_x, (size_t)b->n * X * sizeof(float)) != hipSuccess || hipMalloc((void **)&r->pred_yi, (size_t)b->n * 2 * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(FWGPU_ERR_OOM, "predict batch with a deep head: no memory for the head's inputs");
        }
        r->pred_cap = b->n;
    }
    LaunchPlan plan;
    const char *why = nullptr;
    int rc = plan_head_inputs(r, b, plan, &why);
    if (rc) return fail(rc, why);
    if ((rc = fresh_work_counter(b, plan.p, stream))) return rc;
    record_launch(r, plan, false, r->cfg.optimizer);
    FWGPU_HIP(launch_example_kernel(plan.p, r->cfg.optimizer, false, plan.grid, plan.threads, stream));
    fwgpu_split view;
    view.owner = r;
    view.d_x = r->pred_x;
    view.d_g = r->pred_yi;
    for (uint32_t first = 0; first < b->n; first += kHeadPredictSlab) {
        rc = head_step(r, &view, first, std::min(kHeadPredictSlab, b->n - first), b->pred + first, /*update=*/false, stream);
        if (rc) return rc;
    }
    return FWGPU_OK;
}

// the fused example kernel, the deep head (if any) per example inside it
static int run_batch_fused(fwgpu_regressor *r, fwgpu_batch *b, int mode, int update, hipStream_t stream) {
    LaunchPlan plan;
    const char *why = nullptr;
    int rc = plan_launch(r, b, mode, update, KernelChoice::kOwn, plan, &why);
    if (rc) return fail(rc, why);
    if ((rc = fresh_work_counter(b, plan.p, stream))) return rc;
    // An updating launch always uses device-scope (sc1) accesses; read-only launches use cached loads.
    record_launch(r, plan, false, r->cfg.optimizer);
    FWGPU_HIP(launch_example_kernel(plan.p, r->cfg.optimizer, update != 0, plan.grid, plan.threads, stream));
    return FWGPU_OK;
}

// The FWGPU_ROUTE_* a batch takes, from the regressor and the batch alone -- also where that route then refuses the launch (an updating launch of a
// packed regressor or of a batch with a set) and, for a packed regressor, where there is nothing to launch.
static int32_t pick_route(const fwgpu_regressor *r, const fwgpu_batch *b, int mode, int update) {
    if (r->packed()) {  // fwgpu_packed_enable_caches: one cache (fwgpu_batch_set_cache) or a set
        return r->packed_caches && b->n && !b->req_caches.empty() ? FWGPU_ROUTE_REQUESTS : FWGPU_ROUTE_PACKED;
    }
    if (b->n == 0) return FWGPU_ROUTE_NONE;
    if (!b->req_caches.empty()) return FWGPU_ROUTE_REQUESTS;  // a cache per example (fwgpu_batch_set_caches): the requests kernels, in both modes
    if (b->host_copy) return FWGPU_ROUTE_HOST_WALK;           // (an example beyond what the fused kernel stages: see learn_one_chunked)
    return head_predict_batched(r, b, mode, update) ? FWGPU_ROUTE_HEAD_BATCHED : FWGPU_ROUTE_FUSED;
}

int run_batch(fwgpu_regressor *r, fwgpu_batch *b, int mode, int update, hipStream_t stream, int32_t *route) {
    const int32_t taken = pick_route(r, b, mode, update);
    if (route) *route = taken;
    switch (taken) {
    case FWGPU_ROUTE_NONE: return FWGPU_OK;
    case FWGPU_ROUTE_REQUESTS: return run_batch_requests(r, b, update, stream);
    case FWGPU_ROUTE_PACKED: return run_batch_packed(r, b, mode, update, stream);
    case FWGPU_ROUTE_HOST_WALK: return run_batch_by_example(r, b, update, stream);
    case FWGPU_ROUTE_HEAD_BATCHED: {
        const int rc = run_batch_head_predict(r, b, stream);
        if (rc != FWGPU_ERR_RANGE) {
            if (route && rc == FWGPU_OK) r->pred_n = b->n;
            return rc;
        }
        if (route) *route = FWGPU_ROUTE_HEAD_BATCHED_REFUSED;  // (a shape the v2 kernel cannot stage: the per-example forward)
        return run_batch_fused(r, b, mode, update, stream);
    }
    default: return run_batch_fused(r, b, mode, update, stream);
    }
}

int run_batch_peer(fwgpu_regressor *r, fwgpu_batch *b, int mode, int update, const PeerShards *d_shards, hipStream_t stream,
                   const PushRings *d_push, uint32_t stream_consumers, uint32_t device_share, uint32_t stream_max_consumer_waves, uint32_t n_ranks) {
    if (int rcp = refuse_packed(r, "peer-sharded tables")) return rcp;
    if (b->n == 0 && !stream_consumers) return FWGPU_OK;  // (a streaming step launches for an empty batch too: the rank's consumers serve the peers)
    if (r->nn.n_layers) return fail(FWGPU_ERR_INVALID, "peer-sharded tables: models with a deep head are not covered");
    LaunchPlan plan;
    const char *why = nullptr;
    int rc = plan_launch(r, b, mode, update, KernelChoice::kGeneric, plan, &why);  // the generic kernel carries the owner lookup (kernels.hip ffm_w_base / lr_base)
    if (rc) return fail(rc, why);
    KernelParams &p = plan.p;
    p.shards = d_shards;
    p.push = d_push;
    if (d_push) p.hot_lr_every = 0;  // (owner-side apply: every LR gradient travels to its owner, the constant feature's included)
    p.host_extra_wgs = stream_consumers;
    p.host_share = device_share;
    p.host_stream_max_consumer_waves = stream_max_consumer_waves;
    p.host_stream_min_consumer_waves = (d_push && stream_consumers) ? 2u * (n_ranks ? n_ranks : 1u) : 0u;
    FWGPU_HIP(hipMemsetAsync(b->work, 0, sizeof(uint32_t), stream));
    record_launch(r, plan, false, r->cfg.optimizer);
    FWGPU_HIP(launch_example_kernel(p, r->cfg.optimizer, update != 0, plan.grid, plan.threads, stream));
    return FWGPU_OK;
}

// a batch with an example beyond what the fused kernel stages keeps its entries on the host: it is walked example by example (run_batch)
// does the batch's largest example fit what a workgroup of the fused kernel stages?  (fewer than 4096 entries of each kind can still be more than the
// LDS holds: at k = 8 x 30 fields about 2.5 k features, at k = 16 far fewer -- ADVICE r4)
static bool batch_fits_fused_kernel(fwgpu_batch *b) {
    if (b->max_ffm > 4096 || b->max_lr > 4096) return false;
    if (!b->owner) return true;
    LaunchPlan plan;
    const char *why = nullptr;
    // (a refusal is not an error of the caller's: the batch takes the example-by-example path)
    return plan_launch(b->owner, b, FWGPU_MODE_HOGWILD, 1, KernelChoice::kOwn, plan, &why) != FWGPU_ERR_RANGE;
}
void keep_host_copy_if_oversize(fwgpu_batch *b, HostBatch &&hb) {
    if (hb.max_ffm > 4096 || hb.max_lr > 4096 || !batch_fits_fused_kernel(b)) b->host_copy.reset(new HostBatch(std::move(hb)));
}
bool record_batch_is_oversize(fwgpu_batch *b) { return !batch_fits_fused_kernel(b); }
// ... a RECORD batch (just uploaded: max_ffm / max_lr are known) with a record that translates to more entries than that: translated on the host
int record_batch_host_copy_if_oversize(fwgpu_regressor *r, const fwgpu_translator_config *t, fwgpu_batch *b, const uint32_t *records,
                                       const uint64_t *rec_off, uint32_t n) {
    b->host_copy.reset();
    if (batch_fits_fused_kernel(b)) return FWGPU_OK;
    HostBatch hb;
    hb.clear();
    std::vector<fwgpu_lr_entry> lr;
    std::vector<fwgpu_ffm_entry> ffm;
    for (uint32_t i = 0; i < n; i++) {
        float label, imp;
        int rc = translate_record(t, records + rec_off[i], (uint32_t)(rec_off[i + 1] - rec_off[i]), lr, ffm, &label, &imp);
        if (rc == FWGPU_OK) rc = append_example(r, hb, lr.data(), (uint32_t)lr.size(), ffm.data(), (uint32_t)ffm.size(), label, imp);
        if (rc) return rc;
    }
    keep_host_copy_if_oversize(b, std::move(hb));
    return FWGPU_OK;
}

// ------------------------------------------------------------------ single example

int ensure_one(fwgpu_regressor *r, uint32_t n_lr, uint32_t n_ffm) {
    if (r->one && r->one->n_lr >= n_lr && r->one->n_ffm >= n_ffm) return FWGPU_OK;
    if (r->one) {
        fwgpu_batch_free(r->one);
        r->one = nullptr;
    }
    return batch_alloc(r, 1, std::max<uint32_t>(n_lr * 2, 256), std::max<uint32_t>(n_ffm * 2, 256), &r->one, /*host_mapped=*/true);
}

// the single example's prediction, once the launch has finished
int one_prediction(fwgpu_regressor *r, float *prediction) {
    FWGPU_HIP(hipStreamSynchronize(0));
    *prediction = *reinterpret_cast<const float *>(reinterpret_cast<const unsigned char *>(r->one->pred) + r->one->host_delta);
    return FWGPU_OK;
}

// ---- examples beyond the fused kernel's LDS budget.
// The reference takes an example of any size (block_ffm.rs:294-312: the gradient cache moves to the heap beyond 170 393 floats, the algorithm
// stays what it is).  The fused kernel stages an example's entries in LDS: 4096 FFM features / LR entries at most.  A larger example takes the
// synchronous pipeline instead, CHUNK by chunk -- field sums and LR sums are additive over features:
//   FWD   every chunk of <= kChunkEntries entries is a pseudo-example of a small batch: its partial field sums, self-pair corrections and LR sum
//         go to its split record, its features' own slots to the selfw buffer (pre-update weights, as block_ffm.rs:219-261 uses them);
//   sum   the chunks' records are added in chunk order and the total is copied back into every chunk's record;
//   MID   logit, prediction and general gradient once, from the total;
//   UPD   the chunks IN ORDER on one workgroup, each with the total record: AdaGrad per occurrence in buffer order, rows that repeat or
//         overlap across chunks included (a later chunk re-reads what an earlier one wrote), exactly the reference's update loop (block_ffm.rs:265-288).
// Only the order of the field sums' additions differs from the reference (chunk subtotals): ~1e-7 relative.  Models with a deep head are not covered.
constexpr uint32_t kMaxStagedEntries = 4096;  // what one workgroup of the fused kernel stages (plan_launch)
constexpr uint32_t kChunkEntriesMax = 2048;
// entries per chunk: what the pipeline's workgroups stage beside the field sums (k floats of own-field weights and ~9 words per entry), a power of two
static uint32_t chunk_entries(const fwgpu_regressor *r) {
    const size_t k = r->cfg.ffm_k, F = k ? r->cfg.ffm_num_fields : 0, fixed = 4 * F * F * k + 12288;
    uint32_t n = kChunkEntriesMax;
    while (n > 64 && fixed + (size_t)n * (4 * k + 36) > r->lds_per_cu) n >>= 1;
    return n;
}

static int learn_one_chunked(fwgpu_regressor *r, const HostBatch &hb, uint32_t e, int update, float *prediction) {
    if (int rcp = refuse_packed(r, "an example beyond what one workgroup stages (the chunked pipeline)")) return rcp;
    // With a deep head (regressor.rs:191-323) the chunks' partial records still add up -- per-combo LR sums, field sums, corrections, counts -- so MID forms
    // the head's input x from the TOTAL record once, the head runs once on it (a "mini-batch" of one example is the reference's per-example rule: one
    // AdaGrad step per dense weight with this example's gradient, input gradients from the pre-step weights, block_neural.rs:252-340), and every chunk's
    // update takes the example's per-slot gradients dx.
    const bool head = r->nn.n_layers != 0;
    const uint32_t f0 = hb.ffm_off[e], f1 = hb.ffm_off[e + 1], l0 = hb.lr_off[e], l1 = hb.lr_off[e + 1];
    const uint32_t nf = f1 - f0, nl = l1 - l0, kChunkEntries = chunk_entries(r);
    const uint32_t m = std::max<uint32_t>(1, std::max((nf + kChunkEntries - 1) / kChunkEntries, (nl + kChunkEntries - 1) / kChunkEntries));
    HostBatch hc;
    hc.clear();
    for (uint32_t j = 0; j < m; j++) {
        const uint32_t fa = std::min(nf, j * kChunkEntries), fb = std::min(nf, (j + 1) * kChunkEntries);
        const uint32_t la = std::min(nl, j * kChunkEntries), lb = std::min(nl, (j + 1) * kChunkEntries);
        hc.append_slice(hb, e, f0 + fa, f0 + fb, l0 + la, l0 + lb);
    }
    fwgpu_batch *cb = nullptr;
    fwgpu_split *sp = nullptr;
    int rc = batch_alloc(r, m, hc.lr_hash.size(), hc.ffm_hash.size(), &cb);
    if (rc == FWGPU_OK) rc = batch_upload(cb, hc, 0);
    if (rc == FWGPU_OK) rc = fwgpu_split_create(r, m, kChunkEntries, &sp);
    auto done = [&](int code) {
        (void)hipStreamSynchronize(0);
        if (cb) fwgpu_batch_free(cb);
        if (sp) fwgpu_split_free(sp);
        return code;
    };
    if (rc) return done(rc);
    SplitRanges rg;
    rg.home_lo = 0;
    rg.home_hi = m;  // every chunk is "home": the features-per-field counts of the chunks add up like the sums (the head's diagonal needs the example's)
    if ((rc = split_forward(r, cb, sp, FWGPU_MODE_HOGWILD, rg, 0))) return done(rc);
    const size_t SL = sp->split_len;
    for (uint32_t j = 1; j < m; j++)
        if (launch_add(sp->d_split, sp->d_split + (size_t)j * SL, SL, 0) != hipSuccess) return done(fail(FWGPU_ERR_DEVICE, "chunked example: add failed"));
    {   // ... the label and the importance enter the total ONCE (every chunk carried them)
        const uint32_t F = r->cfg.ffm_k ? r->cfg.ffm_num_fields : 0, R = F * r->cfg.ffm_k;
        const float li[2] = {hb.label[e], hb.importance[e]};
        if (hipMemcpyAsync(sp->d_split + (size_t)F * R + 2 * (size_t)F + sp->nlr, li, sizeof(li), hipMemcpyHostToDevice, 0) != hipSuccess || hipStreamSynchronize(0) != hipSuccess)
            return done(fail(FWGPU_ERR_DEVICE, "chunked example: label write failed"));
    }
    if ((rc = split_mid(r, sp, 0, 1, cb->pred, head, 0))) return done(rc);
    const bool upd = update && hb.importance[e] != 0.0f;  // regressor.rs:366
    if (head && (rc = head_step(r, sp, 0, 1, cb->pred, upd, 0))) return done(rc);
    if (upd) {
        const size_t X = head ? r->nn.X : 0;
        for (uint32_t j = 1; j < m; j++) {
            if (hipMemcpyAsync(sp->d_split + (size_t)j * SL, sp->d_split, SL * 4, hipMemcpyDeviceToDevice, 0) != hipSuccess ||
                (!head && hipMemcpyAsync(sp->d_g + j, sp->d_g, 4, hipMemcpyDeviceToDevice, 0) != hipSuccess) ||
                (head && hipMemcpyAsync(sp->d_dx + (size_t)j * X, sp->d_dx, X * 4, hipMemcpyDeviceToDevice, 0) != hipSuccess))
                return done(fail(FWGPU_ERR_DEVICE, "chunked example: copy failed"));
        }
        if ((rc = split_update(r, cb, sp, FWGPU_MODE_SEQUENTIAL, rg, head, 0))) return done(rc);
    }
    if (hipMemcpyAsync(prediction, cb->pred, 4, hipMemcpyDeviceToHost, 0) != hipSuccess) return done(fail(FWGPU_ERR_DEVICE, "chunked example: read-back failed"));
    return done(FWGPU_OK);
}

// one example of a host batch through the single-example path (fused kernel in order, or chunk by chunk)
static int learn_host_example(fwgpu_regressor *r, const HostBatch &hb, uint32_t e, int update, float *prediction) {
    const uint32_t nf = hb.ffm_off[e + 1] - hb.ffm_off[e], nl = hb.lr_off[e + 1] - hb.lr_off[e];
    if (nf > kMaxStagedEntries || nl > kMaxStagedEntries) return learn_one_chunked(r, hb, e, update, prediction);
    HostBatch one;
    one.clear();
    one.append_slice(hb, e, hb.ffm_off[e], hb.ffm_off[e + 1], hb.lr_off[e], hb.lr_off[e + 1]);
    int rc = ensure_one(r, nl, nf);
    if (rc) return rc;
    if ((rc = batch_upload(r->one, one, 0))) return rc;
    rc = run_batch(r, r->one, FWGPU_MODE_SEQUENTIAL, update, 0);
    if (rc == FWGPU_ERR_RANGE) return learn_one_chunked(r, hb, e, update, prediction);
    if (rc) return rc;
    return one_prediction(r, prediction);
}

// A batch that holds an oversize example keeps its host copy (fwgpu_batch::host_copy) and is walked example by example, in order, whatever the
// mode: the in-order result is one of the outcomes hogwild allows.  The rare path: three launches per chunked example.
static int run_batch_by_example(fwgpu_regressor *r, fwgpu_batch *b, int update, hipStream_t stream) {
    FWGPU_HIP(hipStreamSynchronize(stream));
    const HostBatch &hb = *b->host_copy;
    std::vector<float> preds(hb.size());
    for (uint32_t e = 0; e < hb.size(); e++) {
        int rc = learn_host_example(r, hb, e, update, &preds[e]);
        if (rc) return rc;
    }
    FWGPU_HIP(hipMemcpy(b->pred, preds.data(), preds.size() * 4, hipMemcpyHostToDevice));
    return FWGPU_OK;
}

static int learn_one(fwgpu_regressor *r, const fwgpu_lr_entry *lr, uint32_t n_lr, const fwgpu_ffm_entry *ffm,
                     uint32_t n_ffm, float label, float importance, int update, float *prediction) {
    if (!r || !prediction) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if ((n_lr && !lr) || (n_ffm && !ffm)) return fail(FWGPU_ERR_INVALID, "NULL entry buffer");
    FWGPU_HIP(hipSetDevice(r->device));
    HostBatch hb;
    hb.clear();
    int rc = append_example(r, hb, lr, n_lr, ffm, n_ffm, label, importance);
    if (rc) return rc;
    if (hb.max_ffm > kMaxStagedEntries || hb.max_lr > kMaxStagedEntries) return learn_one_chunked(r, hb, 0, update, prediction);
    rc = ensure_one(r, (uint32_t)hb.lr_hash.size(), (uint32_t)hb.ffm_hash.size());
    if (rc) return rc;
    rc = batch_upload(r->one, hb, 0);
    if (rc) return rc;
    rc = run_batch(r, r->one, FWGPU_MODE_SEQUENTIAL, update, 0);
    // (fewer than 4096 entries of each kind, but together more than the LDS holds: plan_launch refuses before anything is launched)
    if (rc == FWGPU_ERR_RANGE) return learn_one_chunked(r, hb, 0, update, prediction);
    if (rc) return rc;
    return one_prediction(r, prediction);
}

static int split_params(fwgpu_regressor *r, fwgpu_batch *b, fwgpu_split *sp, int mode, int update, const SplitRanges &rg, LaunchPlan &plan) {
    if (!r || !b || !sp) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (b->owner != r || sp->owner != r) return fail(FWGPU_ERR_INVALID, "batch / split buffers belong to another regressor");
    if (b->n > sp->n_cap) return fail(FWGPU_ERR_RANGE, "split buffers are smaller than the batch");
    const char *why = nullptr;
    int rc = plan_launch(r, b, mode, update, KernelChoice::kOwn, plan, &why);
    if (rc) return fail(rc, why);
    KernelParams &p = plan.p;
    if ((uint64_t)p.max_ffm * std::max<uint32_t>(1, p.k) > sp->selfw_stride)
        return fail(FWGPU_ERR_RANGE, "split buffers: an example has more FFM features than they were created for");
    p.split = sp->d_split;
    p.split_len = sp->split_len;
    p.split_nlr = sp->nlr;
    p.split_selfw = sp->d_selfw;
    p.selfw_stride = sp->selfw_stride;
    p.gbuf = sp->d_g;
    p.own_lo_ffm = rg.ffm_lo;
    p.own_hi_ffm = rg.ffm_hi;
    p.own_lo_lr = rg.lr_lo;
    p.own_hi_lr = rg.lr_hi;
    p.home_lo = rg.home_lo;
    p.home_hi = rg.home_hi;
    return FWGPU_OK;
}

int split_forward(fwgpu_regressor *r, fwgpu_batch *b, fwgpu_split *sp, int mode, const SplitRanges &rg, hipStream_t stream,
                  const OccBuffers *occ, uint32_t *max_ffm, uint32_t *max_lr) {
    if (b && b->n == 0) return FWGPU_OK;
    LaunchPlan plan;
    int rc = split_params(r, b, sp, mode, 0, rg, plan);
    if (rc) return rc;
    KernelParams &p = plan.p;
    if (occ) {
        p.occ_ffm_key = occ->ffm_key;
        p.occ_ffm_desc = occ->ffm_desc;
        p.occ_lr_key = occ->lr_key;
        p.occ_lr_desc = occ->lr_desc;
    }
    if (max_ffm) *max_ffm = p.max_ffm;  // the slot strides of the occurrence lists
    if (max_lr) *max_lr = p.max_lr;
    FWGPU_HIP(hipMemsetAsync(b->work, 0, sizeof(uint32_t), stream));
    FWGPU_HIP(launch_example_phase(p, r->cfg.optimizer, 1, plan.grid, plan.threads, stream));
    return FWGPU_OK;
}

// records [first, first + n) of `sp` -> predictions into pred (device, n floats) and general gradients / head inputs
int split_mid(fwgpu_regressor *r, fwgpu_split *sp, uint32_t first, uint32_t n, float *d_pred, bool head, hipStream_t stream) {
    if (!n) return FWGPU_OK;
    KernelParams p{};
    p.F = r->cfg.ffm_k ? r->cfg.ffm_num_fields : 0;
    p.k = r->cfg.ffm_k;
    p.R = p.F * p.k;
    p.has_lr = r->cfg.wiring == FWGPU_WIRING_REGRESSOR;
    p.nn = r->nn;
    p.split = sp->d_split + (size_t)first * sp->split_len;
    p.split_len = sp->split_len;
    p.split_nlr = sp->nlr;
    p.pred = d_pred;
    p.gbuf = head ? sp->d_g + 2 * (size_t)first : sp->d_g + first;
    p.xbuf = head ? sp->d_x + (size_t)first * r->nn.X : nullptr;
    FWGPU_HIP(launch_split_mid(p, n, stream));
    return FWGPU_OK;
}

int split_update(fwgpu_regressor *r, fwgpu_batch *b, fwgpu_split *sp, int mode, const SplitRanges &rg, bool head, hipStream_t stream) {
    if (b && b->n == 0) return FWGPU_OK;
    LaunchPlan plan;
    int rc = split_params(r, b, sp, mode, 1, rg, plan);
    if (rc) return rc;
    plan.p.dxbuf = head ? sp->d_dx : nullptr;
    FWGPU_HIP(hipMemsetAsync(b->work, 0, sizeof(uint32_t), stream));
    FWGPU_HIP(launch_example_phase(plan.p, r->cfg.optimizer, 3, plan.grid, plan.threads, stream));
    return FWGPU_OK;
}
}  // namespace fwgpu

using namespace fwgpu;

extern "C" {

int fwgpu_learn(fwgpu_regressor *r, const fwgpu_lr_entry *lr, uint32_t n_lr, const fwgpu_ffm_entry *ffm, uint32_t n_ffm,
                float label, float importance, int update, float *prediction) {
    return learn_one(r, lr, n_lr, ffm, n_ffm, label, importance, update, prediction);
}

int fwgpu_predict(fwgpu_regressor *r, const fwgpu_lr_entry *lr, uint32_t n_lr, const fwgpu_ffm_entry *ffm,
                  uint32_t n_ffm, float *prediction) {
    return learn_one(r, lr, n_lr, ffm, n_ffm, 0.0f, 1.0f, 0, prediction);
}

// One synchronous micro-batch on one GPU: all of b's examples are scored with the weights as they are, then all updates are
// applied (FWGPU_MODE_SEQUENTIAL: in example order, on one workgroup -- the deterministic mode the oracle's micro-batch
// mode is compared with; FWGPU_MODE_HOGWILD: concurrently).  Models with a deep head take the mini-batched head (head.hip).
int fwgpu_learn_batch_sync(fwgpu_regressor *r, fwgpu_batch *b, fwgpu_split *sp, int mode, void *stream_) {
    if (!r || !b || !sp) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (mode != FWGPU_MODE_SEQUENTIAL && mode != FWGPU_MODE_HOGWILD) return fail(FWGPU_ERR_INVALID, "unknown mode");
    if (int rcp = refuse_packed(r, "learn_batch_sync")) return rcp;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    FWGPU_HIP(hipSetDevice(r->device));
    SplitRanges rg;
    rg.home_hi = b->n;
    const bool head = r->nn.n_layers != 0;
    int rc = split_forward(r, b, sp, mode, rg, stream);
    if (rc == FWGPU_OK) rc = split_mid(r, sp, 0, b->n, b->pred, head, stream);
    if (rc == FWGPU_OK && head) rc = head_step(r, sp, 0, b->n, b->pred, /*update=*/true, stream);
    if (rc == FWGPU_OK) rc = split_update(r, b, sp, mode, rg, head, stream);
    return rc;
}

int fwgpu_learn_batch(fwgpu_regressor *r, fwgpu_batch *b, int mode, int update, void *stream) {
    if (!r || !b) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (b->owner != r) return fail(FWGPU_ERR_INVALID, "batch belongs to another regressor");
    if (mode != FWGPU_MODE_SEQUENTIAL && mode != FWGPU_MODE_HOGWILD) return fail(FWGPU_ERR_INVALID, "unknown mode");
    r->pred_n = 0;
    r->last_route = FWGPU_ROUTE_NONE;
    return run_batch(r, b, mode, update, static_cast<hipStream_t>(stream), &r->last_route);
}

int fwgpu_debug_last_route(const fwgpu_regressor *r, int *route) {
    if (!r || !route) return fail(FWGPU_ERR_INVALID, "NULL argument");
    *route = r->last_route;
    return FWGPU_OK;
}

int fwgpu_debug_last_launch(const fwgpu_regressor *r, int32_t *out, uint32_t n) {
    if (!r || !out) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (n > FWGPU_LAUNCH_INFO_LEN) return fail(FWGPU_ERR_RANGE, "last_launch: more fields than the library fills (FWGPU_LAUNCH_INFO_LEN)");
    for (uint32_t i = 0; i < n; i++) out[i] = r->last_launch[i];
    return FWGPU_OK;
}

int fwgpu_debug_head_inputs(fwgpu_regressor *r, float *out, uint64_t n_floats) {
    if (!r || !out) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (r->last_route != FWGPU_ROUTE_HEAD_BATCHED || !r->pred_n || !r->pred_x)
        return fail(FWGPU_ERR_INVALID, "head_inputs: the regressor's last batch launch was not a batched head predict");
    if (n_floats > (uint64_t)r->pred_n * r->nn.X) return fail(FWGPU_ERR_RANGE, "head_inputs: more floats than the last launch wrote (n * X)");
    FWGPU_HIP(hipDeviceSynchronize());  // (the launch may have run on a stream of the caller's)
    FWGPU_HIP(hipMemcpy(out, r->pred_x, n_floats * sizeof(float), hipMemcpyDeviceToHost));
    return FWGPU_OK;
}

int fwgpu_debug_requests_time(fwgpu_regressor *r, fwgpu_batch *b, int rows, uint32_t reps, float *ms_per_launch) {
    if (!r || !b || !ms_per_launch || reps == 0) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (b->owner != r) return fail(FWGPU_ERR_INVALID, "batch belongs to another regressor");
    if (b->req_caches.empty() || b->n == 0) return fail(FWGPU_ERR_INVALID, "debug_requests_time: the batch has no cache set attached");
    if (rows != 0 && rows != 4 && rows != 8) return fail(FWGPU_ERR_INVALID, "debug_requests_time: rows is 0 (the default), 4 or 8");
    if (rows && !r->packed()) return fail(FWGPU_ERR_INVALID, "debug_requests_time: an f32 table runs its own depth (rows = 0)");
    FWGPU_HIP(hipSetDevice(r->device));
    int rc = run_batch_requests(r, b, 0, 0, rows);  // (warm: the code object, the LDS attribute)
    if (rc) return rc;
    hipEvent_t ev[2] = {nullptr, nullptr};
    FWGPU_HIP(hipEventCreate(&ev[0]));
    hipError_t e = hipEventCreate(&ev[1]);
    if (e == hipSuccess) e = hipEventRecord(ev[0], 0);
    for (uint32_t i = 0; i < reps && e == hipSuccess && rc == FWGPU_OK; i++) rc = run_batch_requests(r, b, 0, 0, rows);
    if (e == hipSuccess) e = hipEventRecord(ev[1], 0);
    if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
    (void)hipEventDestroy(ev[0]);
    if (ev[1]) (void)hipEventDestroy(ev[1]);
    if (rc) return rc;
    if (e != hipSuccess) return fail(FWGPU_ERR_DEVICE, std::string("debug_requests_time: ") + hipGetErrorString(e));
    *ms_per_launch = ms / (float)reps;
    return FWGPU_OK;
}

}  // extern "C"
