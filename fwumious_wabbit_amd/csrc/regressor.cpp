// Host side of the C ABI: the `Regressor` object (regressor.rs:142-147) that owns the device tables -- errors, create / free / init, the launch
// and debug setters, table access, weight (de)serialisation (regressor.rs:426-469) and the quantise / pack block.  Batches live in batch.cpp,
// every launch (single-example learn/predict, regressor.rs:356-395, and micro-batches) in launch.cpp, the context cache in context_cache.cpp.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>

#include "launch.h"

namespace fwgpu {

static thread_local std::string g_last_error;
void set_error(const std::string &msg) { g_last_error = msg; }
int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

// optimizer.rs:121-144 (host: runs once per block at create time, then lives in HBM)
// A packed regressor (fwgpu_model_load_packed) predicts and nothing else: everything that would write or train its tables is refused here, by name
int refuse_packed(const fwgpu_regressor *r, const char *what) {
    if (!r || !r->packed()) return FWGPU_OK;
    return fail(FWGPU_ERR_INVALID, std::string(what) + ": the regressor's FFM weights are packed f16 buckets (fwgpu_model_load_packed): it only predicts");
}

void lut_init(float *lut, float learning_rate, float power_t, float init_acc) {
    const float minus_power_t = -power_t;
    for (uint32_t x = 0; x < (uint32_t)kLutSize; x++) {
        uint32_t b0 = x << (31 - kLutBits), b1 = (x + 1) << (31 - kLutBits);
        float f0, f1;
        memcpy(&f0, &b0, 4);
        memcpy(&f1, &b1, 4);
        const float float_x = f0 + init_acc;
        const float float_x_plus_one = f1 + init_acc;
        float val = learning_rate * (powf(float_x, minus_power_t) + powf(float_x_plus_one, minus_power_t)) * 0.5f;
        if (std::isnan(val) || std::isinf(val)) val = learning_rate;
        lut[x] = val;
    }
}

float initial_acc(int optimizer, float init_acc) {
    // optimizer.rs:40-42 (SGD: no state), 90-92 (Flex: init_acc), 158-161 (LUT: 0.0, folded into the table)
    return optimizer == FWGPU_OPT_ADAGRAD_FLEX ? init_acc : 0.0f;
}

}  // namespace fwgpu

using namespace fwgpu;

extern "C" {

const char *fwgpu_last_error(void) { return g_last_error.c_str(); }
int fwgpu_abi_version(void) { return FWGPU_ABI_VERSION; }

// Where the accumulator table goes relative to the weight table.  Device memory on MI355X falls into groups (tools/placement.hip,
// profiles/r02_placement.txt): the FFM update's pattern -- whole-line read-modify-write of w[h..] and acc[h..] at once -- runs 17 %
// slower when both tables come from the same group (2.45 ms vs 2.04 ms per 3.3 M rows), whatever their addresses.  hipMalloc hands
// out consecutive allocations from one group for several GB, so for tables beyond the Infinity Cache a few candidate allocations
// are tried and timed against w with that very pattern (a fraction of a millisecond each); the fastest is kept, the rest freed.
// FWGPU_PLACEMENT=0 switches the search off (the first allocation is used, as for small tables).
// The search is BOUNDED by who else is on the device: alone (more than 85 % of the device memory free -- a training box) it may hold
// up to 112 candidates / half of the free memory for the few milliseconds it takes (a contending stretch of the allocator is up to
// ~72 table-GB long, profiles/r02_placement.txt; 24 and 64 candidates each left whole boxes on a contending pair this round:
// -10 % examples/s); with other tenants present at most 16 candidates and a tenth of the free memory, and only two candidates when
// more than half of the device is in use (other regressors, ranks, serving replicas must not run out of memory because this
// one is probing).  FWGPU_PLACEMENT=wide forces the wide scan, =0 switches the search off.
static int place_ffm_acc(fwgpu_regressor *r, size_t fbytes) {
    const char *env = std::getenv("FWGPU_PLACEMENT");
    const bool search = fbytes > (256u << 20) && !(env && env[0] == '0');
    const bool wide = env && env[0] == 'w';
    std::vector<float *> cand;
    float single = 0.0f, lo = 1e30f, hi = 0.0f;
    int best = 0;
    if (search) {
        // the weight table alone, until two consecutive readings agree (the first launches of a process run on ramping clocks)
        float prev = 0.0f;
        for (int i = 0; i < 24; i++) {
            if (pair_probe_ms(r->d_ffm_w, nullptr, fbytes, 400000, 2, &single) != hipSuccess) {
                (void)hipGetLastError();
                single = 0.0f;
                break;
            }
            if (prev > 0.0f && std::fabs(single - prev) < 0.02f * prev) break;
            prev = single;
        }
    }
    // the pair costs 1.8x the single table when the two do not contend, 2.2x when they do (profiles/r02_placement.txt)
    const float fast_below = 1.96f * single;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
        (void)hipGetLastError();
        free_b = 0;
    }
    // Candidates are allocations of the table's own size, held until the search ends so that hipMalloc keeps walking forward.
    // (Large "spacer" allocations to skip ahead do not work: they are assembled from elsewhere and the next table-sized block
    // still comes from the same stretch.)  A stretch of contending memory is up to ~72 table-GB long (tools/placement scan of
    // 200 x 1 GiB, profiles/r02_placement.txt), a probe costs about a millisecond.
    const bool crowded = total_b && free_b < total_b / 2;  // someone else (another process, other regressors) holds half the device
    const bool alone = total_b && free_b > total_b / 100 * 85;
    const size_t budget = (wide || alone) ? std::min<size_t>(free_b / 2, 128ull << 30) : free_b / 10;
    const size_t cap = (wide || alone) ? 112 : (crowded ? 2 : 16);
    const int max_tries = search && single > 0.0f ? (int)std::max<size_t>(2, std::min<size_t>(cap, budget / fbytes)) : 1;
    for (int t = 0; t < max_tries; t++) {
        float *c = nullptr;
        if (hipMalloc((void **)&c, fbytes) != hipSuccess) {
            (void)hipGetLastError();
            break;
        }
        cand.push_back(c);
        if (max_tries == 1) break;
        float t_ms = 0.0f;
        if (pair_probe_ms(r->d_ffm_w, c, fbytes, 400000, 2, &t_ms) != hipSuccess) {
            (void)hipGetLastError();
            break;  // (keep what there is; the probe is an optimisation)
        }
        hi = std::max(hi, t_ms);
        if (t_ms < lo) {
            lo = t_ms;
            best = t;
        }
        if (t_ms < fast_below) break;  // does not contend with w: done
    }
    if (cand.empty()) return fail(FWGPU_ERR_DEVICE, "out of device memory (FFM accumulators)");
    r->d_ffm_acc = cand[best];
    for (size_t i = 0; i < cand.size(); i++)
        if ((int)i != best) (void)hipFree(cand[i]);
    // (no search, or no candidate that does not contend: the launches assume contention and use whole-line accesses)
    r->placement_contended = fbytes > (256u << 20) && !(search && single > 0.0f && lo < fast_below);
    r->placement_tries = (int)cand.size();
    r->placement_ms_lo = hi > 0.0f ? lo : 0.0f;
    r->placement_ms_hi = hi;
    r->placement_ms_single = single;
    return FWGPU_OK;
}

static int create_impl(const fwgpu_config *cfg, bool packed, const uint8_t *packed_blob, fwgpu_regressor **out);
int fwgpu_create(const fwgpu_config *cfg, fwgpu_regressor **out) { return create_impl(cfg, false, nullptr, out); }

}  // extern "C"

// The packed form: `blob` is the quantised file's FFM block as it is (8-byte header {f32 increment, f32 min}, then one f16 bucket number per weight),
// lr_w the LR weights [2^bit_precision].  Neither an f32 weight table nor an accumulator table is ever allocated.
int fwgpu::create_packed(const fwgpu_config *cfg, const float *lr_w, const uint8_t *blob, fwgpu_regressor **out) {
    if (!cfg || !lr_w || !blob || !out) return fail(FWGPU_ERR_INVALID, "create_packed: NULL argument");
    if (cfg->optimizer != FWGPU_OPT_SGD) return fail(FWGPU_ERR_INVALID, "create_packed: a packed regressor is an immutable (SGD) one");
    if (!cfg->ffm_k) return fail(FWGPU_ERR_INVALID, "packed regressor: the model has no FFM block, there is nothing to pack");
    if (!packed_shape_ok(cfg->ffm_k, cfg->ffm_num_fields))
        return fail(FWGPU_ERR_INVALID, "packed regressor: ffm_k must be a multiple of 4 and a row (ffm_k x fields) at most 256 weights, or at most 512 with ffm_k dividing 256; got ffm_k = " +
                                           std::to_string(cfg->ffm_k) + ", fields = " + std::to_string(cfg->ffm_num_fields));
    fwgpu_regressor *r = nullptr;
    int rc = create_impl(cfg, true, blob, &r);
    if (rc) return rc;
    std::vector<float> tmp(r->lr_len * 2, 0.0f);
    for (uint64_t i = 0; i < r->lr_len; i++) tmp[2 * i] = lr_w[i];
    if (hipMemcpy(r->d_lr, tmp.data(), r->lr_len * 8, hipMemcpyHostToDevice) != hipSuccess) {
        fwgpu_free(r);
        return fail(FWGPU_ERR_DEVICE, "create_packed: LR upload failed");
    }
    *out = r;
    return FWGPU_OK;
}

extern "C" {

// packed: the FFM weights are a table of bucket numbers, filled from packed_blob or, without one, by the caller (fwgpu_pack_regressor)
static int create_impl(const fwgpu_config *cfg, bool packed, const uint8_t *packed_blob, fwgpu_regressor **out) {
    if (!cfg || !out) return fail(FWGPU_ERR_INVALID, "fwgpu_create: NULL argument");
    *out = nullptr;
    if (cfg->optimizer != FWGPU_OPT_SGD && cfg->optimizer != FWGPU_OPT_ADAGRAD_FLEX &&
        cfg->optimizer != FWGPU_OPT_ADAGRAD_LUT)
        return fail(FWGPU_ERR_INVALID, "fwgpu_create: unknown optimizer");
    if (cfg->bit_precision < 1 || cfg->bit_precision > 31) return fail(FWGPU_ERR_INVALID, "fwgpu_create: bit_precision out of range");
    if (cfg->ffm_k > 0) {
        if (cfg->ffm_bit_precision < 1 || cfg->ffm_bit_precision > 31)
            return fail(FWGPU_ERR_INVALID, "fwgpu_create: ffm_bit_precision out of range");
        if (cfg->ffm_num_fields == 0 || cfg->ffm_num_fields > 255)
            return fail(FWGPU_ERR_INVALID, "fwgpu_create: ffm_num_fields must be in 1..255");
        // block_ffm.rs:96-101
        if ((uint64_t)cfg->ffm_k * cfg->ffm_num_fields * cfg->ffm_num_fields > kFfmContraBufLen)
            return fail(FWGPU_ERR_INVALID, "FFM_CONTRA_BUF_LEN is 41472. It needs to be at least ffm_k * number_of_fields^2");
    }
    if (cfg->wiring != FWGPU_WIRING_REGRESSOR && cfg->wiring != FWGPU_WIRING_FFM_ONLY)
        return fail(FWGPU_ERR_INVALID, "fwgpu_create: unknown wiring");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(FWGPU_ERR_DEVICE, "fwgpu_create: no HIP device available (this library has no CPU path)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(FWGPU_ERR_DEVICE, "fwgpu_create: device ordinal out of range");
    std::unique_ptr<fwgpu_regressor> r(new fwgpu_regressor());
    r->cfg = *cfg;
    r->device = cfg->device;
    FWGPU_HIP(hipSetDevice(r->device));
    hipDeviceProp_t prop;
    FWGPU_HIP(hipGetDeviceProperties(&prop, r->device));
    r->num_cus = prop.multiProcessorCount;
    r->lds_per_cu = prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor : 64 * 1024;
    r->lr_len = 1ull << cfg->bit_precision;
    r->ffm_len = cfg->ffm_k ? (1ull << cfg->ffm_bit_precision) + (uint64_t)cfg->ffm_num_fields * cfg->ffm_k : 0;
    r->lr_hash_mask = lr_hash_mask(cfg->bit_precision);
    r->ffm_hash_mask = ffm_hash_mask(cfg->ffm_bit_precision, cfg->ffm_k);
    // (where the LR table lands relative to the FFM tables was measured not to matter: 3.55 ms per launch either way)
    FWGPU_HIP(hipMalloc((void **)&r->d_lr, r->lr_len * 2 * sizeof(float)));
    FWGPU_HIP(hipMemset(r->d_lr, 0, r->lr_len * 2 * sizeof(float)));
    if (r->ffm_len && packed) {
        // (+128 bytes of slack: the 8-byte vector of a lane beyond the last row's end stays in the allocation even without the descriptor's bound)
        r->ffm_q_bytes = r->ffm_len * 2 + 128;
        FWGPU_HIP(hipMalloc((void **)&r->d_ffm_q, r->ffm_q_bytes));
        FWGPU_HIP(hipMemset(reinterpret_cast<unsigned char *>(r->d_ffm_q) + r->ffm_len * 2, 0, 128));
        if (packed_blob) {
            memcpy(&r->q_increment, packed_blob, 4);
            memcpy(&r->q_min, packed_blob + 4, 4);
            FWGPU_HIP(hipMemcpy(r->d_ffm_q, packed_blob + 8, r->ffm_len * 2, hipMemcpyHostToDevice));
        }
    } else if (r->ffm_len) {
        // +64 floats of slack so that a 16 B vector at the very end of the spill-over tail stays in the allocation
        const size_t fbytes = (r->ffm_len + 64) * sizeof(float);
        FWGPU_HIP(hipMalloc((void **)&r->d_ffm_w, fbytes));
        int rc = place_ffm_acc(r.get(), fbytes);
        if (rc) return rc;
        FWGPU_HIP(hipMemset(r->d_ffm_w, 0, fbytes));
        FWGPU_HIP(hipMemset(r->d_ffm_acc, 0, fbytes));
    }
    // each block owns its optimizer instance: block_lr.rs:63-65, block_ffm.rs:86-91
    std::vector<float> lut(kLutSize);
    FWGPU_HIP(hipMalloc((void **)&r->d_lut_lr, kLutSize * sizeof(float)));
    FWGPU_HIP(hipMalloc((void **)&r->d_lut_ffm, kLutSize * sizeof(float)));
    lut_init(lut.data(), cfg->learning_rate, cfg->power_t, cfg->init_acc_gradient);
    FWGPU_HIP(hipMemcpy(r->d_lut_lr, lut.data(), kLutSize * sizeof(float), hipMemcpyHostToDevice));
    lut_init(lut.data(), cfg->ffm_learning_rate, cfg->ffm_power_t, cfg->ffm_init_acc_gradient);
    FWGPU_HIP(hipMemcpy(r->d_lut_ffm, lut.data(), kLutSize * sizeof(float), hipMemcpyHostToDevice));
    // accumulators start at initial_data() even before init_weights (Vec allocation happens there in the
    // reference; a zero table with initial accumulators is the natural "new_without_weights" state here)
    const float a0 = initial_acc(cfg->optimizer, cfg->init_acc_gradient);
    if (a0 != 0.0f) FWGPU_HIP(launch_fill_lr(r->d_lr, r->lr_len, 0.0f, a0, 0));
    const float fa0 = initial_acc(cfg->optimizer, cfg->ffm_init_acc_gradient);
    if (r->ffm_len && fa0 != 0.0f && !r->packed()) FWGPU_HIP(launch_fill(r->d_ffm_acc, r->ffm_len, fa0, 0));
    FWGPU_HIP(hipDeviceSynchronize());
    *out = r.release();
    return FWGPU_OK;
}

int fwgpu_free(fwgpu_regressor *r) {
    if (!r) return FWGPU_OK;
    (void)hipSetDevice(r->device);
    if (r->one) fwgpu_batch_free(r->one);
    head_scratch_free(r);
    if (r->pred_x) (void)hipFree(r->pred_x);
    if (r->pred_yi) (void)hipFree(r->pred_yi);
    if (r->metrics_scratch) (void)hipFree(r->metrics_scratch);
    (void)hipFree(r->d_lr);
    (void)hipFree(r->d_ffm_w);
    (void)hipFree(r->d_ffm_acc);
    (void)hipFree(r->d_ffm_q);
    (void)hipFree(r->d_lut_lr);
    (void)hipFree(r->d_lut_ffm);
    (void)hipFree(r->d_nn_w);
    (void)hipFree(r->d_nn_acc);
    (void)hipFree(r->d_lut_nn);
    if (r->pinned) (void)hipHostFree(r->pinned);
    delete r;
    return FWGPU_OK;
}

static int nn_init_weights(fwgpu_regressor *r);

int fwgpu_init_weights(fwgpu_regressor *r) {
    if (!r) return fail(FWGPU_ERR_INVALID, "NULL regressor");
    if (int rcp = refuse_packed(r, "init_weights")) return rcp;
    FWGPU_HIP(hipSetDevice(r->device));
    const fwgpu_config &c = r->cfg;
    // block_lr.rs:97-105
    FWGPU_HIP(launch_fill_lr(r->d_lr, r->lr_len, 0.0f, initial_acc(c.optimizer, c.init_acc_gradient), 0));
    // block_ffm.rs:784-829
    if (r->ffm_len)
        FWGPU_HIP(launch_ffm_init(r->d_ffm_w, r->d_ffm_acc, r->ffm_len, c.ffm_k, c.ffm_init_width, c.ffm_init_zero_band,
                                  c.ffm_init_center, initial_acc(c.optimizer, c.ffm_init_acc_gradient), 0));
    if (r->nn.n_layers) {
        int rc = nn_init_weights(r);
        if (rc) return rc;
    }
    FWGPU_HIP(hipDeviceSynchronize());
    return FWGPU_OK;
}

int fwgpu_set_nn(fwgpu_regressor *r, const fwgpu_nn_config *nn) {
    if (!r || !nn) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if (int rcp = refuse_packed(r, "set_nn (the deep head)")) return rcp;
    if (r->cfg.wiring != FWGPU_WIRING_REGRESSOR) return fail(FWGPU_ERR_INVALID, "the deep head needs the REGRESSOR wiring");
    if (nn->n_layers == 0 || nn->n_layers > FWGPU_NN_MAX_LAYERS) return fail(FWGPU_ERR_INVALID, "nn: n_layers must be in 1..8");
    if (nn->topology != 1 && nn->topology != 2)
        return fail(FWGPU_ERR_INVALID, "unknown nn topology (\"one\" and \"two\" are supported; \"four\"/\"five\" use block_normalize, out of scope)");
    FWGPU_HIP(hipSetDevice(r->device));
    DevNN d{};
    const uint32_t F = r->cfg.ffm_k ? r->cfg.ffm_num_fields : 0;
    d.n_layers = nn->n_layers;
    d.topology = nn->topology;
    d.X = r->cfg.num_combos + F * (F + 1) / 2;  // the Join span (regressor.rs:185-189)
    uint32_t in = d.X, off = 0;
    d.max_in = d.X;
    for (uint32_t l = 0; l < nn->n_layers; l++) {
        if (nn->width[l] == 0 || nn->width[l] > 4096) return fail(FWGPU_ERR_INVALID, "nn: layer width must be in 1..4096");
        if (nn->init[l] > FWGPU_NN_INIT_ZERO) return fail(FWGPU_ERR_INVALID, "nn: unknown init type");
        if (in >= 16000) return fail(FWGPU_ERR_INVALID, "nn: too many inputs (MAX_NUM_INPUTS, block_neural.rs:27)");
        d.in[l] = in;
        d.out[l] = nn->width[l];
        d.off[l] = off;
        d.relu[l] = nn->relu[l] ? 1 : 0;
        off += (in + 1) * nn->width[l];  // +1: bias term (block_neural.rs:86)
        d.sum_width += nn->width[l];
        d.max_out = std::max(d.max_out, nn->width[l]);
        in = nn->width[l];
        d.max_in = std::max(d.max_in, in);
    }
    const uint32_t L = nn->n_layers;
    d.in[L] = in + (nn->topology == 1 ? d.X : 0);  // Join(h_last, copy of x), regressor.rs:307-311
    d.out[L] = 1;
    d.off[L] = off;
    off += d.in[L] + 1;
    d.max_in = std::max(d.max_in, d.in[L]);
    d.rate = nn->nn_learning_rate;
    d.minus_power_t = -nn->nn_power_t;
    if (r->d_nn_w) (void)hipFree(r->d_nn_w);
    if (r->d_nn_acc) (void)hipFree(r->d_nn_acc);
    if (r->d_lut_nn) (void)hipFree(r->d_lut_nn);
    r->nn_len = off;
    FWGPU_HIP(hipMalloc((void **)&r->d_nn_w, (size_t)off * 4));
    FWGPU_HIP(hipMalloc((void **)&r->d_nn_acc, (size_t)off * 4));
    FWGPU_HIP(hipMalloc((void **)&r->d_lut_nn, kLutSize * sizeof(float)));
    FWGPU_HIP(hipMemset(r->d_nn_w, 0, (size_t)off * 4));
    std::vector<float> lut(kLutSize);
    lut_init(lut.data(), nn->nn_learning_rate, nn->nn_power_t, nn->nn_init_acc_gradient);  // block_neural.rs:111-112
    FWGPU_HIP(hipMemcpy(r->d_lut_nn, lut.data(), kLutSize * sizeof(float), hipMemcpyHostToDevice));
    FWGPU_HIP(launch_fill(r->d_nn_acc, off, initial_acc(r->cfg.optimizer, nn->nn_init_acc_gradient), 0));
    FWGPU_HIP(hipDeviceSynchronize());
    d.w = r->d_nn_w;
    d.acc = r->d_nn_acc;
    d.lut = r->d_lut_nn;
    r->nn = d;
    r->nn_cfg = *nn;
    return FWGPU_OK;
}

// block_neural.rs:367-424.  The reference seeds Xoshiro256++ per layer and samples rand_distr Normal / Uniform;
// that stream is third-party and unpinned, so the library uses its own deterministic generator with the same
// distributions: Hu = N(0, sqrt(2/in)), Xavier = U(+-sqrt(6)/sqrt(in*out)), One, Zero; biases are always 0.
static int nn_init_weights(fwgpu_regressor *r) {
    const DevNN &d = r->nn;
    std::vector<float> w(r->nn_len, 0.0f);
    auto rng = [](uint64_t &s) {
        uint64_t z = (s += 0x9e3779b97f4a7c15ULL);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
        return z ^ (z >> 31);
    };
    auto u01 = [&](uint64_t &s) { return ((double)(rng(s) >> 11) + 0.5) * (1.0 / 9007199254740992.0); };
    for (uint32_t l = 0; l <= d.n_layers; l++) {
        const uint32_t in = d.in[l], out = d.out[l];
        const size_t bias = (size_t)in * out;
        const uint32_t init = l == d.n_layers ? (uint32_t)FWGPU_NN_INIT_ONE : r->nn_cfg.init[l];  // regressor.rs:312-319
        uint64_t st = 0x5eed0000ULL + 7919ULL * l + in + (bias + out);
        float *wl = w.data() + d.off[l];
        for (size_t i = 0; i < bias; i++) {
            switch (init) {
            case FWGPU_NN_INIT_XAVIER: wl[i] = (float)((2.0 * u01(st) - 1.0) * (sqrt(6.0) / sqrt((double)bias))); break;
            case FWGPU_NN_INIT_HU: {
                const double u1 = u01(st), u2 = u01(st);
                wl[i] = (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2) * sqrt(2.0 / (double)in));
                break;
            }
            case FWGPU_NN_INIT_ONE: wl[i] = 1.0f; break;
            default: wl[i] = 0.0f;
            }
        }
    }
    FWGPU_HIP(hipMemcpy(r->d_nn_w, w.data(), w.size() * 4, hipMemcpyHostToDevice));
    FWGPU_HIP(launch_fill(r->d_nn_acc, r->nn_len, initial_acc(r->cfg.optimizer, r->nn_cfg.nn_init_acc_gradient), 0));
    return FWGPU_OK;
}

int fwgpu_set_wiring(fwgpu_regressor *r, int wiring) {
    if (!r) return fail(FWGPU_ERR_INVALID, "NULL regressor");
    if (wiring != FWGPU_WIRING_REGRESSOR && wiring != FWGPU_WIRING_FFM_ONLY) return fail(FWGPU_ERR_INVALID, "unknown wiring");
    if (wiring != FWGPU_WIRING_REGRESSOR && r->nn.n_layers) return fail(FWGPU_ERR_INVALID, "the deep head needs the REGRESSOR wiring");
    if (wiring == FWGPU_WIRING_FFM_ONLY && !r->cfg.ffm_k) return fail(FWGPU_ERR_INVALID, "FFM_ONLY needs an FFM block");
    r->cfg.wiring = wiring;
    return FWGPU_OK;
}

int fwgpu_set_launch(fwgpu_regressor *r, uint32_t threads, uint32_t workgroups_per_cu) {
    if (!r) return fail(FWGPU_ERR_INVALID, "NULL regressor");
    if (threads) {
        if (threads % 64 || threads > 1024) return fail(FWGPU_ERR_INVALID, "threads must be a multiple of 64, <= 1024");
        r->launch.threads = threads;
        r->launch.threads_set = true;
    }
    r->launch.workgroups_per_cu = workgroups_per_cu;
    return FWGPU_OK;
}

int fwgpu_set_max_in_flight(fwgpu_regressor *r, uint32_t n_examples) {
    if (!r) return fail(FWGPU_ERR_INVALID, "NULL regressor");
    r->launch.max_in_flight = n_examples;
    return FWGPU_OK;
}

int fwgpu_debug_set_option(fwgpu_regressor *r, int option, int value) {
    if (!r) return fail(FWGPU_ERR_INVALID, "NULL regressor");
    switch (option) {
    case 1: r->launch.lut_global = value ? 1 : 0; return FWGPU_OK;
    case 3: r->launch.no_chain = value ? 1 : 0; return FWGPU_OK;  // duplicate-row chains off (A/B runs)
    case 4:  // hogwild launches: the constant feature's LR entry is stepped in LDS and reaches the table every `value` examples (0: off)
        if (value < 0 || value > 1024) return fail(FWGPU_ERR_INVALID, "hot LR entry option: 0 .. 1024 examples");
        r->launch.hot_lr_every = (uint32_t)value;
        return FWGPU_OK;
    case 5:  // FFM row store policy of hogwild launches: 0 write-through, 1 weights write-back, 2 both tables write-back, -1 the build's default
        if (value < -1 || value > 4) return fail(FWGPU_ERR_INVALID, "store policy option: -1, 0, 1, 2, 3 or 4");
        r->launch.store_policy = value;
        return FWGPU_OK;
    case 14:  // predict-only batches of a model with a deep head: 1 / -1 = the batched route where head_predict_batched allows it (default), 0 = the per-example forward for every launch
        if (value < -1 || value > 1) return fail(FWGPU_ERR_INVALID, "batched head predict option: -1, 0 or 1");
        r->launch.head_predict = value;
        return FWGPU_OK;
    case 13:  // rows kept from the gather in the large-table kernel: 0 = none (every row re-read by the update: no last-writer-wins over an example's lifetime), 1 / -1 = kept (default)
        if (value < -1 || value > 1) return fail(FWGPU_ERR_INVALID, "kept-rows option: -1, 0 or 1");
        r->launch.kept_rows = value;
        return FWGPU_OK;
    case 12:  // store policy 4 also on hot LR entries (weight stored alone, accumulator by thinned atomic adds): 0 / 1, -1 = default
        if (value < -1 || value > 1) return fail(FWGPU_ERR_INVALID, "LR thinning option: -1, 0 or 1");
        r->launch.lr_thin = value;
        return FWGPU_OK;
    case 11:  // the deep head of concurrent two-chunk launches as a phase of the v2 kernel (1, default where two workgroups fit a CU) or always on the generic kernel (0); -1 = default
        if (value < -1 || value > 2) return fail(FWGPU_ERR_INVALID, "deep-head kernel option: -1, 0, 1 or 2");
        r->launch.nn_v2 = value;
        return FWGPU_OK;
    case 9:  // policies 3 / 4: a row counts as hot when its accumulators have grown by more than value / 1024 (-1: the default, 0.5)
        if (value < -1 || value > (1 << 24)) return fail(FWGPU_ERR_INVALID, "hot-row threshold option: -1, or 0 .. 2^24 (in 1/1024)");
        r->launch.acc_hot_theta = value < 0 ? -1.0f : (float)value / 1024.0f;
        return FWGPU_OK;
    case 10:  // policies 3 / 4: one example in 2^value touches a hot row's accumulators (-1: the default, 3)
        if (value < -1 || value > 6) return fail(FWGPU_ERR_INVALID, "accumulator sampling option: -1, or 0 .. 6");
        r->launch.acc_sample_log2 = value;
        return FWGPU_OK;
    case 15:  // policy 4: hot rows beyond 8 / 16 / 32 x the threshold are sampled one step of the exponent further each (hot_tiers.h): 1 on, 0 = every hot row at option 10's exponent, -1 = default
        if (value < -1 || value > 1) return fail(FWGPU_ERR_INVALID, "hot-row tiers option: -1, 0 or 1");
        r->launch.acc_tiers = value;
        return FWGPU_OK;
    case 6:  // write-back interval of policies 1 / 2: a workgroup issues buffer_wbl2 every `value` of its examples (0 never, -1 the build's default)
        if (value < -1 || value > 65536) return fail(FWGPU_ERR_INVALID, "write-back interval option: -1 .. 65536 examples");
        r->launch.wb_flush_every = value;
        return FWGPU_OK;
    case 8:  // rows per wave kept in LDS beyond the register-kept ones (-1: automatic)
        if (value < -1 || value > 3) return fail(FWGPU_ERR_INVALID, "LDS-kept rows option: 0 .. 3, or -1 (automatic)");
        r->launch.lds_keep = value;
        return FWGPU_OK;
    case 7: r->launch.prefetch = value ? 1 : 0; return FWGPU_OK;  // next-record prefetch of the v2 kernel's updating launches
    case 2:  // whole-line FFM row updates: 0 off, 1 auto (tables larger than the Infinity Cache; default), 2 always, 3 chained path always with float-granular accesses
        if (value < 0 || value > 3) return fail(FWGPU_ERR_INVALID, "window option: 0, 1, 2 or 3");
        r->launch.window = value;
        return FWGPU_OK;
    }
    return fail(FWGPU_ERR_INVALID, "unknown debug option");
}

int fwgpu_debug_set_kernel_version(fwgpu_regressor *r, int version) {
    if (!r) return fail(FWGPU_ERR_INVALID, "NULL regressor");
    if (version < 0 || version > 2) return fail(FWGPU_ERR_INVALID, "kernel version must be 0 (auto), 1 or 2");
    r->launch.kernel_version = version;
    return FWGPU_OK;
}

// ------------------------------------------------------------------ tables

static int table_ptr(fwgpu_regressor *r, int which, float **p, uint64_t *n) {
    if (!r) return fail(FWGPU_ERR_INVALID, "NULL regressor");
    switch (which) {
    case FWGPU_TABLE_LR: *p = r->d_lr; *n = r->lr_len * 2; return FWGPU_OK;
    case FWGPU_TABLE_FFM_W: *p = r->d_ffm_w; *n = r->ffm_len; return FWGPU_OK;
    case FWGPU_TABLE_FFM_ACC: *p = r->d_ffm_acc; *n = r->ffm_len; return FWGPU_OK;
    case FWGPU_TABLE_NN_W: *p = r->d_nn_w; *n = r->nn_len; return FWGPU_OK;
    case FWGPU_TABLE_NN_ACC: *p = r->d_nn_acc; *n = r->nn_len; return FWGPU_OK;
    }
    return fail(FWGPU_ERR_INVALID, "unknown table");
}

int fwgpu_table_len(fwgpu_regressor *r, int which, uint64_t *n_floats) {
    float *p;
    uint64_t n;
    int rc = table_ptr(r, which, &p, &n);
    if (rc) return rc;
    *n_floats = n;
    return FWGPU_OK;
}

// packed regressor: the FFM tables are not f32 arrays (the weights are buckets, the accumulators do not exist)
static bool is_ffm_table(int which) { return which == FWGPU_TABLE_FFM_W || which == FWGPU_TABLE_FFM_ACC; }

int fwgpu_ffm_storage(fwgpu_regressor *r, int *storage, uint64_t *table_bytes) {
    if (!r || !storage || !table_bytes) return fail(FWGPU_ERR_INVALID, "NULL argument");
    *storage = r->packed() ? FWGPU_FFM_F16_BUCKETS : FWGPU_FFM_F32;
    *table_bytes = r->packed() ? r->ffm_q_bytes : (r->ffm_len ? (r->ffm_len + 64) * sizeof(float) : 0);
    return FWGPU_OK;
}

// a range of the packed weight table as the f32 values it stands for, through the device routine that shares the gather's conversion
static int packed_table_read(fwgpu_regressor *r, uint64_t offset, uint64_t count, float *host_out) {
    FWGPU_HIP(hipSetDevice(r->device));
    FWGPU_HIP(hipDeviceSynchronize());
    const uint64_t kChunk = 16ull << 20;
    float *d = nullptr;
    if (count == 0) return FWGPU_OK;
    if (hipMalloc((void **)&d, std::min(count, kChunk) * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FWGPU_ERR_OOM, "table_read: no memory for the expanded range");
    }
    hipError_t e = hipSuccess;
    for (uint64_t at = 0; at < count && e == hipSuccess; at += kChunk) {
        const uint64_t n = std::min(kChunk, count - at);
        e = launch_packed_expand(r->d_ffm_q + offset + at, d, n, r->q_increment, r->q_min, 0);
        if (e == hipSuccess) e = hipMemcpy(host_out + at, d, n * sizeof(float), hipMemcpyDeviceToHost);
    }
    (void)hipFree(d);
    if (e != hipSuccess) return fail(FWGPU_ERR_DEVICE, std::string("table_read (packed): ") + hipGetErrorString(e));
    return FWGPU_OK;
}

int fwgpu_table_device_ptr(fwgpu_regressor *r, int which, void **dev_ptr) {
    float *p;
    uint64_t n;
    int rc = table_ptr(r, which, &p, &n);
    if (rc) return rc;
    if (is_ffm_table(which) && (rc = refuse_packed(r, "table_device_ptr of an FFM table"))) return rc;
    if (!dev_ptr) return fail(FWGPU_ERR_INVALID, "NULL argument");
    *dev_ptr = p;
    return FWGPU_OK;
}

int fwgpu_table_read(fwgpu_regressor *r, int which, uint64_t offset, uint64_t count, float *host_out) {
    float *p;
    uint64_t n;
    int rc = table_ptr(r, which, &p, &n);
    if (rc) return rc;
    if (offset > n || count > n - offset) return fail(FWGPU_ERR_RANGE, "table_read out of range");
    if (which == FWGPU_TABLE_FFM_ACC && (rc = refuse_packed(r, "table_read of the FFM accumulators"))) return rc;
    if (which == FWGPU_TABLE_FFM_W && r->packed()) return count && !host_out ? fail(FWGPU_ERR_INVALID, "NULL argument") : packed_table_read(r, offset, count, host_out);
    FWGPU_HIP(hipSetDevice(r->device));
    FWGPU_HIP(hipDeviceSynchronize());
    if (count) FWGPU_HIP(hipMemcpy(host_out, p + offset, count * sizeof(float), hipMemcpyDeviceToHost));
    return FWGPU_OK;
}

int fwgpu_table_write(fwgpu_regressor *r, int which, uint64_t offset, uint64_t count, const float *host_in) {
    float *p;
    uint64_t n;
    int rc = table_ptr(r, which, &p, &n);
    if (rc) return rc;
    if (offset > n || count > n - offset) return fail(FWGPU_ERR_RANGE, "table_write out of range");
    if (is_ffm_table(which) && (rc = refuse_packed(r, "table_write of an FFM table"))) return rc;
    FWGPU_HIP(hipSetDevice(r->device));
    FWGPU_HIP(hipDeviceSynchronize());
    if (count) FWGPU_HIP(hipMemcpy(p + offset, host_in, count * sizeof(float), hipMemcpyHostToDevice));
    return FWGPU_OK;
}

int fwgpu_table_fill(fwgpu_regressor *r, int which, float value) {
    float *p;
    uint64_t n;
    int rc = table_ptr(r, which, &p, &n);
    if (rc) return rc;
    if (is_ffm_table(which) && (rc = refuse_packed(r, "table_fill of an FFM table"))) return rc;
    FWGPU_HIP(hipSetDevice(r->device));
    FWGPU_HIP(launch_fill(p, n, value, 0));
    FWGPU_HIP(hipDeviceSynchronize());
    return FWGPU_OK;
}

int fwgpu_table_checksum(fwgpu_regressor *r, int which, uint64_t *checksum) {
    float *p;
    uint64_t n;
    int rc = table_ptr(r, which, &p, &n);
    if (rc) return rc;
    if (which == FWGPU_TABLE_FFM_ACC && (rc = refuse_packed(r, "table_checksum of the FFM accumulators"))) return rc;
    FWGPU_HIP(hipSetDevice(r->device));
    float *expanded = nullptr;  // packed weights: the checksum of the f32 values they stand for
    if (which == FWGPU_TABLE_FFM_W && r->packed()) {
        if (hipMalloc((void **)&expanded, n * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(FWGPU_ERR_OOM, "table_checksum: no memory for the expanded table");
        }
        hipError_t ee = launch_packed_expand(r->d_ffm_q, expanded, n, r->q_increment, r->q_min, 0);
        if (ee != hipSuccess) {
            (void)hipFree(expanded);
            return fail(FWGPU_ERR_DEVICE, std::string("checksum: ") + hipGetErrorString(ee));
        }
        p = expanded;
    }
    unsigned long long *d = nullptr;
    hipError_t e = hipMalloc((void **)&d, sizeof(unsigned long long));
    if (e == hipSuccess) e = launch_checksum(p, n, d, 0);
    unsigned long long h = 0;
    if (e == hipSuccess) e = hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    (void)hipFree(expanded);
    if (e != hipSuccess) return fail(FWGPU_ERR_DEVICE, std::string("checksum: ") + hipGetErrorString(e));
    *checksum = h;
    return FWGPU_OK;
}

int fwgpu_delta_start(const void *table, const void *snapshot, void *local_delta, void *summed_delta, uint64_t n_floats,
                      float scale, void *stream) {
    if (!table || !snapshot || !local_delta || !summed_delta) return fail(FWGPU_ERR_INVALID, "NULL argument");
    FWGPU_HIP(launch_delta_start(static_cast<const float *>(table), static_cast<const float *>(snapshot),
                                 static_cast<float *>(local_delta), static_cast<float *>(summed_delta), n_floats, scale,
                                 static_cast<hipStream_t>(stream)));
    return FWGPU_OK;
}

int fwgpu_delta_finish(void *table, void *snapshot, const void *local_delta, const void *summed_delta, uint64_t n_floats,
                       void *stream) {
    if (!table || !snapshot || !local_delta || !summed_delta) return fail(FWGPU_ERR_INVALID, "NULL argument");
    FWGPU_HIP(launch_delta_finish(static_cast<float *>(table), static_cast<float *>(snapshot),
                                  static_cast<const float *>(local_delta), static_cast<const float *>(summed_delta),
                                  n_floats, static_cast<hipStream_t>(stream)));
    return FWGPU_OK;
}

int fwgpu_debug_placement(const fwgpu_regressor *r, int *tries, float *ms_fastest, float *ms_slowest) {
    if (!r) return fail(FWGPU_ERR_INVALID, "NULL regressor");
    if (tries) *tries = r->placement_tries;
    if (ms_fastest) *ms_fastest = r->placement_ms_lo;
    if (ms_slowest) *ms_slowest = r->placement_ms_hi;
    return FWGPU_OK;
}

int fwgpu_debug_phase_ticks(fwgpu_regressor *r, int enable, uint64_t *out16) {
    if (!r) return fail(FWGPU_ERR_INVALID, "NULL regressor");
    FWGPU_HIP(hipSetDevice(r->device));
    FWGPU_HIP(hipDeviceSynchronize());
    if (out16) {
        if (r->d_ticks)
            FWGPU_HIP(hipMemcpy(out16, r->d_ticks, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
        else
            memset(out16, 0, 16 * sizeof(uint64_t));
    }
    if (enable) {
        if (!r->d_ticks) FWGPU_HIP(hipMalloc((void **)&r->d_ticks, 16 * sizeof(uint64_t)));
        FWGPU_HIP(hipMemset(r->d_ticks, 0, 16 * sizeof(uint64_t)));
    } else if (r->d_ticks) {
        (void)hipFree(r->d_ticks);
        r->d_ticks = nullptr;
    }
    return FWGPU_OK;
}

int fwgpu_debug_coherence_probe(int device, int use_sc1, uint32_t iters, uint32_t *stale_words, uint32_t *timeouts) {
    if (!stale_words || !timeouts) return fail(FWGPU_ERR_INVALID, "NULL argument");
    FWGPU_HIP(hipSetDevice(device));
    unsigned *d = nullptr;
    FWGPU_HIP(hipMalloc((void **)&d, 512 * sizeof(unsigned)));
    hipError_t e = hipMemset(d, 0, 512 * sizeof(unsigned));
    if (e == hipSuccess) e = launch_coherence_probe(d, use_sc1, iters, 16, 0);
    unsigned out[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpy(out, d + 400, sizeof(out), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(FWGPU_ERR_DEVICE, std::string("coherence probe: ") + hipGetErrorString(e));
    *stale_words = out[0];
    *timeouts = out[1];
    return FWGPU_OK;
}

// ------------------------------------------------------------------ weight blob (regressor.rs:426-469)

static uint64_t serialized_elems(const fwgpu_regressor *r) {
    // sum of get_serialized_len(): block_lr.rs:253-255 (weights_len), block_ffm.rs:831-833 (ffm_weights_len)
    return r->lr_len + r->ffm_len + r->nn_len;  // + block_neural.rs:426-428 (weights_len of every dense layer)
}

int fwgpu_serialized_len(fwgpu_regressor *r, uint64_t *n_bytes) {
    if (!r || !n_bytes) return fail(FWGPU_ERR_INVALID, "NULL argument");
    const bool sgd = r->cfg.optimizer == FWGPU_OPT_SGD;
    // SGD's PerWeightStore is PhantomData (0 bytes): optimizer.rs:20
    *n_bytes = 8 + r->lr_len * (sgd ? 4 : 8) + r->ffm_len * (sgd ? 4 : 8) + r->nn_len * (sgd ? 4 : 8);
    return FWGPU_OK;
}

int fwgpu_write_weights(fwgpu_regressor *r, uint8_t *buf, uint64_t cap, uint64_t *written) {
    uint64_t need = 0;
    int rc = fwgpu_serialized_len(r, &need);
    if (rc) return rc;
    if ((rc = refuse_packed(r, "write_weights / model_save"))) return rc;
    if (!buf || cap < need) return fail(FWGPU_ERR_RANGE, "write_weights: buffer too small");
    FWGPU_HIP(hipSetDevice(r->device));
    FWGPU_HIP(hipDeviceSynchronize());
    const bool sgd = r->cfg.optimizer == FWGPU_OPT_SGD;
    const uint64_t total = serialized_elems(r);
    memcpy(buf, &total, 8);  // little-endian host
    uint8_t *o = buf + 8;
    if (!sgd) {
        FWGPU_HIP(hipMemcpy(o, r->d_lr, r->lr_len * 8, hipMemcpyDeviceToHost));
        o += r->lr_len * 8;
    } else {
        std::vector<float> tmp(r->lr_len * 2);
        FWGPU_HIP(hipMemcpy(tmp.data(), r->d_lr, r->lr_len * 8, hipMemcpyDeviceToHost));
        float *dst = reinterpret_cast<float *>(o);
        for (uint64_t i = 0; i < r->lr_len; i++) dst[i] = tmp[2 * i];
        o += r->lr_len * 4;
    }
    if (r->ffm_len) {
        FWGPU_HIP(hipMemcpy(o, r->d_ffm_w, r->ffm_len * 4, hipMemcpyDeviceToHost));
        o += r->ffm_len * 4;
        if (!sgd) {
            FWGPU_HIP(hipMemcpy(o, r->d_ffm_acc, r->ffm_len * 4, hipMemcpyDeviceToHost));
            o += r->ffm_len * 4;
        }
    }
    // dense layers in block order, each: weights then optimizer state (block_neural.rs:430-438)
    for (uint32_t l = 0; r->nn.n_layers && l <= r->nn.n_layers; l++) {
        const size_t len = ((size_t)r->nn.in[l] + 1) * r->nn.out[l];
        FWGPU_HIP(hipMemcpy(o, r->d_nn_w + r->nn.off[l], len * 4, hipMemcpyDeviceToHost));
        o += len * 4;
        if (!sgd) {
            FWGPU_HIP(hipMemcpy(o, r->d_nn_acc + r->nn.off[l], len * 4, hipMemcpyDeviceToHost));
            o += len * 4;
        }
    }
    if (written) *written = (uint64_t)(o - buf);
    return FWGPU_OK;
}

int fwgpu_read_weights(fwgpu_regressor *r, const uint8_t *buf, uint64_t len) {
    uint64_t need = 0;
    int rc = fwgpu_serialized_len(r, &need);
    if (rc) return rc;
    if ((rc = refuse_packed(r, "read_weights / hogwild_load"))) return rc;
    if (!buf || len < need) return fail(FWGPU_ERR_FORMAT, "read_weights: blob shorter than the model");
    uint64_t total = 0;
    memcpy(&total, buf, 8);
    // regressor.rs:452-457: "Lenghts of weights array in regressor file differ"
    if (total != serialized_elems(r)) return fail(FWGPU_ERR_FORMAT, "read_weights: weight count differs from the model's");
    FWGPU_HIP(hipSetDevice(r->device));
    FWGPU_HIP(hipDeviceSynchronize());
    const bool sgd = r->cfg.optimizer == FWGPU_OPT_SGD;
    const uint8_t *o = buf + 8;
    if (!sgd) {
        FWGPU_HIP(hipMemcpy(r->d_lr, o, r->lr_len * 8, hipMemcpyHostToDevice));
        o += r->lr_len * 8;
    } else {
        std::vector<float> tmp(r->lr_len * 2, 0.0f);
        const float *src = reinterpret_cast<const float *>(o);
        for (uint64_t i = 0; i < r->lr_len; i++) tmp[2 * i] = src[i];
        FWGPU_HIP(hipMemcpy(r->d_lr, tmp.data(), r->lr_len * 8, hipMemcpyHostToDevice));
        o += r->lr_len * 4;
    }
    if (r->ffm_len) {
        FWGPU_HIP(hipMemcpy(r->d_ffm_w, o, r->ffm_len * 4, hipMemcpyHostToDevice));
        o += r->ffm_len * 4;
        if (!sgd) {
            FWGPU_HIP(hipMemcpy(r->d_ffm_acc, o, r->ffm_len * 4, hipMemcpyHostToDevice));
            o += r->ffm_len * 4;
        }
    }
    for (uint32_t l = 0; r->nn.n_layers && l <= r->nn.n_layers; l++) {  // block_neural.rs:440-448
        const size_t len = ((size_t)r->nn.in[l] + 1) * r->nn.out[l];
        FWGPU_HIP(hipMemcpy(r->d_nn_w + r->nn.off[l], o, len * 4, hipMemcpyHostToDevice));
        o += len * 4;
        if (!sgd) {
            FWGPU_HIP(hipMemcpy(r->d_nn_acc + r->nn.off[l], o, len * 4, hipMemcpyHostToDevice));
            o += len * 4;
        }
    }
    return FWGPU_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ quantising on the device (quantize.hip): inference save, pack, refresh
namespace fwgpu {

bool quantize_host_forced() {
    const char *env = getenv("FWGPU_QUANTIZE_HOST");  // A/B runs (scripts/bench_publish.py); read at every call: publishing is no hot path
    return env && atoi(env) != 0;
}

int quantize_on_device(int device, const float *d_w, uint64_t n, uint16_t *d_q, float *increment, float *mn, bool *done) {
    *done = false;
    if (quantize_host_forced() || !n) return FWGPU_OK;
    FWGPU_HIP(hipSetDevice(device));
    uint32_t *ws = nullptr;
    FWGPU_HIP(hipMalloc((void **)&ws, kQuantWsWords * sizeof(uint32_t)));
    uint32_t st[3] = {0, 0, 1};
    hipError_t e = launch_quant_stats(d_w, n, ws, 0);
    if (e == hipSuccess) e = hipMemcpy(st, ws, sizeof st, hipMemcpyDeviceToHost);
    (void)hipFree(ws);
    if (e != hipSuccess) return fail(FWGPU_ERR_DEVICE, std::string("quantize (statistics): ") + hipGetErrorString(e));
    float lo, hi;
    memcpy(&lo, &st[0], 4);
    memcpy(&hi, &st[1], 4);
    quantize_header(lo, hi, increment, mn);
    if (st[2] || *increment == 0.0f || !isfinite(*increment)) return FWGPU_OK;  // the host route's cases (quantize.hip)
    FWGPU_HIP(launch_quant_buckets(d_w, n, *increment, *mn, d_q, 0));
    FWGPU_HIP(hipDeviceSynchronize());
    *done = true;
    return FWGPU_OK;
}

// the host route: the table crosses to the host and quantize_ffm runs there
static int ffm_block_on_host(fwgpu_regressor *r, std::vector<uint8_t> &out) {
    std::vector<float> w(r->ffm_len);
    int rc = fwgpu_table_read(r, FWGPU_TABLE_FFM_W, 0, r->ffm_len, w.data());
    if (rc) return rc;
    quantize_ffm(w.data(), r->ffm_len, out);
    return FWGPU_OK;
}

int ffm_quantized_block(fwgpu_regressor *r, std::vector<uint8_t> &out, bool *on_device) {
    if (on_device) *on_device = false;
    int rc = refuse_packed(r, "quantize_ffm_table");
    if (rc) return rc;
    if (!r->ffm_len) return fail(FWGPU_ERR_INVALID, "quantize_ffm_table: the model has no FFM block");
    FWGPU_HIP(hipSetDevice(r->device));
    FWGPU_HIP(hipDeviceSynchronize());
    if (quantize_host_forced()) return ffm_block_on_host(r, out);
    uint16_t *d_q = nullptr;
    if (hipMalloc((void **)&d_q, r->ffm_len * 2) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FWGPU_ERR_OOM, "quantize_ffm_table: no device memory for the bucket table");
    }
    float inc = 0, mn = 0;
    bool done = false;
    rc = quantize_on_device(r->device, r->d_ffm_w, r->ffm_len, d_q, &inc, &mn, &done);
    if (!rc && done) {
        out.resize(8 + 2 * r->ffm_len);
        memcpy(out.data(), &inc, 4);
        memcpy(out.data() + 4, &mn, 4);
        if (hipMemcpy(out.data() + 8, d_q, r->ffm_len * 2, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(FWGPU_ERR_DEVICE, "quantize_ffm_table: bucket download failed");
    }
    (void)hipFree(d_q);
    if (rc) return rc;
    if (!done) return ffm_block_on_host(r, out);
    if (on_device) *on_device = true;
    return FWGPU_OK;
}

int lr_weights_read(fwgpu_regressor *r, float *host_out) {
    FWGPU_HIP(hipSetDevice(r->device));
    FWGPU_HIP(hipDeviceSynchronize());
    if (quantize_host_forced()) {  // the pairs cross, the host drops the accumulators (what fwgpu_write_weights + to_weights_only do)
        std::vector<float> tmp(r->lr_len * 2);
        FWGPU_HIP(hipMemcpy(tmp.data(), r->d_lr, r->lr_len * 8, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < r->lr_len; i++) host_out[i] = tmp[2 * i];
        return FWGPU_OK;
    }
    float *d = nullptr;
    if (hipMalloc((void **)&d, r->lr_len * 4) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FWGPU_ERR_OOM, "no device memory for the compacted LR weights");
    }
    hipError_t e = launch_lr_weights(r->d_lr, r->lr_len, d, 0);
    if (e == hipSuccess) e = hipMemcpy(host_out, d, r->lr_len * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(FWGPU_ERR_DEVICE, std::string("LR weights: ") + hipGetErrorString(e));
    return FWGPU_OK;
}

int nn_weights_read(fwgpu_regressor *r, std::vector<float> &out) {
    out.clear();
    FWGPU_HIP(hipSetDevice(r->device));
    FWGPU_HIP(hipDeviceSynchronize());
    for (uint32_t l = 0; r->nn.n_layers && l <= r->nn.n_layers; l++) {  // block order, as fwgpu_write_weights walks them
        const size_t len = ((size_t)r->nn.in[l] + 1) * r->nn.out[l], at = out.size();
        out.resize(at + len);
        FWGPU_HIP(hipMemcpy(out.data() + at, r->d_nn_w + r->nn.off[l], len * 4, hipMemcpyDeviceToHost));
    }
    return FWGPU_OK;
}

}  // namespace fwgpu

extern "C" {

int fwgpu_quantize_ffm_table(fwgpu_regressor *r, uint8_t *out, uint64_t cap, uint64_t *written) {
    if (!r || !out) return fail(FWGPU_ERR_INVALID, "NULL argument");
    int rc = refuse_packed(r, "quantize_ffm_table");
    if (rc) return rc;
    if (!r->ffm_len) return fail(FWGPU_ERR_INVALID, "quantize_ffm_table: the model has no FFM block");
    if (cap < 8 + 2 * r->ffm_len) return fail(FWGPU_ERR_RANGE, "quantize_ffm_table: buffer too small");
    std::vector<uint8_t> q;
    rc = ffm_quantized_block(r, q);
    if (rc) return rc;
    memcpy(out, q.data(), q.size());
    if (written) *written = q.size();
    return FWGPU_OK;
}

int fwgpu_pack_regressor(fwgpu_regressor *src, fwgpu_regressor **out) {
    if (!src || !out) return fail(FWGPU_ERR_INVALID, "NULL argument");
    int rc = refuse_packed(src, "pack_regressor (the source)");
    if (rc) return rc;
    // the refusals of fwgpu_model_load_packed, in its words
    if (src->nn.n_layers) return fail(FWGPU_ERR_INVALID, "model_load_packed: models with a deep head are not served from packed weights");
    if (!src->ffm_len) return fail(FWGPU_ERR_INVALID, "model_load_packed: the model has no FFM block, there is nothing to pack");
    if (!packed_shape_ok(src->cfg.ffm_k, src->cfg.ffm_num_fields))
        return fail(FWGPU_ERR_INVALID, "packed regressor: ffm_k must be a multiple of 4 and a row (ffm_k x fields) at most 256 weights, or at most 512 with ffm_k dividing 256; got ffm_k = " +
                                           std::to_string(src->cfg.ffm_k) + ", fields = " + std::to_string(src->cfg.ffm_num_fields));
    fwgpu_regressor *dst = *out;
    if (dst) {
        const fwgpu_config &a = src->cfg, &b = dst->cfg;
        if (!dst->packed() || dst->device != src->device || dst->lr_len != src->lr_len || dst->ffm_len != src->ffm_len || a.ffm_k != b.ffm_k ||
            a.ffm_num_fields != b.ffm_num_fields || a.bit_precision != b.bit_precision || a.ffm_bit_precision != b.ffm_bit_precision ||
            a.num_combos != b.num_combos)
            return fail(FWGPU_ERR_INVALID, "pack_regressor: the target is not a packed regressor of the source's geometry on the source's device");
    }
    FWGPU_HIP(hipSetDevice(src->device));
    FWGPU_HIP(hipDeviceSynchronize());
    std::vector<uint8_t> host_block;
    const bool own = dst == nullptr;
    if (own) {
        fwgpu_config cfg = src->cfg;
        cfg.optimizer = FWGPU_OPT_SGD;           // persistence.rs:164 (immutable)
        cfg.wiring = FWGPU_WIRING_REGRESSOR;     // (a model file carries no wiring)
        rc = create_impl(&cfg, true, nullptr, &dst);
        if (rc) return rc;
    }
    float inc = 0, mn = 0;
    bool done = false;
    // table to table on the device; a table the contract sends to the host route (quantize.hip) leaves the target's buckets unwritten until the host's block is there
    rc = quantize_on_device(src->device, src->d_ffm_w, src->ffm_len, dst->d_ffm_q, &inc, &mn, &done);
    if (!rc && !done) rc = ffm_block_on_host(src, host_block);
    hipError_t e = hipSuccess;
    if (!rc) {
        if (!done) {
            memcpy(&inc, host_block.data(), 4);
            memcpy(&mn, host_block.data() + 4, 4);
            e = hipMemcpy(dst->d_ffm_q, host_block.data() + 8, src->ffm_len * 2, hipMemcpyHostToDevice);
        }
        if (e == hipSuccess) e = launch_lr_weights_pairs(src->d_lr, src->lr_len, dst->d_lr, 0);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) rc = fail(FWGPU_ERR_DEVICE, std::string("pack_regressor: ") + hipGetErrorString(e));
    }
    if (rc) {
        if (own) fwgpu_free(dst);
        return rc;
    }
    dst->q_increment = inc;
    dst->q_min = mn;
    if (!own) dst->weights_epoch++;  // (refreshed in place: the caches set up before hold sums of weights that no longer exist)
    *out = dst;
    return FWGPU_OK;
}

int fwgpu_debug_quantize(int device, const float *weights, uint64_t n, uint8_t *out, uint64_t cap, int *on_device) {
    if (!weights || !out || n == 0) return fail(FWGPU_ERR_INVALID, "NULL / empty argument");
    if (cap < 8 + 2 * n) return fail(FWGPU_ERR_RANGE, "buffer too small");
    if (on_device) *on_device = 0;
    FWGPU_HIP(hipSetDevice(device));
    float *d_w = nullptr;
    uint16_t *d_q = nullptr;
    hipError_t e = hipMalloc((void **)&d_w, n * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&d_q, n * 2);
    if (e == hipSuccess) e = hipMemcpy(d_w, weights, n * 4, hipMemcpyHostToDevice);
    float inc = 0, mn = 0;
    bool done = false;
    int rc = e == hipSuccess ? quantize_on_device(device, d_w, n, d_q, &inc, &mn, &done) : fail(FWGPU_ERR_DEVICE, std::string("debug_quantize: ") + hipGetErrorString(e));
    if (!rc && done) {
        memcpy(out, &inc, 4);
        memcpy(out + 4, &mn, 4);
        if (hipMemcpy(out + 8, d_q, n * 2, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(FWGPU_ERR_DEVICE, "debug_quantize: bucket download failed");
    }
    (void)hipFree(d_w);
    (void)hipFree(d_q);
    if (rc) return rc;
    if (!done) return fwgpu_quantize_ffm_weights(weights, n, out, cap);  // the host route, as every caller of quantize_on_device takes it
    if (on_device) *on_device = 1;
    return FWGPU_OK;
}

int fwgpu_debug_quantize_rates(fwgpu_regressor *r, float *ms3) {
    if (!r || !ms3) return fail(FWGPU_ERR_INVALID, "NULL argument");
    int rc = refuse_packed(r, "debug_quantize_rates");
    if (rc) return rc;
    if (!r->ffm_len) return fail(FWGPU_ERR_INVALID, "debug_quantize_rates: the model has no FFM block");
    FWGPU_HIP(hipSetDevice(r->device));
    FWGPU_HIP(hipDeviceSynchronize());
    const uint64_t n = r->ffm_len;
    void *scratch = nullptr;  // the copy's destination; its first half takes the buckets
    uint32_t *ws = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipMalloc(&scratch, n * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&ws, kQuantWsWords * sizeof(uint32_t));
    for (int i = 0; i < 5 && e == hipSuccess; i++) e = hipEventCreate(&ev[i]);
    float w[2] = {0, 0}, inc = 0, mn = 0;
    if (e == hipSuccess) e = hipEventRecord(ev[0], 0);
    if (e == hipSuccess) e = launch_quant_stats(r->d_ffm_w, n, ws, 0);
    if (e == hipSuccess) e = hipEventRecord(ev[1], 0);
    if (e == hipSuccess) e = hipMemcpy(w, ws, sizeof w, hipMemcpyDeviceToHost);
    quantize_header(w[0], w[1], &inc, &mn);
    if (e == hipSuccess && (inc == 0.0f || !isfinite(inc))) inc = 1.0f;  // (a table of the host route: the kernel's time does not depend on the values)
    if (e == hipSuccess) e = hipEventRecord(ev[2], 0);  // (the device was idle while the host formed the header)
    if (e == hipSuccess) e = launch_quant_buckets(r->d_ffm_w, n, inc, mn, static_cast<uint16_t *>(scratch), 0);
    if (e == hipSuccess) e = hipEventRecord(ev[3], 0);
    if (e == hipSuccess) e = hipMemcpyAsync(scratch, r->d_ffm_w, n * 4, hipMemcpyDeviceToDevice, 0);
    if (e == hipSuccess) e = hipEventRecord(ev[4], 0);
    if (e == hipSuccess) e = hipEventSynchronize(ev[4]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms3[0], ev[0], ev[1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms3[1], ev[2], ev[3]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms3[2], ev[3], ev[4]);
    for (int i = 0; i < 5; i++)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    (void)hipFree(scratch);
    (void)hipFree(ws);
    if (e != hipSuccess) return fail(FWGPU_ERR_DEVICE, std::string("debug_quantize_rates: ") + hipGetErrorString(e));
    return FWGPU_OK;
}

}  // extern "C"
