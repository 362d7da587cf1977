// Progressive and hold-out loss scored on the device (include/fwgpu.h "progressive and hold-out loss"): the example loop of the reference has a
// prediction for every example before it learns it (main.rs:246) and benchmark/calc_loss.py turns the written predictions into a log loss; here the
// predictions a launch left in its batch are scored against the batch's own labels by one kernel, so neither crosses to the host.
//
// One thread per example.  A wave reduces the examples that share a (window, side) key -- runs of consecutive lanes, found by ballot -- with
// butterfly shuffles and its leader lane then adds the run's sums to the window's row: one atomic add per wave, touched row and field.  The running
// totals and the prediction histograms of a workgroup gather in LDS first and reach memory once per workgroup -- and so does the row of a workgroup
// whose examples all share one key (the common case: windows of thousands, a launch of one kind), whose sums ARE the workgroup's share of a total:
// the adds of a launch into one 64-byte row, which the L2 serialises, are then eight per workgroup instead of eight per wave.  Counts are integer atomics (exact);
// the f64 sums are hardware f64 atomic adds on device memory, so their last bits depend on the order of arrival.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "fwgpu_internal.h"

namespace fwgpu {

static constexpr int kMetricsThreads = 1024;
static constexpr int kSumFields = 5;    // the doubles of fwgpu_metric_sums, behind its three counts
static constexpr int kCountFields = 3;
static_assert(sizeof(fwgpu_metric_sums) == 64, "fwgpu_metric_sums: three counts and five sums, 64 bytes");
static_assert(sizeof(fwgpu_metric_window) == 136 && sizeof(fwgpu_metric_total) == 64 + 512 * 8, "metrics structs are packed");
static constexpr size_t kTotalsBytes = 2 * sizeof(fwgpu_metric_sums) + 2 * 512 * sizeof(uint64_t);

__device__ __forceinline__ double wave_sum(double v) {  // every lane gets the sum of all 64
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ void add_sums(fwgpu_metric_sums *row, const unsigned long long (&c)[kCountFields], const double (&s)[kSumFields]) {
    unsigned long long *rc = reinterpret_cast<unsigned long long *>(row);
    double *rs = reinterpret_cast<double *>(row) + kCountFields;
#pragma unroll
    for (int f = 0; f < kCountFields; f++)
        if (c[f]) atomicAdd(rc + f, c[f]);
    if (c[0]) {  // (no scored example: every sum of the run is zero)
#pragma unroll
        for (int f = 0; f < kSumFields; f++) unsafeAtomicAdd(rs + f, s[f]);
    }
}

__global__ __launch_bounds__(kMetricsThreads) void metrics_kernel(MetricsLaunch a) {
    __shared__ unsigned int s_hist[2 * 512];
    __shared__ double s_sum[2 * kSumFields];
    __shared__ unsigned int s_cnt[2 * kCountFields];
    __shared__ unsigned long long s_key0;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int j = tid; j < 2 * 512; j += kMetricsThreads) s_hist[j] = 0;
    if (tid < 2 * kSumFields) s_sum[tid] = 0.0;
    if (tid < 2 * kCountFields) s_cnt[tid] = 0;

    const uint64_t i = (uint64_t)blockIdx.x * kMetricsThreads + tid;
    const bool in = i < a.n;
    // kind 0: scored, 1: unlabelled, 2: bad prediction
    int kind = 0, side = 0, hbin = -1;
    uint64_t w = 0;
    double v[kSumFields] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (in) {
        const float pred = a.pred[i];
        float label, imp;
        if (a.records) {
            const uint32_t *rec = a.records + a.rec_off[i];
            label = (float)rec[1];            // feature_buffer.rs:187
            imp = __uint_as_float(rec[2]);    // feature_buffer.rs:188-189
        } else {
            label = a.label[i];
            imp = a.importance[i];
        }
        side = (a.learned ? a.learned[i] != 0 : a.learned_all != 0) ? 0 : 1;
        if (a.window) w = (a.first_number + i - 1) / a.window;
        if (label == (float)kMetricsNoLabel) {
            kind = 1;
        } else if (!isfinite(pred)) {
            kind = 2;
        } else {
            double p = (double)pred;
            p = p < 1e-15 ? 1e-15 : (p > 1.0 - 1e-15 ? 1.0 - 1e-15 : p);  // calc_loss.py: np.clip(p, 1e-15, 1 - 1e-15)
            const double loss = label == 1.0f ? -log(p) : -log(1.0 - p);
            v[0] = (double)imp;
            v[1] = (double)imp * loss;
            v[2] = loss;
            v[3] = (double)pred;
            v[4] = (double)label;
            const float t = pred * 256.0f;  // (exact: a power of two)
            const int bin = t >= 255.0f ? 255 : (t > 0.0f ? (int)t : 0);
            hbin = side * 512 + (label == 1.0f ? 256 : 0) + bin;
        }
    }
    const uint64_t key = w * 2 + (uint64_t)side;
    if (tid == 0) s_key0 = key;  // (thread 0 of a workgroup always has an example)
    __syncthreads();
    const unsigned long long key0 = s_key0;
    const bool uniform = __syncthreads_and(!in || key == key0) != 0;  // one key in the whole workgroup: its row is added once, below
    if (hbin >= 0) atomicAdd(&s_hist[hbin], 1u);
    unsigned long long todo = __ballot(in);
    while (todo) {  // (wave-uniform: one turn per (window, side) the wave's examples fall into)
        const int leader = __ffsll((long long)todo) - 1;
        const uint64_t lk = __shfl(key, leader, 64);
        const bool mine = in && key == lk;
        const unsigned long long m = __ballot(mine);
        todo &= ~m;
        unsigned long long c[kCountFields];
        c[0] = __popcll(__ballot(mine && kind == 0));
        c[1] = __popcll(__ballot(mine && kind == 1));
        c[2] = __popcll(__ballot(mine && kind == 2));
        double s[kSumFields];
        const bool alone = __popcll(m) == 1;  // (window 1: the leader's own values are the run)
#pragma unroll
        for (int f = 0; f < kSumFields; f++) {
            s[f] = mine ? v[f] : 0.0;
            if (!alone && c[0]) s[f] = wave_sum(s[f]);
        }
        if (lane == leader) {
            const uint64_t lw = lk >> 1;
            const int ls = (int)(lk & 1);
            if (!uniform && a.rows && lw < a.n_windows) add_sums(a.rows + lk, c, s);
#pragma unroll
            for (int f = 0; f < kCountFields; f++)
                if (c[f]) atomicAdd(&s_cnt[ls * kCountFields + f], (unsigned int)c[f]);
            if (c[0]) {
#pragma unroll
                for (int f = 0; f < kSumFields; f++) atomicAdd(&s_sum[ls * kSumFields + f], s[f]);
            }
        }
    }
    __syncthreads();
    // the workgroup's share of the running totals and histograms, once
    if (a.hist) {
        for (int j = tid; j < 2 * 512; j += kMetricsThreads)
            if (s_hist[j]) atomicAdd(a.hist + j, (unsigned long long)s_hist[j]);
    }
    const bool row_here = uniform && a.rows && (key0 >> 1) < a.n_windows;  // (then only side key0 & 1 holds anything)
    if (tid < 2 * kCountFields) {
        const int sd = tid / kCountFields, f = tid % kCountFields;
        if (s_cnt[tid]) {
            atomicAdd(reinterpret_cast<unsigned long long *>(a.totals + sd) + f, (unsigned long long)s_cnt[tid]);
            if (row_here) atomicAdd(reinterpret_cast<unsigned long long *>(a.rows + key0) + f, (unsigned long long)s_cnt[tid]);
        }
    } else if (tid >= 64 && tid < 64 + 2 * kSumFields) {
        const int j = tid - 64, sd = j / kSumFields, f = j % kSumFields;
        if (s_cnt[sd * kCountFields]) {
            unsafeAtomicAdd(reinterpret_cast<double *>(a.totals + sd) + kCountFields + f, s_sum[j]);
            if (row_here) unsafeAtomicAdd(reinterpret_cast<double *>(a.rows + key0) + kCountFields + f, s_sum[j]);
        }
    }
}

hipError_t launch_metrics(const MetricsLaunch &a, hipStream_t stream) {
    if (!a.n) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((uint64_t)a.n + kMetricsThreads - 1) / kMetricsThreads);
    hipLaunchKernelGGL(metrics_kernel, dim3(blocks), dim3(kMetricsThreads), 0, stream, a);
    return hipGetLastError();
}

int MetricsTable::score(MetricsLaunch a, hipStream_t stream) {
    if (!a.n) return FWGPU_OK;
    if (!window || a.first_number == 0 || a.first_number + (a.n - 1) < a.first_number)
        return fail(FWGPU_ERR_INVALID, "metrics: window 0, or stream numbers that do not start at 1 or wrap");
    if (!d_totals) {
        FWGPU_HIP(hipMalloc(&d_totals, kTotalsBytes));
        FWGPU_HIP(hipMemsetAsync(d_totals, 0, kTotalsBytes, stream));
    }
    const uint64_t need = (a.first_number + (a.n - 1) - 1) / window + 1;
    if (need > cap) {
        const uint64_t ncap = std::max<uint64_t>(std::max<uint64_t>(need, cap * 2), 64);
        fwgpu_metric_sums *nrows = nullptr;
        FWGPU_HIP(hipMalloc((void **)&nrows, ncap * 2 * sizeof(fwgpu_metric_sums)));
        hipError_t e = hipSuccess;
        if (cap) e = hipMemcpyAsync(nrows, d_rows, cap * 2 * sizeof(fwgpu_metric_sums), hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess) e = hipMemsetAsync(nrows + cap * 2, 0, (ncap - cap) * 2 * sizeof(fwgpu_metric_sums), stream);
        if (e == hipSuccess && d_rows) e = hipStreamSynchronize(stream);  // (the copy has read the old rows)
        if (e != hipSuccess) {
            (void)hipFree(nrows);
            FWGPU_HIP(e);
        }
        if (d_rows) (void)hipFree(d_rows);
        d_rows = nrows;
        cap = ncap;
    }
    used = std::max(used, need);
    a.window = window;
    a.rows = d_rows;
    a.n_windows = cap;
    a.totals = static_cast<fwgpu_metric_sums *>(d_totals);
    a.hist = reinterpret_cast<unsigned long long *>(a.totals + 2);
    FWGPU_HIP(launch_metrics(a, stream));
    return FWGPU_OK;
}

int MetricsTable::fetch(uint64_t first_window, uint64_t n_windows, fwgpu_metric_window *rows, fwgpu_metric_total *learned,
                        fwgpu_metric_total *held_out, hipStream_t stream) {
    FWGPU_HIP(hipStreamSynchronize(stream));
    if (rows && n_windows) {
        if (first_window + n_windows > cap) return fail(FWGPU_ERR_RANGE, "metrics: windows beyond the table");
        std::vector<fwgpu_metric_sums> h((size_t)n_windows * 2);
        FWGPU_HIP(hipMemcpy(h.data(), d_rows + first_window * 2, h.size() * sizeof(fwgpu_metric_sums), hipMemcpyDeviceToHost));
        for (uint64_t j = 0; j < n_windows; j++) {
            rows[j].first_number = (first_window + j) * window + 1;
            rows[j].learned = h[2 * j];
            rows[j].held_out = h[2 * j + 1];
        }
    }
    fwgpu_metric_total *out[2] = {learned, held_out};
    if (!d_totals) {
        for (fwgpu_metric_total *t : out)
            if (t) *t = fwgpu_metric_total{};
        return FWGPU_OK;
    }
    std::vector<unsigned char> h(kTotalsBytes);
    FWGPU_HIP(hipMemcpy(h.data(), d_totals, kTotalsBytes, hipMemcpyDeviceToHost));
    for (int sd = 0; sd < 2; sd++) {
        if (!out[sd]) continue;
        memcpy(&out[sd]->sums, h.data() + sd * sizeof(fwgpu_metric_sums), sizeof(fwgpu_metric_sums));
        memcpy(out[sd]->hist, h.data() + 2 * sizeof(fwgpu_metric_sums) + (size_t)sd * 512 * 8, 512 * 8);
    }
    return FWGPU_OK;
}

void MetricsTable::release() {
    if (d_rows) (void)hipFree(d_rows);
    if (d_totals) (void)hipFree(d_totals);
    d_rows = nullptr;
    d_totals = nullptr;
    cap = used = 0;
}

void metrics_from_batch(const fwgpu_batch *b, uint32_t first, uint32_t n, MetricsLaunch *a) {
    a->pred = b->pred + first;
    a->n = n;
    if (b->records) {
        a->records = b->records;
        a->rec_off = b->rec_off + first;
    } else {
        a->label = b->label + first;
        a->importance = b->importance + first;
    }
}

}  // namespace fwgpu

using namespace fwgpu;

extern "C" int fwgpu_batch_metrics(fwgpu_batch *b, uint32_t first, uint32_t n, int learned, fwgpu_metric_sums *out, uint64_t *hist512, void *stream) {
    if (!b || !out) return fail(FWGPU_ERR_INVALID, "NULL argument");
    if ((uint64_t)first + n > b->n) return fail(FWGPU_ERR_RANGE, "batch_metrics: first + n beyond the batch");
    *out = fwgpu_metric_sums{};
    if (hist512) memset(hist512, 0, 512 * 8);
    if (!n) return FWGPU_OK;
    fwgpu_regressor *r = b->owner;
    if (!r) return fail(FWGPU_ERR_INVALID, "batch_metrics: a batch without a regressor");
    hipStream_t st = static_cast<hipStream_t>(stream);
    FWGPU_HIP(hipSetDevice(r->device));
    if (!r->metrics_scratch) FWGPU_HIP(hipMalloc(&r->metrics_scratch, kTotalsBytes));
    FWGPU_HIP(hipMemsetAsync(r->metrics_scratch, 0, kTotalsBytes, st));
    MetricsLaunch a;
    metrics_from_batch(b, first, n, &a);
    a.learned_all = learned != 0;
    a.totals = static_cast<fwgpu_metric_sums *>(r->metrics_scratch);
    a.hist = reinterpret_cast<unsigned long long *>(a.totals + 2);
    FWGPU_HIP(launch_metrics(a, st));
    const int sd = learned ? 0 : 1;
    FWGPU_HIP(hipMemcpyAsync(out, a.totals + sd, sizeof(*out), hipMemcpyDeviceToHost, st));
    if (hist512) FWGPU_HIP(hipMemcpyAsync(hist512, a.hist + sd * 512, 512 * 8, hipMemcpyDeviceToHost, st));
    FWGPU_HIP(hipStreamSynchronize(st));
    return FWGPU_OK;
}

namespace {
struct DevArrays {  // frees what it allocated when it goes
    void *p[4] = {nullptr, nullptr, nullptr, nullptr};
    int n = 0;
    hipError_t up(const void *host, size_t bytes, void **out) {
        hipError_t e = hipMalloc(&p[n], bytes);
        if (e != hipSuccess) return e;
        *out = p[n++];
        return hipMemcpy(*out, host, bytes, hipMemcpyHostToDevice);
    }
    ~DevArrays() {
        for (int i = 0; i < n; i++) (void)hipFree(p[i]);
    }
};
struct TableGuard {
    MetricsTable t;
    ~TableGuard() { t.release(); }
};
}  // namespace

extern "C" int fwgpu_debug_metrics(const float *pred, const float *label, const float *importance, const uint8_t *learned, uint64_t first_number,
                                   uint32_t n, uint64_t window, uint32_t launch, fwgpu_metric_window *rows, uint64_t cap, uint64_t *n_rows,
                                   fwgpu_metric_total *learned_total, fwgpu_metric_total *held_out_total, void *stream) {
    if (!n_rows || (n && (!pred || !label || !importance || !learned))) return fail(FWGPU_ERR_INVALID, "debug_metrics: NULL argument");
    if (!window || !first_number || first_number + n < first_number) return fail(FWGPU_ERR_INVALID, "debug_metrics: window 0, or stream numbers that do not start at 1 or wrap");
    const uint64_t w0 = (first_number - 1) / window;
    *n_rows = n ? (first_number + n - 2) / window - w0 + 1 : 0;
    if (rows && cap < *n_rows) return fail(FWGPU_ERR_RANGE, "debug_metrics: buffer too small for the windows");
    hipStream_t st = static_cast<hipStream_t>(stream);
    TableGuard g;
    g.t.window = window;
    DevArrays mem;
    MetricsLaunch all;
    if (n) {
        FWGPU_HIP(mem.up(pred, (size_t)n * 4, (void **)&all.pred));
        FWGPU_HIP(mem.up(label, (size_t)n * 4, (void **)&all.label));
        FWGPU_HIP(mem.up(importance, (size_t)n * 4, (void **)&all.importance));
        FWGPU_HIP(mem.up(learned, (size_t)n, (void **)&all.learned));
    }
    const uint32_t step = launch ? launch : n;
    for (uint32_t i = 0; i < n; i += step) {
        MetricsLaunch a;
        a.pred = all.pred + i;
        a.label = all.label + i;
        a.importance = all.importance + i;
        a.learned = all.learned + i;
        a.n = std::min(step, n - i);
        a.first_number = first_number + i;
        int rc = g.t.score(a, st);
        if (rc) return rc;
        if (n - i <= step) break;  // (i += step may wrap)
    }
    return g.t.fetch(w0, rows ? *n_rows : 0, rows, learned_total, held_out_total, st);
}
