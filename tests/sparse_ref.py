"""A plain NumPy float32 restatement of the reduce and apply steps of the row-sparse gradient buckets (sparse.hip), for
test_gpu_sparse_kernels.py (kernel against this, bit for bit) and test_sparse_ref_cpu.py (this against float64 sums).

The kernels take every product and sum with __fmul_rn / __fadd_rn in a stated order and the library is built without FMA
contraction, so the same IEEE float32 operations in the same order give the same bits.  Everything here is an np.float32
scalar or array, one rounded operation per statement (NumPy rounds every elementwise result to float32 before the next one
sees it, so nothing is fused or reordered); the only loops that matter for the order are the ones over occurrences / bucket rows.

Layouts, as the FWD phase of kernels.hip writes them:
  key      = hash << 32 | slot, or ~0 for padding;  slot = example * max_entries + entry
  desc     [slots, 2] uint32: {value bits, field}
  split    [example * split_len + field * R + e]: the field sums T[field] of the example
  selfw    [example * selfw_stride + entry * k + e % k]: the entry's own slot of its row
  gbuf     [example]: the general gradient"""
import numpy as np

NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
OPT_SGD, OPT_ADAGRAD_FLEX, OPT_ADAGRAD_LUT = 100, 200, 300
F32 = np.float32


def sorted_valid(keys):
    """the occurrence keys in the order the reduce kernels see them: ascending as uint64, padding (sorts last) dropped"""
    ks = np.sort(np.asarray(keys, dtype=np.uint64))
    return ks[ks != NO_KEY]


def runs_of(ks):
    """[(start, end)] of the bucket rows of a sorted valid key list: inside every block of 64, each run of equal high words"""
    h = (ks >> np.uint64(32)).astype(np.uint32)
    out = []
    for b0 in range(0, len(ks), 64):
        b1 = min(b0 + 64, len(ks))
        s = b0
        for i in range(b0 + 1, b1 + 1):
            if i == b1 or h[i] != h[s]:
                out.append((s, i))
                s = i
    return out


def reduce_ref(keys, desc, max_entries, R, k, split, split_len, selfw, selfw_stride, gbuf):
    """(count, bucket keys uint32 [count], bucket rows float32 [count, R]; R == 0 (LR): rows [count])"""
    ks = sorted_valid(keys)
    hs = (ks >> np.uint64(32)).astype(np.uint32)
    slots = (ks & np.uint64(0xFFFFFFFF)).astype(np.int64)
    desc = np.asarray(desc, dtype=np.uint32).reshape(-1, 2)
    values = desc[:, 0].copy().view(F32)
    fields = desc[:, 1]
    gbuf = np.asarray(gbuf, dtype=F32)
    runs = runs_of(ks)
    bk_key = np.array([hs[s] for s, _ in runs], dtype=np.uint32)
    if R == 0:
        bk_val = np.zeros(len(runs), dtype=F32)
        for j, (s, t) in enumerate(runs):
            acc = F32(0.0)
            for i in range(s, t):
                slot = slots[i]
                grad = gbuf[slot // max_entries] * values[slot]
                acc = acc + grad
            bk_val[j] = acc
        return len(runs), bk_key, bk_val
    split = np.asarray(split, dtype=F32)
    selfw = np.asarray(selfw, dtype=F32)
    bk_rows = np.zeros((len(runs), R), dtype=F32)
    for j, (s, t) in enumerate(runs):
        row = np.zeros(R, dtype=F32)  # +0.0
        for i in range(s, t):
            slot = int(slots[i])
            ex = slot // max_entries
            ii = slot % max_entries
            v = values[slot]
            f = int(fields[slot])
            g = gbuf[ex]
            x = split[ex * split_len + f * R:ex * split_len + f * R + R].copy()
            # the own-slot correction: the elements e with e // k == f, i.e. e in [f * k, f * k + k), where e % k = e - f * k
            sw = selfw[ex * selfw_stride + ii * k:ex * selfw_stride + ii * k + k]
            swv = sw * v
            own = x[f * k:f * k + k] - swv
            x[f * k:f * k + k] = own
            G = v * x
            gG = g * G
            row = row + gG
        bk_rows[j] = row
    return len(runs), bk_key, bk_rows


def merged_order(all_key, counts, stride):
    """the valid elements i = rank * stride + u, u < counts[rank], sorted by (all_key[i], i)"""
    idx = np.concatenate([r * stride + np.arange(int(c), dtype=np.int64) for r, c in enumerate(counts)] + [np.zeros(0, dtype=np.int64)])
    all_key = np.asarray(all_key, dtype=np.uint32)
    order = np.lexsort((idx, all_key[idx]))
    return idx[order]


def _step(G, w, acc, optimizer, rate, minus_power_t, lut):
    """one optimizer step with the gradients G on the views w / acc, in place; elements with G == 0 are not touched.
    A float64 `w` selects the float64 form of the AdagradFlex update (pow in float64, the accumulator still float32)."""
    on = G != F32(0.0)
    g = G[on]
    if optimizer == OPT_SGD:
        u = g * F32(rate)
    else:
        gg = g * g
        na = acc[on] + gg
        acc[on] = na
        if optimizer == OPT_ADAGRAD_LUT:
            key = (na.view(np.uint32) >> np.uint32(20)) & np.uint32(2047)
            u = g * lut[key]
        else:
            gr = g * F32(rate)
            if w.dtype == np.float64:
                u = gr.astype(np.float64) * np.power(na.astype(np.float64), np.float64(minus_power_t))
            else:
                with np.errstate(all="ignore"):
                    p = np.power(na, F32(minus_power_t))
                    u = gr * p
            u[~np.isfinite(u)] = 0
    w[on] = w[on] - u


def apply_ffm_ref(all_key, all_rows, counts, stride, R, w, acc, optimizer, rate, minus_power_t, lut):
    """(w, acc) after the step; the inputs are not changed"""
    w, acc = np.array(w), np.array(acc, dtype=F32)
    all_rows = np.asarray(all_rows, dtype=F32).reshape(-1, R)
    all_key = np.asarray(all_key, dtype=np.uint32)
    lut = np.asarray(lut, dtype=F32)
    idx = merged_order(all_key, counts, stride)
    hashes, sums = [], []
    a = 0
    while a < len(idx):
        h = int(all_key[idx[a]])
        G = np.zeros(R, dtype=F32)  # +0.0
        while a < len(idx) and int(all_key[idx[a]]) == h:
            G = G + all_rows[idx[a]]
            a += 1
        hashes.append(h)
        sums.append(G)
    for parity in (0, 1):
        for h, G in zip(hashes, sums):  # ascending
            if ((h // R) & 1) == parity:
                _step(G, w[h:h + R], acc[h:h + R], optimizer, rate, minus_power_t, lut)
    return w, acc


def apply_lr_ref(all_key, all_vals, counts, stride, lr, optimizer, rate, minus_power_t, lut):
    """the {w, acc} pair table [entries, 2] after the step"""
    lr = np.array(lr).reshape(-1, 2)
    all_vals = np.asarray(all_vals, dtype=F32)
    all_key = np.asarray(all_key, dtype=np.uint32)
    lut = np.asarray(lut, dtype=F32)
    idx = merged_order(all_key, counts, stride)
    wcol, acol = lr[:, 0].copy(), lr[:, 1].astype(F32)
    a = 0
    while a < len(idx):
        h = int(all_key[idx[a]])
        G = np.zeros(1, dtype=F32)
        while a < len(idx) and int(all_key[idx[a]]) == h:
            G = G + all_vals[idx[a]]
            a += 1
        _step(G, wcol[h:h + 1], acol[h:h + 1], optimizer, rate, minus_power_t, lut)
    return np.stack([wcol, acol.astype(wcol.dtype)], axis=1)
