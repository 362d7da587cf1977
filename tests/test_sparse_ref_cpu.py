"""The float32 restatement of the sparse-bucket reduce and apply steps (sparse_ref.py) against a float64 evaluation of the same
sums, on the CPU: the check that the reference indexes the right things before it judges the kernels bit for bit
(test_gpu_sparse_kernels.py).  The float64 side is written element by element with dictionaries, not with the reference's slices.

Bound: an in-order float32 evaluation of a sum of products differs from the exact one by at most n_ops * 2^-24 * (sum of the
absolute terms) to first order, n_ops the rounded operations on the longest path to the result; the tests allow
n_ops * 2^-23, twice that.  Per occurrence a bucket-row element takes at most 5 rounded operations (sw * v, the subtraction, v * x,
g * G, the addition); an applied element one addition per bucket row and at most 6 for the step."""
import numpy as np
import pytest

import sparse_ref as sr

EPS = 2.0 ** -23


def _reduce_case(seed, F, k, n_ex, max_entries, n_hashes, n_pad):
    rng = np.random.default_rng(seed)
    R = F * k
    split_len = F * R + 3
    selfw_stride = max_entries * k + 1
    slots = n_ex * max_entries
    keys = np.full(slots, sr.NO_KEY, dtype=np.uint64)
    used = rng.permutation(slots)[:slots - n_pad]
    hashes = rng.integers(0, 1 << 12, size=n_hashes)
    keys[used] = (rng.choice(hashes, size=len(used)).astype(np.uint64) << np.uint64(32)) | used.astype(np.uint64)
    desc = np.zeros((slots, 2), dtype=np.uint32)
    desc[:, 0] = np.where(rng.random(slots) < 0.5, 1.0, rng.normal(size=slots)).astype(np.float32).view(np.uint32)
    desc[:, 1] = rng.integers(0, F, size=slots)
    split = rng.normal(size=n_ex * split_len).astype(np.float32)
    selfw = rng.normal(size=n_ex * selfw_stride).astype(np.float32)
    gbuf = rng.normal(size=n_ex).astype(np.float32)
    return dict(keys=keys, desc=desc, max_entries=max_entries, R=R, k=k, split=split, split_len=split_len, selfw=selfw,
                selfw_stride=selfw_stride, gbuf=gbuf)


def _reduce64(c, lr):
    """bucket rows in float64, per element: {(block of 64, hash): (row, sum of absolute terms, occurrences)} in list order"""
    ks = [int(x) for x in np.sort(c["keys"]) if x != sr.NO_KEY]
    val = c["desc"][:, 0].copy().view(np.float32).astype(np.float64)
    out = {}
    for pos, key in enumerate(ks):
        h, slot = key >> 32, key & 0xFFFFFFFF
        ex, ii = divmod(slot, c["max_entries"])
        v, f, g = val[slot], int(c["desc"][slot, 1]), float(c["gbuf"][ex])
        R, k = c["R"], c["k"]
        row, mag, cnt = out.setdefault((pos // 64, h), (np.zeros(max(R, 1)), np.zeros(max(R, 1)), [0]))
        cnt[0] += 1
        if lr:
            row[0] += g * v
            mag[0] += abs(g * v)
            continue
        for e in range(R):
            x = float(c["split"][ex * c["split_len"] + f * R + e])
            own = float(c["selfw"][ex * c["selfw_stride"] + ii * k + e % k]) * v if e // k == f else 0.0
            row[e] += g * (v * (x - own))
            mag[e] += abs(g * v) * (abs(x) + abs(own))
    return out


@pytest.mark.parametrize("seed,F,k,lr", [(1, 3, 2, False), (2, 5, 4, False), (3, 3, 2, True)])
def test_reduce_ref_equals_float64_sums_cpu(seed, F, k, lr):
    c = _reduce_case(seed, F, k, n_ex=40, max_entries=5, n_hashes=9, n_pad=23)
    if lr:
        c = dict(c, R=0)
    count, bk_key, bk_rows = sr.reduce_ref(**c)
    want = _reduce64(c, lr)
    assert count == len(want) == len(bk_key) == len(bk_rows) and count > (200 - 23) // 64 + 1
    # list order: by block, then by hash
    assert [h for _, h in sorted(want)] == [int(h) for h in bk_key]
    longest = 0
    for j, key in enumerate(sorted(want)):
        row, mag, cnt = want[key]
        longest = max(longest, cnt[0])
        got = np.asarray(bk_rows[j], dtype=np.float64).reshape(-1)
        assert got.dtype == np.float64 and bk_rows.dtype == np.float32
        assert np.all(np.abs(got - row) <= 5 * cnt[0] * EPS * mag), (key, float(np.abs(got - row).max()))
        assert np.count_nonzero(row) == row.size  # every element of the row received something
    assert longest >= 10  # runs long enough that a wrong order or a dropped occurrence shows


def _apply_case(seed, R, n_ranks, stride, table):
    rng = np.random.default_rng(seed)
    width = max(R, 1)
    counts = [stride - 1 - r for r in range(n_ranks)]
    base = rng.integers(0, table - width, size=6)
    step = max(width // 4, 1)
    pool = np.unique(np.concatenate([base, base[:3] + step, base[:2] + 2 * step]))  # overlapping rows
    pool = pool[pool <= table - width]
    all_key = rng.choice(pool, size=n_ranks * stride).astype(np.uint32)
    all_rows = rng.normal(size=(n_ranks * stride, width)).astype(np.float32)
    w = rng.normal(size=table).astype(np.float32)
    acc = (1.0 + rng.random(table)).astype(np.float32)
    lut = (0.01 + rng.random(2048)).astype(np.float32)
    return dict(all_key=all_key, all_rows=all_rows, counts=counts, stride=stride), w, acc, lut


def _apply64(c, R, w, acc, optimizer, rate, mpt, lut):
    """the step in float64, element by element: (w, acc, tolerance per element of w, of acc)"""
    width = max(R, 1)
    sums, mags, terms = {}, {}, {}
    for r, cnt in enumerate(c["counts"]):
        for u in range(cnt):
            i = r * c["stride"] + u
            h = int(c["all_key"][i])
            sums[h] = sums.get(h, np.zeros(width)) + c["all_rows"][i].astype(np.float64)
            mags[h] = mags.get(h, np.zeros(width)) + np.abs(c["all_rows"][i].astype(np.float64))
            terms[h] = terms.get(h, 0) + 1
    w64, a64 = w.astype(np.float64), acc.astype(np.float64)
    tw, ta = np.abs(w64) * 0, np.abs(a64) * 0
    order = sorted(sums) if R == 0 else sorted(sums, key=lambda h: ((h // R) & 1, h))
    for h in order:
        for e in range(width):
            G, M, n = sums[h][e], mags[h][e], terms[h] + 6
            if optimizer == sr.OPT_SGD:
                u, um = G * rate, M * rate
            else:
                a64[h + e] += G * G
                ta[h + e] += n * EPS * (a64[h + e] + M * M)
                if optimizer == sr.OPT_ADAGRAD_LUT:
                    key = (int(np.float32(a64[h + e]).view(np.uint32)) >> 20) & 2047
                    u, um = G * float(lut[key]), M * float(lut[key])
                else:
                    p = a64[h + e] ** mpt
                    u, um = G * rate * p, M * rate * p
            tw[h + e] += n * EPS * (abs(w64[h + e]) + um)
            w64[h + e] -= u
    return w64, a64, tw, ta


@pytest.mark.parametrize("seed,R,optimizer", [(11, 8, sr.OPT_SGD), (12, 12, sr.OPT_ADAGRAD_FLEX), (13, 8, sr.OPT_ADAGRAD_LUT),
                                               (14, 0, sr.OPT_SGD), (15, 0, sr.OPT_ADAGRAD_FLEX), (16, 0, sr.OPT_ADAGRAD_LUT)])
def test_apply_ref_equals_float64_steps_cpu(seed, R, optimizer):
    table, rate, mpt = 400, 0.05, -0.5
    c, w, acc, lut = _apply_case(seed, R, n_ranks=3, stride=9, table=table)
    if R:
        w32, a32 = sr.apply_ffm_ref(R=R, w=w, acc=acc, optimizer=optimizer, rate=rate, minus_power_t=mpt, lut=lut, **c)
    else:
        out = sr.apply_lr_ref(c["all_key"], c["all_rows"].reshape(-1), c["counts"], c["stride"], np.stack([w, acc], axis=1), optimizer, rate, mpt, lut)
        w32, a32 = out[:, 0], out[:, 1]
    assert w32.dtype == np.float32 and a32.dtype == np.float32
    w64, a64, tw, ta = _apply64(c, R, w, acc, optimizer, np.float64(np.float32(rate)), mpt, lut)
    assert np.all(np.abs(w32 - w64) <= tw), float(np.abs(w32 - w64).max())
    assert np.all(np.abs(a32 - a64) <= ta), float(np.abs(a32 - a64).max())
    touched = tw > 0
    assert 0 < touched.sum() < table and np.array_equal(w32[~touched], w[~touched]) and np.array_equal(a32[~touched], acc[~touched])
    assert not np.array_equal(w32[touched], w[touched])
    if optimizer == sr.OPT_SGD:
        assert np.array_equal(a32, acc)


def test_a_zero_gradient_sum_touches_nothing_cpu():
    """two bucket rows of one hash that cancel exactly in half of their elements: those elements of w and acc keep their bits"""
    rng = np.random.default_rng(21)
    R = 8
    rows = rng.normal(size=(2, R)).astype(np.float32)
    rows[1, ::2] = -rows[0, ::2]
    w = rng.normal(size=32).astype(np.float32)
    acc = np.ones(32, dtype=np.float32)
    lut = np.full(2048, 0.25, dtype=np.float32)
    w2, a2 = sr.apply_ffm_ref(np.array([8, 8], dtype=np.uint32), rows, [1, 1], 1, R, w, acc, sr.OPT_ADAGRAD_LUT, 0.1, -0.5, lut)
    assert np.array_equal(w2[8:16:2], w[8:16:2]) and np.array_equal(a2[8:16:2], acc[8:16:2])
    assert np.all(w2[9:16:2] != w[9:16:2]) and np.all(a2[9:16:2] != acc[9:16:2])
    assert np.array_equal(w2[:8], w[:8]) and np.array_equal(w2[16:], w[16:])
