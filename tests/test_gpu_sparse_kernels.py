"""The reduce and apply kernels of the row-sparse gradient buckets (sparse.hip), each called directly through
fwgpu_debug_sparse_reduce / fwgpu_debug_sparse_apply and compared BIT FOR BIT with the NumPy float32 restatement in sparse_ref.py
(test_sparse_ref_cpu.py pins that restatement against float64 sums).  The kernels take every product and sum with __fmul_rn / __fadd_rn
in a stated order and the library is built without FMA contraction: both sides do the same IEEE operations in the same order, so there is
no tolerance anywhere except for powf (the AdagradFlex run at minus_power_t = -0.5, see FLEX_POW_ULPS).

Every output buffer lies between two guard zones of at least R sentinel words; the zones, the bucket rows beyond count * R and the bucket
keys beyond count must come back unchanged."""
import ctypes as C
import functools

import numpy as np
import pytest

import sparse_ref as sr
from fwumious_wabbit_amd import _capi as capi

pytestmark = pytest.mark.gpu

U32, F32 = np.uint32, np.float32
SENT = U32(0xDEADBEEF)  # (as a float: -6.26e18, a normal number no sum of the tests comes near)
N_EX, MAX_ENTRIES = 64, 24  # the occurrence slots of the reduce cases: 1 536
HASH_BITS = 15
OPTS = [sr.OPT_SGD, sr.OPT_ADAGRAD_LUT, sr.OPT_ADAGRAD_FLEX]
RATE = 0.05
# AdagradFlex at minus_power_t = -0.5: the largest |update_gpu - update_float64| in units of the last place of the update, over the cases of
# test_flex_with_a_real_exponent_*, measured on an MI355X; the tests assert twice that.  The update is fl(fl(G * rate) * powf(acc, -0.5)):
# half a unit from the product on top of the math library's powf, none of it this project's arithmetic.  Measured per case: R = 40: 1.221,
# R = 280: 1.771, R = 480: 1.801, LR: 0.511.
FLEX_POW_ULPS = 1.801


def _torch():
    import torch

    return torch


def _dev(a):
    """a NumPy array of 32- or 64-bit items on the device, bits unchanged"""
    a = np.ascontiguousarray(a)
    if a.size == 0:
        a = np.zeros(4, dtype=a.dtype)  # (an empty tensor has no address)
    if a.dtype != np.float32:
        a = a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)
    return _torch().from_numpy(a).cuda()


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def _guard(R):
    return (max(R, 8) + 3) // 4 * 4  # at least R words, and the payload stays on a 16-byte boundary


class Guarded:
    """a device buffer of 32-bit words between two guard zones of sentinel words"""

    def __init__(self, init, guard):
        init = np.ascontiguousarray(init).view(U32).reshape(-1)
        self.guard, self.n = guard, len(init)
        self.t = _dev(np.concatenate([np.full(guard, SENT), init, np.full(guard, SENT)]))
        assert self.ptr % 16 == 0

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.guard

    def read(self):
        """the payload as uint32; the guard zones must be as they were"""
        host = self.t.cpu().numpy().view(U32)
        g, n = self.guard, self.n
        assert np.all(host[:g] == SENT), "written before the buffer"
        assert np.all(host[g + n:] == SENT), "written beyond the buffer"
        return host[g:g + n].copy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(U32)


def _same_bits(got_u32, want_f32, what):
    want = _bits(want_f32).reshape(-1)
    got = np.asarray(got_u32).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} words differ, first at {bad[:8].tolist()} .. last {int(bad[-1])}: "
                             f"got {got[bad[:4]].view(F32).tolist()} want {want[bad[:4]].view(F32).tolist()}")


# ------------------------------------------------------------------ reduce
REDUCE_SHAPES = [(4, 2), (10, 4), (16, 16), (17, 16), (30, 16), (33, 16), (28, 10), (65, 4)]
# R =          8        40       256       272       480       528       280       260


def _key_list(rng, hashes_sorted, n_total):
    """keys of the occurrences whose hashes are `hashes_sorted` (that is the order the sorted list will have), each on a random slot of its
    own, at random positions of a list of n_total keys; the other positions are padding"""
    hs = np.asarray(hashes_sorted, dtype=np.uint64)
    slots = rng.permutation(N_EX * MAX_ENTRIES)[:len(hs)].astype(np.uint64)
    keys = np.full(n_total, sr.NO_KEY, dtype=np.uint64)
    keys[rng.permutation(n_total)[:len(hs)]] = (hs << np.uint64(32)) | slots
    return keys


def _big_list(rng):
    """1 473 = 23 * 64 + 1 occurrences: runs of 30 and 34 (the second ends exactly at the first block edge), 20, then ONE HASH 200 TIMES from
    position 84 (the middle of block 1: four bucket rows), 36 (ends at position 320, a block edge), runs of 1..9 for the rest; the last
    block holds one valid key.  63 padding keys are scattered through the unsorted list."""
    lens, total = [30, 34, 20, 200, 36], 320
    while total < 1473:
        lens.append(int(min(rng.integers(1, 10), 1473 - total)))
        total += lens[-1]
    hashes = np.sort(rng.choice(1 << HASH_BITS, size=len(lens), replace=False))
    keys = _key_list(rng, np.repeat(hashes, lens), N_EX * MAX_ENTRIES)
    ks = sr.sorted_valid(keys)
    runs = sr.runs_of(ks)
    hot = [(s, t) for s, t in runs if int(ks[s] >> np.uint64(32)) == int(hashes[3])]
    assert hot == [(84, 128), (128, 192), (192, 256), (256, 284)]
    assert (30, 64) in runs and (284, 320) in runs and runs[-1] == (1472, 1473) and len(ks) % 4 == 1
    assert int(np.sum(keys == sr.NO_KEY)) == 63 and not np.all(keys[-63:] == sr.NO_KEY)
    return keys


def _small_list(rng, n_valid, n_pad):
    pool = np.sort(rng.choice(1 << HASH_BITS, size=5, replace=False))
    return _key_list(rng, np.sort(rng.choice(pool, size=n_valid)), n_valid + n_pad)


@functools.lru_cache(maxsize=None)
def _reduce_shape(F, k):
    """the inputs of one (F, k) shape, its key lists, and the reference's bucket rows for every list -- computed once, shared by the layouts"""
    rng = np.random.default_rng(1000 * F + k)
    R, slots = F * k, N_EX * MAX_ENTRIES
    straddle = 256 // k if 256 % k and 256 // k < F else None  # the field whose k floats lie on both sides of float 256
    special = [0, F - 1] + ([straddle] if straddle is not None else [])
    field = rng.integers(0, F, size=slots)
    pick = rng.random(slots)
    for j, f in enumerate(special):
        field[(pick >= 0.15 * j) & (pick < 0.15 * (j + 1))] = f
    desc = np.zeros((slots, 2), dtype=U32)
    desc[:, 0] = _bits(np.where(rng.random(slots) < 0.5, 1.0, rng.normal(size=slots)))
    desc[:, 1] = field
    d = dict(F=F, k=k, R=R, desc=desc, straddle=straddle,
             split=rng.normal(size=(N_EX, F * R)).astype(F32), selfw=rng.normal(size=(N_EX, MAX_ENTRIES * k)).astype(F32),
             gbuf=rng.normal(size=N_EX).astype(F32))
    lists = {"big": _big_list(rng)}
    for nv in (1, 63, 64, 65, 200):
        lists[f"n{nv}"] = _small_list(rng, nv, 5)
    lists["n64_no_padding"] = _small_list(rng, 64, 0)
    d["lists"] = lists
    used = field[(lists["big"][lists["big"] != sr.NO_KEY] & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    assert all(np.any(used == f) for f in special), "an own field of 0, F - 1 and the straddling field must occur"
    d["ref"] = {name: sr.reduce_ref(keys, desc, MAX_ENTRIES, R, k, d["split"].reshape(-1), F * R, d["selfw"].reshape(-1), MAX_ENTRIES * k, d["gbuf"])
                for name, keys in lists.items()}
    return d


class ReduceDevice:
    """the inputs of a shape on the device, the split records laid out with split_len % 4 == rem (the words between two records are NaNs)"""

    def __init__(self, d, rem):
        F, k, R = d["F"], d["k"], d["R"]
        self.d, self.R, self.k = d, R, k
        self.split_len = F * R + (rem - F * R) % 4 + 4
        assert self.split_len % 4 == rem
        self.selfw_stride = MAX_ENTRIES * k + 1
        split = np.full((N_EX, self.split_len), np.nan, dtype=F32)
        split[:, :F * R] = d["split"]
        selfw = np.full((N_EX, self.selfw_stride), np.nan, dtype=F32)
        selfw[:, :MAX_ENTRIES * k] = d["selfw"]
        self.split, self.selfw, self.gbuf, self.desc = _dev(split), _dev(selfw), _dev(d["gbuf"]), _dev(d["desc"])

    def run(self, keys, R=None):
        """(count, bucket keys, bucket rows as uint32 [count, max(R, 1)]) of fwgpu_debug_sparse_reduce; R = 0: the LR kernel"""
        R = self.R if R is None else R
        n, width, guard = len(keys), max(R, 1), _guard(R)
        bk_key = Guarded(np.full(n, SENT), guard)
        bk_rows = Guarded(np.full(n * width, SENT), guard)
        keys_t = _dev(keys)
        count = C.c_uint32(0xFFFFFFFF)
        capi.check(capi.lib().fwgpu_debug_sparse_reduce(keys_t.data_ptr(), n, 32 + HASH_BITS, self.desc.data_ptr(), MAX_ENTRIES, R, self.k if R else 0,
                                                        self.split.data_ptr(), self.split_len, self.selfw.data_ptr(), self.selfw_stride,
                                                        self.gbuf.data_ptr(), bk_key.ptr, bk_rows.ptr, C.byref(count), _stream()))
        c = count.value
        assert c <= n
        got_key, got_rows = bk_key.read(), bk_rows.read()
        assert np.all(got_key[c:] == SENT), "bucket keys written beyond the count"
        assert np.all(got_rows[c * width:] == SENT), "bucket rows written beyond count * R"
        return c, got_key[:c], got_rows[:c * width].reshape(c, width)


def _check_reduce(got, want, what):
    assert got[0] == want[0], (what, got[0], want[0])
    assert np.array_equal(got[1], want[1]), what
    _same_bits(got[2], want[2], what)


@pytest.mark.parametrize("F,k,rem", [(F, k, rem) for F, k in REDUCE_SHAPES for rem in ((0, 2) if k % 4 == 0 else (0, 3))])
def test_ffm_reduce_kernels_equal_the_float32_restatement_bit_for_bit(F, k, rem):
    """k % 4 == 0 and split_len % 4 == 0: sparse_reduce_ffm4_kernel (16-byte loads); every other (k, split_len): sparse_reduce_ffm_kernel.
    R = 8, 40: one pass with idle lanes; 256: exactly one pass; 260, 272, 280, 480: two passes of the 256-float loop; 528: three.
    (28, 10): field 25 holds floats 250..259, its own-slot correction is split between the passes."""
    d = _reduce_shape(F, k)
    dev = ReduceDevice(d, rem)
    other = ReduceDevice(d, 0) if k % 4 == 0 and rem else None  # the 16-byte kernel on the same data
    for name, keys in d["lists"].items():
        got = dev.run(keys)
        _check_reduce(got, d["ref"][name], (F, k, rem, name))
        if other is not None:
            got4 = other.run(keys)
            assert got4[0] == got[0] and np.array_equal(got4[1], got[1]) and np.array_equal(got4[2], got[2]), (F, k, name)
    assert d["ref"]["big"][0] > 1473 // 9 and d["ref"]["n1"][0] == 1


def test_lr_reduce_kernel_equals_the_float32_restatement_bit_for_bit():
    """sparse_reduce_lr_kernel (R == 0) on the same key lists: one float per bucket row, the in-order sum of g * value"""
    d = _reduce_shape(4, 2)
    dev = ReduceDevice(d, 0)
    for name, keys in d["lists"].items():
        want = sr.reduce_ref(keys, d["desc"], MAX_ENTRIES, 0, 0, None, 0, None, 0, d["gbuf"])
        assert want[0] == d["ref"][name][0]  # the same bucket rows as the FFM side
        _check_reduce(dev.run(keys, R=0), want, ("lr", name))


@pytest.mark.parametrize("F,k,rem,R", [(10, 4, 0, None), (28, 10, 0, None), (30, 16, 2, None), (4, 2, 0, 0)])
def test_reduce_of_nothing_writes_nothing(F, k, rem, R):
    """a list of padding keys only, and an empty list: count 0, no bucket key and no bucket row written (ReduceDevice.run checks the buffers)"""
    dev = ReduceDevice(_reduce_shape(F, k), rem)
    c, keys, rows = dev.run(np.full(70, sr.NO_KEY, dtype=np.uint64), R=R)
    assert c == 0 and len(keys) == 0 and len(rows) == 0
    c, keys, rows = dev.run(np.zeros(0, dtype=np.uint64), R=R)
    assert c == 0


# ------------------------------------------------------------------ apply
APPLY_SHAPES = [(8, 2), (40, 4), (256, 16), (272, 16), (480, 16), (280, 10)]  # (R, k): k4 = k % 4 == 0
NBLK = 12


def _table_len(R):
    return NBLK * R + R // 2 // 4 * 4  # (the last row that fits starts in the middle of block NBLK - 1)


@functools.lru_cache(maxsize=None)
def _apply_case(R, k, n_ranks):
    """the gathered bucket rows of n_ranks ranks (rank 1 of two or more lists nothing) with, in merged order:
      block 0   rows at 0, k, 2k: three rows that overlap, the first at offset 0 of the table
      block 2   rows at 2R + k, 2R + 2k
      block 3   one hash that every rank lists three times
      block 4/5 a row at 4R + R - k and one at 5R: the odd-parity launch reads what the even one wrote
      block 6   one hash listed twice by one rank, the rows exact negatives of each other in the even elements
      block 7   as many rows as put the next block's first element at merged index 61
      block 8   eight hashes, ten elements: the block begins at merged index 61 and ends beyond 64
      block 9+  ten random rows, and the last row that fits into the table"""
    rng = np.random.default_rng(100 * R + n_ranks)
    step = 4 if k % 4 == 0 else 1
    table = _table_len(R)
    live = [r for r in range(n_ranks) if n_ranks == 1 or r != 1]
    elems = []  # (hash, rank, row)

    def add(h, rank, row=None):
        assert h % step == 0 and 0 <= h <= table - R
        elems.append((int(h), rank, rng.normal(size=R).astype(F32) if row is None else row))

    add(0, live[0]), add(k, live[-1]), add(2 * k, live[0]), add(2 * k, live[-1])
    add(2 * R + k, live[-1]), add(2 * R + 2 * k, live[0])
    for r in live:
        for _ in range(3):
            add(3 * R + k, r)
    add(4 * R + R - k, live[0]), add(5 * R, live[-1])
    r1 = rng.normal(size=R).astype(F32)
    r2 = rng.normal(size=R).astype(F32)
    r2[::2] = -r1[::2]
    cancel = 6 * R  # (no other row reaches into [6R, 7R))
    add(cancel, live[0], r1), add(cancel, live[0], r2)
    dense = [8 * R + j * step for j in range(min(8, R // step))]
    for j, h in enumerate(dense):
        add(h, live[j % len(live)])
    add(dense[0], live[-1]), add(dense[-1], live[0])
    for j in range(10):
        add((9 + j % 2) * R + step * int(rng.integers(0, R // step)), live[int(rng.integers(0, len(live)))])
    add(table - R, live[0])
    before = sum(1 for h, _, _ in elems if h < 8 * R)
    for j in range((61 - before) % 64):
        add(7 * R + step * (j % min(16, R // step)), live[j % len(live)])
    per_rank = [[e for e in elems if e[1] == r] for r in range(n_ranks)]
    for r, lst in enumerate(per_rank):
        if n_ranks == 1:
            lst.sort(key=lambda e: e[0])  # (stable) one rank's list is not sorted again: (hash, index) order, as reduce leaves it
        else:
            per_rank[r] = [lst[i] for i in rng.permutation(len(lst))]
    counts = [len(lst) for lst in per_rank]
    stride = max(counts) + 3
    all_key = np.full(n_ranks * stride, SENT, dtype=U32)
    all_rows = np.full((n_ranks * stride, R), np.nan, dtype=F32)
    for r, lst in enumerate(per_rank):
        for u, (h, _, row) in enumerate(lst):
            all_key[r * stride + u] = h
            all_rows[r * stride + u] = row
    merged = all_key[sr.merged_order(all_key, counts, stride)]
    in8 = np.flatnonzero(merged // R == 8)
    assert 60 <= in8[0] <= 63 and in8[-1] >= 64 and len(in8) == len(dense) + 2, "block 8 must cross the first 64-element boundary of the merged list"
    assert all(c < stride for c in counts) and (n_ranks == 1 or counts[1] == 0) and sum(counts) > 70
    return dict(all_key=all_key, all_rows=all_rows, counts=counts, stride=stride, R=R, table=table, cancel=cancel)


def _key_bits(table):
    return 32 + int(np.ceil(np.log2(table)))


@functools.lru_cache(maxsize=None)
def _tables(n, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=n).astype(F32), (1.0 + rng.random(n)).astype(F32), (0.01 + rng.random(2048)).astype(F32)


def _gpu_apply(c, n_ranks, R, k4, w0, acc0, optimizer, mpt, lut):
    """(w, acc) as uint32 after fwgpu_debug_sparse_apply; R == 0: w0 is the {w, acc} pair table and acc comes back as None"""
    guard = _guard(R)
    W = Guarded(w0, guard)
    A = Guarded(acc0, guard) if R else None
    key_t, rows_t, counts_t, lut_t = _dev(c["all_key"]), _dev(c["all_rows"]), _dev(np.asarray(c["counts"], dtype=U32)), _dev(lut)
    capi.check(capi.lib().fwgpu_debug_sparse_apply(key_t.data_ptr(), rows_t.data_ptr(), counts_t.data_ptr(), n_ranks, c["stride"], _key_bits(c["table"]), R,
                                                   int(k4), W.ptr, A.ptr if R else None, optimizer, RATE, mpt, lut_t.data_ptr(), _stream()))
    return W.read(), A.read() if R else None


@pytest.mark.parametrize("n_ranks", [1, 2, 3, 4])
@pytest.mark.parametrize("optimizer", OPTS)
@pytest.mark.parametrize("R,k", APPLY_SHAPES)
def test_ffm_apply_kernels_equal_the_float32_restatement_bit_for_bit(R, k, optimizer, n_ranks):
    """k % 4 == 0: sparse_apply_ffm4_kernel<OPT> (16-byte buffer accesses, one wave per 64 merged elements), and for R = 40 and 480 also
    sparse_apply_ffm_kernel<OPT> on the same rows; k = 2, 10: the scalar kernel.  AdagradFlex with minus_power_t = 0: powf returns exactly 1."""
    c = _apply_case(R, k, n_ranks)
    w0, acc0, lut = _tables(c["table"], 7)
    want_w, want_acc = sr.apply_ffm_ref(c["all_key"], c["all_rows"], c["counts"], c["stride"], R, w0, acc0, optimizer, RATE, 0.0, lut)
    # the reference itself: the rows that cancel leave their even elements as they were, the other elements move
    h = c["cancel"]
    assert np.array_equal(_bits(want_w[h:h + R:2]), _bits(w0[h:h + R:2])) and np.array_equal(_bits(want_acc[h:h + R:2]), _bits(acc0[h:h + R:2]))
    assert np.all(want_w[h + 1:h + R:2] != w0[h + 1:h + R:2])
    assert np.array_equal(want_acc, acc0) == (optimizer == sr.OPT_SGD)
    results = []
    for k4 in ([1, 0] if (k % 4 == 0 and R in (40, 480)) else [int(k % 4 == 0)]):
        got_w, got_acc = _gpu_apply(c, n_ranks, R, k4, w0, acc0, optimizer, 0.0, lut)
        _same_bits(got_acc, want_acc, ("acc", R, k4, optimizer, n_ranks))
        _same_bits(got_w, want_w, ("w", R, k4, optimizer, n_ranks))
        assert np.array_equal(got_w[h:h + R:2], _bits(w0[h:h + R:2])) and np.array_equal(got_acc[h:h + R:2], _bits(acc0[h:h + R:2]))
        results.append((got_w, got_acc))
    for other in results[1:]:
        assert np.array_equal(other[0], results[0][0]) and np.array_equal(other[1], results[0][1])


LR_TABLE = 512


@functools.lru_cache(maxsize=None)
def _lr_apply_case(n_ranks):
    """LR bucket values: the first and the last entry of the table, a hash every rank lists three times, a hash whose two values cancel,
    random entries listed by one or several ranks"""
    rng = np.random.default_rng(50 + n_ranks)
    live = [r for r in range(n_ranks) if n_ranks == 1 or r != 1]
    elems = [(0, live[0], None), (LR_TABLE - 1, live[-1], None), (LR_TABLE - 1, live[0], None), (77, live[0], F32(0.625)), (77, live[-1], F32(-0.625))]
    elems += [(300, r, None) for r in live for _ in range(3)]
    elems += [(int(h), live[int(rng.integers(0, len(live)))], None) for h in rng.choice(np.arange(1, LR_TABLE - 1), size=150) if h != 77]
    elems = [(h, r, F32(rng.normal()) if v is None else v) for h, r, v in elems]
    per_rank = [[e for e in elems if e[1] == r] for r in range(n_ranks)]
    for r, lst in enumerate(per_rank):
        if n_ranks == 1:
            lst.sort(key=lambda e: e[0])
        else:
            per_rank[r] = [lst[i] for i in rng.permutation(len(lst))]
    counts = [len(lst) for lst in per_rank]
    stride = max(counts) + 3
    all_key = np.full(n_ranks * stride, SENT, dtype=U32)
    all_vals = np.full(n_ranks * stride, np.nan, dtype=F32)
    for r, lst in enumerate(per_rank):
        for u, (h, _, v) in enumerate(lst):
            all_key[r * stride + u], all_vals[r * stride + u] = h, v
    return dict(all_key=all_key, all_rows=all_vals, counts=counts, stride=stride, table=LR_TABLE)


@pytest.mark.parametrize("n_ranks", [1, 2, 3, 4])
@pytest.mark.parametrize("optimizer", OPTS)
def test_lr_apply_kernel_equals_the_float32_restatement_bit_for_bit(optimizer, n_ranks):
    """sparse_apply_lr_kernel<OPT> on the {w, acc} pair table: runs across ranks, a sum of exactly 0, the first and the last entry"""
    c = _lr_apply_case(n_ranks)
    w0, acc0, lut = _tables(LR_TABLE, 9)
    lr0 = np.stack([w0, acc0], axis=1)
    want = sr.apply_lr_ref(c["all_key"], c["all_rows"], c["counts"], c["stride"], lr0, optimizer, RATE, 0.0, lut)
    assert np.array_equal(_bits(want[77]), _bits(lr0[77])) and want[0, 0] != lr0[0, 0] and want[LR_TABLE - 1, 0] != lr0[LR_TABLE - 1, 0]
    got, _ = _gpu_apply(c, n_ranks, 0, 0, lr0, None, optimizer, 0.0, lut)
    _same_bits(got, want, ("lr", optimizer, n_ranks))


# ------------------------------------------------------------------ AdagradFlex with a real exponent
def _ulps(update_gpu, update64):
    """|update_gpu - update64| in units of the last place of the float32 next to update64"""
    unit = np.spacing(np.abs(update64).astype(F32)).astype(np.float64)
    return np.abs(update_gpu.astype(np.float64) - update64) / unit


@pytest.mark.parametrize("R,k,n_ranks", [(40, 4, 2), (280, 10, 3), (480, 16, 4), (0, 0, 3)])
def test_flex_with_a_real_exponent_keeps_acc_exact_and_w_within_powf(R, k, n_ranks):
    """minus_power_t = -0.5: acc bit for bit; w against the float64 pow.  The weights start at 0 and every element is stepped once (rows at block
    starts only), so that -w IS the kernel's update and its distance from the float64 one can be counted in units of its last place."""
    rng = np.random.default_rng(300 + R)
    width = max(R, 1)
    table = NBLK * R if R else LR_TABLE
    hashes = [b * R for b in range(NBLK)] if R else [0, 5, 6, 100, 101, 102, 400, LR_TABLE - 1]
    counts = [0 if (r == 1) else 2 * len(hashes) for r in range(n_ranks)]
    stride = 2 * len(hashes) + 1
    all_key = np.full(n_ranks * stride, SENT, dtype=U32)
    all_rows = np.full((n_ranks * stride, width), np.nan, dtype=F32)
    for r, cnt in enumerate(counts):
        if cnt:
            all_key[r * stride:r * stride + cnt] = rng.permutation(np.repeat(hashes, 2))
            all_rows[r * stride:r * stride + cnt] = rng.normal(size=(cnt, width))
    c = dict(all_key=all_key, all_rows=all_rows if R else all_rows.reshape(-1), counts=counts, stride=stride, table=table)
    _, acc0, lut = _tables(table, 11)
    if R:
        w64, want_acc = sr.apply_ffm_ref(all_key, all_rows, counts, stride, R, np.zeros(table), acc0, sr.OPT_ADAGRAD_FLEX, RATE, -0.5, lut)
        got_w, got_acc = _gpu_apply(c, n_ranks, R, k % 4 == 0, np.zeros(table, dtype=F32), acc0, sr.OPT_ADAGRAD_FLEX, -0.5, lut)
    else:
        out = sr.apply_lr_ref(all_key, c["all_rows"], counts, stride, np.stack([np.zeros(table), acc0.astype(np.float64)], axis=1), sr.OPT_ADAGRAD_FLEX, RATE, -0.5, lut)
        w64, want_acc = out[:, 0], out[:, 1].astype(F32)
        got, _ = _gpu_apply(c, n_ranks, 0, 0, np.stack([np.zeros(table, dtype=F32), acc0], axis=1), None, sr.OPT_ADAGRAD_FLEX, -0.5, lut)
        got = got.reshape(-1, 2)
        got_w, got_acc = got[:, 0].copy(), got[:, 1].copy()
    _same_bits(got_acc, want_acc, ("acc", R))
    stepped = w64 != 0
    assert stepped.sum() == len(hashes) * width and np.all(got_w[~stepped] == 0)
    worst = float(_ulps(-got_w.view(F32)[stepped], -w64[stepped]).max())
    print(f"AdagradFlex minus_power_t=-0.5 R={R}: largest update difference from float64 pow = {worst:.3f} units in the last place")
    assert worst <= 2 * FLEX_POW_ULPS, worst


# ------------------------------------------------------------------ reduce -> apply
@pytest.mark.parametrize("F,k", [(30, 16), (28, 10)])
def test_reduce_output_applied_as_three_ranks_equals_the_restatement(F, k):
    """three key lists reduced on the device, their bucket keys and rows handed to the apply as three ranks' buckets: tables bit for bit
    equal to apply_ffm_ref(reduce_ref(...))"""
    d = _reduce_shape(F, k)
    R, table = F * k, _table_len(F * k)
    step = 4 if k % 4 == 0 else 1
    rng = np.random.default_rng(17 * F)
    pool = np.unique(np.concatenate([[0, k, 2 * k, 4 * R + R - k, 5 * R, table - R], step * rng.integers(0, (table - R) // step, size=24)]))
    dev = ReduceDevice(d, 0)
    got, want = [], []
    for nv in (200, 65, 150):
        keys = _key_list(rng, np.sort(rng.choice(pool, size=nv)), nv + 9)
        got.append(dev.run(keys))
        want.append(sr.reduce_ref(keys, d["desc"], MAX_ENTRIES, R, k, d["split"].reshape(-1), F * R, d["selfw"].reshape(-1), MAX_ENTRIES * k, d["gbuf"]))
        _check_reduce(got[-1], want[-1], (F, k, nv))
    counts = [g[0] for g in got]
    stride = max(counts) + 2

    def gathered(parts, as_bits):
        all_key = np.full(3 * stride, SENT, dtype=U32)
        all_rows = np.full((3 * stride, R), np.nan, dtype=F32)
        for r, (cnt, key, rows) in enumerate(parts):
            all_key[r * stride:r * stride + cnt] = key
            all_rows[r * stride:r * stride + cnt] = rows.view(F32) if as_bits else rows
        return all_key, all_rows

    w0, acc0, lut = _tables(table, 13)
    ref_key, ref_rows = gathered(want, False)
    want_w, want_acc = sr.apply_ffm_ref(ref_key, ref_rows, counts, stride, R, w0, acc0, sr.OPT_ADAGRAD_LUT, RATE, -0.5, lut)
    all_key, all_rows = gathered(got, True)
    c = dict(all_key=all_key, all_rows=all_rows, counts=counts, stride=stride, table=table)
    got_w, got_acc = _gpu_apply(c, 3, R, k % 4 == 0, w0, acc0, sr.OPT_ADAGRAD_LUT, -0.5, lut)
    _same_bits(got_acc, want_acc, ("acc", F, k))
    _same_bits(got_w, want_w, ("w", F, k))
    assert not np.array_equal(got_w, _bits(w0))


def test_debug_entry_points_refuse_bad_shapes():
    L = capi.lib()
    t = _dev(np.zeros(64, dtype=F32))
    p, cnt = t.data_ptr(), C.c_uint32(0)
    bad_reduce = [dict(k=0), dict(R=10, k=4), dict(keys=None), dict(bk_rows=None), dict(split=None)]
    for over in bad_reduce:
        a = dict(keys=p, R=8, k=2, split=p, bk_rows=p)
        a.update(over)
        rc = L.fwgpu_debug_sparse_reduce(a["keys"], 0, 47, p, 4, a["R"], a["k"], a["split"], 8, p, 8, p, p, a["bk_rows"], C.byref(cnt), _stream())
        assert rc == capi.ERR_INVALID, over
    for over in (dict(R=10, k4=1), dict(w=None), dict(lut=None), dict(acc=None)):
        a = dict(R=8, k4=0, w=p, lut=p, acc=p)
        a.update(over)
        rc = L.fwgpu_debug_sparse_apply(p, p, p, 1, 0, 47, a["R"], a["k4"], a["w"], a["acc"], sr.OPT_SGD, 0.1, 0.0, a["lut"], _stream())
        assert rc == capi.ERR_INVALID, over
