"""The config-C learn kernel's hand-out of an example's rows to its eight waves (fwumious_wabbit_amd/csrc/wave_balance.h: a range ends on the field
boundary nearest to w nf / 8), on examples built to be lopsided: one field of 60 features, all features in the last field, fewer features than waves,
empty fields, ranges of exactly 23 and 24 rows (a wave keeps 20 + 3 rows from the gather and re-reads the rest in the update).  The rule itself is
checked on the CPU (test_wave_balance_cpu.py); here the kernel that uses it is held to

  1. the CPU oracle and the entry route, in order, on every shape;
  2. the in-order launch, bit for bit, when 1024 such examples that share nothing run concurrently (store policies 1 and 4);
  3. the thinned adds of store policy 4 on hot rows, 37 of an example's 89 rows being re-read ones.

F = 30, k = 8 with the chained float-granular update path forced (set_whole_line_updates(3)), as test_gpu_concurrent_exact.py's A_STREAM cases: the launch
is the fused example kernel on rows of 240 floats, i.e. the instantiation with rows kept from the gather.

What would turn which case red: a field owned by two waves or by none (its rows stepped twice, or never gathered) -- T, hence the predictions, and
FFM_W / FFM_ACC differ from the oracle's; a range that is not one interval -- rows between its fields are gathered by two waves; a chain walked twice or
not at all -- `dups_in_big_field`; a thinning draw of a re-read row that is not the function of (example, row index) that update_rows_win states --
test_hot_reread_rows_default_sampling names the rows whose turn must come from that formula on the CPU."""
import numpy as np
import pytest

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import _capi as capi
from helpers import DisjointStream, check_disjoint, disjoint_models, record_labels

import test_gpu_concurrent_exact as ce

pytestmark = pytest.mark.gpu

LUT = fw.Optimizer.AdagradLUT
F, K, NW, KEPT = 30, 8, 8, 23
NO_FEATURES = 0x80000000
BIG = [60] + [1] * 29

# per-field feature counts (entries, duplicates included)
SHAPES = {
    "one_big_field": dict(counts=BIG),                                   # (i) one wave owns 23 + 37 rows, the others under 23
    "all_in_last_field": dict(counts=[0] * 29 + [40]),                   # (ii)
    "five_features": dict(counts=[1 if f in (0, 6, 12, 18, 29) else 0 for f in range(F)]),  # (iii) fewer features than waves
    "ten_empty_fields": dict(counts=[7] * 10 + [0] * 10 + [7] * 10),     # (iv)
    "one_thirteen": dict(counts=[1, 13] * 15),                           # (v)
    "rows_23": dict(counts=[23, 0, 0] * 8 + [0] * 6),                    # (vi) exactly 23 rows in every wave's range: nothing re-read
    "rows_24": dict(counts=[24, 0, 0] * 8 + [0] * 6),                    # ... and exactly 24: one re-read row each
    "dups_in_big_field": dict(counts=BIG, p_dup=0.1),                    # (vii) chain owners in kept slots and among the re-read rows
    "overlap_in_big_field": dict(counts=BIG, overlap=(30, 45)),          # (viii) entry 45 of the big field starts 8 floats behind entry 30's row: phase B
}

_STREAMS = {}


def lopsided_stream(counts, n, p_dup=0.0, overlap=None, p_weighted=0.2, seed=5):
    """helpers.disjoint_stream with the per-field entry counts given (0 = an empty namespace): n examples that share no FFM row, no 128-byte line and
    no LR entry; row i of the batch starts at float i * S + 8 * (i % 4).  `p_dup`: that share of the entries of field 0 repeat the feature in front
    of them (a chained duplicate row).  `overlap` = (a, b): entry b of field 0 is a feature of its own whose row starts 8 floats behind entry a's -- two
    rows of different hashes that overlap.  The bookkeeping is DisjointStream's."""
    key = (tuple(counts), n, p_dup, overlap, p_weighted, seed)
    if key in _STREAMS:
        return _STREAMS[key]
    rng = np.random.default_rng(seed)
    R = F * K
    S = ((R + 64 + 31) // 32) * 32
    ex, hsh, fld, val = [], [], [], []
    row_hash, row_ex, row_count, row_ffm = [], [], [], []
    recs, off = [], [0]
    vals = np.array([0.5, 2.0, 0.75, 1.5], dtype=np.float32)
    grid = 0
    for e in range(n):
        rec = [0, int(rng.integers(0, 2)), int(np.float32(1.0 if rng.random() < 0.7 else 0.5).view(np.uint32))] + [NO_FEATURES] * F
        for ns, c in enumerate(counts):
            slot = []
            while len(slot) < c:
                v = float(vals[rng.integers(0, 4)]) if rng.random() < p_weighted else 1.0
                j = len(slot)
                if ns == 0 and overlap and j == overlap[1]:
                    h = slot[overlap[0]][0] + 8  # (inside its example's stretch of the table: S >= R + 64)
                    row_hash.append(h), row_ex.append(e), row_count.append(1), row_ffm.append(True)
                elif ns == 0 and j > 0 and rng.random() < p_dup:
                    h = slot[-1][0]
                    row_count[-1] += 1
                else:
                    h = grid * S + 8 * (grid % 4)  # (an overlapping row takes no place of the grid)
                    grid += 1
                    row_hash.append(h), row_ex.append(e), row_count.append(1), row_ffm.append(True)
                slot.append((h, v))
            for h, v in slot:
                ex.append(e), hsh.append(h), fld.append(ns), val.append(v)
            if len(slot) == 1 and slot[0][1] == 1.0:
                rec[3 + ns] = slot[0][0]
            elif slot:
                start = len(rec)
                for h, v in slot:
                    rec += [h, int(np.float32(v).view(np.uint32))]
                assert start <= 0x3fff and len(rec) <= 0xffff
                rec[3 + ns] = 0x80000000 | (start << 16) | len(rec)
        rec[0] = len(rec)
        recs += rec
        off.append(len(recs))
    st = DisjointStream()
    st.F, st.k, st.n, st.R, st.S, st.n_ns, st.lr_only_ns = F, K, n, R, S, F, 0
    st.recs, st.off = np.array(recs, dtype=np.uint32), np.array(off, dtype=np.uint64)
    st.ex, st.hash, st.fld, st.val = np.array(ex), np.array(hsh, dtype=np.int64), np.array(fld), np.array(val, dtype=np.float32)
    st.row_hash, st.row_ex = np.array(row_hash, dtype=np.int64), np.array(row_ex)
    st.row_count, st.row_ffm = np.array(row_count), np.array(row_ffm, dtype=bool)
    st.span = grid * S
    st.ffm_bits = max(10, int(np.ceil(np.log2(st.span))))
    st.bits = st.ffm_bits
    assert st.ffm_bits <= 27
    st.labels = record_labels(st.recs, st.off)
    st.fbs = None
    mi, _, _ = disjoint_models(st, LUT)
    check_disjoint(st, mi)  # (also: the translator's entries are this bookkeeping; fills st.fbs)
    _STREAMS[key] = st
    return st


def _learn_in_order(mi, st, route, setup):
    re = fw.Regressor(mi)
    setup(re)
    p = ce._learn(re, mi, st, route, capi.MODE_SEQUENTIAL)
    assert re.last_route() == capi.ROUTE_FUSED  # (the fused example kernel; rows of 240 floats on the forced chained path: the kept-row instantiation)
    return re, p


# ------------------------------------------------------------------ 1. in order: the oracle, and the entry route
@pytest.mark.parametrize("shape", list(SHAPES))
def test_in_order_parity_on_lopsided_examples(shape):
    st = lopsided_stream(n=64, **SHAPES[shape])
    mi, ocfg, ots = disjoint_models(st, LUT)
    setup = ce._setup(whole=3)
    re_r, p_r = _learn_in_order(mi, st, "records", setup)
    re_e, p_e = _learn_in_order(mi, st, "entries", setup)
    try:
        ce._anchor(st, ocfg, ots, re_r, p_r)
        assert np.array_equal(p_r.view(np.uint32), p_e.view(np.uint32)), "predictions differ between the record and the entry route"
        for t in ce.TABLES:
            assert re_r.table_checksum(t) == re_e.table_checksum(t), ce._first_diff(st, re_r, re_e, t)
    finally:
        re_r.close(), re_e.close()


# ------------------------------------------------------------------ 2. concurrent = in order on examples that share nothing
@pytest.mark.parametrize("policy", [1, 4])
@pytest.mark.parametrize("shape", ["one_big_field", "one_thirteen", "dups_in_big_field"])
def test_concurrent_equals_in_order(shape, policy):
    """fresh accumulators: no row is hot, so policy 4 thins nothing and must be bit-equal too"""
    st = lopsided_stream(n=1024, **SHAPES[shape])
    mi, _, _ = disjoint_models(st, LUT)
    check_disjoint(st, mi)
    for route in ("records", "entries"):
        ce._modes_agree(mi, st, ce._setup(whole=3, policy=policy), route)


# ------------------------------------------------------------------ 3. hot re-read rows under store policy 4
HOT_KEY = "wave_balance_one_big_field"


def _hot(sample_log2):
    """test_gpu_concurrent_exact._Hot on shape (i): every third row hot, 37 of an example's 89 rows re-read.  (_Hot draws its stream from that module's cache by
    its parameters: the lopsided stream is put there under a key of its own.)"""
    st = lopsided_stream(n=1024, **SHAPES["one_big_field"])
    ce.HOT_STREAMS[HOT_KEY] = dict(wave_balance_shape="one_big_field")
    ce._STREAMS[tuple(sorted(ce.HOT_STREAMS[HOT_KEY].items()))] = st
    return ce._Hot(HOT_KEY, LUT, policy=4, sample_log2=sample_log2, whole=3), st


def _reread(st):
    """per row of shape (i): is it re-read?  The big field's 60 rows are one wave's range: its first 23 are kept, rows 23..59 of every example are re-read."""
    return (np.arange(len(st.row_hash)) % 89 >= KEPT) & (np.arange(len(st.row_hash)) % 89 < 60)


def test_hot_reread_rows_one_example_in_one():
    """sample_log2 = 0: every hot row's add lands, with factor 1 -- test_hot_rows_one_example_in_one's assertions, on the lopsided shape"""
    hr, st = _hot(0)
    hr.check_cold_and_gaps()
    assert hr.same_lr, "LR table differs"
    a0, s, h = hr.hot_rows()
    assert np.all((s > a0).any(axis=1)), "the in-order launch must have grown every hot row"
    c = st.row_count[hr.hot][:, None]
    err = np.abs(h - s) / ce._ulps(s)
    print(f"\n{len(s)} hot rows ({int(_reread(st)[hr.hot].sum())} of them re-read), max |concurrent - in-order| = {err.max():.2f} ulps (allowed: 1 per occurrence)")
    bad = np.argwhere(err > c)
    assert not len(bad), (f"{len(bad)} hot accumulators off by more than one ulp per occurrence; first: hot row {int(bad[0][0])} (row {int(np.flatnonzero(hr.hot)[bad[0][0]]) % 89} of its example), "
                          f"float {int(bad[0][1])}: in-order {s[tuple(bad[0])]!r}, concurrent {h[tuple(bad[0])]!r}")


def test_hot_reread_rows_default_sampling():
    """one example in eight: every hot row shows nothing or 8 x the in-order delta (within 8 ulps, as test_hot_rows_default_sampling), and the share of rows
    whose turn came lies in that test's 9-16 % -- over all hot rows and over the re-read ones, whose draw is a function of (example, row index) alone: the same
    share is computed on the CPU from update_rows_win's formula first, and the rows whose turn came must be the ones it names."""
    st = lopsided_stream(n=1024, **SHAPES["one_big_field"])
    rows = np.arange(len(st.row_hash))
    hot, rr = rows % 3 == 0, _reread(st)
    e, i = (rows // 89).astype(np.uint64), (rows % 89).astype(np.uint64)
    draw = ((((e * 2654435761) & 0xffffffff) ^ ((i * 40503) & 0xffffffff)) >> 9)  # single-chunk rows: c = 0
    turn_cpu = (draw & 7) == 0
    share_cpu = float(turn_cpu[hot & rr].mean())
    assert 0.09 <= share_cpu <= 0.16, share_cpu  # (the stream is fit for the check)
    hr, _ = _hot(-1)
    hr.check_cold_and_gaps()
    a0, s, h = hr.hot_rows()
    d, r = s - a0, h - a0
    zero, full = (r == 0.0).all(axis=1), (np.abs(r - 8.0 * d) <= 8.0 * ce._ulps(s)).all(axis=1)
    live = (d > 0).any(axis=1)
    bad = np.flatnonzero(live & ~(zero | full))
    assert not len(bad), f"{len(bad)} hot rows are neither untouched nor 8 x the in-order delta; first: row {int(np.flatnonzero(hot)[bad[0]]) % 89} of example {int(np.flatnonzero(hot)[bad[0]]) // 89}"
    took = full & ~zero
    rr_hot = rr[hot]
    share_all, share_rr = float(took[live].mean()), float(took[live & rr_hot].mean())
    print(f"\n{int(live.sum())} hot rows, turn came for {share_all:.4f}; {int((live & rr_hot).sum())} re-read ones: {share_rr:.4f} (from the draw formula: {share_cpu:.4f})")
    assert 0.09 <= share_all <= 0.16 and 0.09 <= share_rr <= 0.16, (share_all, share_rr)
    # ... and they are the rows the formula names
    assert np.array_equal(took[live & rr_hot], turn_cpu[hot][live & rr_hot]), "the re-read rows whose turn came are not the ones update_rows_win's draw names"
