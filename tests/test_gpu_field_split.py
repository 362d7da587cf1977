"""The config-C learn kernel with ranges that end INSIDE a field (fwumious_wabbit_amd/csrc/wave_balance.h split_cut, kernels.hip FW_SPLIT_FIELDS): the wave
that holds a cut field's first part flushes its partial sum, the wave behind it takes the sum up in a second pass of the gather and adds its lead rows.
The rule itself is checked on the CPU (test_field_split_cpu.py); here the kernel that uses it is held, as test_gpu_wave_balance.py holds its parent, to

  1. the CPU oracle and the entry route, in order;
  2. the in-order launch, bit for bit, when 1024 such examples that share nothing run concurrently (store policies 1 and 4).

Streams (F = 30, k = 8, the chained float-granular update path forced, 512 threads = 8 waves: the instantiation with rows kept from the gather):
  config_c         30 fields of 1 + Poisson(5.67) features, ~200 rows: nearly every cut lies inside a field; example 0 is built so that wave 1's lead is
                   exactly FW_SPLIT_LEAD_MAX rows
  big_field_mixed  test_gpu_wave_balance's one_big_field (89 rows: below the 128 from which the rule applies, so the parent's ranges) alternating
                   with [60] + [5] * 29 (205 rows: cuts that fall back AND cuts that split in one example)
  one_big_field    the lopsided shape itself

What would turn which case red: a lead row added twice or never, or in front of the first part -- the cut field's row of T, hence the predictions and every
row stepped with it, differs from the oracle's (a sum in another order differs from the entry route's bits only if the two routes cut differently: they
do not, so the order is held by the oracle's tolerance and by the CPU test's statement of the rule); a partial self-pair term lost or summed over the
lanes too early -- the prediction; a lead row's own slot not written -- its step; a wave that misses the second barrier -- a hang."""
import numpy as np
import pytest

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import _capi as capi
from helpers import DisjointStream, check_disjoint, disjoint_models, record_labels

import test_gpu_concurrent_exact as ce
import test_gpu_wave_balance as wb
from test_field_split_cpu import LEAD_MAX, MIN_ROWS, _bounds, _py_cut

pytestmark = pytest.mark.gpu

LUT = fw.Optimizer.AdagradLUT
F, K, NW = wb.F, wb.K, wb.NW
LEAD_8 = [25 - 3, 3 + LEAD_MAX] + [25] * 6 + [17] + [0] * 21  # 200 rows; row 25 is 3 rows into a field of 11

_STREAMS = {}


def _counts(shape, n):
    if shape == "config_c":
        rng = np.random.default_rng(20240612)
        return [LEAD_8] + [list(int(c) for c in 1 + rng.poisson(5.67, size=F)) for _ in range(n - 1)]
    if shape == "big_field_mixed":
        return [wb.BIG if e % 2 == 0 else [60] + [5] * 29 for e in range(n)]
    raise KeyError(shape)


def split_stream(shape, n, p_weighted=0.2, seed=11):
    """test_gpu_wave_balance.lopsided_stream with the per-field entry counts given per EXAMPLE: n examples that share no FFM row, no 128-byte line and no
    LR entry; row i of the batch starts at float i * S + 8 * (i % 4).  The bookkeeping is DisjointStream's."""
    if shape == "one_big_field":
        return wb.lopsided_stream(n=n, **wb.SHAPES[shape]), [wb.BIG] * n
    key = (shape, n, p_weighted, seed)
    if key in _STREAMS:
        return _STREAMS[key]
    counts = _counts(shape, n)
    rng = np.random.default_rng(seed)
    R = F * K
    S = ((R + 64 + 31) // 32) * 32
    ex, hsh, fld, val = [], [], [], []
    recs, off = [], [0]
    vals = np.array([0.5, 2.0, 0.75, 1.5], dtype=np.float32)
    grid = 0
    for e in range(n):
        rec = [0, int(rng.integers(0, 2)), int(np.float32(1.0 if rng.random() < 0.7 else 0.5).view(np.uint32))] + [wb.NO_FEATURES] * F
        for ns, c in enumerate(counts[e]):
            slot = []
            for _ in range(c):
                v = float(vals[rng.integers(0, 4)]) if rng.random() < p_weighted else 1.0
                slot.append((grid * S + 8 * (grid % 4), v))
                grid += 1
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
    st.row_hash, st.row_ex = st.hash.copy(), st.ex.copy()
    st.row_count, st.row_ffm = np.ones(len(hsh), dtype=np.int64), np.ones(len(hsh), dtype=bool)
    st.span = grid * S
    st.ffm_bits = max(10, int(np.ceil(np.log2(st.span))))
    st.bits = st.ffm_bits
    assert st.ffm_bits <= 27
    st.labels = record_labels(st.recs, st.off)
    st.fbs = None
    mi, _, _ = disjoint_models(st, LUT)
    check_disjoint(st, mi)  # (also: the translator's entries are this bookkeeping; fills st.fbs)
    _STREAMS[key] = (st, counts)
    return st, counts


def _leads(sizes):
    """the lead of every wave's range under the rule (0: the range starts on a field boundary), and whether any cut fell back"""
    nf = int(sum(sizes))
    if nf < MIN_ROWS:
        return [0] * NW, False
    bounds = sorted(set(int(b) for b in _bounds(sizes)))
    leads, back = [0], False
    for v in range(1, NW):
        c, fell = _py_cut(sizes, v, nf, LEAD_MAX)
        back |= fell
        leads.append(0 if c in bounds else min(b for b in bounds if b > c) - c)
    return leads, back


def test_the_streams_are_fit_for_the_check():
    """asserted on the host from the rule (no launch): what the cases below rest on"""
    leads = [_leads(s)[0] for s in _counts("config_c", 64)]
    assert sum(1 for l in leads if any(l)) >= 32, "fewer than half of the examples have a split"
    assert any(LEAD_MAX in l for l in leads), "no wave has a lead of exactly the most rows"
    assert leads[0][1] == LEAD_MAX
    mixed = [_leads(s) for s in _counts("big_field_mixed", 2)]
    assert mixed[0] == ([0] * NW, False)         # the lopsided shape: too short for the rule, the parent's ranges
    assert mixed[1][1] and any(mixed[1][0])      # ... and its neighbour: cuts that fall back and cuts that split in one example


@pytest.mark.parametrize("shape", ["config_c", "big_field_mixed", "one_big_field"])
def test_in_order_parity(shape):
    st, _ = split_stream(shape, 64)
    mi, ocfg, ots = disjoint_models(st, LUT)
    setup = ce._setup(whole=3)
    re_r, p_r = wb._learn_in_order(mi, st, "records", setup)
    re_e, p_e = wb._learn_in_order(mi, st, "entries", setup)
    try:
        ce._anchor(st, ocfg, ots, re_r, p_r)
        assert np.array_equal(p_r.view(np.uint32), p_e.view(np.uint32)), "predictions differ between the record and the entry route"
        for t in ce.TABLES:
            assert re_r.table_checksum(t) == re_e.table_checksum(t), ce._first_diff(st, re_r, re_e, t)
    finally:
        re_r.close(), re_e.close()


@pytest.mark.parametrize("policy", [1, 4])
@pytest.mark.parametrize("shape", ["config_c", "big_field_mixed", "one_big_field"])
def test_concurrent_equals_in_order(shape, policy):
    """fresh accumulators: no row is hot, so policy 4 thins nothing and must be bit-equal too"""
    st, _ = split_stream(shape, 1024)
    mi, _, _ = disjoint_models(st, LUT)
    for route in ("records", "entries"):
        ce._modes_agree(mi, st, ce._setup(whole=3, policy=policy), route)
