"""Concurrent (MODE_HOGWILD, many workgroups) launches, checked per float.

If no two examples of a batch share an FFM row, a 128-byte line of a row or an LR entry, the order of the examples cannot matter: a concurrent
launch must leave exactly what the in-order launch leaves, and the in-order launch is pinned to the oracle elsewhere (test_gpu_parity.py) and, on
this kind of stream, by the anchors below.  helpers.disjoint_stream builds such batches and helpers.check_disjoint ASSERTS the condition on the host
translator's output; the models have no constant feature (its LR entry is the one thing every example would share).

What would turn which case red (the code paths exist only when p.concurrent / p.grid_wgs > 1, or at launch shapes an in-order launch never takes):
  * a coalesced add (store policy 4: the adds behind the pipelined update loop) shifted by one float: the gradients differ per float here, so every hot kept row of
    test_hot_rows_one_example_in_one is off by far more than its one ulp per occurrence;
  * the second chunk's add dropped: the floats from 256 on of the hot rows of test_hot_rows_one_example_in_one[c_k16 / c_f40] keep their preset
    value where the in-order launch grew them; under the default sampling the unit shows 0 where its share of turns must be 1/8;
  * a parked row written back from the wrong LDS slot: the weights of that row become another row's w - step -- the FFM_W checksum of every
    test_config_c_kernel case with parked rows (lds_keep -1 or 3) differs, and _first_diff names the (example, feature, float);
  * the 128-thread shape reading the neighbouring wave's range: rows of the other wave's share are stepped twice or not at all --
    predictions and FFM_W of test_small_example_shape[ffm32 / lr64] differ from the in-order launch's.
"""
import numpy as np
import pytest

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import _capi as capi
from helpers import check_disjoint, disjoint_models, disjoint_stream, logloss
from oracle import fwo

pytestmark = pytest.mark.gpu

LOGLOSS_TOL = 1e-4  # as helpers._stream_parity
LUT, FLEX, SGD = fw.Optimizer.AdagradLUT, fw.Optimizer.AdagradFlex, fw.Optimizer.SGD
TABLES = (capi.TABLE_LR, capi.TABLE_FFM_W, capi.TABLE_FFM_ACC)
_NAMES = {capi.TABLE_LR: "LR", capi.TABLE_FFM_W: "FFM_W", capi.TABLE_FFM_ACC: "FFM_ACC", capi.TABLE_NN_W: "NN_W"}

_STREAMS = {}


def _stream(**kw):
    """one generated stream per parameter set, shared by the cases that use it and left unchanged"""
    key = tuple(sorted(kw.items()))
    if key not in _STREAMS:
        st = disjoint_stream(**kw)
        mi, _, _ = disjoint_models(st, LUT)
        check_disjoint(st, mi)  # (a test on a stream that fails this proves nothing)
        _STREAMS[key] = st
    return _STREAMS[key]


def _learn(re, mi, st, route, mode):
    fbt = fw.FeatureBufferTranslator(mi)
    b = re.record_batch(fbt, st.recs, st.off) if route == "records" else re.batch(st.fbs)
    re.learn_batch(b, mode, True)
    p = b.predictions().copy()
    b.close()
    return p


def _first_diff(st, re_a, re_b, which):
    """diagnostics only: the first float of the touched span on which the two regressors differ, as (example, feature, float of the row)"""
    mult = 2 if which == capi.TABLE_LR else 1
    count = min(st.span * mult, re_a.table_len(which))
    a, b = re_a.table_read(which, 0, count).view(np.uint32), re_b.table_read(which, 0, count).view(np.uint32)
    bad = np.flatnonzero(a != b)
    if not len(bad):
        return f"{_NAMES[which]}: no difference inside the touched span ({count} floats): a write OUTSIDE every row"
    i = int(bad[0]) // mult
    row = int(np.searchsorted(st.row_hash, i, side="right")) - 1
    return (f"{_NAMES[which]}: {len(bad)} floats differ, first at table float {int(bad[0])}: example {int(st.row_ex[row])}, feature (row) {row} "
            f"starting at {int(st.row_hash[row])} ({int(st.row_hash[row]) * 4 % 128} B into a line, {int(st.row_count[row])} occurrence(s)), "
            f"float {i - int(st.row_hash[row])} of the row: in-order {a[bad[0]:bad[0] + 1].view(np.float32)[0]!r}, concurrent {b[bad[0]:bad[0] + 1].view(np.float32)[0]!r}")


def _modes_agree(mi, st, setup, route, tables=TABLES, keep=False, setup_seq=None):
    """Two regressors with identical setup(re); one learns the batch with MODE_SEQUENTIAL, the other with MODE_HOGWILD: bit-equal predictions,
    equal checksums of `tables`, and the weights did move.  Returns (re_seq, re_hog, p_seq) with keep=True (the caller closes them).
    (`setup_seq`: applied to the in-order regressor after setup -- only to make it take the launch shape the concurrent one takes by itself.)"""
    if st.fbs is None:
        check_disjoint(st, mi)
    res = []
    for mode in (capi.MODE_SEQUENTIAL, capi.MODE_HOGWILD):
        re = fw.Regressor(mi)
        setup(re)
        if setup_seq is not None and mode == capi.MODE_SEQUENTIAL:
            setup_seq(re)
        moved = capi.TABLE_FFM_W if st.k else capi.TABLE_LR
        before = re.table_checksum(moved)
        p = _learn(re, mi, st, route, mode)
        assert np.all(np.isfinite(p))
        assert re.table_checksum(moved) != before, "the batch did not step the weights"
        res.append((re, p))
    (re_s, p_s), (re_h, p_h) = res
    try:
        if not np.array_equal(p_s, p_h):
            e = int(np.flatnonzero(p_s != p_h)[0])
            raise AssertionError(f"{int((p_s != p_h).sum())} predictions differ, first at example {e}: in-order {p_s[e]!r}, concurrent {p_h[e]!r}")
        for t in tables:
            if re_s.table_checksum(t) != re_h.table_checksum(t):
                raise AssertionError(_first_diff(st, re_s, re_h, t) if t in TABLES else f"{_NAMES[t]} differs")
    except AssertionError:
        re_s.close(), re_h.close()
        raise
    if keep:
        return re_s, re_h, p_s
    re_s.close(), re_h.close()


def _anchor(st, ocfg, ots, re_s, p_s, weight_tol=2e-5, om=None, acc0=None, lr0=None):
    """the in-order result IS the reference's single thread on this kind of stream too: _stream_parity's tolerances, on the touched span"""
    om = om if om is not None else fwo.Model(ocfg)
    if acc0 is not None:
        om.ffm_acc[:len(acc0)] = acc0
    if lr0 is not None:
        om.lr_table[:len(lr0)] = lr0
    _, p_ref = om.run_stream(ots, st.recs, st.off, holdout_after=0, nthreads=1)
    d_ll = np.abs(logloss(p_s, st.labels) - logloss(p_ref, st.labels))
    assert d_ll.max() < LOGLOSS_TOL, (d_ll.max(), d_ll.argmax())

    def close(a, b):
        return bool(np.all(np.abs(a - b) <= weight_tol + 1e-5 * np.abs(b)))

    assert close(re_s.table_read(capi.TABLE_LR, 0, 2 * st.span), om.lr_table[:2 * st.span])
    if st.k:
        assert close(re_s.table_read(capi.TABLE_FFM_W, 0, st.span), om.ffm_weights[:st.span])
        assert close(re_s.table_read(capi.TABLE_FFM_ACC, 0, st.span), om.ffm_acc[:st.span])
    om.close()


def _setup(whole=None, policy=None, kept=None, lds_keep=None, prefetch=None, kernel_version=None, head=None, sample_log2=None, threads=None):
    def f(re):
        if threads is not None:
            re.set_launch(threads=threads)
        if whole is not None:
            re.set_whole_line_updates(whole)
        if policy is not None:
            re.set_store_policy(policy)
        if kept is not None:
            re.set_kept_rows(kept)
        if lds_keep is not None:
            re.set_lds_keep(lds_keep)
        if prefetch is not None:
            re.set_prefetch(prefetch)
        if kernel_version is not None:
            capi.check(re.L.fwgpu_debug_set_kernel_version(re.h, kernel_version))
        if head is not None:
            re.set_head_kernel(head)
        if sample_log2 is not None:
            re.set_hot_row_sampling(sample_log2=sample_log2)
    return f


def _run(st, opt, route, anchor=False, **setup):
    kw = dict(init_acc=1.0) if opt == FLEX else (dict(lr=0.05, ffm_lr=0.05) if opt == SGD else {})
    mi, ocfg, ots = disjoint_models(st, opt, **kw)
    re_s, re_h, p_s = _modes_agree(mi, st, _setup(**setup), route, keep=True)
    try:
        if anchor:
            _anchor(st, ocfg, ots, re_s, p_s, weight_tol=5e-5 if opt == FLEX else 2e-5)
    finally:
        re_s.close(), re_h.close()


# ------------------------------------------------------------------ (a) the config-C kernel
A_STREAM = dict(F=30, k=8, n=1024, per_field=(6, 9), p_weighted=0.2, p_dup=0.04, seed=11)  # ~28 rows per wave: kept, parked and re-read slots all used
# (whole-line mode, store policy, kept rows, lds_keep, prefetch, optimizer, route): every value of the issue's list at least once; the shipped default on both routes
A_CASES = {
    "shipped_records": dict(whole=3, opt=LUT, route="records", anchor=True),
    "shipped_entries": dict(whole=3, opt=LUT, route="entries"),
    "lines_pol0_nopark": dict(whole=2, policy=0, lds_keep=0, opt=LUT, route="records"),
    "pol1_flex_park3": dict(whole=3, policy=1, lds_keep=3, opt=FLEX, route="entries"),
    "lines_pol2_sgd_noprefetch": dict(whole=2, policy=2, prefetch=0, opt=SGD, route="records"),
    "pol3_lut": dict(whole=3, policy=3, lds_keep=-1, prefetch=1, opt=LUT, route="records"),
    "lines_pol4_entries": dict(whole=2, policy=4, opt=LUT, route="entries"),
    "pol4_nokept_flex": dict(whole=3, policy=4, kept=0, opt=FLEX, route="records"),
    "lines_pol3_flex_nopark": dict(whole=2, policy=3, lds_keep=0, opt=FLEX, route="records"),
    "pol0_sgd_entries": dict(whole=3, policy=0, opt=SGD, route="entries"),
    "lines_pol4_nokept_sgd": dict(whole=2, policy=4, kept=0, opt=SGD, route="records"),
    "pol2_park3_noprefetch": dict(whole=3, policy=2, lds_keep=3, prefetch=0, opt=LUT, route="records"),
    "default_policy_explicit": dict(whole=3, policy=-1, lds_keep=-1, opt=LUT, route="records"),
}


@pytest.mark.parametrize("case", list(A_CASES))
def test_config_c_kernel(case):
    """F = 30, k = 8, 6-9 features per field: the large-table kernel with rows kept in registers, parked in LDS and re-read, chained duplicates,
    all four start phases of a line -- every store policy, both access granularities, three optimizers, both routes.  (Fresh accumulators: no row
    is hot, so policies 3 / 4 must be bit-equal too; hot rows: below.)"""
    c = dict(A_CASES[case])
    _run(_stream(**A_STREAM), c.pop("opt"), c.pop("route"), **c)


# ------------------------------------------------------------------ (b) the 128-thread small-example shape
# plan_launch (launch.cpp) takes the 128-thread, two-waves-per-example launch when max_ffm <= 32 && max_lr <= 64 (both rounded up to a multiple of 4):
B_CASES = {
    "ffm32": dict(first_ffm=32),  # 32 FFM features in the largest example: the 128-thread launch
    "ffm33": dict(first_ffm=33),  # 33 (-> 36): the 512-thread launch
    "lr64": dict(lr_only_ns=1, first_lr=64),  # 64 LR entries: the 128-thread launch
    "lr65": dict(lr_only_ns=1, first_lr=65),  # 65 (-> 68): the 512-thread launch
}


@pytest.mark.parametrize("route", ["records", "entries"])
@pytest.mark.parametrize("case", list(B_CASES))
def test_small_example_shape(case, route):
    """F = 10, k = 4, one feature per field (config B): on both sides of each of the two limits of the small-example shape, so that whichever side
    the launch takes, an in-order launch (always >= 512 threads) is compared with it."""
    st = _stream(F=10, k=4, n=4096, seed=21, **B_CASES[case])
    _run(st, LUT, route, anchor=(case == "ffm32" and route == "records"))


# ------------------------------------------------------------------ (c) two-chunk rows
C_STREAMS = {"k16": dict(F=30, k=16, n=256, per_field=(1, 3), p_weighted=0.2, p_dup=0.1, seed=31),
             "f40": dict(F=40, k=8, n=256, per_field=(1, 3), p_weighted=0.2, p_dup=0.1, seed=32)}  # R = 320: a partly filled second chunk


@pytest.mark.parametrize("route", ["records", "entries"])
@pytest.mark.parametrize("policy", [-1, 3, 4])
@pytest.mark.parametrize("shape", list(C_STREAMS))
def test_two_chunk_rows(shape, policy, route):
    """R = 480 and R = 320 on the two-chunk instantiation: concurrent launches keep no LDS copy of the entries' own slots (no_selfw), read the
    AdaGrad table through L1 where that lets a second workgroup in (lut_global), and thin re-read rows under policy 3."""
    _run(_stream(**C_STREAMS[shape]), LUT, route, anchor=(shape == "k16" and policy == -1 and route == "records"), whole=2 if policy == 3 else 3, policy=policy)


# ------------------------------------------------------------------ (d) the generic kernel
D_CASES = {
    "k10_scalar": (dict(F=3, k=10, n=512, per_field=(1, 3), p_weighted=0.2, p_dup=0.1, seed=41), {}),
    "k8_forced_generic": (dict(F=30, k=8, n=512, per_field=(1, 3), p_weighted=0.2, p_dup=0.1, seed=42), dict(kernel_version=1)),
    "k16_f40_1024_threads": (dict(F=40, k=16, n=512, per_field=(1, 2), p_weighted=0.2, p_dup=0.1, seed=43), {}),  # R = 640: no v2 instantiation, one 1024-thread workgroup per CU
}


@pytest.mark.parametrize("case", list(D_CASES))
def test_generic_kernel(case):
    skw, setup = D_CASES[case]
    _run(_stream(**skw), LUT, "records", anchor=(case == "k10_scalar"), **setup)
    _run(_stream(**skw), LUT, "entries", **setup)


# ------------------------------------------------------------------ (e) LR only
def test_lr_only():
    st = _stream(F=8, k=0, n=4096, per_field=(1, 2), p_weighted=0.2, p_dup=0.1, seed=51)
    _run(st, LUT, "records", anchor=True)
    _run(st, LUT, "entries")


# ------------------------------------------------------------------ (f) the deep head under real concurrency
F_CASES = {
    # the concurrent default: the head as a phase of the two-chunk kernel (nn_v2), which an in-order launch takes only when forced (option 11 = 2)
    "k16_nn_v2": (dict(F=30, k=16, n=512, per_field=(1, 2), p_weighted=0.2, p_dup=0.1, seed=61), [(256, "relu", "hu"), (256, "relu", "hu")], dict(whole=3)),
    # the generic kernel: concurrently one 1024-thread workgroup per CU, so the in-order launch is given 1024 threads too
    "k16_generic_head": (dict(F=30, k=16, n=512, per_field=(1, 2), p_weighted=0.2, p_dup=0.1, seed=61), [(256, "relu", "hu"), (256, "relu", "hu")], dict(whole=3, head=0, threads=1024)),
    "small_head_generic": (dict(F=6, k=4, n=1024, per_field=(1, 2), p_weighted=0.2, p_dup=0.1, seed=62), [(12, "relu", "hu"), (8, "relu", "hu")], {}),
}


@pytest.mark.parametrize("case", list(F_CASES))
def test_deep_head_with_frozen_dense_weights(case):
    """The dense weights are shared by every example, so they are frozen (nn_learning_rate = 0: test_disjoint_stream_cpu pins that a zero rate leaves them
    bit-identical on the oracle); everything sparse is then order-independent again.  NN_ACC is not compared: its f32 sums depend on the order.
    The in-order launch (by itself the 512-thread generic kernel) is put on the launch shape of the concurrent one, since the head's sums depend on it.
    These cases found that the layer backward added its thread groups' input gradients with LDS float atomics, in the order the groups arrived, and took
    that form in concurrent launches only: with the 2 x 256 heads the predictions were equal but ~37 000 of the ~46 000 touched LR floats were one ulp
    off (first: -0.046730805 in order, -0.046730794 concurrently), another count in every run.  The groups now add in a fixed order, in every updating launch."""
    skw, layers, setup = F_CASES[case]
    st = _stream(**skw)
    mi, ocfg, ots = disjoint_models(st, LUT)
    mi.nn_layers = [dict(width=w, activation=a, init=i) for w, a, i in layers]
    mi.nn_topology, mi.nn_learning_rate, mi.nn_power_t, mi.nn_init_acc_gradient = "one", 0.0, 0.45, 0.0
    om = fwo.Model(ocfg, nn=fwo.make_nn_config(layers, "one", 0.0, 0.45, 0.0))
    w0 = np.concatenate([om.nn_weights(l).copy() for l in range(len(layers) + 1)])
    base = _setup(**setup)

    def setup_re(re):
        base(re)
        assert re.table_len(capi.TABLE_NN_W) == w0.size
        re.table_write(capi.TABLE_NN_W, w0)  # (Hu draws are implementation-defined: the same ones everywhere)

    for route in ("records", "entries"):
        re_s, re_h, p_s = _modes_agree(mi, st, setup_re, route, tables=TABLES + (capi.TABLE_NN_W,), keep=True,
                                       setup_seq=(lambda re: re.set_head_kernel(2)) if case == "k16_nn_v2" else None)
        try:
            assert np.array_equal(re_h.table_read(capi.TABLE_NN_W), w0)
            if route == "records" and case == "k16_nn_v2":
                _anchor(st, ocfg, ots, re_s, p_s, om=om)
                om = None
        finally:
            re_s.close(), re_h.close()
    if om is not None:
        om.close()


# ------------------------------------------------------------------ hot rows, exactly
def _initial_acc(opt, init):
    return float(init) if opt == FLEX else 0.0  # (AdagradLUT folds the initial value into its table: regressor.cpp initial_acc)


HOT_STREAMS = {
    "a": dict(A_STREAM),
    "c_k16": dict(F=30, k=16, n=1024, per_field=(1, 3), p_weighted=0.2, p_dup=0.1, seed=33),  # (n: >= 20 000 hot units)
    "c_f40": dict(F=40, k=8, n=1024, per_field=(1, 3), p_weighted=0.2, p_dup=0.1, seed=34),
}


class _Hot:
    """Both launches of one hot-row case: every third feature's accumulator row preset to init + 1.5 (hot: the threshold is init + 0.5), every
    fifth feature's LR accumulator to init + 40 (hot: lr_hot_theta = init + 32).  Gradients differ per float (the weights are the random init)."""

    def __init__(self, shape, opt, policy, sample_log2, whole, route="records", anchor=False):
        st = self.st = _stream(**HOT_STREAMS[shape])
        assert st.lr_only_ns == 0 and st.k % 4 == 0
        kw = dict(init_acc=1.0) if opt == FLEX else {}
        mi, ocfg, ots = disjoint_models(st, opt, **kw)
        nrows, S, R = len(st.row_hash), st.S, st.R
        self.nrows, self.whole = nrows, whole
        self.start = (st.row_hash & int(fw.FeatureBufferTranslator(mi).ffm_hash_mask))  # where the translator's mask puts each row
        self.hot = np.arange(nrows) % 3 == 0
        self.lr_hot = np.arange(nrows) % 5 == 0
        a_init, l_init = _initial_acc(opt, mi.ffm_init_acc_gradient), _initial_acc(opt, mi.init_acc_gradient)
        acc0 = np.full(nrows * S, a_init, dtype=np.float32)
        self._rows(acc0)[self.hot] = np.float32(a_init + 1.5)
        probe = fw.Regressor(mi)
        lr0 = probe.table_read(capi.TABLE_LR, 0, 2 * nrows * S)
        probe.close()
        lr0[2 * st.row_hash[self.lr_hot] + 1] = np.float32(l_init + 40.0)
        base = _setup(whole=whole, policy=policy, sample_log2=sample_log2)

        def setup_re(re):
            base(re)
            re.table_write(capi.TABLE_FFM_ACC, acc0)
            re.table_write(capi.TABLE_LR, lr0)

        # predictions and the FFM weights: bit-equal (the step of every example uses the accumulator it read + its own g^2, thinned or not)
        self.re_s, self.re_h, p_s = _modes_agree(mi, st, setup_re, route, tables=(capi.TABLE_FFM_W,), keep=True)
        try:
            if anchor:
                _anchor(st, ocfg, ots, self.re_s, p_s, weight_tol=5e-5 if opt == FLEX else 2e-5, acc0=acc0, lr0=lr0)
            self.acc0, self.lr0 = self._rows(acc0).copy(), lr0
            n = nrows * S
            self.acc_s, self.acc_h = self.re_s.table_read(capi.TABLE_FFM_ACC, 0, n), self.re_h.table_read(capi.TABLE_FFM_ACC, 0, n)
            self.lr_s, self.lr_h = self.re_s.table_read(capi.TABLE_LR, 0, 2 * n), self.re_h.table_read(capi.TABLE_LR, 0, 2 * n)
            self.same_lr = self.re_s.table_checksum(capi.TABLE_LR) == self.re_h.table_checksum(capi.TABLE_LR)
        finally:
            self.re_s.close(), self.re_h.close()

    def _rows(self, table):
        """(rows, R) view-by-copy helper: the R floats of every row of a span-sized table; assignment goes through __setitem__ of RowView"""
        return _RowView(table, self.start, self.st.S, self.st.R)

    def check_cold_and_gaps(self):
        """everything that is not a hot row's accumulator -- cold rows, the floats between the rows -- is bit-equal"""
        s, h = self.acc_s.view(np.uint32).copy(), self.acc_h.view(np.uint32).copy()
        _RowView(s, self.start, self.st.S, self.st.R)[self.hot] = 0
        _RowView(h, self.start, self.st.S, self.st.R)[self.hot] = 0
        bad = np.flatnonzero(s != h)
        assert not len(bad), f"{len(bad)} accumulators outside the hot rows differ, first at table float {int(bad[0])} (row {int(bad[0]) // self.st.S})"
        # LR weights (even floats) always; cold entries' accumulators too
        assert np.array_equal(self.lr_s[0::2].view(np.uint32), self.lr_h[0::2].view(np.uint32)), "LR weights differ"
        sa, ha = self.lr_s[1::2].view(np.uint32).copy(), self.lr_h[1::2].view(np.uint32).copy()
        sa[self.st.row_hash[self.lr_hot]] = 0
        ha[self.st.row_hash[self.lr_hot]] = 0
        assert np.array_equal(sa, ha), "cold LR accumulators differ"

    def hot_rows(self):
        """(acc0, in-order, concurrent) accumulators of the hot rows, (n_hot, R) each, float64"""
        sel = self.hot
        return (self.acc0[sel].astype(np.float64), self._rows(self.acc_s)[sel].astype(np.float64), self._rows(self.acc_h)[sel].astype(np.float64))


class _RowView:
    """rows[i] = table[start[i] : start[i] + R] for every row at once; rows of one start phase (i % 4) are a strided block of the (rows, S) table"""

    def __init__(self, table, start, S, R):
        self.t, self.S, self.R = table, S, R
        n = len(start)
        self.m = table[:n * S].reshape(n, S)
        self.offs = []
        for ph in range(4):
            o = start[ph::4] - np.arange(ph, n, 4) * S
            assert len(o) == 0 or (np.all(o == o[0]) and 0 <= o[0] and o[0] + R <= S)
            self.offs.append(int(o[0]) if len(o) else 0)

    def _gather(self):
        out = np.empty((self.m.shape[0], self.R), dtype=self.t.dtype)
        for ph in range(4):
            out[ph::4] = self.m[ph::4, self.offs[ph]:self.offs[ph] + self.R]
        return out

    def __getitem__(self, sel):
        return self._gather()[sel]

    def copy(self):
        return self._gather()

    def __setitem__(self, sel, value):
        idx = np.flatnonzero(sel)
        for ph in range(4):
            r = idx[idx % 4 == ph]
            self.m[r, self.offs[ph]:self.offs[ph] + self.R] = value


def _ulps(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("shape,opt", [("a", LUT), ("a", FLEX), ("c_k16", LUT), ("c_f40", LUT)], ids=["a-lut", "a-flex", "c_k16-lut", "c_f40-lut"])
def test_hot_rows_one_example_in_one(shape, opt):
    """Store policy 4 with one example in ONE (sample_log2 = 0): every hot row's add happens, with factor 1.  Predictions, FFM weights and the whole
    LR table are bit-equal to in-order (an LR entry's add is acc_new - acc_read, exact, so the sum is the in-order accumulator again); every hot
    accumulator is within c ulps of its in-order value, c = the row's occurrences in its example: the in-order store may fuse acc + g*g, the add
    forms the product separately -- one rounding per occurrence, nothing more.  An add on the wrong float, a dropped tail or second chunk, a
    factor that is wrong for one slot class or one start phase: all are many ulps on rows whose gradients differ per float."""
    hr = _Hot(shape, opt, policy=4, sample_log2=0, whole=3 if shape == "a" else 2, anchor=(shape == "a" and opt == LUT))
    hr.check_cold_and_gaps()
    assert hr.same_lr, "LR table differs"
    a0, s, h = hr.hot_rows()
    assert np.all((s > a0).any(axis=1)), "the in-order launch must have grown every hot row"  # (not every float: a g^2 below half an ulp of 1.5 adds nothing)
    c = hr.st.row_count[hr.hot][:, None]
    err = np.abs(h - s) / _ulps(s)
    print(f"\n{shape}: {len(s)} hot rows, max |concurrent - in-order| = {err.max():.2f} ulps (allowed: occurrences = {int(c.max())} at most)")
    bad = np.argwhere(err > c)
    assert not len(bad), (f"{len(bad)} hot accumulators off by more than one ulp per occurrence; first: hot row {int(bad[0][0])} (feature {int(np.flatnonzero(hr.hot)[bad[0][0]])}), "
                          f"float {int(bad[0][1])}: in-order {s[tuple(bad[0])]!r}, concurrent {h[tuple(bad[0])]!r}, preset {a0[tuple(bad[0])]!r}")


@pytest.mark.parametrize("shape,opt,policy", [("a", LUT, 4), ("a", FLEX, 4), ("a", LUT, 3), ("c_k16", LUT, 4), ("c_k16", LUT, 3), ("c_f40", LUT, 4), ("c_f40", FLEX, 3)],
                         ids=["a-lut-pol4", "a-flex-pol4", "a-lut-pol3", "c_k16-lut-pol4", "c_k16-lut-pol3", "c_f40-lut-pol4", "c_f40-flex-pol3"])
def test_hot_rows_default_sampling(shape, opt, policy):
    """One example in m = 8 (the default).  Predictions, FFM and LR weights, cold accumulators: bit-equal to in-order.  With d the in-order delta, the
    accumulator delta of every hot UNIT is either 0 on every float of the unit (not this example's turn: nobody stores, nobody adds) or 8 d on every
    float, within 8 ulps of the accumulator (d's own rounding, half an ulp, scaled by m, plus the add's) -- a unit that mixes the two or shows
    anything else fails.  A unit is a whole row on the single-chunk kernel (kept, parked and re-read rows alike: one 1 KiB chunk) and each 1 KiB chunk
    of a row on the two-chunk kernel (chunks count from the row's first line in whole-line launches, which these are).  The share of units whose
    turn came must lie in [0.09, 0.16] over >= 20 000 units: a condition against "never" and "always" (test_gpu_conservation holds the mean to 10 %).
    Store policy 3 on the SINGLE-chunk kernel thins register-kept rows only (kernels.hip: a thinned store on a parked or re-read row loses its race
    too often), so there a hot unit may also be exactly the in-order row; at least half of the units (20 of a wave's ~28 rows are kept) must be thinned
    ones.  Hot LR entries: policy 4 -- the same two-valued check; policy 3 does not thin the LR block -- the whole table is bit-equal."""
    hr = _Hot(shape, opt, policy=policy, sample_log2=-1, whole=3 if shape == "a" else 2)
    hr.check_cold_and_gaps()
    st = hr.st
    a0, s, h = hr.hot_rows()
    d, r = s - a0, h - a0
    tol = 8.0 * _ulps(s)
    zero, full, plain = r == 0.0, np.abs(r - 8.0 * d) <= tol, h == s
    if st.R > 256:  # two 1 KiB chunks, counted from the row's first line (whole-line launch): the first one ends 256 floats after the line's start
        phase = (hr.start[hr.hot] % 32)[:, None]
        first = np.arange(st.R)[None, :] < 256 - phase
        units = [first, ~first]
    else:
        units = [np.ones_like(zero)]
    units = [np.broadcast_to(u, zero.shape) for u in units]
    n_units = n_turn = n_plain = 0
    for u in units:
        live = ((d > 0) & u).any(axis=1)  # (a unit on which the in-order launch added nothing says nothing)
        z, f, pl = (zero | ~u).all(axis=1), (full | ~u).all(axis=1), (plain | ~u).all(axis=1)
        ok = z | f | (pl if (policy == 3 and st.R <= 256) else False)
        bad = np.flatnonzero(live & ~ok)
        assert not len(bad), (f"{len(bad)} hot units are neither untouched nor 8 x the in-order delta; first: hot row {int(bad[0])} (feature {int(np.flatnonzero(hr.hot)[bad[0]])}, "
                              f"{int(hr.start[hr.hot][bad[0]]) * 4 % 128} B into a line): floats that are 0: {int((zero & u)[bad[0]].sum())}, 8d: {int((full & u)[bad[0]].sum())} of {int(u[bad[0]].sum())}")
        thinned = live & (z | f)
        n_units += int(thinned.sum())
        n_turn += int((thinned & f & ~z).sum())
        n_plain += int((live & pl & ~z & ~f).sum())
    share = n_turn / max(n_units, 1)
    print(f"\n{shape} policy {policy}: {n_units} thinned hot units, turn came for {share:.4f}; {n_plain} hot units stored plainly")
    assert n_units >= 20000, n_units
    assert policy == 3 and st.R <= 256 or n_plain == 0
    assert n_units >= n_plain, (n_units, n_plain)
    assert 0.09 <= share <= 0.16, share
    # hot LR entries
    if policy == 3:
        assert hr.same_lr, "policy 3 does not thin the LR block: the table must be bit-equal"
    else:
        e = st.row_hash[hr.lr_hot]
        l0, ls, lh = (x[2 * e + 1].astype(np.float64) for x in (hr.lr0, hr.lr_s, hr.lr_h))
        dl, rl = ls - l0, lh - l0
        okl = (rl == 0.0) | (np.abs(rl - 8.0 * dl) <= 8.0 * _ulps(ls))
        assert np.all(okl), f"{int((~okl).sum())} hot LR accumulators are neither untouched nor 8 x the in-order delta, first: feature {int(np.flatnonzero(hr.lr_hot)[np.flatnonzero(~okl)[0]])}"
        print(f"  hot LR entries: {len(e)}, turn came for {float(((rl != 0) & (dl > 0)).sum()) / max(int((dl > 0).sum()), 1):.4f}")
