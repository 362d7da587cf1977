"""The batched deep-head predict route (launch.cpp run_batch_head_predict: the example kernel's emit_x epilogue -> head_step(update = false) ->
head_final_kernel) per example against the oracle, and its head inputs slot by slot against a float64 restatement (head_ref.py, pinned against the
oracle on the CPU by test_head_predict_ref_cpu.py).

Every case: the model is trained for a few hundred examples in the in-order mode, gets dense head weights in which every slot of x matters
(head_ref.dense_head_weights), is mirrored into an oracle model, and predicts with MODE_HOGWILD, update = False.  Asserted: the route the launch took
(fwgpu_debug_last_route); |p_gpu - p_oracle| < PRED_TOL and |d logloss| < LOGLOSS_TOL per example (the bars of test_gpu_parity.py); the head inputs
within 2e-5 * sum|terms| + 1e-6 of x64 (f32 sums in another order, as test_head_products_match_a_torch_f32_reference) and bit-zero where the reference
defines 0; the per-example forward (set_head_predict(0)) within PRED_TOL of the batched one; all five tables unchanged; records and entries bit-equal."""
import numpy as np
import pytest

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import _capi as capi
from fwumious_wabbit_amd import persistence as P
from fwumious_wabbit_amd.feed import VwNamespaceMap
import head_ref as hr
from head_ref import LOGLOSS_TOL, PRED_TOL
from helpers import logloss, record_labels
from oracle import fwo

pytestmark = pytest.mark.gpu

TABLES = (capi.TABLE_LR, capi.TABLE_FFM_W, capi.TABLE_FFM_ACC, capi.TABLE_NN_W, capi.TABLE_NN_ACC)
ROUTE_NAME = {capi.ROUTE_NONE: "none", capi.ROUTE_FUSED: "fused kernel", capi.ROUTE_HEAD_BATCHED: "batched head predict",
              capi.ROUTE_HEAD_BATCHED_REFUSED: "batched head predict refused, per example", capi.ROUTE_PACKED: "packed",
              capi.ROUTE_HOST_WALK: "host walk"}


class Ctx:
    """a trained regressor of one shape, its oracle twin, and a test stream with its float64 head inputs"""


_CTX = {}


def _ctx(name, n, design=512):
    """Shape `name` trained on 300 examples (in order, on the device), a test stream of n records, dense head weights designed on its first `design`
    examples, everything mirrored into the oracle.  Built once per shape and shared; a test that changes the tables restores them."""
    if name in _CTX:
        assert _CTX[name].n >= n
        return _CTX[name]
    c = Ctx()
    s = c.s = hr.SHAPES[name]
    c.name, c.n = name, n
    c.mi, ocfg, c.ots, nn = hr.build_shape(name)
    c.C, c.F, c.k, c.L = c.mi.num_combos, s["F"], s["k"], len(s["layers"])
    c.re = fw.Regressor(c.mi)
    c.fbt = fw.FeatureBufferTranslator(c.mi)
    tr_recs, tr_off = hr.stream(name, 300, seed=5)
    b = c.re.record_batch(c.fbt, tr_recs, tr_off)
    c.re.learn_batch(b, capi.MODE_SEQUENTIAL, True)
    b.close()
    c.train = (tr_recs, tr_off)
    c.recs, c.off = hr.stream(name, n, seed=77, first=1000)
    c.y = record_labels(c.recs, c.off)
    c.lr_table, c.ffm_w = c.re.table_read(capi.TABLE_LR), c.re.table_read(capi.TABLE_FFM_W)
    assert np.count_nonzero(c.lr_table[0::2]) > 100  # (the LR weights are not at init)
    d = min(n, design)
    c.en = hr.translate(c.ots, c.recs, c.off, range(d))  # (the examples whose head inputs are compared; all of them where n <= design)
    c.x64, c.sa, c.exact0 = hr.head_inputs64(c.lr_table, c.ffm_w, c.C, c.F, c.k, c.en)
    c.w = hr.dense_head_weights(c.x64, s["layers"], s["topo"], seed=3)
    assert c.re.table_len(capi.TABLE_NN_W) == c.w.size
    c.re.table_write(capi.TABLE_NN_W, c.w)
    c.om = fwo.Model(ocfg, nn=nn)
    hr.mirror_into_oracle(c.om, c.lr_table, c.ffm_w, c.w, c.L)
    c.p_o = c.om.predict_stream(c.ots, c.recs, c.off, nthreads=8)
    assert np.abs(hr.logits_of(c.p_o)).max() < 20.0  # the oracle's logits, every example of the stream
    _CTX[name] = c
    return c


def _sub(c, n):
    """the first n records of the context's stream"""
    return c.recs[:int(c.off[n])], c.off[:n + 1]


def _launch(re, b, want_route, batched=1):
    re.set_head_predict(batched)
    re.learn_batch(b, capi.MODE_HOGWILD, False)
    route = re.last_route()
    assert route == want_route, f"route: {ROUTE_NAME[route]}, expected {ROUTE_NAME[want_route]}"
    if route == capi.ROUTE_HEAD_BATCHED:  # (the head inputs come from the register-resident kernel's read-only launch)
        assert re.last_launch()["family"] == capi.KERNEL_RESIDENT
    return b.predictions().copy()


def _assert_preds(p, p_o, y, what):
    d = np.abs(p.astype(np.float64) - p_o)
    i = int(d.argmax())
    print(f"{what}: max |p_gpu - p_oracle| = {d.max():.3e} at example {i}")
    assert d.max() < PRED_TOL, f"{what}: |p_gpu - p_oracle| = {d.max()} at example {i} (gpu {p[i]}, oracle {p_o[i]})"
    dl = np.abs(logloss(p, y) - logloss(p_o, y))
    assert dl.max() < LOGLOSS_TOL, f"{what}: |d logloss| = {dl.max()} at example {int(dl.argmax())}"


def _assert_head_inputs(x, x64, sa, exact0, what):
    """slot by slot: f32 sums in another order than the float64 ones; bit-zero where the reference defines exactly 0"""
    err = np.abs(x.astype(np.float64) - x64)
    bound = 2e-5 * sa + 1e-6
    e, sl = np.unravel_index(int((err / bound).argmax()), err.shape)
    print(f"{what}: head inputs, slot nearest its bound: example {e} slot {sl}: |x_gpu - x64| = {err[e, sl]:.3e}, bound {bound[e, sl]:.3e}")
    assert np.all(err <= bound), f"{what}: example {e} slot {sl} of x: gpu {x[e, sl]}, x64 {x64[e, sl]}, bound {bound[e, sl]}"
    bits = np.ascontiguousarray(x).view(np.uint32)
    bad = np.argwhere(exact0 & (bits != 0))
    assert len(bad) == 0, f"{what}: slots that the reference defines as exactly 0 are not bit-zero: (example, slot) {bad[:5].tolist()}"


def _check(c, n, want=capi.ROUTE_HEAD_BATCHED, what=None):
    """every assertion of the module's docstring on the first n records of the context's stream"""
    what = what or f"case {c.name}, n = {n}"
    recs, off = _sub(c, n)
    p_o, y = c.p_o[:n].astype(np.float64), c.y[:n]
    before = [c.re.table_checksum(t) for t in TABLES]
    b = c.re.record_batch(c.fbt, recs, off)
    p = _launch(c.re, b, want)
    if want == capi.ROUTE_HEAD_BATCHED:
        m = min(n, c.en.n)
        x = c.re.head_inputs(n)
        _assert_head_inputs(x[:m], c.x64[:m], c.sa[:m], c.exact0[:m], what)
    else:
        with pytest.raises(capi.FwgpuError):
            c.re.head_inputs(1)
    _assert_preds(p, p_o, y, what + ", records")
    # the per-example forward on the same batch
    p_one = _launch(c.re, b, capi.ROUTE_FUSED, batched=0)
    _assert_preds(p_one, p_o, y, what + ", per-example forward")
    assert np.abs(p_one - p).max() < PRED_TOL
    b.close()
    # the entry route: translated on the host
    be = c.re.batch_from_records(c.fbt, recs, off)
    p_e = _launch(c.re, be, want)
    be.close()
    assert np.array_equal(p_e, p), f"{what}: records and entries differ at {np.flatnonzero(p_e != p)[:5].tolist()}"
    assert [c.re.table_checksum(t) for t in TABLES] == before, f"{what}: a predict-only launch changed a table"
    return p


# ------------------------------------------------------------------ the shapes
def test_a_single_chunk_rows_odd_x_and_a_ragged_last_tile():
    """F = 6, k = 4 with one interaction: X = 29 (X % 4 != 0: the odd lda sends the first product to the tiled GEMM), n = 300 (a ragged last tile of
    44 rows); the single-chunk instantiation's emit_x."""
    _check(_ctx("a", 300), 300)


@pytest.mark.parametrize("n", [1000, 4096, 4097])
def test_b_split_k_products_in_a_predict_launch_and_the_switch_to_the_tiled_kernel(n):
    """F = 30, k = 8 (R = 240), X = 496, 2 x 64 ReLU: the split-K kernel with the bias / ReLU epilogue inside a predict launch (n <= 4096) with a
    ragged M (1000), and both sides of the switch between the two GEMM kernels (4096 / 4097)."""
    _check(_ctx("b", 4097), n)


def test_c_two_chunk_rows_with_a_one_row_last_tile():
    """config E's geometry (F = 30, k = 16: R = 480, 2 x 256 ReLU), n = 257: the two-chunk emit_x and a last tile of one row"""
    _check(_ctx("c", 257), 257)


def test_d_topology_two_and_an_identity_layer():
    """F = 5, k = 4, layers (9, none), (7, relu), topology two: head_final_kernel without the direct copy of x, an identity layer and its mask"""
    _check(_ctx("d", 256), 256)


def test_e_k_not_a_power_of_two():
    """k = 12, F = 20 (R = 240): emit_x with k_log2 == 0xff"""
    _check(_ctx("e", 256), 256)


def test_f_the_gate_refuses_rows_beyond_256_floats_whose_k_does_not_divide_256():
    """k = 12, F = 22 (R = 264, 256 % 12 != 0): head_predict_batched says no, the launch runs the fused kernel; the predictions still match the oracle"""
    _check(_ctx("f", 256), 256, want=capi.ROUTE_FUSED)


@pytest.mark.parametrize("name", ["g256", "g260"])
def test_g_both_sides_of_the_chunk_edge_and_the_triangle_index_at_its_largest(name):
    """k = 8, F = 32 (R = 256, the last single-chunk shape) and k = 4, F = 65 (R = 260, the first two-chunk one; NT = 2145 triangle slots recovered through
    sqrtf).  Every slot of x of every example is compared."""
    c = _ctx(name, 256)
    assert c.en.n == 256 and c.x64.shape[1] == c.C + c.F * (c.F + 1) // 2
    _check(c, 256)


def test_h_a_second_slab_and_buffers_that_grow_and_are_reused():
    """F = 4, k = 4, 1 x 8 ReLU, one regressor: 256 examples, then 33 068 (one slab of 32 768 on the tiled GEMM + a ragged second slab of 300 on the
    split-K kernel: the `first` offsets into x, {label, importance} and the predictions; pred_x / pred_yi / the head's scratch regrown), then 256 again."""
    c = _ctx("h", 33068)
    n_big, slab = 33068, 32768
    recs, off = _sub(c, n_big)
    b_big = c.re.record_batch(c.fbt, recs, off)
    for n in (256, n_big, 256):
        if n == 256:
            _check(c, 256, what=f"case h, n = 256 {'before' if b_big is not None else 'after'} the large batch")
            continue
        before = [c.re.table_checksum(t) for t in TABLES]
        p = _launch(c.re, b_big, capi.ROUTE_HEAD_BATCHED)
        x = c.re.head_inputs(n_big)
        p_o = c.p_o[:n_big].astype(np.float64)
        d = np.abs(p - p_o)
        edge = slice(slab - 2, slab + 2)
        assert d.max() < PRED_TOL, (f"|p_gpu - p_oracle| = {d.max()} at example {int(d.argmax())}; examples {slab - 2} .. {slab + 1} around the slab edge: "
                                    f"gpu {p[edge].tolist()}, oracle {c.p_o[edge].tolist()}")
        assert np.abs(logloss(p, c.y[:n_big]) - logloss(p_o, c.y[:n_big])).max() < LOGLOSS_TOL
        # head inputs: the first examples, those on either side of the slab edge, the last ones
        which = np.r_[0:256, slab - 150:slab + 150, n_big - 150:n_big]
        en = hr.translate(c.ots, c.recs, c.off, which)
        x64, sa, exact0 = hr.head_inputs64(c.lr_table, c.ffm_w, c.C, c.F, c.k, en)
        _assert_head_inputs(x[which], x64, sa, exact0, "case h, n = 33068")
        p64, _ = hr.head_forward64(x64, c.w, c.s["layers"], c.s["topo"])
        assert np.abs(p[which] - p64).max() < PRED_TOL
        p_one = _launch(c.re, b_big, capi.ROUTE_FUSED, batched=0)
        assert np.abs(p_one - p).max() < PRED_TOL
        assert [c.re.table_checksum(t) for t in TABLES] == before
        b_big.close()
        b_big = None


# ------------------------------------------------------------------ model a: entries built by hand, the sigmoid's rules, an inference file, an oversize example
def _crafted(c, n=256, seed=9):
    tr = hr.translate(c.ots, *c.train, range(100))
    ex = hr.crafted_examples(np.unique(tr.lr["hash"]), np.unique(tr.ffm["hash"]), c.C, c.F, c.k, n, seed)
    fbs = [fw.lr_and_ffm_vec(lr, ffm, label, imp) for lr, ffm, label, imp in ex]
    return ex, fbs, hr.crafted_entries(ex)


def test_i_entry_batches_built_by_hand():
    """Model a, 256 examples cycling through head_ref.CRAFTED_KINDS: LR entries out of combo order (the by_combo == false scan), duplicate LR hashes, a
    combo with no entry, no LR entries, no FFM features, fields with one feature / the same feature twice / two features, weighted features,
    importance 0 and 0.5.  Entries only: there is no record that translates to entries out of combo order."""
    c = _ctx("a", 300)
    ex, fbs, en = _crafted(c)
    x64, sa, exact0 = hr.head_inputs64(c.lr_table, c.ffm_w, c.C, c.F, c.k, en)
    p_o = np.array([c.om.predict(en.lrs[e], en.ffms[e]) for e in range(en.n)], dtype=np.float64)
    assert np.abs(hr.logits_of(p_o)).max() < 20.0
    y = np.array([e[2] for e in ex], dtype=np.float32)
    before = [c.re.table_checksum(t) for t in TABLES]
    b = c.re.batch(fbs)
    p = _launch(c.re, b, capi.ROUTE_HEAD_BATCHED)
    x = c.re.head_inputs(en.n)
    for kind in range(len(hr.CRAFTED_KINDS)):  # (kind by kind, so that a failure names its kind)
        sel = np.arange(kind, en.n, len(hr.CRAFTED_KINDS))
        what = f"case i, {hr.CRAFTED_KINDS[kind]}"
        _assert_head_inputs(x[sel], x64[sel], sa[sel], exact0[sel], what)
        _assert_preds(p[sel], p_o[sel], y[sel], what)
    p_one = _launch(c.re, b, capi.ROUTE_FUSED, batched=0)
    _assert_preds(p_one, p_o, y, "case i, per-example forward")
    assert np.abs(p_one - p).max() < PRED_TOL
    b.close()
    assert [c.re.table_checksum(t) for t in TABLES] == before


def test_j_the_sigmoid_rules_of_the_final_kernel():
    """Model a with the final neuron's bias at +100, -100 and NaN: head_final_kernel's three branches give logistic(50), logistic(-50) and logistic(0), the
    oracle's values"""
    c = _ctx("a", 300)
    recs, off = _sub(c, 256)
    b = c.re.record_batch(c.fbt, recs, off)
    try:
        for bias, want in ((100.0, 1.0), (-100.0, 1.0 / (1.0 + np.exp(50.0))), (np.nan, 0.5)):  # (logistic(50) is 1 in f32)
            w = c.w.copy()
            w[-1] = bias
            c.re.table_write(capi.TABLE_NN_W, w)
            hr.mirror_into_oracle(c.om, c.lr_table, c.ffm_w, w, c.L)
            p_o = c.om.predict_stream(c.ots, recs, off)
            assert np.allclose(p_o, want, rtol=1e-6, atol=0.0)
            p = _launch(c.re, b, capi.ROUTE_HEAD_BATCHED)
            assert np.allclose(p, p_o, rtol=1e-5, atol=0.0), (bias, p[:4], p_o[:4])
            if bias != -100.0:
                assert np.array_equal(p, p_o)
    finally:
        c.re.table_write(capi.TABLE_NN_W, c.w)
        hr.mirror_into_oracle(c.om, c.lr_table, c.ffm_w, c.w, c.L)
    b.close()


def test_k_an_inference_file_regressor_on_the_batched_route(tmp_path):
    """Model a saved and loaded immutable (an SGD regressor without accumulators): the same predictions on the batched route"""
    c = _ctx("a", 300)
    path = str(tmp_path / "a.fw")
    P.save_regressor_to_filename(path, c.mi, VwNamespaceMap("".join(f"A{i},ns{i}\n" for i in range(c.F))), c.re)
    mi2, _, re2 = P.new_regressor_from_filename(path, immutable=True)
    assert mi2.optimizer == fw.Optimizer.SGD
    recs, off = _sub(c, 300)
    b = c.re.record_batch(c.fbt, recs, off)
    p = _launch(c.re, b, capi.ROUTE_HEAD_BATCHED)
    b.close()
    b2 = re2.record_batch(fw.FeatureBufferTranslator(mi2), recs, off)
    p2 = _launch(re2, b2, capi.ROUTE_HEAD_BATCHED)
    x2 = re2.head_inputs(300)
    _assert_head_inputs(x2, c.x64[:300], c.sa[:300], c.exact0[:300], "case k")
    _assert_preds(p2, c.p_o[:300].astype(np.float64), c.y[:300], "case k, inference-file regressor")
    assert np.abs(p2 - p).max() < PRED_TOL
    b2.close()
    re2.close()


def test_l_an_example_beyond_what_the_batched_route_stages_falls_back():
    """Model a, one example of 2100 FFM features (in field 5) among 255 ordinary ones: run_batch_head_predict refuses the batch with FWGPU_ERR_RANGE
    (more than 4 x 512 features) and the launch is re-run on the fused kernel, per example; all 256 predictions match the oracle."""
    c = _ctx("a", 300)
    ex, _, _ = _crafted(c, n=256, seed=11)
    tr = hr.translate(c.ots, *c.train, range(300))
    pool = np.unique(tr.ffm["hash"])
    rng = np.random.default_rng(12)
    lr, ffm, label, imp = ex[100]
    # (value 1 / 1024 each: the field's sum stays of the size of an ordinary row, so the example's logit stays inside (-20, 20) like the others')
    big = [r for r in ffm if r[2] < 5 * c.k] + [(int(h), 1.0 / 1024, 5 * c.k) for h in rng.choice(pool, size=2100)]
    ex[100] = (lr, big, label, imp)
    fbs = [fw.lr_and_ffm_vec(lr, ffm, label, imp) for lr, ffm, label, imp in ex]
    en = hr.crafted_entries(ex)
    p_o = np.array([c.om.predict(en.lrs[e], en.ffms[e]) for e in range(en.n)], dtype=np.float64)
    assert np.abs(hr.logits_of(p_o)).max() < 20.0
    y = np.array([e[2] for e in ex], dtype=np.float32)
    b = c.re.batch(fbs)
    p = _launch(c.re, b, capi.ROUTE_HEAD_BATCHED_REFUSED)
    with pytest.raises(capi.FwgpuError):
        c.re.head_inputs(1)
    _assert_preds(p, p_o, y, "case l")
    b.close()
