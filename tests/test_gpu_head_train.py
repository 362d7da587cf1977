"""The training step of the mini-batched deep head (head.hip head_step), kernel by kernel, through fwgpu_debug_head_step: forward products with bias,
ReLU and mask; head_final_kernel; the column sums head_colsum_kernel and head_sum_kernel; the gradient products; head_apply_kernel.

STAGE-WISE: every device output is judged against float64 arithmetic on the DEVICE'S OWN inputs of that stage, so every bound is one dot product's,
hr.dot_bound(sum |a||b|) = 2e-5 * sum |a||b| + 1e-6 (the project's number, test_head_products_match_a_torch_f32_reference), and no tolerance compounds
through the chain.  What is not a sum is exact: the general gradient is the f32 expression -(label - p) * importance on the device's own p, dz of the
last layer is fl(g * w_f) times a 0 / 1 mask, the optimizer step is sparse_ref._step on the device's own dW, bit for bit (AdagradFlex: the accumulator
bit for bit, the weight within the powf margin of test_gpu_sparse_kernels.py plus half a unit in the last place of the weight).
WHOLE CHAIN: dW, dx and pred once more against head_ref.head_train64 on the host inputs alone, with the bound that reference propagates from x through
every stage: the check that catches a stage wired to the wrong buffer.

The batches are drawn on the host (head_ref.draw_train_case): examples with a ReLU unit within rounding of 0 are rejected by the reference alone, before
anything goes to the device; test_head_train_ref_cpu.py pins the reference to the oracle and checks the seeds' rejection rates.

An example whose general gradient is 0 learns nothing (oracle: fwo_learn_minibatch): the training step overwrites its rows of x and h with zeros before
the gradient products, so its rows of h come back as zeros; the forward values of every example are checked on a predict-only step of the same batch.

Largest observed ratios to the bounds are in the docstrings of the tests."""
import ctypes as C
import functools

import numpy as np
import pytest

import fwumious_wabbit_amd as fw
import head_ref as hr
import sparse_ref as sr
from fwumious_wabbit_amd import _capi as capi
from helpers import logloss, make_pair, record_labels
from oracle import fwo
from test_gpu_sparse_kernels import FLEX_POW_ULPS

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
ULP = 2.0 ** -23
LUT, SGD, FLEX = fw.Optimizer.AdagradLUT, fw.Optimizer.SGD, fw.Optimizer.AdagradFlex
assert (SGD, FLEX, LUT) == (sr.OPT_SGD, sr.OPT_ADAGRAD_FLEX, sr.OPT_ADAGRAD_LUT)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(U32)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _case(name, n, seed, conc):
    c = hr.draw_train_case(name, n, seed, conc)
    assert c["rejected"] < hr.MAX_REJECTED * c["drawn"], (name, n, c["rejected"], c["drawn"])
    return c


def _regressor(name, optimizer):
    mi, _, _, _ = hr.build_shape(name, optimizer=optimizer)
    mi.nn_init_acc_gradient = 1.0
    if optimizer == FLEX:
        mi.nn_power_t = 0.5  # minus_power_t = -0.5: powf is a real power
    return mi, fw.Regressor(mi)


def _nn_lut(mi):
    """the dense head's step-size table, as the library fills it at creation (optimizer.rs:121-144; the oracle's fwo_lut_init is the same host code)"""
    lut = np.zeros(2048, dtype=F32)
    fwo.lib().fwo_lut_init(lut.ctypes.data_as(C.POINTER(C.c_float)), mi.nn_learning_rate, mi.nn_power_t, mi.nn_init_acc_gradient)
    return lut


def _acc0(total):
    return (1.0 + np.random.default_rng(total).random(total)).astype(F32)


class Ratios(dict):
    """largest |got - want| / bound seen per checked quantity"""

    def check(self, what, got, want, bound, where=None):
        got, want, bound = _f64(got), _f64(want), _f64(bound)
        if where is not None:
            got, want, bound = got[where], want[where], bound[where]
        if got.size == 0:
            return
        assert np.all(np.isfinite(got)), f"{what}: the device's values are not all finite"
        diff = np.abs(got - want)
        r = np.where(diff == 0.0, 0.0, diff / np.where(diff == 0.0, 1.0, bound))  # (an exact 0 needs no bound: dx of an example that learns nothing)
        worst = float(r.max())
        self[what] = max(self.get(what, 0.0), worst)
        assert worst <= 1.0, f"{what}: |got - want| is {worst:.3g} bounds at {np.unravel_index(int(r.argmax()), r.shape)} of {r.shape}"


def _layers_of(c):
    lay, total = hr.head_layout(c["X"], c["layers"], c["topo"])
    w = _f64(c["w"])
    Ws = [w[o:o + out * w_in].reshape(out, w_in) for o, out, w_in in lay]
    bs = [w[o + out * w_in:o + out * w_in + out] for o, out, w_in in lay]
    return lay, total, Ws, bs


def _check_forward(out, c, rows, R):
    """h, mask and pred of a step against float64 on the device's own inputs of each stage, on the examples `rows` (those whose x is finite)"""
    lay, _, Ws, bs = _layers_of(c)
    ref, L = c["ref"], len(c["layers"])
    hin = _f64(c["x"])[rows]
    for l in range(L):
        relu = c["layers"][l][1] == "relu"
        h, m = out["h"][l][rows], out["mask"][l][rows]
        assert np.array_equal(m, ref["mask"][l][rows]), f"mask of layer {l}"
        pre = hin @ Ws[l].T + bs[l]
        bound = hr.dot_bound(np.abs(hin) @ np.abs(Ws[l]).T + np.abs(bs[l]))
        R.check(f"h{l}", h, np.where(m == 0.0, 0.0, pre), bound)
        if relu:
            assert not h[m == 0.0].any(), f"layer {l}: a masked unit is not exactly 0"
        else:
            assert np.all(m == 1.0)
        hin = _f64(h)
    wl = lay[-2][1]
    wf, bf = Ws[L][0], bs[L][0]
    fx = np.concatenate([hin, _f64(c["x"])[rows]], axis=1) if c["topo"] == "one" else hin
    z = fx @ wf + bf
    assert np.abs(z).max() < 4.1 and fx.shape[1] == wf.size and wl == hin.shape[1]
    R.check("pred", out["pred"][rows], 1.0 / (1.0 + np.exp(-z)), 0.25 * hr.dot_bound(np.abs(fx) @ np.abs(wf) + abs(bf)) + ULP)


def _check_backward(out, fwd, c, rows, R):
    """gvec, dz, dx and dW of a training step, each from the device's own buffers of the stage before; fwd: the predict-only step of the same batch"""
    lay, total, Ws, bs = _layers_of(c)
    L, topo, n = len(c["layers"]), c["topo"], len(c["x"])
    label, imp = c["yi"][:, 0], c["yi"][:, 1]
    wl = lay[-2][1]
    w32 = c["w"]
    wf32 = w32[lay[L][0]:lay[L][0] + lay[L][2]]
    assert np.array_equal(_bits(out["pred"]), _bits(fwd["pred"])), "a training step and a predict-only step disagree about a prediction"
    # the general gradient: exactly the f32 expression on the device's own p; exactly 0 for importance 0 and for the other examples
    g = out["gvec"]
    with np.errstate(invalid="ignore"):
        g_want = np.where(imp == 0.0, F32(0.0), -(label - out["pred"]) * imp).astype(F32)
    assert np.array_equal(g[rows], g_want[rows]) and not g[imp == 0.0].any() and not g[~rows].any()
    live = g != 0.0
    assert np.array_equal(live, c["ref"]["g"] != 0.0)
    # rows of h: as the forward left them where the example learns, zeros where it does not
    for l in range(L):
        assert np.array_equal(_bits(out["h"][l][live]), _bits(fwd["h"][l][live])) and not _bits(out["h"][l][~live]).any(), f"h of layer {l} after the step"
        assert np.array_equal(_bits(out["mask"][l][rows]), _bits(fwd["mask"][l][rows]))
    x_eff = _f64(c["x"]).copy()
    x_eff[~live] = 0.0
    assert not out["dx"][~live].any(), "dx of an example that learns nothing"
    # dz of the last layer: fl(g * w_f[i]) times the mask, one rounding per product
    dz_want = (g[:, None] * wf32[None, :wl]) * out["mask"][L - 1]
    assert np.array_equal(out["dz"][L - 1][live], dz_want[live]) and not out["dz"][L - 1][~live].any(), "dz of the last layer"
    dW = out["dW"]
    assert dW.shape == (total,)
    g64 = _f64(g)
    # the final neuron: sum_e g_e [h_last | x]_e (head_colsum_kernel with a scale), its bias sum_e g_e (head_sum_kernel)
    o, _, fin = lay[L]
    fx = np.concatenate([_f64(out["h"][L - 1]), x_eff], axis=1) if topo == "one" else _f64(out["h"][L - 1])
    R.check("dW_final", dW[o:o + fin], g64 @ fx, hr.dot_bound(np.abs(g64) @ np.abs(fx)))
    R.check("dW_final_bias", dW[o + fin:o + fin + 1], [g64.sum()], hr.dot_bound([np.abs(g64).sum()]))
    for l in range(L - 1, -1, -1):
        o, width, w_in = lay[l]
        dz = _f64(out["dz"][l])
        lin = x_eff if l == 0 else _f64(out["h"][l - 1])
        R.check(f"dW{l}", dW[o:o + width * w_in].reshape(width, w_in), dz.T @ lin, hr.dot_bound(np.abs(dz).T @ np.abs(lin)))
        R.check(f"dW{l}_bias", dW[o + width * w_in:o + width * w_in + width], dz.sum(axis=0), hr.dot_bound(np.abs(dz).sum(axis=0)))
        din, sa = dz @ Ws[l], np.abs(dz) @ np.abs(Ws[l])
        if l > 0:
            m = _f64(out["mask"][l - 1])
            R.check(f"dz{l - 1}", out["dz"][l - 1], din * m, hr.dot_bound(sa), where=live)
            assert not out["dz"][l - 1][live][m[live] == 0.0].any() and not out["dz"][l - 1][~live].any(), f"dz of layer {l - 1}: a masked unit is not 0"
        else:
            direct = _f64(g[:, None] * wf32[None, wl:]) if topo == "one" else np.zeros((n, c["X"]))
            R.check("dx", out["dx"], direct + din, hr.dot_bound(np.abs(direct) + sa), where=live)
            if topo == "two":
                no_path = ~np.any(out["dz"][0] != 0.0, axis=1)
                assert not out["dx"][no_path].any(), "topology two: dx of an example without a path"


def _check_step(out, mi, optimizer, w0, acc0, w1, acc1, lut):
    """TABLE_NN_W / TABLE_NN_ACC after the step == sparse_ref._step with the device's own dW"""
    G = out["dW"]
    rate, mpt = F32(mi.nn_learning_rate), F32(-mi.nn_power_t)
    still = G == 0.0
    assert np.array_equal(_bits(w1)[still], _bits(w0)[still]) and np.array_equal(_bits(acc1)[still], _bits(acc0)[still]), "an entry with dW == 0 moved"
    assert not np.isnan(w1).any() and not np.isnan(acc1).any(), "NaN in the dense tables after the step"
    assert (~still).any()
    if optimizer != FLEX:
        w_want, acc_want = w0.copy(), acc0.copy()
        sr._step(G, w_want, acc_want, optimizer, rate, mpt, lut)
        assert np.array_equal(_bits(acc1), _bits(acc_want)), "accumulators after the step"
        assert np.array_equal(_bits(w1), _bits(w_want)), "weights after the step"
        assert np.array_equal(_bits(acc1), _bits(acc0)) == (optimizer == SGD)
        return 0.0
    w64, acc_want = _f64(w0).copy(), acc0.copy()
    sr._step(G, w64, acc_want, optimizer, rate, mpt, lut)
    assert np.array_equal(_bits(acc1), _bits(acc_want)), "accumulators after the step"
    upd = _f64(w0) - w64
    margin = 2 * FLEX_POW_ULPS * _f64(np.spacing(np.abs(upd).astype(F32))) + 0.5 * _f64(np.spacing(np.abs(w1)))
    r = np.abs(_f64(w1) - w64)[~still] / margin[~still]
    assert r.max() <= 1.0, f"AdagradFlex weights: {float(r.max()):.3g} margins"
    return float(r.max())


def _check_whole_chain(out, c, rows, R):
    """dW, dx and pred against head_train64 on the host inputs alone, within the bound it propagates through the chain"""
    ref = c["ref"]
    R.check("chain_dW", out["dW"], ref["dW"], ref["tol"]["dW"])
    R.check("chain_dx", out["dx"], ref["dx"], ref["tol"]["dx"], where=rows)
    R.check("chain_pred", out["pred"], ref["p"], ref["tol"]["p"], where=rows)
    assert np.all(ref["tol"]["dW"] < 0.05 * np.abs(ref["dW"]).max()), "the propagated bound is no check at this shape"


def _run_case(re, mi, c, optimizer, rows=None):
    """a predict-only step, then a training step of the batch c on the regressor; every check; the ratios"""
    n = len(c["x"])
    rows = np.ones(n, dtype=bool) if rows is None else rows
    total = re.table_len(capi.TABLE_NN_W)
    assert total == c["w"].size
    w0, acc0, lut = c["w"], _acc0(total), _nn_lut(mi)
    re.table_write(capi.TABLE_NN_W, w0)
    re.table_write(capi.TABLE_NN_ACC, acc0)
    sums = [re.table_checksum(t) for t in (capi.TABLE_NN_W, capi.TABLE_NN_ACC)]
    R = Ratios()
    fwd = re.debug_head_step(c["x"], c["yi"], update=False)
    assert sums == [re.table_checksum(t) for t in (capi.TABLE_NN_W, capi.TABLE_NN_ACC)], "a predict-only step changed the dense tables"
    assert not fwd["gvec"].any(), "a predict-only step has a general gradient"
    _check_forward(fwd, c, rows, R)
    out = re.debug_head_step(c["x"], c["yi"], update=True)
    w1, acc1 = re.table_read(capi.TABLE_NN_W), re.table_read(capi.TABLE_NN_ACC)
    _check_backward(out, fwd, c, rows, R)
    R["flex_w"] = _check_step(out, mi, optimizer, w0, acc0, w1, acc1, lut)
    _check_whole_chain(out, c, rows, R)
    print(f"head step {c['layers']} {c['topo']} n={n} opt={optimizer}: " + " ".join(f"{k}={v:.3g}" for k, v in sorted(R.items())))
    return R


@pytest.mark.parametrize("name,n,seed,conc", hr.TRAIN_CASES, ids=[f"{c[0]}-{c[1]}" for c in hr.TRAIN_CASES])
def test_each_kernel_of_the_training_step_against_float64_on_its_own_inputs(name, n, seed, conc):
    """AdagradLUT.  Largest |got - want| / bound measured on an MI355X, per shape over its batch sizes: the largest stage-wise ratio (and where), then
    the whole-chain ratios of dW, dx and pred to the propagated bound:
      a    (12, 8 ReLU, one)     stage 0.0113 (dW0)   chain 0.0021  0.0029  0.0029
      w65  (65, 65)              stage 0.0118 (h0)    chain 0.0019  0.0001  0.0004
      w63  (63, 63)              stage 0.0127 (h1)    chain 0.0021  0.0001  0.0004
      w64  (64, 64)              stage 0.0083 (h0)    chain 0.0012  0.0001  0.0002
      w1   (one unit)            stage 0.0064 (h0)    chain 0.0008  0.0038  0.0027
      d    (9 identity, 7, two)  stage 0.0072 (h0)    chain 0.0004  0.0010  0.0012
      c    (256, 256: config E)  stage 0.0257 (h0)    chain 0.0044  0.0030  0.0030
    (f32 sums of at most 496 terms err by ~1e-7 of their absolute sum; the bound allows 2e-5.)  gvec, dz of the last layer and the optimizer step
    are exact.  With a mutated kernel the ratios are in the thousands: `per = n / 16` in head_colsum_kernel fails dW_final at every n % 16 != 0, a bias
    sum that starts at example 1 fails dW_final_bias everywhere, dx without topology one's direct term fails dx, a step that does not store the
    accumulator fails the bit-for-bit comparison of TABLE_NN_ACC."""
    mi, re = _regressor(name, LUT)
    try:
        _run_case(re, mi, _case(name, n, seed, conc), LUT)
    finally:
        re.close()


@pytest.mark.parametrize("n", [17, 72])
@pytest.mark.parametrize("optimizer", [SGD, FLEX], ids=["sgd", "flex"])
def test_the_optimizer_step_of_sgd_and_adagrad_flex(optimizer, n):
    """shape a; SGD: the accumulators keep their bits; AdagradFlex at minus_power_t = -0.5: accumulators bit for bit, weights within the powf margin
    (measured: 0.99 of the margin, which is as it must be -- the weight's own rounding, half a unit in its last place, is most of the margin)"""
    mi, re = _regressor("a", optimizer)
    try:
        _run_case(re, mi, _case("a", n, 1000 + n, 0.0), optimizer)
    finally:
        re.close()


def test_a_larger_batch_after_a_smaller_one_regrows_the_scratch_buffers():
    """n = 16, then 128, then 17 on ONE regressor: HeadScratch frees and reallocates for the second, and serves the third from the larger buffers"""
    mi, re = _regressor("a", LUT)
    try:
        for case in hr.REGROW_CASES:
            _run_case(re, mi, _case(*case), LUT)
    finally:
        re.close()


def test_a_predict_only_step_leaves_gradients_and_tables_alone():
    """update = 0 on shape w65, n = 65: pred by the bound, gvec == 0, TABLE_NN_W / TABLE_NN_ACC checksums unchanged (every case above checks the same
    before its training step; this one stands alone)"""
    mi, re = _regressor("w65", LUT)
    try:
        c = _case("w65", 65, 2065, 0.0)
        re.table_write(capi.TABLE_NN_W, c["w"])
        sums = [re.table_checksum(t) for t in (capi.TABLE_NN_W, capi.TABLE_NN_ACC)]
        fwd = re.debug_head_step(c["x"], c["yi"], update=False)
        _check_forward(fwd, c, np.ones(65, dtype=bool), Ratios())
        assert not fwd["gvec"].any() and set(fwd) == {"pred", "gvec", "h", "mask", "ms"}
        assert sums == [re.table_checksum(t) for t in (capi.TABLE_NN_W, capi.TABLE_NN_ACC)]
    finally:
        re.close()


# ------------------------------------------------------------------ saturated and non-finite logits
@functools.lru_cache(maxsize=None)
def _bad_case(name, sign):
    """the n = 64 batch of a shape with three examples changed on the host: one whose x is scaled until the logit is beyond sign * 50 (finite x), one
    with +inf in an LR slot, one with a NaN in a triangle slot.  All three have importance 1."""
    base = _case(name, 64, {"a": 1064, "w65": 2064}[name], 0.0)
    x, yi, w = base["x"].copy(), base["yi"].copy(), base["w"]
    cand = [e for e in range(64) if yi[e, 1] == 1.0]
    far = hr.head_forward64(_f64(x[cand]) * 1e4, w, base["layers"], base["topo"])[1]
    e_sat = cand[int(np.flatnonzero(sign * far > 50.0)[0])]
    e_inf, e_nan = [e for e in cand if e != e_sat][:2]
    x[e_sat] *= F32(1e4)
    x[e_inf, 3] = np.inf
    x[e_nan, 8 + 2] = np.nan
    assert np.all(np.isfinite(x[e_sat]))
    c = dict(base, x=x, yi=yi, ref=hr.head_train64(x, yi, w, base["layers"], base["topo"]))
    ref = c["ref"]
    assert sign * ref["z"][e_sat] > 50.0 and not np.isfinite(ref["z"][[e_inf, e_nan]]).any() and not ref["g"][[e_sat, e_inf, e_nan]].any()
    assert ref["p"][e_sat] == 1.0 / (1.0 + np.exp(-sign * 50.0)) and np.count_nonzero(ref["g"]) == np.count_nonzero(base["ref"]["g"]) - 3
    return c, [e_sat, e_inf, e_nan]


@pytest.mark.parametrize("sign", [1, -1], ids=["beyond+50", "beyond-50"])
@pytest.mark.parametrize("name", ["a", "w65"])
def test_saturated_and_non_finite_logits_learn_nothing(name, sign):
    """Three of 64 examples: a logit beyond +50 (or -50) from a finite x, a +inf slot, a NaN slot.  p by the sigmoid's rules, g == 0 and dx == 0 for
    them, dW finite and equal -- by the same bounds as everywhere -- to the reference's over the other 61, no NaN in the dense tables after the step.
    Before head_final_kernel neutralised such an example's rows of x and h, this failed at `dW_final`: 0 * inf = NaN in the final neuron's weight
    gradients, then in every dW, then in TABLE_NN_W and TABLE_NN_ACC."""
    c, bad = _bad_case(name, sign)
    rows = np.ones(64, dtype=bool)
    rows[bad] = False  # the other 61: checked as everywhere
    mi, re = _regressor(name, LUT)
    try:
        total = re.table_len(capi.TABLE_NN_W)
        w0, acc0, lut = c["w"], _acc0(total), _nn_lut(mi)
        re.table_write(capi.TABLE_NN_W, w0)
        re.table_write(capi.TABLE_NN_ACC, acc0)
        R = Ratios()
        fwd = re.debug_head_step(c["x"], c["yi"], update=False)
        _check_forward(fwd, c, rows, R)
        out = re.debug_head_step(c["x"], c["yi"], update=True)
        w1, acc1 = re.table_read(capi.TABLE_NN_W), re.table_read(capi.TABLE_NN_ACC)
        assert np.abs(_f64(out["pred"][bad]) - c["ref"]["p"][bad]).max() <= ULP, (out["pred"][bad], c["ref"]["p"][bad])
        assert not out["gvec"][bad].any() and not out["dx"][bad].any()
        assert np.all(np.isfinite(out["dW"])), f"{int((~np.isfinite(out['dW'])).sum())} of {total} gradient sums are not finite"
        _check_backward(out, fwd, c, rows, R)
        _check_step(out, mi, LUT, w0, acc0, w1, acc1, lut)
        _check_whole_chain(out, c, rows, R)
        assert np.all(np.isfinite(w1)) and np.all(np.isfinite(acc1))
        print(f"bad logits {name} {sign}: " + " ".join(f"{k}={v:.3g}" for k, v in sorted(R.items())))
    finally:
        re.close()


# ------------------------------------------------------------------ end to end: fwgpu_learn_batch_sync against the oracle's micro-batch mode
WEIGHT_TOL = 2e-5  # + 1e-5 |w|: the tolerances of test_gpu_parity.py _sync_parity


def _sync_run(batch_sizes, seed, plant=False):
    """a shape-a-like model (6 fields, k = 4, one interaction, 12 + 8 ReLU units, topology one, AdagradLUT) through micro-batches of the given sizes on
    ONE regressor, in order, against om.learn_minibatch.  plant: one LR weight that exactly one example of the (single) batch reads is +inf in both."""
    layers = [(12, "relu", "hu"), (8, "relu", "hu")]
    mi, ocfg, ots = make_pair(6, 4, 12, 12, LUT, interactions=[(0, 1)])
    mi.nn_layers = [dict(width=w, activation=a, init=i) for w, a, i in layers]
    mi.nn_topology, mi.nn_learning_rate, mi.nn_power_t, mi.nn_init_acc_gradient = "one", 0.02, 0.45, 1.0
    n = sum(batch_sizes)
    recs, off = fw.synth_records(6, 1.0, 1.1, 3000, 0.2, seed, 0, n)
    y = record_labels(recs, off)
    om = fwo.Model(ocfg, nn=fwo.make_nn_config(layers, "one", 0.02, 0.45, 1.0))
    re = fw.Regressor(mi)
    L = len(layers)
    re.table_write(capi.TABLE_NN_W, np.concatenate([om.nn_weights(l).copy() for l in range(L + 1)]))
    planted = None
    if plant:
        assert len(batch_sizes) == 1
        en = hr.translate(ots, recs, off)
        e_bad = n // 2
        others = np.concatenate([en.lrs[e]["hash"] for e in range(n) if e != e_bad])
        planted = [int(h) for h, v in zip(en.lrs[e_bad]["hash"], en.lrs[e_bad]["value"]) if h not in others and v != 0.0][0]
        t = re.table_read(capi.TABLE_LR)
        t[2 * planted] = np.inf
        re.table_write(capi.TABLE_LR, t)
        om.lr_table[2 * planted] = np.inf
    fbt = fw.FeatureBufferTranslator(mi)
    sp = re.split_buffers(max(batch_sizes), 512)
    s0 = 0
    for mb in batch_sizes:
        e0 = s0 + mb
        sub, so = recs[int(off[s0]):int(off[e0])], off[s0:e0 + 1] - off[s0]
        p_ref = om.learn_minibatch(ots, sub, so)
        b = re.record_batch(fbt, sub, so)
        re.learn_batch_sync(b, sp, capi.MODE_SEQUENTIAL)
        p_gpu = b.predictions()
        d = np.abs(logloss(p_gpu, y[s0:e0]) - logloss(p_ref, y[s0:e0])).max()
        assert d < hr.LOGLOSS_TOL, f"micro-batch of {mb} at {s0}: max per-example |d logloss| = {d}"
        b.close()
        s0 = e0

    def close(a, b_):
        return bool(np.all(np.abs(a - b_) <= WEIGHT_TOL + 1e-5 * np.abs(b_)))

    w1 = np.concatenate([om.nn_weights(l) for l in range(L + 1)])
    a1 = np.concatenate([om.nn_acc(l) for l in range(L + 1)])
    gw, ga = re.table_read(capi.TABLE_NN_W), re.table_read(capi.TABLE_NN_ACC)
    assert np.all(np.isfinite(w1)) and np.all(np.isfinite(a1))
    assert close(gw, w1), f"dense weights: {int(np.isnan(gw).sum())} NaN, max difference {np.nanmax(np.abs(gw - w1))}"
    assert close(ga, a1), f"dense accumulators: {int(np.isnan(ga).sum())} NaN"
    lr_g, lr_o = re.table_read(capi.TABLE_LR), om.lr_table.copy()
    if plant:
        assert _bits(lr_g)[2 * planted] == _bits(F32(np.inf)) and _bits(lr_o)[2 * planted] == _bits(F32(np.inf)), "the planted entry moved"
        lr_g[2 * planted] = lr_o[2 * planted] = 0.0
    assert close(lr_g, lr_o)
    assert close(re.table_read(capi.TABLE_FFM_W), om.ffm_weights) and close(re.table_read(capi.TABLE_FFM_ACC), om.ffm_acc)
    sp.close()
    re.close()


def test_sync_micro_batches_with_a_ragged_last_batch_match_the_oracle():
    _sync_run([64, 64, 22], seed=71)  # a stream of 150 at mb = 64


def test_sync_micro_batches_of_one_example_then_seventeen_match_the_oracle():
    _sync_run([1] * 20 + [17], seed=72)


def test_sync_micro_batches_that_grow_and_shrink_on_one_regressor_match_the_oracle():
    _sync_run([16, 96, 16], seed=73)


def test_an_example_reading_an_infinite_weight_leaves_the_dense_head_to_the_others():
    """one LR weight, read by exactly one example of a 64-batch, is +inf on the device and in the oracle: that example's logit is not finite, its general
    gradient 0; all dense weights and accumulators must equal the oracle's, the planted entry keeps its bits, the other tables agree with it masked"""
    _sync_run([64], seed=74, plant=True)
