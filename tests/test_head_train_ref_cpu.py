"""The float64 restatement of one training step of the mini-batched head (head_ref.head_train64) against the oracle's micro-batch mode
(fwo_learn_minibatch), on the CPU: the check that the reference is right before it judges the kernels (test_gpu_head_train.py).

SGD, so that the oracle's summed gradient can be read back from its weights: w_after = fl(w - fl(G * rate)), hence
(w_before - w_after) / rate is the oracle's f32 sum G up to one rounding of G * rate (part of the relative term) and one rounding of the
weight, HALF_ULP * |w| / rate.  The bound on |dW64 - that| is therefore
    2e-5 * sum |products| + 1e-6 + 2^-24 * |w_before| / rate
with the sum of absolute products head_train64 returns for the element: the oracle adds the same products in f32, in example order.
Predictions: |p64 - p_oracle| <= PRED_TOL.

Every batch holds one example of importance 0 and one whose x holds an inf (an LR weight preset to +inf that this example alone reads): their
general gradient is 0 and neither may move a dense weight -- checked on a batch of these two alone, whose dense weights must keep their bits."""
import numpy as np
import pytest

import head_ref as hr
from oracle import fwo

N = 40
E_IMP0, E_INF = 7, 23


def _nn(om, L, acc=False):
    return np.concatenate([(om.nn_acc(l) if acc else om.nn_weights(l)).copy() for l in range(L + 1)])


def _batch(name, ots, seed):
    """40 records, example E_IMP0 with importance 0; (records, offsets, entries, an LR hash that E_INF alone reads)"""
    recs, off = hr.stream(name, N, seed, first=1000)
    recs = recs.copy()
    recs[int(off[E_IMP0]) + 2] = np.float32(0.0).view(np.uint32)
    en = hr.translate(ots, recs, off)
    others = np.concatenate([en.lrs[e]["hash"] for e in range(N) if e != E_INF])
    own = [int(h) for h, v in zip(en.lrs[E_INF]["hash"], en.lrs[E_INF]["value"]) if h not in others and v != 0.0]
    assert own, "the example shares every LR entry"
    return recs, off, en, own[0]


@pytest.mark.parametrize("name", ["a", "d", "h"])
def test_float64_head_training_step_matches_the_oracle_micro_batch_cpu(name):
    s = hr.SHAPES[name]
    layers, topo, L = s["layers"], s["topo"], len(s["layers"])
    mi, ocfg, ots, nn = hr.build_shape(name, optimizer=fwo.OPT_SGD)
    om = fwo.Model(ocfg, nn=nn)
    tr, tro = hr.stream(name, 200, 5)
    om.run_stream(ots, tr, tro, holdout_after=0, nthreads=1, want_preds=False)
    recs, off, en, h_inf = _batch(name, ots, seed=78)
    C, F, k = mi.num_combos, s["F"], s["k"]
    x_fin, _, _ = hr.head_inputs64(om.lr_table, om.ffm_weights, C, F, k, en)
    w0 = hr.dense_head_weights(x_fin, layers, topo, seed=6)
    lr_t = om.lr_table.copy()
    lr_t[2 * h_inf] = np.inf
    hr.mirror_into_oracle(om, lr_t, om.ffm_weights.copy(), w0, L)
    with np.errstate(invalid="ignore"):
        x64, _, _ = hr.head_inputs64(om.lr_table, om.ffm_weights, C, F, k, en)
    assert np.isinf(x64[E_INF]).sum() >= 1 and np.all(np.isfinite(np.delete(x64, E_INF, axis=0)))
    yi = np.array([[recs[int(o) + 1], recs[int(o) + 2:int(o) + 3].view(np.float32)[0]] for o in off[:-1]], dtype=np.float64)
    assert yi[E_IMP0, 1] == 0.0 and set(yi[:, 0]) == {0.0, 1.0}
    ref = hr.head_train64(x64, yi, w0, layers, topo)
    assert ref["g"][E_IMP0] == 0.0 and ref["g"][E_INF] == 0.0 and np.count_nonzero(ref["g"]) == N - 2
    assert not ref["dx"][E_IMP0].any() and not ref["dx"][E_INF].any() and np.all(np.isfinite(ref["dW"])) and np.all(np.isfinite(ref["dx"]))
    # no ReLU unit of a learning example so near 0 that f32 and float64 could disagree about its mask
    on = ref["g"] != 0.0
    for l, (_, act) in enumerate(layers):
        if act == "relu":
            assert np.all(np.abs(ref["pre"][l][on]) > 4 * hr.dot_bound(ref["sa"]["pre"][l][on]))
    # the two examples alone: predictions by the sigmoid's rules, no dense weight moves
    two = [E_IMP0, E_INF]
    sub = np.concatenate([recs[int(off[e]):int(off[e + 1])] for e in two])
    so = np.cumsum([0] + [int(off[e + 1] - off[e]) for e in two]).astype(np.uint64)
    keep = om.lr_table.copy(), om.ffm_weights.copy()
    p2 = om.learn_minibatch(ots, sub, so)
    assert np.abs(p2 - ref["p"][two]).max() <= hr.PRED_TOL
    assert np.array_equal(_nn(om, L).view(np.uint32), w0.view(np.uint32)), "an example with g == 0 moved a dense weight of the oracle"
    hr.mirror_into_oracle(om, keep[0], keep[1], w0, L)
    # the whole batch
    rate = float(nn.nn_learning_rate)
    p_o = om.learn_minibatch(ots, recs, off)
    w1 = _nn(om, L)
    assert np.all(np.isfinite(w1))
    assert np.abs(p_o - ref["p"]).max() <= hr.PRED_TOL, np.abs(p_o - ref["p"]).max()
    dW_o = (w0.astype(np.float64) - w1.astype(np.float64)) / rate
    bound = hr.dot_bound(ref["sa"]["dW"]) + 2.0 ** -24 * np.abs(w0.astype(np.float64)) / rate
    ratio = np.abs(dW_o - ref["dW"]) / bound
    assert ratio.max() <= 1.0, (name, float(ratio.max()), int(ratio.argmax()))
    # the comparison has teeth: in every block of the layout there are gradients far above their own bound
    lay, _ = hr.head_layout(x64.shape[1], layers, topo)
    size = np.abs(ref["dW"]) / bound
    for o, out, w_in in lay:
        assert size[o:o + out * w_in].max() > 100 and size[o + out * w_in:o + out * w_in + out].max() > 100, (name, o)


def test_float64_head_training_step_leaves_out_what_the_rules_leave_out_cpu():
    """head_train64 on drawn inputs: importance 0, a NaN logit and logits beyond +-50 give g == 0, dx == 0 and no share of dW; dx is g
    times the slope of the logit in both topologies (the direct term of topology one included); topology two without a path has dx == 0; an
    identity layer's mask is all ones"""
    rng = np.random.default_rng(3)
    layers, X, n = [(5, "none"), (4, "relu")], 6, 12
    for topo in ("one", "two"):
        lay, total = hr.head_layout(X, layers, topo)
        w = rng.standard_normal(total) * 0.3
        x = rng.standard_normal((n, X))
        yi = np.stack([rng.integers(0, 2, n).astype(float), np.ones(n)], axis=1)
        yi[2, 1] = 0.0
        x[5, 1] = np.nan
        x[6, 2] = np.inf
        x[7] *= 1e4
        ref = hr.head_train64(x, yi, w, layers, topo)
        off_rows = [2, 5, 6, 7]
        assert not ref["g"][off_rows].any() and not ref["dx"][off_rows].any() and abs(ref["z"][7]) > 50
        assert np.all(ref["mask"][0] == 1.0)
        live = np.setdiff1d(np.arange(n), off_rows)
        sub = hr.head_train64(x[live], yi[live], w, layers, topo)
        assert np.array_equal(sub["dW"], ref["dW"]) and np.array_equal(sub["dx"], ref["dx"][live])
        o, _, fin = lay[-1]
        assert np.isclose(ref["dW"][o + fin], ref["g"].sum())
        # dx = g * d logit / d x, the derivative taken from head_forward64 by central differences (the head is piecewise linear in x)
        for e in live:
            for i in range(X):
                xp, xm = x[e:e + 1].copy(), x[e:e + 1].copy()
                xp[0, i] += 1e-6
                xm[0, i] -= 1e-6
                slope = (hr.head_forward64(xp, w, layers, topo)[1][0] - hr.head_forward64(xm, w, layers, topo)[1][0]) / 2e-6
                assert abs(ref["dx"][e, i] - ref["g"][e] * slope) < 1e-7, (topo, e, i)
        if topo == "two":
            w2 = w.copy()
            w2[lay[1][0]:lay[1][0] + 4 * 5] = 0.0  # the second layer's weights at 0: no path from the logit back to x
            assert not hr.head_train64(x, yi, w2, layers, topo)["dx"].any()
        else:
            assert np.abs(ref["dx"][live]).min() > 0


def test_the_seeded_batches_of_the_device_tests_reject_few_draws_cpu():
    """every batch test_gpu_head_train.py draws: fewer than a tenth of the examples looked at had a ReLU unit within RELU_MARGIN forward bounds of 0;
    every batch of six or more examples mixes labels 0 / 1 and importances 1 / 0.5 / 0; logits inside +-4; both mask values occur in every ReLU layer"""
    for name, n, seed, conc in hr.TRAIN_CASES:
        c = hr.draw_train_case(name, n, seed, conc)
        assert c["rejected"] < hr.MAX_REJECTED * c["drawn"], (name, n, c["rejected"], c["drawn"])
        ref = c["ref"]
        assert np.abs(ref["z"]).max() < 4.0
        if n >= 6:
            assert set(c["yi"][:, 0]) == {0.0, 1.0} and set(c["yi"][:, 1]) == {0.0, 0.5, 1.0}
            assert np.array_equal(ref["g"] == 0.0, c["yi"][:, 1] == 0.0)
            for m, (_, act) in zip(ref["mask"], c["layers"]):
                assert (0.0 < m.mean() < 1.0) == (act == "relu")
