"""The float64 restatement of the deep head's predict-only forward (head_ref.py) against the oracle's own predict, on the CPU: the check that the
reference is right before it judges the device (test_gpu_head_predict.py).  Every shape of the batched-route tests, the oracle's own tables after a few
hundred learned examples, dense head weights in which every slot of x matters; bound |p64 - p_oracle| < 1e-6."""
import numpy as np
import pytest

import head_ref as hr
from oracle import fwo

REF_TOL = 1e-6


def _trained_oracle(name, n_train=200, seed=5):
    mi, ocfg, ots, nn = hr.build_shape(name)
    om = fwo.Model(ocfg, nn=nn)
    recs, off = hr.stream(name, n_train, seed)
    om.run_stream(ots, recs, off, holdout_after=0, nthreads=1, want_preds=False)
    return mi, ots, om, recs, off


def _nn_w(om, L):
    return np.concatenate([om.nn_weights(l).copy() for l in range(L + 1)])


@pytest.mark.parametrize("name", list(hr.SHAPES))
def test_float64_head_predict_matches_the_oracle_on_every_shape_cpu(name):
    s = hr.SHAPES[name]
    mi, ots, om, _, _ = _trained_oracle(name)
    recs, off = hr.stream(name, 36, seed=77, first=1000)
    en = hr.translate(ots, recs, off)
    C, F, k = mi.num_combos, s["F"], s["k"]
    x64, sa, exact0 = hr.head_inputs64(om.lr_table, om.ffm_weights, C, F, k, en)
    assert x64.shape[1] == C + F * (F + 1) // 2 and np.all(x64[exact0] == 0.0) and np.all(sa >= np.abs(x64) - 1e-12)
    # first on the head the oracle trained, then on dense weights in which every slot of x matters
    for w in (_nn_w(om, len(s["layers"])), hr.dense_head_weights(x64, s["layers"], s["topo"], seed=3)):
        hr.mirror_into_oracle(om, om.lr_table.copy(), om.ffm_weights.copy(), w, len(s["layers"]))
        p64, z64 = hr.head_forward64(x64, w, s["layers"], s["topo"])
        p_o = np.array([om.predict(en.lrs[e], en.ffms[e]) for e in range(en.n)])
        assert np.abs(z64).max() < 20.0
        assert np.abs(p64 - p_o).max() < REF_TOL, (name, np.abs(p64 - p_o).max(), int(np.abs(p64 - p_o).argmax()))
        assert np.array_equal(om.predict_stream(ots, recs, off), p_o.astype(np.float32))
    # the dense weights do what they are for: exchanging two slots of x moves a prediction by far more than the device tests' tolerance
    xs = x64.copy()
    xs[:, [1, C + 1]] = xs[:, [C + 1, 1]]
    p_s, _ = hr.head_forward64(xs, w, s["layers"], s["topo"])
    assert np.abs(p_s - p64).max() > 100 * hr.PRED_TOL


def test_float64_head_predict_matches_the_oracle_on_crafted_entries_and_at_the_sigmoid_rules_cpu():
    s = hr.SHAPES["a"]
    mi, ots, om, recs, off = _trained_oracle("a")
    tr = hr.translate(ots, recs, off, range(100))
    C, F, k, L = mi.num_combos, s["F"], s["k"], len(s["layers"])
    ex = hr.crafted_examples(np.unique(tr.lr["hash"]), np.unique(tr.ffm["hash"]), C, F, k, 40, seed=9)
    en = hr.crafted_entries(ex)
    x64, sa, exact0 = hr.head_inputs64(om.lr_table, om.ffm_weights, C, F, k, en)
    assert exact0[2, 3] and exact0[3, :C].all() and exact0[4, C:][np.tril_indices(F)[0] == np.tril_indices(F)[1]].all()
    w = hr.dense_head_weights(x64, s["layers"], s["topo"], seed=4)
    hr.mirror_into_oracle(om, om.lr_table.copy(), om.ffm_weights.copy(), w, L)
    p64, _ = hr.head_forward64(x64, w, s["layers"], s["topo"])
    p_o = np.array([om.predict(en.lrs[e], en.ffms[e]) for e in range(en.n)])
    assert np.abs(p64 - p_o).max() < REF_TOL, (np.abs(p64 - p_o).max(), hr.CRAFTED_KINDS[int(np.abs(p64 - p_o).argmax()) % 10])
    # the final neuron's bias at +100, -100 and NaN: logistic(50), logistic(-50) and logistic(0), as sigmoid_block has them
    for bias, want in ((100.0, 1.0 / (1.0 + np.exp(-50.0))), (-100.0, 1.0 / (1.0 + np.exp(50.0))), (np.nan, 0.5)):
        wb = w.copy()
        wb[-1] = bias
        hr.mirror_into_oracle(om, om.lr_table.copy(), om.ffm_weights.copy(), wb, L)
        pb, _ = hr.head_forward64(x64, wb, s["layers"], s["topo"])
        p_o = np.array([om.predict(en.lrs[e], en.ffms[e]) for e in range(en.n)])
        assert np.abs(pb - want).max() < 1e-12 and np.abs(pb - p_o).max() < REF_TOL
