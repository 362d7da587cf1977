"""The per-example step rule of the mini-batched head (fwgpu_head_set_step_rule, csrc/head_seq.hip): the dense tables after a step against a host
replay of the examples IN ORDER from the device's own dz, h and gvec (sparse_ref._step per example), float64 on the host inputs, and the sync route."""
import numpy as np
import pytest

import fwumious_wabbit_amd as fw
import head_ref as hr
import sparse_ref as sr
from fwumious_wabbit_amd import _capi as capi
from helpers import logloss, make_pair, record_labels
from oracle import fwo
from test_gpu_head_train import FLEX, LUT, SGD, WEIGHT_TOL, _acc0, _bits, _case, _f64, _nn_lut, _regressor
from test_gpu_sparse_kernels import FLEX_POW_ULPS

pytestmark = pytest.mark.gpu

F32 = np.float32
NN_W, NN_ACC = capi.TABLE_NN_W, capi.TABLE_NN_ACC
REPLAY = [c for c in hr.TRAIN_CASES if (c[0] == "a" and c[1] in (1, 15, 17, 65, 128)) or (c[0] in ("w65", "d", "w1", "c") and c[1] == 72)]


def _step(re, c, acc0):
    re.table_write(NN_W, c["w"])
    re.table_write(NN_ACC, acc0)
    re.set_head_step_rule(capi.HEAD_STEP_PER_EXAMPLE)
    out = re.debug_head_step(c["x"], c["yi"], update=True)
    return out, re.table_read(NN_W), re.table_read(NN_ACC)


def _replay(out, c, acc0, mi, optimizer, w_dtype=F32):
    """(w, acc, moved, margin): the tables after the examples' steps in order; which entries saw a G != 0; for a float64 w the sum over the steps of
    test_gpu_head_train.py's AdagradFlex margin (powf's error on the update + half a unit in the last place of the weight)"""
    lay, total = hr.head_layout(c["X"], c["layers"], c["topo"])
    L, n, x, g = len(c["layers"]), len(c["x"]), c["x"], out["gvec"]
    w, acc, lut = c["w"].astype(w_dtype), acc0.copy(), _nn_lut(mi)
    moved, margin = np.zeros(total, dtype=bool), np.zeros(total)
    for l, (o, rows, w_in) in enumerate(lay):
        dz = out["dz"][l] if l < L else g[:, None]
        src = (x if l == 0 else out["h"][l - 1]) if l < L else (np.concatenate([out["h"][L - 1], x], axis=1) if c["topo"] == "one" else out["h"][L - 1])
        sl = slice(o, o + rows * (w_in + 1))
        assert src.shape == (n, w_in) and dz.shape == (n, rows) and src.dtype == dz.dtype == F32
        for e in range(n):
            G = np.concatenate([(dz[e][:, None] * src[e][None, :]).reshape(-1), dz[e]])  # W[j * in + i], then the biases
            before = w[sl].copy()
            sr._step(G, w[sl], acc[sl], optimizer, F32(mi.nn_learning_rate), F32(-mi.nn_power_t), lut)
            moved[sl] |= G != 0.0
            if w_dtype != F32:
                upd = np.abs(before - w[sl]).astype(F32)
                margin[sl] += (G != 0.0) * (2 * FLEX_POW_ULPS * _f64(np.spacing(upd)) + 0.5 * _f64(np.spacing(np.abs(w[sl]).astype(F32))))
    return w, acc, moved, margin


@pytest.mark.parametrize("optimizer", [LUT, SGD], ids=["lut", "sgd"])
@pytest.mark.parametrize("name,n,seed,conc", REPLAY, ids=[f"{c[0]}-{c[1]}" for c in REPLAY])
def test_the_tables_after_a_step_are_the_in_order_replay_bit_for_bit(name, n, seed, conc, optimizer):
    mi, re = _regressor(name, optimizer)
    try:
        c = _case(name, n, seed, conc)
        acc0 = _acc0(c["w"].size)
        out, w1, acc1 = _step(re, c, acc0)
        w_want, acc_want, moved, _ = _replay(out, c, acc0, mi, optimizer)
        assert moved.any() and np.any(_bits(w1) != _bits(c["w"]))
        assert np.array_equal(_bits(acc1), _bits(acc_want)), f"{int((_bits(acc1) != _bits(acc_want)).sum())} accumulators differ from the replay"
        assert np.array_equal(_bits(w1), _bits(w_want)), f"{int((_bits(w1) != _bits(w_want)).sum())} weights differ from the replay"
        assert np.array_equal(_bits(w1)[~moved], _bits(c["w"])[~moved]) and np.array_equal(_bits(acc1)[~moved], _bits(acc0)[~moved]), "G == 0 moved an entry"
        assert np.array_equal(_bits(acc1), _bits(acc0)) == (optimizer == SGD)
        _, w2, acc2 = _step(re, c, acc0)
        assert np.array_equal(_bits(w2), _bits(w1)) and np.array_equal(_bits(acc2), _bits(acc1)), "a second launch from the same start"
    finally:
        re.close()


@pytest.mark.parametrize("name,n,seed,conc", [c for c in REPLAY if c[:2] in (("a", 17), ("w65", 72))], ids=["a-17", "w65-72"])
def test_adagrad_flex_accumulators_exactly_and_weights_within_the_summed_powf_margin(name, n, seed, conc):
    mi, re = _regressor(name, FLEX)
    try:
        c = _case(name, n, seed, conc)
        acc0 = _acc0(c["w"].size)
        out, w1, acc1 = _step(re, c, acc0)
        w64, acc_want, moved, margin = _replay(out, c, acc0, mi, FLEX, w_dtype=np.float64)
        assert np.array_equal(_bits(acc1), _bits(acc_want)) and np.array_equal(_bits(w1)[~moved], _bits(c["w"])[~moved])
        r = np.abs(_f64(w1) - w64)[moved] / margin[moved]
        assert r.max() <= 1.0
    finally:
        re.close()


@pytest.mark.parametrize("name,n,seed,conc", [c for c in REPLAY if c[:2] in (("a", 65), ("d", 72), ("c", 72))], ids=["a-65", "d-72", "c-72"])
def test_the_whole_chain_under_sgd_against_float64_on_the_host_inputs(name, n, seed, conc):
    """the rules differ only by rounding under SGD: w0 - rate * dW of head_train64, its propagated bound plus one rounding of w per step"""
    mi, re = _regressor(name, SGD)
    try:
        c = _case(name, n, seed, conc)
        _, w1, _ = _step(re, c, _acc0(c["w"].size))
        rate, ref = float(F32(mi.nn_learning_rate)), c["ref"]
        bound = rate * ref["tol"]["dW"] + (n + 1) * _f64(np.spacing(np.maximum(np.abs(c["w"]), np.abs(w1))))
        r = np.abs(_f64(w1) - (_f64(c["w"]) - rate * ref["dW"])) / bound
        assert r.max() <= 1.0
    finally:
        re.close()


def _sync_model(optimizer, n, seed):
    layers = [(12, "relu", "hu"), (8, "relu", "hu")]
    mi, ocfg, ots = make_pair(6, 4, 12, 12, optimizer, interactions=[(0, 1)])
    mi.nn_layers = [dict(width=w, activation=a, init=i) for w, a, i in layers]
    mi.nn_topology, mi.nn_learning_rate, mi.nn_power_t, mi.nn_init_acc_gradient = "one", 0.02, 0.45, 1.0
    recs, off = fw.synth_records(6, 1.0, 1.1, 3000, 0.2, seed, 0, n)
    om = fwo.Model(ocfg, nn=fwo.make_nn_config(layers, "one", 0.02, 0.45, 1.0))
    return mi, ots, om, recs, off, np.concatenate([om.nn_weights(l).copy() for l in range(3)])


def _sync_regressor(mi, w0, rule):
    re = fw.Regressor(mi)
    re.table_write(NN_W, w0)
    re.set_head_step_rule(rule)
    return re, fw.FeatureBufferTranslator(mi), re.split_buffers(64, 512)


def _sync_batch(re, fbt, sp, recs, off, s0, e0):
    b = re.record_batch(fbt, recs[int(off[s0]):int(off[e0])], off[s0:e0 + 1] - off[s0])
    re.learn_batch_sync(b, sp, capi.MODE_SEQUENTIAL)
    p = b.predictions()
    b.close()
    return p


@pytest.mark.parametrize("optimizer,sizes", [(LUT, [1] * 20), (SGD, [16, 33])], ids=["lut-ones", "sgd-16-33"])
def test_sync_micro_batches_under_the_per_example_rule_match_the_oracle(optimizer, sizes):
    mi, ots, om, recs, off, w0 = _sync_model(optimizer, sum(sizes), 75)
    re, fbt, sp = _sync_regressor(mi, w0, capi.HEAD_STEP_PER_EXAMPLE)
    y, s0 = record_labels(recs, off), 0
    for mb in sizes:
        p_ref = om.learn_minibatch(ots, recs[int(off[s0]):int(off[s0 + mb])], off[s0:s0 + mb + 1] - off[s0])
        p_gpu = _sync_batch(re, fbt, sp, recs, off, s0, s0 + mb)
        assert np.abs(logloss(p_gpu, y[s0:s0 + mb]) - logloss(p_ref, y[s0:s0 + mb])).max() < hr.LOGLOSS_TOL
        s0 += mb
    for table, want in ((NN_W, [om.nn_weights(l) for l in range(3)]), (NN_ACC, [om.nn_acc(l) for l in range(3)])):
        got, want = re.table_read(table), np.concatenate(want)
        assert np.all(np.abs(got - want) <= WEIGHT_TOL + 1e-5 * np.abs(want)), f"table {table}: max difference {np.abs(got - want).max()}"
    sp.close()
    re.close()


def test_the_switch_reaches_the_sync_route_and_switches_back():
    mi, _, _, recs, off, w0 = _sync_model(LUT, 66, 76)
    (ra, fa, sa), (rb, fb, sb) = _sync_regressor(mi, w0, capi.HEAD_STEP_PER_EXAMPLE), _sync_regressor(mi, w0, capi.HEAD_STEP_SUMMED)
    _sync_batch(ra, fa, sa, recs, off, 0, 33), _sync_batch(rb, fb, sb, recs, off, 0, 33)
    assert not np.array_equal(_bits(ra.table_read(NN_ACC)), _bits(rb.table_read(NN_ACC))), "both rules left the same dense accumulators"
    tables = (capi.TABLE_LR, capi.TABLE_FFM_W, capi.TABLE_FFM_ACC, NN_W, NN_ACC)
    for t in tables:  # the twins start the fresh batch from the same state
        ra.table_write(t, rb.table_read(t))
    assert (ra.head_step_rule(), rb.head_step_rule()) == (capi.HEAD_STEP_PER_EXAMPLE, capi.HEAD_STEP_SUMMED)
    ra.set_head_step_rule(capi.HEAD_STEP_SUMMED)
    _sync_batch(ra, fa, sa, recs, off, 33, 66), _sync_batch(rb, fb, sb, recs, off, 33, 66)
    for t in tables:
        assert np.array_equal(_bits(ra.table_read(t)), _bits(rb.table_read(t))), f"table {t} after switching back"
    for q in (sa, sb, ra, rb):
        q.close()


def test_refusals_say_why():
    mi, _, _ = make_pair(6, 4, 12, 12, LUT)
    plain = fw.Regressor(mi)
    packed = plain.pack()
    _, headed = _regressor("a", LUT)
    for re, rule, word in ((plain, capi.HEAD_STEP_PER_EXAMPLE, "no deep head"), (packed, capi.HEAD_STEP_PER_EXAMPLE, "packed"), (headed, 7, "unknown rule 7")):
        with pytest.raises(capi.FwgpuError) as err:
            re.set_head_step_rule(rule)
        assert err.value.code == capi.ERR_INVALID and word in err.value.message, err.value.message
    assert headed.head_step_rule() == capi.HEAD_STEP_SUMMED
    for re in (packed, plain, headed):
        re.close()
