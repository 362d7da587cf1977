"""The deep head's predict-only forward in one launch (fwgpu_enable_fused_head; csrc/head_fused.hip head_forward_fused_kernel) against the float64 head.

Every case: a shape of head_ref with drawn LR / FFM tables and dense head weights in which every slot of x matters (head_ref.dense_head_weights, designed
on the device's own x), the switch on, a predict-only ENTRY batch in MODE_HOGWILD.  Asserted: the route (HEAD_BATCHED at any n) and the kernel family
(HEAD_FUSED, 512 threads, 32 (Xpad + 2 Wpad) floats of LDS); every prediction against head_ref.head_forward64 of the x the launch left on the device
(fwgpu_debug_head_inputs), under the bar test_gpu_head_predict.py holds the GEMM route to (its _assert_preds: PRED_TOL, LOGLOSS_TOL)."""
import numpy as np
import pytest

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import _capi as capi
import head_ref as hr
import test_gpu_head_predict as hp
from helpers import make_pair, record_labels

pytestmark = pytest.mark.gpu

# a: X = 29, widths 12 / 8 (below one tile, K % 8 != 0, scalar loads); d: identity layer, topology two; w63 / w64 / w65: either side of a tile edge, a
# wave with two tiles, a masked last tile; b: X = 496, 16-byte loads; c: config E, one tile per wave, 126 KB of LDS
HEADS = ("a", "d", "w63", "w64", "w65", "b", "c")
NS = (1, 31, 32, 33, 100)
N_MAX = 100
_CTX = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _pad8(v):
    return (v + 7) // 8 * 8


class Ctx:
    pass


def _ctx(name, layers=None):
    """shape `name` (the heads of TRAIN_SHAPES sit on shape a's inputs; `layers`: another head on them), tables drawn, the switch on, N_MAX records"""
    key = (name, str(layers))
    if key in _CTX:
        return _CTX[key]
    c = Ctx()
    c.mi = hr.build_shape(name)[0]
    c.X, c.layers, c.topo = hr.shape_of(name)
    if layers:
        c.layers = layers
        c.mi.nn_layers = [dict(width=w, activation=a, init="hu") for w, a in layers]
    c.re, c.fbt = fw.Regressor(c.mi), fw.FeatureBufferTranslator(c.mi)
    rng = np.random.default_rng(5)
    c.lr = np.ones(c.re.table_len(capi.TABLE_LR), dtype=np.float32)  # interleaved {w, acc}
    c.lr[0::2] = rng.normal(0.0, 0.3, c.lr.size // 2)
    c.re.table_write(capi.TABLE_LR, c.lr)
    c.re.table_write(capi.TABLE_FFM_W, rng.normal(0.0, 0.3, c.re.table_len(capi.TABLE_FFM_W)))
    c.recs, c.off = hr.stream(name if name in hr.SHAPES else "a", N_MAX, seed=77, first=1000)
    c.y = record_labels(c.recs, c.off)
    c.re.enable_fused_head()
    _, x = _launch(c, N_MAX, fused=c.re.fused_head_state()[1] != 0)
    c.w = hr.dense_head_weights(x.astype(np.float64), c.layers, c.topo, seed=3)
    c.re.table_write(capi.TABLE_NN_W, c.w)
    _CTX[key] = c
    return c


def _launch(c, n, fused=True, batch=None):
    """(predictions, x) of the first n records as an entry batch (or of `batch`); the route, and which head ran"""
    b = batch or c.re.batch_from_records(c.fbt, c.recs[:int(c.off[n])], c.off[:n + 1])
    c.re.learn_batch(b, capi.MODE_HOGWILD, False)
    p = b.predictions().copy()
    if batch is None:
        b.close()
    assert c.re.last_route() == capi.ROUTE_HEAD_BATCHED
    info = c.re.last_launch()
    if fused:
        lds = 32 * (_pad8(c.X) + 2 * _pad8(max(w for w, _ in c.layers))) * 4
        assert (info["family"], info["threads"], info["lds_bytes"]) == (capi.KERNEL_HEAD_FUSED, 512, lds), info
    else:
        assert info["family"] == capi.KERNEL_RESIDENT, info
    return p, c.re.head_inputs(len(p))


def _assert_against_float64(c, p, x, what):
    p64, z = hr.head_forward64(x.astype(np.float64), c.w, c.layers, c.topo)
    assert np.abs(z).max() < 20.0
    hp._assert_preds(p, p64, c.y[:len(p)], what)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", HEADS)
def test_every_prediction_against_the_float64_head(name, n):
    c = _ctx(name)
    p, x = _launch(c, n)
    _assert_against_float64(c, p, x, f"head {name}, n = {n}")


def test_the_sigmoid_rules():
    """Head a with the first layer blind to slot 0 of x and the final neuron's direct weight on it at 1: one LR entry in combo 0 puts the logit above
    +50, below -50 and at NaN -> logistic(50), logistic(-50), logistic(0), head_final_kernel's values (test_j of test_gpu_head_predict.py)"""
    c = _ctx("a")
    lay, _ = hr.head_layout(c.X, c.layers, c.topo)
    w = c.w.copy()
    w[lay[0][0]:lay[0][0] + lay[0][1] * c.X:c.X] = 0.0
    w[lay[-1][0] + c.layers[-1][0]] = 1.0
    h = 5
    # (one FFM feature, alone in field 0: every triangle slot stays 0)
    fbs = [fw.lr_and_ffm_vec([(h, float(v), 0)], [(64, 1.0, 0)], 0.0, 1.0) for v in (1e4 / c.lr[2 * h], -1e4 / c.lr[2 * h], np.nan, 0.0)]
    b = c.re.batch(fbs)
    try:
        c.re.table_write(capi.TABLE_NN_W, w)
        p, x = _launch(c, len(fbs), batch=b)
    finally:
        c.re.table_write(capi.TABLE_NN_W, c.w)
        b.close()
    p64, z = hr.head_forward64(x.astype(np.float64), w, c.layers, c.topo)
    assert z[0] > 50.0 and z[1] < -50.0 and np.isnan(z[2]) and abs(z[3]) < 20.0, z
    assert p[0] == np.float32(1.0) and p[2] == np.float32(0.5), p  # (logistic(50) is 1 in f32)
    assert np.allclose(p, p64, rtol=1e-5, atol=0.0), (p, p64)


def test_the_same_bits_again_and_whoever_shares_the_tile():
    c = _ctx("c")
    p, _ = _launch(c, N_MAX)
    p2, _ = _launch(c, N_MAX)
    assert np.array_equal(_bits(p2), _bits(p)), "two launches differ"
    p32, _ = _launch(c, 32)
    assert np.array_equal(_bits(p32), _bits(p[:32])), "the first tile alone differs from the first tile among four"


def test_the_switch_refuses_a_headless_and_a_packed_regressor():
    plain = fw.Regressor(make_pair(4, 4, 14, 14, fw.Optimizer.AdagradLUT)[0])
    packed = plain.pack()
    try:
        assert plain.fused_head_state()[:2] == (False, 0)
        for re, word in ((plain, "no deep head"), (packed, "packed")):
            with pytest.raises(capi.FwgpuError) as e:
                re.enable_fused_head()
            assert e.value.code == capi.ERR_INVALID and word in e.value.message, e.value
    finally:
        packed.close()
        plain.close()


def test_a_head_too_wide_for_the_lds_keeps_the_gemm_route():
    """one layer on shape a's inputs, eight units wider than what 32 (Xpad + 2 Wpad) floats of the CU's LDS hold"""
    a = _ctx("a")
    lds_per_cu = a.re.fused_head_state()[2]
    width = _pad8((lds_per_cu // 128 - _pad8(a.X)) // 2) + 8
    c = _ctx("a", layers=[(width, "relu")])
    assert c.re.fused_head_state()[:2] == (True, 0)
    p, x = _launch(c, N_MAX, fused=False)
    _assert_against_float64(c, p, x, f"one layer of {width} units")
