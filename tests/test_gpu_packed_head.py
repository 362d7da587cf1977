"""Deep-head models served from packed FFM weights (fwgpu_model_load_packed_head, new_regressor_from_filename(packed=True, packed_head=True); csrc/head_packed.hip, FWGPU_ROUTE_PACKED_HEAD).

Per shape: an f32 head regressor trained in order on 300 synthetic records (14-bit tables), dense head weights in which every slot of x matters
(head_ref.dense_head_weights), saved, converted with quantize_weights, and loaded f32 and packed.  The reference is float64 on the values the buckets
stand for: head_ref.head_inputs64 on the packed regressor's own table_read (bit-exact by test_gpu_packed.py), then head_ref.head_forward64.  The bars
are the project's: x slot by slot within 2e-5 * sum|terms| + 1e-6 and bit-zero where the reference defines 0
(test_gpu_head_predict._assert_head_inputs), predictions within PRED_TOL."""
from types import SimpleNamespace

import numpy as np
import pytest

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import _capi as capi
from fwumious_wabbit_amd import persistence as P
from fwumious_wabbit_amd.feed import VwNamespaceMap
import head_ref as hr
from head_ref import PRED_TOL
from helpers import make_pair
from test_gpu_head_predict import _assert_head_inputs

pytestmark = pytest.mark.gpu

# F x k: one lane per slot and fewer fields than waves; three lanes per slot; R = 256, the last lane of the chunk live; two chunks, X = 496 (config E)
SHAPES = [(4, 4), (20, 12), (8, 32), (30, 16)]
LAYERS, TOPO = [(16, "relu"), (8, "relu")], "one"
TABLES = (capi.TABLE_LR, capi.TABLE_FFM_W, capi.TABLE_NN_W)
N = 100


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _vwmap(n):
    return VwNamespaceMap("".join(f"N{i:02d},ns{i}\n" for i in range(n)))


def _head_mi(F, k):
    mi, _, ots = make_pair(F, k, 14, 14, fw.Optimizer.AdagradLUT)
    mi.nn_layers = [dict(width=w, activation=a, init="hu") for w, a in LAYERS]
    mi.nn_topology = TOPO
    return mi, ots


def _build(F, k, tmp):
    """the shape's files, its two loads, the 100 examples and their float64 reference"""
    c = SimpleNamespace(F=F, k=k)
    mi, ots = _head_mi(F, k)
    c.C = mi.num_combos
    re = fw.Regressor(mi)
    recs, off = fw.synth_records(F, 1.0, 1.1, 3000, 0.1, 5, 0, 300)
    b = re.record_batch(fw.FeatureBufferTranslator(mi), recs, off)
    re.learn_batch(b, capi.MODE_SEQUENTIAL, True)
    b.close()
    # example 0: field 1 with nine weighted features (the 4-row pipeline twice and a remainder), field 0 with one, the others empty; then
    # head_ref.CRAFTED_KINDS in turn: no FFM entry at all, fields of one and of two features, weighted values, a combo without an entry, ...
    tr = hr.translate(ots, recs, off, range(100))
    pool_lr, pool_ffm = np.unique(tr.lr["hash"]), np.unique(tr.ffm["hash"])
    rng = np.random.default_rng(17)
    nine = [(int(pool_ffm[0]), 1.0, 0)] + [(int(h), float(v), k) for h, v in zip(rng.choice(pool_ffm, 9), rng.choice([0.5, 1.0, 2.0, -0.75], 9))]
    c.ex = [([(int(rng.choice(pool_lr)), 1.0, cc) for cc in range(c.C)], nine, 1.0, 1.0)] + hr.crafted_examples(pool_lr, pool_ffm, c.C, F, k, N - 1, 9)
    c.fbs = [fw.lr_and_ffm_vec(lr, ffm, label, imp) for lr, ffm, label, imp in c.ex]
    c.en = hr.crafted_entries(c.ex)
    x_design, _, _ = hr.head_inputs64(re.table_read(capi.TABLE_LR), re.table_read(capi.TABLE_FFM_W), c.C, F, k, c.en)
    re.table_write(capi.TABLE_NN_W, hr.dense_head_weights(x_design, LAYERS, TOPO, seed=3))
    c.t, c.q, c.u = (str(tmp / f"{F}x{k}.{s}") for s in "tqu")
    P.save_regressor_to_filename(c.t, mi, _vwmap(F), re)
    re.close()
    P.convert_inference_regressor(c.t, c.q, quantize_weights=True)
    P.convert_inference_regressor(c.t, c.u)
    _, _, c.rf = P.new_regressor_from_filename(c.q, immutable=True)
    c.mi, _, c.rp = P.new_regressor_from_filename(c.q, immutable=True, packed=True, packed_head=True)
    assert c.rp.ffm_storage()[0] == capi.FFM_F16_BUCKETS
    c.w = c.rp.table_read(capi.TABLE_NN_W)
    c.x64, c.sa, c.exact0 = hr.head_inputs64(c.rp.table_read(capi.TABLE_LR), c.rp.table_read(capi.TABLE_FFM_W), c.C, F, k, c.en)
    c.p64, z = hr.head_forward64(c.x64, c.w, LAYERS, TOPO)
    assert np.abs(z).max() < 20.0 and np.std(c.p64) > 0.02  # (a model that says something)
    return c


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("packed_head")


@pytest.fixture(scope="module")
def ctx(tmp):
    """ctx(F, k): _build's result, made once per shape and module; its regressors are closed when the module is done"""
    built = {}

    def get(F, k):
        if (F, k) not in built:
            built[(F, k)] = _build(F, k, tmp)
        return built[(F, k)]

    yield get
    for c in built.values():
        c.rf.close()
        c.rp.close()


def _launch(re, b, mode=capi.MODE_HOGWILD):
    re.learn_batch(b, mode, False)
    return b.predictions().copy()


@pytest.mark.parametrize("n", [1, 3, N])
@pytest.mark.parametrize("F,k", SHAPES, ids=[f"{F}x{k}" for F, k in SHAPES])
def test_head_inputs_and_predictions_from_buckets(ctx, F, k, n):
    c = ctx(F, k)
    what = f"{F}x{k}, n = {n}"
    before = [c.rp.table_checksum(t) for t in TABLES]
    assert np.array_equal(_bits(c.w), _bits(c.rf.table_read(capi.TABLE_NN_W)))  # the head's tables: what the f32 load holds
    b = c.rp.batch(c.fbs[:n])
    p = _launch(c.rp, b)
    info = c.rp.last_launch()
    assert c.rp.last_route() == capi.ROUTE_PACKED_HEAD and info["family"] == capi.KERNEL_PACKED_HEAD, info
    assert info["chunks"] == (1 if F * k <= 256 else 2) and info["threads"] == 256 and 0 < info["lds_bytes"] <= 160 * 1024, info
    x = c.rp.head_inputs(n)
    _assert_head_inputs(x, c.x64[:n], c.sa[:n], c.exact0[:n], what)
    d = np.abs(p - c.p64[:n])
    print(f"{what}: max |p - p64| = {d.max():.3e}")
    assert d.max() < PRED_TOL, (what, int(d.argmax()), d.max())
    # a second launch and the in-order mode: the same bits
    for mode in (capi.MODE_HOGWILD, capi.MODE_SEQUENTIAL):
        p2 = _launch(c.rp, b, mode)
        assert c.rp.last_route() == capi.ROUTE_PACKED_HEAD
        assert np.array_equal(_bits(p2), _bits(p)) and np.array_equal(_bits(c.rp.head_inputs(n)), _bits(x)), (what, mode)
    # an updating launch is refused, as on any packed regressor
    with pytest.raises(capi.FwgpuError) as e:
        c.rp.learn_batch(b, capi.MODE_HOGWILD, True)
    assert e.value.code == capi.ERR_INVALID and "updating" in e.value.message
    b.close()
    if n == N:  # the f32 load of the same file, whichever route it takes
        bf = c.rf.batch(c.fbs)
        pf = _launch(c.rf, bf)
        bf.close()
        assert np.abs(pf - p).max() < PRED_TOL, (what, np.abs(pf - p).max())
    assert [c.rp.table_checksum(t) for t in TABLES] == before


def test_the_three_file_kinds_load_to_the_same_tables(ctx):
    c = ctx(20, 12)
    for path in (c.t, c.u):  # a training file (optimizer state behind every block) and an unquantised inference file
        _, _, r = P.new_regressor_from_filename(path, immutable=True, packed=True, packed_head=True)
        try:
            for t in TABLES:
                assert np.array_equal(_bits(r.table_read(t)), _bits(c.rp.table_read(t))), (path, t)
        finally:
            r.close()


def test_the_fused_head_on_a_packed_regressor(ctx):
    c = ctx(20, 12)
    _, _, r = P.new_regressor_from_filename(c.q, immutable=True, packed=True, packed_head=True)
    try:
        r.enable_fused_head()
        b = r.batch(c.fbs[:33])
        p = _launch(r, b)
        b.close()
        assert r.last_route() == capi.ROUTE_PACKED_HEAD and r.last_launch()["family"] == capi.KERNEL_HEAD_FUSED
        assert np.abs(p - c.p64[:33]).max() < PRED_TOL
    finally:
        r.close()


def test_refusals_name_the_head(ctx, tmp):
    c = ctx(4, 4)

    def refused(call, word, *args):
        with pytest.raises(capi.FwgpuError) as e:
            call(*args)
        assert e.value.code == capi.ERR_INVALID and word in e.value.message, e.value

    refused(c.rp.enable_head_requests, "head")
    refused(c.rp.enable_packed_caches, "head")
    refused(c.rp.apply_diff, "head", b"\x01\x02")
    for mi, into in ((_head_mi(4, 4)[0], None), (make_pair(4, 4, 14, 14, fw.Optimizer.AdagradLUT)[0], c.rp)):  # from a head trainer; into a packed head regressor
        trainer = fw.Regressor(mi)
        try:
            refused(trainer.pack, "head", into)
        finally:
            trainer.close()
    # 30 x 12: R = 360 does not split at the chunk edge -- refused at the load, as for a headless model
    mi, _ = _head_mi(30, 12)
    re = fw.Regressor(mi)
    path = str(tmp / "30x12.t")
    P.save_regressor_to_filename(path, mi, _vwmap(30), re)
    re.close()
    refused(P.new_regressor_from_filename, "ffm_k", path, True, 0, True, False, True)
    refused(P.new_regressor_from_filename, "deep head", c.q, True, 0, True)  # without packed_head: refused as ever


def test_serving_whole_lines_with_packed_weights(ctx):
    from fwumious_wabbit_amd.serving import Predictor
    c = ctx(30, 16)
    rng = np.random.default_rng(5)
    lines = [" ".join(f"|N{ns:02d} " + " ".join(f"{rng.integers(0, 3000)}" + (":0.5" if rng.random() < 0.2 else "") for _ in range(rng.integers(1, 4)))
                      for ns in rng.permutation(30)[: rng.integers(5, 31)]) + "\n" for _ in range(40)]
    pf = Predictor(f"fw -i {c.q} -t --foreground")
    pp = Predictor(f"fw -i {c.q} -t --foreground --packed_weights")
    try:
        want = pf.predict_batch(lines)
        got = pp.predict_batch(lines)
        assert np.std(want) > 0.01 and np.abs(got - want).max() < PRED_TOL, np.abs(got - want).max()
        # the one-line calls: the line as an entry batch of one; with a context set the whole context + candidate line (no cache on packed weights)
        one = np.array([pp.predict(s) for s in lines[:5]])
        assert np.abs(one - want[:5]).max() < PRED_TOL, (one, want[:5])
        context, cands = "|N00 11 12 |N01 13:0.5 \n", [s for s in lines if "|N00" not in s and "|N01" not in s][:5]
        assert len(cands) == 5 and pf.setup_cache(context) == 0.0 and pp.setup_cache(context) == 0.0
        cw, cg = (np.array([q.predict_with_cache(s) for s in cands]) for q in (pf, pp))
        assert cw.min() > 0.0 and np.abs(cg - cw).max() < PRED_TOL, (cg, cw)
    finally:
        pf.close()
        pp.close()
