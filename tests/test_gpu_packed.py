"""Packed FFM weights on the device (fwgpu_model_load_packed): the quantised inference file's f16 bucket numbers stay two bytes per weight in
device memory and the predict kernel converts them while it gathers -- w = min + f32(bucket) * increment, bit for bit the host's
dequantize_ffm_weights (quantization.rs:82-98).  Conversion on every f16 pattern, size, predictions against the CPU oracle holding the very
weights the buckets stand for, refusals, and the serving FFI."""
import struct

import numpy as np
import pytest

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import capi
from fwumious_wabbit_amd import persistence as P
from fwumious_wabbit_amd.feed import VowpalParser, VwNamespaceMap
from helpers import make_pair, logloss, record_labels
from oracle import fwo

pytestmark = pytest.mark.gpu

PRED_TOL = 1e-5      # tests/test_gpu_parity.py: |p_gpu - p_ref| on a single prediction (f32 summation-order noise)
LOGLOSS_TOL = 1e-4   # ... and the per-example log-loss tolerance
CACHE_TOL = 5e-6     # the reference's assert_epsilon! (block_helpers.rs:30-40) between cached and plain routes

VW6 = "".join(f"A{i},ns{i}\n" for i in range(6))


def _vwmap(n):
    return VwNamespaceMap("".join(f"N{i:02d},ns{i}\n" for i in range(n)))


def _trained(opt=fw.Optimizer.AdagradLUT, n=600, seed=31, nn=False, k=4):
    mi, _, _ = make_pair(6, k, 12, 12, opt, lr=0.05, ffm_lr=0.05)
    if nn:
        mi.nn_layers = [dict(width="9", activation="relu"), dict(width="5", activation="relu", init="xavier")]
    recs, off = fw.synth_records(6, 1.0, 1.1, 3000, 0.2, seed, 0, n)
    re = fw.Regressor(mi)
    b = re.record_batch(fw.FeatureBufferTranslator(mi), recs, off)
    re.learn_batch(b, capi.MODE_SEQUENTIAL, True)
    b.close()
    return mi, re, recs, off


def _predict_all(re, mi, recs, off, mode=capi.MODE_SEQUENTIAL, records=True):
    fbt = fw.FeatureBufferTranslator(mi)
    b = re.record_batch(fbt, recs, off) if records else re.batch_from_records(fbt, recs, off)
    re.learn_batch(b, mode, False)
    p = b.predictions().copy()
    b.close()
    return p


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ 4. the conversion, on every f16 bit pattern
@pytest.mark.parametrize("inc,mn", [(3.0517578e-05, -0.731), (1.7e-3, 0.0421)])
def test_every_f16_bucket_pattern_converts_like_the_host(tmp_path, inc, mn):
    mi, _, _ = make_pair(4, 4, 10, 16, fw.Optimizer.AdagradLUT)
    vw = _vwmap(4)
    re = fw.Regressor(mi)
    n = re.table_len(capi.TABLE_FFM_W)
    assert n == 65536 + 16
    t, q = str(tmp_path / "t.fw"), str(tmp_path / "q.fw")
    P.save_regressor_to_filename(t, mi, vw, re)
    P.convert_inference_regressor(t, q, quantize_weights=True)
    re.close()
    # the file ends with the FFM block: 8-byte header {increment, min}, then one f16 bucket number per weight
    raw = bytearray(open(q, "rb").read())
    at = len(raw) - (8 + 2 * n)
    blob = bytearray(raw[at:])
    blob[0:8] = struct.pack("<ff", inc, mn)
    blob[8:8 + 2 * 65536] = np.arange(65536, dtype="<u2").tobytes()
    raw[at:] = blob
    open(q, "wb").write(bytes(raw))
    want = P.dequantize_ffm_weights(bytes(blob), n)
    _, _, rp = P.new_regressor_from_filename(q, immutable=True, packed=True)
    assert rp.ffm_storage()[0] == capi.FFM_F16_BUCKETS
    got = rp.table_read(capi.TABLE_FFM_W)
    assert got.shape == want.shape
    pat = np.arange(65536, dtype=np.uint32)
    is_nan = ((pat >> 10) & 31 == 31) & ((pat & 0x3ff) != 0)
    assert int(is_nan.sum()) == 2046
    ok = np.ones(n, dtype=bool)
    ok[:65536] = ~is_nan
    assert np.array_equal(_bits(got)[ok], _bits(want)[ok])            # every pattern that is no NaN, and the tail: bit for bit
    assert np.isnan(got[:65536][is_nan]).all() and np.isnan(want[:65536][is_nan]).all()
    assert np.isinf(got[0x7c00]) and np.isinf(got[0xfc00]) and got[0x7c00] > 0 > got[0xfc00]
    assert got[0] == np.float32(mn) and _bits(got[1:2])[0] == _bits(want[1:2])[0]  # zero, and the smallest subnormal
    # a sub-range read goes through the same routine
    assert np.array_equal(_bits(rp.table_read(capi.TABLE_FFM_W, 1021, 4099)), _bits(got[1021:1021 + 4099]))
    rp.close()


# ------------------------------------------------------------------ 5. / 7. same file, two loads; an unquantised file loaded packed
def test_same_quantised_file_loaded_f32_and_packed(tmp_path):
    vw = VwNamespaceMap(VW6)
    mi, re, recs, off = _trained(seed=51)
    t, q = str(tmp_path / "t.fw"), str(tmp_path / "q.fw")
    P.save_regressor_to_filename(t, mi, vw, re)
    P.convert_inference_regressor(t, q, quantize_weights=True)
    mi_f, _, rf = P.new_regressor_from_filename(q, immutable=True)
    mi_p, _, rp = P.new_regressor_from_filename(q, immutable=True, packed=True)
    assert mi_p == mi_f and mi_p.optimizer == fw.Optimizer.SGD
    n = rp.table_len(capi.TABLE_FFM_W)
    assert n == rf.table_len(capi.TABLE_FFM_W)
    assert np.array_equal(_bits(rp.table_read(capi.TABLE_FFM_W)), _bits(rf.table_read(capi.TABLE_FFM_W)))
    assert np.array_equal(rp.table_read(capi.TABLE_LR), rf.table_read(capi.TABLE_LR))
    assert rp.table_checksum(capi.TABLE_FFM_W) == rf.table_checksum(capi.TABLE_FFM_W)
    st, nb = rp.ffm_storage()
    assert st == capi.FFM_F16_BUCKETS and 2 * n <= nb <= 2 * n + 4096
    st, nb = rf.ffm_storage()
    assert st == capi.FFM_F32 and 4 * n <= nb <= 4 * n + 4096
    # 7: a training file loaded packed holds what the conversion with quantize_weights would have written
    _, _, rt = P.new_regressor_from_filename(t, immutable=True, packed=True)
    assert np.array_equal(_bits(rt.table_read(capi.TABLE_FFM_W)), _bits(rp.table_read(capi.TABLE_FFM_W)))
    assert np.array_equal(rt.table_read(capi.TABLE_LR), rp.table_read(capi.TABLE_LR))
    # ... and so does an unquantised inference file
    u = str(tmp_path / "u.fw")
    P.convert_inference_regressor(t, u)
    _, _, ru = P.new_regressor_from_filename(u, immutable=True, packed=True)
    assert np.array_equal(_bits(ru.table_read(capi.TABLE_FFM_W)), _bits(rp.table_read(capi.TABLE_FFM_W)))
    p_f = _predict_all(rf, mi_f, recs, off)
    for x in (rp, rt, ru):
        assert np.abs(_predict_all(x, mi_p, recs, off) - p_f).max() < PRED_TOL
    for x in (re, rf, rp, rt, ru):
        x.close()


# ------------------------------------------------------------------ 6. predictions against the oracle
@pytest.mark.parametrize("fields,k,ffm_only", [(30, 8, False), (10, 4, False), (30, 16, False), (30, 8, True)],
                         ids=["k8x30", "k4x10", "k16x30", "k8x30-ffm-only"])
def test_packed_predictions_match_the_oracle_on_the_weights_the_buckets_stand_for(tmp_path, fields, k, ffm_only):
    mi, ocfg, ots = make_pair(fields, k, 18, 18, fw.Optimizer.AdagradLUT)
    recs, off = fw.synth_records(fields, 5.67, 1.05, 100000, 0.1, 21, 0, 600)
    y = record_labels(recs, off)
    om = fwo.Model(ocfg)
    om.run_stream(ots, recs[: int(off[300])], off[:301], nthreads=1)  # train the oracle on the first half
    re = fw.Regressor(mi)
    re.table_write(capi.TABLE_LR, om.lr_table)
    re.table_write(capi.TABLE_FFM_W, om.ffm_weights)
    re.table_write(capi.TABLE_FFM_ACC, om.ffm_acc)
    w_full = re.table_read(capi.TABLE_FFM_W)
    t, q = str(tmp_path / "t.fw"), str(tmp_path / "q.fw")
    P.save_regressor_to_filename(t, mi, _vwmap(fields), re)
    P.convert_inference_regressor(t, q, quantize_weights=True)
    re.close()
    mi_p, _, rp = P.new_regressor_from_filename(t, immutable=True, packed=True)
    mi_f, _, rf = P.new_regressor_from_filename(q, immutable=True)
    assert rp.ffm_storage()[0] == capi.FFM_F16_BUCKETS
    # the oracle predicts with exactly the weights the packed table stands for
    dq = P.dequantize_ffm_weights(P.quantize_ffm_weights(w_full), w_full.size)
    assert np.array_equal(_bits(rp.table_read(capi.TABLE_FFM_W)), _bits(dq))
    if ffm_only:
        ocfg.wiring = fwo.WIRING_FFM_ONLY
        om2 = fwo.Model(ocfg)
        om2.lr_table[:] = om.lr_table
        om2.ffm_acc[:] = om.ffm_acc
        om = om2
        rp.set_wiring(capi.WIRING_FFM_ONLY)
        rf.set_wiring(capi.WIRING_FFM_ONLY)
    om.ffm_weights[:] = dq[: len(om.ffm_weights)]
    p_ref = np.zeros(600, dtype=np.float32)
    for i in range(600):
        lr, ffm, _, _ = ots.translate(recs[int(off[i]):int(off[i + 1])])
        p_ref[i] = om.predict(lr, ffm)
    assert 0.02 < p_ref.std()  # (a model that says something)
    fbt = fw.FeatureBufferTranslator(mi_p)
    bit_equal = True
    for kind in ("entries", "records"):
        b = rp.batch_from_records(fbt, recs, off) if kind == "entries" else rp.record_batch(fbt, recs, off)
        bf = rf.batch_from_records(fbt, recs, off) if kind == "entries" else rf.record_batch(fbt, recs, off)
        for mode in (capi.MODE_HOGWILD, capi.MODE_SEQUENTIAL):
            rp.learn_batch(b, mode, False)
            assert rp.last_launch()["family"] == capi.KERNEL_PACKED
            p = b.predictions().copy()
            print(f"{kind} mode {mode}: max |p_packed - p_oracle| = {np.abs(p - p_ref).max():.3e}, "
                  f"max |d logloss| = {np.abs(logloss(p, y) - logloss(p_ref, y)).max():.3e}")
            assert np.abs(p - p_ref).max() < PRED_TOL
            assert np.abs(logloss(p, y) - logloss(p_ref, y)).max() < LOGLOSS_TOL
            rp.learn_batch(b, mode, False)
            assert np.array_equal(b.predictions(), p)  # two identical launches
            rf.learn_batch(bf, mode, False)
            assert rf.last_launch()["family"] == capi.KERNEL_RESIDENT
            pf = bf.predictions().copy()
            assert np.abs(p - pf).max() < PRED_TOL   # the f32 load of the same quantised model
            bit_equal = bit_equal and np.array_equal(p, pf)
        b.close()
        bf.close()
    print("packed == f32 load of the quantised file, bit for bit:", bit_equal)
    # single-example calls take the same kernel
    for i in (0, 7, 599):
        fb = fbt.translate(recs[int(off[i]):int(off[i + 1])])
        assert abs(rp.predict(fb) - p_ref[i]) < PRED_TOL
        assert abs(rp.learn(fb, None, False) - p_ref[i]) < PRED_TOL
    rp.close()
    rf.close()


# ------------------------------------------------------------------ 8. refusals
def test_everything_that_would_write_or_train_is_refused_and_leaves_the_regressor_usable(tmp_path):
    vw = VwNamespaceMap(VW6)
    mi, re, recs, off = _trained(seed=71)
    t = str(tmp_path / "t.fw")
    P.save_regressor_to_filename(t, mi, vw, re)
    mi_p, _, rp = P.new_regressor_from_filename(t, immutable=True, packed=True)
    fbt = fw.FeatureBufferTranslator(mi_p)
    p0 = _predict_all(rp, mi_p, recs, off)
    fb = fbt.translate(recs[int(off[3]):int(off[4])])
    fb.label, fb.example_importance = 1.0, 1.0
    b = rp.record_batch(fbt, recs, off)
    be = rp.batch_from_records(fbt, recs, off)
    split = rp.split_buffers(len(off) - 1)
    n = rp.table_len(capi.TABLE_FFM_W)
    blob = re.write_weights_to_buf()

    def trainer():
        fw.regressor.HogwildTrainer(rp, mi_p)

    def dist_group():
        from fwumious_wabbit_amd.dist import DistGroup
        DistGroup([rp])

    refused = {
        "learn(update=1)": lambda: rp.learn(fb, None, True),
        "learn_batch(update=1), records": lambda: rp.learn_batch(b, capi.MODE_HOGWILD, True),
        "learn_batch(update=1), entries, in order": lambda: rp.learn_batch(be, capi.MODE_SEQUENTIAL, True),
        "learn_batch_sync": lambda: rp.learn_batch_sync(be, split),
        "table_write FFM_W": lambda: rp.table_write(capi.TABLE_FFM_W, np.zeros(8, dtype=np.float32)),
        "table_write FFM_ACC": lambda: rp.table_write(capi.TABLE_FFM_ACC, np.zeros(8, dtype=np.float32)),
        "table_fill FFM_W": lambda: rp.table_fill(capi.TABLE_FFM_W, 0.5),
        "table_fill FFM_ACC": lambda: rp.table_fill(capi.TABLE_FFM_ACC, 0.5),
        "table_device_ptr FFM_W": lambda: rp.table_device_ptr(capi.TABLE_FFM_W),
        "read_weights": lambda: rp.overwrite_weights_from_buf(blob),
        "write_weights": lambda: rp.write_weights_to_buf(),
        "model_save": lambda: P.save_regressor_to_filename(str(tmp_path / "no.fw"), mi_p, vw, rp),
        "trainer_create": trainer,
        "dist group": dist_group,
        "hogwild_load": lambda: P.hogwild_load(rp, t),
        "setup_cache": lambda: rp.setup_cache(fb),
        "allocate_and_init_weights": lambda: rp.allocate_and_init_weights(),
    }
    for what, call in refused.items():
        with pytest.raises(capi.FwgpuError) as e:
            call()
        assert e.value.code == capi.ERR_INVALID, (what, str(e.value))
        assert "packed" in e.value.message, (what, e.value.message)
        assert np.array_equal(_predict_all(rp, mi_p, recs, off), p0), what
    assert rp.table_len(capi.TABLE_FFM_W) == n and rp.ffm_storage()[0] == capi.FFM_F16_BUCKETS
    # the shape this form refuses at the launch: raw entries that did not pass the translator's mask (a row must start on a multiple of 4 buckets)
    raw = fw.lr_and_ffm_vec([(5, 1.0, 0)], [(8, 1.0, 0), (22, 1.0, 4)])
    with pytest.raises(capi.FwgpuError) as e:
        rp.predict(raw)
    assert e.value.code == capi.ERR_INVALID and "multiple of 4" in e.value.message
    assert np.array_equal(_predict_all(rp, mi_p, recs, off), p0)
    assert np.array_equal(_predict_all(rp, mi_p, recs, off, capi.MODE_HOGWILD, records=False), _predict_all(rp, mi_p, recs, off, capi.MODE_HOGWILD, records=False))
    for x in (b, be):
        x.close()
    split.close()
    rp.close()
    re.close()


def test_shapes_the_packed_form_does_not_serve_are_refused_when_it_is_created(tmp_path):
    vw = VwNamespaceMap(VW6)
    # a deep head
    mi, re, _, _ = _trained(opt=fw.Optimizer.AdagradFlex, nn=True, n=50)
    t = str(tmp_path / "head.fw")
    P.save_regressor_to_filename(t, mi, vw, re)
    re.close()
    with pytest.raises(capi.FwgpuError) as e:
        P.new_regressor_from_filename(t, immutable=True, packed=True)
    assert e.value.code == capi.ERR_INVALID and "deep head" in e.value.message
    # ffm_k = 10 (config A): rows are not made of 8-byte groups of buckets
    mi, re, _, _ = _trained(n=50, k=10)
    t = str(tmp_path / "k10.fw")
    P.save_regressor_to_filename(t, mi, vw, re)
    re.close()
    with pytest.raises(capi.FwgpuError) as e:
        P.new_regressor_from_filename(t, immutable=True, packed=True)
    assert e.value.code == capi.ERR_INVALID and "multiple of 4" in e.value.message
    # no FFM block at all
    mi, _, _ = make_pair(6, 0, 12, 12, fw.Optimizer.AdagradLUT)
    re = fw.Regressor(mi)
    t = str(tmp_path / "lr.fw")
    P.save_regressor_to_filename(t, mi, vw, re)
    re.close()
    with pytest.raises(capi.FwgpuError) as e:
        P.new_regressor_from_filename(t, immutable=True, packed=True)
    assert e.value.code == capi.ERR_INVALID
    # ... while the plain load of each still works
    _, _, r2 = P.new_regressor_from_filename(t, immutable=True)
    assert r2.ffm_storage() == (capi.FFM_F32, 0)
    r2.close()


# ------------------------------------------------------------------ 9. serving
def test_serving_ffi_with_packed_weights(tmp_path):
    from fwumious_wabbit_amd.serving import Predictor
    vw = VwNamespaceMap(VW6)
    mi, re, recs, off = _trained(seed=61)
    path = str(tmp_path / "model.fw")
    P.save_regressor_to_filename(path, mi, vw, re)
    re.close()
    mi_p, _, rp = P.new_regressor_from_filename(path, immutable=True, packed=True)
    pr = Predictor(f"fw -i {path} -t --foreground --packed_weights")
    parser = VowpalParser(vw)
    fbt = fw.FeatureBufferTranslator(mi_p)
    rng = np.random.default_rng(5)

    def feats(ns):
        return f"|A{ns} " + " ".join(f"{rng.integers(0, 3000)}" + (f":{rng.random() * 2:.3f}" if rng.random() < 0.3 else "")
                                      for _ in range(rng.integers(1, 4)))

    lines = [" ".join(feats(ns) for ns in rng.permutation(6)[: rng.integers(2, 7)]) + "\n" for _ in range(64)]

    def own(line):
        return rp.predict(fbt.translate(parser.next_vowpal(line.encode())))

    want = np.array([own(l) for l in lines], dtype=np.float32)
    assert 0.01 < want.std()
    assert np.array_equal(np.array([pr.predict(l) for l in lines], dtype=np.float32), want)
    assert np.array_equal(pr.predict_batch(lines), want)
    ctx = "|A0 17 23:0.5 |A1 99 "
    cands = [f"|A2 {i} |A3 {i * 7}:1.5 |A5 {i % 3}\n" for i in range(40)]
    whole = np.array([own(ctx + c) for c in cands], dtype=np.float32)
    assert np.array_equal(np.array([pr.predict(ctx + c) for c in cands], dtype=np.float32), whole)
    assert pr.setup_cache(ctx + "\n") == 0.0
    with_cache = np.array([pr.predict_with_cache(c) for c in cands], dtype=np.float32)
    assert np.abs(with_cache - whole).max() < CACHE_TOL
    assert np.abs(pr.predict_batch(cands, with_cache=True) - whole).max() < CACHE_TOL
    assert np.array_equal(pr.predict_batch([ctx + c for c in cands], with_cache=False), whole)
    big = [f"|A2 {i} {i + 1}:0.5 |A3 {i * 7}:1.5 |A4 {i % 11} |A5 {i % 3}\n" for i in range(600)]  # several parser threads
    assert np.abs(pr.predict_batch(big, with_cache=True) - np.array([own(ctx + c) for c in big], dtype=np.float32)).max() < CACHE_TOL
    # a clone_lite copy shares the packed table and predicts the same bits
    cl = pr.clone_lite()
    assert np.array_equal(np.array([cl.predict(l) for l in lines], dtype=np.float32), want)
    assert cl.setup_cache(ctx + "\n") == 0.0
    assert np.array_equal(np.array([cl.predict_with_cache(c) for c in cands], dtype=np.float32), with_cache)
    assert np.array_equal(cl.predict_batch(lines), want)
    cl.close()
    pr.close()
    rp.close()


# ------------------------------------------------------------------ 10. every shape the packed form accepts, per example against float64
PACKED_SHAPES = [(6, 4), (30, 8),                        # one chunk
                 (20, 12), (21, 12), (12, 20), (10, 24),  # k no power of two: a real division in the packed gather; 21 x 12: the last lane partly filled
                 (8, 32), (2, 128),                      # a full single chunk (256 buckets)
                 (16, 32), (4, 128), (5, 64),            # two chunks: full, full, nearly empty (320 buckets)
                 (30, 16), (40, 8)]                      # shapes the stream tests run


@pytest.mark.parametrize("F,k", PACKED_SHAPES, ids=[f"{F}x{k}" for F, k in PACKED_SHAPES])
def test_packed_predictions_per_example_against_float64(F, k):
    """Regressor.pack() of the shape's warm state (tests/ffm_ref.py: probe_stream, warm_state, as test_gpu_ffm_step.py's predict-only case), then
    predict-only launches of the packed regressor from entry and record batches, concurrent and in order: every prediction within
    min(C_P * M_p + 4 ulp, 5e-5) of the float64 forward pass (ffm_ref.judge_prediction) on the values the buckets stand for -- the packed
    regressor's own table_read -- and the source's LR table."""
    from types import SimpleNamespace

    import ffm_ref
    from helpers import check_disjoint, disjoint_models

    st = ffm_ref.probe_stream(F, k)
    mi, _, _ = disjoint_models(st, ffm_ref.LUT)
    check_disjoint(st, mi)
    re = fw.Regressor(mi)
    rp = None
    try:
        for t, v in zip((capi.TABLE_FFM_W, capi.TABLE_FFM_ACC, capi.TABLE_LR), ffm_ref.warm_state(st)):
            re.table_write(t, v)
        rp = re.pack()
        assert rp.ffm_storage()[0] == capi.FFM_F16_BUCKETS
        w, lr = rp.table_read(capi.TABLE_FFM_W), re.table_read(capi.TABLE_LR)
        assert np.array_equal(_bits(rp.table_read(capi.TABLE_LR)[0::2]), _bits(lr[0::2]))  # (the weights; an immutable regressor keeps no accumulators)
        assert not np.array_equal(_bits(w), _bits(re.table_read(capi.TABLE_FFM_W)))  # (the buckets' values, not the source's)
        cfg = SimpleNamespace(F=F, k=k)
        ref = [ffm_ref.predict(cfg, w, lr, fb.lr_buffer, fb.ffm_buffer) for fb in st.fbs]
        assert np.std([r[0] for r in ref]) > 0.02  # (a model that says something)
        fbt = fw.FeatureBufferTranslator(rp.mi)
        for route in ("entries", "records"):
            b = rp.batch(st.fbs) if route == "entries" else rp.record_batch(fbt, st.recs, st.off)
            try:
                for mode in (capi.MODE_HOGWILD, capi.MODE_SEQUENTIAL):
                    rp.learn_batch(b, mode, False)
                    info = rp.last_launch()
                    assert info["family"] == capi.KERNEL_PACKED and info["chunks"] == (1 if F * k <= 256 else 2), info
                    p = b.predictions().copy()
                    worst = 0.0
                    for e in range(st.n):
                        err, bound, need = ffm_ref.judge_prediction(p[e], *ref[e])
                        worst = max(worst, need)
                        assert err <= bound, (route, mode, e, float(p[e]), ref[e], err, bound, need, ffm_ref.C_P)
                    print(f"PACKEDPREDICT {F}x{k} {route} mode {mode}: needs c_p = {worst:.3e} = {worst / ffm_ref.C_P:.3f} C_P")
            finally:
                b.close()
    finally:
        if rp is not None:
            rp.close()
        re.close()
