"""The byte diff of published inference models on the device (csrc/patch.hip) and what is built on it: fwgpu_image_*, fwgpu_image_diff,
fwgpu_packed_apply_diff, fwgpu_predictor_apply_diff.  Every result is defined byte for byte by host code: the stream by the host codec
(fwgpu_diff_bytes, itself held to the reference's known answers in tests/test_diff_stream_cpu.py), an image by the file
fwgpu_model_save_inference writes, a patched regressor by fwgpu_model_load_packed of the next file.  So every comparison is equality."""
import numpy as np
import pytest

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import capi
from fwumious_wabbit_amd import persistence as P
import publish_cases as K

pytestmark = pytest.mark.gpu

OPTIMIZERS = [fw.Optimizer.SGD, fw.Optimizer.AdagradFlex, fw.Optimizer.AdagradLUT]
OPT_IDS = ["SGD", "AdagradFlex", "AdagradLUT"]


@pytest.fixture(scope="module")
def tile():
    t = P.debug_diff_geometry()
    assert t >= 64 and t % 16 == 0
    return t


def _check(a, b, name):
    """the kernels' stream for every offset: the host codec's bytes, the count, and the same bytes again"""
    a, b = a.tobytes(), b.tobytes()
    count = sum(x != y for x, y in zip(a, b)) if len(a) < 100000 else int((np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8)).sum())
    for base, prev in K.OFFSETS:
        want, want_changed = P.diff_bytes(a, b, base, prev, with_changed=True)
        got, changed = P.debug_diff(a, b, base, prev)
        assert want_changed == count
        assert changed == count, (name, len(a), base)
        if got != want:
            first = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
            raise AssertionError(f"{name}, n = {len(a)}, base_offset = {base}: {len(got)} bytes vs {len(want)}, first difference at stream byte {first}")
        assert P.debug_diff(a, b, base, prev) == (got, changed), (name, len(a), base)  # (the same bytes when called twice)
    return want


# ------------------------------------------------------------------ 1. the kernels against the host codec
@pytest.mark.parametrize("which", range(9))
def test_kernels_give_the_host_codecs_stream(tile, which):
    n = K.lengths(tile)[which]
    for name, a, b in K.patterns(n, tile):
        stream = _check(a, b, name)
        if name == "none":
            assert stream == b""
        if name == "all" and n:
            assert len(stream) >= 2 * n


def test_prev_is_carried_across_empty_tiles(tile):
    a, b = K.carried_prev(tile)
    assert len(P.diff_bytes(a.tobytes(), b.tobytes())) == 2 + (4 if 40 * tile < 2**21 else 5)  # delta 5, and a delta of 40 tiles
    _check(a, b, "carried-prev")


def test_a_gap_beyond_2_to_21_takes_a_four_byte_varint(tile):
    a, b = K.long_gap(tile)
    stream = P.diff_bytes(a.tobytes(), b.tobytes())
    assert len(stream) == 2 + 5
    _check(a, b, "long-gap")


# ------------------------------------------------------------------ 2. image = file
@pytest.mark.parametrize("opt,nn", [(fw.Optimizer.SGD, False), (fw.Optimizer.AdagradFlex, False), (fw.Optimizer.AdagradLUT, False),
                                    (fw.Optimizer.AdagradFlex, True)], ids=OPT_IDS + ["two-layer-head"])
def test_an_image_reads_as_the_file_save_inference_writes(tmp_path, opt, nn):
    vw = K.vwmap()
    mi, re = K.model(opt, nn=nn)
    tables = (capi.TABLE_LR, capi.TABLE_FFM_W)
    before = [re.table_checksum(t) for t in tables]
    for quantize in (True, False):
        path = str(tmp_path / f"inference{int(quantize)}.fw")
        P.save_inference_regressor(path, mi, vw, re, quantize_weights=quantize)
        want = open(path, "rb").read()
        img = P.Image.capture(mi, vw, re, quantize_weights=quantize)
        got = img.read()
        assert sum(img.lengths()) == len(want)
        assert got == want, f"quantize = {quantize}: first difference at byte {next(i for i in range(len(want)) if got[i] != want[i])}"
        loaded = P.Image.load(path)
        assert loaded.lengths() == img.lengths()
        assert loaded.read() == want
        assert img.diff(loaded) == b""
        img.close()
        loaded.close()
    assert [re.table_checksum(t) for t in tables] == before
    K.train(re, mi, *K.records(50, first=300))  # the source still trains
    assert re.table_checksum(capi.TABLE_FFM_W) != before[1]
    re.close()


def test_image_refusals(tmp_path):
    vw = K.vwmap()
    mi, re = K.model(n=50)
    rp = re.pack()
    with pytest.raises(capi.FwgpuError) as e:
        P.Image.capture(rp.mi, vw, rp, quantize_weights=True)
    assert e.value.code == capi.ERR_INVALID and "packed" in e.value.message
    mi2, re2 = K.model(bits=12, n=50)
    a, b = P.Image.capture(mi, vw, re, True), P.Image.capture(mi2, vw, re2, True)
    with pytest.raises(capi.FwgpuError) as e:
        a.diff(b)
    assert e.value.code == capi.ERR_INVALID and "lengths" in e.value.message
    t = str(tmp_path / "training.fw")
    P.save_regressor_to_filename(t, mi, vw, re)
    with pytest.raises(capi.FwgpuError) as e:
        P.Image.load(t)
    assert e.value.code == capi.ERR_INVALID and "inference" in e.value.message
    for x in (a, b, re, re2, rp):
        x.close()


# ------------------------------------------------------------------ 3. diff end to end; 4. hot patch
@pytest.fixture(scope="module")
def two_publishes(tmp_path_factory):
    """file 0 and file 1 of one trainer, 40 examples apart, with the quantiser's extremes pinned; their images' diff"""
    d = tmp_path_factory.mktemp("publish")
    vw = K.vwmap()
    mi, re, (recs, off) = K.pinned_model()
    f0, f1 = str(d / "publish0.fw"), str(d / "publish1.fw")
    P.save_inference_regressor(f0, mi, vw, re, quantize_weights=True)
    img0 = P.Image.capture(mi, vw, re, quantize_weights=True)
    K.train(re, mi, recs, off)
    P.save_inference_regressor(f1, mi, vw, re, quantize_weights=True)
    img1 = P.Image.capture(mi, vw, re, quantize_weights=True)
    stream, changed = img0.diff(img1, with_changed=True)
    out = dict(mi=mi, f0=f0, f1=f1, bytes0=open(f0, "rb").read(), bytes1=open(f1, "rb").read(), stream=stream, changed=changed,
               header_bytes=img0.lengths()[0], records=K.records(200, first=1000))
    assert img0.read() == out["bytes0"] and img1.read() == out["bytes1"]
    for x in (img0, img1, re):
        x.close()
    return out


def test_image_diff_is_the_host_codecs_stream_of_the_two_files(two_publishes):
    t = two_publishes
    b0, b1 = t["bytes0"], t["bytes1"]
    want, want_changed = P.diff_bytes(b0, b1, with_changed=True)
    # the case is not vacuous, by the host codec on the two files alone: something changed, less than half the bucket bytes, the header stayed
    mi = t["mi"]
    lr_bytes, n_ffm = 4 << mi.bit_precision, (1 << mi.ffm_bit_precision) + 6 * 4
    q_at = t["header_bytes"] + lr_bytes
    assert len(b0) == len(b1) == q_at + 8 + 2 * n_ffm
    assert b0[q_at: q_at + 8] == b1[q_at: q_at + 8]
    assert b0[: t["header_bytes"]] == b1[: t["header_bytes"]]
    assert 0 < want_changed < n_ffm  # (half of the 2 n_ffm bucket bytes)
    assert P.apply_diff_bytes(b0, want) == b1
    # the device route
    assert t["changed"] == want_changed
    assert t["stream"] == want
    assert P.apply_diff_bytes(b0, t["stream"]) == b1


def _same_packed(a, b, mi, recs, off):
    assert a.ffm_storage() == b.ffm_storage() and a.ffm_storage()[0] == capi.FFM_F16_BUCKETS
    assert np.array_equal(K.bits(a.table_read(capi.TABLE_FFM_W)), K.bits(b.table_read(capi.TABLE_FFM_W)))
    assert np.array_equal(K.bits(a.table_read(capi.TABLE_LR)), K.bits(b.table_read(capi.TABLE_LR)))
    pa, pb = K.predictions(a, mi, recs, off), K.predictions(b, mi, recs, off)
    assert np.array_equal(pa, pb)
    assert 0.005 < pa.std()  # (a model that says something)
    return pa


def test_hot_patch_equals_the_packed_load_of_the_next_file(two_publishes):
    t = two_publishes
    recs, off = t["records"]
    mi_p, _, r0 = P.new_regressor_from_filename(t["f0"], immutable=True, packed=True)
    _, _, r1 = P.new_regressor_from_filename(t["f1"], immutable=True, packed=True)
    p0 = K.predictions(r0, mi_p, recs, off)
    assert r0.apply_diff(b"") == 0  # an empty stream changes nothing
    assert np.array_equal(K.predictions(r0, mi_p, recs, off), p0)
    assert r0.apply_diff(t["stream"]) == t["changed"]
    p1 = _same_packed(r0, r1, mi_p, recs, off)
    assert not np.array_equal(p0, p1)  # (the 40 examples moved the model)
    r0.close()
    r1.close()


def test_hot_patch_when_the_quantisers_header_moves(tmp_path):
    vw = K.vwmap()
    mi, re = K.model(n=300)
    f0, f1 = str(tmp_path / "a.fw"), str(tmp_path / "b.fw")
    P.save_inference_regressor(f0, mi, vw, re, quantize_weights=True)
    img0 = P.Image.capture(mi, vw, re, quantize_weights=True)
    re.table_write(capi.TABLE_FFM_W, [5.0], offset=1001)  # a new maximum: the increment moves and with it nearly every bucket
    P.save_inference_regressor(f1, mi, vw, re, quantize_weights=True)
    img1 = P.Image.capture(mi, vw, re, quantize_weights=True)
    stream, changed = img0.diff(img1, with_changed=True)
    b0, b1 = open(f0, "rb").read(), open(f1, "rb").read()
    assert stream == P.diff_bytes(b0, b1)
    n_ffm = (1 << mi.ffm_bit_precision) + 6 * 4
    q_at = img0.lengths()[0] + (4 << mi.bit_precision)
    assert b0[q_at: q_at + 8] != b1[q_at: q_at + 8]
    assert changed > n_ffm  # more than half of the bucket bytes: the case to ship the file instead
    recs, off = K.records(200, first=1000)
    mi_p, _, r0 = P.new_regressor_from_filename(f0, immutable=True, packed=True)
    _, _, r1 = P.new_regressor_from_filename(f1, immutable=True, packed=True)
    assert r0.apply_diff(stream) == changed
    _same_packed(r0, r1, mi_p, recs, off)  # (equal only if q_increment and q_min were patched too)
    for x in (img0, img1, re, r0, r1):
        x.close()


# ------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_regressor_predicting_the_same_bits(two_publishes, tmp_path):
    t = two_publishes
    recs, off = t["records"]
    vw = K.vwmap()

    def refused(r, mi, stream, code, word):
        before = K.predictions(r, mi, recs, off)
        with pytest.raises(capi.FwgpuError) as e:
            r.apply_diff(stream)
        assert e.value.code == code and word in e.value.message, e.value.message
        assert np.array_equal(K.predictions(r, mi, recs, off), before), word

    # regressors that have no quantised file's bytes behind them
    mi_f, _, rf = P.new_regressor_from_filename(t["f0"], immutable=True)
    refused(rf, mi_f, t["stream"], capi.ERR_INVALID, "f32")
    mi, re = K.model(bits=16, n=100)
    rp = re.pack()
    refused(rp, rp.mi, t["stream"], capi.ERR_INVALID, "fwgpu_pack_regressor")
    plain = str(tmp_path / "plain.fw")
    P.save_inference_regressor(plain, mi, vw, re, quantize_weights=False)
    mi_q, _, rq = P.new_regressor_from_filename(plain, immutable=True, packed=True)
    refused(rq, mi_q, t["stream"], capi.ERR_INVALID, "quantised at load")
    # streams
    mi_p, _, r0 = P.new_regressor_from_filename(t["f0"], immutable=True, packed=True)
    refused(r0, mi_p, bytes([3, 0x55]) + t["stream"][:0], capi.ERR_INVALID, "the model's header changed: load the file")
    refused(r0, mi_p, t["stream"][:-1], capi.ERR_FORMAT, "ends inside an entry")
    beyond = P.diff_bytes(b"\0", b"\1", base_offset=len(t["bytes0"]))  # one entry at the file's length
    refused(r0, mi_p, beyond, capi.ERR_FORMAT, "beyond")
    # ... and the patch that IS allowed still goes through afterwards
    assert r0.apply_diff(t["stream"]) == t["changed"]
    _, _, r1 = P.new_regressor_from_filename(t["f1"], immutable=True, packed=True)
    _same_packed(r0, r1, mi_p, recs, off)
    for x in (rf, re, rp, rq, r0, r1):
        x.close()


# ------------------------------------------------------------------ 6. serving
def test_serving_predictors_see_the_patch(two_publishes):
    from fwumious_wabbit_amd.serving import Predictor
    t = two_publishes
    rng = np.random.default_rng(5)

    def feats(ns):
        return f"|A{ns} " + " ".join(f"{rng.integers(0, 3000)}" + (f":{rng.random() * 2:.3f}" if rng.random() < 0.3 else "")
                                      for _ in range(rng.integers(1, 4)))

    lines = [" ".join(feats(ns) for ns in rng.permutation(6)[: rng.integers(2, 7)]) + "\n" for _ in range(48)]
    ctx = "|A0 17 23:0.5 |A1 99 "
    cands = [f"|A2 {i} |A3 {i * 7}:1.5 |A5 {i % 3}\n" for i in range(24)]

    def say(p):
        assert p.setup_cache(ctx + "\n") == 0.0
        return (np.array([p.predict(l) for l in lines], dtype=np.float32), np.array([p.predict_with_cache(c) for c in cands], dtype=np.float32),
                p.predict_batch(lines), p.predict_batch(cands, with_cache=True))

    fresh = Predictor(f"fw -i {t['f1']} -t --foreground --packed_weights")
    want = say(fresh)
    pr = Predictor(f"fw -i {t['f0']} -t --foreground --packed_weights")
    clone = pr.clone_lite()
    old = say(pr)
    say(clone)
    assert not np.array_equal(old[0], want[0])
    clone.apply_diff(t["stream"])
    for p in (pr, clone):
        for got, w in zip(say(p), want):
            assert np.array_equal(got, w)
    assert len(np.unique(want[0])) > len(lines) // 2  # (a model that tells the lines apart)
    f32 = Predictor(f"fw -i {t['f0']} -t --foreground")
    with pytest.raises(capi.FwgpuError) as e:
        f32.apply_diff(t["stream"])
    assert e.value.code == capi.ERR_INVALID and "--packed_weights" in e.value.message
    for p in (fresh, pr, clone, f32):
        p.close()
