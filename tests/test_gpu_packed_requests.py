"""Context caches and the requests route on PACKED FFM weights, on the device (fwgpu_packed_enable_caches; csrc/requests.hip: packed_cache_build_kernel and
the packed instantiation of requests_predict_kernel; serving: --packed_weights --packed_context_cache).

Per shape of packed_requests_cases.SHAPES the four caches and 96 interleaved candidates of requests_cases.case, on a packed regressor made from the
perturbed source tables by table_write + fwgpu_pack_regressor.  EVERY prediction is held to the project's bar

    |p - p_ref| <= min(C_P * M_p + 4 ulp(p), 5e-5)                      (ffm_ref.judge_prediction)

with p_ref the float64 forward pass over the WHOLE request on the values the buckets stand for: the packed regressor's own table_read(TABLE_FFM_W).
What would turn a case red is planted in float32 numpy in tests/test_packed_requests_cpu.py."""
from types import SimpleNamespace

import numpy as np
import pytest

import cache_cases as cc
import ffm_ref
import fwumious_wabbit_amd as fw
import packed_requests_cases as pq
import publish_cases as K
import requests_cases as rq
from fwumious_wabbit_amd import _capi as capi
from fwumious_wabbit_amd import persistence as P

pytestmark = pytest.mark.gpu

TABLES = (capi.TABLE_FFM_W, capi.TABLE_FFM_ACC, capi.TABLE_LR)
SHAPES = pytest.mark.parametrize("F,k", pq.SHAPES, ids=[f"{F}x{k}" for F, k in pq.SHAPES])


def _fb(lr, ffm):
    return fw.FeatureBuffer(label=0.0, example_importance=1.0, example_number=0, lr_buffer=lr, ffm_buffer=ffm)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _launch(re, b, mode=capi.MODE_HOGWILD, update=False):
    re.learn_batch(b, mode, update)
    return b.predictions().copy()


def _judge(tag, p, refs):
    assert np.all(np.isfinite(p)), tag
    worst = 0.0
    for i in range(len(p)):
        err, bound, need = ffm_ref.judge_prediction(p[i], *refs[i])
        worst = max(worst, need)
        print(f"PACKED REQUESTS {tag}, candidate {i}: p = {p[i]!r}, float64 {refs[i][0]!r}, |d| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, f"{tag}, candidate {i}: prediction {p[i]!r}, float64 {refs[i][0]!r}: |d| = {err:.3e}, bound {bound:.3e} (needs c_p = {need:.3e}, C_P = {ffm_ref.C_P:.3e})"
    print(f"PACKED REQUESTS {tag}: needs c_p = {worst:.3e} = {worst / ffm_ref.C_P:.3f} C_P")


def _refused(fn, code=capi.ERR_INVALID):
    with pytest.raises(capi.FwgpuError) as e:
        fn()
    assert e.value.code == code, e.value
    return e.value.message


class _Device:
    """the f32 source regressor on the case's perturbed tables, the packed regressor made from it (caches enabled unless told otherwise), the values its
    buckets stand for and the candidates' float64 references on them, and the four caches"""

    def __init__(self, pc, enable=True, caches=True):
        self.pc = pc
        self.src = fw.Regressor(cc.models(pc.rs))
        self.closing = []
        for t, v in zip(TABLES, (pc.src_w, pc.acc, pc.lr)):
            assert self.src.table_len(t) == len(v)
            self.src.table_write(t, v)
        self.re = self.src.pack()
        assert self.re.ffm_storage()[0] == capi.FFM_F16_BUCKETS
        if enable:
            self.re.enable_packed_caches()
        self.read_tables()
        self.caches = [self.re.setup_cache(_fb(lr, ffm)) for lr, ffm in pc.contexts] if enable and caches else []

    def read_tables(self):
        pc = self.pc
        self.w, self.lr = self.re.table_read(capi.TABLE_FFM_W), self.re.table_read(capi.TABLE_LR)
        self.refs = [ffm_ref.predict(pc.cfg, self.w, self.lr, x.lr, x.whole) for x in pc.cands]

    def close(self):
        for c in self.closing + self.caches:
            c.close()
        self.re.close()
        self.src.close()


def _expected_launch(pc, max_ffm):
    """(threads, LDS bytes) of requests_launch_shape: min(F, max_ffm) * R floats per wave, up to four waves in 64 KiB, at least one"""
    per_wave = max(1, min(pc.F, max_ffm)) * pc.R * 4
    waves = min(4, max(1, (64 * 1024) // per_wave))
    return 64 * waves, per_wave * waves


# ------------------------------------------------------------------ opt-in
def test_the_switch_is_opt_in_and_one_way():
    pc = pq.case(6, 4)
    dev = _Device(pc, enable=False)
    re = dev.re
    try:
        assert re.packed_caches_state() == (False, 0)
        ctx = _fb(*pc.contexts[0])
        assert "packed" in _refused(lambda: re.setup_cache(ctx))  # as today
        b = re.batch([_fb(x.lr, x.rest) for x in pc.cands[:8]])
        dev.closing.append(b)
        before = _launch(re, b)
        assert re.last_route() == capi.ROUTE_PACKED
        msg = _refused(lambda: dev.src.enable_packed_caches())  # an f32 regressor needs no switch and has none
        assert "f32" in msg
        assert dev.src.packed_caches_state() == (False, 0)
        re.enable_packed_caches()
        re.enable_packed_caches()  # (again: still on)
        assert re.packed_caches_state() == (True, 0)
        cache = re.setup_cache(ctx)
        dev.closing.append(cache)
        assert cache.debug_read()[3] == 0
        # a batch without a cache still takes the packed predict kernel, with the same bits
        assert np.array_equal(_bits(_launch(re, b)), _bits(before)) and re.last_route() == capi.ROUTE_PACKED
    finally:
        dev.close()


@pytest.mark.parametrize("F,k", pq.REFUSED, ids=[f"{F}x{k}" for F, k in pq.REFUSED])
def test_shapes_the_packed_form_refuses_stay_refused(F, k):
    rs = cc.request_set(F, k)
    src = fw.Regressor(cc.models(rs))
    try:
        msg = _refused(lambda: src.pack())
        assert "packed regressor" in msg and "ffm_k" in msg, msg
    finally:
        src.close()


# ------------------------------------------------------------------ the block and the caches' contents
@SHAPES
def test_cache_contents_are_the_restated_build_kernel(F, k):
    pc = pq.case(F, k)
    dev = _Device(pc)
    try:
        # the device's quantiser gives the block the numpy restatement gives: the CPU file's faults were planted on THESE values
        assert np.array_equal(_bits(dev.w), _bits(pc.w))
        for c, (lr, ffm) in zip(dev.caches, pc.contexts):
            T, dcf, cnt, epoch = c.debug_read()
            wT, wdcf, wcnt = pq.build_cache(F, k, dev.w, ffm)
            assert epoch == 0
            assert np.array_equal(cnt, wcnt)
            assert np.array_equal(_bits(T), _bits(wT)), "T"
            assert np.array_equal(_bits(dcf), _bits(wdcf)), "dcf"
            # two builds give the same bits
            assert dev.re.setup_cache(_fb(lr, ffm), c) is c
            T2, dcf2, cnt2, _ = c.debug_read()
            assert np.array_equal(_bits(T2), _bits(T)) and np.array_equal(_bits(dcf2), _bits(dcf)) and np.array_equal(cnt2, cnt)
        assert np.all(dev.caches[3].debug_read()[0] == 0.0) and np.all(dev.caches[3].debug_read()[2] == 0)
    finally:
        dev.close()


# ------------------------------------------------------------------ the route
@SHAPES
def test_packed_requests_route_per_candidate(F, k):
    pc = pq.case(F, k)
    dev = _Device(pc)
    re, caches, refs = dev.re, dev.caches, dev.refs
    f32 = None
    try:
        tag = f"{F}x{k}"
        for x in pc.cands:
            assert np.array_equal(caches[x.cache].filter(x.whole), x.rest)
        sums = [re.table_checksum(t) for t in (capi.TABLE_FFM_W, capi.TABLE_LR)]
        idx = np.array([x.cache for x in pc.cands], dtype=np.uint32)
        fbs = [_fb(x.lr, x.rest) for x in pc.cands]
        b = re.batch(fbs)
        dev.closing.append(b)
        plain = _launch(re, b)
        assert re.last_route() == capi.ROUTE_PACKED
        plain5 = re.predict(_fb(pc.cands[5].lr, pc.cands[5].rest))

        # ---- the set: route, kernel family, launch shape, the bar
        b.set_caches(caches, idx)
        p = _launch(re, b)
        assert re.last_route() == capi.ROUTE_REQUESTS
        info = re.last_launch()
        max_ffm = max(len(x.rest) for x in pc.cands)
        threads, lds = _expected_launch(pc, max_ffm)
        assert (info["family"], info["chunks"], info["threads"], info["lds_bytes"]) == (capi.KERNEL_PACKED_REQUESTS, (pc.R + 255) // 256, threads, lds), info
        assert (info["window"], info["chain"], info["no_kept_rows"], info["lds_keep"]) == (0, 0, 0, 0), info
        _judge(tag, p, refs)

        # ---- the same bits: again, in order, grouped by cache, repeated over many workgroups
        assert np.array_equal(_bits(_launch(re, b)), _bits(p)), "two launches differ"
        assert np.array_equal(_bits(_launch(re, b, capi.MODE_SEQUENTIAL)), _bits(p)), "MODE_SEQUENTIAL differs from MODE_HOGWILD"
        assert re.last_route() == capi.ROUTE_REQUESTS
        order = np.argsort(idx, kind="stable")
        gb = re.batch([fbs[i] for i in order])
        dev.closing.append(gb)
        gb.set_caches(caches, idx[order])
        assert np.array_equal(_bits(_launch(re, gb)), _bits(p)[order]), "grouped by cache differs from interleaved"
        reps = 48
        big = re.batch(fbs * reps)
        dev.closing.append(big)
        big.set_caches(caches, np.tile(idx, reps))
        pb = _bits(_launch(re, big)).reshape(reps, len(fbs))
        assert np.array_equal(pb, np.broadcast_to(_bits(p), pb.shape)), "a repeat of the set differs"

        # ---- one cache: set_cache is the set of one, on the same route; predict_with_cache is that launch for one example
        own = [i for i, x in enumerate(pc.cands) if x.cache == 0]
        ob = re.batch([fbs[i] for i in own])
        dev.closing.append(ob)
        ob.set_caches(caches[:1], np.zeros(len(own), dtype=np.uint32))
        p_one = _launch(re, ob)
        assert re.last_route() == capi.ROUTE_REQUESTS
        assert np.array_equal(_bits(p_one), _bits(p)[own])
        ob.set_cache(caches[0])  # (replaces the set)
        p_set = _launch(re, ob)
        assert re.last_route() == capi.ROUTE_REQUESTS and re.last_launch()["family"] == capi.KERNEL_PACKED_REQUESTS
        assert np.array_equal(_bits(p_set), _bits(p_one)), "set_cache differs from the set of one"
        ob.set_cache(None)
        assert np.array_equal(_bits(_launch(re, ob)), _bits(plain)[own]) and re.last_route() == capi.ROUTE_PACKED
        some = list(range(16))  # four candidates of each cache, the empty one among them
        single = np.array([re.predict_with_cache(_fb(pc.cands[i].lr, pc.cands[i].whole), None, caches[pc.cands[i].cache]) for i in some], dtype=np.float32)
        assert np.array_equal(_bits(single), _bits(p)[some]), "predict_with_cache differs from the batch"
        # (the single-example call leaves no set behind: a plain predict is the packed kernel's)
        assert re.predict(_fb(pc.cands[5].lr, pc.cands[5].rest)) == plain5

        # ---- nothing was written
        assert [re.table_checksum(t) for t in (capi.TABLE_FFM_W, capi.TABLE_LR)] == sums

        # ---- packed against f32: an f32 regressor that holds the dequantised values sums the same floats in the same order
        f32 = fw.Regressor(cc.models(pc.rs))
        for t, v in zip(TABLES, (dev.w, pc.acc, pc.lr)):
            f32.table_write(t, v)
        fcaches = [f32.setup_cache(_fb(lr, ffm)) for lr, ffm in pc.contexts]
        dev.closing += fcaches
        for c, fc in zip(caches, fcaches):
            for name, got, want in zip(("T", "dcf", "cnt"), c.debug_read()[:3], fc.debug_read()[:3]):
                assert np.array_equal(_bits(got) if name != "cnt" else got, _bits(want) if name != "cnt" else want), f"cache contents, {name}"
        fb32 = f32.batch(fbs)
        dev.closing.append(fb32)
        fb32.set_caches(fcaches, idx)
        p32 = _launch(f32, fb32)
        assert f32.last_route() == capi.ROUTE_REQUESTS and f32.last_launch()["family"] == capi.KERNEL_REQUESTS
        assert np.array_equal(_bits(p32), _bits(p)), "packed differs from f32 on the dequantised values"

        # ---- detached: the plain launch's bits are the bits before any set was attached
        b.set_caches([], [])
        assert np.array_equal(_bits(_launch(re, b)), _bits(plain)) and re.last_route() == capi.ROUTE_PACKED
    finally:
        dev.close()
        if f32 is not None:
            f32.close()


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_regressor_as_it_was():
    F, k = 6, 4
    pc = pq.case(F, k)
    dev = _Device(pc)
    re, caches = dev.re, dev.caches
    try:
        idx = np.array([x.cache for x in pc.cands], dtype=np.uint32)
        fbs = [_fb(x.lr, x.rest) for x in pc.cands]
        b = re.batch(fbs)
        dev.closing.append(b)
        b.set_caches(caches, idx)
        p = _launch(re, b)

        def still_the_set():
            assert np.array_equal(_bits(_launch(re, b)), _bits(p)) and re.last_route() == capi.ROUTE_REQUESTS

        # an updating launch
        assert "update" in _refused(lambda: re.learn_batch(b, capi.MODE_HOGWILD, True))
        still_the_set()
        # a cache of another regressor: the f32 source's, and a second packed regressor's
        foreign = dev.src.setup_cache(_fb(*pc.contexts[0]))
        dev.closing.append(foreign)
        assert "another regressor" in _refused(lambda: b.set_caches(caches[:3] + [foreign], idx))
        still_the_set()
        other = dev.src.pack()
        dev.closing.append(other)
        other.enable_packed_caches()
        foreign2 = other.setup_cache(_fb(*pc.contexts[0]))
        dev.closing.insert(0, foreign2)
        assert "another regressor" in _refused(lambda: b.set_caches([foreign2], np.zeros(len(fbs), dtype=np.uint32)))
        ob = re.batch(fbs[:4])
        dev.closing.append(ob)
        assert "another regressor" in _refused(lambda: ob.set_cache(foreign2))
        assert "another regressor" in _refused(lambda: re.predict_with_cache(_fb(pc.cands[0].lr, pc.cands[0].whole), None, foreign2))
        still_the_set()
        # a record batch with a cache: the cover is refused, and so is the attachment; both name the entry route
        fbt = fw.FeatureBufferTranslator(cc.models(pc.rs))
        recs = [q.rec for q in pc.rs.requests[:cc.N_RECORD_ROUTE]]
        off = np.zeros(len(recs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(r) for r in recs])
        rb = re.record_batch(fbt, np.concatenate(recs), off)
        dev.closing.append(rb)
        before = _launch(re, rb)
        assert "entry" in _refused(lambda: caches[0].cover_record(fbt, pc.rs.ctx_rec))
        assert "entry" in _refused(lambda: rb.set_cache(caches[0]))
        assert "record batch" in _refused(lambda: rb.set_caches(caches[:1], np.zeros(len(recs), dtype=np.uint32)))
        assert np.array_equal(_bits(_launch(re, rb)), _bits(before)) and re.last_route() == capi.ROUTE_PACKED
        # rows off the 4-bucket boundary (raw entries)
        sh = cc.shifted(pc.rs, 2)
        sb = re.batch([_fb(q.lr, q.rest) for q in sh.requests])
        dev.closing.append(sb)
        assert "16-byte" in _refused(lambda: sb.set_caches(caches[:1], np.zeros(len(sh.requests), dtype=np.uint32)))
        assert "multiple of 4" in _refused(lambda: re.setup_cache(_fb(sh.ctx_lr, sh.ctx_ffm)))
        still_the_set()
    finally:
        dev.close()


# ------------------------------------------------------------------ staleness
def test_a_refresh_makes_the_caches_stale_until_they_are_set_up_again():
    F, k = 6, 4
    pc = pq.case(F, k)
    dev = _Device(pc)
    re, caches = dev.re, dev.caches
    try:
        idx = np.array([x.cache for x in pc.cands], dtype=np.uint32)
        fbs = [_fb(x.lr, x.rest) for x in pc.cands]
        b = re.batch(fbs)
        dev.closing.append(b)
        b.set_caches(caches, idx)
        p0 = _launch(re, b)
        _judge("6x4 before the refresh", p0, dev.refs)
        old_refs = dev.refs
        # the source's tables change, the packed regressor is refreshed in place: the switch stays, the epoch moves
        src2, inc2, mn2, b2 = pq.refreshed(pc)
        dev.src.table_write(capi.TABLE_FFM_W, src2)
        assert dev.src.pack(into=re) is re
        assert re.packed_caches_state() == (True, 1)
        dev.read_tables()
        assert np.array_equal(_bits(dev.w), _bits(pq.dequantize(inc2, mn2, b2)))
        # every door is shut to the old caches, and the batch is left as it was
        assert "stale" in _refused(lambda: re.learn_batch(b, capi.MODE_HOGWILD, False))
        assert "stale" in _refused(lambda: b.set_caches(caches, idx))
        ob = re.batch(fbs[:4])
        dev.closing.append(ob)
        assert "stale" in _refused(lambda: ob.set_cache(caches[0]))
        assert "stale" in _refused(lambda: re.predict_with_cache(_fb(pc.cands[0].lr, pc.cands[0].whole), None, caches[0]))
        plain = _launch(re, ob)  # (nothing was attached to it)
        assert re.last_route() == capi.ROUTE_PACKED and np.all(np.isfinite(plain))
        # one cache set up again is not enough for a set that holds four
        assert re.setup_cache(_fb(*pc.contexts[0]), caches[0]) is caches[0]
        assert caches[0].debug_read()[3] == 1 and caches[1].debug_read()[3] == 0
        assert "stale" in _refused(lambda: re.learn_batch(b, capi.MODE_HOGWILD, False))
        for c, (lr, ffm) in zip(caches[1:], pc.contexts[1:]):
            assert re.setup_cache(_fb(lr, ffm), c) is c
        p1 = _launch(re, b)  # (the set that stayed attached, its caches refilled in place)
        assert re.last_route() == capi.ROUTE_REQUESTS
        _judge("6x4 after the refresh", p1, dev.refs)
        outside = sum(ffm_ref.judge_prediction(p0[i], *dev.refs[i])[0] > ffm_ref.judge_prediction(p0[i], *dev.refs[i])[1] for i in range(len(p0)))
        assert outside >= 24, "the refresh did not move the model: the case shows nothing"
        assert old_refs is not dev.refs
    finally:
        dev.close()


# ------------------------------------------------------------------ two published files: the hot patch, at the C ABI and through the serving FFI
@pytest.fixture(scope="module")
def two_publishes(tmp_path_factory):
    """file 0 and file 1 of one trainer, 40 examples apart, with the quantiser's extremes pinned (tests/test_gpu_publish_diff.py); their images' diff"""
    d = tmp_path_factory.mktemp("packed_requests_publish")
    vw = K.vwmap()
    mi, re, (recs, off) = K.pinned_model()
    f0, f1 = str(d / "publish0.fw"), str(d / "publish1.fw")
    P.save_inference_regressor(f0, mi, vw, re, quantize_weights=True)
    img0 = P.Image.capture(mi, vw, re, quantize_weights=True)
    K.train(re, mi, recs, off)
    P.save_inference_regressor(f1, mi, vw, re, quantize_weights=True)
    img1 = P.Image.capture(mi, vw, re, quantize_weights=True)
    stream, changed = img0.diff(img1, with_changed=True)
    assert changed > 0
    for x in (img0, img1, re):
        x.close()
    return dict(f0=f0, f1=f1, stream=stream, changed=changed)


CONTEXTS = ["|A0 17 23:0.5 |A1 99 ", "|A0 5 |A1 12:2 7 ", "|A0 400:0.5 401 |A1 3 "]


def _lines(seed, n):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        parts = []
        for ns in (2, 3, 4, 5):
            m = int(rng.integers(0, 3)) if ns != 2 else int(rng.integers(1, 3))
            if m:
                parts.append(f"|A{ns} " + " ".join(f"{int(rng.integers(0, 3000))}" + (f":{rng.random() * 2:.3f}" if rng.random() < 0.3 else "") for _ in range(m)))
        out.append(" ".join(parts) + "\n")
    return out


def _whole_line_refs(mi, re, ctx, cands):
    """the float64 pass over context + candidate on the regressor's own tables, and the translated buffers"""
    from fwumious_wabbit_amd.feed import VowpalParser

    host = VowpalParser(K.vwmap())
    fbt = fw.FeatureBufferTranslator(mi)
    w, lr = re.table_read(capi.TABLE_FFM_W), re.table_read(capi.TABLE_LR)
    cfg = SimpleNamespace(F=len(mi.ffm_fields), k=mi.ffm_k)
    fbs = [fbt.translate(host.next_vowpal((ctx + c).encode())) for c in cands]
    ctx_fb = fbt.translate(host.next_vowpal((ctx + "\n").encode()))
    host.close()
    return ctx_fb, fbs, [ffm_ref.predict(cfg, w, lr, fb.lr_buffer, fb.ffm_buffer) for fb in fbs]


def test_a_hot_patch_makes_the_caches_stale(two_publishes):
    t = two_publishes
    mi, _, r0 = P.new_regressor_from_filename(t["f0"], immutable=True, packed=True, packed_caches=True)
    _, _, r1 = P.new_regressor_from_filename(t["f1"], immutable=True, packed=True, packed_caches=True)
    closing = []
    try:
        assert r0.packed_caches_state() == (True, 0)
        with pytest.raises(ValueError):
            P.new_regressor_from_filename(t["f0"], immutable=True, packed_caches=True)
        ctx, cands = CONTEXTS[0], _lines(11, 24)
        ctx_fb, fbs, refs0 = _whole_line_refs(mi, r0, ctx, cands)
        _, _, refs1 = _whole_line_refs(mi, r1, ctx, cands)

        def attached(re):
            cache = re.setup_cache(ctx_fb)
            b = re.batch([_fb(fb.lr_buffer, cache.filter(fb.ffm_buffer)) for fb in fbs])
            closing[:0] = [b, cache]
            b.set_cache(cache)
            return cache, b

        c0, b0 = attached(r0)
        c1, b1 = attached(r1)
        p0 = _launch(r0, b0)
        assert r0.last_route() == capi.ROUTE_REQUESTS
        _judge("file 0", p0, refs0)
        assert r0.apply_diff(b"") == 0 and r0.packed_caches_state() == (True, 0)  # an empty stream changes nothing, the epoch included
        assert np.array_equal(_bits(_launch(r0, b0)), _bits(p0))
        assert r0.apply_diff(t["stream"]) == t["changed"]
        assert r0.packed_caches_state() == (True, 1)
        assert "stale" in _refused(lambda: r0.learn_batch(b0, capi.MODE_HOGWILD, False))
        assert "stale" in _refused(lambda: r0.predict_with_cache(fbs[0], None, c0))
        assert r0.setup_cache(ctx_fb, c0) is c0
        p1 = _launch(r0, b0)
        _judge("file 0 patched to file 1", p1, refs1)
        want = _launch(r1, b1)
        _judge("file 1", want, refs1)
        assert np.array_equal(_bits(p1), _bits(want)), "the patched regressor differs from the load of the next file"
        assert not np.array_equal(_bits(p1), _bits(p0))
    finally:
        for x in closing + [r0, r1]:
            x.close()


def test_serving_with_packed_context_caches(two_publishes):
    from fwumious_wabbit_amd import serving
    from fwumious_wabbit_amd.serving import Predictor

    t = two_publishes
    flags = "--packed_weights --packed_context_cache"
    mi, _, twin0 = P.new_regressor_from_filename(t["f0"], immutable=True, packed=True)
    _, _, twin1 = P.new_regressor_from_filename(t["f1"], immutable=True, packed=True)
    prs = []
    try:
        proto = Predictor(f"fw -i {t['f0']} -t --foreground {flags}")
        prs.append(proto)
        prs += [proto.clone_lite() for _ in range(15)]
        contexts = [CONTEXTS[i % 3] for i in range(16)]
        requests = [_lines(100 + i, 12) for i in range(16)]
        refs0 = [_whole_line_refs(mi, twin0, c, q)[2] for c, q in zip(contexts, requests)]
        refs1 = [_whole_line_refs(mi, twin1, c, q)[2] for c, q in zip(contexts, requests)]
        for pr, c in zip(prs, contexts):
            assert pr.setup_cache(c + "\n") == 0.0

        def say(pr, q):
            return np.array([pr.predict_with_cache(x) for x in q], dtype=np.float32), pr.predict_batch(q, with_cache=True)

        # ---- every cached call against float64 on the whole line; the calls agree bit for bit
        one, batch = say(prs[0], requests[0])
        _judge("serving predict_with_cache", one, refs0[0])
        _judge("serving predict_batch", batch, refs0[0])
        assert np.array_equal(_bits(one), _bits(batch))
        text = prs[0].predict_text("".join(requests[0]).encode(), with_cache=True)
        assert prs[0].last_text_route()[2] is True  # (the existing fall-back to the batch route, which is now cached)
        assert np.array_equal(_bits(text), _bits(batch))
        # ---- 16 predictors in one call: their own per-request calls, bit for bit
        per_request = [pr.predict_batch(q, with_cache=True) for pr, q in zip(prs, requests)]
        outs = serving.predict_requests(prs, requests)
        for r in range(16):
            _judge(f"serving predict_requests, request {r}", outs[r], refs0[r])
            assert np.array_equal(_bits(outs[r]), _bits(per_request[r])), r
        # ---- a clone with its parent's context (clone 3 holds context 0 in a cache of its own) is its parent
        assert contexts[3] == contexts[0]
        assert np.array_equal(_bits(prs[3].predict_batch(requests[0], with_cache=True)), _bits(batch))
        assert np.array_equal(_bits(say(prs[3], requests[0])[0]), _bits(one))
        # ---- a plain --packed_weights predictor next to them behaves as before
        plain = Predictor(f"fw -i {t['f0']} -t --foreground --packed_weights")
        prs.append(plain)
        assert plain.setup_cache(contexts[0] + "\n") == 0.0
        msg = _refused(lambda: serving.predict_requests([plain], [requests[0]]))
        assert "packed" in msg and "fwgpu_predictor_predict_batch" in msg
        _judge("serving, plain packed predictor (whole lines)", plain.predict_batch(requests[0], with_cache=True), refs0[0])
        # ---- the hot patch: every predictor's next cached call is the fresh predictor's of the next file, with no call of the caller's in between
        prs[5].apply_diff(t["stream"])
        fresh = Predictor(f"fw -i {t['f1']} -t --foreground {flags}")
        prs.append(fresh)
        assert fresh.setup_cache(contexts[0] + "\n") == 0.0
        want_one, want_batch = say(fresh, requests[0])
        _judge("serving, the next file", want_batch, refs1[0])
        got_one, got_batch = say(prs[0], requests[0])
        assert np.array_equal(_bits(got_one), _bits(want_one)) and np.array_equal(_bits(got_batch), _bits(want_batch))
        assert not np.array_equal(_bits(got_batch), _bits(batch))
        outs1 = serving.predict_requests(prs[:16], requests)  # (15 of them still hold stale caches: rebuilt before the set is attached)
        for r in range(16):
            _judge(f"serving predict_requests after the patch, request {r}", outs1[r], refs1[r])
        assert np.array_equal(_bits(outs1[0]), _bits(want_batch))
    finally:
        for pr in prs:
            pr.close()
        twin0.close()
        twin1.close()
