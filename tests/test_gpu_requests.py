"""The requests route on the device: candidates of many requests in one launch, each against its own context cache (fwgpu_batch_set_caches,
csrc/requests.hip; serving: fwgpu_predictor_predict_requests).

Per shape of requests_cases.SHAPES four caches (three contexts and an empty one) and 96 candidates interleaved round-robin over them; EVERY prediction
is held to the project's bar

    |p - p_ref| <= min(C_P * M_p + 4 ulp(p), 5e-5)                      (ffm_ref.judge_prediction)

with p_ref the float64 forward pass over the WHOLE request (context + candidate) on the device's own tables.  What would turn a case red is planted in
float32 numpy in tests/test_requests_cpu.py: base(S) left out, every candidate read against cache 0, the cross term of two gathered fields or the
candidate's own self-pair term dropped, a cache row's second chunk read from its first."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

import cache_cases as cc
import ffm_ref
import fwumious_wabbit_amd as fw
import requests_cases as rq
from fwumious_wabbit_amd import _capi as capi

pytestmark = pytest.mark.gpu

TABLES = (capi.TABLE_FFM_W, capi.TABLE_FFM_ACC, capi.TABLE_LR)
LDS_LIMIT = 160 * 1024
SHAPES = pytest.mark.parametrize("F,k", rq.SHAPES, ids=[f"{F}x{k}" for F, k in rq.SHAPES])


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
        print(f"REQUESTS {tag}, candidate {i}: p = {p[i]!r}, float64 {refs[i][0]!r}, |d| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, f"{tag}, candidate {i}: prediction {p[i]!r}, float64 {refs[i][0]!r}: |d| = {err:.3e}, bound {bound:.3e} (needs c_p = {need:.3e}, C_P = {ffm_ref.C_P:.3e})"
    print(f"REQUESTS {tag}: needs c_p = {worst:.3e} = {worst / ffm_ref.C_P:.3f} C_P")


def _refused(fn):
    with pytest.raises(capi.FwgpuError) as e:
        fn()
    assert e.value.code == capi.ERR_INVALID, e.value
    return e.value.message


class _Device:
    """a regressor on the shape's warm tables with the four caches of requests_cases.case"""

    def __init__(self, cs, mi=None):
        self.cs = cs
        self.re = fw.Regressor(cc.models(cs.rs) if mi is None else mi)
        self.caches = []
        for t, v in zip(TABLES, (cs.w, cs.acc, cs.lr)):
            assert self.re.table_len(t) == len(v)
            self.re.table_write(t, v)
        for lr, ffm in cs.contexts:
            self.caches.append(self.re.setup_cache(_fb(lr, ffm)))

    def close(self):
        for c in self.caches:
            c.close()
        self.re.close()


def _expected_launch(cs, max_ffm):
    """(threads, LDS bytes) of requests_launch_shape: min(F, max_ffm) * R floats per wave, up to four waves in 64 KiB, at least one"""
    per_wave = max(1, min(cs.F, max_ffm)) * cs.R * 4
    waves = min(4, max(1, (64 * 1024) // per_wave))
    return 64 * waves, per_wave * waves


@SHAPES
def test_requests_route_per_candidate(F, k):
    cs = rq.case(F, k)
    dev = _Device(cs)
    re, caches = dev.re, dev.caches
    batches = []
    try:
        tag = f"{F}x{k}"
        for x in cs.cands:
            assert np.array_equal(caches[x.cache].filter(x.whole), x.rest)
        sums = [re.table_checksum(t) for t in TABLES]
        refs = [x.ref for x in cs.cands]
        idx = np.array([x.cache for x in cs.cands], dtype=np.uint32)
        fbs = [_fb(x.lr, x.rest) for x in cs.cands]
        b = re.batch(fbs)
        batches.append(b)
        plain = _launch(re, b)  # (no cache: the candidates' own features alone -- only its bits matter, below)
        assert re.last_route() == capi.ROUTE_FUSED

        # ---- the set: route, launch shape, the bar
        b.set_caches(caches, idx)
        p = _launch(re, b)
        assert re.last_route() == capi.ROUTE_REQUESTS
        info = re.last_launch()
        max_ffm = max(len(x.rest) for x in cs.cands)
        threads, lds = _expected_launch(cs, max_ffm)
        # (40 x 16: min(40, max_ffm) = 40 slices of 640 floats = 102 400 bytes, one wave per workgroup: below the 160 KiB limit, so it is SERVED)
        assert max(1, min(F, max_ffm)) * cs.R * 4 <= LDS_LIMIT
        assert (info["family"], info["chunks"], info["threads"], info["lds_bytes"]) == (capi.KERNEL_REQUESTS, (cs.R + 255) // 256, threads, lds), info
        assert (info["window"], info["chain"], info["no_kept_rows"], info["lds_keep"]) == (0, 0, 0, 0), info
        _judge(tag, p, refs)
        zero = [i for i, x in enumerate(cs.cands) if len(x.rest) == 0]
        assert len(zero) == 3, "request 0 of each set: base + LR"

        # ---- the same bits: again, in order, grouped by cache, repeated over many workgroups
        assert np.array_equal(_bits(_launch(re, b)), _bits(p)), "two launches differ"
        assert np.array_equal(_bits(_launch(re, b, capi.MODE_SEQUENTIAL)), _bits(p)), "MODE_SEQUENTIAL differs from MODE_HOGWILD"
        assert re.last_route() == capi.ROUTE_REQUESTS
        order = np.argsort(idx, kind="stable")
        gb = re.batch([fbs[i] for i in order])
        batches.append(gb)
        gb.set_caches(caches, idx[order])
        assert np.array_equal(_bits(_launch(re, gb)), _bits(p)[order]), "grouped by cache differs from interleaved"
        reps = 48
        big = re.batch(fbs * reps)
        batches.append(big)
        big.set_caches(caches, np.tile(idx, reps))
        pb = _bits(_launch(re, big)).reshape(reps, len(fbs))
        assert np.array_equal(pb, np.broadcast_to(_bits(p), pb.shape)), "a repeat of the set differs"

        # ---- one cache: the set of one, and the existing set_cache route on the same batch, both to the bar
        own = [i for i, x in enumerate(cs.cands) if x.cache == 0]
        ob = re.batch([fbs[i] for i in own])
        batches.append(ob)
        ob.set_caches(caches[:1], np.zeros(len(own), dtype=np.uint32))
        p_one = _launch(re, ob)
        assert re.last_route() == capi.ROUTE_REQUESTS
        _judge(tag + " one cache", p_one, [refs[i] for i in own])
        assert np.array_equal(_bits(p_one), _bits(p)[own])
        ob.set_cache(caches[0])  # (replaces the set)
        p_old = _launch(re, ob)
        assert re.last_route() == capi.ROUTE_FUSED and re.last_launch()["family"] != capi.KERNEL_REQUESTS
        _judge(tag + " set_cache", p_old, [refs[i] for i in own])
        ob.set_caches(caches[:1], np.zeros(len(own), dtype=np.uint32))  # (... and the other way round)
        assert np.array_equal(_bits(_launch(re, ob)), _bits(p_one)) and re.last_route() == capi.ROUTE_REQUESTS

        # ---- nothing was written
        assert [re.table_checksum(t) for t in TABLES] == sums

        # ---- a refilled handle: cache 1 now holds the first set's context, and the NEXT launch reads it (base is formed at the head of every launch)
        new_lr, new_ffm = cs.contexts[0]
        assert re.setup_cache(_fb(new_lr, new_ffm), caches[1]) is caches[1]
        p2 = _launch(re, b)
        refs2 = list(refs)
        for i, x in enumerate(cs.cands):
            if x.cache == 1:  # the new whole request: the new context's FFM features and the entries the example holds
                both = np.concatenate([new_ffm, x.rest])
                both = both[np.argsort(both["contra_field_index"], kind="stable")]
                refs2[i] = ffm_ref.predict(cs.cfg, cs.w, cs.lr, x.lr, both)
        _judge(tag + " refilled", p2, refs2)
        moved = [i for i, x in enumerate(cs.cands) if x.cache == 1]
        assert not np.array_equal(_bits(p2)[moved], _bits(p)[moved])
        rest = [i for i, x in enumerate(cs.cands) if x.cache != 1]
        assert np.array_equal(_bits(p2)[rest], _bits(p)[rest])

        # ---- detached: the plain launch's bits are the bits before any set was attached
        b.set_caches([], [])
        assert np.array_equal(_bits(_launch(re, b)), _bits(plain)) and re.last_route() == capi.ROUTE_FUSED
    finally:
        for x in batches:
            x.close()
        dev.close()


def test_refusals_leave_the_batch_as_it_was():
    F, k = 6, 4
    cs = rq.case(F, k)
    dev = _Device(cs)
    re, caches = dev.re, dev.caches
    closing = []
    try:
        idx = np.array([x.cache for x in cs.cands], dtype=np.uint32)
        fbs = [_fb(x.lr, x.rest) for x in cs.cands]
        b = re.batch(fbs)
        closing.append(b)
        plain = _launch(re, b)
        b.set_caches(caches, idx)
        p = _launch(re, b)

        def still_the_set():
            assert np.array_equal(_bits(_launch(re, b)), _bits(p)) and re.last_route() == capi.ROUTE_REQUESTS

        # an updating launch
        msg = _refused(lambda: re.learn_batch(b, capi.MODE_HOGWILD, True))
        assert "update" in msg
        still_the_set()
        # an index out of range; a NULL-free set with a cache of a second regressor
        bad = idx.copy()
        bad[5] = len(caches)
        assert "n_caches" in _refused(lambda: b.set_caches(caches, bad))
        still_the_set()
        re2 = fw.Regressor(cc.models(cs.rs))
        closing.append(re2)
        foreign = re2.setup_cache(_fb(*cs.contexts[0]))
        closing.insert(0, foreign)
        assert "another regressor" in _refused(lambda: b.set_caches(caches[:3] + [foreign], idx))
        still_the_set()
        # a record batch
        fbt = fw.FeatureBufferTranslator(cc.models(cs.rs))
        recs = [q.rec for q in cs.rs.requests[:cc.N_RECORD_ROUTE]]
        off = np.zeros(len(recs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(r) for r in recs])
        rb = re.record_batch(fbt, np.concatenate(recs), off)
        closing.append(rb)
        before = _launch(re, rb)
        assert "record batch" in _refused(lambda: rb.set_caches(caches[:1], np.zeros(len(recs), dtype=np.uint32)))
        assert np.array_equal(_bits(_launch(re, rb)), _bits(before)) and re.last_route() == capi.ROUTE_FUSED
        # rows off the 16-byte boundary (raw entries)
        sh = cc.shifted(cs.rs, 2)
        sb = re.batch([_fb(q.lr, q.rest) for q in sh.requests])
        closing.append(sb)
        before = _launch(re, sb)
        assert "16-byte" in _refused(lambda: sb.set_caches(caches[:1], np.zeros(len(sh.requests), dtype=np.uint32)))
        assert np.array_equal(_bits(_launch(re, sb)), _bits(before)) and re.last_route() == capi.ROUTE_FUSED
        # detaching
        b.set_caches([], [])
        assert np.array_equal(_bits(_launch(re, b)), _bits(plain)) and re.last_route() == capi.ROUTE_FUSED
    finally:
        for x in closing:
            x.close()
        dev.close()


@pytest.mark.parametrize("what", ["deep head", "k = 10"])
def test_models_the_route_does_not_serve(what):
    """a deep head, and ffm_k % 4 != 0 (there is no one-float-per-lane form): refused with the reason, the batch launches as before"""
    F, k = (6, 4) if what == "deep head" else (6, 10)
    rs = cc.request_set(F, k)
    mi = cc.models(rs)
    if what == "deep head":
        mi.nn_layers = [dict(width="9", activation="relu")]
    re = fw.Regressor(mi)
    cache = b = None
    try:
        w, acc, lr = cc.warm_tables(F, k, rs.ffm_bits, rs.bits)
        for t, v in zip(TABLES, (w, acc, lr)):
            re.table_write(t, v)
        cache = re.setup_cache(_fb(rs.ctx_lr, rs.ctx_ffm))
        b = re.batch([_fb(q.lr, q.rest) for q in rs.requests])
        b.set_cache(cache)
        before = _launch(re, b)
        msg = _refused(lambda: b.set_caches([cache], np.zeros(len(rs.requests), dtype=np.uint32)))
        assert ("deep head" if what == "deep head" else "multiple of 4") in msg, msg
        assert np.array_equal(_bits(_launch(re, b)), _bits(before)) and re.last_route() != capi.ROUTE_REQUESTS  # (the one cache is still attached)
    finally:
        if b is not None:
            b.close()
        if cache is not None:
            cache.close()
        re.close()


# ------------------------------------------------------------------ serving: several predictors' requests in one call
CONTEXTS = ["|A ca |Bb cb1 cb2:0.5 ", "|A cx cy:2 |Bb cz ", "|A cq |Bb cr:0.5 cs ct "]
UNCOVERED = ["C", "Ddd", "E", "F"]  # namespaces the contexts leave to the candidates (tests/test_gpu_cached_predict.py)
BAD_LINE = "|C a:b:c:d\n"
SERVING_SEED = 300  # the first seed whose 120 candidates keep C_P * M_p below the cap unless saturated, at k = 4 and k = 64 (the float64 reference alone decides)


@pytest.mark.parametrize("k", [4, 64], ids=["k4", "k64"])
def test_serving_requests_in_one_call(tmp_path, k):
    from fwumious_wabbit_amd import persistence as P
    from fwumious_wabbit_amd import serving
    from fwumious_wabbit_amd.feed import VowpalParser, VwNamespaceMap
    from fwumious_wabbit_amd.serving import Predictor
    from helpers import make_pair
    from text_candidates import CSV, gen_candidate

    F = 6
    vw = VwNamespaceMap(CSV)
    mi, _, _ = make_pair(F, k, 12, 12, fw.Optimizer.AdagradLUT)
    re = fw.Regressor(mi)
    host = VowpalParser(vw)
    prs = []
    try:
        for t, v in zip(TABLES, cc.warm_tables(F, k, 12, 12, seed=9)):
            assert re.table_len(t) == len(v)
            re.table_write(t, v)
        w, lr = re.table_read(capi.TABLE_FFM_W), re.table_read(capi.TABLE_LR)
        path = str(tmp_path / "model.fw")
        P.save_regressor_to_filename(path, mi, vw, re)
        prs.append(Predictor(f"fw -i {path} -t --foreground"))
        prs += [prs[0].clone_lite(), prs[0].clone_lite()]
        rng = random.Random(SERVING_SEED)
        fbt = fw.FeatureBufferTranslator(mi)
        cfg = SimpleNamespace(F=F, k=k)
        requests, refs = [], []
        for ctx in CONTEXTS:
            cands = [gen_candidate(rng, namespaces=UNCOVERED, f32_nan=False) + "\n" for _ in range(40)]
            fbs = [fbt.translate(host.next_vowpal((ctx + c).encode())) for c in cands]
            ref = [ffm_ref.predict(cfg, w, lr, fb.lr_buffer, fb.ffm_buffer) for fb in fbs]
            # (as in test_serving_routes_per_request: gen_candidate's weights reach 750, the cap must bind on saturated sigmoids only)
            assert all(ffm_ref.C_P * M_p < ffm_ref.PRED_CAP or min(p, 1.0 - p) < 1e-6 for p, M_p in ref)
            requests.append(cands[:20] + [BAD_LINE] + cands[20:])
            refs.append(ref)

        # a predictor without setup_cache is refused, and so is the whole call
        msg = _refused(lambda: serving.predict_requests(prs, requests))
        assert "fwgpu_predictor_predict_batch" in msg and "fw_setup_cache" in msg
        for pr, ctx in zip(prs, CONTEXTS):
            assert pr.setup_cache(ctx + "\n") == 0.0
        before = [pr.predict_batch(req, with_cache=True) for pr, req in zip(prs, requests)]
        outs = serving.predict_requests(prs, requests)
        assert re.last_route() != capi.ROUTE_REQUESTS  # (the twin regressor is not the predictors')
        for r, (out, ref) in enumerate(zip(outs, refs)):
            assert len(out) == 41 and out[20] == -1.0 and before[r][20] == -1.0
            got = np.concatenate([out[:20], out[21:]])
            _judge(f"serving 6x{k} request {r}", got, ref)
            _judge(f"serving 6x{k} request {r}, predict_batch", np.concatenate([before[r][:20], before[r][21:]]), ref)
        # the same predictor twice, and a single request
        twice = serving.predict_requests([prs[1], prs[0], prs[1]], [requests[1], requests[0], requests[1]])
        assert np.array_equal(_bits(twice[0]), _bits(outs[1])) and np.array_equal(_bits(twice[2]), _bits(outs[1])) and np.array_equal(_bits(twice[1]), _bits(outs[0]))
        assert np.array_equal(_bits(serving.predict_requests(prs[2:], requests[2:])[0]), _bits(outs[2]))
        # the existing call keeps its bits
        for pr, req, was in zip(prs, requests, before):
            assert np.array_equal(_bits(pr.predict_batch(req, with_cache=True)), _bits(was))
        # a --packed_weights predictor keeps no device cache
        packed = Predictor(f"fw -i {path} -t --foreground --packed_weights")
        prs.append(packed)
        assert packed.setup_cache(CONTEXTS[0] + "\n") == 0.0
        msg = _refused(lambda: serving.predict_requests([packed], [requests[0]]))
        assert "packed" in msg and "fwgpu_predictor_predict_batch" in msg
        # predictors of different models
        other = Predictor(f"fw -i {path} -t --foreground")
        prs.append(other)
        assert other.setup_cache(CONTEXTS[0] + "\n") == 0.0
        assert "ONE model" in _refused(lambda: serving.predict_requests([prs[0], other], requests[:2]))
    finally:
        for pr in prs:
            pr.close()
        host.close()
        re.close()
