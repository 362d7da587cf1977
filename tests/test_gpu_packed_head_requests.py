"""Context caches and the requests route on a PACKED regressor with a deep head (fwgpu_packed_enable_head_requests; the packed form of
csrc/requests_head.hip's requests_head_kernel; serving: --packed_weights --packed_head_requests).  Per shape a head model trained in order on 300
records, saved, quantised, loaded packed and f32; the four caches and 96 interleaved candidates of test_gpu_head_requests.  The reference is float64
of the WHOLE request on the packed regressor's own table_read, at the project's bars (_assert_head_inputs, PRED_TOL)."""
from types import SimpleNamespace

import numpy as np
import pytest

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import _capi as capi
from fwumious_wabbit_amd import persistence as P
from fwumious_wabbit_amd import serving
import head_ref as hr
import test_gpu_head_cache as hc
import test_gpu_packed_head as ph
from head_ref import PRED_TOL
from helpers import make_pair
from test_gpu_head_predict import _assert_head_inputs
from test_gpu_head_requests import N_CACHES, N_CAND, _bits, _refused

pytestmark = pytest.mark.gpu
_BUILT = {}


def _requests(c, lr_table, ffm_w):
    """on these tables: three contexts with cached counts 0, 1, 2 cycling over the fields (shifted per context) and an empty one; candidate e goes
    against cache e % 4 with (e + f) % 3 own features in field f, every eighth with none"""
    c.lr_table, c.ffm_w = lr_table, ffm_w
    cands = [(lr, [[] for _ in own] if e % 8 == 5 else own, y) for e, (lr, own, y) in enumerate(hc._candidates(c, N_CAND, seed=22))]
    ctxs = [hc._context(c, [(f + r) % 3 for f in range(c.F)], False, seed=21 + r) for r in range(3)] + [[[] for _ in range(c.F)]]
    c.reqs = [hc.Request(c, ctxs[r], cands[r::N_CACHES]) for r in range(N_CACHES)]
    return lambda attr: [getattr(c.reqs[e % N_CACHES], attr)[e // N_CACHES] for e in range(N_CAND)]  # candidate e's, interleaved


@pytest.fixture
def ctx(tmp_path_factory):
    def build(F, k):
        if (F, k) in _BUILT:
            return _BUILT[(F, k)]
        c = SimpleNamespace(F=F, k=k)
        mi, ots = ph._head_mi(F, k)
        c.C = mi.num_combos
        re = fw.Regressor(mi)
        recs, off = fw.synth_records(F, 1.0, 1.1, 3000, 0.1, 5, 0, 300)
        b = re.record_batch(fw.FeatureBufferTranslator(mi), recs, off)
        re.learn_batch(b, capi.MODE_SEQUENTIAL, True)
        b.close()
        tr = hr.translate(ots, recs, off)
        c.pool_lr, pool = np.unique(tr.lr["hash"]), np.unique(tr.ffm["hash"])
        c.pool_ctx, c.pool_own = pool[0::2], pool[1::2]  # (disjoint: a candidate never repeats a cached feature)
        design = _requests(c, re.table_read(capi.TABLE_LR), re.table_read(capi.TABLE_FFM_W))("x64")  # (the trainer's tables: to shape the head weights)
        re.table_write(capi.TABLE_NN_W, hr.dense_head_weights(np.array(design), ph.LAYERS, ph.TOPO, seed=3))
        t, c.q = (str(tmp_path_factory.mktemp(f"phr{F}x{k}") / s) for s in "tq")
        P.save_regressor_to_filename(t, mi, ph._vwmap(F), re)
        re.close()
        P.convert_inference_regressor(t, c.q, quantize_weights=True)
        _, _, c.rf = P.new_regressor_from_filename(c.q, immutable=True)
        _, _, c.rp = P.new_regressor_from_filename(c.q, immutable=True, packed=True, packed_head=True)
        pick = _requests(c, c.rp.table_read(capi.TABLE_LR), c.rp.table_read(capi.TABLE_FFM_W))
        assert {(0, 0), (1, 0), (2, 0), (0, 1), (1, 2), (2, 2)} <= set().union(*(q.branches for q in c.reqs))
        c.x64, c.sa, c.exact0 = (np.array(pick(a)) for a in ("x64", "sa", "exact0"))
        c.own_fbs, c.whole_fbs, c.idx = pick("own_fbs"), pick("whole_fbs"), (np.arange(N_CAND) % N_CACHES).astype(np.uint32)
        c.p64, z = hr.head_forward64(c.x64, c.rp.table_read(capi.TABLE_NN_W), ph.LAYERS, ph.TOPO)
        assert np.abs(z).max() < 20.0
        return _BUILT.setdefault((F, k), c)

    return build


def _launch(re, b, family, mode=capi.MODE_HOGWILD):
    re.learn_batch(b, mode, False)
    assert re.last_route() == capi.ROUTE_REQUESTS and re.last_launch()["family"] == family, re.last_launch()
    return b.predictions().copy(), re.head_inputs(b.n)


@pytest.mark.parametrize("F,k", ph.SHAPES, ids=[f"{F}x{k}" for F, k in ph.SHAPES])
def test_packed_head_requests_per_candidate(ctx, F, k):
    c, what, PHR = ctx(F, k), f"{F}x{k}", capi.KERNEL_PACKED_HEAD_REQUESTS
    rp, rf, closing = c.rp, c.rf, []
    rp.enable_packed_head_requests()
    rf.enable_head_requests()
    try:
        caches, fcaches = ([r.setup_cache(q.ctx_fb) for q in c.reqs] for r in (rp, rf))
        order = np.argsort(c.idx, kind="stable")
        b, wb, gb, fb = rp.batch(c.own_fbs), rp.batch(c.whole_fbs), rp.batch([c.own_fbs[i] for i in order]), rf.batch(c.own_fbs)
        closing += [b, wb, gb, fb] + caches + fcaches
        sums = [rp.table_checksum(t) for t in ph.TABLES]
        b.set_caches(caches, c.idx)
        p, x = _launch(rp, b, PHR)
        # ---- the launch shape of the f32 head-requests kernels: min(F, max_ffm) * R + NT floats per wave, up to four waves in 64 KiB, at least one
        R, NT, info = F * k, F * (F + 1) // 2, rp.last_launch()
        per_wave = (min(F, max(len(e.ffm_buffer) for e in c.own_fbs)) * R + NT) * 4
        waves = min(4, max(1, (64 * 1024) // per_wave))
        assert (info["chunks"], info["threads"], info["lds_bytes"]) == ((R + 255) // 256, 64 * waves, per_wave * waves), info
        # ---- x slot by slot, the predictions against the float64 head and against the whole lines on the packed head route
        _assert_head_inputs(x, c.x64, c.sa, c.exact0, what)
        hc._close(p, c.p64, PRED_TOL, f"{what}: packed head requests against the float64 head")
        rp.learn_batch(wb, capi.MODE_HOGWILD, False)
        assert rp.last_route() == capi.ROUTE_PACKED_HEAD
        hc._close(p, wb.predictions(), PRED_TOL, f"{what}: packed head requests against the whole lines")
        # ---- the same bits: again, in order, grouped by cache, and on the f32 load of the same quantised file through enable_head_requests
        for mode in (capi.MODE_HOGWILD, capi.MODE_SEQUENTIAL):
            p2, x2 = _launch(rp, b, PHR, mode)
            assert np.array_equal(_bits(p2), _bits(p)) and np.array_equal(_bits(x2), _bits(x)), (what, mode)
        gb.set_caches(caches, c.idx[order])
        pg, xg = _launch(rp, gb, PHR)
        assert np.array_equal(_bits(xg), _bits(x)[order]) and np.array_equal(_bits(pg), _bits(p)[order]), "grouped by cache differs from interleaved"
        fb.set_caches(fcaches, c.idx)
        pf, xf = _launch(rf, fb, capi.KERNEL_HEAD_REQUESTS)
        assert np.array_equal(_bits(xf), _bits(x)), f"{what}: x differs from the f32 load in {np.count_nonzero(_bits(xf) != _bits(x))} slots"
        assert np.array_equal(_bits(pf), _bits(p)), f"{what}: predictions differ from the f32 load"
        assert [rp.table_checksum(t) for t in ph.TABLES] == sums
    finally:
        for o in closing:
            o.close()


def test_the_switch(ctx):
    c = ctx(4, 4)
    q, closing = c.reqs[0], []
    try:
        _refused(c.rf.enable_packed_head_requests, "f32")
        closing.append(fw.Regressor(make_pair(4, 4, 14, 14, fw.Optimizer.AdagradLUT)[0]))
        closing.append(closing[0].pack())
        _refused(closing[1].enable_packed_head_requests, "no deep head")
        _, _, r = P.new_regressor_from_filename(c.q, immutable=True, packed=True, packed_head=True)
        wb, ob = r.batch(q.whole_fbs[:8]), r.batch(q.own_fbs[:8])
        closing[:0] = [wb, ob, r]
        r.learn_batch(wb, capi.MODE_HOGWILD, False)
        before = wb.predictions().copy()
        _refused(lambda: r.setup_cache(q.ctx_fb), "packed")  # before the switch: no cache, as ever
        assert not r.packed_head_requests_state()
        r.enable_packed_head_requests()
        assert r.packed_head_requests_state()
        assert "a packed regressor with a deep head keeps no context cache" in _refused(r.enable_packed_caches, "head")
        assert "the deep head of a packed regressor is served from whole examples only" in _refused(r.enable_head_requests, "head")
        r.learn_batch(wb, capi.MODE_HOGWILD, False)  # a batch without a cache: the route and the bits it had
        assert r.last_route() == capi.ROUTE_PACKED_HEAD and np.array_equal(_bits(wb.predictions()), _bits(before))
        cache = r.setup_cache(q.ctx_fb)
        closing.insert(0, cache)
        ob.set_caches([cache], np.zeros(8, dtype=np.uint32))
        p, _ = _launch(r, ob, capi.KERNEL_PACKED_HEAD_REQUESTS)
        hc._close(p, before, PRED_TOL, "4x4: a set against the whole lines")
        _refused(lambda: r.learn_batch(ob, capi.MODE_HOGWILD, True), "predict-only: update must be 0")
        ob.set_cache(cache)  # the set of ONE
        assert np.array_equal(_bits(_launch(r, ob, capi.KERNEL_PACKED_HEAD_REQUESTS)[0]), _bits(p))
        hc._close([r.predict_with_cache(e, None, cache) for e in q.whole_fbs[:3]], before[:3], PRED_TOL, "4x4: predict_with_cache against the whole lines")
    finally:
        for o in closing:
            o.close()


def test_serving_packed_head_requests_in_one_call(ctx):
    c = ctx(30, 16)
    ctxs = [hc._line({i: " ".join(f"{1000 + 100 * r + 10 * i + j}:{hc.VALUES[(i + j + r) % 4]}" for j in range((i + r) % 3))
                      for i in range(20) if (i + r) % 3}).rstrip("\n") + " " for r in range(3)]
    cands = [hc._line(x) for x in hc._serving_texts(c.F, 40)[1]]
    prs = []
    try:
        for flags in ("--packed_weights --packed_head_requests", "--head_requests", "--packed_weights"):
            proto = serving.Predictor(f"fw -i {c.q} -t --foreground {flags}")
            prs.append([proto, proto.clone_lite(), proto.clone_lite()])
            assert [pr.setup_cache(text + "\n") for pr, text in zip(prs[-1], ctxs)] == [0.0] * 3
        packed, f32, whole = prs
        outs = serving.predict_requests(packed, [cands] * 3)
        for r, (out, want) in enumerate(zip(outs, serving.predict_requests(f32, [cands] * 3))):
            assert out.min() > 0.0 and np.array_equal(_bits(out), _bits(want)), f"request {r} differs from the f32 --head_requests load"
            hc._close(out, whole[r].predict_batch([ctxs[r] + s for s in cands]), PRED_TOL, f"request {r} against the whole-line packed predictor")
            hc._close(out, packed[r].predict_batch(cands, with_cache=True), PRED_TOL, f"request {r} against predict_batch(with_cache)")
            hc._close(out[:2], [packed[r].predict_with_cache(s) for s in cands[:2]], PRED_TOL, f"request {r} against fw_predict_with_cache")
        _refused(lambda: serving.predict_requests(whole, [cands] * 3), "keeps no device cache")
    finally:
        for pr in sum(prs, []):
            pr.close()
