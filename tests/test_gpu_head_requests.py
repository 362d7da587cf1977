"""The requests route on a model with a deep head (fwgpu_enable_head_requests; csrc/requests_head.hip): the candidates of many requests in one launch,
each candidate's head input x formed from its context cache and its own few features, then the layers over the whole batch.

The yardstick is head_ref.head_inputs64 / head_forward64 of the WHOLE request (context + candidate) on the device's own tables: x slot by slot within
2e-5 * sum|terms| + 1e-6 and bit-zero where the reference defines 0, predictions within PRED_TOL (1e-5) of the float64 head and of the existing
per-request set_cache launch.  The bits of x and of the predictions are the same in a second launch, in MODE_SEQUENTIAL and with the candidates grouped
by cache.  Shapes: 4 x 4 (one lane per slot), 20 x 12 (three lanes per slot), 30 x 12 (R = 360: field 21's slot lies across the chunk edge),
30 x 16 (two chunks, X = 496)."""
import numpy as np
import pytest

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import _capi as capi
from fwumious_wabbit_amd import persistence as P
from fwumious_wabbit_amd import serving
from fwumious_wabbit_amd.feed import VowpalParser, VwNamespaceMap
import head_ref as hr
import test_gpu_head_cache as hc
import test_gpu_head_predict as hp
from head_ref import PRED_TOL
from helpers import make_pair

pytestmark = pytest.mark.gpu

SHAPES = {"4x4": (4, 4, [(10, "relu")]), "20x12": (20, 12, [(16, "relu")]), "30x12": (30, 12, [(16, "relu")]),
          "30x16": (30, 16, [(32, "relu"), (32, "relu")])}
N_CAND, N_CACHES = 96, 4
_MODELS = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _refused(fn, word):
    with pytest.raises(capi.FwgpuError) as e:
        fn()
    assert e.value.code == capi.ERR_INVALID and word in e.value.message, e.value
    return e.value.message


def _head_mi(F, k, layers):
    mi, _, _ = make_pair(F, k, 14, 14, fw.Optimizer.AdagradLUT)
    mi.nn_layers = [dict(width=w, activation=a, init="hu") for w, a in layers]
    mi.nn_topology = "one"
    return mi


def _model(name):
    """a head model of the shape trained in order on 300 records; three contexts (cached counts 0, 1, 2 cycling over the fields, shifted per context) and
    an empty one; 96 candidates, candidate e against cache e % 4: (e + f) % 3 own features in field f, every eighth candidate none at all; dense head
    weights that make every slot of x matter.  Built once per shape."""
    if name in _MODELS:
        return _MODELS[name]
    m = hc.Model()
    m.name = name
    m.F, m.k, m.layers = SHAPES[name]
    m.mi = _head_mi(m.F, m.k, m.layers)
    m.C = m.mi.num_combos
    m.re = fw.Regressor(m.mi)
    m.fbt = fw.FeatureBufferTranslator(m.mi)
    recs, off = fw.synth_records(m.F, 1.0, 1.1, 3000, 0.1, 5, 0, 300)
    b = m.re.record_batch(m.fbt, recs, off)
    m.re.learn_batch(b, capi.MODE_SEQUENTIAL, True)
    b.close()
    m.lr_table, m.ffm_w = m.re.table_read(capi.TABLE_LR), m.re.table_read(capi.TABLE_FFM_W)
    _, _, ots = make_pair(m.F, m.k, 14, 14, fw.Optimizer.AdagradLUT)
    tr = hr.translate(ots, recs, off)
    m.pool_lr, pool = np.unique(tr.lr["hash"]), np.unique(tr.ffm["hash"])
    m.pool_ctx, m.pool_own = pool[0::2], pool[1::2]  # (disjoint: a candidate never repeats a cached feature)
    cands = hc._candidates(m, N_CAND, seed=22)
    cands = [(lr, [[] for _ in own] if e % 8 == 5 else own, y) for e, (lr, own, y) in enumerate(cands)]
    ctxs = [hc._context(m, [(f + r) % 3 for f in range(m.F)], False, seed=21 + r) for r in range(3)] + [[[] for _ in range(m.F)]]
    m.reqs = [hc.Request(m, ctxs[r], cands[r::N_CACHES]) for r in range(N_CACHES)]
    assert {(0, 0), (1, 0), (2, 0), (0, 1), (1, 2), (2, 2)} <= set().union(*(q.branches for q in m.reqs))

    def interleaved(attr):
        out = np.empty((N_CAND,) + getattr(m.reqs[0], attr).shape[1:], dtype=getattr(m.reqs[0], attr).dtype)
        for r, q in enumerate(m.reqs):
            out[r::N_CACHES] = getattr(q, attr)
        return out

    m.x64, m.sa, m.exact0 = interleaved("x64"), interleaved("sa"), interleaved("exact0")
    m.own_fbs = [m.reqs[e % N_CACHES].own_fbs[e // N_CACHES] for e in range(N_CAND)]
    m.idx = (np.arange(N_CAND) % N_CACHES).astype(np.uint32)
    m.w = hr.dense_head_weights(m.x64, m.layers, "one", seed=3)
    m.re.table_write(capi.TABLE_NN_W, m.w)
    m.p64, z = hr.head_forward64(m.x64, m.w, m.layers, "one")
    assert np.abs(z).max() < 20.0
    _MODELS[name] = m
    return m


def _launch(m, b, mode=capi.MODE_HOGWILD):
    m.re.learn_batch(b, mode, False)
    assert m.re.last_route() == capi.ROUTE_REQUESTS and m.re.last_launch()["family"] == capi.KERNEL_HEAD_REQUESTS
    return b.predictions().copy(), m.re.head_inputs(b.n)


@pytest.mark.parametrize("name", list(SHAPES))
def test_head_requests_per_candidate(name):
    m = _model(name)
    re = m.re
    re.enable_head_requests()
    caches = [re.setup_cache(q.ctx_fb) for q in m.reqs]
    batches = []
    try:
        sums = [re.table_checksum(t) for t in hp.TABLES]
        b = re.batch(m.own_fbs)
        batches.append(b)
        b.set_caches(caches, m.idx)
        p, x = _launch(m, b)
        # ---- the launch shape: min(F, max_ffm) * R + NT floats per wave, up to four waves in 64 KiB, at least one
        R, NT = m.F * m.k, m.F * (m.F + 1) // 2
        per_wave = (min(m.F, max(len(fb.ffm_buffer) for fb in m.own_fbs)) * R + NT) * 4
        waves = min(4, max(1, (64 * 1024) // per_wave))
        info = re.last_launch()
        assert (info["chunks"], info["threads"], info["lds_bytes"]) == ((R + 255) // 256, 64 * waves, per_wave * waves), info
        # ---- x slot by slot, the predictions against the float64 head and against the per-request set_cache launch
        hp._assert_head_inputs(x, m.x64, m.sa, m.exact0, name)
        hc._close(p, m.p64, PRED_TOL, f"{name}: head requests against the float64 head")
        for r, q in enumerate(m.reqs):
            ob = re.batch(q.own_fbs)
            batches.append(ob)
            ob.set_cache(caches[r])
            re.learn_batch(ob, capi.MODE_HOGWILD, False)
            assert re.last_route() == capi.ROUTE_FUSED
            hc._close(p[r::N_CACHES], ob.predictions(), PRED_TOL, f"{name}: head requests against set_cache, request {r}")
        # ---- the same bits: again, in order, grouped by cache
        p2, x2 = _launch(m, b)
        assert np.array_equal(_bits(p2), _bits(p)) and np.array_equal(_bits(x2), _bits(x)), "two launches differ"
        p3, x3 = _launch(m, b, capi.MODE_SEQUENTIAL)
        assert np.array_equal(_bits(p3), _bits(p)) and np.array_equal(_bits(x3), _bits(x)), "MODE_SEQUENTIAL differs from MODE_HOGWILD"
        order = np.argsort(m.idx, kind="stable")
        gb = re.batch([m.own_fbs[i] for i in order])
        batches.append(gb)
        gb.set_caches(caches, m.idx[order])
        pg, xg = _launch(m, gb)
        assert np.array_equal(_bits(xg), _bits(x)[order]), "x: grouped by cache differs from interleaved"
        assert np.array_equal(_bits(pg), _bits(p)[order]), "grouped by cache differs from interleaved"
        assert [re.table_checksum(t) for t in hp.TABLES] == sums
    finally:
        for o in batches + caches:
            o.close()


def test_the_switch():
    closing = []
    try:
        # refused: no head, packed weights, k = 10
        mi, _, _ = make_pair(4, 4, 14, 14, fw.Optimizer.AdagradLUT)
        plain = fw.Regressor(mi)
        closing.append(plain)
        _refused(plain.enable_head_requests, "no deep head")
        packed = plain.pack()
        closing.append(packed)
        _refused(packed.enable_head_requests, "packed")
        k10 = fw.Regressor(_head_mi(3, 10, [(10, "relu")]))
        closing.append(k10)
        _refused(k10.enable_head_requests, "multiple of 4")
        assert not k10.head_requests_state()
        # a head model: refused before the switch exactly as ever, served after it; what stays refused keeps today's words
        m = _model("4x4")
        re = fw.Regressor(m.mi)
        closing.append(re)
        cache = re.setup_cache(m.reqs[0].ctx_fb)
        closing.insert(0, cache)
        b = re.batch(m.own_fbs[:8])
        closing.insert(0, b)
        zeros = np.zeros(8, dtype=np.uint32)
        assert not re.head_requests_state()
        assert "set_caches: models with a deep head are not served by the requests route (fwgpu_batch_set_cache serves them)" in _refused(lambda: b.set_caches([cache], zeros), "deep head")
        re.enable_head_requests()
        assert re.head_requests_state()
        b.set_caches([cache], zeros)
        re.learn_batch(b, capi.MODE_HOGWILD, False)
        assert re.last_route() == capi.ROUTE_REQUESTS and re.last_launch()["family"] == capi.KERNEL_HEAD_REQUESTS
        _refused(lambda: re.learn_batch(b, capi.MODE_HOGWILD, True), "predict-only: update must be 0")
        recs, off = fw.synth_records(m.F, 1.0, 1.1, 3000, 0.1, 5, 0, 8)
        rb = re.record_batch(fw.FeatureBufferTranslator(m.mi), recs, off)
        closing.insert(0, rb)
        _refused(lambda: rb.set_caches([cache], zeros), "a record batch is not served by the requests route")
        foreign = m.re.setup_cache(m.reqs[0].ctx_fb)
        closing.insert(0, foreign)
        _refused(lambda: b.set_caches([cache, foreign], zeros), "a cache belongs to another regressor")
    finally:
        for o in closing:
            o.close()


@pytest.mark.parametrize("name", ["4x4", "30x16"])
def test_serving_head_requests_in_one_call(name, tmp_path):
    m = _model(name)
    F = m.F
    path = str(tmp_path / "head.fw")
    vw = VwNamespaceMap("".join(f"{hc._ns(i)},ns{i}\n" for i in range(F)))
    P.save_regressor_to_filename(path, m.mi, vw, m.re)
    parser = VowpalParser(vw)
    n_ctx = max(3, 2 * F // 3)
    ctxs = [hc._line({i: " ".join(f"{1000 + 100 * r + 10 * i + j}:{hc.VALUES[(i + j + r) % 4]}" for j in range((i + r) % 3))
                      for i in range(n_ctx) if (i + r) % 3}).rstrip("\n") + " " for r in range(3)]
    cands = [hc._line(c) for c in hc._serving_texts(F, 40)[1]]
    requests = [cands[:20] + [f"|{hc._ns(F - 1)} a:b:c:d\n"] + cands[20:]] * 3
    prs = []
    try:
        prs.append(serving.Predictor(f"fw -i {path} -t --foreground --head_requests"))
        prs += [prs[0].clone_lite(), prs[0].clone_lite()]
        for pr, ctx in zip(prs, ctxs):
            assert pr.setup_cache(ctx + "\n") == 0.0
        outs = serving.predict_requests(prs, requests)
        for r, (pr, ctx, out) in enumerate(zip(prs, ctxs, outs)):
            assert len(out) == 41 and out[20] == -1.0
            got = np.delete(out, 20)
            hc._close(got, np.delete(pr.predict_batch(requests[r], with_cache=True), 20), PRED_TOL, f"{name}: request {r} against predict_batch")
            fbs = [m.fbt.translate(parser.next_vowpal((ctx + c).encode())) for c in cands]
            en = hr.Entries([np.asarray(fb.lr_buffer, dtype=hr.fwo.LR_ENTRY) for fb in fbs], [np.asarray(fb.ffm_buffer, dtype=hr.fwo.FFM_ENTRY) for fb in fbs])
            x64, _, _ = hr.head_inputs64(m.lr_table, m.ffm_w, m.C, F, m.k, en)
            p64, z = hr.head_forward64(x64, m.w, m.layers, "one")
            assert np.abs(z).max() < 20.0
            hc._close(got, p64, PRED_TOL, f"{name}: request {r} against the float64 head")
        twice = serving.predict_requests([prs[1], prs[0], prs[1]], [requests[1], requests[0], requests[1]])
        assert np.array_equal(_bits(twice[0]), _bits(outs[1])) and np.array_equal(_bits(twice[2]), _bits(outs[1])) and np.array_equal(_bits(twice[1]), _bits(outs[0]))
        plain = serving.Predictor(f"fw -i {path} -t --foreground")
        prs.append(plain)
        assert plain.setup_cache(ctxs[0] + "\n") == 0.0
        _refused(lambda: serving.predict_requests([plain], requests[:1]), "predict_requests: models with a deep head are not served by the requests route")
    finally:
        for pr in prs:
            pr.close()
        parser.close()
