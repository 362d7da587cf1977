"""Context-cached predict launches per request against float64 (tests/ffm_ref.py), on every kernel family they are dispatched to.

The cached cases of test_gpu_parity.py compare the device with itself (cached against plain, 5e-6) on random contexts and on four shapes.  Here every
shape of cache_cases.CACHED_MATRIX -- the smallest at which each branch of the cached gather is taken: the scalar kernel beyond one chunk, the generic
16-byte kernel at all, the resident kernel where e0 / k is a real division and where the second chunk is nearly empty, cover bitmaps of three words --
serves the 24 requests of cache_cases.request_set, in which all nine classes {0, 1, 2} cached x {0, 1, 2} gathered features of a field occur by
construction, and EVERY prediction of EVERY route is held to

    |p - p_ref| <= min(C_P * M_p + 4 ulp(p), 5e-5)                      (ffm_ref.judge_prediction; C_P measured on the oracle, ffm_ref.C_P)

with p_ref the float64 forward pass over the WHOLE request (context + candidate) on the device's own tables.  The routes: predict_with_cache (one call
per request); an entry batch of the filtered buffers with the cache attached, concurrent and in order; for requests 0-15 a record batch of the merged
records after cover_record, concurrent and in order.  The kernel family and the chunks per row are asserted from Regressor.last_launch after every
cached launch and after setup_cache, so a later dispatch change cannot move a case onto another kernel unnoticed.

What would turn which case red (planted in float32 numpy, tests/test_cache_cases_cpu.py): dcf not carried over from the cache, the diagonal's count rule
on the gathered features alone (both: at least half of every set's requests); a cached row's second chunk read from its first (every shape of more
than one chunk); a field the candidate leaves empty filled with zeros instead of the cache's sums.

The serving routes (Predictor: predict_text from candidate-only records that never leave the device, predict_batch, fw_predict_with_cache, fw_predict)
are held to the same bar on one shape per family."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

import cache_cases as cc
import ffm_ref
import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import _capi as capi

pytestmark = pytest.mark.gpu

FAMILY = {"scalar": capi.KERNEL_SCALAR, "vec4": capi.KERNEL_VEC4, "resident": capi.KERNEL_RESIDENT}
TABLES = (capi.TABLE_FFM_W, capi.TABLE_FFM_ACC, capi.TABLE_LR)
MODES = (("concurrent", capi.MODE_HOGWILD), ("in order", capi.MODE_SEQUENTIAL))
CASES = [dict(F=F, k=k, family=fam, chunks=ch) for F, k, fam, ch in cc.CACHED_MATRIX]
CASES += [dict(F=6, k=4, family="scalar", chunks=1, shift=2),           # rows 2 floats off the 16-byte boundary (raw entries): the entry route only
          dict(F=30, k=8, family="vec4", chunks=1, kernel_version=1)]  # the generic kernel forced onto a shape of the resident one


def _id(c):
    return "-".join(f"{k}{v}" for k, v in c.items())


def _fb(lr, ffm):
    return fw.FeatureBuffer(label=0.0, example_importance=1.0, example_number=0, lr_buffer=lr, ffm_buffer=ffm)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _launch(re, b, mode, expect):
    re.learn_batch(b, mode, False)
    info = re.last_launch()
    assert (info["family"], info["chunks"]) == expect, info
    return b.predictions().copy()


def _routes(re, fbt, rs, cache, ctx_rec, expect, records, n_record=cc.N_RECORD_ROUTE):
    """every cached route's predictions: {route: float32[requests]} (the record routes: the first n_record requests)"""
    out = {}
    single = []
    for q in rs.requests:
        single.append(re.predict_with_cache(_fb(q.lr, q.ffm), None, cache))
        info = re.last_launch()
        if len(cache.filter(q.ffm)) or records:  # (unaligned rows: a launch that gathers no row has none off the boundary)
            assert (info["family"], info["chunks"]) == expect, info
    out["predict_with_cache"] = np.array(single, dtype=np.float32)
    eb = re.batch([_fb(q.lr, cache.filter(q.ffm)) for q in rs.requests])
    try:
        eb.set_cache(cache)
        for name, mode in MODES:
            out[f"entries, {name}"] = _launch(re, eb, mode, expect)
        eb.set_cache(None)
    finally:
        eb.close()
    if records:
        cache.cover_record(fbt, ctx_rec)
        recs = [q.rec for q in rs.requests[:n_record]]
        off = np.zeros(len(recs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(r) for r in recs])
        rb = re.record_batch(fbt, np.concatenate(recs), off)
        try:
            rb.set_cache(cache)
            for name, mode in MODES:
                out[f"records, {name}"] = _launch(re, rb, mode, expect)
            rb.set_cache(None)
        finally:
            rb.close()
    return out


def _judge(tag, routes, ref):
    worst_all = 0.0
    for route, p in routes.items():
        assert np.all(np.isfinite(p)), (tag, route)
        worst = 0.0
        for i in range(len(p)):
            err, bound, need = ffm_ref.judge_prediction(p[i], *ref[i])
            worst = max(worst, need)
            assert err <= bound, f"{tag} {route}, request {i}: prediction {p[i]!r}, float64 {ref[i][0]!r}: |d| = {err:.3e}, bound {bound:.3e} (needs c_p = {need:.3e}, C_P = {ffm_ref.C_P:.3e})"
        print(f"CACHEDPREDICT {tag} {route}: needs c_p = {worst:.3e} = {worst / ffm_ref.C_P:.3f} C_P")
        worst_all = max(worst_all, worst)
    return worst_all


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_cached_routes_per_request(c):
    F, k, shift = c["F"], c["k"], c.get("shift", 0)
    expect = (FAMILY[c["family"]], c["chunks"])
    records = not shift
    base = cc.request_set(F, k)
    rs = cc.shifted(base, shift) if shift else base
    mi = cc.models(base)
    cfg = SimpleNamespace(F=F, k=k)
    fbt = fw.FeatureBufferTranslator(mi)
    re = fw.Regressor(mi)
    caches = []
    try:
        if "kernel_version" in c:
            capi.check(re.L.fwgpu_debug_set_kernel_version(re.h, c["kernel_version"]))
        for t, v in zip(TABLES, cc.warm_tables(F, k, base.ffm_bits, base.bits)):
            assert re.table_len(t) == len(v)
            re.table_write(t, v)
        w, lr = re.table_read(capi.TABLE_FFM_W), re.table_read(capi.TABLE_LR)
        sums = [re.table_checksum(t) for t in TABLES]
        ref = [ffm_ref.predict(cfg, w, lr, q.lr, q.ffm) for q in rs.requests]
        tag = f"{F}x{k}" + (f" shift={shift}" if shift else "") + (" generic kernel forced" if "kernel_version" in c else "")

        # ---- before any cache exists: the plain predict-only launch of the whole requests
        whole = re.batch([_fb(q.lr, q.ffm) for q in rs.requests])
        plain = _launch(re, whole, capi.MODE_HOGWILD, expect)
        _judge(tag, {"no cache": plain}, ref)

        # ---- the context's cache
        cache = re.setup_cache(_fb(rs.ctx_lr, rs.ctx_ffm))
        caches.append(cache)
        info = re.last_launch()
        assert (info["family"], info["chunks"]) == expect, ("setup_cache", info)
        keys = set(zip(rs.ctx_ffm["hash"].tolist(), rs.ctx_ffm["contra_field_index"].tolist()))
        for q in rs.requests:
            rest = cache.filter(q.ffm)
            assert np.array_equal(rest, q.rest)  # the entries outside the context, order kept
            assert not keys & set(zip(rest["hash"].tolist(), rest["contra_field_index"].tolist()))
        fresh = _routes(re, fbt, rs, cache, base.ctx_rec, expect, records)
        if records:
            assert [cache.record_ok(fbt, q.rec) for q in rs.requests] == [q.record_route for q in rs.requests]
        _judge(tag, fresh, ref)

        # ---- an empty context: a setup_cache of no FFM feature; everything is gathered, from zero sums
        empty = re.setup_cache(_fb(rs.ctx_lr, rs.ctx_ffm[:0]))
        caches.append(empty)
        assert all(len(empty.filter(q.ffm)) == len(q.ffm) for q in rs.requests)
        _judge(tag + " empty context", _routes(re, fbt, rs, empty, base.empty_rec, expect, records, n_record=cc.N_REQUESTS), ref)

        # ---- refill: a cache set up from a larger context, then refilled on the same handle with the real one, gives the bits of a fresh cache
        big = rs.requests[cc.REFILL_REQUEST]
        again = re.setup_cache(_fb(big.lr, big.ffm))
        caches.append(again)
        if records:
            again.cover_record(fbt, big.rec)
        assert re.setup_cache(_fb(rs.ctx_lr, rs.ctx_ffm), again) is again
        refilled = _routes(re, fbt, rs, again, base.ctx_rec, expect, records)
        assert refilled.keys() == fresh.keys()
        for route in fresh:
            assert np.array_equal(_bits(refilled[route]), _bits(fresh[route])), (tag, route, "a refilled cache differs from a fresh one")

        # ---- nothing was written; a batch the cache is taken off again is the batch it was
        assert [re.table_checksum(t) for t in TABLES] == sums
        whole.set_cache(cache)
        whole.set_cache(None)
        assert np.array_equal(_bits(_launch(re, whole, capi.MODE_HOGWILD, expect)), _bits(plain))
        whole.close()
    finally:
        for x in caches:
            x.close()
        re.close()


def test_the_matrix_holds_the_cases_it_claims():
    """generic 16-byte and scalar at two or more chunks, resident with k no power of two (k_log2 = 0xff) and with a nearly empty second chunk, a cover
    bitmap of more than one word"""
    m = cc.CACHED_MATRIX
    assert any(fam == "vec4" and ch >= 2 for _, _, fam, ch in m) and any(fam == "scalar" and ch >= 2 for _, _, fam, ch in m)
    assert any(fam == "resident" and k & (k - 1) for _, k, fam, _ in m)
    assert (5, 64, "resident", 2) in m and any(F + min(F, 4) > 64 for F, _, _, _ in m)


# ------------------------------------------------------------------ the serving routes, one shape per family
CTX = "|A ca |Bb cb1 cb2:0.5 "
UNCOVERED = ["C", "Ddd", "E", "F"]  # namespaces the context leaves to the candidates (tests/test_gpu_serving_text.py)
SERVING = [(4, "resident", 1), (10, "scalar", 1), (24, "resident", 1), (64, "resident", 2), (48, "vec4", 2)]
SERVING_SEED = {24: 125}  # k -> the candidates' seed where the default (100 + k) draws an unsaturated candidate beyond the cap (see the test)


@pytest.mark.parametrize("k,family,chunks", SERVING, ids=[f"k{k}-{fam}" for k, fam, _ in SERVING])
def test_serving_routes_per_request(tmp_path, k, family, chunks):
    from fwumious_wabbit_amd import persistence as P
    from fwumious_wabbit_amd.feed import VowpalParser, VwNamespaceMap
    from fwumious_wabbit_amd.serving import Predictor
    from helpers import make_pair
    from text_candidates import CSV, gen_candidate

    F = 6
    vw = VwNamespaceMap(CSV)
    mi, _, _ = make_pair(F, k, 12, 12, fw.Optimizer.AdagradLUT)
    re = fw.Regressor(mi)
    host = VowpalParser(vw)
    pr = None
    try:
        for t, v in zip(TABLES, cc.warm_tables(F, k, 12, 12, seed=9)):
            assert re.table_len(t) == len(v)
            re.table_write(t, v)
        w, lr = re.table_read(capi.TABLE_FFM_W), re.table_read(capi.TABLE_LR)
        path = str(tmp_path / "model.fw")
        P.save_regressor_to_filename(path, mi, vw, re)
        pr = Predictor(f"fw -i {path} -t --foreground")
        rng = random.Random(SERVING_SEED.get(k, 100 + k))
        cands = [gen_candidate(rng, namespaces=UNCOVERED, f32_nan=False) + "\n" for _ in range(40)]
        # the reference: the host parser's record of context + candidate, translated, in float64 on the twin's tables
        fbt = fw.FeatureBufferTranslator(mi)
        fbs = [fbt.translate(host.next_vowpal((CTX + c).encode())) for c in cands]
        cfg = SimpleNamespace(F=F, k=k)
        ref = [ffm_ref.predict(cfg, w, lr, fb.lr_buffer, fb.ffm_buffer) for fb in fbs]
        # (the reference alone decides the seed: gen_candidate's weights reach 750, and a candidate whose C_P * M_p exceeds the cap is held to a bound that is
        # no bound of float32 sums -- unless its sigmoid is saturated, where an error of the logit does not reach p.  The cap binds nowhere else.)
        assert all(ffm_ref.C_P * M_p < ffm_ref.PRED_CAP or min(p, 1.0 - p) < 1e-6 for p, M_p in ref)
        # the family, on the twin regressor of the same ModelInstance
        b = re.batch(fbs)
        plain = _launch(re, b, capi.MODE_HOGWILD, (FAMILY[family], chunks))
        b.close()
        cache = re.setup_cache(fbt.translate(host.next_vowpal(CTX.encode())))
        info = re.last_launch()
        cache.close()
        assert (info["family"], info["chunks"]) == (FAMILY[family], chunks), info
        assert pr.setup_cache(CTX + "\n") == 0.0
        text = pr.predict_text("".join(cands).encode(), with_cache=True)
        assert pr.last_text_route() == (40, 0, False)  # the candidate-only records never left the device
        routes = {"twin, no cache": plain, "predict_text": text, "predict_batch": pr.predict_batch(cands, with_cache=True),
                  "fw_predict_with_cache": np.array([pr.predict_with_cache(c) for c in cands], dtype=np.float32),
                  "fw_predict": np.array([pr.predict(CTX + c) for c in cands], dtype=np.float32)}
        assert np.array_equal(_bits(routes["predict_text"]), _bits(routes["predict_batch"]))
        p_ref = np.array([r[0] for r in ref])
        print(f"CACHEDPREDICT serving 6x{k}: float64 p in [{p_ref.min():.3f}, {p_ref.max():.3f}], std {p_ref.std():.3f}")
        _judge(f"serving 6x{k}", routes, ref)
    finally:
        if pr is not None:
            pr.close()
        host.close()
        re.close()
