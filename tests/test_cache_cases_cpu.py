"""tests/cache_cases.py where no GPU is needed: every request set of the cached-predict matrix shows the field classes it promises, its float64
predictions spread, its buffers and records are what the host translator makes of them, a correct float32 pass in the cached order stays far inside
ffm_ref.judge_prediction's bound, and four planted faults of the cached route do not."""
from types import SimpleNamespace

import numpy as np
import pytest

import cache_cases as cc
import ffm_ref

_SETS = {}


def _set(F, k):
    """the shape's request set, its warm tables and the float64 reference of every WHOLE request: made once, shared, left unchanged"""
    if (F, k) not in _SETS:
        rs = cc.request_set(F, k)
        w, _, lr = cc.warm_tables(F, k, rs.ffm_bits, rs.bits)
        cfg = SimpleNamespace(F=F, k=k)
        ref = [ffm_ref.predict(cfg, w, lr, q.lr, q.ffm) for q in rs.requests]
        _SETS[(F, k)] = (rs, w, lr, ref)
    return _SETS[(F, k)]


SHAPES = pytest.mark.parametrize("F,k", cc.CACHED_SHAPES, ids=[f"{F}x{k}" for F, k in cc.CACHED_SHAPES])


@SHAPES
def test_every_field_class_is_forced(F, k):
    rs = _set(F, k)[0]
    nine = {(c, n) for c in range(3) for n in range(3)}
    assert len(rs.requests) == cc.N_REQUESTS
    assert cc.classes(rs) == nine
    assert cc.classes(rs, rs.requests[2:cc.N_RECORD_ROUTE]) == nine, "the record route's candidates alone"
    assert cc.classes(rs, rs.requests[cc.N_RECORD_ROUTE:]) == nine, "the entry-only requests alone"
    # every field is filled by some request: by the context, or by a candidate
    assert all(rs.c[f] > 0 or any(q.n[f] > 0 for q in rs.requests) for f in range(F))
    # a context that holds the same feature twice, and one that holds two different ones
    two = [rs.ctx_slots[f] for f in range(F) if rs.c[f] == 2]
    assert any(s[0][0] == s[1][0] for s in two) and any(s[0][0] != s[1][0] for s in two)
    q0, q1 = rs.requests[0], rs.requests[1]
    assert len(q0.rest) == 0 and np.array_equal(q0.ffm, rs.ctx_ffm) and np.array_equal(q0.lr, rs.ctx_lr)
    assert len(q1.rest) > 0 and set(q1.lr["hash"].tolist()) <= set(rs.ctx_lr["hash"].tolist())
    P = cc.next_pow2(k)
    cached = set(zip(rs.ctx_ffm["hash"].tolist(), rs.ctx_ffm["contra_field_index"].tolist()))
    for r, q in enumerate(rs.requests):
        assert np.all(q.ffm["hash"] % P == 0) and int(q.ffm["hash"].max()) < 1 << rs.ffm_bits
        assert len(q.ffm) == len(rs.ctx_ffm) + len(q.rest) and len(q.lr) == len(q.ffm)
        assert not cached & set(zip(q.rest["hash"].tolist(), q.rest["contra_field_index"].tolist())), "the filter would drop a feature of the candidate's own"
        assert q.record_route == (r < cc.N_RECORD_ROUTE)
        slots, ctx_slots = q.rec[3:3 + rs.n_ns], rs.ctx_rec[3:3 + rs.n_ns]
        covered = ctx_slots != cc.NO_FEATURES
        assert np.array_equal(covered[:F], rs.c > 0) and not covered[F:].any()
        # the record route's condition (fwgpu_block_cache_record_ok): no covered slot of the merged record differs from the context's
        assert np.array_equal(slots[covered], ctx_slots[covered]) == q.record_route
        H = 3 + rs.n_ns
        assert np.array_equal(q.rec[1:3], rs.ctx_rec[1:3]) and np.array_equal(q.rec[H:len(rs.ctx_rec)], rs.ctx_rec[H:]), "the context's words stay where they are"
        assert q.rec[0] == len(q.rec)
    assert rs.n_ns <= 64 or (rs.n_ns + 31) // 32 == 3


@SHAPES
def test_buffers_and_records_are_the_host_translators(F, k):
    import fwumious_wabbit_amd as fw

    rs = _set(F, k)[0]
    fbt = fw.FeatureBufferTranslator(cc.models(rs))
    assert fbt.ffm_hash_mask & ((1 << rs.ffm_bits) - 1) == ((1 << rs.ffm_bits) - 1) & ~(cc.next_pow2(k) - 1)
    for rec, lr, ffm in [(rs.ctx_rec, rs.ctx_lr, rs.ctx_ffm), (rs.empty_rec, rs.ctx_lr[:0], rs.ctx_ffm[:0])] + [(q.rec, q.lr, q.ffm) for q in rs.requests]:
        fb = fbt.translate(rec)
        assert np.array_equal(fb.lr_buffer, lr) and np.array_equal(fb.ffm_buffer, ffm)


@SHAPES
def test_float64_predictions_spread(F, k):
    """the bound is never the cap and never that of a saturated sigmoid: the reference alone decides the seed (cache_cases.SEED_BUMP)"""
    rs, w, lr, ref = _set(F, k)
    p = np.array([r[0] for r in ref])
    M = np.array([r[1] for r in ref])
    print(f"CACHECASES {F}x{k}: p in [{p.min():.3f}, {p.max():.3f}], std {p.std():.3f}, C_P M_p up to {ffm_ref.C_P * M.max():.2e}")
    assert p.std() > 0.05 and p.min() >= 0.02 and p.max() <= 0.98
    assert ffm_ref.C_P * M.max() < ffm_ref.PRED_CAP


@SHAPES
def test_clean_float32_pass_in_the_cached_order_meets_the_bar(F, k):
    rs, w, lr, ref = _set(F, k)
    worst = 0.0
    for r, q in enumerate(rs.requests):
        p = cc.emulate_cached(F, k, w, lr, rs.ctx_ffm, (q.lr, q.rest))
        err, bound, need = ffm_ref.judge_prediction(p, *ref[r])
        worst = max(worst, need)
        assert err <= bound, (r, float(p), ref[r], err, bound, need)
        # ... and from an empty cache (everything gathered) it is the plain pass
        p0 = cc.emulate_cached(F, k, w, lr, rs.ctx_ffm[:0], (q.lr, q.ffm))
        err, bound, _ = ffm_ref.judge_prediction(p0, *ref[r])
        assert err <= bound, (r, "empty context")
    print(f"CACHECASES {F}x{k}: the float32 emulation needs c_p = {worst:.3e} = {worst / ffm_ref.C_P:.3f} C_P")


@SHAPES
def test_planted_faults_fail_the_judge(F, k):
    rs, w, lr, ref = _set(F, k)
    for fault in cc.FAULTS:
        failed = 0
        for r, q in enumerate(rs.requests):
            p = cc.emulate_cached(F, k, w, lr, rs.ctx_ffm, (q.lr, q.rest), fault=fault)
            err, bound, _ = ffm_ref.judge_prediction(p, *ref[r])
            failed += err > bound
        print(f"CACHECASES {F}x{k}: fault {fault!r} fails {failed} of {len(rs.requests)} requests")
        assert failed >= (len(rs.requests) // 2 if fault in ("dcf", "count") else 1), fault
