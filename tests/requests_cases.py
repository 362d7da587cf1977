"""Cache sets for the requests route (fwgpu_batch_set_caches: candidates of many requests in one launch, a context cache per example), and that route
restated in float32 numpy.  Pure numpy; nothing here touches the device.

PER SHAPE four caches: the contexts of cache_cases.request_set(F, k), request_set(F, k, 9001) and request_set(F, k, 9002) -- a shape's table sizes do
not depend on the seed, so one model and one set of warm tables serves all three -- and a fourth set up from no FFM feature (ctx_ffm[:0]).
96 candidates: the 24 requests of each set against their own context (the entries the filter leaves), and the 24 requests of the first set against
the empty cache with nothing filtered; interleaved round-robin over the caches, so neighbouring waves never share one.  Request 0 of each set leaves
no FFM entry: it must read base + LR.

emulate() is the regrouped pass (requests.hip) with strictly sequential float32 sums, and five planted faults."""
from types import SimpleNamespace

import numpy as np

import cache_cases as cc
import ffm_ref

# the shapes of tests/test_gpu_requests.py: R = 24 (most lanes idle); config C's; k no power of two (a real division; 252 floats: the last lane
# empty); two chunks full, nearly empty and config E's; a field slot across the chunk boundary; three chunks and the largest LDS slice
SHAPES = [(6, 4), (30, 8), (20, 12), (21, 12), (16, 32), (5, 64), (30, 16), (30, 12), (40, 16)]
SEEDS = (None, 9001, 9002)
EXTRA_SEEDS = {}  # (F, k) -> the two extra seeds, where the default ones leave a planted fault green (the float64 reference alone decides)
FAULTS = ("base", "cache0", "cross", "self", "chunk")
N_CACHES = 4

_CASES = {}


def case(F, k):
    """the shape's sets, tables, candidates and float64 references: made once, shared, left unchanged"""
    if (F, k) in _CASES:
        return _CASES[(F, k)]
    seeds = (None,) + tuple(EXTRA_SEEDS.get((F, k), SEEDS[1:]))
    sets = [cc.request_set(F, k, s) for s in seeds]
    rs = sets[0]
    assert all((s.ffm_bits, s.bits, s.n_ns) == (rs.ffm_bits, rs.bits, rs.n_ns) for s in sets)
    w, acc, lr = cc.warm_tables(F, k, rs.ffm_bits, rs.bits)
    cfg = SimpleNamespace(F=F, k=k)
    contexts = [(s.ctx_lr, s.ctx_ffm) for s in sets] + [(rs.ctx_lr, rs.ctx_ffm[:0])]
    per_cache = [[SimpleNamespace(cache=c, request=r, lr=q.lr, rest=q.rest, whole=q.ffm) for r, q in enumerate(s.requests)] for c, s in enumerate(sets)]
    per_cache.append([SimpleNamespace(cache=3, request=r, lr=q.lr, rest=q.ffm, whole=q.ffm) for r, q in enumerate(rs.requests)])
    cands = [per_cache[c][j] for j in range(cc.N_REQUESTS) for c in range(N_CACHES)]  # round-robin, not grouped
    for x in cands:
        x.ref = ffm_ref.predict(cfg, w, lr, x.lr, x.whole)
    out = SimpleNamespace(F=F, k=k, R=F * k, sets=sets, rs=rs, w=w, acc=acc, lr=lr, cfg=cfg, contexts=contexts, cands=cands)
    _CASES[(F, k)] = out
    return out


def _seq(x):
    """the strictly sequential float32 sum of x"""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    return np.float32(np.cumsum(x, dtype=np.float32)[-1]) if len(x) else np.float32(0.0)


class Cache:
    """what fwgpu_setup_cache leaves: d_T (F x R; row f holds (S[z][f], z = 0..F-1)), dcf, and base(S)"""

    def __init__(self, F, k, w, ctx_ffm):
        R = F * k
        S, self.dcf, cnt = np.zeros((F, R), np.float32), np.zeros(F, np.float32), np.zeros(F, np.int64)
        cc._sums(F, k, np.asarray(w, dtype=np.float32), ctx_ffm, S, self.dcf, cnt)
        S3 = S.reshape(F, F, k)
        self.T = np.ascontiguousarray(S3.transpose(1, 0, 2)).reshape(F, R)  # T[f][z k + kk] = S[z][f][kk]
        pairs = [S3[f, z] * S3[z, f] for f in range(F) for z in range(f + 1, F)]
        diag = [np.float32(0.5) * (_seq(S3[f, f] * S3[f, f]) - self.dcf[f]) for f in range(F)]
        self.base = _seq([_seq(np.concatenate(pairs)) if pairs else np.float32(0.0), _seq(diag)])


def caches(cs):
    if not hasattr(cs, "emu_caches"):
        cs.emu_caches = [Cache(cs.F, cs.k, cs.w, ctx_ffm) for _, ctx_ffm in cs.contexts]
    return cs.emu_caches


def emulate(cs, x, fault=None):
    """the prediction of candidate x on the requests route, float32 throughout.  fault: None or one of FAULTS --
        "base"    base(S) left out
        "cache0"  every candidate read against cache 0
        "cross"   the cross term of two gathered fields dropped
        "self"    the candidate's own self-pair term dropped
        "chunk"   floats 256.. of a cache row read from floats 0.. (shapes of more than one chunk)"""
    assert fault is None or fault in FAULTS
    F, k, R = cs.F, cs.k, cs.R
    c = caches(cs)[0 if fault == "cache0" else x.cache]
    w = np.asarray(cs.w, dtype=np.float32)
    D, ddcf, n = np.zeros((F, R), np.float32), np.zeros(F, np.float32), np.zeros(F, np.int64)
    cc._sums(F, k, w, x.rest, D, ddcf, n)
    D3 = D.reshape(F, F, k)
    C = [f for f in range(F) if n[f]]
    terms = [_seq(np.asarray(cs.lr, dtype=np.float32)[2 * x.lr["hash"].astype(np.int64)] * x.lr["value"])]
    if fault != "base":
        terms.append(c.base)
    for f in C:
        row = c.T[f]
        if fault == "chunk" and R > 256:
            row = row.copy()
            row[256:] = c.T[f][:R - 256]
        terms.append(_seq(D[f] * row))
    if fault != "cross":
        terms += [_seq(D3[f, z] * D3[z, f]) for i, f in enumerate(C) for z in C[i + 1:]]
    if fault != "self":
        terms += [np.float32(0.5) * (_seq(D3[f, f] * D3[f, f]) - ddcf[f]) for f in C]
    logit = _seq(terms)
    if np.isnan(logit):
        return np.float32(0.5)
    logit = np.float32(min(max(logit, np.float32(-50.0)), np.float32(50.0)))
    return np.float32(1.0) / (np.float32(1.0) + np.exp(-logit, dtype=np.float32))


def applies(cs, fault):
    """the candidates a fault can move at all"""
    if fault == "chunk":
        return cs.cands if cs.R > 256 else []
    if fault == "cache0":
        return [x for x in cs.cands if x.cache != 0]
    return cs.cands
