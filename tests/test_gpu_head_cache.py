"""Deep-head models served through the context cache (context_cache.cpp fwgpu_setup_cache / fwgpu_predict_with_cache / fwgpu_batch_set_cache, serving.cpp).

The cache keeps, next to the context's field sums T and self-pair corrections dcf, how many features it holds per field.  With c the cached and n the
gathered count of a field, the head's input diagonal is: c == 0 -- what an uncached launch computes; c + n <= 1 -- exactly 0; otherwise
0.5 (|T_ff|^2 - dcf_f) with the cache's share in both (kernels.hip nn_forward and the v2 kernel's emit_x epilogue).

The yardstick is never the cached route itself: it is the uncached prediction of the WHOLE example (context + candidate) on the device, the CPU oracle's
prediction of it, and head_ref.head_inputs64 of it.  Tolerances, all stated elsewhere in this suite:
  * CACHE_TOL (5e-6, test_gpu_parity.py) between a cached prediction and the plain prediction of the same launch route (batched against batched,
    per example against Regressor.predict);
  * PRED_TOL / LOGLOSS_TOL per example against the oracle, and PRED_TOL between the batched and the per-example forward -- the bars
    test_gpu_head_predict.py holds the uncached batched route to;
  * head inputs slot by slot within 2e-5 * sum|terms| + 1e-6 of the float64 restatement and bit-zero where the reference defines 0
    (test_gpu_head_predict._assert_head_inputs).
Shapes: F = 4, k = 4, head 1 x 10 (single-chunk v2 kernel); F = 30, k = 16, head 2 x 32 (two-chunk v2 kernel, R = 480); F = 3, k = 10, head 1 x 10 (the
generic kernel only: never batched)."""
import os

import numpy as np
import pytest

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import _capi as capi
from fwumious_wabbit_amd import persistence as P
from fwumious_wabbit_amd.feed import VowpalParser, VwNamespaceMap
import head_ref as hr
import test_gpu_head_predict as hp
from head_ref import PRED_TOL
from helpers import make_pair
from oracle import fwo

pytestmark = pytest.mark.gpu

CACHE_TOL = 5e-6  # assert_epsilon! of the reference's *_with_cache tests (block_helpers.rs:30-40), as test_gpu_parity.py
SHAPES = {
    "s4": dict(F=4, k=4, layers=[(10, "relu")], batched=True),
    "e30": dict(F=30, k=16, layers=[(32, "relu"), (32, "relu")], batched=True),
    "g3": dict(F=3, k=10, layers=[(10, "relu")], batched=False),
}
VALUES = (0.5, 2.0, 0.75, -1.5)  # (none is 1: a value forgotten somewhere shows)
BRANCHES = {(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (0, 2), (2, 1)}  # (cached, own) feature counts of a field


class Model:
    pass


_MODELS = {}


def _model(name):
    """a head model of SHAPES[name] trained in order on 300 records, and the hashes that stream touched; built once per shape"""
    if name in _MODELS:
        return _MODELS[name]
    m = Model()
    s = m.s = SHAPES[name]
    m.name, m.F, m.k = name, s["F"], s["k"]
    m.mi, m.ocfg, m.ots = make_pair(m.F, m.k, 14, 14, fw.Optimizer.AdagradLUT)
    layers = [(w, a, "hu") for w, a in s["layers"]]
    m.mi.nn_layers = [dict(width=w, activation=a, init=i) for w, a, i in layers]
    m.mi.nn_topology = "one"
    m.nn = fwo.make_nn_config(layers, "one", m.mi.nn_learning_rate, m.mi.nn_power_t, m.mi.nn_init_acc_gradient)
    m.C, m.L = m.mi.num_combos, len(layers)
    m.re = fw.Regressor(m.mi)
    m.fbt = fw.FeatureBufferTranslator(m.mi)
    recs, off = fw.synth_records(m.F, 1.0, 1.1, 3000, 0.1, 5, 0, 300)
    b = m.re.record_batch(m.fbt, recs, off)
    m.re.learn_batch(b, capi.MODE_SEQUENTIAL, True)
    b.close()
    m.lr_table, m.ffm_w = m.re.table_read(capi.TABLE_LR), m.re.table_read(capi.TABLE_FFM_W)
    tr = hr.translate(m.ots, recs, off)
    m.pool_lr, pool = np.unique(tr.lr["hash"]), np.unique(tr.ffm["hash"])
    assert len(pool) >= 64
    m.pool_ctx, m.pool_own = pool[0::2], pool[1::2]  # (disjoint: a candidate never repeats a cached feature)
    m.om = fwo.Model(m.ocfg, nn=m.nn)
    m.w = None
    _MODELS[name] = m
    return m


def _context(m, counts, dup, seed):
    """the context's FFM rows, by field: counts[f] features of field f with values from VALUES; dup: a field of two holds the SAME feature twice"""
    rng = np.random.default_rng(seed)
    rows = []
    for f in range(m.F):
        hs = [int(h) for h in rng.choice(m.pool_ctx, size=2, replace=False)]
        if dup:
            hs[1] = hs[0]
        rows.append([(hs[j], VALUES[(f + j) % 4], f * m.k) for j in range(counts[f])])
    return rows


def _candidates(m, n, seed):
    """n candidates: LR entries of every combo, (e + f) % 3 own features in field f -- every field sees 0, 1 and 2 of them"""
    rng = np.random.default_rng(seed)
    out = []
    for e in range(n):
        lr = [(int(rng.choice(m.pool_lr)), VALUES[(e + c) % 4], c) for c in range(m.C)]
        own = [[(int(h), VALUES[(e + f + j + 1) % 4], f * m.k) for j, h in enumerate(rng.choice(m.pool_own, size=(e + f) % 3, replace=False))]
               for f in range(m.F)]
        out.append((lr, own, float(e & 1)))
    return out


class Request:
    """a context and n candidates: the whole examples (context rows first inside every field, as the translator orders a context + candidate line), what
    the candidates alone add, and the three yardsticks of the whole examples"""

    def __init__(self, m, ctx_rows, cands):
        self.ctx_rows = ctx_rows
        self.ctx_fb = fw.lr_and_ffm_vec([], [r for fl in ctx_rows for r in fl], 0.0, 1.0)
        self.whole = [(lr, [r for f in range(m.F) for r in ctx_rows[f] + own[f]], y, 1.0) for lr, own, y in cands]
        self.whole_fbs = [fw.lr_and_ffm_vec(lr, ffm, y, 1.0) for lr, ffm, y, _ in self.whole]
        self.own_fbs = [fw.lr_and_ffm_vec(lr, [r for fl in own for r in fl], y, 1.0) for lr, own, y in cands]
        self.branches = {(len(ctx_rows[f]), len(own[f])) for _, own, _ in cands for f in range(m.F)}
        self.y = np.array([y for _, _, y in cands], dtype=np.float32)
        self.en = hr.crafted_entries(self.whole)
        self.x64, self.sa, self.exact0 = hr.head_inputs64(m.lr_table, m.ffm_w, m.C, m.F, m.k, self.en)

    def yardsticks(self, m):
        """(oracle, Regressor.predict) of the whole examples, once"""
        if not hasattr(self, "p_o"):
            self.p_o = np.array([m.om.predict(self.en.lrs[e], self.en.ffms[e]) for e in range(self.en.n)], dtype=np.float64)
            assert np.abs(hr.logits_of(self.p_o)).max() < 20.0
            self.plain = np.array([m.re.predict(fb) for fb in self.whole_fbs], dtype=np.float32)
            hp._assert_preds(self.plain, self.p_o, self.y, f"{m.name}: Regressor.predict of the whole examples")
        return self.p_o, self.plain


_REQ = {}
COUNTS = {"distinct": lambda F: [f % 3 for f in range(F)], "duplicate": lambda F: [(f + 1) % 3 for f in range(F)]}


def _request(name, kind, n=300):
    """the crafted request of a shape: cached counts 0, 1, 2 cycling over the fields (`duplicate`: shifted by one field, and a field of two holds one
    feature twice).  The model gets its dense head weights (every slot of x matters) from the first request built, and the oracle its mirror."""
    key = (name, kind)
    if key in _REQ:
        return _model(name), _REQ[key]
    m = _model(name)
    q = Request(m, _context(m, COUNTS[kind](m.F), kind == "duplicate", seed=21), _candidates(m, n, seed=22))
    if m.w is None:
        m.w = hr.dense_head_weights(q.x64, m.s["layers"], "one", seed=3)
        assert m.re.table_len(capi.TABLE_NN_W) == m.w.size
        m.re.table_write(capi.TABLE_NN_W, m.w)
        hr.mirror_into_oracle(m.om, m.lr_table, m.ffm_w, m.w, m.L)
    _REQ[key] = q
    return m, q


def _cached_batch(m, q, cache, n, want, batched=1):
    """the first n candidates as an entry batch that holds only what they add, launched from the cache: (predictions, head inputs or None)"""
    eb = m.re.batch(q.own_fbs[:n])
    eb.set_cache(cache)
    p = hp._launch(m.re, eb, want, batched)
    x = m.re.head_inputs(n) if want == capi.ROUTE_HEAD_BATCHED else None
    eb.set_cache(None)
    eb.close()
    m.re.set_head_predict(-1)
    return p, x


def _plain_batch(m, q, n, want, batched=1):
    b = m.re.batch(q.whole_fbs[:n])
    p = hp._launch(m.re, b, want, batched)
    b.close()
    m.re.set_head_predict(-1)
    return p


def _close(a, b, tol, what):
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    print(f"{what}: max difference {d.max():.3e} (bound {tol:.1e})")
    assert d.max() < tol, f"{what}: {d.max()} at example {int(d.argmax())}"


def _check_request(m, q, cache, what):
    """every assertion on a 300-candidate cached launch: route, head inputs slot by slot, predictions against all three yardsticks"""
    p_o, plain = q.yardsticks(m)
    n = q.en.n
    want = capi.ROUTE_HEAD_BATCHED if m.s["batched"] else capi.ROUTE_FUSED
    before = [m.re.table_checksum(t) for t in hp.TABLES]
    p, x = _cached_batch(m, q, cache, n, want)
    if x is not None:
        hp._assert_head_inputs(x, q.x64, q.sa, q.exact0, what)
    hp._assert_preds(p, p_o, q.y, what + ", cached launch")
    _close(p, _plain_batch(m, q, n, want), CACHE_TOL, what + ": cached launch against the uncached launch of the whole examples")
    _close(p, plain, PRED_TOL if x is not None else CACHE_TOL, what + ": cached launch against Regressor.predict")
    assert [m.re.table_checksum(t) for t in hp.TABLES] == before
    return p


# ------------------------------------------------------------------ the diagonal rule
@pytest.mark.parametrize("kind", ["distinct", "duplicate"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_branch_of_the_diagonal_rule_in_one_cached_launch(name, kind):
    """300 candidates from one cache.  Per field the (cached, own) counts (0,0), (1,0), (0,1), (1,1), (2,0), (0,2), (2,1) all occur (and (1,2), (2,2)); values
    other than 1; `duplicate`: the context holds one feature twice in a field; fields that only the context / only the candidates fill.  Before the cache
    carried counts the first setup_cache on a head regressor raised ERR_INVALID; with only the refusals lifted the (1,0), (2,0), (1,1), (2,1) diagonals are
    wrong: (1,0) is not bit-zero, the others miss the cached features' share."""
    m, q = _request(name, kind)
    assert BRANCHES <= q.branches
    cache = m.re.setup_cache(q.ctx_fb)
    _check_request(m, q, cache, f"{name}, {kind} context")
    cache.close()


@pytest.mark.parametrize("name", list(SHAPES))
def test_below_the_threshold_and_with_the_batched_route_switched_off(name):
    """The same examples as a batch of 40 (the fused per-example kernel), one by one through predict_with_cache, and all 300 with option 14 = 0: each the
    whole example's plain prediction within CACHE_TOL (same kernel, same per-example forward) and the oracle's within PRED_TOL."""
    m, q = _request(name, "distinct")
    p_o, plain = q.yardsticks(m)
    cache = m.re.setup_cache(q.ctx_fb)
    p40, _ = _cached_batch(m, q, cache, 40, capi.ROUTE_FUSED)
    hp._assert_preds(p40, p_o[:40], q.y[:40], f"{name}: 40 cached candidates")
    _close(p40, plain[:40], CACHE_TOL, f"{name}: 40 cached candidates against Regressor.predict")
    one = np.array([m.re.predict_with_cache(fb, None, cache) for fb in q.whole_fbs[:60]], dtype=np.float32)
    hp._assert_preds(one, p_o[:60], q.y[:60], f"{name}: predict_with_cache one by one")
    _close(one, plain[:60], CACHE_TOL, f"{name}: predict_with_cache against Regressor.predict")
    p_off, _ = _cached_batch(m, q, cache, q.en.n, capi.ROUTE_FUSED, batched=0)
    hp._assert_preds(p_off, p_o, q.y, f"{name}: 300 cached candidates, option 14 = 0")
    _close(p_off, plain, CACHE_TOL, f"{name}: 300 cached candidates, option 14 = 0, against Regressor.predict")
    cache.close()


# ------------------------------------------------------------------ a refilled cache
@pytest.mark.parametrize("name", ["s4", "e30"])
def test_a_refilled_cache_refreshes_the_counts(name):
    """setup_cache twice on one handle.  The second context moves field 2 from two cached features to one and field 1 from one to none: with the first
    context's counts still in place, field 2 of a candidate that adds nothing there would take 0.5 (|T|^2 - dcf) -- not bit-zero -- and field 1 of a
    candidate with one feature there likewise (the head-input check's exact-zero rule catches both).  Then the empty context (bit-equal to the uncached
    launch: no field has a cached feature) and context == whole example (the candidates add LR entries only)."""
    m, q1 = _request(name, "distinct")
    counts = COUNTS["distinct"](m.F)
    assert counts[1] == 1 and counts[2] == 2
    counts2 = list(counts)
    counts2[1], counts2[2] = 0, 1
    cands = _candidates(m, 300, seed=22)
    q2 = Request(m, [rows[:c] for rows, c in zip(q1.ctx_rows, counts2)], cands)
    assert {(0, 1), (1, 0)} <= {(len(q2.ctx_rows[f]), len(own[f])) for _, own, _ in cands for f in (1, 2)}  # (where a stale count flips the rule)
    cache = m.re.setup_cache(q1.ctx_fb)
    _check_request(m, q1, cache, f"{name}, first context")
    assert m.re.setup_cache(q2.ctx_fb, cache) is cache
    _check_request(m, q2, cache, f"{name}, refilled with a smaller context")
    # the empty context
    q0 = Request(m, [[] for _ in range(m.F)], cands)
    m.re.setup_cache(q0.ctx_fb, cache)
    p0 = _check_request(m, q0, cache, f"{name}, empty context")
    assert np.array_equal(p0, _plain_batch(m, q0, 300, capi.ROUTE_HEAD_BATCHED))
    # context == whole example: every candidate is the first context plus LR entries
    qw = Request(m, q1.ctx_rows, [(lr, [[] for _ in range(m.F)], y) for lr, _, y in cands])
    m.re.setup_cache(qw.ctx_fb, cache)
    _check_request(m, qw, cache, f"{name}, context == whole example")
    _close([m.re.predict_with_cache(fb, None, cache) for fb in qw.whole_fbs[:10]], qw.plain[:10], CACHE_TOL, f"{name}: context == whole example, single calls")
    m.re.setup_cache(q1.ctx_fb, cache)
    _check_request(m, q1, cache, f"{name}, refilled with the first context again")
    cache.close()


# ------------------------------------------------------------------ the serving FFI
def _ns(i):
    return f"N{i:02d}"


def _line(parts):
    """{namespace: "tokens"} -> a VW line without label, namespaces in index order"""
    return " ".join(f"|{_ns(i)} {parts[i]}" for i in sorted(parts)) + "\n"


def _serving_texts(F, n):
    """A context over the first two thirds of the namespaces with 0, 1, 2 features cycling (weighted), and n candidates over the rest with 0, 1, 2 features
    per namespace; feature names are numbers (context: 1000 + ..., candidates: below 1000, so no candidate repeats a cached feature)."""
    n_ctx = max(3, 2 * F // 3)
    ctx = {i: " ".join(f"{1000 + 10 * i + j}:{VALUES[(i + j) % 4]}" for j in range(i % 3)) for i in range(n_ctx) if i % 3}
    cands = []
    for e in range(n):
        cnt = {i: (e + i) % 3 for i in range(n_ctx, F)}
        cnt[F - 1] = cnt[F - 1] or 1  # (a candidate is never an empty line)
        cands.append({i: " ".join(f"{(7 * e + 13 * i + j) % 997}:{VALUES[(e + i + j) % 4]}" for j in range(c)) for i, c in cnt.items() if c})
    return ctx, cands


@pytest.mark.parametrize("name", ["s4", "e30"])
def test_serving_ffi_on_a_saved_head_model(name, tmp_path):
    """Predictor on a saved head model: predict_batch(with_cache = True) against predict_batch(with_cache = False) of the whole lines (CACHE_TOL: with
    300 candidates both take the batched head route, with 20 both the per-example kernel) and against single predict_with_cache calls (PRED_TOL between
    the batched and the per-example forward at 300, CACHE_TOL at 20); the same with whole context + candidate records (FWGPU_SERVING_MERGED_RECORDS) and on
    the entry route (FWGPU_SERVING_ENTRY_ROUTE); a request in which one candidate names a covered namespace again -- the whole request takes the entry
    route, and that candidate's yardstick is the example whose field holds the context's features and then its own; clone_lite shares the model; a second
    setup_cache replaces the first (two cached features of a namespace become one, one becomes none)."""
    from fwumious_wabbit_amd.serving import Predictor
    m, _ = _request(name, "distinct")  # (the model with its dense head weights)
    F = m.F
    path = str(tmp_path / "head.fw")
    vw = VwNamespaceMap("".join(f"{_ns(i)},ns{i}\n" for i in range(F)))
    P.save_regressor_to_filename(path, m.mi, vw, m.re)
    pr = Predictor(f"fw -i {path} -t --foreground")
    parser = VowpalParser(vw)
    ctx, cands300 = _serving_texts(F, 300)
    ctx_text = _line(ctx).rstrip("\n") + " "
    assert pr.setup_cache(ctx_text + "\n") == 0.0

    def compare(p, parts_list, ctx_parts, text, what):
        cands = [_line(c) for c in parts_list]
        whole = pr.predict_batch([text + c for c in cands], with_cache=False)
        assert whole.min() > 0.0  # (every line parsed)
        n = len(cands)
        for env in (None, "FWGPU_SERVING_MERGED_RECORDS", "FWGPU_SERVING_ENTRY_ROUTE"):
            if env:
                os.environ[env] = "1"
            try:
                cached = p.predict_batch(cands, with_cache=True)
            finally:
                if env:
                    del os.environ[env]
            _close(cached, whole, CACHE_TOL, f"{what}, {n} candidates, {env or 'candidate-only records'}: cached against whole lines")
        k = min(n, 40)
        single = np.array([p.predict_with_cache(c) for c in cands[:k]], dtype=np.float32)
        _close(single, np.array([pr.predict(text + c) for c in cands[:k]], dtype=np.float32), CACHE_TOL, f"{what}: predict_with_cache against predict")
        _close(cached[:k], single, PRED_TOL if n >= 256 else CACHE_TOL, f"{what}, {n} candidates: batch against single calls")
        # one candidate names a covered namespace again: the entry route for the whole request
        i_cov = min(i for i in ctx_parts if ctx_parts[i])
        again = dict(parts_list[3])
        again[i_cov] = "5:0.5"
        merged = dict(ctx_parts)
        merged[i_cov] = ctx_parts[i_cov] + " 5:0.5"
        got = p.predict_batch(cands[:7] + [_line(again)] + cands[7:], with_cache=True)
        _close(np.delete(got, 7), whole, CACHE_TOL, f"{what}, {n + 1} candidates, a covered namespace named again: the other candidates")
        # (that candidate's record holds its own features of the namespace in place of the context's, parser.rs:318-326, while the cache still holds the
        # context's: the FFM block sees both, the LR block -- whose cache is inert, block_lr.rs:236-239 -- the record's.  The regressor the file was saved from
        # predicts that example whole.)
        both = m.fbt.translate(parser.next_vowpal(_line({**merged, **parts_list[3]}).encode()))
        own = m.fbt.translate(parser.next_vowpal(_line({**ctx_parts, **again}).encode()))
        ex = fw.FeatureBuffer(label=0.0, example_importance=1.0, example_number=0, lr_buffer=own.lr_buffer, ffm_buffer=both.ffm_buffer)
        _close(got[7:8], [m.re.predict(ex)], CACHE_TOL if n < 256 else PRED_TOL, f"{what}, {n + 1} candidates: the candidate that names it again")

    compare(pr, cands300, ctx, ctx_text, f"{name}")
    compare(pr, cands300[:20], ctx, ctx_text, f"{name}")
    # a clone shares the model and has a cache of its own; a second setup_cache replaces the first
    ctx2 = dict(ctx)
    i_two, i_one = (min(i for i, t in ctx.items() if len(t.split(" ")) == c) for c in (2, 1))
    ctx2[i_two] = ctx[i_two].split(" ")[0]
    del ctx2[i_one]
    ctx2_text = _line(ctx2).rstrip("\n") + " "
    cl = pr.clone_lite()
    assert cl.setup_cache(ctx2_text + "\n") == 0.0
    compare(cl, cands300, ctx2, ctx2_text, f"{name}, clone with another context")
    compare(pr, cands300[:20], ctx, ctx_text, f"{name}, the prototype's cache after the clone's")
    assert pr.setup_cache(ctx2_text + "\n") == 0.0
    compare(pr, cands300, ctx2, ctx2_text, f"{name}, second setup_cache")
    cl.close()
    pr.close()


# ------------------------------------------------------------------ unchanged ground
def test_uncached_head_launches_and_headless_cached_launches_are_what_they_were():
    """What the cache's counts must not touch, asserted in-process against the uncached route: a head model's uncached batched launch gives the same bits
    before and after cached launches on the regressor, and the same bits as a launch from the empty cache (no field has a cached feature: the uncached
    code, bit for bit); a headless model (no head, so no diagonal) from the empty cache is bit-equal to its uncached launch, from a real cache within
    CACHE_TOL of it, and its batch and single cached calls agree bit for bit as before."""
    m, q = _request("s4", "distinct")
    first = _plain_batch(m, q, 300, capi.ROUTE_HEAD_BATCHED)
    cache = m.re.setup_cache(q.ctx_fb)
    _cached_batch(m, q, cache, 300, capi.ROUTE_HEAD_BATCHED)
    cache.close()
    assert np.array_equal(_plain_batch(m, q, 300, capi.ROUTE_HEAD_BATCHED), first)
    empty = m.re.setup_cache(fw.lr_and_ffm_vec([], [], 0.0, 1.0))
    eb = m.re.batch(q.whole_fbs)
    eb.set_cache(empty)
    assert np.array_equal(hp._launch(m.re, eb, capi.ROUTE_HEAD_BATCHED), first)
    eb.set_cache(None)
    eb.close()
    empty.close()
    m.re.set_head_predict(-1)
    # headless, same geometry
    mi, _, _ = make_pair(m.F, m.k, 14, 14, fw.Optimizer.AdagradLUT)
    re = fw.Regressor(mi)
    recs, off = fw.synth_records(m.F, 1.0, 1.1, 3000, 0.1, 5, 0, 300)
    b = re.record_batch(fw.FeatureBufferTranslator(mi), recs, off)
    re.learn_batch(b, capi.MODE_SEQUENTIAL, True)
    b.close()

    def launch(fbs, cache):
        eb = re.batch(fbs)
        eb.set_cache(cache)
        re.learn_batch(eb, capi.MODE_HOGWILD, False)
        p = eb.predictions().copy()
        eb.set_cache(None)
        eb.close()
        return p

    plain = launch(q.whole_fbs, None)
    empty = re.setup_cache(fw.lr_and_ffm_vec([], [], 0.0, 1.0))
    assert np.array_equal(launch(q.whole_fbs, empty), plain)
    empty.close()
    cache = re.setup_cache(q.ctx_fb)
    cached = launch(q.own_fbs, cache)
    _close(cached, plain, CACHE_TOL, "headless: cached against uncached")
    single = np.array([re.predict_with_cache(fb, None, cache) for fb in q.whole_fbs[:40]], dtype=np.float32)
    _close(single, plain[:40], CACHE_TOL, "headless: predict_with_cache against uncached")
    cache.close()
    re.close()
