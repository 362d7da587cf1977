"""tests/ffm_ref.py against the oracle, where no GPU is needed: the float64 step agrees with the oracle on the probe sets of every shape of the one-step
matrix (tests/test_gpu_ffm_step.py) within the recorded maximum that C is derived from, few enough probes are left out, and the judge turns red on
three planted faults that the stream tests' bar (2e-5 + 1e-5 |ref|) lets through."""
import numpy as np
import pytest

import ffm_ref
from ffm_ref import FLEX, LUT, MATRIX, SGD
from helpers import check_disjoint, disjoint_models
from oracle import fwo

_RUNS = {}


class _Run:
    pass


def _oracle_run(F, k, opt, cold=False, dist=None, minibatch=False, **model_kw):
    """the oracle's own step on every probe of the shape, from the warm state (cold: from freshly initialised tables, the regime of the stream tests):
    tables before / after, predictions and the verdict per probe (computed once per shape and optimizer, shared and left unchanged).
    dist = "dup" / "nodup": the multi-rank routes' probe set (ffm_ref.dist_probe_stream) instead of probe_stream's; minibatch: all probes through ONE
    call of the oracle's synchronous micro-batch mode instead of one sequential step each; model_kw: the models' constants (default: opt_kwargs)"""
    key = (F, k, opt, cold, dist, minibatch, tuple(sorted(model_kw.items())))
    if key in _RUNS:
        return _RUNS[key]
    st = ffm_ref.probe_stream(F, k) if dist is None else ffm_ref.dist_probe_stream(F, k, dist == "dup")
    mi, ocfg, ots = disjoint_models(st, opt, **(model_kw or ffm_ref.opt_kwargs(opt)))
    check_disjoint(st, mi)
    om = fwo.Model(ocfg, init=cold)
    if not cold:
        w, acc, lr = ffm_ref.warm_state(st)
        om.ffm_weights[:len(w)] = w
        om.ffm_acc[:len(acc)] = acc
        om.lr_table[:len(lr)] = lr
    r = _Run()
    r.st, r.cfg = st, ffm_ref.StepConfig.from_oracle_config(ocfg)
    r.before = (om.ffm_weights.copy(), om.ffm_acc.copy(), om.lr_table.copy())
    r.p_predict = np.array([om.predict(fb.lr_buffer, fb.ffm_buffer) for fb in st.fbs], dtype=np.float32)  # the oracle's OTHER forward pass (ffm_forward)
    if minibatch:
        r.p = om.learn_minibatch(ots, st.recs, st.off)
    else:
        r.p = np.array([om.learn(fb.lr_buffer, fb.ffm_buffer, fb.label, fb.example_importance, True) for fb in st.fbs], dtype=np.float32)
    r.after = (om.ffm_weights.copy(), om.ffm_acc.copy(), om.lr_table.copy())
    om.close()
    r.verdicts = [ffm_ref.judge_example(r.cfg, r.before, r.after, fb.lr_buffer, fb.ffm_buffer, fb.label, fb.example_importance, r.p[e])
                  for e, fb in enumerate(st.fbs)]
    r.predict_verdicts = [ffm_ref.judge_prediction(r.p_predict[e], v.ref.p, v.ref.M_p) for e, v in enumerate(r.verdicts)]
    _RUNS[key] = r
    return r


def _worst(r):
    return max(v.worst for v in r.verdicts)


def _worst_p(r):
    """the largest c_p either of the oracle's forward passes needs"""
    return max(max(v.p_ratio for v in r.verdicts), max(need for _, _, need in r.predict_verdicts))


@pytest.mark.parametrize("F,k", MATRIX, ids=[f"{F}x{k}" for F, k in MATRIX])
def test_oracle_stays_within_the_recorded_maximum(F, k):
    """AdagradLUT on every shape: the oracle needs no more than ORACLE_MAX_RATIO (C / 8) on any float; every float outside the touched rows and entries
    is bit-identical; at most one probe in ten is left out for |p - y| < 0.05; the probe set has what the matrix promises (a chained duplicate, a
    weighted feature, an empty field)."""
    r = _oracle_run(F, k, LUT)
    st = r.st
    worst = _worst(r)
    print(f"{F}x{k}: oracle max ratio {worst:.3e}, skipped {sum(v.skipped for v in r.verdicts)} of {st.n}")
    assert worst <= ffm_ref.ORACLE_MAX_RATIO, [v.where for v in r.verdicts if v.worst == worst]
    bounds = [v.p_bound for v in r.verdicts]
    print(f"{F}x{k}: oracle max p ratio {_worst_p(r):.3e}, max |p - p64| {max(v.p_err for v in r.verdicts):.3e}, prediction bound {min(bounds):.3e} .. {max(bounds):.3e}")
    assert _worst_p(r) <= ffm_ref.ORACLE_MAX_P_RATIO
    assert max(bounds) < ffm_ref.PRED_CAP  # the cap is a guarantee, not what decides on these probes
    assert sum(v.skipped for v in r.verdicts) <= ffm_ref.MAX_SKIPPED_SHARE * st.n
    touched = np.concatenate([v.ref.ffm_idx for v in r.verdicts])
    assert ffm_ref.untouched_identical(r.before[0], r.after[0], touched) and ffm_ref.untouched_identical(r.before[1], r.after[1], touched)
    lr_touched = np.concatenate([v.ref.lr_idx for v in r.verdicts])
    assert ffm_ref.untouched_identical(r.before[2], r.after[2], np.concatenate([2 * lr_touched, 2 * lr_touched + 1]))
    assert not np.array_equal(r.before[0], r.after[0]) and not np.array_equal(r.before[1], r.after[1])
    assert st.row_count.max() == 2 and np.any(st.val != 1.0)
    assert F < 8 or any(len(np.unique(fb.ffm_buffer["contra_field_index"])) < F for fb in st.fbs)
    assert np.all(np.abs([v.ref.logit for v in r.verdicts]) < 20.0)  # the warm state's logits are O(1): no probe sits on the +-50 rule


def test_the_recorded_maximum_is_reached():
    """ORACLE_MAX_RATIO is the measurement, not a round number above it: the shape named next to it reaches it (to the three digits it is recorded with)"""
    F, k = (int(x) for x in ffm_ref.ORACLE_MAX_RATIO_SHAPE.split("x"))
    assert ffm_ref.ORACLE_MAX_RATIO_SET in ("matrix", "dist")
    dist = "dup" if ffm_ref.ORACLE_MAX_RATIO_SET == "dist" else None
    assert (F, k) in (ffm_ref.DIST_MATRIX if dist else MATRIX)
    assert _worst(_oracle_run(F, k, LUT, dist=dist)) >= ffm_ref.ORACLE_MAX_RATIO * 0.99
    assert ffm_ref.C == 8 * ffm_ref.ORACLE_MAX_RATIO
    F, k = (int(x) for x in ffm_ref.ORACLE_MAX_P_RATIO_SHAPE.split("x"))
    assert (F, k) in MATRIX
    assert _worst_p(_oracle_run(F, k, LUT)) >= ffm_ref.ORACLE_MAX_P_RATIO * 0.99
    assert ffm_ref.C_P == 8 * ffm_ref.ORACLE_MAX_P_RATIO and ffm_ref.C_P < ffm_ref.C


@pytest.mark.parametrize("opt", [SGD, FLEX], ids=["sgd", "flex"])
@pytest.mark.parametrize("F,k", [(30, 10), (20, 12), (16, 32), (40, 16), (30, 8)], ids=lambda x: str(x))
def test_sgd_and_flex_stay_within_c(F, k, opt):
    """the other two optimizers on one shape of each family: the oracle passes the judge at C (SGD leaves every accumulator bit-identical)"""
    r = _oracle_run(F, k, opt)
    print(f"{F}x{k} opt {opt}: oracle max ratio {_worst(r):.3e}")
    assert _worst(r) <= ffm_ref.C and _worst_p(r) <= ffm_ref.C_P
    assert sum(v.skipped for v in r.verdicts) <= ffm_ref.MAX_SKIPPED_SHARE * r.st.n
    if opt == SGD:
        assert np.array_equal(r.before[1].view(np.uint32), r.after[1].view(np.uint32))
        assert np.array_equal(r.before[2][1::2].view(np.uint32), r.after[2][1::2].view(np.uint32))


def test_saturated_nan_and_unweighted_examples_follow_the_rules():
    """the +-50 and NaN rules and importance 0, against the oracle on crafted single examples (F = 2, k = 4)"""
    ocfg = fwo.make_config(optimizer=LUT, learning_rate=0.1, ffm_learning_rate=0.1, bit_precision=8, num_combos=2, ffm_k=4, ffm_bit_precision=8,
                           ffm_num_fields=2, init_acc_gradient=1.0, ffm_init_acc_gradient=1.0)
    cfg = ffm_ref.StepConfig.from_oracle_config(ocfg)
    lr = fwo.lr_entries([(3, 1.0, 0), (9, 2.0, 1)])
    ffm = fwo.ffm_entries([(16, 1.0, 0), (32, 0.5, 4)])
    for fill, lr_w, imp, want_g0 in ((0.2, 0.1, 1.0, False), (0.2, 60.0, 1.0, True), (0.2, -60.0, 1.0, True), (np.nan, 0.1, 1.0, True), (0.2, 0.1, 0.0, True)):
        om = fwo.Model(ocfg)
        om.ffm_fill(fill)
        om.lr_table[0::2] = lr_w
        before = (om.ffm_weights.copy(), om.ffm_acc.copy(), om.lr_table.copy())
        p = om.learn(lr, ffm, 1.0, imp, True)
        after = (om.ffm_weights.copy(), om.ffm_acc.copy(), om.lr_table.copy())
        om.close()
        v = ffm_ref.judge_example(cfg, before, after, lr, ffm, 1.0, imp, p)
        assert (v.ref.g == 0.0 or not v.ref.updated) == want_g0
        if not np.isnan(fill):
            assert v.worst <= ffm_ref.C, (fill, lr_w, imp, v.where)
            assert v.p_err <= v.p_bound, (fill, lr_w, imp, v.p_err, v.p_bound)
        else:
            assert p == 0.5 == v.ref.p
        if want_g0:  # no step: the weights are what they were, bit for bit
            assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)) and np.array_equal(before[2][0::2].view(np.uint32), after[2][0::2].view(np.uint32))


# ------------------------------------------------------------------ the judge itself: three planted faults
def _faulty(F, k, fault):
    """a probe set's oracle result with one fault planted in example `e`'s step (the tables a subtly wrong kernel would leave); returns
    (run, e, after_faulty).  From freshly initialised tables: the regime of the stream tests, whose bar the faults are shown to pass (on the
    warm state of the one-step matrix the same faults are ten to a thousand times the old bar: steps grow with the weights)."""
    r = _oracle_run(F, k, LUT, cold=True)
    st, cfg = r.st, r.cfg
    w1, a1, l1 = (t.copy() for t in r.after)
    w0, a0, _ = r.before
    R = F * k
    if fault == "slot":  # the gradient of ONE field slot of one row 1e-3 (relative) wrong: the step of those k floats with it
        e = next(e for e, v in enumerate(r.verdicts) if not v.skipped)
        fb = st.fbs[e]
        h = int(fb.ffm_buffer["hash"][0])
        z = next(z for z in range(F) if np.any(w1[h + z * k:h + (z + 1) * k] != w0[h + z * k:h + (z + 1) * k]))
        sl = slice(h + z * k, h + (z + 1) * k)
        w1[sl] = (w0[sl].astype(np.float64) + (w1[sl].astype(np.float64) - w0[sl]) * (1.0 + 1e-3)).astype(np.float32)
        return r, e, (w1, a1, l1)
    # a row that occurs twice in its example, both times with value 1
    for e, fb in enumerate(st.fbs):
        hs, vs = fb.ffm_buffer["hash"], fb.ffm_buffer["value"]
        dup = [i for i in range(1, len(hs)) if hs[i] == hs[i - 1] and vs[i] == vs[i - 1] == 1.0]
        if dup and not r.verdicts[e].skipped:
            break
    else:
        raise AssertionError("the probe set has no chained duplicate of unweighted features")
    i = dup[0]
    h = int(hs[i])
    f = int(fb.ffm_buffer["contra_field_index"][i]) // k
    v1, v2 = float(fb.ffm_buffer["value"][i - 1]), float(fb.ffm_buffer["value"][i])
    ref = r.verdicts[e].ref
    T = ffm_ref.forward(cfg, w0, r.before[2], fb.lr_buffer, fb.ffm_buffer)[2]
    idx = np.arange(h, h + R)
    if fault == "chain":  # the second occurrence's self-pair term taken from the weight the first occurrence has just stepped
        # grad2 = g v2 (T[f][f] - w v2): with w = w0 + dw1 the slot-f gradients shift by -g v2^2 dw1, the step by that times the rate
        sl = slice(h + f * k, h + (f + 1) * k)
        facing = T[f, f] - w0[sl].astype(np.float64) * v1
        a_mid = a0[sl].astype(np.float64) + (ref.g * v1 * facing) ** 2
        dw1 = -(ref.g * v1 * facing) * cfg.lut_ffm[ffm_ref._lut_key(a_mid.astype(np.float32))]
        rate2 = cfg.lut_ffm[ffm_ref._lut_key(a1[sl])]
        w1[sl] = (w1[sl].astype(np.float64) + ref.g * v2 * v2 * dw1 * rate2).astype(np.float32)
        assert np.any(w1[sl] != r.after[0][sl])
        return r, e, (w1, a1, l1)
    if fault == "g2":  # the accumulators of the row miss the second occurrence's g^2
        facing = T[:, f, :].copy()
        facing[f] -= w0[h + f * k:h + (f + 1) * k].astype(np.float64) * v2
        a1[idx] = (a1[idx].astype(np.float64) - (ref.g * v2 * facing.reshape(-1)) ** 2).astype(np.float32)
        assert np.any(a1[idx] != r.after[1][idx])
        return r, e, (w1, a1, l1)
    raise ValueError(fault)


@pytest.mark.parametrize("F,k", [(30, 8), (20, 12), (30, 10)], ids=lambda x: str(x))
@pytest.mark.parametrize("fault", ["slot", "chain", "g2"])
def test_planted_faults_fail_the_judge_and_pass_the_old_bar(fault, F, k):
    """the gap this judge closes: each fault leaves tables that the stream tests' bar accepts against the oracle's -- and the judge refuses"""
    r, e, after = _faulty(F, k, fault)
    fb = r.st.fbs[e]
    for got, ref in zip(after, r.after):
        assert ffm_ref.old_bar(got, ref)
    clean = r.verdicts[e]
    v = ffm_ref.judge_example(r.cfg, r.before, after, fb.lr_buffer, fb.ffm_buffer, fb.label, fb.example_importance, r.p[e])
    print(f"{fault} on {F}x{k}: clean ratio {clean.worst:.3e}, faulty {v.worst:.3e} (C = {ffm_ref.C:.3e}) at {v.where}")
    assert clean.worst <= ffm_ref.C
    assert v.worst > ffm_ref.C and v.where[0] == ("acc" if fault == "g2" else "w")


# ------------------------------------------------------------------ ... and two faults of the forward pass alone
@pytest.mark.parametrize("F,k", [(30, 8), (20, 12), (30, 10), (2, 128), (20, 64)], ids=lambda x: str(x))
@pytest.mark.parametrize("fault", ["pair_element", "self_pair"])
def test_planted_forward_faults_fail_the_prediction_bound(fault, F, k):
    """what a wrong read-only kernel would return: ONE of the k products of one field pair dropped from the logit; the self-pair correction of ONE feature
    left out.  On every probe the clean oracle prediction (either forward pass) is inside the bound and the faulty one outside."""
    r = _oracle_run(F, k, LUT)
    for e, fb in enumerate(r.st.fbs):
        ref = r.verdicts[e].ref
        _, _, T, _, rows = ffm_ref.forward(r.cfg, r.before[0], r.before[2], fb.lr_buffer, fb.ffm_buffer)
        fld = (fb.ffm_buffer["contra_field_index"] // k).astype(np.int64)
        if fault == "pair_element":
            f, z = sorted(np.unique(fld))[-1], sorted(np.unique(fld))[0]  # two fields that have features: T[f][z] . T[z][f], element 0
            assert f > z
            term = T[f, z, 0] * T[z, f, 0]
        else:
            v = float(fb.ffm_buffer["value"][0])
            term = -0.5 * v * v * float(np.sum(rows[0, fld[0]] ** 2))
        assert term != 0.0
        p_faulty = np.float32(ffm_ref.logistic(ref.logit - term))
        for p_clean in (r.p[e], r.p_predict[e]):
            err, bound, _ = ffm_ref.judge_prediction(p_clean, ref.p, ref.M_p)
            assert err <= bound
        err, bound, _ = ffm_ref.judge_prediction(p_faulty, ref.p, ref.M_p)
        assert err > bound, (e, err, bound, term)


# ------------------------------------------------------------------ the multi-rank routes' probe sets (tests/test_gpu_dist_step.py)
DIST_OPT_SHAPES = [(6, 4), (30, 10), (40, 16)]


def _same_bits(r, q):
    return np.array_equal(r.p.view(np.uint32), q.p.view(np.uint32)) and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(r.after, q.after))


@pytest.mark.parametrize("dist", ["dup", "nodup"])
@pytest.mark.parametrize("F,k", ffm_ref.DIST_MATRIX, ids=[f"{F}x{k}" for F, k in ffm_ref.DIST_MATRIX])
def test_oracle_on_the_multi_rank_probe_sets(F, k, dist):
    """What tests/test_gpu_dist_step.py rests on, on the oracle: over probes that share nothing, ONE synchronous micro-batch of all twenty leaves the
    bits that twenty sequential steps leave (tables and predictions) -- so every route, in order or concurrent, whoever owns a row, is held to one
    sequential step per example.  And the new sets are probe sets like MATRIX's: the oracle within the recorded maxima that C and C_P are 8 times,
    at most one probe in ten left out by the float64 reference, nothing outside the touched rows changed, the rows dealt over all four quarters."""
    r, q = _oracle_run(F, k, LUT, dist=dist), _oracle_run(F, k, LUT, dist=dist, minibatch=True)
    assert _same_bits(r, q), "the micro-batch mode and the sequential steps leave different bits on examples that share nothing"
    st = r.st
    print(f"{F}x{k} {dist}: oracle max ratio {_worst(r):.3e}, max p ratio {_worst_p(r):.3e}, skipped {sum(v.skipped for v in r.verdicts)} of {st.n}, 2^{st.ffm_bits} floats")
    assert _worst(r) <= ffm_ref.ORACLE_MAX_RATIO, [v.where for v in r.verdicts if v.worst == _worst(r)]
    assert _worst_p(r) <= ffm_ref.ORACLE_MAX_P_RATIO
    assert max(v.p_bound for v in r.verdicts) < ffm_ref.PRED_CAP
    assert sum(v.skipped for v in r.verdicts) <= ffm_ref.MAX_SKIPPED_SHARE * st.n
    touched = np.concatenate([v.ref.ffm_idx for v in r.verdicts])
    assert ffm_ref.untouched_identical(r.before[0], r.after[0], touched) and ffm_ref.untouched_identical(r.before[1], r.after[1], touched)
    lr_touched = np.concatenate([v.ref.lr_idx for v in r.verdicts])
    assert ffm_ref.untouched_identical(r.before[2], r.after[2], np.concatenate([2 * lr_touched, 2 * lr_touched + 1]))
    assert not np.array_equal(r.before[0], r.after[0]) and not np.array_equal(r.before[1], r.after[1])
    assert (st.row_count.max() == 2) == (dist == "dup") and np.any(st.val != 1.0)
    assert st.scatter == 4 and (1 << st.ffm_bits) <= 1 << 20
    assert np.all(np.abs([v.ref.logit for v in r.verdicts]) < 20.0)
    quarter = (1 << st.ffm_bits) // 4
    for j in range(4):  # every owner of a 4-rank job holds rows of at least three probes; every probe of four or more rows has rows at all of them
        assert sum(1 for fb in st.fbs if np.any(fb.ffm_buffer["hash"].astype(np.int64) // quarter == j)) >= 3
    for fb in st.fbs:
        if len(np.unique(fb.ffm_buffer["hash"])) >= 4:
            assert len(np.unique(fb.ffm_buffer["hash"].astype(np.int64) // quarter)) == 4


@pytest.mark.parametrize("dist", ["dup", "nodup"])
@pytest.mark.parametrize("opt", [SGD, FLEX], ids=["sgd", "flex"])
@pytest.mark.parametrize("F,k", DIST_OPT_SHAPES, ids=lambda x: str(x))
def test_sgd_and_flex_on_the_multi_rank_probe_sets(F, k, opt, dist):
    r, q = _oracle_run(F, k, opt, dist=dist), _oracle_run(F, k, opt, dist=dist, minibatch=True)
    assert _same_bits(r, q)
    assert _worst(r) <= ffm_ref.C and _worst_p(r) <= ffm_ref.C_P
    assert sum(v.skipped for v in r.verdicts) <= ffm_ref.MAX_SKIPPED_SHARE * r.st.n


# ------------------------------------------------------------------ the owner route in float32 numpy, and four faults planted in it
def _owner_route_f32(cfg, before, fb, g, fault=None, row=0):
    """One example through the owner-side apply as the device splits it, every product and sum in float32: the SOURCE forms the field sums T in buffer
    order and pushes one gradient row per occurrence, float e of a row of field f being g * (v * (T[e / k][f][e % k] - [e / k == f] * own[e - (e / k) * k] * v))
    (own: the occurrence's own field slot, staged next to T); the OWNER applies the pushed rows in push order on its tables: acc += grad^2, w -= step.
    g: the general gradient (from the float64 forward pass).  Returns (w, acc, lr) after the example.
    fault: "chunk2" -- floats 256 .. 511 of pushed row `row` arrive as zeros (a dropped second 16-byte chunk); "zshift" -- e / k taken as e >> 4 where k = 12;
    "twice" -- pushed row `row` applied a second time; "flex_acc" -- the owner does not store row `row`'s accumulators back."""
    f32 = np.float32
    w, a, l = (t.copy() for t in before)
    F, k = cfg.F, cfg.k
    R = F * k
    ent = fb.ffm_buffer
    n = len(ent)
    h, fld, v = ent["hash"].astype(np.int64), (ent["contra_field_index"] // k).astype(np.int64), ent["value"].astype(f32)
    rows = before[0][h[:, None] + np.arange(R)[None, :]].reshape(n, F, k)
    T = np.zeros((F, F, k), dtype=f32)
    for i in range(n):
        T[fld[i]] += rows[i] * v[i]
    own = np.concatenate([rows[np.arange(n), fld].reshape(-1), np.zeros(2 * R, dtype=f32)])  # own[i * k + kk]; what lies behind it in the model: zeros
    g = f32(g)
    e = np.arange(R)
    z = e >> 4 if fault == "zshift" else e // k
    lut_f, lut_l = cfg.lut_ffm.astype(f32), cfg.lut_lr.astype(f32)

    def apply(wt, at, idx, grad, rate, power_t, lut, keep_acc=False):
        acc = at[idx] + grad * grad if cfg.optimizer != SGD else at[idx]
        if cfg.optimizer == SGD:
            step = grad * f32(rate)
        elif cfg.optimizer == FLEX:
            step = grad * f32(rate) * np.power(acc, f32(-power_t), dtype=f32)
        else:
            step = grad * lut[ffm_ref._lut_key(acc)]
        wt[idx] = wt[idx] - step.astype(f32)
        if not keep_acc:
            at[idx] = acc

    for i in range(n):
        t = T[:, fld[i], :].reshape(-1).copy()  # t[e] = T[e / k][f][e % k]
        self_ = z == fld[i]
        t[self_] = t[self_] - own[i * k + (e - z * k)[self_]] * v[i]
        grad = (g * (v[i] * t)).astype(f32)
        if fault == "chunk2" and i == row:
            grad[256:512] = 0.0
        idx = h[i] + e
        for _ in range(2 if fault == "twice" and i == row else 1):
            apply(w, a, idx, grad, cfg.ffm_lr, cfg.ffm_power_t, lut_f, keep_acc=fault == "flex_acc" and i == row)
    lw, la = l[0::2].copy(), l[1::2].copy()
    for hh, vv in zip(fb.lr_buffer["hash"].astype(np.int64), fb.lr_buffer["value"].astype(f32)):
        apply(lw, la, np.array([hh]), np.array([g * vv], dtype=f32), cfg.lr, cfg.power_t, lut_l)
    l[0::2], l[1::2] = lw, la
    return w, a, l


OWNER_FAULTS = [("chunk2", 16, 32, LUT), ("chunk2", 5, 64, LUT), ("chunk2", 40, 16, LUT), ("zshift", 20, 12, LUT), ("twice", 30, 8, LUT), ("twice", 30, 3, LUT),
                ("flex_acc", 30, 10, FLEX), ("flex_acc", 40, 16, FLEX)]


@pytest.mark.parametrize("fault,F,k,opt", OWNER_FAULTS, ids=[f"{f}-{F}x{k}" for f, F, k, _ in OWNER_FAULTS])
def test_planted_owner_route_faults_fail_the_judge(fault, F, k, opt):
    """tests/test_gpu_dist_step.py's "what would turn which case red", as a tested statement: on every judged probe of the shape the clean float32
    model of the owner route passes the judge at C and each of the four faults fails it"""
    r = _oracle_run(F, k, opt, dist="dup")
    n_judged = 0
    for e, fb in enumerate(r.st.fbs):
        ref = r.verdicts[e].ref
        if r.verdicts[e].skipped:
            continue
        n_judged += 1
        clean = ffm_ref.judge_example(r.cfg, r.before, _owner_route_f32(r.cfg, r.before, fb, ref.g), fb.lr_buffer, fb.ffm_buffer, fb.label, fb.example_importance, r.p[e])
        assert clean.worst <= ffm_ref.C, (e, clean.worst, clean.where)
        v = ffm_ref.judge_example(r.cfg, r.before, _owner_route_f32(r.cfg, r.before, fb, ref.g, fault), fb.lr_buffer, fb.ffm_buffer, fb.label, fb.example_importance, r.p[e])
        assert v.worst > ffm_ref.C and v.where[0] == ("acc" if fault == "flex_acc" else "w"), (e, v.worst, v.where)
    assert n_judged >= 18


STREAM_REGIMES = {"lut-0.05": (LUT, 0.05), "sgd-0.01": (SGD, 0.01)}  # tests/test_gpu_dist.py: the in-order and sharded stream tests; the streaming form's


@pytest.mark.parametrize("fault,F,k,regime", [("chunk2", 5, 64, "lut-0.05"), ("chunk2", 16, 32, "lut-0.05"), ("chunk2", 40, 16, "sgd-0.01"), ("zshift", 20, 12, "sgd-0.01")],
                         ids=lambda x: str(x))
def test_planted_owner_route_faults_pass_the_stream_bar(fault, F, k, regime):
    """... and the bar the multi-rank stream tests hold these routes to -- |got - ref| <= 3e-5 + 1e-5 |ref| against the oracle's tables, in their regimes
    (freshly initialised tables; AdagradLUT at learning rates 0.05, SGD at 0.01) -- lets a dropped second chunk and a shifted z through: planted in one
    probe at a time, the faulty tables pass that bar against the oracle's for some probes at least (a first step from such tables moves most floats by
    less than 3e-5), while the judge refuses every one of them"""
    opt, rate = STREAM_REGIMES[regime]
    r = _oracle_run(F, k, opt, cold=True, dist="dup", lr=rate, ffm_lr=rate)
    accepted = judged = 0
    for e, fb in enumerate(r.st.fbs):
        if r.verdicts[e].skipped:
            continue
        judged += 1
        after = _owner_route_f32(r.cfg, r.before, fb, r.verdicts[e].ref.g, fault)
        v = ffm_ref.judge_example(r.cfg, r.before, after, fb.lr_buffer, fb.ffm_buffer, fb.label, fb.example_importance, r.p[e])
        assert v.worst > ffm_ref.C, (e, v.worst)
        # the whole tables as such a run would leave them: the oracle's, with this probe's floats from the faulty model
        got = [t.copy() for t in r.after]
        idx, lidx = v.ref.ffm_idx, v.ref.lr_idx
        got[0][idx], got[1][idx] = after[0][idx], after[1][idx]
        got[2][2 * lidx], got[2][2 * lidx + 1] = after[2][2 * lidx], after[2][2 * lidx + 1]
        accepted += all(ffm_ref.old_bar(x, y, weight_tol=3e-5) for x, y in zip(got, r.after))
    print(f"{fault} on {F}x{k}, {regime}: the stream bar accepts {accepted} of {judged} faulty probes, the judge none")
    assert accepted >= 1
