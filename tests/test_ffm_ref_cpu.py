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


def _oracle_run(F, k, opt, cold=False):
    """the oracle's own step on every probe of the shape, from the warm state (cold: from freshly initialised tables, the regime of the stream tests):
    tables before / after, predictions and the verdict per probe (computed once per shape and optimizer, shared and left unchanged)"""
    if (F, k, opt, cold) in _RUNS:
        return _RUNS[(F, k, opt, cold)]
    st = ffm_ref.probe_stream(F, k)
    mi, ocfg, _ = disjoint_models(st, opt, **ffm_ref.opt_kwargs(opt))
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
    r.p = np.array([om.learn(fb.lr_buffer, fb.ffm_buffer, fb.label, fb.example_importance, True) for fb in st.fbs], dtype=np.float32)
    r.after = (om.ffm_weights.copy(), om.ffm_acc.copy(), om.lr_table.copy())
    om.close()
    r.verdicts = [ffm_ref.judge_example(r.cfg, r.before, r.after, fb.lr_buffer, fb.ffm_buffer, fb.label, fb.example_importance, r.p[e])
                  for e, fb in enumerate(st.fbs)]
    r.predict_verdicts = [ffm_ref.judge_prediction(r.p_predict[e], v.ref.p, v.ref.M_p) for e, v in enumerate(r.verdicts)]
    _RUNS[(F, k, opt, cold)] = r
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
    assert (F, k) in MATRIX
    assert _worst(_oracle_run(F, k, LUT)) >= ffm_ref.ORACLE_MAX_RATIO * 0.99
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
