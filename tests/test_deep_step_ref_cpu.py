"""tests/deep_ref.py against the oracle, where no GPU is needed: on every case of deep_ref.CASES the oracle's own step of one example through the deep head
(fwo.Model(..., nn=...).learn from the written state) passes the float64 judge within the recorded maxima that C_DENSE, C_SPARSE and C_P are derived from, no
case loses more than one probe in ten, and the judge turns red on five planted errors -- for each it is printed whether the stream tests' bar
(2e-5 + 1e-5 |ref| against the oracle's tables) would have let it through."""
import numpy as np
import pytest

import deep_ref
from deep_ref import CASES, TABLE_NAMES
from ffm_ref import SGD, old_bar
from oracle import fwo

_RUNS = {}


class _Run:
    pass


def _oracle_run(name):
    """the oracle's step on every probe of the case, each from the written state: tables before / after, prediction and verdict per probe (computed once per
    case, shared and left unchanged)"""
    if name in _RUNS:
        return _RUNS[name]
    cs = deep_ref.build_case(name)
    om = fwo.Model(cs.ocfg, nn=cs.nn)
    r = _Run()
    r.cs, r.before, r.after, r.p, r.verdicts = cs, [], [], [], []
    for e, fb in enumerate(cs.fbs):
        deep_ref.write_oracle(om, cs, e)
        r.before.append(deep_ref.read_oracle(om, cs))
        r.p.append(np.float32(om.learn(fb.lr_buffer, fb.ffm_buffer, fb.label, fb.example_importance, True)))
        r.after.append(deep_ref.read_oracle(om, cs))
        r.verdicts.append(deep_ref.judge_example(cs.cfg, r.before[e], r.after[e], fb.lr_buffer, fb.ffm_buffer, fb.label, fb.example_importance, r.p[e]))
    om.close()
    _RUNS[name] = r
    return r


def _worst(r):
    return max(v.dense for v in r.verdicts), max(v.sparse for v in r.verdicts), max(v.p_ratio for v in r.verdicts)


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_stays_within_the_recorded_maxima(name):
    """the oracle needs no more than the recorded maxima (C / 8) on any float or prediction; every float outside the stepped rows, units and entries is
    bit-identical -- the rows, biases and accumulators of the units with a zero output gradient among them; no probe is rejected for a ReLU unit at its
    margin or left out for a small |p - y| beyond one in ten; the probe set has what the cases promise (a chained duplicate, a weighted feature, a field without
    a feature, dead and live ReLU units)"""
    r = _oracle_run(name)
    cs, n = r.cs, len(r.verdicts)
    dense, sparse, p = _worst(r)
    print(f"DEEPREF {name}: oracle max ratios dense {dense:.3e} sparse {sparse:.3e} p {p:.3e}; rejected {sum(v.rejected for v in r.verdicts)}, "
          f"skipped {sum(v.skipped for v in r.verdicts)} of {n}")
    assert dense <= deep_ref.ORACLE_MAX_DENSE_RATIO, [v.where_dense for v in r.verdicts if v.dense == dense]
    assert sparse <= deep_ref.ORACLE_MAX_SPARSE_RATIO, [v.where_sparse for v in r.verdicts if v.sparse == sparse]
    assert p <= deep_ref.ORACLE_MAX_P_RATIO
    assert all(v.untouched is None for v in r.verdicts), [v.untouched for v in r.verdicts]
    assert all(v.p_err <= v.p_bound for v in r.verdicts)
    assert sum(v.rejected for v in r.verdicts) <= deep_ref.MAX_REJECTED * n
    assert sum(v.skipped for v in r.verdicts) <= deep_ref.MAX_SKIPPED_SHARE * n
    st = cs.st
    assert st.row_count.max() == 2 and np.any(st.val != 1.0)
    assert any(len(np.unique(fb.ffm_buffer["contra_field_index"])) < cs.cfg.F for fb in cs.fbs)
    assert all(abs(v.ref.z) <= deep_ref.Z_MAX * 1.001 and v.ref.g != 0.0 for v in r.verdicts)
    for e, v in enumerate(r.verdicts):
        assert not np.array_equal(r.before[e][3], r.after[e][3]), "the head did not learn"
        if cs.c["opt"] == SGD:
            for t in (2, 4):
                assert np.array_equal(r.before[e][t].view(np.uint32), r.after[e][t].view(np.uint32))
    assert any(not np.array_equal(r.before[e][1], r.after[e][1]) for e in range(n)) and any(not np.array_equal(r.before[e][0], r.after[e][0]) for e in range(n))
    relu = [l for l, (_, act) in enumerate(cs.cfg.layers) if act == "relu"]
    assert any(np.any(v.ref.og[l] == 0.0) for v in r.verdicts for l in relu) and all(np.any(v.ref.og[l] != 0.0) for v in r.verdicts for l in relu)


def test_a_zero_gradient_leaves_the_weight_alone_where_the_accumulator_is_zero():
    """nn_init_acc_gradient = 0 (case a_init0): the accumulators left at 0 belong to weights whose input is exactly 0; the reference gives them d = 0 and M = 0, so
    the judge holds them to their two half ulps -- and the oracle leaves them bit-identical"""
    r = _oracle_run("a_init0")
    seen = 0
    for e, v in enumerate(r.verdicts):
        ref = v.ref
        zero = ref.nn_idx[(r.before[e][4][ref.nn_idx] == 0.0)]
        seen += len(zero)
        assert np.all(ref.nn_M[np.isin(ref.nn_idx, zero)] == 0.0)
        for t in (3, 4):
            assert np.array_equal(r.before[e][t][zero].view(np.uint32), r.after[e][t][zero].view(np.uint32))
    assert seen > 0


def test_the_recorded_maxima_are_reached():
    """the recorded maxima are the measurements, not round numbers above them: the cases named next to them reach them (to the three digits they are recorded with)"""
    for i, (mx, case, c) in enumerate(((deep_ref.ORACLE_MAX_DENSE_RATIO, deep_ref.ORACLE_MAX_DENSE_RATIO_CASE, deep_ref.C_DENSE),
                                       (deep_ref.ORACLE_MAX_SPARSE_RATIO, deep_ref.ORACLE_MAX_SPARSE_RATIO_CASE, deep_ref.C_SPARSE),
                                       (deep_ref.ORACLE_MAX_P_RATIO, deep_ref.ORACLE_MAX_P_RATIO_CASE, deep_ref.C_P))):
        assert case in CASES
        assert _worst(_oracle_run(case))[i] >= 0.99 * mx
        assert c == 8 * mx


# ------------------------------------------------------------------ the judge itself: five planted errors
PLANTS = ("dx_from_the_post_update_weight", "a_bias_step_dropped", "a_dead_units_accumulator_touched", "row_gradient_from_the_neighbouring_slot", "lr_entry_stepped_with_g")


def _faulty(name, plant):
    """(run, e, tables a subtly wrong kernel would leave after probe e): the oracle's result with one error planted"""
    r = _oracle_run(name)
    cs, cfg = r.cs, r.cs.cfg
    e = next(e for e, v in enumerate(r.verdicts) if not (v.rejected or v.skipped))
    fb, before = cs.fbs[e], r.before[e]
    after = [t.copy() for t in r.after[e]]
    ref = r.verdicts[e].ref
    if plant in ("dx_from_the_post_update_weight", "row_gradient_from_the_neighbouring_slot", "lr_entry_stepped_with_g"):
        kind = {"dx_from_the_post_update_weight": "post_update_dx", "row_gradient_from_the_neighbouring_slot": "tri_neighbour", "lr_entry_stepped_with_g": "lr_takes_g"}[plant]
        bad = deep_ref.step(cfg, before, fb.lr_buffer, fb.ffm_buffer, fb.label, fb.example_importance, after=r.after[e], plant=kind)
        for t, idx, d_bad, d_ref in ((0, 2 * ref.lr_idx, bad.lr_dw, ref.lr_dw), (0, 2 * ref.lr_idx + 1, bad.lr_dacc, ref.lr_dacc),
                                     (1, ref.ffm_idx, bad.ffm_dw, ref.ffm_dw), (2, ref.ffm_idx, bad.ffm_dacc, ref.ffm_dacc)):
            after[t][idx] = (after[t][idx].astype(np.float64) + (d_bad - d_ref)).astype(np.float32)
    elif plant == "a_bias_step_dropped":
        o, out, w_in = cfg.lay[0]
        j = int(np.flatnonzero(ref.og[0] != 0.0)[0])
        for t in (3, 4):
            after[t][o + out * w_in + j] = before[t][o + out * w_in + j]
    elif plant == "a_dead_units_accumulator_touched":
        l = next(l for l in range(len(cfg.layers)) if np.any(ref.og[l] == 0.0))
        o, out, w_in = cfg.lay[l]
        j = int(np.flatnonzero(ref.og[l] == 0.0)[0])
        after[4][o + j * w_in] = np.nextafter(after[4][o + j * w_in], np.float32(np.inf))  # (g^2 of a gradient that should have been exactly 0)
    else:
        raise ValueError(plant)
    return r, e, tuple(after)


@pytest.mark.parametrize("name", ["a", "g"])
@pytest.mark.parametrize("plant", PLANTS)
def test_planted_errors_fail_the_judge(plant, name):
    """each error leaves tables the judge refuses, while the oracle's own pass it; whether |faulty - oracle| <= 2e-5 + 1e-5 |oracle| holds on all five tables (the
    stream tests' bar) is printed"""
    r, e, after = _faulty(name, plant)
    cs, fb = r.cs, r.cs.fbs[e]
    assert deep_ref.passes(r.verdicts[e])
    assert any(not np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(after, r.after[e])), "nothing was planted"
    v = deep_ref.judge_example(cs.cfg, r.before[e], after, fb.lr_buffer, fb.ffm_buffer, fb.label, fb.example_importance, r.p[e])
    old = {t: old_bar(a, b) for t, a, b in zip(TABLE_NAMES, after, r.after[e])}
    print(f"DEEPPLANT {plant} on {name}: dense needs {v.dense:.3e} (C {deep_ref.C_DENSE:.3e}) at {v.where_dense}; sparse needs {v.sparse:.3e} (C {deep_ref.C_SPARSE:.3e}) at "
          f"{v.where_sparse}; untouched: {v.untouched}; the old bar {'PASSES it' if all(old.values()) else 'fails it on ' + ', '.join(t for t, ok in old.items() if not ok)}")
    assert not deep_ref.passes(v)
    if plant == "a_dead_units_accumulator_touched":
        assert v.untouched == "NN_ACC"
    elif plant == "a_bias_step_dropped":
        assert v.dense > deep_ref.C_DENSE and "bias" in v.where_dense
    else:
        assert v.sparse > deep_ref.C_SPARSE
