"""ONE learning step of one example through the per-example deep head of csrc/kernels.hip, judged per float against float64 (tests/deep_ref.py).

The stream tests hold the head's training path (nn_forward / nn_backward / nn_layer_backward / nn_layer_backward_vec, a phase of fw_example_kernel<..., NN = true>
and of fw_example_kernel_r<..., NN = true>) to |gpu - ref| <= 2e-5 + 1e-5 |ref| on the final tables of a whole stream; the concurrent test freezes the dense weights.
Here every probe of a case gets its own one-example MODE_SEQUENTIAL launch from a state the test wrote (all five tables rewritten in between: the sparse warm
state, dense weights from head_ref.dense_head_weights, NN_ACC log-uniform over 48 LUT buckets with a quarter left at the initial value), and every float the
example steps -- LR, FFM_W, FFM_ACC, NN_W, NN_ACC -- is held to

    |after - (before + d_ref)| <= C * M + ulp(before) / 2 + ulp(after) / 2        (deep_ref: C_DENSE / C_SPARSE measured on the oracle, M the propagated magnitude)

with d_ref from the DEVICE's own before-state, every other float bit-identical (the rows, biases and accumulators of units with a zero output gradient among them),
the prediction within C_P * 0.25 * t_z + 4 ulp, the two feeding routes bit-equal, and the kernel family, chunk count and workgroup size the case claims asserted
from the launch's resolved parameters.  What would turn a case red: the input gradient formed from a post-update weight (3e-4 .. 8e-4 against C_SPARSE = 6e-6), a bias
step dropped, a dead unit's accumulator touched, the row gradient of a field slot taken from the neighbouring triangle slot, the LR entries stepped with g instead of
dx[combo] (all planted in tests/test_deep_step_ref_cpu.py); an active neuron lost by the compaction past 64 or by the split over the thread groups (that unit's
row keeps its old value: needs c = inf); a tail slot of nn_layer_backward / nn_layer_backward_vec stepping a neighbour (a float outside the stepped set changes)."""
import numpy as np
import pytest

import deep_ref
import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import _capi as capi

pytestmark = pytest.mark.gpu

SCALAR, VEC4, RESIDENT = capi.KERNEL_SCALAR, capi.KERNEL_VEC4, capi.KERNEL_RESIDENT
TABLES = (capi.TABLE_LR, capi.TABLE_FFM_W, capi.TABLE_FFM_ACC, capi.TABLE_NN_W, capi.TABLE_NN_ACC)  # deep_ref.TABLE_NAMES' order
NN_V2 = dict(whole=3, head=2)  # in-order launches forced onto the head as a phase of the two-chunk large-table kernel (nn_v2)

# id -> (case of deep_ref.CASES, launch options, family, chunks, threads)
CONFIGS = {
    "a": ("a", {}, VEC4, 1, 512),
    "a_init0": ("a_init0", {}, VEC4, 1, 512),
    "b": ("b", {}, VEC4, 1, 512),
    "b64": ("b64", {}, VEC4, 1, 512),
    "c": ("c", {}, VEC4, 1, 512),
    "d": ("d", {}, VEC4, 1, 512),
    "e": ("e", {}, VEC4, 1, 512),
    "f_5x16": ("f_5x16", {}, VEC4, 1, 512),
    "f_3x5": ("f_3x5", {}, SCALAR, 1, 512),
    "g": ("g", {}, VEC4, 2, 512),
    "g_1024": ("g", dict(threads=1024), VEC4, 2, 1024),
    "g_nn_v2": ("g", NN_V2, RESIDENT, 2, 512),
    "a_sgd": ("a_sgd", {}, VEC4, 1, 512),
    "a_flex": ("a_flex", {}, VEC4, 1, 512),
    "g_sgd": ("g_sgd", {}, VEC4, 2, 512),
    "g_sgd_nn_v2": ("g_sgd", NN_V2, RESIDENT, 2, 512),
    "g_flex": ("g_flex", {}, VEC4, 2, 512),
    "g_flex_nn_v2": ("g_flex", NN_V2, RESIDENT, 2, 512),
}


def _regressor(cs, threads=None, whole=None, head=None, policy=None):
    re = fw.Regressor(cs.mi)
    if threads is not None:
        re.set_launch(threads=threads)
    if whole is not None:
        re.set_whole_line_updates(whole)
    if head is not None:
        re.set_head_kernel(head)
    if policy is not None:
        re.set_store_policy(policy)
    assert re.table_len(capi.TABLE_LR) == len(cs.lr) and re.table_len(capi.TABLE_FFM_W) >= len(cs.ffm_w)
    assert re.table_len(capi.TABLE_NN_W) == cs.cfg.total == re.table_len(capi.TABLE_NN_ACC)
    return re


def _write(re, cs, e):
    """the case's written state, with probe e's NN_ACC"""
    for t, values in zip(TABLES, (cs.lr, cs.ffm_w, cs.ffm_acc, cs.nn_w, cs.nn_acc[e])):
        re.table_write(t, values)


def _read(re):
    return tuple(re.table_read(t) for t in TABLES)


def _launch(re, cs, picks, route, mode):
    """one launch over the probes `picks` = [(probe, importance or None: the probe's own)]; returns the predictions"""
    st = cs.st
    if route == "records":
        recs, off = [], [0]
        for e, imp in picks:
            rec = st.recs[int(st.off[e]):int(st.off[e + 1])].copy()
            if imp is not None:
                rec[2] = np.float32(imp).view(np.uint32)
            recs.append(rec)
            off.append(off[-1] + len(rec))
        b = re.record_batch(fw.FeatureBufferTranslator(cs.mi), np.concatenate(recs), np.array(off, dtype=np.uint64))
    else:
        fbs = []
        for i, (e, imp) in enumerate(picks):
            fb = cs.fbs[e]
            fbs.append(fw.FeatureBuffer(fb.label, fb.example_importance if imp is None else imp, i, fb.lr_buffer, fb.ffm_buffer))
        b = re.batch(fbs)
    try:
        re.learn_batch(b, mode, True)
        return b.predictions().copy()
    finally:
        b.close()


def _same_bits(xs, ys):
    return all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(xs, ys))


def _judge(tag, cs, e, before, after, p):
    """(dense ratio, sparse ratio, p ratio) of probe e's step; raises with the failing float's coordinates"""
    fb = cs.fbs[e]
    v = deep_ref.judge_example(cs.cfg, before, after, fb.lr_buffer, fb.ffm_buffer, fb.label, fb.example_importance, p)
    assert not v.rejected and not v.skipped, f"{tag} probe {e}: left out by the reference (rejected {v.rejected}, skipped {v.skipped}): the CPU test asserts that none is"
    assert v.p_err <= v.p_bound, (f"{tag} probe {e}: prediction {float(p)!r}, float64 {v.ref.p!r}: |d| = {v.p_err:.3e}, bound {v.p_bound:.3e} "
                                  f"(needs c_p = {v.p_ratio:.3e}, C_P = {deep_ref.C_P:.3e})")
    assert v.untouched is None, f"{tag} probe {e}: {v.untouched}: a float outside the stepped rows, units and entries changed"
    assert v.dense <= deep_ref.C_DENSE, f"{tag} probe {e}: {v.where_dense}: needs c = {v.dense:.3e}, C_DENSE = {deep_ref.C_DENSE:.3e}"
    assert v.sparse <= deep_ref.C_SPARSE, f"{tag} probe {e}: {v.where_sparse}: needs c = {v.sparse:.3e}, C_SPARSE = {deep_ref.C_SPARSE:.3e}"
    assert not np.array_equal(before[3], after[3]), "the head did not learn"
    return v.dense, v.sparse, v.p_ratio


def _report(tag, info, worst):
    d, s, p = (max(w[i] for w in worst) for i in range(3))
    print(f"HEADSTEP {tag}: family {info['family']} chunks {info['chunks']} threads {info['threads']}: dense needs c = {d:.3e} = {d / deep_ref.C_DENSE:.3f} C_DENSE, "
          f"sparse c = {s:.3e} = {s / deep_ref.C_SPARSE:.3f} C_SPARSE, prediction c_p = {p:.3e} = {p / deep_ref.C_P:.3f} C_P")


@pytest.mark.parametrize("cid", list(CONFIGS))
def test_one_step_per_probe(cid):
    """every probe alone, in order, both routes from the same written state"""
    name, setup, family, chunks, threads = CONFIGS[cid]
    cs = deep_ref.build_case(name)
    re = _regressor(cs, **setup)
    worst = []
    try:
        for e in range(len(cs.fbs)):
            runs = []
            for route in ("entries", "records"):
                _write(re, cs, e)
                before = _read(re) if route == "entries" else None
                p = _launch(re, cs, [(e, None)], route, capi.MODE_SEQUENTIAL)
                info = re.last_launch()
                assert (info["family"], info["chunks"], info["threads"]) == (family, chunks, threads), info
                assert 0 < info["lds_bytes"] <= 160 * 1024, info
                runs.append((before, _read(re), p))
            assert np.isfinite(runs[0][2][0])
            assert _same_bits([runs[0][2]], [runs[1][2]]), "the two routes' predictions differ"
            assert _same_bits(runs[0][1], runs[1][1]), "the two routes leave different tables"
            worst.append(_judge(cid, cs, e, runs[0][0], runs[0][1], runs[0][2][0]))
    finally:
        re.close()
    _report(cid, info, worst)


def test_the_cases_cover_both_backward_forms_and_the_edges_they_claim():
    """nn_layer_backward_any's gate restated (deep_ref.vec_form): the 16-byte form and the scalar form each run on a first layer, a hidden layer and the final
    neuron; and, from the reference's own output gradients on the written state: b64's hidden layer has more active units than its G = 32 thread groups with a
    remainder, c's first layer an active unit past the compaction's first 64, every case a dead and a live ReLU unit."""
    seen = {"first": set(), "hidden": set(), "final": set()}
    for name, setup, _, _, threads in CONFIGS.values():
        cfg = deep_ref.build_case(name).cfg
        forms = deep_ref.vec_form(cfg, threads)
        for l, form in enumerate(forms):
            seen["first" if l == 0 else "final" if l == len(forms) - 1 else "hidden"].add(form)
    assert all(s == {True, False} for s in seen.values()), seen
    expect = {"a": [False, True, False], "b": [True, True, True], "b64": [True, True, True], "c": [True, False, False], "d": [False, True], "g": [True, True, True]}
    for name, want in expect.items():
        assert deep_ref.vec_form(deep_ref.build_case(name).cfg, 512) == want, name

    def live(name, l):
        cs = deep_ref.build_case(name)
        return [np.flatnonzero(deep_ref.step(cs.cfg, (cs.lr, cs.ffm_w, cs.ffm_acc, cs.nn_w, cs.nn_acc[e]), fb.lr_buffer, fb.ffm_buffer, fb.label,
                                             fb.example_importance).og[l] != 0.0) for e, fb in enumerate(cs.fbs)]

    G = 512 // (64 // 4)
    assert G == 32 and any(len(j) > G and len(j) % G for j in live("b64", 1))
    assert any(j.max() >= 64 and len(j) < 65 for j in live("c", 0))
    d = deep_ref.build_case("d").cfg
    assert d.lay[0][1] == 516 > 512 and d.lay[1][2] == 552 and d.lay[1][0] % 4 == 0


# ------------------------------------------------------------------ the concurrent kernels, deterministically
HOGWILD = {
    "a": ("a", {}, VEC4, 1, 512),
    "b": ("b", {}, VEC4, 1, 512),
    "g": ("g", dict(whole=3), RESIDENT, 2, 512),  # nn_v2, the concurrent default where the large-table update path runs
}


@pytest.mark.parametrize("cid", list(HOGWILD))
def test_one_updating_example_in_a_concurrent_launch(cid):
    """One MODE_HOGWILD launch of 256 examples of which exactly ONE has an importance other than 0; the others are only predicted (do_update_now).  The grid has
    more than one workgroup, so the concurrent-only code runs -- the 16-byte forward (vec16), the no_selfw diagonal and nn_v2 by default on g, the hot LR entry's
    atomics on the constant feature -- and the tables afterwards are still one example's step, judged at the same bar.  set_store_policy(1): weight rows written
    back through the L2, NO accumulator store thinned (policy 3, the default, would thin them on hot rows).  The other examples' predictions only need to be finite."""
    name, setup, family, chunks, threads = HOGWILD[cid]
    cs = deep_ref.build_case(name)
    n, at, e = 256, 137, 1
    picks = [((i % len(cs.fbs)), 0.0) for i in range(n)]
    picks[at] = (e, None)
    re = _regressor(cs, policy=1, **setup)
    runs = []
    try:
        for route in ("entries", "records"):
            _write(re, cs, e)
            before = _read(re)
            p = _launch(re, cs, picks, route, capi.MODE_HOGWILD)
            info = re.last_launch()
            assert (info["family"], info["chunks"], info["threads"]) == (family, chunks, threads), info
            runs.append((before, _read(re), p))
    finally:
        re.close()
    for before, after, p in runs:
        assert np.all(np.isfinite(p))
        _report(f"hogwild {cid}", info, [_judge(f"hogwild {cid}", cs, e, before, after, p[at])])
    assert _same_bits(runs[0][1], runs[1][1]), "the two routes leave different tables"


# ------------------------------------------------------------------ chaining
@pytest.mark.parametrize("cid", ["a", "g", "g_nn_v2"])
def test_three_examples_in_order_equal_three_launches(cid):
    """an in-order launch of 3 examples leaves bit-identical tables and predictions to three one-example launches of the same kernel from the same state (the
    dense weights, the constant's LR entry and -- in a -- the interaction's entries are shared by the examples: each must see the one before it)"""
    name, setup, family, chunks, threads = CONFIGS[cid]
    cs = deep_ref.build_case(name)
    re = _regressor(cs, **setup)
    try:
        _write(re, cs, 0)
        p3 = _launch(re, cs, [(0, None), (1, None), (2, None)], "records", capi.MODE_SEQUENTIAL)
        info = re.last_launch()
        assert (info["family"], info["chunks"], info["threads"]) == (family, chunks, threads), info
        t3 = _read(re)
        _write(re, cs, 0)
        p1 = np.concatenate([_launch(re, cs, [(e, None)], "records", capi.MODE_SEQUENTIAL) for e in range(3)])
        t1 = _read(re)
    finally:
        re.close()
    assert _same_bits([p3], [p1]), (p3, p1)
    for name_, a, b in zip(deep_ref.TABLE_NAMES, t3, t1):
        assert _same_bits([a], [b]), f"{name_}: {int(np.sum(a.view(np.uint32) != b.view(np.uint32)))} floats differ"
