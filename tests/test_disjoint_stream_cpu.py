"""The generator behind tests/test_gpu_concurrent_exact.py, checked where no GPU is needed: the disjointness condition on the host translator's
output, and the oracle fact the frozen-head cases rest on."""
import numpy as np
import pytest

import fwumious_wabbit_amd as fw
from helpers import check_disjoint, disjoint_models, disjoint_stream
from oracle import fwo


@pytest.mark.parametrize("kw", [
    dict(F=30, k=8, n=24, per_field=(6, 9), p_weighted=0.2, p_dup=0.04),
    dict(F=10, k=4, n=64, first_ffm=33),
    dict(F=10, k=4, n=64, lr_only_ns=1, first_lr=65),
    dict(F=30, k=16, n=16, per_field=(1, 3), p_weighted=0.2, p_dup=0.1),
    dict(F=40, k=8, n=16, per_field=(1, 3), p_dup=0.1),
    dict(F=3, k=10, n=64, per_field=(1, 3), p_dup=0.1),
    dict(F=8, k=0, n=64, per_field=(1, 2), p_weighted=0.2, p_dup=0.1),
], ids=lambda kw: f"F{kw['F']}k{kw['k']}")
def test_disjoint_stream_is_disjoint(kw):
    st = disjoint_stream(seed=5, **kw)
    mi, _, _ = disjoint_models(st, fw.Optimizer.AdagradLUT)
    fbs = check_disjoint(st, mi)
    assert len(fbs) == st.n and (1 << st.ffm_bits) >= st.span
    if "first_ffm" in kw:
        assert max(len(f.ffm_buffer) for f in fbs) == kw["first_ffm"] == len(fbs[0].ffm_buffer)
    if "first_lr" in kw:
        assert max(len(f.lr_buffer) for f in fbs) == kw["first_lr"] == len(fbs[0].lr_buffer)
    if kw["k"] == 8:  # all four 32-byte start phases of a line occur
        assert set(np.unique(st.row_hash * 4 % 128)) == {0, 32, 64, 96}
    if kw.get("p_dup"):
        assert st.row_count.max() == 2


def test_check_disjoint_refuses_a_shared_row():
    st = disjoint_stream(F=6, k=4, n=8, seed=6)
    mi, _, _ = disjoint_models(st, fw.Optimizer.AdagradLUT)
    # example 1's first feature becomes example 0's: the bookkeeping follows, so only the disjointness asserts can object
    st.recs[int(st.off[1]) + 3] = st.recs[3]
    st.hash[6] = st.hash[0]
    with pytest.raises(AssertionError, match="128-byte line|LR entry"):
        check_disjoint(st, mi)


@pytest.mark.parametrize("opt", [fwo.OPT_ADAGRAD_LUT, fwo.OPT_ADAGRAD_FLEX])
def test_zero_nn_learning_rate_freezes_the_dense_weights_on_the_oracle(opt):
    st = disjoint_stream(F=6, k=4, n=200, per_field=(1, 2), p_weighted=0.2, p_dup=0.1, seed=7)
    _, ocfg, ots = disjoint_models(st, opt)
    layers = [(12, "relu", "hu"), (8, "relu", "hu")]
    om = fwo.Model(ocfg, nn=fwo.make_nn_config(layers, "one", 0.0, 0.45, 0.0))
    w0 = [om.nn_weights(l).copy() for l in range(3)]
    f0 = om.ffm_weights.copy()
    _, p = om.run_stream(ots, st.recs, st.off, holdout_after=0, nthreads=1)
    assert np.all(np.isfinite(p)) and not np.array_equal(f0, om.ffm_weights)
    for l in range(3):
        assert np.array_equal(w0[l].view(np.uint32), om.nn_weights(l).view(np.uint32))
    om.close()
