"""The generator behind tests/test_gpu_concurrent_exact.py, checked where no GPU is needed: the disjointness condition on the host translator's
output, and the oracle fact the frozen-head cases rest on."""
import numpy as np
import pytest

import ffm_ref
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


# zlib.crc32 of (recs, off) of ffm_ref.probe_stream as the generator laid it out before it learned to scatter
DEFAULT_LAYOUT_CRC = {(30, 8): (0x6f936384, 0x9b6686f8), (6, 4): (0xee1ec32f, 0x76f27982)}


@pytest.mark.parametrize("F,k", list(DEFAULT_LAYOUT_CRC), ids=lambda x: str(x))
def test_default_layout_is_unchanged(F, k):
    """scatter = 1 (the default): the records every one-step test has run on since, bit for bit"""
    import zlib

    st = ffm_ref.probe_stream(F, k)
    assert st.scatter == 1 and st.recs.dtype == np.uint32 and st.off.dtype == np.uint64
    assert (zlib.crc32(st.recs.tobytes()), zlib.crc32(st.off.tobytes())) == DEFAULT_LAYOUT_CRC[(F, k)]
    assert st.span == len(st.row_hash) * st.S


@pytest.mark.parametrize("dup", [True, False], ids=["dup", "nodup"])
@pytest.mark.parametrize("F,k", ffm_ref.DIST_MATRIX, ids=lambda x: str(x))
def test_scattered_stream_is_disjoint_and_draws_the_unscattered_features(F, k, dup):
    """scatter = 4 on every shape of the multi-rank matrix: no row crosses a quarter of the table, rows of different examples share no line, no
    LR hash occurs twice, every quarter holds rows, and values, labels, importances and duplicate counts are those of the unscattered stream of
    the same seed"""
    st = ffm_ref.dist_probe_stream(F, k, dup)
    mi, _, _ = disjoint_models(st, fw.Optimizer.AdagradLUT)
    fbs = check_disjoint(st, mi)
    assert st.scatter == 4 and st.span == 1 << st.ffm_bits and st.ffm_bits <= 20
    quarter = (1 << st.ffm_bits) // 4
    R = F * k
    lines = []
    for e, fb in enumerate(fbs):
        h = np.unique(fb.ffm_buffer["hash"].astype(np.int64))
        assert np.all(h // quarter == (h + R - 1) // quarter), e                          # no row crosses a quarter ...
        assert np.all((h * 4 // 128 * 128) // (4 * quarter) == (((h + R) * 4 + 127) // 128 * 128 - 1) // (4 * quarter)), e  # ... nor do its lines
        lines += [(int(lo), int(hi), e) for lo, hi in zip(h * 4 // 128, ((h + R) * 4 - 1) // 128)]
        if len(h) >= 4:
            assert len(np.unique(h // quarter)) == 4, e                                  # consecutive rows lie in consecutive quarters
    lines.sort()
    for (lo0, hi0, e0), (lo1, hi1, e1) in zip(lines[:-1], lines[1:]):
        assert lo1 > hi0, (e0, e1)
    assert {h // quarter for h in st.row_hash[st.row_ffm]} == {0, 1, 2, 3}
    allh = np.concatenate([np.unique(fb.lr_buffer["hash"]) for fb in fbs])
    assert len(np.unique(allh)) == len(allh)
    plain = disjoint_stream(F, k, st.n, per_field=(0, 2) if F >= 8 else (1, 2), p_weighted=0.3, p_dup=0.15 if dup else 0.0,
                            seed=(2000 if dup else 3000) + 7 * F + k + ffm_ref.DIST_SEED_BUMP.get((F, k, dup), 0))
    assert plain.scatter == 1
    for a in ("val", "labels", "row_count", "row_ex", "fld", "ex", "off"):
        assert np.array_equal(getattr(st, a), getattr(plain, a)), a
    assert [fb.example_importance for fb in fbs] == [fb.example_importance for fb in check_disjoint(plain, disjoint_models(plain, fw.Optimizer.AdagradLUT)[0])]
    assert (st.row_count.max() == 2) == dup
    if k % 4 == 0:  # the start phases of a line stay as in the unscattered layout
        assert np.array_equal(st.row_hash % 32, plain.row_hash % 32)


def test_check_disjoint_refuses_a_shared_row_of_a_scattered_stream():
    st = disjoint_stream(F=6, k=4, n=8, seed=6, scatter=4)
    mi, _, _ = disjoint_models(st, fw.Optimizer.AdagradLUT)
    st.recs[int(st.off[1]) + 3] = st.recs[3]
    st.hash[6] = st.hash[0]
    with pytest.raises(AssertionError, match="128-byte line|LR entry"):
        check_disjoint(st, mi)


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
