"""ONE in-order learning step per kernel shape, judged per float against float64 (tests/ffm_ref.py).

The stream tests judge final tables by |gpu - ref| <= 2e-5 + 1e-5 |ref| -- above the whole change of most weights over such a stream, so a gradient a
few per cent off in one field slot, a chained duplicate stepped on the post-update weight or a dropped g^2 pass them (tests/test_ffm_ref_cpu.py plants
the three and asserts it).  Here every example of a batch starts from a state the test wrote (helpers.disjoint_stream: the examples share no row, no
line, no LR entry), so one MODE_SEQUENTIAL launch steps 20 probes and every float they touch is held to

    |after - (before + d_ref)| <= C * M + ulp(before) / 2 + ulp(after) / 2          (ffm_ref.judge_floats; C measured on the oracle, ffm_ref.C)

with d_ref from the DEVICE's own before-state, every float outside the touched rows bit-identical, the two feeding routes (entries translated on the
host, raw records translated in the kernel) bit-equal, and the kernel family and chunk count the case claims asserted from the launch's resolved
parameters (Regressor.last_launch) -- a later dispatch change cannot silently move a case onto another kernel.

What would turn which case red: a field slot's gradient off by 1e-3 relative (any case: ~14 x the bound on that slot's floats); the odd last chunk of
the scalar kernel's chunk groups skipped (scalar 30x10: floats 256.. of every row keep their old value); e0 / k by a shift where k is no power of
two (resident 20x12 ...: every float of a row takes another slot's gradient); a second chunk addressed from float 256 of T instead of its field
(16x32, 4x128); the generic kernel's chunk loop one short (20x64: floats 1024.. untouched)."""
import numpy as np
import pytest

import ffm_ref
import fwumious_wabbit_amd as fw
from ffm_ref import FLEX, LUT, SGD
from fwumious_wabbit_amd import _capi as capi
from helpers import check_disjoint, disjoint_models

pytestmark = pytest.mark.gpu

SCALAR, VEC4, RESIDENT = capi.KERNEL_SCALAR, capi.KERNEL_VEC4, capi.KERNEL_RESIDENT
TABLES = (capi.TABLE_FFM_W, capi.TABLE_FFM_ACC, capi.TABLE_LR)

_PROBES = {}


def _probe(F, k):
    """the shape's probe set (ffm_ref.probe_stream: the one test_ffm_ref_cpu.py calibrates C on), generated and checked once, left unchanged"""
    if (F, k) not in _PROBES:
        st = ffm_ref.probe_stream(F, k)
        mi, _, _ = disjoint_models(st, LUT)
        check_disjoint(st, mi)
        _PROBES[(F, k)] = st
    return _PROBES[(F, k)]


def _shifted(fbs, shift):
    """the entry route's buffers with every FFM row `shift` floats further on: rows off the 16-byte boundary, as raw entry batches may hold them
    (rows are at least 64 floats apart: still disjoint)"""
    out = []
    for fb in fbs:
        ffm = fb.ffm_buffer.copy()
        ffm["hash"] += shift
        out.append(fw.FeatureBuffer(fb.label, fb.example_importance, fb.example_number, fb.lr_buffer.copy(), ffm))
    return out


def _setup(re, whole=None, kept=None, lds_keep=None, kernel_version=None):
    if whole is not None:
        re.set_whole_line_updates(whole)
    if kept is not None:
        re.set_kept_rows(kept)
    if lds_keep is not None:
        re.set_lds_keep(lds_keep)
    if kernel_version is not None:
        capi.check(re.L.fwgpu_debug_set_kernel_version(re.h, kernel_version))


def _warm_regressor(mi, st, **setup):
    re = fw.Regressor(mi)
    _setup(re, **setup)
    w, acc, lr = ffm_ref.warm_state(st)
    re.table_write(capi.TABLE_FFM_W, w)
    re.table_write(capi.TABLE_FFM_ACC, acc)
    re.table_write(capi.TABLE_LR, lr)
    return re


def _launch(re, mi, st, fbs, route, mode, update):
    b = re.record_batch(fw.FeatureBufferTranslator(mi), st.recs, st.off) if route == "records" else re.batch(fbs)
    try:
        re.learn_batch(b, mode, update)
        return b.predictions().copy()
    finally:
        b.close()


def _one_step(F, k, opt=LUT, shift=0, family=None, chunks=None, window=None, **setup):
    """the case: both routes from the same written state, bit-equal; the launch is what the case claims; every probe judged.  Returns
    (tables after, predictions, largest needed c / C)."""
    st = _probe(F, k)
    mi, ocfg, _ = disjoint_models(st, opt, **ffm_ref.opt_kwargs(opt))
    cfg = ffm_ref.StepConfig.from_oracle_config(ocfg)
    fbs = _shifted(st.fbs, shift) if shift else st.fbs
    runs = []
    for route in (("entries",) if shift else ("entries", "records")):
        re = _warm_regressor(mi, st, **setup)
        try:
            before = [re.table_read(t) for t in TABLES]
            p = _launch(re, mi, st, fbs, route, capi.MODE_SEQUENTIAL, True)
            info = re.last_launch()
            after = [re.table_read(t) for t in TABLES]
        finally:
            re.close()
        assert np.all(np.isfinite(p))
        assert (info["family"], info["chunks"]) == (family, chunks), info
        if window is not None:
            assert info["window"] == window and info["chain"] == (1 if window or family != RESIDENT else 0), info
        assert info["threads"] == 512 and 0 < info["lds_bytes"] <= 160 * 1024, info
        if "kept" in setup:
            assert info["no_kept_rows"] == (0 if setup["kept"] else 1), info
        if "lds_keep" in setup or not info["window"]:  # rows parked in LDS: the chained single-chunk update only, as many as asked for
            assert info["lds_keep"] == (setup.get("lds_keep", 0) if info["window"] and info["chunks"] == 1 and family == RESIDENT else 0), info
        runs.append((before, after, p))
    for other in runs[1:]:
        assert np.array_equal(runs[0][2].view(np.uint32), other[2].view(np.uint32)), "the two routes' predictions differ"
        for a, b in zip(runs[0][1], other[1]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "the two routes leave different tables"
    before, after, p = runs[0]
    worst, where, skipped, worst_p = 0.0, None, 0, 0.0
    touched, lr_touched = [], []
    for e, fb in enumerate(fbs):
        v = ffm_ref.judge_example(cfg, before, after, fb.lr_buffer, fb.ffm_buffer, fb.label, fb.example_importance, p[e])
        assert v.p_err <= v.p_bound, f"example {e}: prediction {p[e]!r}, float64 {v.ref.p!r}: |d| = {v.p_err:.3e}, bound {v.p_bound:.3e} (needs c_p = {v.p_ratio:.3e}, C_P = {ffm_ref.C_P:.3e})"
        worst_p = max(worst_p, v.p_ratio)
        skipped += v.skipped
        touched.append(v.ref.ffm_idx), lr_touched.append(v.ref.lr_idx)
        if v.worst > worst:
            worst, where = v.worst, (e,) + v.where
    print(f"FFMSTEP {F}x{k} opt={opt} shift={shift} {setup} family={family} chunks={chunks}: needs c = {worst:.3e} = {worst / ffm_ref.C:.3f} C at {where}, c_p = {worst_p:.3e} = {worst_p / ffm_ref.C_P:.3f} C_P, {skipped} probes skipped")
    if where is not None and worst > ffm_ref.C:
        e, name, idx = where
        row = int(np.searchsorted(st.row_hash + shift, idx, side="right")) - 1
        raise AssertionError(f"example {e}, table {name}, float {idx}: row {row} (starts at {int(st.row_hash[row]) + shift}, {int(st.row_count[row])} occurrence(s)), float "
                             f"{idx - int(st.row_hash[row]) - shift} of the row = field slot {(idx - int(st.row_hash[row]) - shift) // max(k, 1)}: needs c = {worst:.3e}, C = {ffm_ref.C:.3e}")
    assert skipped <= ffm_ref.MAX_SKIPPED_SHARE * st.n
    touched, lr_touched = np.concatenate(touched), np.concatenate(lr_touched)
    assert ffm_ref.untouched_identical(before[0], after[0], touched), "FFM_W: a float outside every row changed"
    assert ffm_ref.untouched_identical(before[1], after[1], touched if opt != SGD else np.zeros(0, dtype=np.int64)), "FFM_ACC: a float outside every row changed"
    assert ffm_ref.untouched_identical(before[2], after[2], np.concatenate([2 * lr_touched, 2 * lr_touched + 1] if opt != SGD else [2 * lr_touched])), "LR: an untouched float changed"
    assert not np.array_equal(before[0], after[0]), "the launch stepped nothing"
    return after, p, worst / ffm_ref.C


def _id(c):
    return "-".join(f"{k}{v}" for k, v in c.items())


# ------------------------------------------------------------------ the scalar kernel (one float per lane; update_rows' chunk groups of two)
SCALAR_CASES = [dict(F=30, k=10, chunks=5), dict(F=65, k=2, chunks=3), dict(F=30, k=3, chunks=2), dict(F=65, k=1, chunks=2)]


@pytest.mark.parametrize("c", SCALAR_CASES, ids=_id)
def test_scalar_kernel(c):
    """rows of more than one 64-float chunk: 300 floats = 5 chunks (two groups and an odd tail), 130 = 3, 90 and 65 = 2 with a nearly empty last one"""
    _one_step(c["F"], c["k"], family=SCALAR, chunks=c["chunks"])


@pytest.mark.parametrize("shift", [1, 2, 3])
@pytest.mark.parametrize("F,k,chunks", [(6, 4, 1), (30, 8, 4)])
def test_scalar_kernel_chosen_for_unaligned_rows(F, k, chunks, shift):
    """k % 4 == 0 but the entry batch's rows start 1, 2, 3 floats off a 16-byte boundary (raw entries, not the translator's): aligned4 = 0"""
    _one_step(F, k, shift=shift, family=SCALAR, chunks=chunks)


# ------------------------------------------------------------------ the register-resident kernel where k is no power of two
@pytest.mark.parametrize("F,k", [(20, 12), (21, 12), (12, 20), (10, 24)])
def test_resident_kernel_k_not_a_power_of_two(F, k):
    """k_log2 = 0xff: e0 / k a real division, the window path denied; 21 x 12 = 252 floats leaves the last lane of a row partly filled"""
    _one_step(F, k, family=RESIDENT, chunks=1, window=0)


def test_window_request_is_denied_where_k_is_not_a_power_of_two():
    """20 x 12 with whole-line updates asked for: the same kernel runs (window 0) and leaves the same bits"""
    a0, p0, _ = _one_step(20, 12, family=RESIDENT, chunks=1, window=0)
    a2, p2, _ = _one_step(20, 12, family=RESIDENT, chunks=1, window=0, whole=2)
    assert np.array_equal(p0.view(np.uint32), p2.view(np.uint32))
    for x, y in zip(a0, a2):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


# ------------------------------------------------------------------ ... and large k
@pytest.mark.parametrize("whole", [None, 2])
@pytest.mark.parametrize("F,k,chunks", [(8, 32, 1), (2, 128, 1), (16, 32, 2), (4, 128, 2), (5, 64, 2)])
def test_resident_kernel_large_k(F, k, chunks, whole):
    """a full single chunk (256 floats), a full second chunk (512) and a nearly empty one (320); float-granular and whole-line chained updates"""
    _one_step(F, k, family=RESIDENT, chunks=chunks, window=1 if whole else 0, whole=whole)


# ------------------------------------------------------------------ the generic 16-byte kernel without a deep head
@pytest.mark.parametrize("F,k,chunks", [(30, 12, 2), (21, 24, 2), (40, 16, 3), (25, 32, 4), (20, 64, 5)])
def test_generic_vec4_kernel(F, k, chunks):
    """rows the resident kernel does not take: 256 % k != 0 beyond 256 floats (360, 504), and 3, 4, 5 chunks of 256 (640, 800, 1280 floats)"""
    _one_step(F, k, family=VEC4, chunks=chunks, window=0)


@pytest.mark.parametrize("F,k", [(30, 8), (10, 4)])
def test_generic_vec4_kernel_forced(F, k):
    _one_step(F, k, family=VEC4, chunks=1, window=0, kernel_version=1)


# ------------------------------------------------------------------ shapes the stream tests run, now at this bar
def test_config_b_shape():
    _one_step(10, 4, family=RESIDENT, chunks=1, window=0)


@pytest.mark.parametrize("c", [dict(), dict(whole=0), dict(whole=2), dict(whole=3), dict(whole=3, kept=0), dict(whole=3, lds_keep=0), dict(whole=3, lds_keep=3),
                               dict(whole=2, lds_keep=3)], ids=_id)
def test_config_c_shape(c):
    """30 x 8: float-granular, whole-line and chained updates, no kept rows, rows parked in LDS"""
    window = 1 if c.get("whole", 0) >= 2 else 0
    _one_step(30, 8, family=RESIDENT, chunks=1, window=window, **c)


@pytest.mark.parametrize("whole", [None, 2])
@pytest.mark.parametrize("F,k", [(30, 16), (40, 8)])
def test_two_chunk_shapes(F, k, whole):
    _one_step(F, k, family=RESIDENT, chunks=2, window=1 if whole else 0, whole=whole)


# ------------------------------------------------------------------ SGD and AdagradFlex, one shape of each family
@pytest.mark.parametrize("opt", [SGD, FLEX], ids=["sgd", "flex"])
@pytest.mark.parametrize("c", [dict(F=30, k=10, family=SCALAR, chunks=5), dict(F=30, k=8, shift=2, family=SCALAR, chunks=4), dict(F=20, k=12, family=RESIDENT, chunks=1),
                               dict(F=16, k=32, family=RESIDENT, chunks=2, whole=2), dict(F=40, k=16, family=VEC4, chunks=3), dict(F=30, k=8, family=RESIDENT, chunks=1, whole=3)],
                         ids=_id)
def test_sgd_and_flex(c, opt):
    c = dict(c)
    _one_step(c.pop("F"), c.pop("k"), opt=opt, **c)


# ------------------------------------------------------------------ predict-only launches
@pytest.mark.parametrize("F,k", ffm_ref.MATRIX, ids=[f"{F}x{k}" for F, k in ffm_ref.MATRIX])
def test_predict_only_launch(F, k):
    """the same warm state through a concurrent predict-only launch (both routes; 6 x 4 and 30 x 8 also with rows 2 floats off the boundary): every
    prediction within min(C_P * M_p + 4 ulp, 5e-5) of the float64 forward pass (ffm_ref.judge_prediction: C_P measured on the oracle's two forward
    passes; one dropped pair element or self-pair term is 30 to 3000 times that), the tables' checksums unchanged"""
    st = _probe(F, k)
    mi, ocfg, _ = disjoint_models(st, LUT)
    cfg = ffm_ref.StepConfig.from_oracle_config(ocfg)
    re = _warm_regressor(mi, st)
    try:
        w, lr = re.table_read(capi.TABLE_FFM_W), re.table_read(capi.TABLE_LR)
        sums = [re.table_checksum(t) for t in TABLES]
        for route, shift in (("entries", 0), ("records", 0)) + ((("entries", 2),) if (F, k) in ((6, 4), (30, 8)) else ()):
            fbs = _shifted(st.fbs, shift) if shift else st.fbs
            p = _launch(re, mi, st, fbs, route, capi.MODE_HOGWILD, False)
            worst_p = 0.0
            assert re.last_launch()["family"] == (SCALAR if k % 4 or shift else RESIDENT if (F * k <= 256 or (F * k <= 512 and 256 % k == 0)) else VEC4)
            for e, fb in enumerate(fbs):
                want, M_p = ffm_ref.predict(cfg, w, lr, fb.lr_buffer, fb.ffm_buffer)
                err, bound, need = ffm_ref.judge_prediction(p[e], want, M_p)
                worst_p = max(worst_p, need)
                assert err <= bound, (route, shift, e, float(p[e]), want, err, bound, need, ffm_ref.C_P)
            print(f"FFMPREDICT {F}x{k} {route} shift={shift}: needs c_p = {worst_p:.3e} = {worst_p / ffm_ref.C_P:.3f} C_P")
            assert [re.table_checksum(t) for t in TABLES] == sums
    finally:
        re.close()



# ------------------------------------------------------------------ the reference's limit
def test_refusal_at_the_references_limit():
    """36 x 32: k * F^2 = 41472 floats of field sums, the largest model the reference accepts (block_ffm.rs:96-101) -- 162 KiB, more than the 160 KiB of LDS
    whatever the batch holds.  The regressor is created; every launch (updating and predict-only, both routes) comes back with FWGPU_ERR_RANGE before
    anything ran: no launch is recorded and the three tables are bit-identical.  (No batch of any size fits this shape, so what "the library serves
    a small batch correctly afterwards" can mean is checked in the same process on a shape that fits: 10 x 4 at the full one-step bar.)"""
    from helpers import disjoint_stream

    F, k = 36, 32
    st = disjoint_stream(F, k, 6, per_field=(0, 2), p_weighted=0.3, p_dup=0.15, seed=77)
    mi, _, _ = disjoint_models(st, LUT)
    check_disjoint(st, mi)
    assert k * F * F == 41472
    re = _warm_regressor(mi, st)
    try:
        before = [re.table_read(t) for t in TABLES]
        for route in ("entries", "records"):
            for mode, update in ((capi.MODE_SEQUENTIAL, True), (capi.MODE_HOGWILD, True), (capi.MODE_HOGWILD, False)):
                with pytest.raises(capi.FwgpuError) as ei:
                    _launch(re, mi, st, st.fbs, route, mode, update)
                assert ei.value.code == capi.ERR_RANGE, (route, mode, update, ei.value)
                assert re.last_launch()["family"] == -1
        for t, b in zip(TABLES, before):
            assert np.array_equal(re.table_read(t).view(np.uint32), b.view(np.uint32))
    finally:
        re.close()
    _one_step(10, 4, family=RESIDENT, chunks=1, window=0)


# ------------------------------------------------------------------ streams on the shapes no stream ran: collisions, overlapping rows, record prefetch, kept rows
# (the bars of helpers._stream_parity; one step does not cover what examples do to each other)
STREAMS = {
    "scalar_30x10": (SCALAR, dict(n_ns=30, k=10, bits=14, ffm_bits=14, optimizer=LUT, n=150, mean_extra=1.0, p_weighted=0.1, ids=3000, seed=81)),
    "scalar_65x2": (SCALAR, dict(n_ns=65, k=2, bits=13, ffm_bits=13, optimizer=LUT, n=150, mean_extra=1.0, p_weighted=0.1, ids=3000, seed=82)),
    "scalar_30x6_flex": (SCALAR, dict(n_ns=30, k=6, bits=14, ffm_bits=14, optimizer=FLEX, n=150, mean_extra=1.0, p_weighted=0.2, ids=3000, seed=83, init_acc=1.0, weight_tol=5e-5)),
    "resident_20x12": (RESIDENT, dict(n_ns=20, k=12, bits=14, ffm_bits=14, optimizer=LUT, n=200, mean_extra=1.0, p_weighted=0.1, ids=3000, seed=84)),
    "resident_21x12_flex": (RESIDENT, dict(n_ns=21, k=12, bits=14, ffm_bits=14, optimizer=FLEX, n=200, mean_extra=1.0, p_weighted=0.2, ids=3000, seed=85, init_acc=1.0, weight_tol=5e-5)),
    "vec4_30x12": (VEC4, dict(n_ns=30, k=12, bits=14, ffm_bits=14, optimizer=LUT, n=150, mean_extra=1.0, p_weighted=0.1, ids=3000, seed=86)),
    "vec4_21x24_flex": (VEC4, dict(n_ns=21, k=24, bits=14, ffm_bits=14, optimizer=FLEX, n=150, mean_extra=1.0, p_weighted=0.2, ids=3000, seed=87, init_acc=1.0, weight_tol=5e-5)),
    "vec4_40x16": (VEC4, dict(n_ns=40, k=16, bits=15, ffm_bits=15, optimizer=LUT, n=100, mean_extra=1.0, p_weighted=0.1, ids=3000, seed=88)),
    "vec4_20x64": (VEC4, dict(n_ns=20, k=64, bits=15, ffm_bits=15, optimizer=LUT, n=100, mean_extra=1.0, p_weighted=0.1, ids=3000, seed=89)),
    "resident_16x32": (RESIDENT, dict(n_ns=16, k=32, bits=14, ffm_bits=14, optimizer=LUT, n=100, mean_extra=1.0, p_weighted=0.1, ids=3000, seed=90)),
    "resident_5x64_flex": (RESIDENT, dict(n_ns=5, k=64, bits=14, ffm_bits=14, optimizer=FLEX, n=100, mean_extra=1.0, p_weighted=0.2, ids=3000, seed=91, init_acc=1.0, weight_tol=5e-5)),
    "resident_8x32_sgd": (RESIDENT, dict(n_ns=8, k=32, bits=14, ffm_bits=14, optimizer=SGD, n=100, mean_extra=1.0, p_weighted=0.2, ids=3000, seed=92, lr=0.05, ffm_lr=0.05)),
}


@pytest.mark.parametrize("name", list(STREAMS))
def test_stream_on_a_shape_no_stream_ran(name):
    from helpers import _stream_parity

    family, kw = STREAMS[name]
    launches = []
    kw = dict(kw)
    _stream_parity(kw.pop("n_ns"), kw.pop("k"), kw.pop("bits"), kw.pop("ffm_bits"), kw.pop("optimizer"), launches=launches, **kw)
    assert [i["family"] for i in launches] == [family, family], launches  # the entries' and the records' launch
