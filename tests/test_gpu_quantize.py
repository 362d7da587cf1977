"""The FFM weight quantiser on the device (csrc/quantize.hip) and what is built on it: fwgpu_quantize_ffm_table, fwgpu_model_save_inference,
fwgpu_pack_regressor (create and refresh).  Every result is defined bit for bit by host code the project already has -- the host quantiser
(fwgpu_quantize_ffm_weights), save + convert, fwgpu_model_load_packed -- so every comparison here is equality of bytes or bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import capi
from fwumious_wabbit_amd import persistence as P
from fwumious_wabbit_amd.feed import VwNamespaceMap
from fwumious_wabbit_amd.regressor import debug_quantize
from helpers import make_pair
import quantize_cases as Q

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIMIZERS = [fw.Optimizer.SGD, fw.Optimizer.AdagradFlex, fw.Optimizer.AdagradLUT]
OPT_IDS = ["SGD", "AdagradFlex", "AdagradLUT"]


def _vwmap(n):
    return VwNamespaceMap("".join(f"N{i:02d},ns{i}\n" for i in range(n)))


def _records(fields, n, first=0):
    if fields == 6:
        return fw.synth_records(6, 1.0, 1.1, 3000, 0.2, 31, first, n)
    return fw.synth_records(fields, 5.67, 1.05, 100000, 0.1, 21, first, n)


def _train(re, mi, recs, off):
    b = re.record_batch(fw.FeatureBufferTranslator(mi), recs, off)
    re.learn_batch(b, capi.MODE_SEQUENTIAL, True)
    b.close()


def _trained(opt=fw.Optimizer.AdagradLUT, fields=6, k=4, bits=18, n=600, nn=False):
    """tests/test_gpu_packed.py's _trained, on 18-bit tables"""
    mi, _, _ = make_pair(fields, k, bits, bits, opt, lr=0.05, ffm_lr=0.05)
    if nn:
        mi.nn_layers = [dict(width="9", activation="relu"), dict(width="5", activation="relu", init="xavier")]
    recs, off = _records(fields, n)
    re = fw.Regressor(mi)
    _train(re, mi, recs, off)
    return mi, re, recs, off


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _predictions(re, mi, recs, off):
    """600 predictions per (batch kind, mode), and the kernel family of every launch"""
    fbt = fw.FeatureBufferTranslator(mi)
    out, families = [], set()
    for records in (False, True):
        b = re.record_batch(fbt, recs, off) if records else re.batch_from_records(fbt, recs, off)
        for mode in (capi.MODE_HOGWILD, capi.MODE_SEQUENTIAL):
            re.learn_batch(b, mode, False)
            families.add(re.last_launch()["family"])
            out.append(b.predictions().copy())
        b.close()
    return np.stack(out), families


def _assert_same_packed(a, b, mi, recs, off):
    assert a.ffm_storage() == b.ffm_storage() and a.ffm_storage()[0] == capi.FFM_F16_BUCKETS
    assert np.array_equal(_bits(a.table_read(capi.TABLE_FFM_W)), _bits(b.table_read(capi.TABLE_FFM_W)))
    assert np.array_equal(_bits(a.table_read(capi.TABLE_LR)), _bits(b.table_read(capi.TABLE_LR)))
    assert a.table_checksum(capi.TABLE_FFM_W) == b.table_checksum(capi.TABLE_FFM_W)
    assert a.table_checksum(capi.TABLE_LR) == b.table_checksum(capi.TABLE_LR)
    pa, fa = _predictions(a, mi, recs, off)
    pb, fb = _predictions(b, mi, recs, off)
    assert fa == fb == {capi.KERNEL_PACKED}
    assert np.array_equal(pa, pb)
    assert 0.005 < pa.std()  # (a model that says something)
    return pa


# ------------------------------------------------------------------ 1. the kernels against the host quantiser
@pytest.mark.parametrize("n", Q.LENGTHS + (Q.WRAP_LENGTH,))
def test_kernels_give_the_host_quantisers_bytes(n):
    tables = [("normal", Q.normal_table(n), None)] + Q.crafted(n)
    for name, table, check in tables:
        want = P.quantize_ffm_weights(table)
        if check is not None and n >= Q.MIN_CHECKED_LEN:
            inc, mn, q = Q.split(want, n)
            check(q, inc, mn)  # the table does what it was crafted for, by the host quantiser alone
        got, on_device = debug_quantize(table)
        # (a table of one weight is a constant table: the contract's host route)
        assert on_device == Q.takes_device_route(want, table), (n, name)
        if n > 1:
            assert on_device, (n, name)
        if got != want:
            g, w = Q.split(got, n)[2], Q.split(want, n)[2]
            bad = np.nonzero(g != w)[0]
            raise AssertionError(f"n = {n}, {name}: header {got[:8].hex()} vs {want[:8].hex()}, {bad.size} buckets differ, first at {bad[:8]}: "
                                 f"{g[bad[:8]]} vs {w[bad[:8]]} for weights {table[bad[:8]]}")


# ------------------------------------------------------------------ 2. the host route where the contract says so
def test_tables_the_contract_sends_to_the_host_return_the_hosts_bytes():
    for name, table in Q.host_route_tables():
        got, on_device = debug_quantize(table)
        assert not on_device, name
        assert got == P.quantize_ffm_weights(table), name


# ------------------------------------------------------------------ 3. a live regressor's table
@pytest.mark.parametrize("opt", OPTIMIZERS, ids=OPT_IDS)
def test_quantize_ffm_table_of_a_trained_regressor(opt):
    mi, re, recs, off = _trained(opt)
    tables = (capi.TABLE_LR, capi.TABLE_FFM_W, capi.TABLE_FFM_ACC)
    before = [re.table_checksum(t) for t in tables]
    w = re.table_read(capi.TABLE_FFM_W)
    assert 0 < np.abs(w).max() and np.isfinite(w).all()
    got = re.quantize_ffm_table()
    assert got == P.quantize_ffm_weights(w)
    assert [re.table_checksum(t) for t in tables] == before
    _train(re, mi, *_records(6, 50, first=600))  # the source still trains
    assert re.table_checksum(capi.TABLE_FFM_W) != before[1]
    re.close()


def test_quantize_ffm_table_refusals(tmp_path):
    mi, re, _, _ = _trained(n=50)
    rp = re.pack()
    with pytest.raises(capi.FwgpuError) as e:
        rp.quantize_ffm_table()
    assert e.value.code == capi.ERR_INVALID and "packed" in e.value.message
    mi0, _, _ = make_pair(6, 0, 12, 12, fw.Optimizer.AdagradLUT)
    r0 = fw.Regressor(mi0)
    out = np.zeros(64, dtype=np.uint8)
    assert capi.lib().fwgpu_quantize_ffm_table(r0.h, capi.ptr(out), out.size, None) == capi.ERR_INVALID
    for x in (re, rp, r0):
        x.close()


# ------------------------------------------------------------------ 4. files, byte for byte
@pytest.mark.parametrize("opt,nn", [(fw.Optimizer.SGD, False), (fw.Optimizer.AdagradFlex, False), (fw.Optimizer.AdagradLUT, False),
                                    (fw.Optimizer.AdagradFlex, True)], ids=OPT_IDS + ["two-layer-head"])
def test_save_inference_writes_the_file_of_save_and_convert(tmp_path, opt, nn):
    vw = _vwmap(6)
    mi, re, _, _ = _trained(opt, nn=nn, n=300)
    before = re.table_checksum(capi.TABLE_FFM_W), re.table_checksum(capi.TABLE_LR)
    t = str(tmp_path / "t.fw")
    P.save_regressor_to_filename(t, mi, vw, re)
    for quantize in (False, True):
        c, d = str(tmp_path / f"convert{int(quantize)}.fw"), str(tmp_path / f"direct{int(quantize)}.fw")
        P.convert_inference_regressor(t, c, quantize_weights=quantize)
        P.save_inference_regressor(d, mi, vw, re, quantize_weights=quantize)
        want, got = open(c, "rb").read(), open(d, "rb").read()
        assert len(got) == len(want)
        assert got == want, f"quantize = {quantize}: first difference at byte {next(i for i in range(len(want)) if got[i] != want[i])}"
    assert (re.table_checksum(capi.TABLE_FFM_W), re.table_checksum(capi.TABLE_LR)) == before
    _train(re, mi, *_records(6, 50, first=300))
    re.close()


_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
from fwumious_wabbit_amd import persistence as P
mi, vw, re = P.new_regressor_from_filename(sys.argv[2], immutable=True)
P.save_regressor_to_filename(sys.argv[3], mi, vw, re, quantize_weights=True)
re.close()
"""


def test_model_save_quantized_equals_the_host_route_of_a_fresh_process(tmp_path):
    vw = _vwmap(6)
    mi, re, _, _ = _trained(n=300)
    t, u = str(tmp_path / "t.fw"), str(tmp_path / "u.fw")
    P.save_regressor_to_filename(t, mi, vw, re)
    re.close()
    P.convert_inference_regressor(t, u)
    mi_f, vw_f, rf = P.new_regressor_from_filename(u, immutable=True)
    here, child = str(tmp_path / "device.fw"), str(tmp_path / "host.fw")
    P.save_regressor_to_filename(here, mi_f, vw_f, rf, quantize_weights=True)
    rf.close()
    env = dict(os.environ, FWGPU_QUANTIZE_HOST="1")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, u, child], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert open(here, "rb").read() == open(child, "rb").read()
    # ... which is the file the host-only conversion writes
    q = str(tmp_path / "q.fw")
    P.convert_inference_regressor(t, q, quantize_weights=True)
    assert open(here, "rb").read() == open(q, "rb").read()


# ------------------------------------------------------------------ 5. pack
@pytest.mark.parametrize("fields,k", [(6, 4), (30, 8), (30, 16)], ids=["6x4", "30x8", "30x16"])
def test_pack_equals_the_packed_load_of_the_saved_file(tmp_path, fields, k):
    mi, re, recs, off = _trained(fields=fields, k=k)
    before = [re.table_checksum(t) for t in (capi.TABLE_LR, capi.TABLE_FFM_W, capi.TABLE_FFM_ACC)]
    t = str(tmp_path / "t.fw")
    P.save_regressor_to_filename(t, mi, _vwmap(fields), re)
    mi_p, _, rf = P.new_regressor_from_filename(t, immutable=True, packed=True)
    rp = re.pack()
    assert rp.mi == mi_p
    _assert_same_packed(rp, rf, mi_p, recs, off)
    assert [re.table_checksum(t) for t in (capi.TABLE_LR, capi.TABLE_FFM_W, capi.TABLE_FFM_ACC)] == before
    _train(re, mi, *_records(fields, 50, first=600))
    for x in (re, rp, rf):
        x.close()


# ------------------------------------------------------------------ 6. refresh
def test_refresh_in_place_equals_a_fresh_pack():
    mi, re, recs, off = _trained()
    rp = re.pack()
    p0, _ = _predictions(rp, rp.mi, recs, off)
    _train(re, mi, *_records(6, 300, first=600))
    assert re.pack(into=rp) is rp
    fresh = re.pack()
    p1 = _assert_same_packed(rp, fresh, rp.mi, recs, off)
    assert not np.array_equal(p0, p1)  # (the 300 examples moved the model)
    for x in (re, rp, fresh):
        x.close()


def test_refresh_and_pack_refusals_leave_the_target_as_it_was():
    mi, re, recs, off = _trained()
    rp = re.pack()
    p0, _ = _predictions(rp, rp.mi, recs, off)
    _train(re, mi, *_records(6, 100, first=600))  # (a refresh that went through would change rp)

    def refused(source, target, word):
        with pytest.raises(capi.FwgpuError) as e:
            source.pack(into=target)
        assert e.value.code == capi.ERR_INVALID and word in e.value.message, e.value.message

    # targets: a packed regressor of other geometry, and an f32 regressor
    mi_s, rs, recs_s, off_s = _trained(bits=12, n=100)
    rsp = rs.pack()
    ps, _ = _predictions(rsp, rsp.mi, recs_s, off_s)
    refused(re, rsp, "geometry")
    assert np.array_equal(_predictions(rsp, rsp.mi, recs_s, off_s)[0], ps)
    mi_f = fw.ModelInstance(**{**mi.__dict__, "optimizer": fw.Optimizer.SGD})
    rf = fw.Regressor(mi_f)
    pf, _ = _predictions(rf, mi_f, recs, off)
    refused(re, rf, "packed regressor")
    assert np.array_equal(_predictions(rf, mi_f, recs, off)[0], pf)
    # sources: a deep head, ffm_k = 10, a packed regressor -- with and without a target
    _, rh, _, _ = _trained(opt=fw.Optimizer.AdagradFlex, nn=True, n=50)
    _, r10, _, _ = _trained(k=10, n=50)
    for source, word in ((rh, "deep head"), (r10, "multiple of 4"), (rsp, "packed")):
        refused(source, rp, word)
        refused(source, None, word)
        assert np.array_equal(_predictions(rp, rp.mi, recs, off)[0], p0), word
    # ... and the refresh that IS allowed still goes through afterwards
    re.pack(into=rp)
    assert not np.array_equal(_predictions(rp, rp.mi, recs, off)[0], p0)
    for x in (re, rp, rs, rsp, rf, rh, r10):
        x.close()
