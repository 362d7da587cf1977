"""Device metrics without a device: the C ABI's new symbols and argument checks, the float64 yardstick (tests/metrics_ref.py) on a case worked by
hand, and binned_auc on a hand-made histogram.  (fwgpu_trainer_set_metrics after digesting needs a trainer, and a trainer needs a regressor on a
device: that refusal is checked in tests/test_gpu_metrics.py.)"""
import ctypes as C
import math

import numpy as np

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import _capi as capi

import metrics_ref as mr


def test_symbols_and_struct_layouts():
    L = C.CDLL(capi.LIB_PATH)
    for name in ("fwgpu_batch_metrics", "fwgpu_trainer_set_metrics", "fwgpu_trainer_metrics", "fwgpu_debug_metrics"):
        assert hasattr(L, name), name
    assert capi.lib().fwgpu_abi_version() == 1
    assert capi.METRIC_SUMS.itemsize == 64 and capi.METRIC_WINDOW.itemsize == 8 + 2 * 64 and capi.METRIC_TOTAL.itemsize == 64 + 512 * 8
    assert fw.Trainer is fw.HogwildTrainer and hasattr(fw.Trainer, "set_metrics") and hasattr(fw.Trainer, "metrics")


def test_null_and_bad_arguments_are_refused():
    L = capi.lib()
    sums = np.zeros(1, dtype=capi.METRIC_SUMS)
    n = C.c_uint64()
    assert L.fwgpu_batch_metrics(None, 0, 1, 0, capi.ptr(sums), None, None) == capi.ERR_INVALID
    assert L.fwgpu_trainer_set_metrics(None, 37) == capi.ERR_INVALID
    assert L.fwgpu_trainer_metrics(None, None, 0, C.byref(n), None, None) == capi.ERR_INVALID
    one = np.ones(4, dtype=np.float32)
    flags = np.ones(4, dtype=np.uint8)
    rows = np.zeros(4, dtype=capi.METRIC_WINDOW)
    args = (capi.ptr(one), capi.ptr(one), capi.ptr(one), capi.ptr(flags))
    assert L.fwgpu_debug_metrics(*args, 1, 4, 2, 0, capi.ptr(rows), 4, None, None, None, None) == capi.ERR_INVALID            # no n_rows
    assert L.fwgpu_debug_metrics(None, *args[1:], 1, 4, 2, 0, capi.ptr(rows), 4, C.byref(n), None, None, None) == capi.ERR_INVALID
    assert L.fwgpu_debug_metrics(*args, 1, 4, 0, 0, capi.ptr(rows), 4, C.byref(n), None, None, None) == capi.ERR_INVALID      # window 0
    assert L.fwgpu_debug_metrics(*args, 0, 4, 2, 0, capi.ptr(rows), 4, C.byref(n), None, None, None) == capi.ERR_INVALID      # numbers start at 1
    # examples 2 .. 5 in windows of 2 are the windows 0, 1 and 2: a buffer of two rows is too small, as for fwgpu_trainer_predictions
    assert L.fwgpu_debug_metrics(*args, 2, 4, 2, 0, capi.ptr(rows), 2, C.byref(n), None, None, None) == capi.ERR_RANGE
    assert n.value == 3 and b"too small" in L.fwgpu_last_error()


def test_metrics_ref_on_three_examples_by_hand():
    pred = np.array([0.5, 0.25, 0.0], dtype=np.float32)
    label = np.array([1.0, 0.0, 1.0], dtype=np.float32)
    imp = np.array([1.0, 2.0, 0.5], dtype=np.float32)
    l0, l1, l2 = math.log(2.0), -math.log(0.75), -math.log(1e-15)  # the third prediction is clipped to 1e-15
    s = mr.sums(pred, label, imp)
    assert (s["n"], s["n_unlabelled"], s["n_bad"]) == (3, 0, 0)
    assert s["sum_importance"] == 3.5 and s["sum_pred"] == 0.75 and s["sum_label"] == 2.0
    assert math.isclose(s["sum_loss_plain"], l0 + l1 + l2, rel_tol=4e-16)
    assert math.isclose(s["sum_loss"], l0 + 2.0 * l1 + 0.5 * l2, rel_tol=4e-16)
    assert 34.5 < l2 < 34.6
    # an unlabelled and a bad example enter no sum; windows of two, entered at number 4: {4}, {5, 6}, {7}
    pred = np.array([0.5, 0.25, np.nan, 0.0, 0.9], dtype=np.float32)
    label = np.array([1.0, 0.0, 1.0, 1.0, 255.0], dtype=np.float32)
    imp = np.array([1.0, 2.0, 4.0, 0.5, 8.0], dtype=np.float32)
    s = mr.sums(pred, label, imp)
    assert (s["n"], s["n_unlabelled"], s["n_bad"]) == (3, 1, 1) and s["sum_importance"] == 3.5
    rows = mr.windows(pred[:4], label[:4], imp[:4], [True, True, False, False], 4, 2)
    assert [r[0] for r in rows] == [3, 5, 7]
    assert rows[0][1]["n"] == 1 and rows[0][2]["n"] == 0 and math.isclose(rows[0][1]["sum_loss"], l0, rel_tol=4e-16)
    assert rows[1][1]["n"] == 1 and rows[1][2]["n"] == 0 and rows[1][2]["n_bad"] == 1 and math.isclose(rows[1][1]["sum_loss"], 2.0 * l1, rel_tol=4e-16)
    assert rows[2][1]["n"] == 0 and rows[2][2]["n"] == 1 and math.isclose(rows[2][2]["sum_loss"], 0.5 * l2, rel_tol=4e-16)
    h = mr.hist(pred, label)
    assert h.sum() == 3 and h[1, 128] == 1 and h[0, 64] == 1 and h[1, 0] == 1
    assert mr.hist(np.array([1.0, 255.0 / 256.0, 254.9 / 256.0], dtype=np.float32), np.zeros(3, dtype=np.float32))[0, 253:].tolist() == [0, 1, 2]
    assert mr.bound(96) == 100 * 2.0 ** -52


def test_binned_auc_on_a_hand_made_histogram():
    h = np.zeros((2, 256), dtype=np.uint64)
    h[0, 0], h[0, 5] = 2, 1            # three negatives
    h[1, 5], h[1, 9] = 1, 3            # four positives: the one in bin 5 beats two negatives and ties with one
    assert fw.binned_auc(h) == (2 + 0.5 + 3 * 3) / 12
    assert fw.binned_auc(h.reshape(-1)) == 11.5 / 12  # the flat hist[512] of the C struct
    sep = np.zeros((2, 256), dtype=np.uint64)
    sep[0, 10], sep[1, 200] = 7, 5
    assert fw.binned_auc(sep) == 1.0 and fw.binned_auc(sep[::-1]) == 0.0
    tie = np.zeros((2, 256), dtype=np.uint64)
    tie[0, 77], tie[1, 77] = 4, 9      # everything in one bin: no order at all
    assert fw.binned_auc(tie) == 0.5
    assert math.isnan(fw.binned_auc(np.zeros((2, 256)))) and math.isnan(fw.binned_auc(h * np.array([[1], [0]], dtype=np.uint64)))
