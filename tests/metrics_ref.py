"""float64 yardstick of the device metrics (csrc/metrics.hip, include/fwgpu.h "progressive and hold-out loss"): the log loss of bench.py / the
reference's benchmark/calc_loss.py -- p = clip(pred, 1e-15, 1 - 1e-15), loss = -log(p) if label == 1 else -log(1 - p) -- per example in numpy
float64, summed exactly (math.fsum) window by window and side by side.

Tolerance of a device f64 sum against it (derived, not measured): every loss term is non-negative, the device adds a window's n terms in some
order (at most n - 1 roundings of 2^-53 relative to a partial sum that never exceeds the total) and its log is correctly rounded give or take
2 ulp against numpy's, so |got - want| <= (n + 4) * 2^-52 * want on sum_loss, sum_loss_plain and sum_importance, and the same bound relative
to sum |term| on sum_pred and sum_label.  Counts and histograms are integers and must be equal."""
import math

import numpy as np

NO_LABEL = 255.0  # parser.rs:28, as the translator turns the record's word 1 into a float
COUNTS = ("n", "n_unlabelled", "n_bad")
SUMS = ("sum_importance", "sum_loss", "sum_loss_plain", "sum_pred", "sum_label")


def logloss64(pred, label):
    """bench.py:146-148 / calc_loss.py per example, float64"""
    p = np.clip(np.asarray(pred, dtype=np.float32).astype(np.float64), 1e-15, 1 - 1e-15)
    with np.errstate(invalid="ignore", divide="ignore"):
        return -np.where(np.asarray(label) == 1, np.log(p), np.log(1 - p))


def kinds(pred, label):
    """(scored, unlabelled, bad) masks: NO_LABEL first, then a prediction that is not finite"""
    pred, label = np.asarray(pred, dtype=np.float32), np.asarray(label, dtype=np.float32)
    unl = label == np.float32(NO_LABEL)
    bad = ~unl & ~np.isfinite(pred)
    return ~(unl | bad), unl, bad


def sums(pred, label, importance, sel=None):
    """one side's fwgpu_metric_sums of the selected examples, as a dict; abs_pred / abs_label are the sum |term| the bound of sum_pred / sum_label is relative to"""
    pred, label, importance = (np.asarray(a, dtype=np.float32) for a in (pred, label, importance))
    sel = np.ones(len(pred), dtype=bool) if sel is None else np.asarray(sel, dtype=bool)
    ok, unl, bad = kinds(pred, label)
    ok, unl, bad = ok & sel, unl & sel, bad & sel
    loss = logloss64(pred[ok], label[ok])
    imp, p, y = importance[ok].astype(np.float64), pred[ok].astype(np.float64), label[ok].astype(np.float64)
    return {"n": int(ok.sum()), "n_unlabelled": int(unl.sum()), "n_bad": int(bad.sum()),
            "sum_importance": math.fsum(imp), "sum_loss": math.fsum(imp * loss), "sum_loss_plain": math.fsum(loss),
            "sum_pred": math.fsum(p), "sum_label": math.fsum(y), "abs_pred": math.fsum(np.abs(p)), "abs_label": math.fsum(np.abs(y)),
            "abs_importance": math.fsum(np.abs(imp)), "abs_loss": math.fsum(np.abs(imp * loss))}


def hist(pred, label, sel=None):
    """[2, 256] counts of the scored, selected examples: class 1 = label == 1, bin = min(255, int(pred * 256)) on the raw f32 prediction"""
    pred, label = np.asarray(pred, dtype=np.float32), np.asarray(label, dtype=np.float32)
    ok = kinds(pred, label)[0]
    if sel is not None:
        ok = ok & np.asarray(sel, dtype=bool)
    b = np.clip(pred[ok].astype(np.float64) * 256.0, 0.0, 255.0).astype(np.int64)  # (trunc == floor: not negative)
    out = np.zeros((2, 256), dtype=np.uint64)
    np.add.at(out, ((label[ok] == 1).astype(np.int64), b), 1)
    return out


def windows(pred, label, importance, learned, first_number, window):
    """[(first number of the window, learned sums, held-out sums)] for the windows the examples first_number .. first_number + n - 1 fall into"""
    n = len(pred)
    learned = np.broadcast_to(np.asarray(learned, dtype=bool), (n,))
    w = (first_number - 1 + np.arange(n, dtype=np.int64)) // window
    out = []
    for k in range(int(w[0]), int(w[-1]) + 1) if n else []:
        m = w == k
        out.append((k * window + 1, sums(pred, label, importance, m & learned), sums(pred, label, importance, m & ~learned)))
    return out


def totals(pred, label, importance, learned):
    """((learned sums, learned hist), (held-out sums, held-out hist))"""
    learned = np.broadcast_to(np.asarray(learned, dtype=bool), (len(pred),))
    return ((sums(pred, label, importance, learned), hist(pred, label, learned)),
            (sums(pred, label, importance, ~learned), hist(pred, label, ~learned)))


def bound(n, sides=1):
    return sides * (n + 4) * 2.0 ** -52


def check_sums(got, want, what="", sides=1):
    """a fwgpu_metric_sums record (numpy) against a dict of sums(); sides = 2: `want` carries the same error (two device runs)"""
    for f in COUNTS:
        assert int(got[f]) == int(want[f]), (what, f, int(got[f]), int(want[f]))
    b = bound(int(want["n"]), sides)
    names = want.dtype.names if hasattr(want, "dtype") else want.keys()  # (a device record has no abs_*: its terms are not negative)
    for f, ref in (("sum_importance", "abs_importance"), ("sum_loss", "abs_loss"), ("sum_loss_plain", "sum_loss_plain"), ("sum_pred", "abs_pred"),
                   ("sum_label", "abs_label")):
        scale = abs(float(want[ref] if ref in names else want[f]))
        assert abs(float(got[f]) - float(want[f])) <= b * scale, (what, f, float(got[f]), float(want[f]), b * scale)


def check_rows(rows, want, sides=1):
    """the rows of fwgpu_trainer_metrics / fwgpu_debug_metrics against windows()"""
    assert len(rows) == len(want), (len(rows), len(want))
    for r, (first, lw, hw) in zip(rows, want):
        assert int(r["first_number"]) == first
        check_sums(r["learned"], lw, f"window at {first}, learned", sides)
        check_sums(r["held_out"], hw, f"window at {first}, held out", sides)


def check_total(got, want, what="", sides=1):
    check_sums(got["sums"], want[0], what, sides)
    assert np.array_equal(np.asarray(got["hist"]).reshape(2, 256), want[1]), what
    assert int(np.asarray(got["hist"]).sum()) == int(want[0]["n"])
