"""The delayed protocol's eligibility rule (fwgpu_debug_delay_plan: the host function the trainer's ring is driven by, include/fwgpu.h "predicting
with a model delayed by N examples") against the brute-force restatement tests/delay_ref.py, the two bounds the header states, and the
restatement itself against the reference's loop on the CPU oracle.  No GPU."""
import numpy as np
import pytest

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import capi
from oracle import fwo

import delay_ref
from helpers import make_pair

DELAYS = [1, 2, 7, 8, 9, 100]
MAX_WINDOW = 8


def _windows(seed, n=90):
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(1, MAX_WINDOW + 1, size=n)]


@pytest.mark.parametrize("delay", DELAYS)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_plan_equals_the_brute_force_rule(seed, delay):
    windows = _windows(seed)
    ends = np.cumsum(windows)
    got = fw.debug_delay_plan(ends, delay)
    want = delay_ref.plan(windows, delay)
    assert [int(x) for x in got] == [w[0] for w in want]
    assert int(got[-1]) > 0 or delay == 100 and ends[-1] < 100 + MAX_WINDOW  # (the case has windows that are learned)
    # every prefix is a plan of its own: the rule never looks ahead
    for m in (1, 2, 17):
        assert np.array_equal(fw.debug_delay_plan(ends[:m], delay), got[:m])


@pytest.mark.parametrize("delay", DELAYS)
@pytest.mark.parametrize("full", [False, True], ids=["ragged", "full-windows"])
def test_the_two_bounds_hold_for_every_example(full, delay):
    windows = [MAX_WINDOW] * 40 if full else _windows(7, 120)
    ends = np.cumsum(windows)
    after = fw.debug_delay_plan(ends, delay)
    tight_upper = tight_lower = False
    for j, e in enumerate(ends):
        model = int(after[j - 1]) if j else 0  # what window j's predict launch sees
        for i in range(int(e) - windows[j] + 1, int(e) + 1):
            assert model <= max(0, i - 1 - delay), (i, model)                         # never fresher than the reference's
            assert model >= i - 1 - delay - (2 * MAX_WINDOW - 2), (i, model)          # never staler than this
            tight_upper |= model == i - 1 - delay and model > 0
            tight_lower |= model == i - 1 - delay - (2 * MAX_WINDOW - 2) and model > 0
    assert int(ends[-1]) > delay + 3 * MAX_WINDOW
    # both bounds are met.  Full windows: a window's first example meets the upper one iff the delay is a whole number of windows, its last example
    # the lower one iff delay = 8 q + 1; ragged windows: the upper one wherever two window ends lie exactly `delay` apart
    if full:
        assert tight_upper == (delay % MAX_WINDOW == 0) and tight_lower == (delay % MAX_WINDOW == 1)
    else:
        assert tight_upper


@pytest.mark.parametrize("delay", DELAYS)
def test_windows_of_one_are_the_reference_loop(delay):
    ends = np.arange(1, 301, dtype=np.uint64)
    assert [int(x) for x in fw.debug_delay_plan(ends, delay)] == [max(0, i - delay) for i in range(1, 301)]


def test_plan_refuses_what_is_no_plan():
    L = capi.lib()
    out = np.zeros(3, dtype=np.uint64)
    for ends, delay in (([1, 2, 3], 0), ([0, 1, 2], 1), ([1, 3, 3], 1), ([4, 2, 9], 2)):
        a = np.array(ends, dtype=np.uint64)
        assert L.fwgpu_debug_delay_plan(capi.ptr(a), 3, delay, capi.ptr(out)) == capi.ERR_INVALID
        assert b"delay" in L.fwgpu_last_error()
    assert L.fwgpu_debug_delay_plan(None, 0, 1, None) == capi.OK


@pytest.mark.parametrize("delay,predictions_after", [(1, 0), (5, 7), (64, 0), (400, 3)])
def test_window_rule_with_windows_of_one_is_the_reference_loop_on_the_oracle(delay, predictions_after):
    n = 250
    _, ocfg, ots = make_pair(5, 4, 14, 14, fw.Optimizer.AdagradLUT)
    recs, off = fw.synth_records(5, 1.0, 1.1, 40, 0.2, 11, 0, n)
    a, b = fwo.Model(ocfg), fwo.Model(ocfg)
    p_loop = delay_ref.reference_loop(a, ots, recs, off, delay, predictions_after)
    p_rule = delay_ref.window_rule(b, ots, recs, off, [1] * n, delay, predictions_after)
    assert len(p_loop) == n - predictions_after and np.array_equal(p_loop, p_rule)
    for name in ("lr_table", "ffm_weights", "ffm_acc"):
        assert np.array_equal(getattr(a, name), getattr(b, name))
    # the loop did learn, and left the last `delay` examples unlearned: one more example would change the tables
    c = fwo.Model(ocfg)
    assert (delay >= n) == bool(np.array_equal(a.ffm_weights, c.ffm_weights))
    assert len(np.unique(p_loop)) > (n - predictions_after) // 2


def test_cut_is_what_the_header_says():
    assert delay_ref.cut(50, 16) == [16, 16, 16, 2]
    assert delay_ref.cut(50, 16, 7) == [7, 16, 16, 11]
    assert delay_ref.cut(50, 16, 20) == [16, 4, 16, 14]
    assert delay_ref.cut(5, 16, 20) == [5]
