"""The delayed-prediction protocol restated on the CPU oracle (oracle/fwo.py), for tests/test_delay_cpu.py and tests/test_gpu_delay.py.

reference_loop is the reference's example loop for `--prediction_model_delay N` (main.rs:248-258) with a deque; window_rule is the trainer's
rule as include/fwgpu.h states it ("predicting with a model delayed by N examples"), written the slow and obvious way: after every window ALL
pending windows are looked at.  plan() is the rule's bookkeeping alone, without a model.  Examples are numbered from 1."""
from collections import deque

import numpy as np


def _examples(ots, recs, off):
    return [ots.translate(recs[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def reference_loop(om, ots, recs, off, N, predictions_after=0):
    """main.rs:248-258 on the oracle model `om` -> the predictions of the examples numbered > predictions_after"""
    assert N > 0
    queue, preds = deque(), []
    for i, (lr, ffm, label, imp) in enumerate(_examples(ots, recs, off), start=1):
        if i > predictions_after:
            preds.append(om.learn(lr, ffm, label, imp, update=False))
        queue.append((lr, ffm, label, imp))
        if len(queue) > N:
            lr, ffm, label, imp = queue.popleft()
            om.learn(lr, ffm, label, imp, update=True)
    return np.array(preds, dtype=np.float32)


def plan(windows, N):
    """windows: sizes of consecutive windows -> per window (last example number learned, examples pending, windows pending) after its step"""
    ends = np.cumsum(np.asarray(windows, dtype=np.int64))
    learned = np.zeros(len(ends), dtype=bool)
    out = []
    for j, e in enumerate(ends):
        for v in range(j + 1):  # every window taken so far, the new one included
            if not learned[v] and ends[v] <= e - N:
                assert v == 0 or learned[v - 1]  # oldest first
                learned[v] = True
        done = [v for v in range(j + 1) if learned[v]]
        through = int(ends[done[-1]]) if done else 0
        out.append((through, int(e) - through, j + 1 - len(done)))
    return out


def window_rule(om, ots, recs, off, windows, N, predictions_after=0, shift=0):
    """The trainer's rule on the oracle model `om`: `windows` are the sizes of the consecutive windows it cut.  -> the predictions of the
    examples numbered > predictions_after.  A window's examples are predicted with one model and learned in stream order.
    shift = +1 / -1 moves every learn step one window later / earlier (a wrong rule: the tests' teeth)."""
    assert N > 0 and sum(windows) == len(off) - 1
    ex = _examples(ots, recs, off)
    ends = [int(e) for e in np.cumsum(np.asarray(windows, dtype=np.int64))]
    learned = [False] * len(ends)
    preds = []
    for j, e in enumerate(ends):
        first = e - windows[j] + 1
        assert first > predictions_after or e <= predictions_after, "a window straddles predictions_after"
        if first > predictions_after:
            for lr, ffm, label, imp in ex[first - 1:e]:
                preds.append(om.learn(lr, ffm, label, imp, update=False))
        if shift > 0:
            e_rule = ends[j - 1] if j else 0
        elif shift < 0:
            e_rule = ends[j + 1] if j + 1 < len(ends) else e + windows[j]
        else:
            e_rule = e
        for v in range(j + 1):
            if not learned[v] and ends[v] <= e_rule - N:
                learned[v] = True
                for lr, ffm, label, imp in ex[ends[v] - windows[v]:ends[v]]:
                    om.learn(lr, ffm, label, imp, update=True)
    return np.array(preds, dtype=np.float32)


def cut(n, micro_batch, predictions_after=0):
    """the windows the host-fed trainer cuts from n examples digested without a fwgpu_finish in between, the last one closed by fwgpu_finish"""
    edge = min(n, predictions_after)
    return [min(micro_batch, edge - a) for a in range(0, edge, micro_batch)] + [min(micro_batch, n - a) for a in range(edge, n, micro_batch)]
