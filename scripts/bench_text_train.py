"""Training from VW text: the device text route (HogwildTrainer.digest_text_device: parse, micro-batch plan and placement on the device) against
the host route (HogwildTrainer.digest_text with 16 parser threads), config C's geometry (30 fields, k = 8, 28-bit tables, AdagradLUT, micro-batch
16 384), text from the generator of scripts/bench_text_parse.py repeated to at least 2 M lines.  One process; the legs alternate, each on a fresh
regressor of the same model, after a warm-up of both routes that is not timed.  A leg is timed by the host clock around digest + finish (finish
waits for the device).  Writes profiles/text_train.json: examples/s per leg (all runs, median, min, max), the share of lines the host parsed on
the device route and the time the host spent waiting for the parser's stream.

--metrics WINDOW: the progressive log loss scored on the device (HogwildTrainer.set_metrics, csrc/metrics.hip).  Every repeat then times the device
route twice, metrics off and metrics on, the one that goes first alternating; the host route runs once with metrics on.  Prints the last window's progressive log loss of
both routes and writes profiles/trainer_metrics.json: both rates with their min - max, and whether the difference of the medians lies inside the
off runs' own min - max.  profiles/text_train.json is not written in this mode."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_train.json"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--lines", type=int, default=2_000_000)
ap.add_argument("--bits", type=int, default=28)
ap.add_argument("--micro-batch", dest="micro_batch", type=int, default=16384)
ap.add_argument("--metrics", type=int, default=0, metavar="WINDOW", help="score the progressive log loss in windows of WINDOW examples; on/off rates to --metrics-out")
ap.add_argument("--metrics-out", dest="metrics_out", default=os.path.join(ROOT, "profiles", "trainer_metrics.json"))
args = ap.parse_args()
assert args.reps >= 1 and args.metrics >= 0

import fwumious_wabbit_amd as fw  # noqa: E402
from fwumious_wabbit_amd import capi  # noqa: E402
from fwumious_wabbit_amd.feed import DeviceVowpalParser, VowpalParser, VwNamespaceMap  # noqa: E402

F = 30
BLOCK = 20000
vw = VwNamespaceMap("".join(f"A{i},ns{i}\n" for i in range(F)))
rng = np.random.default_rng(1)
lines = []
for i in range(BLOCK):  # scripts/bench_text_parse.py's generator
    parts = ["1" if rng.random() < 0.3 else "-1"]
    for ns in range(F):
        k = 1 + rng.poisson(5.67)
        parts.append(f"|A{ns} " + " ".join(f"{rng.integers(0, 10_000_000)}" + (f":{0.5 + 1.5 * rng.random():.3f}" if rng.random() < 0.1 else "") for _ in range(k)))
    lines.append(" ".join(parts) + "\n")
text = "".join(lines).encode()
copies = -(-args.lines // BLOCK)
big = text * copies
N = BLOCK * copies

mi = fw.ModelInstance(learning_rate=0.025, ffm_learning_rate=0.025, power_t=0.38, ffm_power_t=0.38, bit_precision=args.bits, ffm_k=8,
                      ffm_bit_precision=args.bits, optimizer=fw.Optimizer.AdagradLUT, ffm_init_acc_gradient=1.0,
                      feature_combo_descs=[fw.FeatureComboDesc([fw.NamespaceDescriptor(i)]) for i in range(F)],
                      ffm_fields=[[fw.NamespaceDescriptor(i)] for i in range(F)])
host = VowpalParser(vw)
dev = DeviceVowpalParser(vw)


def leg(device, t, n_want, window=0, rows_out=None):
    """one pass over `t` on a fresh regressor -> (seconds, host lines, ns the host waited for the parser's stream); window: metrics on, the
    window rows and the learned total go to rows_out"""
    re = fw.Regressor(mi)
    tr = fw.HogwildTrainer(re, mi, micro_batch=args.micro_batch)
    if window:
        tr.set_metrics(window)
    t0 = time.perf_counter()
    if device:
        n, used, rc = tr.digest_text_device(dev, t)
    else:
        n, used, rc = tr.digest_text(host, t, threads=args.threads)
    tr.block_until_workers_finished()
    dt = time.perf_counter() - t0
    assert (n, used, rc) == (n_want, len(t), capi.OK) and tr.examples_seen() == n_want
    by_host, wait = 0, C.c_uint64()
    if device:
        by_host = dev.last_lines()[1]
        capi.check(capi.lib().fwgpu_text_parser_last_wait_ns(dev.h, C.byref(wait)))
    if window and rows_out is not None:
        rows_out[:] = tr.metrics()[:2]
    tr.close()
    re.close()
    return dt, by_host, wait.value


leg(True, text * 4, BLOCK * 4, args.metrics), leg(False, text * 4, BLOCK * 4)  # warm-up: staging, both buffer sets at their piece size, parser threads, code objects


def summary(ts):
    rates = [N / t for t in ts]
    return {"seconds": ts, "examples_per_sec": rates, "median_examples_per_sec": float(np.median(rates)), "min_examples_per_sec": min(rates),
            "max_examples_per_sec": max(rates)}


def last_window(m):
    """progressive log loss of the last full window and of the whole stream, from the rows and the learned total of HogwildTrainer.metrics()"""
    rows, total = m
    full = [r for r in rows if int(r["learned"]["n"]) + int(r["learned"]["n_unlabelled"]) + int(r["learned"]["n_bad"]) == args.metrics]
    r = (full or list(rows))[-1]["learned"]
    return {"first_number": int((full or list(rows))[-1]["first_number"]), "n": int(r["n"]), "logloss": float(r["sum_loss"] / r["sum_importance"]),
            "stream_logloss": float(total["sums"]["sum_loss"] / total["sums"]["sum_importance"]), "stream_n": int(total["sums"]["n"]),
            "stream_binned_auc": fw.binned_auc(total["hist"])}


if args.metrics:
    t_off, t_on, m_dev, m_host = [], [], [], []
    for r in range(args.reps):  # the same repeats, both settings in every repeat, the one that goes first alternating
        for on_leg in ((False, True) if r % 2 == 0 else (True, False)):
            if on_leg:
                t_on.append(leg(True, big, N, args.metrics, m_dev)[0])
            else:
                t_off.append(leg(True, big, N)[0])
    leg(False, big, N, args.metrics, m_host)
    off, on = summary(t_off), summary(t_on)
    diff = off["median_examples_per_sec"] - on["median_examples_per_sec"]
    inside = off["min_examples_per_sec"] <= on["median_examples_per_sec"] <= off["max_examples_per_sec"]
    out = {"lines": N, "text_bytes": len(big), "micro_batch": args.micro_batch, "table_bits": args.bits, "reps": args.reps, "window": args.metrics,
           "what": "digest_text_device + finish on a fresh regressor; metrics off and on in every repeat of one process, the first of the two alternating",
           "metrics_off": off, "metrics_on": on, "median_off_minus_on_examples_per_sec": diff, "on_over_off_median": on["median_examples_per_sec"] / off["median_examples_per_sec"],
           "on_median_inside_off_min_max": bool(inside),
           "progressive_logloss_device_route": last_window(m_dev), "progressive_logloss_host_route": last_window(m_host)}
    for route in ("device", "host"):
        w = out[f"progressive_logloss_{route}_route"]
        print(f"{route} route: window at {w['first_number']} ({w['n']} examples) progressive log loss {w['logloss']:.6f}; stream {w['stream_logloss']:.6f}")
    json.dump(out, open(args.metrics_out, "w"), indent=1)
    print(json.dumps(out))
    sys.exit(0)

td, th, by_host, waits = [], [], 0, []
for r in range(args.reps):
    dt, by_host, wait = leg(True, big, N)
    td.append(dt)
    waits.append(wait / 1e9)
    th.append(leg(False, big, N)[0])

out = {"lines": N, "text_bytes": len(big), "micro_batch": args.micro_batch, "table_bits": args.bits, "reps": args.reps,
       "device_route": dict(summary(td), what="digest_text_device + finish on a fresh regressor", host_lines_over_lines=by_host / N,
                            host_wait_on_parser_stream_seconds=waits,
                            host_wait_share_of_leg=float(np.median([w / t for w, t in zip(waits, td)]))),
       "host_route": dict(summary(th), what=f"digest_text with {args.threads} parser threads + finish on a fresh regressor")}
out["device_over_host_median"] = out["device_route"]["median_examples_per_sec"] / out["host_route"]["median_examples_per_sec"]
json.dump(out, open(args.out, "w"), indent=1)
print(json.dumps(out))
