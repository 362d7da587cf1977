"""Training from VW text: the device text route (HogwildTrainer.digest_text_device: parse, micro-batch plan and placement on the device) against
the host route (HogwildTrainer.digest_text with 16 parser threads), config C's geometry (30 fields, k = 8, 28-bit tables, AdagradLUT, micro-batch
16 384), text from the generator of scripts/bench_text_parse.py repeated to at least 2 M lines.  One process; the legs alternate, each on a fresh
regressor of the same model, after a warm-up of both routes that is not timed.  A leg is timed by the host clock around digest + finish (finish
waits for the device).  Writes profiles/text_train.json: examples/s per leg (all runs, median, min, max), the share of lines the host parsed on
the device route and the time the host spent waiting for the parser's stream."""
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
args = ap.parse_args()
assert args.reps >= 1

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


def leg(device, t, n_want):
    """one pass over `t` on a fresh regressor -> (seconds, host lines, ns the host waited for the parser's stream)"""
    re = fw.Regressor(mi)
    tr = fw.HogwildTrainer(re, mi, micro_batch=args.micro_batch)
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
    tr.close()
    re.close()
    return dt, by_host, wait.value


leg(True, text * 4, BLOCK * 4), leg(False, text * 4, BLOCK * 4)  # warm-up: staging, both buffer sets at their piece size, parser threads, code objects
td, th, by_host, waits = [], [], 0, []
for r in range(args.reps):
    dt, by_host, wait = leg(True, big, N)
    td.append(dt)
    waits.append(wait / 1e9)
    th.append(leg(False, big, N)[0])


def summary(ts):
    rates = [N / t for t in ts]
    return {"seconds": ts, "examples_per_sec": rates, "median_examples_per_sec": float(np.median(rates)), "min_examples_per_sec": min(rates),
            "max_examples_per_sec": max(rates)}


out = {"lines": N, "text_bytes": len(big), "micro_batch": args.micro_batch, "table_bits": args.bits, "reps": args.reps,
       "device_route": dict(summary(td), what="digest_text_device + finish on a fresh regressor", host_lines_over_lines=by_host / N,
                            host_wait_on_parser_stream_seconds=waits,
                            host_wait_share_of_leg=float(np.median([w / t for w, t in zip(waits, td)]))),
       "host_route": dict(summary(th), what=f"digest_text with {args.threads} parser threads + finish on a fresh regressor")}
out["device_over_host_median"] = out["device_route"]["median_examples_per_sec"] / out["host_route"]["median_examples_per_sec"]
json.dump(out, open(args.out, "w"), indent=1)
print(json.dumps(out))
