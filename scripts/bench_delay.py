"""Cost of the delayed protocol (HogwildTrainer.set_delay, `--prediction_model_delay`): config C's geometry (30 fields, k = 8, 28-bit tables,
AdagradLUT), records from fwgpu_synth_records in host memory, fed through digest_records at the default micro-batch of the trainer scripts
(16 384).  One process, one regressor; every leg is a fresh trainer and is timed by the host clock around digest + finish (finish waits for the
device) over the same --examples records, after an untimed lead-in:
  (a) plain training                      lead-in: two micro-batches
  (b) a predict-only pass (testonly)      lead-in: two micro-batches
  (c) delayed training, per delay         lead-in: delay + two micro-batches, so that the ring is full and every timed window costs its predict
                                          launch AND the learn launch of the window that leaves the ring
The legs alternate within every repeat.  Writes profiles/trainer_delay.json: per leg all rates, median, min, max; (c) next to
1 / (1/a + 1/b), the cost of the two launches a window consists of; the share of a leg the host spends inside digest (the rest is finish
waiting for the device: a leg that waits little is bound by the host's staging and upload, not by the launches); the ring's bytes."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trainer_delay.json"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--examples", type=int, default=1 << 20, help="examples of the timed section of every leg")
ap.add_argument("--delays", type=int, nargs="+", default=[65536, 1 << 20])
ap.add_argument("--micro-batch", dest="micro_batch", type=int, default=16384)
ap.add_argument("--bits", type=int, default=28)
args = ap.parse_args()

import bench  # noqa: E402
import fwumious_wabbit_amd as fw  # noqa: E402


class G:  # bench.py's config C
    fields, k, nn_layers, nn_width = 30, 8, 0, 256
    mean_extra, zipf, ids, p_weighted, seed = 5.67, 1.05, 10_000_000, 0.1, 20240612


G.bits = G.ffm_bits = args.bits
MB, M = args.micro_batch, args.examples
S = max(M, max(args.delays) + 2 * MB)
mi = bench.build_model_instance(fw, G, 0)
recs, off = bench.gen_records(fw, G, 0, S)
re = fw.Regressor(mi)


def feed(tr, n):
    t0 = time.perf_counter()
    tr.digest_records(recs[: int(off[n])], off[: n + 1])
    t1 = time.perf_counter()
    tr.block_until_workers_finished()
    return t1 - t0, time.perf_counter() - t1


def leg(kind, delay=0):
    tr = fw.HogwildTrainer(re, mi, micro_batch=MB)
    if kind == "predict":
        tr.set_holdout(testonly=True)
    if delay:
        tr.set_delay(delay)
    feed(tr, delay + 2 * MB)  # lead-in
    before = tr.delay_state()
    t_digest, t_finish = feed(tr, M)
    state = tr.delay_state()
    if delay:  # steady state: what came in went out
        assert state["learned_through"] - before["learned_through"] >= M - MB and state["pending_examples"] <= delay + 2 * MB, (before, state)
    tr.close()
    return t_digest, t_finish, state["ring_bytes"]


legs = [("plain", 0), ("predict", 0)] + [("delayed", d) for d in args.delays]
times = {l: [] for l in legs}
for r in range(args.reps):
    for l in legs[r % len(legs):] + legs[: r % len(legs)]:
        times[l].append(leg(*l))


def summary(ts):
    rates = [M / (a + b) for a, b, _ in ts]
    return {"seconds": [a + b for a, b, _ in ts], "examples_per_sec": rates, "median_examples_per_sec": float(np.median(rates)),
            "min_examples_per_sec": min(rates), "max_examples_per_sec": max(rates),
            "host_in_digest_share_of_leg": float(np.median([a / (a + b) for a, b, _ in ts]))}


out = {"examples_timed": M, "micro_batch": MB, "table_bits": args.bits, "reps": args.reps, "record_bytes": int(recs[: int(off[M])].nbytes),
       "what": "digest_records + finish from host memory on one regressor, a fresh trainer per leg, after an untimed lead-in (delayed: the ring full)",
       "plain": summary(times[("plain", 0)]), "predict_only": summary(times[("predict", 0)]), "delayed": {}}
a, b = out["plain"]["median_examples_per_sec"], out["predict_only"]["median_examples_per_sec"]
both = 1.0 / (1.0 / a + 1.0 / b)
out["two_launches_examples_per_sec"] = both
out["two_launches_over_plain"] = both / a
for d in args.delays:
    s = summary(times[("delayed", d)])
    s["ring_bytes"] = times[("delayed", d)][-1][2]
    s["over_two_launches"] = s["median_examples_per_sec"] / both
    s["over_plain"] = s["median_examples_per_sec"] / a
    out["delayed"][str(d)] = s
    print(f"delay {d}: {s['median_examples_per_sec'] / 1e6:.2f} M examples/s ({s['min_examples_per_sec'] / 1e6:.2f} - {s['max_examples_per_sec'] / 1e6:.2f}), "
          f"{s['over_two_launches']:.3f} of 1 / (1/a + 1/b) = {both / 1e6:.2f} M; the host inside digest {s['host_in_digest_share_of_leg']:.0%} of the leg; "
          f"ring {s['ring_bytes'] / 2 ** 20:.0f} MiB")
print(f"plain {a / 1e6:.2f} M examples/s, predict-only {b / 1e6:.2f} M examples/s")
json.dump(out, open(args.out, "w"), indent=1)
print(json.dumps(out))
re.close()
