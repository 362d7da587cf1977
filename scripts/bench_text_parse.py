"""VW text -> raw-record batch in HBM: the device text route against the host route, config C shaped lines (the generator of
scripts/feed_rate.py, 480 000 lines).  One process, the two routes alternating:
  (a) fwgpu_record_batch_from_text: text in pageable host memory -> batch ready;
  (b) 16 host parser threads (parse_buffer on 16 slices cut at line breaks) -> fwgpu_record_batch_create.
  (c) the kernels alone come from a rocprofv3 kernel trace of a run of its own:
        rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_text_parse.py --trace-leg
        python scripts/bench_text_parse.py --kernel-stats DIR/.../*_kernel_stats.csv --out profiles/text_parse.json   (adds them to the file)
Writes profiles/text_parse.json: lines/s, GB/s of text, host_lines / lines."""
import argparse
import csv
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_parse.json"))
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--trace-leg", action="store_true", help="route (a) once and nothing else: the run rocprofv3 traces")
ap.add_argument("--kernel-stats", help="rocprofv3's kernel_stats.csv of a --trace-leg run: add the text kernels' totals to --out")
args = ap.parse_args()

if args.kernel_stats:
    d = json.load(open(args.out))
    rows = [r for r in csv.DictReader(open(args.kernel_stats)) if "text_" in r["Name"]]
    ks = {r["Name"].split("(")[0]: {"calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6} for r in rows}
    parse_ms = sum(v["total_ms"] for k, v in ks.items() if "text_parse" in k)
    all_ms = sum(v["total_ms"] for v in ks.values())
    d["c_kernels_alone"] = {"kernels": ks, "parse_kernels_ms": parse_ms, "all_text_kernels_ms": all_ms,
                            "lines_per_sec": d["lines"] / (all_ms / 1e3), "text_GB_per_sec": d["text_bytes"] / (all_ms / 1e3) / 1e9,
                            "what": "status pass + write pass + line index of one route-(a) call, summed from a rocprofv3 kernel trace of a run of its own"}
    json.dump(d, open(args.out, "w"), indent=1)
    print(json.dumps(d["c_kernels_alone"]))
    sys.exit(0)

import fwumious_wabbit_amd as fw  # noqa: E402
from fwumious_wabbit_amd.feed import DeviceVowpalParser, VowpalParser, VwNamespaceMap  # noqa: E402

F = 30
vw = VwNamespaceMap("".join(f"A{i},ns{i}\n" for i in range(F)))
rng = np.random.default_rng(1)
lines = []
for i in range(20000):  # scripts/feed_rate.py's generator
    parts = ["1" if rng.random() < 0.3 else "-1"]
    for ns in range(F):
        k = 1 + rng.poisson(5.67)
        parts.append(f"|A{ns} " + " ".join(f"{rng.integers(0, 10_000_000)}" + (f":{0.5 + 1.5 * rng.random():.3f}" if rng.random() < 0.1 else "") for _ in range(k)))
    lines.append(" ".join(parts) + "\n")
text = "".join(lines).encode()
big = text * 24
N = 20000 * 24

mi = fw.ModelInstance(learning_rate=0.025, ffm_learning_rate=0.025, power_t=0.38, ffm_power_t=0.38, bit_precision=24, ffm_k=8,
                      ffm_bit_precision=24, optimizer=fw.Optimizer.AdagradLUT, ffm_init_acc_gradient=1.0,
                      feature_combo_descs=[fw.FeatureComboDesc([fw.NamespaceDescriptor(i)]) for i in range(F)],
                      ffm_fields=[[fw.NamespaceDescriptor(i)] for i in range(F)])
re = fw.Regressor(mi)
fbt = fw.FeatureBufferTranslator(mi)
dev = DeviceVowpalParser(vw)


def route_a(t):
    t0 = time.perf_counter()
    b = re.record_batch_from_text(fbt, dev, t)
    dt = time.perf_counter() - t0
    n, host = b.n, dev.last_lines()[1]
    b.close()
    return dt, n, host


if args.trace_leg:
    dt, n, host = route_a(big)
    print(f"trace leg: {n} lines in {dt:.3f} s, {host} on the host")
    sys.exit(0)

T = args.threads
parsers = [VowpalParser(vw) for _ in range(T)]
pool = ThreadPoolExecutor(T)


def route_b(t):
    t0 = time.perf_counter()
    cuts = [0]
    for k in range(1, T):
        cuts.append(t.index(b"\n", max(cuts[-1], len(t) * k // T)) + 1)
    cuts.append(len(t))
    view = memoryview(t)
    parts = list(pool.map(lambda k: parsers[k].parse_buffer(bytes(view[cuts[k]:cuts[k + 1]])), range(T)))
    assert all(p[3] == 0 for p in parts)
    words = np.concatenate([p[0] for p in parts])
    offs, base = [np.zeros(1, dtype=np.uint64)], 0
    for p in parts:
        offs.append(p[1][1:] + np.uint64(base))
        base += int(p[1][-1])
    b = re.record_batch(fbt, words, np.concatenate(offs))
    dt = time.perf_counter() - t0
    n = b.n
    b.close()
    return dt, n


route_a(text), route_b(text)  # warm-up: staging, device buffers, worker threads
ta, tb, host = [], [], 0
for r in range(args.reps):
    dt, n, host = route_a(big)
    assert n == N
    ta.append(dt)
    dt, n = route_b(big)
    assert n == N
    tb.append(dt)


def leg(ts):
    m = sorted(ts)[len(ts) // 2]
    return {"seconds": ts, "median_seconds": m, "lines_per_sec": N / m, "text_GB_per_sec": len(big) / m / 1e9}


out = {"lines": N, "text_bytes": len(big), "host_lines_over_lines": host / N,
       "a_device_route": dict(leg(ta), what="fwgpu_record_batch_from_text, pageable text -> batch ready"),
       "b_host_route_16_threads": dict(leg(tb), what=f"{T} parse_buffer threads on slices -> fwgpu_record_batch_create (unchanged code: the parent's number)")}
json.dump(out, open(args.out, "w"), indent=1)
print(json.dumps(out))
