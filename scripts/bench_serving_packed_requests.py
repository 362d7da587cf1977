"""Context caches and the many-request launch on PACKED weights (--packed_weights --packed_context_cache: fwgpu_packed_enable_caches, csrc/requests.hip)
against what a packed server does without them, and against the f32 requests route, on the same lines in the same run.  The setup is
scripts/bench_serving_requests.py's: config C's geometry (30 fields, k = 8, 28-bit tables); every request has its own context of about 150 features over
20 namespaces, its candidates hold 5 - 20 features in the other 10.  Grid: R in {1, 16, 64, 256} requests x C in {16, 64, 256} candidates.  Per point
    (a) a plain --packed_weights predictor, one fwgpu_predictor_predict_batch(with_cache = 1) call per request: whole lines scored (the parent commit),
    (b) a --packed_weights --packed_context_cache predictor, one such call per request: the filtered candidate against the cache,
    (c) the predictors of (b), ONE fwgpu_predictor_predict_requests call,
    (d) f32 predictors, ONE fwgpu_predictor_predict_requests call -- the leg of profiles/serving_requests.json, measured again here and compared with
        the minimum and maximum recorded there,
the legs alternating, every shape warmed up first, medians of ROUNDS with min - max, a host clock around calls that end in a synchronise.  All three models
are loaded from ONE quantised inference file, so the f32 predictors hold the very values the buckets stand for: (c) and (d) must agree bit for bit.
Also: fw_setup_cache per context, packed and f32; and the requests kernels alone on a pre-built entry batch of 16 x 256 candidates by device events
(fwgpu_debug_requests_time), the packed predict kernel with 4 and with 8 rows in flight, alternating.  No ratio is fixed in advance.
Writes profiles/serving_packed_requests.json.     usage: python3 scripts/bench_serving_packed_requests.py [--rounds 5] [--small] [--bits 28] [--out FILE]"""
import argparse, json, os, shutil, sys, tempfile, time
os.environ.setdefault("FWGPU_SERVING_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import _capi as capi, persistence as P, serving
from fwumious_wabbit_amd.feed import VowpalParser, VwNamespaceMap
from fwumious_wabbit_amd.serving import Predictor

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--small", action="store_true", help="R <= 16, C <= 64")
ap.add_argument("--bits", type=int, default=28)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "serving_packed_requests.json"))
ap.add_argument("--earlier", default=os.path.join(ROOT, "profiles", "serving_requests.json"))
args = ap.parse_args()

F, K, NCTX = 30, 8, 20
RS, CS = ([1, 16], [16, 64]) if args.small else ([1, 16, 64, 256], [16, 64, 256])
RMAX, CMAX = max(RS), max(CS)
KR, KC, KREPS = min(16, RMAX), CMAX, 50  # the kernels-only batch
vw = VwNamespaceMap("".join(f"N{i:02d},ns{i}\n" for i in range(F)))
rng = np.random.default_rng(1)


def feature():
    return f"f{rng.zipf(1.3) % 100000}"


def context():  # about 150 features over the first 20 namespaces
    return " ".join(f"|N{i:02d} " + " ".join(feature() for _ in range(1 + rng.poisson(6.5))) for i in range(NCTX)) + " "


def candidate():  # 5 - 20 features in the other 10 namespaces
    while True:
        n = rng.integers(0, 3, F - NCTX)
        if 5 <= n.sum() <= 20:
            return " ".join(f"|N{NCTX + i:02d} " + " ".join(feature() for _ in range(n[i])) for i in range(F - NCTX) if n[i]) + "\n"


def stats(ts, n):
    ts = np.asarray(ts)
    return dict(candidates_per_s=float(n / np.median(ts)), ms_median=float(np.median(ts) * 1e3), ms_min=float(ts.min() * 1e3), ms_max=float(ts.max() * 1e3))


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def fmt(s):
    return f"{s['ms_median']:.3f} ms ({s['ms_min']:.3f} - {s['ms_max']:.3f})"


# ---- the model: config C's geometry, a short training pass so that the weights are not the initial ones; ONE quantised inference file
mi = fw.ModelInstance(learning_rate=0.025, ffm_learning_rate=0.025, power_t=0.38, ffm_power_t=0.38, bit_precision=args.bits, ffm_k=K,
                      ffm_bit_precision=args.bits, optimizer=fw.Optimizer.AdagradLUT, ffm_init_acc_gradient=1.0,
                      feature_combo_descs=[fw.FeatureComboDesc([fw.NamespaceDescriptor(i)]) for i in range(F)],
                      ffm_fields=[[fw.NamespaceDescriptor(i)] for i in range(F)])
re = fw.Regressor(mi)
recs, off = fw.synth_records(F, 5.67, 1.05, 1_000_000, 0.1, 5, 0, 20000)
b = re.record_batch(fw.FeatureBufferTranslator(mi), recs, off)
re.learn_batch(b, capi.MODE_HOGWILD, True)
b.predictions()
b.close()
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "q.fw")
P.save_inference_regressor(path, mi, vw, re, quantize_weights=True)
re.close()
print("inference file written", flush=True)
protos = dict(plain=Predictor(f"fw -i {path} -t --packed_weights"), cached=Predictor(f"fw -i {path} -t --packed_weights --packed_context_cache"),
              f32=Predictor(f"fw -i {path} -t"))
mi_p, _, rp = P.new_regressor_from_filename(path, immutable=True, packed=True, packed_caches=True)  # the kernels-only legs
mi_f, _, rf = P.new_regressor_from_filename(path, immutable=True)
shutil.rmtree(tmp)
prs = {name: [p] + [p.clone_lite() for _ in range(RMAX - 1)] for name, p in protos.items()}
ctxs = [context() for _ in range(RMAX)]
lines = [[candidate() for _ in range(CMAX)] for _ in range(RMAX)]

# ---- fw_setup_cache per context (the plain packed predictor only keeps the text)
setup = {}
for name in ("plain", "cached", "f32"):
    for pr, ctx in zip(prs[name], ctxs):  # (the first pass: allocations, code objects)
        assert pr.setup_cache(ctx + "\n") == 0.0
    ts = []
    for _ in range(args.rounds):
        ts.append(clock(lambda: [pr.setup_cache(ctx + "\n") for pr, ctx in zip(prs[name], ctxs)]) / RMAX)
    setup[name] = stats(ts, 1)
    print(f"fw_setup_cache per context, {name}: {fmt(setup[name])}", flush=True)
print(f"{RMAX} predictors of each kind ready; contexts of {np.mean([len(c.split()) - NCTX for c in ctxs]):.0f} features, candidates of "
      f"{np.mean([len(l.split()) - l.count('|') for r in lines for l in r]):.1f}", flush=True)

earlier = {}
if os.path.exists(args.earlier):
    for row in json.load(open(args.earlier))["points"]:
        earlier[(row["requests"], row["candidates_per_request"])] = row["predict_requests"]


def point(R, C):
    n = R * C
    arrs = [Predictor.encode_batch(l[:C]) for l in lines[:R]]  # what a C caller holds
    legs = dict(a_packed_whole_lines_per_request=lambda: [prs["plain"][r].predict_batch(arrs[r], with_cache=True) for r in range(R)],
                b_packed_cached_per_request=lambda: [prs["cached"][r].predict_batch(arrs[r], with_cache=True) for r in range(R)],
                c_packed_predict_requests=lambda: serving.predict_requests(prs["cached"][:R], arrs),
                d_f32_predict_requests=lambda: serving.predict_requests(prs["f32"][:R], arrs))
    first = {name: np.concatenate(fn()) for name, fn in legs.items()}  # (also the warm-up of this shape)
    assert all((p > 0).all() for p in first.values())
    for fn in legs.values():
        fn()
    ts = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, fn in legs.items():
            ts[name].append(clock(fn))
    row = dict(requests=R, candidates_per_request=C, candidates=n, **{name: stats(t, n) for name, t in ts.items()})
    row["max_abs_difference"] = dict(b_against_a=float(np.abs(first["b_packed_cached_per_request"] - first["a_packed_whole_lines_per_request"]).max()),
                                     c_against_b=float(np.abs(first["c_packed_predict_requests"] - first["b_packed_cached_per_request"]).max()),
                                     c_against_d=float(np.abs(first["c_packed_predict_requests"] - first["d_f32_predict_requests"]).max()))
    ms = lambda name: row[name]["ms_median"]
    row["a_ms_over_b_ms"] = ms("a_packed_whole_lines_per_request") / ms("b_packed_cached_per_request")
    row["a_ms_over_c_ms"] = ms("a_packed_whole_lines_per_request") / ms("c_packed_predict_requests")
    row["d_ms_over_c_ms"] = ms("d_f32_predict_requests") / ms("c_packed_predict_requests")
    e = earlier.get((R, C))
    if e:
        row["d_earlier"] = dict(ms_median=e["ms_median"], ms_min=e["ms_min"], ms_max=e["ms_max"])
        row["d_median_inside_earlier_min_max"] = bool(e["ms_min"] <= ms("d_f32_predict_requests") <= e["ms_max"])
        row["d_not_slower_than_earlier_max"] = bool(ms("d_f32_predict_requests") <= e["ms_max"])
    print(f"R = {R:3d} x C = {C:3d}: (a) {fmt(row['a_packed_whole_lines_per_request'])}  (b) {fmt(row['b_packed_cached_per_request'])}  (c) {fmt(row['c_packed_predict_requests'])}  "
          f"(d) {fmt(row['d_f32_predict_requests'])}" + (f"  [earlier (d): {e['ms_median']:.3f} ({e['ms_min']:.3f} - {e['ms_max']:.3f})]" if e else "") +
          f"  max |d|: b-a {row['max_abs_difference']['b_against_a']:.2e}, c-b {row['max_abs_difference']['c_against_b']:.2e}, c-d {row['max_abs_difference']['c_against_d']:.2e}", flush=True)
    return row


rows = [point(R, C) for R in RS for C in CS]

# ---- the kernels alone, by device events: one entry batch of KR x KC filtered candidates with a cache per example, on the packed and on the f32 regressor
host = VowpalParser(vw)
kernels = {}
for name, reg, mi_x in (("packed", rp, mi_p), ("f32", rf, mi_f)):
    fbt = fw.FeatureBufferTranslator(mi_x)
    caches = [reg.setup_cache(fbt.translate(host.next_vowpal((ctx + "\n").encode()))) for ctx in ctxs[:KR]]
    fbs = []
    for r in range(KR):
        for t in lines[r][:KC]:
            fb = fbt.translate(host.next_vowpal((ctxs[r] + t).encode()))
            fbs.append(fw.FeatureBuffer(label=0.0, example_importance=1.0, example_number=0, lr_buffer=fb.lr_buffer.copy(), ffm_buffer=caches[r].filter(fb.ffm_buffer)))
    eb = reg.batch(fbs)
    eb.set_caches(caches, np.repeat(np.arange(KR, dtype=np.uint32), KC))
    depths = (4, 8) if name == "packed" else (0,)
    ts = {d: [] for d in depths}
    for d in depths:
        reg.debug_requests_time(eb, d, KREPS)
    for _ in range(args.rounds):
        for d in depths:
            ts[d].append(reg.debug_requests_time(eb, d, KREPS) * 1e-3)
    kernels[name] = {("rows_in_flight_%d" % d if d else "rows_in_flight_4"): stats(ts[d], KR * KC) for d in depths}
    kernels[name]["launch"] = reg.last_launch()
    for d in depths:
        print(f"requests kernels alone, {name}, {d or 4} rows in flight, {KR} x {KC} candidates: {fmt(stats(ts[d], KR * KC))} per launch", flush=True)
    eb.close()
    for c in caches:
        c.close()
host.close()

out = dict(what="context caches on packed weights: (a) plain --packed_weights predictors, one predict_batch(with_cache = 1) per request (whole lines); (b) "
                "--packed_weights --packed_context_cache predictors, the same calls (filtered candidates against the cache); (c) those predictors, one "
                "predict_requests call; (d) f32 predictors, one predict_requests call, with the numbers of profiles/serving_requests.json beside it; legs "
                "alternating in one process.  setup_cache: fw_setup_cache per context.  kernels: base + predict kernel per launch by device events",
           geometry=dict(fields=F, k=K, bits=args.bits, context_namespaces=NCTX), rounds=args.rounds, serving_threads=int(os.environ["FWGPU_SERVING_THREADS"]),
           setup_cache_per_context=setup, kernels=dict(requests=KR, candidates_per_request=KC, launches_per_timing=KREPS, **kernels), points=rows)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
for group in prs.values():
    for pr in group:
        pr.close()
rp.close()
rf.close()
