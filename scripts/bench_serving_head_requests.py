"""The many-request launch on a DEEP-HEAD model (--head_requests: fwgpu_enable_head_requests, csrc/requests_head.hip) against what such a server does
without it, on the same lines in the same run.  Config E's geometry (30 fields, k = 16, two hidden layers of 256 ReLU units); every request has its own
context of about 150 features over 20 namespaces, its candidates hold 5 - 20 features in the other 10.  Grid: R in {1, 16, 64, 256} requests x
C in {16, 64, 256} candidates.  Per point
    (a) ONE fwgpu_predictor_predict_requests call,
    (b) R fwgpu_predictor_predict_batch(with_cache = 1) calls, one per request,
the legs alternating, every shape warmed up first, medians of ROUNDS with min - max, a host clock around calls that end in a synchronise, and the largest
|p_a - p_b|.  Also the launches alone at the C ABI on pre-built entry batches of 16 x 256 filtered candidates: one launch with a cache per example
(fwgpu_debug_requests_time: base kernel + head-input kernel + the layers, by device events) against 16 launches with one cache each
(fwgpu_batch_set_cache, a host clock around the 16 launches and one synchronise).  No ratio is fixed in advance.
Writes profiles/serving_head_requests.json.     usage: python3 scripts/bench_serving_head_requests.py [--rounds 5] [--small] [--bits 24] [--out FILE]"""
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
ap.add_argument("--bits", type=int, default=24)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "serving_head_requests.json"))
args = ap.parse_args()

F, K, NCTX, WIDTH = 30, 16, 20, 256
RS, CS = ([1, 16], [16, 64]) if args.small else ([1, 16, 64, 256], [16, 64, 256])
RMAX, CMAX = max(RS), max(CS)
KR, KC, KREPS = min(16, RMAX), CMAX, 20  # the launches-only batches
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


# ---- the model: config E's geometry, a short training pass so that the weights are not the initial ones
mi = fw.ModelInstance(learning_rate=0.025, ffm_learning_rate=0.025, power_t=0.38, ffm_power_t=0.38, bit_precision=args.bits, ffm_k=K,
                      ffm_bit_precision=args.bits, optimizer=fw.Optimizer.AdagradLUT, ffm_init_acc_gradient=1.0,
                      feature_combo_descs=[fw.FeatureComboDesc([fw.NamespaceDescriptor(i)]) for i in range(F)],
                      ffm_fields=[[fw.NamespaceDescriptor(i)] for i in range(F)])
mi.nn_layers = [dict(width=WIDTH, activation="relu", init="hu"), dict(width=WIDTH, activation="relu", init="hu")]
mi.nn_topology = "one"
re = fw.Regressor(mi)
recs, off = fw.synth_records(F, 5.67, 1.05, 1_000_000, 0.1, 5, 0, 20000)
b = re.record_batch(fw.FeatureBufferTranslator(mi), recs, off)
re.learn_batch(b, capi.MODE_HOGWILD, True)
b.predictions()
b.close()
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "head.fw")
P.save_regressor_to_filename(path, mi, vw, re)
re.close()
proto = Predictor(f"fw -i {path} -t --head_requests")
mi_k, _, rk = P.new_regressor_from_filename(path, immutable=True)  # the launches-only legs
shutil.rmtree(tmp)
prs = [proto] + [proto.clone_lite() for _ in range(RMAX - 1)]
ctxs = [context() for _ in range(RMAX)]
lines = [[candidate() for _ in range(CMAX)] for _ in range(RMAX)]
for pr, ctx in zip(prs, ctxs):
    assert pr.setup_cache(ctx + "\n") == 0.0
print(f"{RMAX} predictors ready; contexts of {np.mean([len(c.split()) - NCTX for c in ctxs]):.0f} features, candidates of "
      f"{np.mean([len(l.split()) - l.count('|') for r in lines for l in r]):.1f}", flush=True)


def point(R, C):
    n = R * C
    arrs = [Predictor.encode_batch(l[:C]) for l in lines[:R]]  # what a C caller holds
    legs = dict(a_predict_requests=lambda: serving.predict_requests(prs[:R], arrs),
                b_predict_batch_per_request=lambda: [prs[r].predict_batch(arrs[r], with_cache=True) for r in range(R)])
    first = {name: np.concatenate(fn()) for name, fn in legs.items()}  # (also the warm-up of this shape)
    assert all((p > 0).all() for p in first.values())
    for fn in legs.values():
        fn()
    ts = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, fn in legs.items():
            ts[name].append(clock(fn))
    row = dict(requests=R, candidates_per_request=C, candidates=n, **{name: stats(t, n) for name, t in ts.items()})
    row["max_abs_difference"] = float(np.abs(first["a_predict_requests"] - first["b_predict_batch_per_request"]).max())
    row["b_ms_over_a_ms"] = row["b_predict_batch_per_request"]["ms_median"] / row["a_predict_requests"]["ms_median"]
    print(f"R = {R:3d} x C = {C:3d}: (a) {fmt(row['a_predict_requests'])}  (b) {fmt(row['b_predict_batch_per_request'])}  b / a = {row['b_ms_over_a_ms']:.2f}  "
          f"max |d| {row['max_abs_difference']:.2e}", flush=True)
    return row


rows = [point(R, C) for R in RS for C in CS]

# ---- the launches alone: KR x KC filtered candidates, one launch with a cache per example against KR launches with one cache each
rk.enable_head_requests()
host = VowpalParser(vw)
fbt = fw.FeatureBufferTranslator(mi_k)
caches = [rk.setup_cache(fbt.translate(host.next_vowpal((ctx + "\n").encode()))) for ctx in ctxs[:KR]]
per_req = []
for r in range(KR):
    fbs = []
    for t in lines[r][:KC]:
        fb = fbt.translate(host.next_vowpal((ctxs[r] + t).encode()))
        fbs.append(fw.FeatureBuffer(label=0.0, example_importance=1.0, example_number=0, lr_buffer=fb.lr_buffer.copy(), ffm_buffer=caches[r].filter(fb.ffm_buffer)))
    per_req.append(fbs)
eb = rk.batch([fb for fbs in per_req for fb in fbs])
eb.set_caches(caches, np.repeat(np.arange(KR, dtype=np.uint32), KC))
obs = [rk.batch(fbs) for fbs in per_req]
for ob, c in zip(obs, caches):
    ob.set_cache(c)


def loop():
    for ob in obs:
        rk.learn_batch(ob, capi.MODE_HOGWILD, False)
    obs[-1].predictions()  # (one stream: the last batch's copy waits for them all)


rk.debug_requests_time(eb, 0, KREPS)
loop()
t_one, t_loop = [], []
for _ in range(args.rounds):
    t_one.append(rk.debug_requests_time(eb, 0, KREPS) * 1e-3)
    t_loop.append(clock(loop))
launch = rk.last_launch()
rk.learn_batch(eb, capi.MODE_HOGWILD, False)
kernels = dict(requests=KR, candidates_per_request=KC, launches_per_timing=KREPS, one_launch_with_a_cache_per_example=stats(t_one, KR * KC),
               one_launch_per_request_set_cache=stats(t_loop, KR * KC), head_requests_launch=rk.last_launch(), per_request_launch=launch)
print(f"launches alone, {KR} x {KC} candidates: one launch {fmt(kernels['one_launch_with_a_cache_per_example'])}, "
      f"{KR} launches {fmt(kernels['one_launch_per_request_set_cache'])}", flush=True)
for o in obs + [eb] + caches:
    o.close()
host.close()

out = dict(what="the requests route on a deep-head model: (a) one predict_requests call on --head_requests predictors; (b) the same predictors, one "
                "predict_batch(with_cache = 1) call per request; legs alternating in one process.  kernels: the launches alone at the C ABI on pre-built "
                "entry batches -- one launch with a cache per example by device events, against one launch per request by a host clock",
           geometry=dict(fields=F, k=K, bits=args.bits, hidden=[WIDTH, WIDTH], context_namespaces=NCTX), rounds=args.rounds,
           serving_threads=int(os.environ["FWGPU_SERVING_THREADS"]), kernels=kernels, points=rows)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
for pr in prs:
    pr.close()
rk.close()
