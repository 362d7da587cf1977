"""The many-request launch on a DEEP-HEAD model served from PACKED FFM weights (--packed_weights --packed_head_requests:
fwgpu_packed_enable_head_requests, the packed form of csrc/requests_head.hip) against what such a server does without the token and against the f32
load, on the same lines in the same run.  Config E's geometry (30 fields, k = 16, two hidden layers of 256 ReLU units); every request has its own context
of about 150 features over 20 namespaces, its candidates hold 5 - 20 features in the other 10.  All predictors load ONE quantised inference file.
Grid: R in {1, 16, 64, 256} requests x C in {16, 64, 256} candidates.  Per point
    (a) R fwgpu_predictor_predict_batch(with_cache = 1) calls on --packed_weights predictors: whole context + candidate lines (no device cache),
    (b) ONE fwgpu_predictor_predict_requests call on --packed_weights --packed_head_requests predictors,
    (c) ONE fwgpu_predictor_predict_requests call on --head_requests predictors (f32 tables),
the legs alternating, every shape warmed up first, medians of ROUNDS with min - max, a host clock around calls that end in a synchronise, and the largest
|p_b - p_a|, |p_b - p_c|.  Also the launches alone at the C ABI on pre-built entry batches of 16 x 256 candidates, by device events
(fwgpu_debug_requests_time: base kernel + head-input kernel + the layers): the packed table at 4 and at 8 rows in flight and the f32 table, filtered
candidates with a cache per example; and the whole lines on the packed head route (FWGPU_ROUTE_PACKED_HEAD), a host clock around one launch and its
synchronise.  No ratio is fixed in advance.
Writes profiles/serving_packed_head_requests.json.     usage: python3 scripts/bench_serving_packed_head_requests.py [--rounds 5] [--small] [--bits 24] [--out FILE]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "serving_packed_head_requests.json"))
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


# ---- the model: config E's geometry, a short training pass so that the weights are not the initial ones; ONE quantised file for every load
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
trained, path = os.path.join(tmp, "head.fw"), os.path.join(tmp, "head.q.fw")
P.save_regressor_to_filename(trained, mi, vw, re)
re.close()
P.convert_inference_regressor(trained, path, quantize_weights=True)
FLAGS = dict(a="--packed_weights", b="--packed_weights --packed_head_requests", c="--head_requests")
protos = {leg: Predictor(f"fw -i {path} -t {flags}") for leg, flags in FLAGS.items()}
mi_k, _, rp = P.new_regressor_from_filename(path, immutable=True, packed=True, packed_head=True)  # the launches-only legs
_, _, rf = P.new_regressor_from_filename(path, immutable=True)
shutil.rmtree(tmp)
prs = {leg: [proto] + [proto.clone_lite() for _ in range(RMAX - 1)] for leg, proto in protos.items()}
ctxs = [context() for _ in range(RMAX)]
lines = [[candidate() for _ in range(CMAX)] for _ in range(RMAX)]
for leg in prs:
    for pr, ctx in zip(prs[leg], ctxs):
        assert pr.setup_cache(ctx + "\n") == 0.0
print(f"3 x {RMAX} predictors ready; contexts of {np.mean([len(c.split()) - NCTX for c in ctxs]):.0f} features, candidates of "
      f"{np.mean([len(l.split()) - l.count('|') for r in lines for l in r]):.1f}", flush=True)
NAMES = dict(a="a_packed_whole_lines_per_request", b="b_packed_head_requests_one_call", c="c_f32_head_requests_one_call")


def point(R, C):
    n = R * C
    arrs = [Predictor.encode_batch(l[:C]) for l in lines[:R]]  # what a C caller holds
    legs = {NAMES["a"]: lambda: [prs["a"][r].predict_batch(arrs[r], with_cache=True) for r in range(R)],
            NAMES["b"]: lambda: serving.predict_requests(prs["b"][:R], arrs),
            NAMES["c"]: lambda: serving.predict_requests(prs["c"][:R], arrs)}
    first = {name: np.concatenate(fn()) for name, fn in legs.items()}  # (also the warm-up of this shape)
    assert all((p > 0).all() for p in first.values())
    for fn in legs.values():
        fn()
    ts = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, fn in legs.items():
            ts[name].append(clock(fn))
    row = dict(requests=R, candidates_per_request=C, candidates=n, **{name: stats(t, n) for name, t in ts.items()})
    row["max_abs_difference_b_a"] = float(np.abs(first[NAMES["b"]] - first[NAMES["a"]]).max())
    row["max_abs_difference_b_c"] = float(np.abs(first[NAMES["b"]] - first[NAMES["c"]]).max())
    row["a_ms_over_b_ms"] = row[NAMES["a"]]["ms_median"] / row[NAMES["b"]]["ms_median"]
    row["c_ms_over_b_ms"] = row[NAMES["c"]]["ms_median"] / row[NAMES["b"]]["ms_median"]
    print(f"R = {R:3d} x C = {C:3d}: (a) {fmt(row[NAMES['a']])}  (b) {fmt(row[NAMES['b']])}  (c) {fmt(row[NAMES['c']])}  a / b = {row['a_ms_over_b_ms']:.2f}  "
          f"c / b = {row['c_ms_over_b_ms']:.2f}  max |b - a| {row['max_abs_difference_b_a']:.2e}  max |b - c| {row['max_abs_difference_b_c']:.2e}", flush=True)
    return row


rows = [point(R, C) for R in RS for C in CS]

# ---- the launches alone: KR x KC candidates
rp.enable_packed_head_requests()
rf.enable_head_requests()
host = VowpalParser(vw)
fbt = fw.FeatureBufferTranslator(mi_k)
ctx_fbs = [fbt.translate(host.next_vowpal((ctx + "\n").encode())) for ctx in ctxs[:KR]]
whole = [[fbt.translate(host.next_vowpal((ctxs[r] + t).encode())) for t in lines[r][:KC]] for r in range(KR)]
which = np.repeat(np.arange(KR, dtype=np.uint32), KC)
closing, sets = [], {}
for name, rk in (("packed", rp), ("f32", rf)):
    caches = [rk.setup_cache(fb) for fb in ctx_fbs]
    own = [fw.FeatureBuffer(label=0.0, example_importance=1.0, example_number=0, lr_buffer=fb.lr_buffer.copy(), ffm_buffer=caches[r].filter(fb.ffm_buffer))
           for r in range(KR) for fb in whole[r]]
    eb = rk.batch(own)
    eb.set_caches(caches, which)
    sets[name] = (rk, eb)
    closing += [eb] + caches
wb = rp.batch([fb for fbs in whole for fb in fbs])
closing.insert(0, wb)


def whole_lines():
    rp.learn_batch(wb, capi.MODE_HOGWILD, False)
    wb.predictions()


timed = {"packed_rows_4": lambda: sets["packed"][0].debug_requests_time(sets["packed"][1], 4, KREPS) * 1e-3,
         "packed_rows_8": lambda: sets["packed"][0].debug_requests_time(sets["packed"][1], 8, KREPS) * 1e-3,
         "f32": lambda: sets["f32"][0].debug_requests_time(sets["f32"][1], 0, KREPS) * 1e-3,
         "packed_whole_lines_one_launch": lambda: clock(whole_lines)}
for fn in timed.values():
    fn()
ts = {name: [] for name in timed}
for _ in range(args.rounds):
    for name, fn in timed.items():
        ts[name].append(fn())
rp.learn_batch(sets["packed"][1], capi.MODE_HOGWILD, False)
kernels = dict(requests=KR, candidates_per_request=KC, launches_per_timing=KREPS, packed_head_requests_launch=rp.last_launch(),
               **{name: stats(t, KR * KC) for name, t in ts.items()})
print(f"launches alone, {KR} x {KC} candidates: " + ", ".join(f"{name} {fmt(kernels[name])}" for name in timed), flush=True)
for o in closing:
    o.close()
host.close()

out = dict(what="the requests route on a deep-head model served from packed FFM weights: (a) --packed_weights predictors, one predict_batch(with_cache = 1) "
                "call per request, whole context + candidate lines; (b) one predict_requests call on --packed_weights --packed_head_requests predictors; "
                "(c) one predict_requests call on f32 --head_requests predictors; one quantised file, legs alternating in one process.  kernels: the "
                "launches alone at the C ABI on pre-built entry batches by device events (the whole-line launch by a host clock)",
           geometry=dict(fields=F, k=K, bits=args.bits, hidden=[WIDTH, WIDTH], context_namespaces=NCTX), rounds=args.rounds,
           serving_threads=int(os.environ["FWGPU_SERVING_THREADS"]), kernels=kernels, points=rows)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
for leg in prs.values():
    for pr in leg:
        pr.close()
rp.close()
rf.close()
