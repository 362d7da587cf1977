"""Candidates of SEVERAL requests in one launch (fwgpu_predictor_predict_requests, fwgpu_batch_set_caches: csrc/requests.hip) against the unchanged
per-request route (one fwgpu_predictor_predict_batch(with_cache = 1) call per request) on the same lines in the same run.  Config C's geometry (30
fields, k = 8, 28-bit tables); every request has its own context of about 150 features over 20 namespaces, its candidates hold 5 - 20 features in the
other 10.  Grid: R in {1, 16, 64, 256} requests x C in {16, 64, 256} candidates, and R = 1, C = 20 000.  Per point
    (1) ONE fwgpu_predictor_predict_requests call,
    (2) R fwgpu_predictor_predict_batch(with_cache = 1) calls, alternating with (1),
    (3) at the C ABI, kernel only, on pre-built entry batches of the filtered buffers: one launch of the batch with a cache per example against R
        launches of per-request batches with fwgpu_batch_set_cache (enqueued back to back, one synchronisation at the end),
every shape warmed up first, medians of ROUNDS with min - max, a host clock around calls that end in a synchronise.  The predictions of (1) and (2)
are compared at every timed size (max |a - b|; the sums are in another order).  No ratio is fixed in advance: the numbers are what they are.
Writes profiles/serving_requests.json.     usage: python3 scripts/bench_serving_requests.py [--rounds 5] [--small] [--out FILE]"""
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
ap.add_argument("--small", action="store_true", help="R <= 16, C <= 64 and no 20 000-candidate request: the run a profiler traces")
ap.add_argument("--bits", type=int, default=28)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "serving_requests.json"))
args = ap.parse_args()

F, K, NCTX = 30, 8, 20
RS, CS, BIG = ([1, 16], [16, 64], 0) if args.small else ([1, 16, 64, 256], [16, 64, 256], 20000)
RMAX, CMAX = max(RS), max(CS)
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


# ---- the model: config C's geometry, a short training pass so that the weights are not the initial ones
mi = fw.ModelInstance(learning_rate=0.025, ffm_learning_rate=0.025, power_t=0.38, ffm_power_t=0.38, bit_precision=args.bits, ffm_k=K,
                      ffm_bit_precision=args.bits, optimizer=fw.Optimizer.AdagradLUT, ffm_init_acc_gradient=1.0,
                      feature_combo_descs=[fw.FeatureComboDesc([fw.NamespaceDescriptor(i)]) for i in range(F)],
                      ffm_fields=[[fw.NamespaceDescriptor(i)] for i in range(F)])
re = fw.Regressor(mi)
fbt = fw.FeatureBufferTranslator(mi)
recs, off = fw.synth_records(F, 5.67, 1.05, 1_000_000, 0.1, 5, 0, 20000)
b = re.record_batch(fbt, recs, off)
re.learn_batch(b, capi.MODE_HOGWILD, True)
b.predictions()
b.close()
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "m.fw")
P.save_regressor_to_filename(path, mi, vw, re)
proto = Predictor(f"fw -i {path} -t")
shutil.rmtree(tmp)
prs = [proto] + [proto.clone_lite() for _ in range(RMAX - 1)]
ctxs = [context() for _ in range(RMAX)]
lines = [[candidate() for _ in range(CMAX)] for _ in range(RMAX)]
for pr, ctx in zip(prs, ctxs):
    assert pr.setup_cache(ctx + "\n") == 0.0
print(f"model and {RMAX} predictors ready; contexts of {np.mean([len(c.split()) - NCTX for c in ctxs]):.0f} features, candidates of "
      f"{np.mean([len(l.split()) - l.count('|') for r in lines for l in r]):.1f}", flush=True)

# ---- (3)'s inputs: the twin regressor's caches and the filtered entry buffers of every line (what the serving calls build per call)
host = VowpalParser(vw)
caches = [re.setup_cache(fbt.translate(host.next_vowpal((ctx + "\n").encode()))) for ctx in ctxs]
RK = RMAX


def entries(r, text):
    fb = fbt.translate(host.next_vowpal((ctxs[r] + text).encode()))
    return fw.FeatureBuffer(label=0.0, example_importance=1.0, example_number=0, lr_buffer=fb.lr_buffer.copy(), ffm_buffer=caches[r].filter(fb.ffm_buffer))


fbs = [[entries(r, t) for t in lines[r]] for r in range(RK)]
print("entry buffers ready", flush=True)


def point(R, C, req_lines, kernel_only):
    n = R * C
    arrs = [Predictor.encode_batch(l) for l in req_lines]  # what a C caller holds
    one = lambda: serving.predict_requests(prs[:R], arrs)
    per = lambda: [prs[r].predict_batch(arrs[r], with_cache=True) for r in range(R)]
    a, bb = np.concatenate(one()), np.concatenate(per())  # (also the warm-up of this shape)
    assert (a > 0).all() and (bb > 0).all()
    one(), per()
    t1, t2 = [], []
    for _ in range(args.rounds):
        t1.append(clock(one))
        t2.append(clock(per))
    row = dict(requests=R, candidates_per_request=C, candidates=n, max_abs_difference=float(np.abs(a - bb).max()),
               predict_requests=stats(t1, n), predict_batch_per_request=stats(t2, n), launches=dict(predict_requests="1 (+ the base kernel)", predict_batch_per_request=R))
    row["per_request_ms_over_requests_ms"] = row["predict_batch_per_request"]["ms_median"] / row["predict_requests"]["ms_median"]
    msg = f"R = {R:3d} x C = {C:5d}: predict_requests {fmt(row['predict_requests'])}, {R} x predict_batch {fmt(row['predict_batch_per_request'])} = x{row['per_request_ms_over_requests_ms']:.2f}, max |d| = {row['max_abs_difference']:.2e}"
    if kernel_only:
        shared = re.batch([fb for r in range(R) for fb in fbs[r][:C]])
        shared.set_caches(caches[:R], np.repeat(np.arange(R, dtype=np.uint32), C))
        singles = [re.batch(fbs[r][:C]) for r in range(R)]
        for r in range(R):
            singles[r].set_cache(caches[r])

        def k1():
            re.learn_batch(shared, capi.MODE_HOGWILD, False)
            shared.predictions()

        def k2():
            for s in singles:
                re.learn_batch(s, capi.MODE_HOGWILD, False)
            singles[-1].predictions()  # (the launches share the null stream: this waits for all of them)

        k1(), k2()
        pa = shared.predictions()
        pb = np.concatenate([s.predictions() for s in singles])
        u1, u2 = [], []
        for _ in range(args.rounds):
            u1.append(clock(k1))
            u2.append(clock(k2))
        row["kernel_only"] = dict(set_caches_one_launch=stats(u1, n), set_cache_launch_per_request=stats(u2, n), max_abs_difference=float(np.abs(pa - pb).max()),
                                  launch=re.last_launch())
        row["kernel_only"]["per_request_ms_over_one_launch_ms"] = row["kernel_only"]["set_cache_launch_per_request"]["ms_median"] / row["kernel_only"]["set_caches_one_launch"]["ms_median"]
        msg += f"; launches only: {fmt(row['kernel_only']['set_caches_one_launch'])} against {fmt(row['kernel_only']['set_cache_launch_per_request'])} = x{row['kernel_only']['per_request_ms_over_one_launch_ms']:.2f}"
        shared.close()
        for s in singles:
            s.close()
    print(msg, flush=True)
    return row


rows = [point(R, C, [lines[r][:C] for r in range(R)], R <= RK) for R in RS for C in CS]
if BIG:
    rows.append(point(1, BIG, [[candidate() for _ in range(BIG)]], False))
out = dict(what="candidates of several requests in one launch (fwgpu_predictor_predict_requests) against one fwgpu_predictor_predict_batch(with_cache = 1) call per "
                "request on the same lines, alternating in one process; kernel_only: one launch of an entry batch with a cache per example (fwgpu_batch_set_caches) "
                "against one launch per request of entry batches with fwgpu_batch_set_cache; ratio > 1: the one launch is faster",
           geometry=dict(fields=F, k=K, bits=args.bits, context_namespaces=NCTX), rounds=args.rounds, serving_threads=int(os.environ["FWGPU_SERVING_THREADS"]),
           kernel_only_up_to_requests=RK, points=rows)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
for c in caches:
    c.close()
for pr in prs:
    pr.close()
host.close()
re.close()
