"""The deep head's predict-only forward in one launch (fwgpu_enable_fused_head, csrc/head_fused.hip) against the routes it replaces, in the same run.
Config E's head: X = 496, two hidden layers of 256 ReLU units, topology one (30 fields, k = 16).
  head alone   n in {16, 64, 256, 1024, 4096, 32768}: the head over inputs already on the device (fwgpu_debug_head_forward_time, device events over REPS
               passes after a warm-up pass): leg one head_step(update = false) -- a GEMM launch per layer + head_final_kernel --, leg two the fused kernel;
               the largest |p_fused - p_gemm|.
  small batch  n in {16, 64}: a whole predict-only launch of an entry batch (host clock around REPS launches and one read-back), switch off -- the
               per-example forward inside the fused example kernel, the route such a batch takes today -- against switch on.
  serving      one fwgpu_predictor_predict_requests call at 16 x 16, 16 x 256 and 64 x 64 (requests x candidates) on --head_requests predictors, without
               and with --fused_head (the setup of scripts/bench_serving_head_requests.py; host clock around a call that ends in a synchronise).
The legs of a point alternate in one process; medians of ROUNDS with min - max.  N_fused (launch.cpp kHeadFusedMaxN) is the largest n of `head alone` at which
the fused leg's slowest run is below the GEMM leg's fastest; the script prints it.  No ratio is fixed in advance.
Writes profiles/head_fused.json.     usage: python3 scripts/bench_head_fused.py [--rounds 5] [--bits 22] [--out FILE]"""
import argparse, json, os, shutil, sys, tempfile, time
os.environ.setdefault("FWGPU_SERVING_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import _capi as capi, persistence as P, serving
from fwumious_wabbit_amd.feed import VwNamespaceMap
from fwumious_wabbit_amd.serving import Predictor

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--bits", type=int, default=22)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_fused.json"))
args = ap.parse_args()

F, K, NCTX, WIDTH = 30, 16, 20, 256
SIZES = [16, 64, 256, 1024, 4096, 32768]
POINTS = [(16, 16), (16, 256), (64, 64)]
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


def stats(ms):
    ms = np.asarray(ms)
    return dict(ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()))


def fmt(s):
    return f"{s['ms_median']:.4f} ms ({s['ms_min']:.4f} - {s['ms_max']:.4f})"


def alternate(legs):
    """{name: stats} of callables that return milliseconds, each warmed up once, then ROUNDS rounds with the legs taking turns"""
    for fn in legs.values():
        fn()
    ms = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, fn in legs.items():
            ms[name].append(fn())
    return {name: stats(v) for name, v in ms.items()}


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
protos = dict(gemm_route=Predictor(f"fw -i {path} -t --head_requests"), fused_head=Predictor(f"fw -i {path} -t --head_requests --fused_head"))
mi_k, _, r_off = P.new_regressor_from_filename(path, immutable=True)  # the switch is one-way: a regressor for each side
_, _, r_on = P.new_regressor_from_filename(path, immutable=True)
shutil.rmtree(tmp)
r_on.enable_fused_head()
fbt = fw.FeatureBufferTranslator(mi_k)
precs, poff = fw.synth_records(F, 5.67, 1.05, 1_000_000, 0.1, 9, 50000, max(SIZES))

# ---- the head alone, over the x of 32 768 examples that one predict launch leaves on the device
big = r_on.record_batch(fbt, precs, poff)
r_on.learn_batch(big, capi.MODE_HOGWILD, False)
big.predictions()
assert r_on.last_route() == capi.ROUTE_HEAD_BATCHED
head_rows = []
for n in SIZES:
    reps = 200 if n <= 4096 else 40
    p_g, p_f = r_on.debug_head_forward_time(n, False, 1)[1], r_on.debug_head_forward_time(n, True, 1)[1]
    row = dict(n=n, passes_per_timing=reps, max_abs_difference=float(np.abs(p_g - p_f).max()),
               **alternate(dict(gemm_route=lambda: r_on.debug_head_forward_time(n, False, reps)[0], fused=lambda: r_on.debug_head_forward_time(n, True, reps)[0])))
    row["fused_slowest_below_gemm_fastest"] = row["fused"]["ms_max"] < row["gemm_route"]["ms_min"]
    head_rows.append(row)
    print(f"head alone, n = {n:5d}: GEMM route {fmt(row['gemm_route'])}  fused {fmt(row['fused'])}  max |d| {row['max_abs_difference']:.2e}", flush=True)
big.close()
wins = [r["n"] for r in head_rows if r["fused_slowest_below_gemm_fastest"]]
n_fused = max(wins) if wins else 0
print(f"N_fused = {n_fused} (0: the fused leg wins at no measured size)", flush=True)

# ---- a whole predict-only launch of a small entry batch: the per-example forward (switch off) against the batched route with the fused head (switch on)
small_rows = []
for n in (16, 64):
    reps = 50
    bs = {name: r.batch_from_records(fbt, precs[:int(poff[n])], poff[:n + 1]) for name, r in (("per_example_forward", r_off), ("fused_head", r_on))}

    def launches(name, r):
        t0 = time.perf_counter()
        for _ in range(reps):
            r.learn_batch(bs[name], capi.MODE_HOGWILD, False)
        bs[name].predictions()
        return (time.perf_counter() - t0) * 1e3 / reps

    row = dict(n=n, launches_per_timing=reps, **alternate(dict(per_example_forward=lambda: launches("per_example_forward", r_off),
                                                                 fused_head=lambda: launches("fused_head", r_on))))
    row["routes"] = dict(per_example_forward=r_off.last_route(), fused_head=r_on.last_route())
    row["max_abs_difference"] = float(np.abs(bs["per_example_forward"].predictions() - bs["fused_head"].predictions()).max())
    assert row["routes"] == dict(per_example_forward=capi.ROUTE_FUSED, fused_head=capi.ROUTE_HEAD_BATCHED), row["routes"]
    small_rows.append(row)
    print(f"whole launch, n = {n}: per-example forward {fmt(row['per_example_forward'])}  fused head {fmt(row['fused_head'])}  "
          f"max |d| {row['max_abs_difference']:.2e}", flush=True)
    for o in bs.values():
        o.close()

# ---- serving: one predict_requests call, without and with --fused_head
RMAX, CMAX = max(R for R, _ in POINTS), max(C for _, C in POINTS)
ctxs = [context() for _ in range(RMAX)]
lines = [[candidate() for _ in range(CMAX)] for _ in range(RMAX)]
prs = {name: [proto] + [proto.clone_lite() for _ in range(RMAX - 1)] for name, proto in protos.items()}
for group in prs.values():
    for pr, ctx in zip(group, ctxs):
        assert pr.setup_cache(ctx + "\n") == 0.0
serving_rows = []
for R, C in POINTS:
    arrs = [Predictor.encode_batch(l[:C]) for l in lines[:R]]
    first = {name: np.concatenate(serving.predict_requests(group[:R], arrs)) for name, group in prs.items()}

    def call(name):
        t0 = time.perf_counter()
        serving.predict_requests(prs[name][:R], arrs)
        return (time.perf_counter() - t0) * 1e3

    row = dict(requests=R, candidates_per_request=C, **alternate({name: (lambda name=name: call(name)) for name in prs}))
    row["max_abs_difference"] = float(np.abs(first["gemm_route"] - first["fused_head"]).max())
    serving_rows.append(row)
    print(f"predict_requests {R:2d} x {C:3d}: GEMM route {fmt(row['gemm_route'])}  --fused_head {fmt(row['fused_head'])}  "
          f"max |d| {row['max_abs_difference']:.2e}", flush=True)

out = dict(what="the deep head's predict-only forward: head_forward_fused_kernel (one launch, a workgroup per 32 examples) against head_step(update = false) "
                "(a GEMM launch per layer + the final kernel) over the same device-resident inputs, by device events; whole predict-only launches of small "
                "entry batches against the per-example forward; one predict_requests call without and with --fused_head.  Legs alternate in one process.",
           geometry=dict(fields=F, k=K, bits=args.bits, X=F + F * (F + 1) // 2, hidden=[WIDTH, WIDTH], topology="one"), rounds=args.rounds,
           n_fused=n_fused, head_alone=head_rows, small_batches=small_rows, predict_requests=serving_rows)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
for group in prs.values():
    for pr in group:
        pr.close()
r_on.close()
r_off.close()
