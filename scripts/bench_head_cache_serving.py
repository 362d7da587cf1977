"""Serving a deep-head model through the context cache: candidates/s of one request = context (20 of the 30 namespaces) + N candidates (the other 10) at
config E's geometry (30 fields, k = 16, 2 x 256 ReLU head), N = 64 / 256 / 1024 / 8192, through fwgpu_predictor_predict_batch
  (a) uncached: every candidate scored as the whole context + candidate line, and
  (b) cached: fw_setup_cache once, the candidates gather only what they add (256 candidates or more: the batched head route; fewer: the per-example kernel).
The two routes alternate in ONE process, ROUNDS times each; medians with the spread.  The kernels' share: the same request as entry batches on a Regressor
(no text, no parsing, no upload) -- launch + predictions per request, cached and whole -- as a fraction of the text route's time.
Writes profiles/head_cache_serving.json.     usage: python3 scripts/bench_head_cache_serving.py [--rounds 7] [--out profiles/head_cache_serving.json]"""
import argparse, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import _capi as capi, persistence as P
from fwumious_wabbit_amd.feed import VowpalParser, VwNamespaceMap
from fwumious_wabbit_amd.serving import Predictor

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--sizes", type=int, nargs="+", default=[64, 256, 1024, 8192])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_cache_serving.json"))
args = ap.parse_args()
assert args.rounds >= 5

F, K, NCTX, WIDTH = 30, 16, 20, 256
vw = VwNamespaceMap("".join(f"N{i:02d},ns{i}\n" for i in range(F)))
mi = fw.ModelInstance(learning_rate=0.025, ffm_learning_rate=0.025, power_t=0.38, ffm_power_t=0.38, bit_precision=24, ffm_k=K,
                      ffm_bit_precision=24, optimizer=fw.Optimizer.AdagradLUT, ffm_init_acc_gradient=1.0,
                      feature_combo_descs=[fw.FeatureComboDesc([fw.NamespaceDescriptor(i)]) for i in range(F)],
                      ffm_fields=[[fw.NamespaceDescriptor(i)] for i in range(F)],
                      nn_layers=[dict(width=WIDTH, activation="relu", init="hu") for _ in range(2)], nn_topology="one")
re = fw.Regressor(mi)
recs, off = fw.synth_records(F, 5.67, 1.05, 1_000_000, 0.1, 5, 0, 20000)
b = re.record_batch(fw.FeatureBufferTranslator(mi), recs, off)
re.learn_batch(b, capi.MODE_HOGWILD, True)
b.predictions()
b.close()
rng = np.random.default_rng(1)


def ns_text(i):
    n = 1 + rng.poisson(5.67)
    return f"|N{i:02d} " + " ".join(f"f{rng.zipf(1.3) % 100000}" for _ in range(n))


ctx = " ".join(ns_text(i) for i in range(NCTX)) + " "
d = tempfile.mkdtemp()
path = os.path.join(d, "m.fw")
P.save_regressor_to_filename(path, mi, vw, re)
P.convert_inference_regressor(path, path + ".inf")
pr = Predictor(f"fw -i {path}.inf -t")
assert pr.setup_cache(ctx + "\n") == 0.0
parser, fbt = VowpalParser(vw), fw.FeatureBufferTranslator(mi)
cfb = fbt.translate(parser.next_vowpal((ctx + "\n").encode()))
cache = re.setup_cache(cfb)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def stats(ts, n):
    ts = np.asarray(ts)
    return dict(candidates_per_s=float(n / np.median(ts)), ms_median=float(np.median(ts) * 1e3), ms_min=float(ts.min() * 1e3), ms_max=float(ts.max() * 1e3))


rows = []
for N in args.sizes:
    cands = [" ".join(ns_text(i) for i in range(NCTX, F)) + "\n" for _ in range(N)]
    full = [ctx + c for c in cands]
    want, got = pr.predict_batch(full), pr.predict_batch(cands, with_cache=True)
    full_c, cands_c = pr.encode_batch(full), pr.encode_batch(cands)  # the char** of a C / Rust caller (Python's str -> bytes is not the library's time)
    t_u, t_c = [], []
    for _ in range(args.rounds):  # alternating: both routes see the same clocks
        t_u.append(timed(lambda: pr.predict_batch(full_c)))
        t_c.append(timed(lambda: pr.predict_batch(cands_c, with_cache=True)))
    # kernels only: the same request as entry batches (launch + predictions)
    fbs = [fbt.translate(parser.next_vowpal(l.encode())) for l in full]
    cut = [fw.FeatureBuffer(label=0.0, example_importance=1.0, example_number=0, lr_buffer=f.lr_buffer, ffm_buffer=cache.filter(f.ffm_buffer)) for f in fbs]
    bf, bc = re.batch(fbs), re.batch(cut)
    bc.set_cache(cache)
    k_u, k_c, routes = [], [], {}
    for name, bb, ts in (("uncached", bf, k_u), ("cached", bc, k_c)):
        re.learn_batch(bb, capi.MODE_HOGWILD, False)
        bb.predictions()
        routes[name] = re.last_route()
    for _ in range(args.rounds):
        for bb, ts in ((bf, k_u), (bc, k_c)):
            def launches(bb=bb):
                for _ in range(10):
                    re.learn_batch(bb, capi.MODE_HOGWILD, False)
                bb.predictions()
            ts.append(timed(launches) / 10)
    k_diff = float(np.abs(bc.predictions() - bf.predictions()).max())
    bc.set_cache(None)
    bf.close()
    bc.close()
    row = dict(candidates=N, context_features=len(ctx.split()) - NCTX, candidate_features_mean=float(np.mean([len(c.split()) - (F - NCTX) for c in cands])),
               max_abs_cached_minus_uncached=float(np.abs(got - want).max()), kernel_max_abs_cached_minus_uncached=k_diff,
               text_uncached=stats(t_u, N), text_cached=stats(t_c, N), kernels_uncached=stats(k_u, N), kernels_cached=stats(k_c, N),
               kernel_route_uncached=routes["uncached"], kernel_route_cached=routes["cached"])
    row["cached_over_uncached"] = row["text_cached"]["candidates_per_s"] / row["text_uncached"]["candidates_per_s"]
    row["kernels_cached_over_uncached"] = row["kernels_cached"]["candidates_per_s"] / row["kernels_uncached"]["candidates_per_s"]
    row["kernel_share_uncached"] = row["kernels_uncached"]["ms_median"] / row["text_uncached"]["ms_median"]
    row["kernel_share_cached"] = row["kernels_cached"]["ms_median"] / row["text_cached"]["ms_median"]
    rows.append(row)
    print(f"N = {N:5d}: text route uncached {row['text_uncached']['candidates_per_s']:>12,.0f} cand/s ({row['text_uncached']['ms_median']:.3f} ms), cached "
          f"{row['text_cached']['candidates_per_s']:>12,.0f} cand/s ({row['text_cached']['ms_median']:.3f} ms) = x{row['cached_over_uncached']:.2f}; kernels only "
          f"{row['kernels_uncached']['ms_median']:.3f} / {row['kernels_cached']['ms_median']:.3f} ms = x{row['kernels_cached_over_uncached']:.2f}, share of the request "
          f"{row['kernel_share_uncached']:.0%} / {row['kernel_share_cached']:.0%}; max |cached - uncached| {row['max_abs_cached_minus_uncached']:.1e}", flush=True)
out = dict(what="deep-head serving through the context cache: fwgpu_predictor_predict_batch, cached against uncached, alternating in one process",
           geometry=dict(fields=F, k=K, context_namespaces=NCTX, head=f"2 x {WIDTH} relu, topology one", bits=24), rounds=args.rounds,
           route_names={str(v): k for k, v in vars(capi).items() if k.startswith("ROUTE_")}, requests=rows)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
