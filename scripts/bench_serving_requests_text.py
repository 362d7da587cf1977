"""Candidates of SEVERAL requests scored from their TEXT on the device (fwgpu_predictor_predict_requests_text: device parser, csrc/requests_text.hip,
one launch of the requests kernels) against the host-translated route (fwgpu_predictor_predict_requests) on the same lines in the same run.  The
geometry, contexts (about 150 features over 20 namespaces) and candidates (5 - 20 features in the other 10) of scripts/bench_serving_requests.py; an
f32 model and the same model quantised, on --packed_weights --packed_context_cache predictors.  Grid: R in {1, 16, 64, 256} requests x C in
{16, 64, 256} candidates; legs alternating, every shape warmed up first, medians of ROUNDS with min - max, a host clock around calls that end in a
synchronise; the two legs' predictions must be equal bit for bit and the text leg must not have fallen back.  No ratio is fixed in advance.
The new kernels alone, at 16 x 256 on the f32 model: a child process of this script with FWGPU_SERVING_TIMING=1, under which the call puts device events
around its count + scan and emit launches and prints the two times to stderr; medians of ROUNDS calls after the warm-up.
Writes profiles/serving_requests_text.json.     usage: python3 scripts/bench_serving_requests_text.py [--rounds 5] [--small] [--bits 28] [--out FILE]"""
import argparse, json, os, re as regex, shutil, subprocess, sys, tempfile, time
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
ap.add_argument("--small", action="store_true", help="R <= 16, C <= 64")
ap.add_argument("--bits", type=int, default=28)
ap.add_argument("--kernels-child", action="store_true", help="(internal) 16 x 256 on the f32 model only, ROUNDS timed calls: the parent reads the kernels' times from stderr")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "serving_requests_text.json"))
args = ap.parse_args()

F, K, NCTX = 30, 8, 20
RS, CS = ([1, 16], [16, 64]) if args.small else ([1, 16, 64, 256], [16, 64, 256])
if args.kernels_child:
    RS, CS = [16], [256]
RMAX, CMAX = max(RS), max(CS)
vw = VwNamespaceMap("".join(f"N{i:02d},ns{i}\n" for i in range(F)))
rng = np.random.default_rng(1)


def feature():
    return f"f{rng.zipf(1.3) % 100000}"


def context():
    return " ".join(f"|N{i:02d} " + " ".join(feature() for _ in range(1 + rng.poisson(6.5))) for i in range(NCTX)) + " "


def candidate():
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
whole, quantised = os.path.join(tmp, "m.fw"), os.path.join(tmp, "q.fw")
P.save_regressor_to_filename(whole, mi, vw, re)
re.close()
P.convert_inference_regressor(whole, quantised, quantize_weights=True)
ctxs = [context() for _ in range(RMAX)]
lines = [[candidate() for _ in range(CMAX)] for _ in range(RMAX)]
models = {}
for name, command in (("f32", f"fw -i {whole} -t"), ("packed", f"fw -i {quantised} -t --packed_weights --packed_context_cache"))[: 1 if args.kernels_child else 2]:
    proto = Predictor(command)
    models[name] = [proto] + [proto.clone_lite() for _ in range(RMAX - 1)]
    for pr, ctx in zip(models[name], ctxs):
        assert pr.setup_cache(ctx + "\n") == 0.0
shutil.rmtree(tmp)
print(f"{len(models)} models x {RMAX} predictors ready", flush=True)


def point(name, R, C):
    prs, n = models[name][:R], R * C
    arrs = [Predictor.encode_batch(lines[r][:C]) for r in range(R)]  # what a C caller of the host route holds
    texts = ["".join(lines[r][:C]).encode() for r in range(R)]       # ... and of the text route
    caps = [C] * R
    host = lambda: serving.predict_requests(prs, arrs)
    text = lambda: serving.predict_requests_text(prs, texts, caps)
    a, t = np.concatenate(host()), np.concatenate(text())  # (also the warm-up of this shape)
    assert (a > 0).all() and np.array_equal(a.view(np.uint32), t.view(np.uint32)), "the two routes differ"
    assert prs[0].last_text_route() == (n, 0, False), prs[0].last_text_route()
    host(), text()
    t1, t2 = [], []
    for _ in range(args.rounds):
        t1.append(clock(host))
        t2.append(clock(text))
    row = dict(model=name, requests=R, candidates_per_request=C, candidates=n, bit_equal=True, predict_requests=stats(t1, n), predict_requests_text=stats(t2, n))
    row["host_route_ms_over_text_route_ms"] = row["predict_requests"]["ms_median"] / row["predict_requests_text"]["ms_median"]
    print(f"{name:6s} R = {R:3d} x C = {C:3d}: predict_requests {fmt(row['predict_requests'])}, predict_requests_text {fmt(row['predict_requests_text'])} "
          f"= x{row['host_route_ms_over_text_route_ms']:.2f}", flush=True)
    return row


rows = [point(name, R, C) for name in models for R in RS for C in CS]
if args.kernels_child:  # (point() made 2 warm-up and ROUNDS timed text calls: their stderr lines are the result)
    sys.exit(0)
child = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernels-child", "--rounds", str(args.rounds), "--bits", str(args.bits)],
                       env=dict(os.environ, FWGPU_SERVING_TIMING="1"), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600)
found = regex.findall(r"\[predict_requests_text\] 16 requests, 4096 lines: count \+ scan ([0-9.]+) ms, emit ([0-9.]+) ms", child.stderr)
assert child.returncode == 0 and len(found) >= args.rounds, child.stderr[-2000:]
timed = np.array(found[-args.rounds:], dtype=np.float64)
kernels = dict(requests=16, candidates_per_request=256, model="f32", calls=args.rounds,
               count_and_scan_ms=dict(median=float(np.median(timed[:, 0])), min=float(timed[:, 0].min()), max=float(timed[:, 0].max())),
               emit_ms=dict(median=float(np.median(timed[:, 1])), min=float(timed[:, 1].min()), max=float(timed[:, 1].max())))
print(f"kernels alone at 16 x 256 (device events): count + scan {kernels['count_and_scan_ms']['median']:.4f} ms "
      f"({kernels['count_and_scan_ms']['min']:.4f} - {kernels['count_and_scan_ms']['max']:.4f}), emit {kernels['emit_ms']['median']:.4f} ms "
      f"({kernels['emit_ms']['min']:.4f} - {kernels['emit_ms']['max']:.4f})", flush=True)
out = dict(what="fwgpu_predictor_predict_requests_text (device parser, count / scan / emit kernels of requests_text.hip, one launch of the requests kernels) "
                "against fwgpu_predictor_predict_requests (host worker threads parse, translate and filter) on the same lines, alternating in one process; "
                "bit-equal predictions at every point; ratio > 1: the text route is faster",
           geometry=dict(fields=F, k=K, bits=args.bits, context_namespaces=NCTX), rounds=args.rounds, serving_threads=int(os.environ["FWGPU_SERVING_THREADS"]),
           kernels_alone=kernels, points=rows)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
for prs in models.values():
    for pr in prs:
        pr.close()
