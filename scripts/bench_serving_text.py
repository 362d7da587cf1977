"""A request's candidates scored from their text on the device (fwgpu_predictor_predict_text) against the unchanged host-parsed route
(fwgpu_predictor_predict_batch, with_cache) on the same lines: one context over 20 of 30 namespaces + N candidates over the other 10, at config E's
geometry (30 fields, k = 16) with its 2 x 256 ReLU head and headless, N = 64 / 256 / 1024 / 8192 / 20 000.  Both entry points get what a C caller
holds (one buffer of lines / a char** of the same lines), their predictions are compared bit for bit before anything is timed, and the two alternate
in ONE process, ROUNDS times each after a warm-up; medians with the spread.  FWGPU_SERVING_THREADS=16: the host route's parser threads on 16 cores;
the same host route with ONE parser thread is timed in the same rounds, since predict_text itself parses on no host thread at all.
Writes profiles/serving_text.json.     usage: python3 scripts/bench_serving_text.py [--rounds 9] [--out profiles/serving_text.json]"""
import argparse, json, os, sys, tempfile, time
os.environ.setdefault("FWGPU_SERVING_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import _capi as capi, persistence as P
from fwumious_wabbit_amd.feed import VwNamespaceMap
from fwumious_wabbit_amd.serving import Predictor

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--sizes", type=int, nargs="+", default=[64, 256, 1024, 8192, 20000])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "serving_text.json"))
args = ap.parse_args()
assert args.rounds >= 7

F, K, NCTX, WIDTH = 30, 16, 20, 256
THREADS = os.environ["FWGPU_SERVING_THREADS"]
vw = VwNamespaceMap("".join(f"N{i:02d},ns{i}\n" for i in range(F)))
rng = np.random.default_rng(1)


def ns_text(i):
    n = 1 + rng.poisson(5.67)
    return f"|N{i:02d} " + " ".join(f"f{rng.zipf(1.3) % 100000}" for _ in range(n))


def timed(fn, threads=None):
    if threads is not None:
        os.environ["FWGPU_SERVING_THREADS"] = str(threads)  # (read by every call)
    t0 = time.perf_counter()
    fn()
    dt = time.perf_counter() - t0
    os.environ["FWGPU_SERVING_THREADS"] = THREADS
    return dt


def stats(ts, n):
    ts = np.asarray(ts)
    return dict(candidates_per_s=float(n / np.median(ts)), ms_median=float(np.median(ts) * 1e3), ms_min=float(ts.min() * 1e3), ms_max=float(ts.max() * 1e3))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


ctx = " ".join(ns_text(i) for i in range(NCTX)) + " "
requests = {N: [" ".join(ns_text(i) for i in range(NCTX, F)) + "\n" for _ in range(N)] for N in args.sizes}
recs, off = fw.synth_records(F, 5.67, 1.05, 1_000_000, 0.1, 5, 0, 20000)
geometries = []
for name, head in (("config E head (2 x 256 relu, topology one)", True), ("headless", False)):
    kw = dict(nn_layers=[dict(width=WIDTH, activation="relu", init="hu") for _ in range(2)], nn_topology="one") if head else {}
    mi = fw.ModelInstance(learning_rate=0.025, ffm_learning_rate=0.025, power_t=0.38, ffm_power_t=0.38, bit_precision=24, ffm_k=K,
                          ffm_bit_precision=24, optimizer=fw.Optimizer.AdagradLUT, ffm_init_acc_gradient=1.0,
                          feature_combo_descs=[fw.FeatureComboDesc([fw.NamespaceDescriptor(i)]) for i in range(F)],
                          ffm_fields=[[fw.NamespaceDescriptor(i)] for i in range(F)], **kw)
    re = fw.Regressor(mi)
    b = re.record_batch(fw.FeatureBufferTranslator(mi), recs, off)
    re.learn_batch(b, capi.MODE_HOGWILD, True)
    b.predictions()
    b.close()
    path = os.path.join(tempfile.mkdtemp(), "m.fw")
    P.save_regressor_to_filename(path, mi, vw, re)
    P.convert_inference_regressor(path, path + ".inf")
    re.close()
    pr = Predictor(f"fw -i {path}.inf -t")
    assert pr.setup_cache(ctx + "\n") == 0.0
    rows = []
    for N in args.sizes:
        cands = requests[N]
        text, cands_c = "".join(cands).encode(), pr.encode_batch(cands)  # what a C / Rust caller holds: one buffer, or a char**
        got, want = pr.predict_text(text, with_cache=True), pr.predict_batch(cands_c, with_cache=True)
        lines, host_lines, fell_back = pr.last_text_route()
        assert np.array_equal(bits(got), bits(want)) and (want > 0).all() and (lines, host_lines, fell_back) == (N, 0, False)
        for _ in range(2):  # warm-up: buffers grown, parser threads started
            pr.predict_text(text, with_cache=True)
            pr.predict_batch(cands_c, with_cache=True)
        t_t, t_b, t_1 = [], [], []
        for _ in range(args.rounds):  # alternating: the routes see the same clocks
            t_t.append(timed(lambda: pr.predict_text(text, with_cache=True)))
            t_b.append(timed(lambda: pr.predict_batch(cands_c, with_cache=True)))
            t_1.append(timed(lambda: pr.predict_batch(cands_c, with_cache=True), threads=1))
        row = dict(candidates=N, text_bytes=len(text), context_features=len(ctx.split()) - NCTX, host_lines=host_lines, bit_equal=True,
                   predict_text=stats(t_t, N), predict_batch=stats(t_b, N), predict_batch_one_thread=stats(t_1, N))
        row["predict_batch_ms_over_predict_text_ms"] = row["predict_batch"]["ms_median"] / row["predict_text"]["ms_median"]
        row["predict_batch_one_thread_ms_over_predict_text_ms"] = row["predict_batch_one_thread"]["ms_median"] / row["predict_text"]["ms_median"]
        rows.append(row)
        print(f"{name}: N = {N:5d}: predict_text {row['predict_text']['ms_median']:.3f} ms ({row['predict_text']['ms_min']:.3f} .. {row['predict_text']['ms_max']:.3f}), "
              f"predict_batch {row['predict_batch']['ms_median']:.3f} ms ({row['predict_batch']['ms_min']:.3f} .. {row['predict_batch']['ms_max']:.3f}) "
              f"= x{row['predict_batch_ms_over_predict_text_ms']:.2f}; predict_batch on one thread {row['predict_batch_one_thread']['ms_median']:.3f} ms "
              f"= x{row['predict_batch_one_thread_ms_over_predict_text_ms']:.2f}", flush=True)
    pr.close()
    geometries.append(dict(model=name, requests=rows))
out = dict(what="serving from text: fwgpu_predictor_predict_text (device parser, records never on the host) against fwgpu_predictor_predict_batch "
                "(with_cache, host parser threads) on the same lines, alternating in one process; ratio > 1: predict_text is faster",
           geometry=dict(fields=F, k=K, context_namespaces=NCTX, bits=24), rounds=args.rounds, serving_threads=int(os.environ["FWGPU_SERVING_THREADS"]),
           models=geometries)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
