"""The two step rules of the mini-batched deep head (fwgpu_head_set_step_rule) side by side, in one process.
  step time   config E's head (X = 496, two hidden layers of 256 ReLU units, topology one: 193 777 dense weights), AdagradLUT, n in {256, 1024, 4096,
              16 384}: fwgpu_debug_head_step's step_ms (device events around the step's kernels) under the summed rule -- dW GEMMs, column sums,
              head_apply_kernel -- and under the per-example rule (csrc/head_seq.hip) with 16-row and 32-row weight tiles (fwgpu_debug_set_option 16).
              The legs alternate, every leg from the same tables; medians of ROUNDS with min - max.  The per-example rule has 2 n x 194 k dependent
              steps to do where the summed rule has one product: there is no speed bar, the table says SLOWER where it is.
  stream      shape b of tests/head_ref.py (30 fields, k = 8, 64 x 64 ReLU) with small tables (2^18 LR entries, 2^24 FFM floats; learning rate 0.025, power_t 0.38; dense head 0.02, 0.45,
              accumulators from 1) over a synthetic stream through
              fwgpu_learn_batch_sync (MODE_SEQUENTIAL) at micro-batch 1024 under each rule: the progressive log loss (every example scored before the
              batch it belongs to is learned) beside the oracle's sequential learner on the same stream.  Reported, not gated.
Writes profiles/head_step_rule.json.     usage: python3 scripts/bench_head_step_rule.py [--rounds 5] [--examples 204800] [--out FILE]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import fwumious_wabbit_amd as fw
import head_ref as hr
from fwumious_wabbit_amd import _capi as capi
from helpers import logloss, make_pair, record_labels
from oracle import fwo

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--examples", type=int, default=204800)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_step_rule.json"))
args = ap.parse_args()
SIZES, MB = [256, 1024, 4096, 16384], 1024
LEGS = dict(summed=(capi.HEAD_STEP_SUMMED, -1), per_example_16_rows=(capi.HEAD_STEP_PER_EXAMPLE, 16), per_example_32_rows=(capi.HEAD_STEP_PER_EXAMPLE, 32))


def stats(ms):
    ms = np.asarray(ms)
    return dict(ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()))


def fmt(s):
    return f"{s['ms_median']:.3f} ms ({s['ms_min']:.3f} - {s['ms_max']:.3f})"


# ---- step time at config E's head
mi, _, _, _ = hr.build_shape("c")
mi.nn_init_acc_gradient = 1.0
re = fw.Regressor(mi)
total = re.table_len(capi.TABLE_NN_W)
X = hr.shape_of("c")[0]
rng = np.random.default_rng(3)
w0, acc0 = re.table_read(capi.TABLE_NN_W), (1.0 + rng.random(total)).astype(np.float32)
time_rows = []
for n in SIZES:
    x = rng.standard_normal((n, X)).astype(np.float32)
    yi = np.stack([rng.integers(0, 2, n), np.ones(n)], axis=1).astype(np.float32)

    def step(rule, rows):
        re.table_write(capi.TABLE_NN_W, w0)
        re.table_write(capi.TABLE_NN_ACC, acc0)
        re.set_head_step_rule(rule)
        re.set_head_step_tile(rows)
        return re.debug_head_step(x, yi, update=True)["ms"]

    for leg in LEGS.values():  # warm-up: the scratch buffers grow on the first step of a size
        step(*leg)
    ms = {name: [] for name in LEGS}
    for _ in range(args.rounds):
        for name, leg in LEGS.items():
            ms[name].append(step(*leg))
    row = dict(n=n, **{name: stats(v) for name, v in ms.items()})
    for name in ("per_example_16_rows", "per_example_32_rows"):
        row[name]["against_summed"] = "SLOWER" if row[name]["ms_median"] > row["summed"]["ms_median"] else "not slower"
        row[name]["ratio_to_summed"] = row[name]["ms_median"] / row["summed"]["ms_median"]
    time_rows.append(row)
    print(f"n = {n:5d}: summed {fmt(row['summed'])}   per example, 16 rows {fmt(row['per_example_16_rows'])} {row['per_example_16_rows']['against_summed']}"
          f"   32 rows {fmt(row['per_example_32_rows'])} {row['per_example_32_rows']['against_summed']}", flush=True)
re.close()

# ---- one stream under each rule, beside the oracle's sequential learner
shape = hr.SHAPES["b"]
layers = [(w, a, "hu") for w, a in shape["layers"]]
mi, ocfg, ots = make_pair(shape["F"], shape["k"], 18, 24,fw.Optimizer.AdagradLUT, lr=0.025, ffm_lr=0.025, power_t=0.38, ffm_power_t=0.38)
mi.nn_layers = [dict(width=w, activation=a, init=i) for w, a, i in layers]
mi.nn_topology, mi.nn_init_acc_gradient = shape["topo"], 1.0
nn = fwo.make_nn_config(layers, shape["topo"], mi.nn_learning_rate, mi.nn_power_t, mi.nn_init_acc_gradient)
recs, off = hr.stream("b", args.examples, 11)
y = record_labels(recs, off)
om = fwo.Model(ocfg, nn=nn)
w_start = np.concatenate([om.nn_weights(l).copy() for l in range(3)])
_, p_oracle = om.run_stream(ots, recs, off)
curves = dict(oracle_sequential=p_oracle)
for name, rule in (("summed", capi.HEAD_STEP_SUMMED), ("per_example", capi.HEAD_STEP_PER_EXAMPLE)):
    re = fw.Regressor(mi)
    re.table_write(capi.TABLE_NN_W, w_start)
    re.set_head_step_rule(rule)
    fbt, sp, preds = fw.FeatureBufferTranslator(mi), re.split_buffers(MB, 1024), []
    for s0 in range(0, args.examples, MB):
        e0 = min(args.examples, s0 + MB)
        b = re.record_batch(fbt, recs[int(off[s0]):int(off[e0])], off[s0:e0 + 1] - off[s0])
        re.learn_batch_sync(b, sp, capi.MODE_SEQUENTIAL)
        preds.append(b.predictions())
        b.close()
    curves[name] = np.concatenate(preds)
    sp.close()
    re.close()
half = args.examples // 2
stream_rows = {name: dict(progressive_logloss=float(logloss(p, y).mean()), second_half=float(logloss(p[half:], y[half:]).mean())) for name, p in curves.items()}
for name, r in stream_rows.items():
    print(f"{name:18s} progressive log loss {r['progressive_logloss']:.5f}   second half {r['second_half']:.5f}", flush=True)

out = dict(what="the mini-batched head's step rules: fwgpu_debug_head_step's step_ms at config E's head under the summed rule and under the per-example rule "
                "(head_seq.hip) with 16-row and 32-row weight tiles, legs alternating in one process; one stream through fwgpu_learn_batch_sync at "
                "micro-batch 1024 under each rule beside the oracle's sequential learner",
           geometry=dict(X=X, hidden=[256, 256], topology="one", dense_weights=int(total), optimizer="AdagradLUT"), rounds=args.rounds, step_time=time_rows,
           stream=dict(shape="b", examples=args.examples, micro_batch=MB, mode="MODE_SEQUENTIAL", **stream_rows))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
