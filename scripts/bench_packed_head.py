"""A deep-head model served from packed FFM weights (fwgpu_model_load_packed_head, csrc/head_packed.hip, FWGPU_ROUTE_PACKED_HEAD) against the f32 load of the
same quantised inference file, in the same run.  Config E's geometry: 30 fields, k = 16, two hidden layers of 256 ReLU units, topology one.
  predict-only entry batches of 64, 1024, 16 384 and 131 072 records of the synthetic stream (about 200 FFM entries a record), MODE_HOGWILD:
    call     host clock around one fwgpu_learn_batch and the read-back of its predictions
    kernels  device events around the launches of that call on the null stream: the head-input kernel and the layers
  leg f32: whichever route the f32 regressor takes (the fused example kernel per example below 256 records, the v2 example kernel's emit_x and the
  layers' GEMMs from there); leg packed: packed_head_inputs_kernel and the same layers.  The two legs alternate in one process; medians of ROUNDS with
  min - max; the bytes of ffm_storage() for both loads; the largest |p_packed - p_f32| per size.  No ratio is fixed in advance.
Writes profiles/packed_head.json.     usage: python3 scripts/bench_packed_head.py [--rounds 5] [--bits 22] [--out FILE]"""
import argparse, json, os, shutil, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import _capi as capi, persistence as P
from fwumious_wabbit_amd.feed import VwNamespaceMap

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--bits", type=int, default=22)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_head.json"))
args = ap.parse_args()

F, K, WIDTH = 30, 16, 256
SIZES = [64, 1024, 16384, 131072]
ROUTES = {capi.ROUTE_FUSED: "fused example kernel, head per example", capi.ROUTE_HEAD_BATCHED: "v2 example kernel emit_x + layers",
          capi.ROUTE_PACKED_HEAD: "packed_head_inputs_kernel + layers"}


def stats(ms):
    ms = np.asarray(ms)
    return dict(ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()))


def fmt(s):
    return f"{s['ms_median']:.4f} ms ({s['ms_min']:.4f} - {s['ms_max']:.4f})"


mi = fw.ModelInstance(learning_rate=0.025, ffm_learning_rate=0.025, power_t=0.38, ffm_power_t=0.38, bit_precision=args.bits, ffm_k=K,
                      ffm_bit_precision=args.bits, optimizer=fw.Optimizer.AdagradLUT, ffm_init_acc_gradient=1.0,
                      feature_combo_descs=[fw.FeatureComboDesc([fw.NamespaceDescriptor(i)]) for i in range(F)],
                      ffm_fields=[[fw.NamespaceDescriptor(i)] for i in range(F)])
mi.nn_layers = [dict(width=WIDTH, activation="relu", init="hu"), dict(width=WIDTH, activation="relu", init="hu")]
mi.nn_topology = "one"
re = fw.Regressor(mi)
recs, off = fw.synth_records(F, 5.67, 1.05, 1_000_000, 0.1, 5, 0, 20000)
b = re.record_batch(fw.FeatureBufferTranslator(mi), recs, off)
re.learn_batch(b, capi.MODE_HOGWILD, True)  # a short training pass: the weights are not the initial ones
b.close()
tmp = tempfile.mkdtemp()
t, q = os.path.join(tmp, "t.fw"), os.path.join(tmp, "q.fw")
P.save_regressor_to_filename(t, mi, VwNamespaceMap("".join(f"N{i:02d},ns{i}\n" for i in range(F))), re)
re.close()
P.convert_inference_regressor(t, q, quantize_weights=True)
mi_f, _, rf = P.new_regressor_from_filename(q, immutable=True)
mi_p, _, rp = P.new_regressor_from_filename(q, immutable=True, packed=True, packed_head=True)
shutil.rmtree(tmp)
result = dict(config=dict(fields=F, k=K, layers=[WIDTH, WIDTH], bits=args.bits, rounds=args.rounds),
              ffm_storage_bytes=dict(f32=rf.ffm_storage()[1], packed=rp.ffm_storage()[1]), sizes=[])
print(f"ffm_storage: f32 {rf.ffm_storage()[1]} bytes, packed {rp.ffm_storage()[1]} bytes")
recs, off = fw.synth_records(F, 5.67, 1.05, 1_000_000, 0.1, 77, 100000, max(SIZES))
for n in SIZES:
    sub = recs[:int(off[n])], off[:n + 1]
    legs = {"f32": (rf, rf.batch_from_records(fw.FeatureBufferTranslator(mi_f), *sub)), "packed": (rp, rp.batch_from_records(fw.FeatureBufferTranslator(mi_p), *sub))}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    call, kern, pred, route = {k: [] for k in legs}, {k: [] for k in legs}, {}, {}
    for rnd in range(args.rounds + 1):  # (round 0 warms both legs up and is not counted)
        for name, (r, bt) in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev[0].record()
            r.learn_batch(bt, capi.MODE_HOGWILD, False)
            ev[1].record()
            pred[name] = bt.predictions().copy()
            t1 = time.perf_counter()
            ev[1].synchronize()
            route[name] = r.last_route()
            if rnd:
                call[name].append((t1 - t0) * 1e3)
                kern[name].append(ev[0].elapsed_time(ev[1]))
    row = dict(n=n, max_abs_diff=float(np.abs(pred["f32"] - pred["packed"]).max()),
               legs={name: dict(route=ROUTES.get(route[name], str(route[name])), call=stats(call[name]), kernels=stats(kern[name])) for name in legs})
    result["sizes"].append(row)
    for name in legs:
        print(f"n = {n:6d}  {name:6s} [{row['legs'][name]['route']}]  call {fmt(row['legs'][name]['call'])}  kernels {fmt(row['legs'][name]['kernels'])}")
    print(f"n = {n:6d}  max |p_packed - p_f32| = {row['max_abs_diff']:.3e}")
    for _, bt in legs.values():
        bt.close()
rf.close()
rp.close()
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", args.out)
