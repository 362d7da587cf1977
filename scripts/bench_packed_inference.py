"""Predict-only rate of a packed regressor (FFM weights as f16 buckets, fwgpu_model_load_packed) against the f32 load of the SAME model file, in the
same process, at config C's serving shape: 30 fields, k = 8, ffm_bit_precision 28, -b 28, batches of 65 536 records resident on the device,
MODE_HOGWILD, update = 0.  Repeats alternate f32 / packed; every timed region ends in a stream synchronise.  Needs a GPU: no fallback.
usage: python3 scripts/bench_packed_inference.py [--out profiles/packed_inference.json] [--repeats 5] [--launches 20] [--bits 28] [--batch 65536]
       --profile: a short run for `rocprofv3 --kernel-trace --stats -- python3 scripts/bench_packed_inference.py --profile` (no file written)"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fwumious_wabbit_amd as fw  # noqa: E402
from fwumious_wabbit_amd import capi  # noqa: E402
from fwumious_wabbit_amd import persistence as P  # noqa: E402
from fwumious_wabbit_amd.feed import VwNamespaceMap  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_inference.json"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--bits", type=int, default=28)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--profile", action="store_true")
ap.add_argument("--commit", default=None, help="recorded as git_commit where the tree runs without its git metadata")
a = ap.parse_args()
assert a.repeats >= 5 and a.launches >= 20 or a.profile, "at least 5 repeats of at least 20 launches"

F, K = 30, 8
ND = fw.NamespaceDescriptor
mi = fw.ModelInstance(learning_rate=0.1, ffm_learning_rate=0.1, power_t=0.5, ffm_power_t=0.5, bit_precision=a.bits, ffm_k=K,
                      ffm_bit_precision=a.bits, optimizer=fw.Optimizer.SGD, add_constant_feature=True,
                      feature_combo_descs=[fw.FeatureComboDesc([ND(i)]) for i in range(F)], ffm_fields=[[ND(i)] for i in range(F)])
vw = VwNamespaceMap("".join(f"N{i:02d},ns{i}\n" for i in range(F)))
t0 = time.time()
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "model.fw")
    re = fw.Regressor(mi)  # (fails without a GPU)
    # LR weights as a trained model has them (the initial ones are all zero); FFM weights: the reference's own initialisation
    lr = re.table_read(capi.TABLE_LR)
    lr[0::2] = np.random.default_rng(a.seed).normal(0.0, 0.05, lr.size // 2).astype(np.float32)
    re.table_write(capi.TABLE_LR, lr)
    del lr
    P.save_regressor_to_filename(path, mi, vw, re)
    re.close()
    print(f"model file: {os.path.getsize(path) / 2**30:.2f} GiB, {time.time() - t0:.0f} s", flush=True)
    mi_f, _, rf = P.new_regressor_from_filename(path, immutable=True)
    print(f"f32 load done, {time.time() - t0:.0f} s", flush=True)
    mi_p, _, rp = P.new_regressor_from_filename(path, immutable=True, packed=True)
    print(f"packed load done, {time.time() - t0:.0f} s", flush=True)

recs, off = fw.synth_records(F, 5.67, 1.05, 10**7, 0.1, a.seed, 0, a.batch)
fbt = fw.FeatureBufferTranslator(mi_f)
sides = {}
for name, r in (("f32", rf), ("packed", rp)):
    b = r.record_batch(fbt, recs, off)
    st, nb = r.ffm_storage()
    sides[name] = dict(r=r, b=b, storage=st, table_bytes=nb, rates=[])
L = capi.lib()
one = np.zeros(1, dtype=np.float32)


def sync(b):  # a one-float copy on the launch's stream followed by its synchronise
    capi.check(L.fwgpu_batch_predictions(b.h, capi.ptr(one), 1, None))


def run(side, launches):
    r, b = side["r"], side["b"]
    sync(b)
    t = time.perf_counter()
    for _ in range(launches):
        r.learn_batch(b, capi.MODE_HOGWILD, False)
    sync(b)
    return launches * b.n / (time.perf_counter() - t)


for s in sides.values():  # warm both
    run(s, 3)
p_f, p_p = sides["f32"]["b"].predictions(), sides["packed"]["b"].predictions()
print(f"max |p_packed - p_f32| over the batch = {np.abs(p_p - p_f).max():.3e} (the f32 load holds the unquantised weights)", flush=True)
if a.profile:
    for s in sides.values():
        run(s, 5)
    sys.exit(0)
for rep in range(a.repeats):
    for name in ("f32", "packed"):
        sides[name]["rates"].append(run(sides[name], a.launches))
    print(f"repeat {rep}: f32 {sides['f32']['rates'][-1] / 1e6:.2f} M/s, packed {sides['packed']['rates'][-1] / 1e6:.2f} M/s", flush=True)

b = sides["f32"]["b"]
n, R = b.n, F * K
rec_words = float(off[-1] - off[0]) / n
n_ffm, n_lr = b.n_ffm / n, b.n_lr / n
out = {"shape": dict(fields=F, ffm_k=K, ffm_bit_precision=a.bits, bit_precision=a.bits, batch=n, mode="hogwild", update=0,
                     launches_per_repeat=a.launches, repeats=a.repeats, ffm_rows_per_example=n_ffm, lr_entries_per_example=n_lr,
                     record_words_per_example=rec_words),
       "git_commit": subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or a.commit}
for name, bytes_per_w in (("f32", 4), ("packed", 2)):
    s = sides[name]
    rates = np.array(s["rates"])
    bpe = n_ffm * bytes_per_w * R + 4 * n_lr + 4 * rec_words + 4
    med = float(np.median(rates))
    out[name] = dict(examples_per_s=[float(x) for x in rates], median=med, spread=float((rates.max() - rates.min()) / med),
                     algorithmic_bytes_per_example=bpe, share_of_8TBps=med * bpe / 8e12, ffm_storage=s["storage"], ffm_table_bytes=s["table_bytes"])
out["packed_over_f32"] = out["packed"]["median"] / out["f32"]["median"]
out["faster_by_more_than_the_f32_spread"] = bool(out["packed"]["median"] > out["f32"]["median"] * (1.0 + out["f32"]["spread"]))
out["max_abs_prediction_difference"] = float(np.abs(p_p - p_f).max())
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
json.dump(out, open(a.out, "w"), indent=1)
print(json.dumps(out, indent=1))
