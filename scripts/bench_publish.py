"""Publishing a trained regressor: the device routes (csrc/quantize.hip: fwgpu_pack_regressor, fwgpu_model_save_inference, fwgpu_quantize_ffm_table)
against the host routes they replace, in ONE process at config C's table sizes (30 fields, k = 8, ffm_bit_precision 28, -b 28, AdagradLUT), on a
randomly filled regressor:
  (a) pack      fwgpu_pack_regressor                          vs  fwgpu_model_save + fwgpu_model_load_packed under FWGPU_QUANTIZE_HOST=1
  (b) save      fwgpu_model_save_inference(quantize = 1)      vs  fwgpu_model_save + fwgpu_model_convert_inference(quantize = 1)
  (c) quantize  fwgpu_quantize_ffm_table                      vs  fwgpu_table_read + fwgpu_quantize_ffm_weights
Both sides of a pair must give identical bytes / checksums before a time is reported.  Medians of --repeats (>= 5) repetitions with min - max; the
bytes each side moves over PCIe are computed from the sizes; the two kernels' achieved bytes/s are set against a device-to-device copy of the same
table timed in the same run (fwgpu_debug_quantize_rates).  Files go to a memory-backed directory so that no disk is timed.  Needs a GPU: no fallback.
usage: python3 scripts/bench_publish.py [--out profiles/publish.json] [--repeats 5] [--bits 28] [--dir /dev/shm]"""
import argparse
import ctypes as C
import hashlib
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "publish.json"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--bits", type=int, default=28)
ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--commit", default=None, help="recorded as git_commit where the tree runs without its git metadata")
a = ap.parse_args()
assert a.repeats >= 5, "at least 5 repetitions"

F, K = 30, 8
ND = fw.NamespaceDescriptor
mi = fw.ModelInstance(learning_rate=0.1, ffm_learning_rate=0.1, power_t=0.5, ffm_power_t=0.5, bit_precision=a.bits, ffm_k=K,
                      ffm_bit_precision=a.bits, optimizer=fw.Optimizer.AdagradLUT, add_constant_feature=True,
                      feature_combo_descs=[fw.FeatureComboDesc([ND(i)]) for i in range(F)], ffm_fields=[[ND(i)] for i in range(F)])
vw = VwNamespaceMap("".join(f"N{i:02d},ns{i}\n" for i in range(F)))
t0 = time.time()


def say(msg):
    print(f"[{time.time() - t0:6.0f} s] {msg}", flush=True)


re = fw.Regressor(mi)  # (fails without a GPU); FFM weights: the reference's own random initialisation
rng = np.random.default_rng(a.seed)
L_LR = re.table_len(capi.TABLE_LR) // 2
N_FFM = re.table_len(capi.TABLE_FFM_W)
chunk = 1 << 24
for at in range(0, 2 * L_LR, chunk):  # LR pairs as a trained model has them: {w, accumulator}
    n = min(chunk, 2 * L_LR - at)
    v = np.empty(n, dtype=np.float32)
    v[0::2] = rng.normal(0.0, 0.05, n // 2)
    v[1::2] = 1.0 + rng.random(n // 2, dtype=np.float32)
    re.table_write(capi.TABLE_LR, v, at)
say(f"regressor filled: LR {L_LR} entries, FFM {N_FFM} weights")

sums = [re.table_checksum(t) for t in (capi.TABLE_LR, capi.TABLE_FFM_W, capi.TABLE_FFM_ACC)]
lib = capi.lib()


def digest(path):
    h = hashlib.blake2b()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(1 << 24), b""):
            h.update(block)
    return h.hexdigest()


def packed_identity(r):
    return (r.table_checksum(capi.TABLE_FFM_W), r.table_checksum(capi.TABLE_LR), r.ffm_storage())


times = {k: [] for k in ("pack_device", "pack_host", "save_device", "save_host", "quantize_device", "quantize_host")}
kernel_ms = []
with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
    t_path, q_path, d_path = (os.path.join(tmp, x) for x in ("train.fw", "convert.fw", "direct.fw"))
    for rep in range(a.repeats):
        # ---- (a) pack
        t = time.perf_counter()
        rp = re.pack()
        times["pack_device"].append(time.perf_counter() - t)
        os.environ["FWGPU_QUANTIZE_HOST"] = "1"
        t = time.perf_counter()
        P.save_regressor_to_filename(t_path, mi, vw, re)
        _, _, rh = P.new_regressor_from_filename(t_path, immutable=True, packed=True)
        times["pack_host"].append(time.perf_counter() - t)
        del os.environ["FWGPU_QUANTIZE_HOST"]
        if rep == 0:
            assert packed_identity(rp) == packed_identity(rh), "pack: the device route and the file route differ"
        rp.close()
        rh.close()
        say(f"repeat {rep}: pack       device {times['pack_device'][-1]:8.3f} s   host {times['pack_host'][-1]:8.3f} s")
        # ---- (b) inference save
        t = time.perf_counter()
        P.save_inference_regressor(d_path, mi, vw, re, quantize_weights=True)
        times["save_device"].append(time.perf_counter() - t)
        os.environ["FWGPU_QUANTIZE_HOST"] = "1"
        t = time.perf_counter()
        P.save_regressor_to_filename(t_path, mi, vw, re)
        P.convert_inference_regressor(t_path, q_path, quantize_weights=True)
        times["save_host"].append(time.perf_counter() - t)
        del os.environ["FWGPU_QUANTIZE_HOST"]
        if rep == 0:
            assert os.path.getsize(d_path) == os.path.getsize(q_path) and digest(d_path) == digest(q_path), "save: the two files differ"
            file_bytes = dict(training=os.path.getsize(t_path), inference=os.path.getsize(q_path))
        say(f"repeat {rep}: save       device {times['save_device'][-1]:8.3f} s   host {times['save_host'][-1]:8.3f} s")
        os.remove(t_path)
        # ---- (c) the quantised block
        t = time.perf_counter()
        qd = re.quantize_ffm_table()
        times["quantize_device"].append(time.perf_counter() - t)
        t = time.perf_counter()
        qh = P.quantize_ffm_weights(re.table_read(capi.TABLE_FFM_W))
        times["quantize_host"].append(time.perf_counter() - t)
        if rep == 0:
            assert qd == qh, "quantize: the device's block and the host's differ"
        del qd, qh
        say(f"repeat {rep}: quantize   device {times['quantize_device'][-1]:8.3f} s   host {times['quantize_host'][-1]:8.3f} s")
        ms = (C.c_float * 3)()
        capi.check(lib.fwgpu_debug_quantize_rates(re.h, ms))
        kernel_ms.append([float(x) for x in ms])
assert [re.table_checksum(t) for t in (capi.TABLE_LR, capi.TABLE_FFM_W, capi.TABLE_FFM_ACC)] == sums, "the source regressor changed"
re.close()


def stat(xs):
    xs = np.array(xs, dtype=np.float64)
    return dict(median_s=float(np.median(xs)), min_s=float(xs.min()), max_s=float(xs.max()), all_s=[float(x) for x in xs])


blob = 8 * L_LR + 8 * N_FFM  # the training blob: LR {w, acc} pairs, FFM weights, FFM accumulators
pcie = {"pack_device": 12, "pack_host": blob + 8 * L_LR + 2 * N_FFM,  # (12: the statistics' three words; host: the blob down, LR pairs and buckets up)
        "save_device": 4 * L_LR + 2 * N_FFM + 12, "save_host": blob,
        "quantize_device": 2 * N_FFM + 12, "quantize_host": 4 * N_FFM}
out = {"shape": dict(fields=F, ffm_k=K, bit_precision=a.bits, ffm_bit_precision=a.bits, optimizer="AdagradLUT", lr_entries=L_LR, ffm_weights=N_FFM,
                     repeats=a.repeats, file_dir=a.dir or tempfile.gettempdir(), file_bytes=file_bytes),
       "git_commit": subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or a.commit,
       "identical": "packed regressors: checksums of the FFM weights and of the LR table, and ffm_storage; files: size and blake2b; blocks: every byte"}
for pair in ("pack", "save", "quantize"):
    d, h = stat(times[pair + "_device"]), stat(times[pair + "_host"])
    d["pcie_bytes"], h["pcie_bytes"] = pcie[pair + "_device"], pcie[pair + "_host"]
    out[pair] = dict(device=d, host=h, host_over_device=h["median_s"] / d["median_s"],
                     device_wins=bool(d["max_s"] < h["min_s"]))  # (every repetition of one side below every repetition of the other)
km = np.median(np.array(kernel_ms), axis=0)
copy_rate = 8 * N_FFM / (km[2] * 1e-3)
out["kernels"] = dict(ms_all=kernel_ms, statistics=dict(median_ms=float(km[0]), bytes=4 * N_FFM, bytes_per_s=4 * N_FFM / (km[0] * 1e-3)),
                      buckets=dict(median_ms=float(km[1]), bytes=6 * N_FFM, bytes_per_s=6 * N_FFM / (km[1] * 1e-3)),
                      device_copy=dict(median_ms=float(km[2]), bytes=8 * N_FFM, bytes_per_s=copy_rate))
for k in ("statistics", "buckets"):
    out["kernels"][k]["share_of_device_copy_rate"] = out["kernels"][k]["bytes_per_s"] / copy_rate
out["verdict"] = ("the device route wins on (a) pack" if out["pack"]["device_wins"] else "THE DEVICE ROUTE DOES NOT WIN ON (a) pack") + \
    f": host / device = {out['pack']['host_over_device']:.1f}; (b) save {out['save']['host_over_device']:.1f}; (c) quantize {out['quantize']['host_over_device']:.1f}"
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
json.dump(out, open(a.out, "w"), indent=1)
print(json.dumps(out, indent=1))
