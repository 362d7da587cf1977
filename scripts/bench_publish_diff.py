"""Publishing the DIFFERENCE between two inference models: the device route (fwgpu_image_capture + fwgpu_image_diff, csrc/patch.hip: the last
published weights section stays on the device, the next one is diffed against it there and only the stream crosses PCIe) against the host route
(fwgpu_model_save_inference + fwgpu_diff_bytes on the two files), in ONE process at config C's table sizes (30 fields, k = 8, ffm_bit_precision 28,
-b 28, AdagradLUT); and the hot patch of a packed serving regressor (fwgpu_packed_apply_diff) against fwgpu_model_load_packed of the next file.
  base      fwgpu_image_capture of the regressor as published
  train     --examples more examples (synthetic records); reported: the share of weights-section bytes that changed, the stream's size, whether
            the quantiser's 8-byte header moved (--pin_extremes keeps it where it is: the case the reference's rounding of the extremes is for)
  device    fwgpu_image_capture + fwgpu_image_diff, whole calls
  host      fwgpu_model_save_inference of the next file + both files read + fwgpu_diff_bytes (the base file is there from the last publish; its
            save is timed too and reported beside)
  apply     fwgpu_packed_apply_diff on the regressor loaded from the base file  vs  fwgpu_model_load_packed of the next file
Both streams must be byte-identical or the script fails.  Medians of --repeats (>= 5) repetitions with min - max.  The three kernels' times by device
events stand beside a device-to-device copy of one weights section in the same run (fwgpu_debug_diff_rates).  Files go to a memory-backed directory.
THE BAR: the device route's slowest whole call is faster than the host route's fastest.  Needs a GPU: no fallback.
usage: python3 scripts/bench_publish_diff.py [--out profiles/publish_diff.json] [--repeats 5] [--bits 28] [--examples 2000] [--pin_extremes] [--dir /dev/shm]"""
import argparse
import ctypes as C
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "publish_diff.json"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--bits", type=int, default=28)
ap.add_argument("--examples", type=int, default=2000)
ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None)
ap.add_argument("--pin_extremes", action="store_true", help="write +x and -x, x beyond every trained weight, into the last two FFM weights before the "
                "base publish: the quantiser's rounded extremes, and with them its 8-byte header, then stay put between the two publishes")
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
lib = capi.lib()


def say(msg):
    print(f"[{time.time() - t0:6.0f} s] {msg}", flush=True)


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t


def train(first, n):
    recs, off = fw.synth_records(F, 5.67, 1.05, 100000, 0.1, 21, first, n)
    b = re.record_batch(fw.FeatureBufferTranslator(mi), recs, off)
    re.learn_batch(b, capi.MODE_SEQUENTIAL, True)
    b.close()


def image_diff_once(base, nxt, buf):
    """one fwgpu_image_diff call into a buffer that fits (the size is known from the first repetition) -> (stream bytes, changed)"""
    n, ch = C.c_uint64(0), C.c_uint64(0)
    capi.check(lib.fwgpu_image_diff(base.h, nxt.h, capi.ptr(buf), buf.size, C.byref(n), C.byref(ch)))
    return n.value, ch.value


def host_diff(path0, path1, buf):
    x, y = np.fromfile(path0, dtype=np.uint8), np.fromfile(path1, dtype=np.uint8)
    n, ch = C.c_uint64(0), C.c_uint64(0)
    capi.check(lib.fwgpu_diff_bytes(capi.ptr(x), capi.ptr(y), x.size, 0, 0, capi.ptr(buf), buf.size, C.byref(n), C.byref(ch)))
    return n.value, ch.value


re = fw.Regressor(mi)  # (fails without a GPU); FFM weights: the reference's own random initialisation
train(0, a.examples)   # (a model that has trained before its first publish)
if a.pin_extremes:
    n_ffm = re.table_len(capi.TABLE_FFM_W)
    x = float(np.ceil(np.abs(re.table_read(capi.TABLE_FFM_W)).max() * 2 + 1))
    re.table_write(capi.TABLE_FFM_W, [x, -x], offset=n_ffm - 2)
say(f"regressor trained on {a.examples} examples" + (f", extremes pinned at +-{x}" if a.pin_extremes else ""))
times = {k: [] for k in ("capture_base", "capture_next", "image_diff", "device_route", "save_base", "save_next", "host_diff", "host_route",
                         "apply_diff", "load_packed")}
kernel_ms = []
with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
    f0, f1 = os.path.join(tmp, "publish0.fw"), os.path.join(tmp, "publish1.fw")
    base = None
    for rep in range(a.repeats):
        if base is not None:
            base.close()
        base, s = timed(lambda: P.Image.capture(mi, vw, re, quantize_weights=True))
        times["capture_base"].append(s)
        _, s = timed(lambda: P.save_inference_regressor(f0, mi, vw, re, quantize_weights=True))
        times["save_base"].append(s)
    header_bytes, weights_bytes = base.lengths()
    say(f"base published: header {header_bytes} bytes, weights section {weights_bytes} bytes; capture {np.median(times['capture_base']):.3f} s, "
        f"save {np.median(times['save_base']):.3f} s")
    train(a.examples, a.examples)
    say(f"{a.examples} more examples trained")
    # sizes first (untimed), so that the timed calls are single calls into a buffer that fits
    nxt = P.Image.capture(mi, vw, re, quantize_weights=True)
    stream, changed = base.diff(nxt, with_changed=True)
    nxt.close()
    buf_d, buf_h = np.zeros(len(stream) + 16, dtype=np.uint8), np.zeros(len(stream) + 16, dtype=np.uint8)
    for rep in range(a.repeats):
        t = time.perf_counter()
        nxt = P.Image.capture(mi, vw, re, quantize_weights=True)
        t1 = time.perf_counter()
        got = image_diff_once(base, nxt, buf_d)
        t2 = time.perf_counter()
        times["capture_next"].append(t1 - t)
        times["image_diff"].append(t2 - t1)
        times["device_route"].append(t2 - t)
        assert got == (len(stream), changed)
        t = time.perf_counter()
        P.save_inference_regressor(f1, mi, vw, re, quantize_weights=True)
        t1 = time.perf_counter()
        got_h = host_diff(f0, f1, buf_h)
        t2 = time.perf_counter()
        times["save_next"].append(t1 - t)
        times["host_diff"].append(t2 - t1)
        times["host_route"].append(t2 - t)
        assert got_h == got and buf_h[: got[0]].tobytes() == buf_d[: got[0]].tobytes() == stream, "THE DEVICE'S STREAM AND THE HOST'S DIFFER"
        kernel_ms.append(list(P.debug_diff_rates(base, nxt)))
        nxt.close()
        say(f"repeat {rep}: device {times['device_route'][-1]:8.3f} s (capture {times['capture_next'][-1]:.3f} + diff {times['image_diff'][-1]:.3f})   "
            f"host {times['host_route'][-1]:8.3f} s (save {times['save_next'][-1]:.3f} + diff {times['host_diff'][-1]:.3f})")
    base.close()
    b0, b1 = np.fromfile(f0, dtype=np.uint8), np.fromfile(f1, dtype=np.uint8)
    q_at = header_bytes + 4 * (1 << a.bits)
    header_moved = bool((b0[q_at: q_at + 8] != b1[q_at: q_at + 8]).any())
    del b0, b1
    re.close()
    # ---- the hot patch against the reload
    _, _, served = P.new_regressor_from_filename(f0, immutable=True, packed=True)
    for rep in range(a.repeats):  # (applying the same stream again stores the same bytes: the same work)
        n, s = timed(lambda: served.apply_diff(stream))
        times["apply_diff"].append(s)
        assert n == changed
        (_, _, fresh), s = timed(lambda: P.new_regressor_from_filename(f1, immutable=True, packed=True))
        times["load_packed"].append(s)
        if rep == 0:
            same = [served.table_checksum(t) == fresh.table_checksum(t) for t in (capi.TABLE_FFM_W, capi.TABLE_LR)]
            assert all(same), "the patched regressor differs from the one loaded from the next file"
        fresh.close()
        say(f"repeat {rep}: apply_diff {times['apply_diff'][-1]:8.4f} s   load_packed {times['load_packed'][-1]:8.3f} s")
    served.close()


def stat(xs):
    xs = np.array(xs, dtype=np.float64)
    return dict(median_s=float(np.median(xs)), min_s=float(xs.min()), max_s=float(xs.max()), all_s=[float(x) for x in xs])


out = {"shape": dict(fields=F, ffm_k=K, bit_precision=a.bits, ffm_bit_precision=a.bits, optimizer="AdagradLUT", repeats=a.repeats,
                     pin_extremes=a.pin_extremes, header_bytes=header_bytes, weights_bytes=weights_bytes, file_dir=a.dir or tempfile.gettempdir()),
       "git_commit": subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or a.commit,
       "change": dict(examples_before_base=a.examples, examples_between=a.examples, changed_bytes=changed, share_of_weights_bytes=changed / weights_bytes,
                      stream_bytes=len(stream), stream_bytes_per_changed_byte=len(stream) / max(changed, 1), quantiser_header_moved=header_moved),
       "identical": "the device's stream, the host's stream of the two files: every byte; patched and reloaded regressors: checksums of both tables"}
out.update({k: stat(v) for k, v in times.items()})
out["host_route_with_both_saves"] = stat(np.array(times["host_route"]) + np.array(times["save_base"]))
out["pcie_bytes"] = dict(device_route=len(stream) + 8 + 12 + 16, host_route=weights_bytes, apply_diff=9 * changed, load_packed=weights_bytes)
km = np.median(np.array(kernel_ms), axis=0)
copy_rate = 2 * weights_bytes / (km[3] * 1e-3)
out["kernels"] = dict(ms_all=kernel_ms, tile_bytes=P.debug_diff_geometry(),
                      size_pass=dict(median_ms=float(km[0]), bytes=2 * weights_bytes, bytes_per_s=2 * weights_bytes / (km[0] * 1e-3)),
                      tile_scan=dict(median_ms=float(km[1])),
                      emit_pass=dict(median_ms=float(km[2]), bytes=2 * weights_bytes + len(stream), bytes_per_s=(2 * weights_bytes + len(stream)) / (km[2] * 1e-3)),
                      device_copy=dict(median_ms=float(km[3]), bytes=2 * weights_bytes, bytes_per_s=copy_rate))
for k in ("size_pass", "emit_pass"):
    out["kernels"][k]["share_of_device_copy_rate"] = out["kernels"][k]["bytes_per_s"] / copy_rate
out["bar_met"] = bool(out["device_route"]["max_s"] < out["host_route"]["min_s"])
out["apply_faster_than_reload"] = bool(out["apply_diff"]["max_s"] < out["load_packed"]["min_s"])
out["verdict"] = (("the device route's slowest call is faster than the host route's fastest" if out["bar_met"] else "THE BAR IS NOT MET") +
                  f": device {out['device_route']['median_s']:.3f} s, host {out['host_route']['median_s']:.3f} s; apply_diff "
                  f"{out['apply_diff']['median_s']:.4f} s against load_packed {out['load_packed']['median_s']:.3f} s")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
json.dump(out, open(a.out, "w"), indent=1)
print(json.dumps(out, indent=1))
