#!/usr/bin/env python3
"""Headline benchmark: examples/sec (+ final log-loss) of LR+FFM online training on MI355X.

  python bench.py --gpus N --steps K --warmup W          (N=1)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A "step" is one pass of the learn path over one micro-batch of synthetic records (BASELINE.json config C:
30 fields, k=8, 28-bit hashes, ~200 nnz/example, AdagradLUT) with the translated batch already resident in HBM.
Rank 0 prints ONE JSON line (see the driver contract in the task description).

A plain run sets up, warms up, times the steps, writes --dump-outputs if asked and prints the line.  `--full` adds every side figure and
check: the CPU baseline, the other configurations' legs, the host-fed rate, live traffic, the copy peak, the CPU oracle's curves and, N > 1,
the other multi-GPU modes.

N > 1: every rank owns a full replica and trains on its own shard of the stream (weak scaling); replicas are
kept together by an RCCL all-reduce of the weight/accumulator deltas every --sync-every steps (DESIGN.md,
"Multi-GPU").  The syncs that fall inside the timed steps are timed.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

# the host driver of this pool only supports dmabuf IPC: RCCL between processes needs this (already exported on the boxes)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec


# Hyper-parameters: the reference's production-like command line (run_one.sh: `-l 0.025 --adaptive --power_t 0.38`,
# k=8, FFM inheriting lr / power_t / init_acc_gradient=1.0 from the LR block: model_instance.rs:418-428).
# `-l 0.1` (the benchmark/ LR setting, ~13 nnz/example) DIVERGES on this ~200-nnz stream even in the sequential
# reference algorithm (scripts/oracle_convergence.py: hold-out log-loss 2.12 vs 0.659 at 0.025), and a diverged run
# saturates the sigmoid, which skips updates and inflates examples/sec.
LR, POWER_T, INIT_ACC = 0.025, 0.38, 1.0
# deep head (config E only): the reference's defaults (model_instance.rs:139-142) except init_acc 0 -> 1.0 like the blocks above
NN_LR, NN_POWER_T, NN_INIT_ACC = 0.02, 0.45, 1.0


def build_model_instance(fw, args, device):
    F = args.fields
    return fw.ModelInstance(
        learning_rate=getattr(args, "lr", LR), ffm_learning_rate=getattr(args, "lr", LR), power_t=getattr(args, "power_t", POWER_T),
        ffm_power_t=getattr(args, "power_t", POWER_T), init_acc_gradient=INIT_ACC,
        ffm_init_acc_gradient=INIT_ACC, bit_precision=args.bits, ffm_bit_precision=args.ffm_bits, ffm_k=args.k,
        add_constant_feature=not os.environ.get("FWGPU_BENCH_NO_CONSTANT"), optimizer=fw.Optimizer.AdagradLUT,  # (experiment switch: the constant feature is the one LR entry every example writes)
        feature_combo_descs=[fw.FeatureComboDesc([fw.NamespaceDescriptor(i)]) for i in range(F)],
        ffm_fields=[[fw.NamespaceDescriptor(i)] for i in range(F)], device=device,
        # config E: `--nn_layers 2 --nn 0:width:256 --nn 0:activation:relu ...`, topology "one" 
        nn_layers=[dict(width=args.nn_width, activation="relu", init="hu") for _ in range(args.nn_layers)],
        nn_topology="one", nn_learning_rate=NN_LR, nn_power_t=NN_POWER_T, nn_init_acc_gradient=NN_INIT_ACC)


# The second stream family at config C's size (tests/test_zz_gpu_hogwild_quality.py's `zipf13_noise` recipe): another teacher
# (the teacher's scores and the ids' streams both derive from the seed), a heavier head (Zipf 1.3: the hot rows are hotter), 5 % of the labels flipped
# (a loss floor well above the teacher's entropy).  `--family 2`; oracle curves: tests/golden/bench_oracle_curve_fam2_*.json.
FAMILY2 = {"seed": 4242, "zipf": 1.3, "label_flip": 0.05}


def apply_family(args, family):
    if family == 2:
        for k_, v_ in FAMILY2.items():
            setattr(args, k_, v_)


def _flip_mask(seed, first, n, frac):
    """label noise that does not depend on how the stream is cut into chunks: example number e is flipped iff splitmix64(seed, e) < frac * 2^64"""
    with np.errstate(over="ignore"):
        x = (np.arange(first, first + n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed) * np.uint64(0xD1342543DE82EF95)
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return (x >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53)) < frac


def synth_one_pass(args, first, n):
    """fw.synth_records with one pass of the generator instead of two (sizing the stream, then writing it): fwgpu_synth_records writes straight
    into room for n of the longest records the configuration can produce -- the 3-word header, one slot per namespace and at most 64 (hash,
    value) pairs per namespace (translate.cpp) -- and the words it wrote are returned.  The same records and offsets."""
    import ctypes as C

    from fwumious_wabbit_amd import _capi as capi

    cap = n * (3 + args.fields * (1 + 2 * 64))
    records = np.empty(cap, dtype=np.uint32)  # (only the pages written become resident)
    rec_off = np.zeros(n + 1, dtype=np.uint64)
    nw = C.c_uint64(0)
    cfg = capi.SynthConfig(args.fields, args.mean_extra, args.zipf, args.ids, args.p_weighted, args.seed)
    capi.check(capi.lib().fwgpu_synth_records(C.byref(cfg), first, n, capi.ptr(records), cap, capi.ptr(rec_off), C.byref(nw)))
    return records[: nw.value], rec_off


GEN_THREADS = min(16, len(os.sched_getaffinity(0)))  # the host CPUs this process may use, at most 16


def gen_records(fw, args, first, n, threads=GEN_THREADS):
    """Synthetic stream [first, first+n) in chunks on a thread pool (ctypes releases the GIL); every example is a function of its number
    alone, so the records do not depend on the number of threads."""
    chunk = 2048
    jobs = [(first + s, min(chunk, n - s)) for s in range(0, n, chunk)]

    def one(j):
        return synth_one_pass(args, j[0], j[1])

    with ThreadPoolExecutor(max_workers=threads) as ex:
        parts = list(ex.map(one, jobs))
    recs = np.concatenate([p[0] for p in parts])
    offs = [np.zeros(1, dtype=np.uint64)]
    base = 0
    for r, o in parts:
        offs.append(o[1:] + np.uint64(base))
        base += len(r)
    off = np.concatenate(offs)
    flip = getattr(args, "label_flip", 0.0)
    if flip:  # record word 1 = the label (parser.rs:57-60): 1 <-> 0
        idx = off[:-1].astype(np.int64) + 1
        f = _flip_mask(args.seed, first, n, flip)
        recs[idx[f]] = 1 - recs[idx[f]]
    return recs, off


def algorithmic_bytes(args, batch, n_words):
    """train, AdaGrad: n_ffm*16*R + n_lr*16 + 4*record_len + 4 per example."""
    R = args.fields * args.k
    b = batch.n_ffm * 16 * R + batch.n_lr * 16 + 4 * n_words + 4 * batch.n
    if args.nn_layers:  # config E: + the dense weights once per launch (16 B each: w, acc read and written)
        X = args.fields + 1 + args.fields * (args.fields + 1) // 2
        wn, i = 0, X
        for _ in range(args.nn_layers):
            wn += (i + 1) * args.nn_width
            i = args.nn_width
        b += 16 * (wn + i + X + 1)
    return b


def logloss(p, y):
    p = np.clip(p.astype(np.float64), 1e-15, 1 - 1e-15)  # benchmark/calc_loss.py:5-25
    return float(np.mean(-np.where(y == 1, np.log(p), np.log(1 - p))))


DUMP_BLOCKS, DUMP_BLOCK = 256, 4096  # --dump-outputs: per table, 256 blocks of 4096 consecutive floats (4 MiB)
DUMP_MAX_BYTES = 64 << 20


def dump_outputs(re, capi, fbt, records, rec_off, sync, stream, out_dir, seed):
    """--dump-outputs, as float32 .npy files.  The timed steps run concurrently (hogwild: unsynchronised read-modify-write of rows that many
    examples hold), so the model they leave and every prediction made from it depend on timing and differ from run to run on the same inputs.
    What is written instead is a function of the inputs and the build alone, so that two builds can be compared output for output: the last timed
    step's records through the step's own entry (learn_batch, or learn_batch_sync for synchronous steps) on `re`, a FRESH model of the same
    configuration, in the library's in-order mode (FWGPU_MODE_SEQUENTIAL: one workgroup walking the batch in example order; launches that are
    concurrent-only -- store policies 3 / 4, the small-example shape, the head as a phase -- do not run there) -> inorder_predictions and the
    tables it updated (whole, or DUMP_BLOCKS blocks at offsets drawn from a fixed seed where a table is larger); then a predict-only CONCURRENT
    launch of the timed steps' shape over the same records on that model -> concurrent_predictions (no writes: nothing races)."""
    b = re.record_batch(fbt, records, rec_off)
    if sync:
        re.learn_batch_sync(b, re.split_buffers(b.n, 1024), capi.MODE_SEQUENTIAL, stream)
    else:
        re.learn_batch(b, capi.MODE_SEQUENTIAL, True, stream)
    arrays = {"inorder_predictions": b.predictions(stream)}
    tables = {"lr_table": capi.TABLE_LR, "ffm_weights": capi.TABLE_FFM_W, "ffm_accumulators": capi.TABLE_FFM_ACC,
              "nn_weights": capi.TABLE_NN_W, "nn_accumulators": capi.TABLE_NN_ACC}
    for name, which in tables.items():
        n = re.table_len(which)
        if n == 0:  # (no deep head)
            continue
        if n <= DUMP_BLOCKS * DUMP_BLOCK:
            arrays["inorder_" + name] = re.table_read(which)
        else:
            rng = np.random.default_rng([seed, which])
            starts = np.sort(rng.choice(n // DUMP_BLOCK, DUMP_BLOCKS, replace=False)) * DUMP_BLOCK
            arrays["inorder_" + name + "_sample"] = np.concatenate([re.table_read(which, int(s), DUMP_BLOCK) for s in starts])
    re.learn_batch(b, capi.MODE_HOGWILD, False, stream)
    arrays["concurrent_predictions"] = b.predictions(stream)
    b.close()
    assert sum(a.nbytes for a in arrays.values()) <= DUMP_MAX_BYTES
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a.astype(np.float32, copy=False))


def oracle_reference_curves(args, world, holdout=None):
    """Hold-out log-loss of the reference algorithm on this very stream and hold-out tail after N examples: numbers produced by
    scripts/make_bench_oracle_curve.py from the CPU oracle and committed as data (tests/golden/bench_oracle_curve_*.json) -- the reference's single
    thread ("seq", deterministic) and its 16-thread hogwild mode ("hog16", three runs: racy by definition).  Only for the default single-GPU stream
    (with N > 1 every rank trains on its own shard: another example order); {} when the run's stream is another one.  The files hold the loss on the
    262 144-example hold-out and on its first 8 192 examples (rounds 1-4's yardstick): --holdout picks one of the two."""
    import glob

    out = {"seq": {}, "hog16": []}
    if world != 1:
        return out
    holdout = args.holdout if holdout is None else holdout
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "bench_oracle_curve_*.json"))):
        d = json.load(open(path))
        if holdout == d["config"]["holdout"]:
            key = "logloss"
        elif holdout == 8192 and "logloss_first_8192" in d:
            key = "logloss_first_8192"
        else:
            continue
        c = dict(d["config"])
        c.pop("holdout")
        c.setdefault("nn_layers", 0)
        c.setdefault("label_flip", 0.0)
        if not c["nn_layers"]:
            c.pop("nn_width", None)
        same = all(getattr(args, k, 0.0 if k == "label_flip" else None) == v for k, v in c.items()) and d["hyper"] == {"lr": getattr(args, "lr", LR), "power_t": getattr(args, "power_t", POWER_T), "init_acc": INIT_ACC}
        if not same:
            continue
        curve = dict(zip(d["examples"], d[key]))
        if d.get("threads", 1) == 1:
            out["seq"].update(curve)  # (the sequential curve is deterministic: a longer run's file only adds checkpoints)
        else:
            out["hog16"].append(curve)
    return out


def link_bytes_per_example(args, world, n_ffm, n_lr, rec_words, sync_every, table_bytes):
    """What one example puts on the xGMI links of ONE rank (bytes sent + received), per multi-GPU mode, for this run's model and N
    (analytic, from the modes' exchange steps -- the sparse mode's measured figure is dp_modes.sparse.bytes_sent_per_example)."""
    N = world
    if N <= 1:
        return None
    R4 = args.fields * args.k * 4            # one FFM row, bytes
    SL4 = (args.fields * args.fields * args.k + 3 * args.fields + 8) * 4  # one split record (T, corrections, counts, LR sum, label, importance)
    rows, f = n_ffm * R4, (N - 1) / N
    return {
        "replica": 2 * f * table_bytes / (sync_every * args.batch * 1.0),                    # ring all-reduce of the table deltas, once per sync_every steps
        "sparse_upper_bound": (rows + n_ffm * 4 + n_lr * 8) * N,                               # undeduplicated row gradients: own bucket out, N - 1 buckets in
        "sharded": 4 * rec_words * (N - 1) + 2 * SL4 * f + (SL4 + 4) * (N - 1),               # records all-gathered, field sums reduce-scattered, records + gradients all-gathered
        "peer": (5 * rows + 4 * n_lr * 8) * f,                                                 # gather w; read w, acc; write w, acc -- all in the owner's memory
        "owner_apply": (2 * rows + n_ffm * 8 + 2 * n_lr * 8) * f,                               # fetch w from the owner, push the gradient row to the owner (fwgpu_dist_*_owner)
        "owner_stream": (2 * rows + n_ffm * 12 + 2 * n_lr * 12) * f,                            # the same rows, streaming form: + a tag word per row and a free-generation word back (dp_modes.owner_stream)
        "what": "bytes per example on one rank's links (sent + received), (N-1)/N of the rows being remote",
    }


def cpu_baseline(args, n_examples):
    """The CPU oracle (a C restatement of the reference algorithm; the Rust reference cannot be built here)
    timed on this box's host cores in hogwild mode on a bounded sample of the same stream."""
    import fwumious_wabbit_amd as fw
    from oracle import fwo

    cores = os.cpu_count() or 1
    F = args.fields
    lr_, pt_ = getattr(args, "lr", LR), getattr(args, "power_t", POWER_T)
    ocfg = fwo.make_config(optimizer=fwo.OPT_ADAGRAD_LUT, learning_rate=lr_, ffm_learning_rate=lr_, power_t=pt_,
                           ffm_power_t=pt_, init_acc_gradient=INIT_ACC, ffm_init_acc_gradient=INIT_ACC,
                           bit_precision=args.bits, num_combos=F + 1, ffm_k=args.k, ffm_bit_precision=args.ffm_bits,
                           ffm_num_fields=F)
    ots = fwo.TranslatorSpec([([(i, False)], 1.0) for i in range(F)], [[(i, False)] for i in range(F)], True, args.bits,
                             args.k, args.ffm_bits)
    nn = None
    if args.nn_layers:
        nn = fwo.make_nn_config([(args.nn_width, "relu", "hu")] * args.nn_layers, "one", NN_LR, NN_POWER_T, NN_INIT_ACC)
    try:
        om = fwo.Model(ocfg, native=True, nn=nn)
    except Exception:
        om = fwo.Model(ocfg, native=False, nn=nn)
    recs, off = gen_records(fw, args, 10_000_000, n_examples)
    # single thread = the reference's default execution mode (main.rs:213-270)
    n1 = min(n_examples, 4000)
    dt1, _ = om.run_stream(ots, recs[: int(off[n1])], off[: n1 + 1], nthreads=1, want_preds=False)
    # hogwild: the reference's default is 16 threads (main.rs:189-194); also try more of the box and keep the best
    tried = {}
    for t in sorted({min(16, cores), min(64, cores), cores}):
        dt, _ = om.run_stream(ots, recs, off, nthreads=t, want_preds=False)
        tried[t] = n_examples / dt
    best = max(tried, key=tried.get)
    # ... and what the CPU path has learned from its sample (BASELINE.md 2 promises the loss beside the rate): hold-out log-loss of the model the runs above left
    # (every run continues the same model over the same sample), on the first 8192 examples of the bench's hold-out tail
    hrecs, hoff = gen_records(fw, args, 1_000_000_000, 8192)
    hy = hrecs[hoff[:-1].astype(np.int64) + 1].astype(np.float32)
    cpu_ll = logloss(om.predict_stream(ots, hrecs, hoff, nthreads=min(16, cores)), hy)
    learned = n1 + n_examples * len(tried)
    om.close()
    return {"value": tried[best], "unit": "examples/sec", "cores": best, "kind": "port", "final_logloss": cpu_ll, "final_logloss_examples_learned": learned,
            "final_logloss_what": f"hold-out log-loss (first 8192 examples of the bench's hold-out tail) of the oracle model after the timed runs: {n1} examples single-threaded + "
                                  f"{len(tried)} hogwild passes over the same {n_examples}-example sample = {learned} learn calls",
            "sample": f"{n_examples} examples of the same synthetic stream per run, C oracle in hogwild mode "
                      f"(hogwild.rs semantics); threads -> examples/sec: "
                      + ", ".join(f"{t}: {v:.0f}" for t, v in sorted(tried.items()))
                      + f"; single thread (reference default mode): {n1 / dt1:.0f} on {n1} examples; host has {cores} cores",
            "single_thread_value": n1 / dt1}


def measure_traffic(args):
    """HBM bytes per learn launch of THIS workload, measured now: two short child runs of this script under
    `rocprofv3 --kernel-trace --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (separate passes, as MI355X_MICROARCH.md's HBM section
    prescribes; FETCH_SIZE doubled: on gfx950 it reports half of a 16 B/lane coalesced read; KB = 1024 B, calibrated on a 2 GiB
    fill).  Returns (bytes per launch or None, description)."""
    import glob
    import shutil
    import sqlite3
    import subprocess
    import tempfile

    if not shutil.which("rocprofv3"):
        return None, "rocprofv3 not on PATH"
    # (20 + 4 launches, as the driver's shape: the counters of the launches from the 16th on are the figure -- by then the stream's hot rows ARE hot, and store policy 4
    # issues an eighth of their accumulator traffic; the first three launches are kept beside it)
    fwd = ["--steps", "20", "--warmup", "4", "--no-cpu-baseline", "--no-traffic", "--no-config-e", "--no-config-b", "--batch", str(args.batch), "--fields", str(args.fields),
           "--k", str(args.k), "--bits", str(args.bits), "--ffm-bits", str(args.ffm_bits), "--mean-extra", str(args.mean_extra),
           "--zipf", str(args.zipf), "--ids", str(args.ids), "--p-weighted", str(args.p_weighted), "--seed", str(args.seed),
           "--holdout", "256", "--nn-layers", str(args.nn_layers), "--nn-width", str(args.nn_width), "--head", args.head]
    if args.sync:
        fwd.append("--sync")
    if args.threads:
        fwd += ["--threads", str(args.threads)]
    if args.wgs:
        fwd += ["--wgs-per-cu", str(args.wgs)]
    kb, kb_first = {}, {}
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            d = tempfile.mkdtemp(prefix="fwbench_pmc_", dir="/tmp")
            try:
                env = dict(os.environ, TMPDIR="/tmp")
                subprocess.run(["rocprofv3", "--kernel-trace", "--pmc", ctr, "-d", d, "-o", "t", "--", sys.executable,
                                os.path.abspath(__file__)] + fwd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL,
                               stderr=subprocess.DEVNULL, timeout=300, check=False)
                vals = []
                for db in glob.glob(os.path.join(d, "**", "*.db"), recursive=True):
                    con = sqlite3.connect(db)
                    rows = None
                    for order in ("dispatch_id", "start", "rowid"):  # (the dispatches in launch order, whatever this rocprofv3's view calls it)
                        try:
                            rows = list(con.execute(f"select kernel_name, value from counters_collection where counter_name = ? and "
                                                    f"kernel_name like '%fw_example_kernel%' order by {order}", (ctr,)))
                            break
                        except sqlite3.Error:
                            continue
                    con.close()
                    if rows is None:
                        continue
                    # the updating launches are the coherent (sc1) instantiations: template argument COH, the 2nd of
                    # fw_example_kernel_r<OPT, COH, MAXR, WIN> and the 3rd of fw_example_kernel<VEC, OPT, COH, PHASE, NN>
                    for name, v in rows:
                        targs = name[name.index("<") + 1:name.index(">")].replace(" ", "").split(",") if "<" in name else []
                        coh = targs[1] if "kernel_r<" in name else (targs[2] if len(targs) > 2 else "")
                        if coh == "true":
                            vals.append(v)
                if not vals:
                    return None, f"rocprofv3 --pmc {ctr}: no dispatch of the learn kernel found"
                # every dispatch of the child has the same shape; what store policy 4 sends depends on how hot the rows are by then: the late launches are the figure
                late = vals[15:] if len(vals) > 18 else vals
                kb[ctr] = float(np.median(late))
                kb_first[ctr] = float(np.median(vals[:3]))
            finally:
                shutil.rmtree(d, ignore_errors=True)
    except Exception as e:  # a side measurement: never lose the bench line over it
        return None, f"traffic measurement failed: {e!r}"
    total = (2.0 * kb["FETCH_SIZE"] + kb["WRITE_SIZE"]) * 1024.0
    first = (2.0 * kb_first["FETCH_SIZE"] + kb_first["WRITE_SIZE"]) * 1024.0
    return total, (f"measured in this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE / --pmc WRITE_SIZE on child runs of the same command "
                   f"(24 launches; median over the learn dispatches from the 16th on: FETCH_SIZE {kb['FETCH_SIZE']:.0f} KB x2 (gfx950 16 B/lane correction) + WRITE_SIZE {kb['WRITE_SIZE']:.0f} KB; "
                   f"the first three launches, where few rows are hot yet: {first / 1e9:.2f} GB = FETCH_SIZE {kb_first['FETCH_SIZE']:.0f} KB x2 + WRITE_SIZE {kb_first['WRITE_SIZE']:.0f} KB)")


def _child_leg(cmd, timeout=420, env=None):
    import subprocess

    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, check=False, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        raise RuntimeError((p.stderr or p.stdout)[-300:])
    return json.loads(lines[-1])


def config_e_leg(args):
    """BASELINE configs[4] next to the headline line: a short child run of this script with k = 16 and the 2 x 256 ReLU head (exact
    per-example head, hogwild), so that a --full run of the default shape measures it too.  A reported side figure, never `value`.
    `oracle_final_logloss`: the sequential CPU oracle on the same 229 376 examples and the same hold-out (tests/golden/bench_oracle_curve_confige_seq.json)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--k", "16", "--nn-layers", "2", "--nn-width", "256", "--head", "exact", "--batch", "8192",
           "--steps", "24", "--warmup", "4", "--holdout", "65536", "--full", "--no-cpu-baseline", "--no-traffic", "--no-config-e", "--no-config-b",
           "--fields", str(args.fields), "--bits", str(args.bits), "--ffm-bits", str(args.ffm_bits)]
    try:
        d = _child_leg(cmd)
        return {"value": d["value"], "unit": d["unit"], "final_logloss": d["final_logloss"], "oracle_final_logloss": d.get("oracle_final_logloss"),
                "ms_per_step": d["ms_per_step"], "roofline_frac": d["roofline"]["frac"], "examples_learned": (d["steps"] + d["warmup"]) * 8192,
                "holdout_examples": 65536, "workload": d["config"]["workload"], "kernel": d["roofline"]["kernel"]}
    except Exception as e:  # a side measurement: never lose the bench line over it
        return {"value": None, "error": repr(e)}


def no_kept_rows_leg(args, steps, warmup):
    """The same stream and the same number of launches with NO rows kept from the gather (fwgpu_debug_set_option 13 = 0 / FWGPU_KEPT_ROWS=0: every row re-read by the update, no
    last-writer-wins over an example's lifetime): the concurrent mode whose hold-out curve on this stream IS the reference's (profiles/r06_kept_rows_long.txt) -- 14 % slower,
    and on the second stream family 0.004 above the reference where the shipped mode is on it.  A reported side figure, never `value`."""
    cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(steps), "--warmup", str(warmup), "--full", "--no-cpu-baseline", "--no-traffic", "--no-config-e", "--no-config-b",
           "--fields", str(args.fields), "--k", str(args.k), "--bits", str(args.bits), "--ffm-bits", str(args.ffm_bits), "--holdout", str(args.holdout)]
    try:
        d = _child_leg(cmd, env=dict(os.environ, FWGPU_KEPT_ROWS="0"))
        return {"value": d["value"], "unit": d["unit"], "final_logloss": d["final_logloss"], "oracle_final_logloss": d.get("oracle_final_logloss"),
                "oracle_hogwild16_final_logloss": d.get("oracle_hogwild16_final_logloss"), "roofline_frac": d["roofline"]["frac"], "steps": d["steps"], "warmup": d["warmup"],
                "what": "FWGPU_KEPT_ROWS=0: the large-table kernel re-reads every row in the update instead of writing 20 + 3 rows per wave back as w_gather - step"}
    except Exception as e:  # a side measurement: never lose the bench line over it
        return {"value": None, "error": repr(e)}


def config_b_leg(args):
    """BASELINE configs[1] next to the headline line: 10 fields (one feature each), k = 4, 22-bit tables, micro-batch 4096, AdagradLUT lr 0.1 / power_t 0.5
    (SURVEY 8d "Config B"), 20 + 200 steps in a fresh child process.  The tables (2 x 16.8 MB + 33.5 MB) live in the L2 / Infinity Cache: the figure is
    reported against the HBM peak all the same, with the oracle's loss on the same 901 120 examples beside the GPU's."""
    cmd = [sys.executable, os.path.abspath(__file__), "--fields", "10", "--k", "4", "--bits", "22", "--ffm-bits", "22", "--mean-extra", "0", "--zipf", "1.1",
           "--ids", "100000", "--p-weighted", "0", "--seed", "20240611", "--lr", "0.1", "--power-t", "0.5", "--batch", "4096", "--steps", "200", "--warmup", "20",
           "--holdout", "65536", "--full", "--no-cpu-baseline", "--no-traffic", "--no-config-e", "--no-config-b"]
    try:
        d = _child_leg(cmd)
        return {"value": d["value"], "unit": d["unit"], "final_logloss": d["final_logloss"], "oracle_final_logloss": d.get("oracle_final_logloss"),
                "oracle_hogwild16_final_logloss": d.get("oracle_hogwild16_final_logloss"), "ms_per_step": d["ms_per_step"],
                "roofline_frac": d["roofline"]["frac"], "avg_launch_ms": d["roofline"]["avg_launch_ms"], "examples_learned": (d["steps"] + d["warmup"]) * 4096,
                "holdout_examples": 65536, "micro_batch": 4096, "workload": d["config"]["workload"], "kernel": d["roofline"]["kernel"]}
    except Exception as e:  # a side measurement: never lose the bench line over it
        return {"value": None, "error": repr(e)}


LONG_TOLERANCE = 0.003  # |GPU final hold-out - reference's concurrent mode's| at the end of the long protocol (stated before measuring, round 6)


def two_sided_verdict(finals, merged, seq_final, hog_final, spread):
    gpu = float(np.mean(finals))
    ref = float(np.mean(hog_final)) if hog_final else seq_final
    curve = {n: float(np.mean(v)) for n, v in merged.items()} if merged else {}
    lo_n = min(curve, key=curve.get) if curve else None
    rise = (gpu - curve[lo_n]) if curve else None
    return {"two_sided": True, "tolerance": LONG_TOLERANCE, "gpu_mean_final": gpu, "reference": "oracle, 16-thread hogwild" if hog_final else "oracle, single thread",
            "reference_final": ref, "oracle_single_thread_final": seq_final, "abs_diff": abs(gpu - ref), "within": bool(abs(gpu - ref) <= LONG_TOLERANCE),
            "minimum": curve.get(lo_n) if curve else None, "minimum_at_examples": lo_n, "rise_after_minimum": rise,
            "non_increasing_after_minimum": (bool(rise <= max(spread, 0.001)) if rise is not None else None)}


def long_protocol(args):
    """`bench.py --long`: SURVEY 8d's protocol at its stated length on one GPU -- 16 Mi training examples (256 steps of 65 536) of the config-C stream, hold-out
    = 262 144 examples of the stream's tail that are predicted and never learned (main.rs:184-185, 238-241; loss as benchmark/calc_loss.py:5-25) -- in
    `--long-passes` passes from freshly initialised weights over the same device-resident batches: the concurrent mode is racy, so the FINAL log-loss is
    reported per pass with its spread, next to the CPU oracle's on the same stream (sequential, and the reference's 16-thread hogwild mode: committed data,
    tests/golden/bench_oracle_curve_*.json).  Pass 0 is the timed one (no checkpoints inside); the later passes carry the hold-out checkpoints."""
    import torch

    import fwumious_wabbit_amd as fw
    from fwumious_wabbit_amd import _capi as capi

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (there is no CPU path)")
    torch.cuda.set_device(0)
    B, P = args.batch or 65536, max(1, args.long_passes)
    K = (args.examples // B) if args.examples else args.long_steps
    mi = build_model_instance(fw, args, 0)
    re = fw.Regressor(mi)
    if args.max_in_flight:
        re.set_max_in_flight(args.max_in_flight)
    if args.store_policy is not None:
        re.set_store_policy(args.store_policy)
    fbt = fw.FeatureBufferTranslator(mi)
    t0 = time.time()
    gen_threads = min(128, os.cpu_count() or 8)
    batches, words = [], []
    for s in range(K):  # generated and uploaded step by step: 29 GB of records end up in HBM, never in host memory at once
        recs, off = gen_records(fw, args, s * B, B, threads=gen_threads)
        batches.append(re.record_batch(fbt, recs, off))
        words.append(len(recs))
    hrecs, hoff = gen_records(fw, args, 1_000_000_000, args.holdout, threads=gen_threads)
    hbatch = re.record_batch(fbt, hrecs, hoff)
    hy = hrecs[hoff[:-1].astype(np.int64) + 1].astype(np.float32)
    prep_s = time.time() - t0
    stream = torch.cuda.current_stream()
    sptr = stream.cuda_stream
    for _ in range(16):
        re.learn_batch(hbatch, capi.MODE_HOGWILD, False, sptr)
    torch.cuda.synchronize()
    every = max(1, args.curve_every or 16)
    finals, curves, rates, launch_ms = [], [], [], None
    for ps in range(P):
        re.allocate_and_init_weights()
        torch.cuda.synchronize()
        curve = {}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * K)] if ps == 0 else None
        t_start = time.perf_counter()
        for i in range(K):
            if ev:
                ev[2 * i].record(stream)
            re.learn_batch(batches[i], capi.MODE_HOGWILD, True, sptr)
            if ev:
                ev[2 * i + 1].record(stream)
            if ps > 0 and (i + 1) % every == 0 and i + 1 < K:  # hold-out checkpoint (predict-only), passes 1.. only
                re.learn_batch(hbatch, capi.MODE_HOGWILD, False, sptr)
                curve[(i + 1) * B] = logloss(hbatch.predictions(sptr), hy)
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t_start
        re.learn_batch(hbatch, capi.MODE_HOGWILD, False, sptr)
        final = logloss(hbatch.predictions(sptr), hy)
        curve[K * B] = final
        finals.append(final)
        curves.append(curve)
        rates.append(K * B / elapsed)
        if ev:
            launch_ms = [ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(K)]
            elapsed0 = elapsed
    oc = oracle_reference_curves(args, 1)
    n_final = K * B
    seq_final = oc["seq"].get(n_final)
    hog_final = [c.get(n_final) for c in oc["hog16"] if c.get(n_final) is not None]
    # One more pass WITHOUT rows kept from the gather (fwgpu_debug_set_option 13 = 0): every row re-read by the update, no last-writer-wins over an example's lifetime on the rows many
    # examples hold -- the concurrent mode whose curve on BASELINE configs[2]'s stream is the reference's own.  Reported beside the shipped mode's passes.
    no_kept = None
    if not args.nn_layers and args.k % 4 == 0 and args.fields * args.k <= 256:
        re.set_kept_rows(0)
        re.allocate_and_init_weights()
        torch.cuda.synchronize()
        nk_curve = {}
        t_start = time.perf_counter()
        t_ckpt = 0.0
        for i in range(K):
            re.learn_batch(batches[i], capi.MODE_HOGWILD, True, sptr)
            if (i + 1) % every == 0 or i + 1 == K:
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                re.learn_batch(hbatch, capi.MODE_HOGWILD, False, sptr)
                nk_curve[(i + 1) * B] = logloss(hbatch.predictions(sptr), hy)
                t_ckpt += time.perf_counter() - t1
        nk_elapsed = time.perf_counter() - t_start - t_ckpt
        re.set_kept_rows(-1)
        ref_nk = float(np.mean(hog_final)) if hog_final else seq_final

        def ref_at(n):  # the reference's concurrent mode at n examples (its single thread where no hogwild curve covers n)
            v = [c.get(n) for c in oc["hog16"] if c.get(n) is not None]
            return float(np.mean(v)) if v else oc["seq"].get(n)

        gaps = {n: abs(v - ref_at(n)) for n, v in nk_curve.items() if ref_at(n) is not None}
        lo_n = min(nk_curve, key=nk_curve.get)
        no_kept = {"what": "one pass with fwgpu_debug_set_option(h, 13, 0) / FWGPU_KEPT_ROWS=0: every row re-read by the update", "examples_per_sec": K * B / nk_elapsed,
                   "final_logloss": nk_curve[K * B], "abs_diff": (abs(nk_curve[K * B] - ref_nk) if ref_nk is not None else None),
                   "within": (bool(abs(nk_curve[K * B] - ref_nk) <= LONG_TOLERANCE) if ref_nk is not None else None),
                   "largest_abs_diff_at_any_checkpoint": (max(gaps.values()) if gaps else None),
                   "largest_abs_diff_from_a_quarter_of_the_run_on": (max(v for n, v in gaps.items() if n >= K * B // 4) if gaps else None),
                   "rise_after_minimum": nk_curve[K * B] - nk_curve[lo_n], "minimum_at_examples": lo_n,
                   "logloss_after_examples": {str(n): v for n, v in sorted(nk_curve.items())}}
    spread = max(finals) - min(finals)
    refs = [v for v in [seq_final] + hog_final if v is not None]
    alg_bytes = float(np.mean([algorithmic_bytes(args, batches[i], words[i]) for i in range(K)]))
    avg_ms = float(np.mean(launch_ms))
    achieved = alg_bytes / (avg_ms * 1e-3) / 1e9
    merged = {}
    for c in curves[1:]:
        for n, v in c.items():
            merged.setdefault(n, []).append(v)
    out = {
        "metric": "examples/sec + final log-loss, 30-field k=8 FFM, at 1/2/4/8 MI355X",
        "value": K * B / elapsed0, "unit": "examples/sec", "n_gpus": 1, "steps": K, "warmup": 0, "ms_per_step": 1e3 * elapsed0 / K,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "protocol": f"--long: {K * B} training examples from freshly initialised weights, hold-out of {args.holdout} examples predicted and never learned "
                    f"(main.rs:184-185, 238-241), {P} passes over the same batches; pass 0 timed without checkpoints, `value` is its rate",
        "final_logloss": float(np.mean(finals)),
        "final_logloss_passes": finals,
        "final_logloss_spread": spread,
        "examples_per_sec_passes": rates,
        "oracle_final_logloss": seq_final,
        "oracle_hogwild16_final_logloss": hog_final or None,
        # The bar of VERDICT r5 item 1c, stated BEFORE the 64 Mi-example runs were made: TWO-sided -- the concurrent mode's final hold-out loss within LONG_TOLERANCE of the
        # reference's own concurrent mode (16-thread hogwild; its single thread where no hogwild curve of this length is committed) -- and, beside it, whether the GPU's
        # curve is non-increasing after its minimum (within the larger of the run-to-run spread and 0.001): reported as measured, both of them.
        "final_logloss_vs_oracle": (two_sided_verdict(finals, merged, seq_final, hog_final, spread) if refs else None),
        "no_kept_rows": no_kept,
        "holdout_prior_logloss": logloss(np.full(len(hy), float(np.mean(hy == 1)), dtype=np.float64), hy),
        "logloss_after_examples": {str(n): v for n, v in sorted(merged.items())},
        "oracle_logloss_after_examples": {str(n): oc["seq"].get(n) for n in sorted(merged)},
        "oracle_hogwild16_logloss_after_examples": {str(n): ([c.get(n) for c in oc["hog16"] if c.get(n) is not None] or None) for n in sorted(merged)},
        "config": {"hyperparameters": f"AdagradLUT lr={args.lr} power_t={args.power_t} init_acc_gradient={INIT_ACC}" + (" (run_one.sh)" if (args.lr, args.power_t) == (LR, POWER_T) else ""),
                   "workload": f"BASELINE.json configs[2] at SURVEY 8d's length: synthetic {args.fields}-field k={args.k} FFM + LR, {args.ffm_bits}-bit FFM hash, {args.bits}-bit LR hash, "
                               f"~{int(args.fields * (1 + args.mean_extra))} nnz/example, AdagradLUT, fused learn, {K * B} train + {args.holdout} hold-out examples",
                   "examples_per_step_per_gpu": B, "global_batch": B, "mode": "hogwild (device-wide concurrent examples)", "parallelism": "1 GPU",
                   "holdout_examples": args.holdout, "prep_seconds": prep_s, "max_in_flight": args.max_in_flight or None, "store_policy": args.store_policy},
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": None,
                     "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_ms": avg_ms},
    }
    print(json.dumps(out), flush=True)
    return 0


def self_launch(args):
    """`python3 bench.py --gpus N` with no launcher around it: this process becomes the launcher of its own N ranks.  It makes NO GPU call and imports
    neither torch nor the library (a process that has touched the GPU must not be replaced, and a parent that holds a context would sit on rank 0's
    device): it starts N fresh children of this very command line with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set as
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1` would, relays rank 0's stdout (the JSON line is its last
    line) and every rank's stderr, and returns non-zero if any rank does; a rank that fails or a run that outlives --launch-timeout ends the others
    (each child leads a process group of its own; the groups this parent started are signalled by their exact ids, nothing is matched by name)."""
    import signal
    import socket
    import subprocess
    import threading

    n = args.gpus
    port = os.environ.get("MASTER_PORT")
    if not port:
        with socket.socket() as so:  # a free port of the loopback interface
            so.bind(("127.0.0.1", 0))
            port = str(so.getsockname()[1])
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True, start_new_session=True))

    def relay(r, pipe, to_stdout):
        for line in pipe:
            if to_stdout:
                sys.stdout.write(line)
                sys.stdout.flush()
            else:
                sys.stderr.write(f"[rank {r}] {line}")
        pipe.close()

    threads = []
    for r, p in enumerate(procs):
        threads.append(threading.Thread(target=relay, args=(r, p.stdout, r == 0), daemon=True))
        threads.append(threading.Thread(target=relay, args=(r, p.stderr, False), daemon=True))
    for t in threads:
        t.start()

    def end_all(sig):
        for p in procs:
            if p.poll() is None:
                try:
                    os.killpg(p.pid, sig)  # the child is the leader of its own session: pgid == pid
                except ProcessLookupError:
                    pass

    deadline = time.time() + args.launch_timeout
    rc = 0
    while True:
        codes = [p.poll() for p in procs]
        bad = [(r, c) for r, c in enumerate(codes) if c not in (None, 0)]
        if bad:
            rc = bad[0][1] if bad[0][1] > 0 else 1
            print(f"[bench launcher] rank {bad[0][0]} exited with {bad[0][1]}: ending the other ranks", file=sys.stderr)
            break
        if all(c == 0 for c in codes):
            break
        if time.time() > deadline:
            rc = 124
            print(f"[bench launcher] {n} ranks did not finish within {args.launch_timeout:.0f} s: ending them", file=sys.stderr)
            break
        time.sleep(0.2)
    if rc:
        end_all(signal.SIGTERM)
        t_end = time.time() + 10
        while time.time() < t_end and any(p.poll() is None for p in procs):
            time.sleep(0.2)
        end_all(signal.SIGKILL)
    for p in procs:
        p.wait()
    for t in threads:
        t.join(timeout=5)
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--batch", type=int, default=None,
                    help="examples per step per GPU (default 65536; --dp-mode sharded: 1024 / n_gpus, --dp-mode sparse: 8192 / n_gpus; the synchronous step is stable "
                         "up to a GLOBAL micro-batch of ~1024 examples at these hyper-parameters: 2048 degrades and diverges in longer runs, profiles/r02_sync_batch_stability.txt, r02_group_modes.txt)")
    ap.add_argument("--fields", type=int, default=30)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--bits", type=int, default=28)
    ap.add_argument("--ffm-bits", dest="ffm_bits", type=int, default=28)
    ap.add_argument("--mean-extra", dest="mean_extra", type=float, default=5.67)
    ap.add_argument("--zipf", type=float, default=1.05)
    ap.add_argument("--ids", type=int, default=10_000_000)
    ap.add_argument("--p-weighted", dest="p_weighted", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=20240612)
    ap.add_argument("--label-flip", dest="label_flip", type=float, default=0.0, help="fraction of the labels flipped (label noise; chunk-invariant)")
    ap.add_argument("--family", type=int, default=1, choices=[1, 2],
                    help="2: the second stream family at config C's size (another teacher seed, Zipf 1.3 ids, 5 %% label flips: FAMILY2)")
    ap.add_argument("--holdout", type=int, default=262144,
                    help="hold-out examples of the stream's tail, predicted and never learned (main.rs:238-241); 262 144: standard error of the mean log-loss ~0.0005. "
                         "(8192 = rounds 1-4's yardstick, the first 8192 of the same tail)")
    ap.add_argument("--nn-layers", dest="nn_layers", type=int, default=0, help="config E: hidden ReLU layers of the deep head")
    ap.add_argument("--nn-width", dest="nn_width", type=int, default=256)
    ap.add_argument("--head", choices=["minibatch", "exact"], default="exact",
                    help="config E (--nn-layers > 0): 'minibatch' = synchronous micro-batches with the deep head on the matrix cores "
                         "(frozen dense weights per batch, summed gradients, one AdaGrad step per weight: head.hip); 'exact' = the "
                         "reference's per-example head inside the fused kernel")
    ap.add_argument("--sync", action="store_true", help="run the steps as synchronous micro-batches (fwgpu_learn_batch_sync) also without a deep head")
    ap.add_argument("--whole-lines", dest="whole_lines", type=int, default=None, choices=[0, 1, 2],
                    help="update path: 0 = round-1 path (float-granular, repeated rows serialised), 1 = auto (default: duplicate-row chains; whole 128 B lines only "
                         "when the accumulator table could not be placed away from the weight table), 2 = chains + whole lines always (A/B runs)")
    ap.add_argument("--threads", type=int, default=0, help="workgroup size override")
    ap.add_argument("--wgs-per-cu", dest="wgs", type=int, default=0)
    ap.add_argument("--max-in-flight", dest="max_in_flight", type=int, default=0,
                    help="cap on concurrently processed examples (hogwild.rs runs 16 threads; 0 = what the device holds)")
    ap.add_argument("--sync-every", dest="sync_every", type=int, default=0, help="N>1: steps between delta all-reduces")
    ap.add_argument("--combine", choices=["mean", "sum"], default="mean",
                    help="N>1: the agreed model moves by the mean (default) or the sum of the replicas' deltas")
    ap.add_argument("--no-other-modes", dest="other_modes", action="store_false",
                    help="N>1 replica run: skip the short sparse / sharded legs that are reported as dp_modes")
    ap.add_argument("--other-modes-timeout", dest="other_modes_timeout", type=float, default=240.0,
                    help="seconds after which the dp_modes legs are given up and the line is printed without them")
    ap.add_argument("--dp-mode", dest="dp_mode", choices=["replica", "sharded", "sparse", "peer"], default="replica",
                    help="N>1: 'replica' = full replicas + overlapped RCCL all-reduce of the table deltas every --sync-every steps "
                         "(the timed mode of a multi-GPU run); 'sharded' = owner-sharded tables, synchronous step with all-gather / "
                         "reduce-scatter of field sums (fwgpu_dist_learn_sharded_batch).  A replica run also times a short "
                         "sharded leg and reports it as dp_modes.sharded; 'sparse' = full replicas, per-micro-batch all-gather of "
                         "deduplicated row gradients, one summed-gradient step per row (fwgpu_dist_learn_sparse_batch), also timed "
                         "as dp_modes.sparse on a replica run; 'peer' = tables sharded by owner, every rank runs the fused hogwild kernel on its own batches and "
                         "reaches each row in its owner's memory through IPC-mapped tables (fwgpu_dist_peer_attach / learn_peer_batch): no collective per step")
    ap.add_argument("--rccl", choices=["library", "torch"], default="library",
                    help="N>1 replica exchange: through the library's own RCCL communicator (C ABI, fwgpu_dist_all_reduce_sum) or torch.distributed")
    ap.add_argument("--blocking-sync", dest="blocking_sync", action="store_true",
                    help="N>1: blocking delta all-reduce instead of the overlapped one")
    ap.add_argument("--dist-backend", dest="dist_backend", default="nccl",
                    help="torch.distributed backend; 'gloo' + --same-device lets the N>1 path be exercised on a one-GPU box")
    ap.add_argument("--same-device", dest="same_device", action="store_true", help="debug: every rank uses cuda:0")
    ap.add_argument("--library-comm", dest="library_comm", action="store_true",
                    help="use the library's own communicator (fwgpu_dist_*) whatever the torch backend: with --dist-backend gloo --same-device and "
                         "FWGPU_RCCL_LIBRARY=tests/fake_rccl/libfwgpu_fakerccl.so the whole N > 1 flow of this script runs with N processes on ONE GPU")
    ap.add_argument("--force-dist", dest="force_dist", action="store_true",
                    help="run the RCCL replica-sync path even with one rank (smoke test of the N>1 code on one GPU)")
    ap.add_argument("--no-traffic", dest="traffic", action="store_false",
                    help="skip the live HBM-traffic measurement (two short rocprofv3 --pmc child runs of this very command)")
    ap.add_argument("--curve-every", dest="curve_every", type=int, default=0,
                    help="hold-out log-loss checkpoints: a predict-only pass over the hold-out tail after every this many timed steps, queued on the "
                         "stream between steps and read after the timed region (0 = about 5 checkpoints per run; each costs ~0.3 ms of the timed wall time)")
    ap.add_argument("--target-logloss", dest="target_logloss", type=float, default=None,
                    help="seconds_to_logloss target (default: 0.985 x the loss of always predicting the hold-out's positive rate)")
    ap.add_argument("--no-cpu-baseline", dest="cpu", action="store_false")
    ap.add_argument("--no-config-e", dest="config_e", action="store_false",
                    help="skip the short config-E leg (k = 16 + 2 x 256 ReLU head, a child run) that the single-GPU --full line reports as `config_e`")
    ap.add_argument("--no-config-b", dest="config_b", action="store_false",
                    help="skip the short config-B leg (10 fields, k = 4, 22-bit tables, micro-batch 4096: a child run) that the single-GPU --full line reports as `config_b`")
    ap.add_argument("--cpu-examples", dest="cpu_examples", type=int, default=0)
    ap.add_argument("--lr", type=float, default=LR, help="learning rate of the LR and FFM blocks (default: run_one.sh's 0.025; config B: 0.1, SURVEY 8d)")
    ap.add_argument("--power-t", dest="power_t", type=float, default=POWER_T)
    ap.add_argument("--long", action="store_true",
                    help="SURVEY 8d's protocol at its stated length: 16 Mi training examples + the 262 144-example hold-out, --long-passes passes from fresh weights; "
                         "the line carries final_logloss per pass, the spread and the CPU oracle's values (sequential and 16-thread hogwild) on the same stream")
    ap.add_argument("--long-steps", dest="long_steps", type=int, default=256)
    ap.add_argument("--examples", type=int, default=0, help="--long: training examples (a multiple of the batch; 67108864 = round 6's 64 Mi protocol); overrides --long-steps")
    ap.add_argument("--long-passes", dest="long_passes", type=int, default=3)
    ap.add_argument("--store-policy", dest="store_policy", type=int, default=None, choices=[0, 1, 2, 3, 4], help="A/B: FFM row store policy (kernels.hip top); default = the build's")
    ap.add_argument("--launch-timeout", dest="launch_timeout", type=float, default=900.0,
                    help="self-launched N>1 run (no WORLD_SIZE in the environment): seconds after which the parent ends its ranks and exits non-zero")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline line does not need: the CPU baseline, the config-E / config-B / no-kept-rows legs, the "
                         "host-fed (pcie_inclusive) rate, the live HBM traffic, the measured copy peak, the CPU oracle's committed curves beside the "
                         "run's own (oracle_*) and, N>1, the other multi-GPU modes (dp_modes).  The --no-* switches above leave parts of it out; --long "
                         "is a protocol of its own and reports all of its figures either way")
    ap.add_argument("--dump-outputs", dest="dump_outputs", metavar="DIR", default=None,
                    help="after the timed steps, rank 0 replays the last step's records on a fresh model in the in-order mode and writes its predictions, "
                         "a seeded sample of its tables and a concurrent predict-only pass as DIR/<name>.npy (float32), the same every run")
    args = ap.parse_args()
    if args.dump_outputs and args.long:
        ap.error("--dump-outputs is not supported with --long")
    apply_family(args, args.family)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python3 bench.py --gpus N` as the driver types it for N = 1, with nothing else set: be the launcher
        raise SystemExit(self_launch(args))
    if args.long:
        raise SystemExit(long_protocol(args))
    if os.environ.get("FWGPU_BENCH_DEBUG"):  # where is a hung run?  Python stacks of all threads to stderr after that many seconds
        import faulthandler

        faulthandler.dump_traceback_later(float(os.environ["FWGPU_BENCH_DEBUG"]), exit=False)

    import torch
    import torch.distributed as dist

    import fwumious_wabbit_amd as fw
    from fwumious_wabbit_amd import _capi as capi

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if os.environ.get("FWGPU_BENCH_FAIL_RANK") == str(rank):  # test hook: this rank dies before the rendezvous (tests/test_gpu_scale_launch.py)
        raise SystemExit(f"rank {rank}: FWGPU_BENCH_FAIL_RANK")
    local_rank = 0 if args.same_device else int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (there is no CPU path)")
    torch.cuda.set_device(local_rank)
    use_dist = world > 1 or args.force_dist
    if args.dump_outputs and use_dist and args.dp_mode != "replica":
        raise SystemExit(f"--dump-outputs: the steps of --dp-mode {args.dp_mode} are collectives across the ranks, which one rank's model cannot replay")
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(args.dist_backend, rank=rank, world_size=world)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"

    mi = build_model_instance(fw, args, local_rank)

    def new_regressor():
        r = fw.Regressor(mi)
        if args.whole_lines is not None:
            r.set_whole_line_updates(args.whole_lines)
        if os.environ.get("FWGPU_BENCH_NO_CHAIN"):
            capi.check(capi.lib().fwgpu_debug_set_option(r.h, 3, 1))
        if args.threads or args.wgs:
            r.set_launch(args.threads, args.wgs)
        if args.max_in_flight:
            r.set_max_in_flight(args.max_in_flight)
        if args.store_policy is not None:
            r.set_store_policy(args.store_policy)
        return r

    re = new_regressor()
    fbt = fw.FeatureBufferTranslator(mi)

    sync_steps = args.sync or (args.nn_layers > 0 and args.head == "minibatch")
    if args.batch is None:
        # synchronous micro-batches with per-occurrence steps are stable up to ~1024 examples at these hyper-parameters (profiles/r02_sync_batch_stability.txt)
        args.batch = (max(64, 1024 // world) if (use_dist and args.dp_mode == "sharded") else
                      max(256, 8192 // world) if (use_dist and args.dp_mode == "sparse") else (1024 if sync_steps else 65536))
    K, W, B = args.steps, args.warmup, args.batch
    # every rank trains on its own shard of the stream: examples [rank*(W+K)*B, ...)
    t0 = time.time()
    first = rank * (W + K) * B
    recs, off = gen_records(fw, args, first, (W + K) * B)
    batches, words, blabels = [], [], []
    for s in range(W + K):
        lo, hi = s * B, (s + 1) * B
        sub = recs[int(off[lo]):int(off[hi])]
        # raw records in HBM; FeatureBufferTranslator::translate (a2) runs inside the kernel's stage phase
        batches.append(re.record_batch(fbt, sub, off[lo:hi + 1] - off[lo]))
        words.append(len(sub))
        if s == W + K - 1 and args.dump_outputs:
            last_records = (sub.copy(), off[lo:hi + 1] - off[lo])
        blabels.append(sub[(off[lo:hi] - off[lo]).astype(np.int64) + 1].astype(np.float32))
    hrecs, hoff = gen_records(fw, args, 1_000_000_000, args.holdout)  # same hold-out tail on every rank
    hbatch = re.record_batch(fbt, hrecs, hoff)
    hy = hrecs[hoff[:-1].astype(np.int64) + 1].astype(np.float32)
    # loss-vs-examples curve: hold-out passes between timed steps, each into a batch object of its own (predictions are read after the run)
    curve_every = args.curve_every or max(1, K // 5)
    curve_steps = [i for i in range(K) if (i + 1) % curve_every == 0 and i + 1 < K]
    # (checkpoints inside the timed wall time run on the first 8192 hold-out examples -- 0.3 ms each at config C; the FINAL loss is on the whole tail)
    cn = min(8192, args.holdout)
    curve_batches = {i: re.record_batch(fbt, hrecs[: int(hoff[cn])], hoff[: cn + 1]) for i in curve_steps}
    del recs
    prep_s = time.time() - t0

    stream = torch.cuda.current_stream()
    sptr = stream.cuda_stream

    def measured_copy_rate():
        """What this device's memory delivers to the plainest kernel there is, measured in this run: a 1 GiB device-to-device copy (read + write bytes over
        the time of 8 copies, HIP events).  The figure SURVEY 8d asks for next to the 8 TB/s spec: `roofline.peak_measured`."""
        try:
            n = 1 << 30
            a = torch.empty(n, dtype=torch.uint8, device="cuda")
            b = torch.empty(n, dtype=torch.uint8, device="cuda")
            a.zero_()
            for _ in range(3):
                b.copy_(a)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(8):
                b.copy_(a)
            e1.record(stream)
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / 8
            del a, b
            torch.cuda.empty_cache()
            return 2.0 * n / (ms * 1e-3) / 1e9
        except Exception:  # a side measurement
            return None

    peak_measured = measured_copy_rate() if (args.full and rank == 0 and not use_dist) else None

    # ---- N>1: replicas + delta all-reduce (local SGD: the agreed model moves by the mean of the replicas' deltas)
    # Cadence: one exchange per 32 steps (0.5 M examples per GPU, ~150 ms of training); a shorter run still times one
    # whole exchange, started at its midpoint.  Every exchange started in the timed region also lands inside it.
    sync_every = args.sync_every or (32 if K >= 48 else max(1, K // 2))
    last_sync_step = K - 1 if args.blocking_sync or K < 3 else K - 2  # an exchange started at the very last step could not overlap anything
    syncer = None
    dist_rank = None
    if use_dist:
        from fwumious_wabbit_amd.dist_sync import DeltaAllReduce

        if ((args.dist_backend == "nccl" and not args.same_device) or args.library_comm) and not args.nn_layers:
            # the library's own RCCL communicator (C ABI): rank 0 draws the id, torch.distributed is only the side channel
            from fwumious_wabbit_amd.dist import DistRank, unique_id

            # (any failure here -- no librccl for the library, an id that does not get through -- leaves the torch.distributed
            # exchange in place: a multi-GPU bench line must not die on the choice of communicator)
            try:
                box = [unique_id() if rank == 0 else None]
            except Exception as e:
                box = [None]
                print(f"[bench] library RCCL unavailable ({e!r}): torch.distributed does the exchange", file=sys.stderr)
            dist.broadcast_object_list(box, src=0)
            if box[0] is not None:
                try:
                    dist_rank = DistRank(re, box[0], rank, world)
                    ok = 1
                except Exception as e:
                    ok = 0
                    print(f"[bench] fwgpu_dist_init failed on rank {rank} ({e!r})", file=sys.stderr)
                flag = torch.tensor([ok], dtype=torch.int32, device="cuda")
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                if int(flag.item()) == 0:  # all ranks or none
                    if dist_rank is not None:
                        dist_rank.close()
                    dist_rank = None
                    if args.library_comm:
                        # --library-comm ASKED for the library's communicator: failing to get it is the run's failure, said once and at once (every rank leaves here,
                        # after the all-reduce above: nobody waits for anybody)
                        if rank == 0:
                            print("[bench] --library-comm: the library's RCCL communicator could not be created on every rank (see the ranks' messages above): no line", file=sys.stderr)
                        sys.stderr.flush()
                        os._exit(4)
        tabs = [capi.TABLE_LR, capi.TABLE_FFM_W, capi.TABLE_FFM_ACC]
        if args.nn_layers:  # the dense head is part of the replica (config E)
            tabs += [capi.TABLE_NN_W, capi.TABLE_NN_ACC]
        # zero-copy torch views of the library's tables
        syncer = DeltaAllReduce([re.table_as_torch(w) for w in tabs], overlap=not args.blocking_sync, combine=args.combine,
                                dist_rank=dist_rank if args.rccl == "library" else None)

    def sync_replicas():
        # table <- snapshot + mean_r (table_r - snapshot): every replica ends with the same tables.  Overlapped mode: land the previous exchange, start the next; RCCL runs in the background
        # while the following steps train.
        syncer.step()

    # device warm-up that touches no model state (clock ramp, page tables): predict-only passes over the hold-out batch
    for _ in range(16 if args.holdout > 65536 else 64):
        re.learn_batch(hbatch, capi.MODE_HOGWILD, False, sptr)
    torch.cuda.synchronize()
    sparse_main = use_dist and args.dp_mode == "sparse"
    peer_main = use_dist and args.dp_mode == "peer"
    sharded_main = (use_dist and args.dp_mode == "sharded") or sparse_main or peer_main  # (all: steps inside the library, no replica exchange)
    if sharded_main and dist_rank is None:
        raise SystemExit(f"--dp-mode {args.dp_mode} needs the RCCL backend (one rank per GPU) and a model without a deep head")

    split = re.split_buffers(B, 1024) if sync_steps else None

    if peer_main:
        dist_rank.peer_attach()

    def step(b):
        if peer_main:  # peer-sharded hogwild: own batch, rows in their owners' tables, no collective
            dist_rank.learn_peer_batch(fbt, b, True, sptr)
        elif sparse_main:  # row-sparse gradient buckets: full replicas, all-gather of deduplicated row gradients, one step per row
            dist_rank.learn_sparse_batch(fbt, b)
        elif sharded_main:  # owner-sharded synchronous step: all-gather records, reduce-scatter field sums, owner-side updates
            dist_rank.learn_sharded_batch(fbt, b)
        elif sync_steps:  # synchronous micro-batch on this GPU (deep head: mini-batched on the matrix cores)
            re.learn_batch_sync(b, split, capi.MODE_HOGWILD, sptr)
        else:
            re.learn_batch(b, capi.MODE_HOGWILD, True, sptr)

    for i in range(W):
        step(batches[i])
    if use_dist and W and not sharded_main:
        sync_replicas()
        syncer.finish()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * K)]
    t_start = time.perf_counter()
    for i in range(K):
        ev[2 * i].record(stream)
        step(batches[W + i])
        ev[2 * i + 1].record(stream)
        if use_dist and not sharded_main and (i + 1) % sync_every == 0 and i <= last_sync_step:
            sync_replicas()
        if i in curve_batches and not sharded_main:  # hold-out checkpoint (predict-only, main.rs:238-241), inside the wall time, outside the step's events
            re.learn_batch(curve_batches[i], capi.MODE_HOGWILD, False, sptr)
    if use_dist and not sharded_main:
        syncer.finish()  # the exchange still in flight lands INSIDE the timed region
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t_start
    if use_dist:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())

    kernel_ms = [ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(K)]
    if peer_main:
        dist_rank.gather_tables()  # (barrier inside) every rank gets the whole model back for the hold-out pass
    elif sharded_main:  # the step runs on the library's own stream and is host-synchronous: the step time is the wall time
        kernel_ms = [1e3 * elapsed / K] * K
        if sparse_main:
            rows_f, rows_l = dist_rank.sparse_last_rows()
            lb = batches[W + K - 1]
            sparse_exchange = {"ffm_occurrences": int(lb.n_ffm), "ffm_bucket_rows": rows_f, "lr_occurrences": int(lb.n_lr), "lr_bucket_entries": rows_l,
                               "bytes_sent_per_example": (rows_f * (args.fields * args.k * 4 + 4) + rows_l * 8) / B,
                               "what": "last timed step of rank 0: occurrences (entries of the micro-batch) vs deduplicated bucket rows put on the wire"}
        else:
            dist_rank.gather_tables()  # every rank gets the whole model back for the hold-out pass
    if args.dump_outputs and rank == 0:
        rd = new_regressor()
        dump_outputs(rd, capi, fbt, *last_records, sync_steps, sptr, args.dump_outputs, args.seed)
        rd.close()
    avg_kernel_ms = float(np.mean(kernel_ms))
    alg_bytes = float(np.mean([algorithmic_bytes(args, batches[W + i], words[W + i]) for i in range(K)]))

    # ---- final hold-out log-loss (main.rs:238-241 --holdout_after semantics: predicted, never learned)
    re.learn_batch(hbatch, capi.MODE_HOGWILD, False, sptr)
    p_final = hbatch.predictions(sptr)
    final_ll = logloss(p_final, hy)
    final_ll_cn = logloss(p_final[:cn], hy[:cn])
    # time to quality (benchmark/calc_loss.py:5-25 on the hold-out tail): loss after n learned examples (warm-up steps learn too), and the
    # wall time this run needs to reach a stated target at its measured rate
    prior_ll = logloss(np.full(len(hy), float(np.mean(hy == 1)), dtype=np.float64), hy)
    curve = {}
    if not sharded_main:
        for i in curve_steps:
            curve[(W + i + 1) * B * world] = logloss(curve_batches[i].predictions(sptr), hy[:cn])
    curve[(W + K) * B * world] = final_ll_cn
    # progressive validation on the training stream itself (the prediction every example got BEFORE it was learned), per timed step
    progressive = [] if sharded_main else [round(logloss(batches[W + i].predictions(sptr), blabels[W + i]), 5) for i in range(K)]
    target_ll = args.target_logloss if args.target_logloss is not None else 0.985 * prior_ll
    reached = [n for n, v in sorted(curve.items()) if v <= target_ll]  # (on the checkpoints' prefix of the hold-out)
    # guard: a saturated sigmoid (|logit| > 50, block_loss_functions.rs:125-133) skips the update; report how many of
    # the last timed step's examples were in that state (healthy training: 0)
    p_last = batches[W + K - 1].predictions(sptr)
    saturated = float(np.mean((p_last < 1e-20) | (p_last > 1.0 - 1e-7)))

    # ---- secondary figure, never `value`: the same workload fed from HOST memory through the HogwildTrainer replacement
    # (fwgpu_digest_records: pinned staging, PCIe, device-side translation + learn; hogwild.rs:51-60's boundary)
    pcie = None
    if args.full and rank == 0 and world == 1 and not use_dist and not sync_steps and args.cpu:
        try:
            n_p = 4 * min(B, 65536)
            precs, poff = gen_records(fw, args, 3_000_000_000, n_p)
            tr = fw.HogwildTrainer(re, mi, micro_batch=16384)
            n_w = min(n_p, 2 * 16384)  # warm-up: both staging slots of the trainer allocated at their full size (pinned memory, first use)
            tr.digest_records(precs[: int(poff[n_w])], poff[: n_w + 1])
            tr.block_until_workers_finished()
            tp = time.perf_counter()
            tr.digest_records(precs, poff)
            tr.block_until_workers_finished()
            dtp = time.perf_counter() - tp
            tr.close()
            pcie = {"value": n_p / dtp, "unit": "examples/sec", "examples": n_p, "megabytes": precs.nbytes / 1e6,
                    "what": "records in pageable host memory -> fwgpu_digest_records (pinned staging, PCIe, 16 384-example micro-batches) -> learned"}
            del precs
        except Exception as e:
            pcie = {"value": None, "what": f"failed: {e!r}"}

    # ---- the OTHER multi-GPU modes, timed on short legs of their own AFTER the line's figures are settled (a replica run reports
    # them as dp_modes; the owner-sharded step leaves every rank with only its own range current, so it comes last).  They have
    # never run on more than one GPU: a watchdog prints the line without them if they do not come back.
    def run_other_modes():
        if os.environ.get("FWGPU_BENCH_HANG_OTHER_MODES"):  # (tests: a leg that never comes back -- the watchdog's business)
            time.sleep(10 ** 6)
        Kp, Bp = min(K, 16), max(256, 8192 // world)  # global micro-batch of 8192 examples: the summed-gradient rule's stable range
        precs_, poff_ = gen_records(fw, args, 2_500_000_000 + rank * Kp * Bp, Kp * Bp)
        pb = [re.record_batch(fbt, precs_[int(poff_[j * Bp]):int(poff_[(j + 1) * Bp])], poff_[j * Bp:(j + 1) * Bp + 1] - poff_[j * Bp]) for j in range(Kp)]
        dist_rank.learn_sparse_batch(fbt, pb[0])
        torch.cuda.synchronize()
        dist.barrier()
        ts = time.perf_counter()
        for j in range(Kp):
            dist_rank.learn_sparse_batch(fbt, pb[j])
        torch.cuda.synchronize()
        dist.barrier()
        tsp = torch.tensor([time.perf_counter() - ts], dtype=torch.float64, device="cuda")
        dist.all_reduce(tsp, op=dist.ReduceOp.MAX)
        sp_rows = dist_rank.sparse_last_rows()
        for x in pb:
            x.close()
        del precs_
        Ks, Bs = min(K, 48), max(64, 1024 // world)  # global synchronous micro-batch of 1024 examples (2048 is already marginal, see --batch)
        srecs, soff = gen_records(fw, args, 2_000_000_000 + rank * Ks * Bs, Ks * Bs)
        sb = [re.record_batch(fbt, srecs[int(soff[j * Bs]):int(soff[(j + 1) * Bs])], soff[j * Bs:(j + 1) * Bs + 1] - soff[j * Bs]) for j in range(Ks)]
        dist_rank.learn_sharded_batch(fbt, sb[0])  # warm-up: buffers, communicator channels
        torch.cuda.synchronize()
        dist.barrier()
        ts = time.perf_counter()
        for j in range(Ks):
            dist_rank.learn_sharded_batch(fbt, sb[j])
        torch.cuda.synchronize()
        dist.barrier()
        tsh = torch.tensor([time.perf_counter() - ts], dtype=torch.float64, device="cuda")
        dist.all_reduce(tsh, op=dist.ReduceOp.MAX)
        for x in sb:
            x.close()
        # The streaming owner-side apply (owner-sharded tables, every rank's fused kernel pushes gradient rows to the rows' owners, whose consumer workgroups run
        # the optimizer while the sources push; no collective inside a step) -- the one mode designed to SCALE: global steps of 65 536 examples from host records.
        # Last: it maps the peers' tables and regions (IPC) and leaves every rank with its own range current.
        owner_stream = None
        try:
            Ko, Bo = min(K, 8), max(1024, 65536 // world)
            orecs, ooff = gen_records(fw, args, 3_000_000_000 + rank * (Ko + 1) * Bo, (Ko + 1) * Bo)
            dist_rank.set_mode(capi.MODE_HOGWILD)
            dist_rank.owner_stream_attach()
            cut = lambda j: (orecs[int(ooff[j * Bo]):int(ooff[(j + 1) * Bo])], ooff[j * Bo:(j + 1) * Bo + 1] - ooff[j * Bo])  # noqa: E731
            dist_rank.learn_owner_stream(fbt, *cut(0))  # warm-up
            torch.cuda.synchronize()
            dist.barrier()
            ts = time.perf_counter()
            for j in range(1, Ko + 1):
                dist_rank.learn_owner_stream(fbt, *cut(j))
            torch.cuda.synchronize()
            dist.barrier()
            tos = torch.tensor([time.perf_counter() - ts], dtype=torch.float64, device="cuda")
            dist.all_reduce(tos, op=dist.ReduceOp.MAX)
            owner_stream = {"value": world * Ko * Bo / float(tos.item()), "unit": "examples/sec", "steps": Ko, "examples_per_step_per_gpu": Bo,
                            "ms_per_step": 1e3 * float(tos.item()) / Ko,
                            "what": "owner-sharded tables, streaming owner-side apply (fwgpu_dist_learn_owner_stream): hogwild across the GPUs -- gradient rows pushed into circular "
                                    "regions in the owner's memory and applied there while the sources run; no collective inside a step; records come from host memory (PCIe-inclusive)"}
        except Exception as e:  # (a side leg: a collective that hangs instead is the watchdog's business)
            owner_stream = {"value": None, "error": repr(e)[:300]}
        return {"replica": "the timed mode of this line", "owner_stream": owner_stream,
                "sparse": {"value": world * Kp * Bp / float(tsp.item()), "unit": "examples/sec", "steps": Kp,
                           "examples_per_step_per_gpu": Bp, "ms_per_step": 1e3 * float(tsp.item()) / Kp,
                           "bucket_rows_last_step": {"ffm": sp_rows[0], "lr": sp_rows[1]},
                           "bytes_sent_per_example": (sp_rows[0] * (args.fields * args.k * 4 + 4) + sp_rows[1] * 8) / Bp,
                           "what": "full replicas, per-micro-batch all-gather of deduplicated row gradients, every rank applies all of "
                                   "them: one summed-gradient AdaGrad step per row (fwgpu_dist_learn_sparse_batch)"},
                "sharded": {"value": world * Ks * Bs / float(tsh.item()), "unit": "examples/sec", "steps": Ks,
                            "examples_per_step_per_gpu": Bs, "ms_per_step": 1e3 * float(tsh.item()) / Ks,
                            "what": "owner-sharded tables, synchronous step of n_gpus x examples_per_step_per_gpu examples: all-gather of "
                                    "records, reduce-scatter + all-gather of field sums, owner-side AdaGrad (fwgpu_dist_learn_sharded_batch)"}}

    # HBM traffic per launch: PMC counters cannot be read from inside this process; the figure is the rocprofv3
    # measurement of this very command (separate --pmc FETCH_SIZE / WRITE_SIZE passes, gfx950 x2 correction on the
    # read side) committed under profiles/, reported only when the run uses the profiled configuration.
    traffic, traffic_src = None, None
    if args.full and args.traffic and rank == 0 and world == 1 and not use_dist:
        traffic, traffic_src = measure_traffic(args)

    if rank == 0:
        oracle = {}
        if args.full:
            oc = oracle_reference_curves(args, world) if not (sync_steps or use_dist) or (args.nn_layers and args.head == "exact" and not use_dist) else {"seq": {}, "hog16": []}
            oracle_curve = oc["seq"]
            same_stream = not (sync_steps or use_dist) or (args.nn_layers and args.head == "exact" and not use_dist)
            occ = oracle_reference_curves(args, world, cn) if same_stream else {"seq": {}, "hog16": []}  # ... on the checkpoints' prefix of the hold-out

            def hog16_at(n, which=None):  # the 16-thread hogwild oracle's runs at n examples (None where not precomputed)
                v = [c.get(n) for c in (which or oc)["hog16"] if c.get(n) is not None]
                return v or None
            oracle = {
                # the sequential CPU oracle (= the reference's single-thread algorithm) on the same stream, same hold-out tail, same number of examples:
                # null where it was not precomputed (tests/golden/bench_oracle_curve_seq.json: every multiple of 65 536 up to 3.4 M, every 262 144 up to 16.8 M)
                "oracle_logloss_after_examples": {str(n): occ["seq"].get(n) for n, v in sorted(curve.items())},
                "oracle_final_logloss": oracle_curve.get((W + K) * B * world),
                # ... and the oracle in the reference's 16-thread hogwild mode (hogwild.rs:89-103), every committed run
                "oracle_hogwild16_logloss_after_examples": {str(n): hog16_at(n, occ) for n, v in sorted(curve.items())},
                "oracle_hogwild16_final_logloss": hog16_at((W + K) * B * world),
            }
        achieved = alg_bytes / (avg_kernel_ms * 1e-3) / 1e9
        out = {
            "metric": "examples/sec + final log-loss, 30-field k=8 FFM, at 1/2/4/8 MI355X",
            "value": world * K * B / elapsed,
            "unit": "examples/sec",
            "n_gpus": world,
            # ranks of the job as the library's RCCL communicator counts them (ncclCommCount), not WORLD_SIZE; null when no communicator exists (N = 1)
            "rccl_ranks": (dist_rank.comm_count() if dist_rank is not None else None),
            "steps": K,
            "warmup": W,
            "ms_per_step": 1e3 * elapsed / K,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "table_placement": dict(zip(("candidates_tried", "pair_probe_ms_kept", "pair_probe_ms_slowest"), re.placement())),
            "final_logloss": final_ll,
            # what "learned" means on this hold-out tail: the loss of always predicting its positive rate (the untrained model reads ln 2)
            "holdout_prior_logloss": prior_ll,
            # hold-out checkpoints during the run: on the FIRST `curve_holdout_examples` examples of the hold-out tail (cheap enough to sit inside the timed wall time)
            "curve_holdout_examples": cn,
            "logloss_after_examples": {str(n): v for n, v in sorted(curve.items())},
            **oracle,  # (--full)
            "progressive_logloss_per_step": progressive,
            "seconds_to_logloss": {"target": target_ll, "examples": reached[0] if reached else None,
                                   "seconds": (reached[0] / (world * K * B / elapsed)) if reached else None,
                                   "what": "first hold-out checkpoint at or below the target; seconds = examples learned so far (warm-up included) / this run's examples/sec"},
            "saturated_fraction_last_step": saturated,
            "config": {
                "hyperparameters": f"AdagradLUT lr={args.lr} power_t={args.power_t} init_acc_gradient={INIT_ACC}" + (" (run_one.sh)" if (args.lr, args.power_t) == (LR, POWER_T) else ""),
                "workload": f"BASELINE.json configs[{4 if args.nn_layers else 1 if (args.fields, args.k, args.ffm_bits) == (10, 4, 22) else 2}]: synthetic {args.fields}-field k={args.k} FFM + LR"
                            + (f" + deep head {args.nn_layers}x{args.nn_width} ReLU (topology one, " + ("mini-batched on MFMA: summed dense gradients, one step per batch)" if sync_steps else "per-example updates)") if args.nn_layers else "") + ", "
                            f"{args.ffm_bits}-bit FFM hash, {args.bits}-bit LR hash, ~{int(args.fields * (1 + args.mean_extra))} nnz/example, "
                            f"AdagradLUT, fused learn (record translation + forward + sigmoid/log-loss + AdaGrad scatter-update)",
                "examples_per_step_per_gpu": B,
                "global_batch": B * world,
                "mode": ("synchronous micro-batches (every example sees the batch-start weights; FWD / MID / head on MFMA / UPD kernels)" if sync_steps
                         else "hogwild (device-wide concurrent examples, racy RMW; device-scope loads and accumulator stores, weight rows stored write-back through L2; store policy "
                              + (str(args.store_policy) if args.store_policy is not None else "4 (hot rows' accumulators: one example in eight adds eight times its g^2 with device-scope float atomics instead of every example storing the row)") + ")"),
                "parallelism": ("1 GPU" if not use_dist else
                                f"dp{world} peer: tables sharded by owner, every rank's fused hogwild kernel reaches each row in its owner's memory (IPC-mapped tables over xGMI), "
                                f"no collective per step, {world} x {B} examples per step" if peer_main else
                                f"dp{world} sparse: full replicas, per-micro-batch all-gather of deduplicated row gradients of {world} x {B} examples, "
                                f"one summed-gradient AdaGrad step per row on every replica, RCCL inside the library" if sparse_main else
                                f"dp{world} sharded: owner-sharded tables, synchronous step of {world} x {B} examples (records all-gathered, field sums "
                                f"reduce-scattered / all-gathered, owner-side AdaGrad), RCCL inside the library" if sharded_main else
                                f"dp{world}: replicas, {'blocking' if args.blocking_sync else 'overlapped'} RCCL all-reduce ({'library communicator, C ABI' if syncer.dist_rank is not None else 'torch.distributed'}) "
                                f"of the replicas' {args.combine} delta, {syncer.bytes_per_sync() / 1e9:.2f} GB every "
                                f"{sync_every} steps ({syncer.n_syncs} syncs incl. warmup)"),
                "holdout_examples": args.holdout,
                "prep_seconds": prep_s,
            },
            "roofline": {
                "bound": "hbm",
                "kernel": ("fw_example_kernel<4, AdagradLUT, coherent, peer-sharded> (generic kernel with the owner lookup, system-scope row accesses)" if peer_main else
                           "FWD / MID / " + ("head GEMMs (v_mfma_f32_32x32x2_f32) / " if args.nn_layers else "") + "UPD kernels of the synchronous micro-batch (generic row kernel)"
                           if sync_steps or sharded_main else
                           "fw_example_kernel_r<AdagradLUT, coherent, MAXR=20, duplicate-row chains, store policy 4> (2 workgroups x 512 threads per CU at 128 VGPRs; 20 rows per wave kept from the gather in registers + 3 in LDS and written back as w_gather - step by a pipelined update; accumulators of hot rows: one example in eight ADDS eight times its g^2 with device-scope float atomics instead of every example storing the row -- fewer accumulator writes than `frac`'s algorithmic count, see frac_traffic; whole-line row accesses only when w and acc contend for one memory region)"
                           if args.k % 4 == 0 and args.fields * args.k <= 256 and not args.nn_layers else
                           "fw_example_kernel_r<AdagradLUT, coherent, MAXR=0, duplicate-row chains, NC=2> (two 16-byte chunks per lane and row; 2 workgroups x 512 threads per CU)"
                           if args.k % 4 == 0 and args.fields * args.k <= 512 and 256 % args.k == 0 and not args.nn_layers else
                           "fw_example_kernel_r<AdagradLUT, coherent, MAXR=0, duplicate-row chains, NC=2, NN> (the per-example deep head as a phase of the large-table kernel: 2 workgroups x 512 threads per CU; FWGPU_NN_V2=0: the generic kernel, one 1024-thread workgroup per CU)"
                           if args.nn_layers and args.k % 4 == 0 and 256 < args.fields * args.k <= 512 and 256 % args.k == 0 and args.head == "exact" and os.environ.get("FWGPU_NN_V2", "1") != "0" else
                           "fw_example_kernel<VEC=4, AdagradLUT, coherent> (generic rows, duplicate-row chains" + (" + per-example deep head)" if args.nn_layers else ")")),
                "achieved": achieved,
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS,
                # (frac is against the 8 TB/s spec; this is what a 1 GiB device-to-device copy reaches on this very device in this run, read + write bytes)
                "peak_measured": peak_measured,
                "frac_of_peak_measured": (achieved / peak_measured) if peak_measured else None,
                "traffic": traffic,
                "traffic_source": traffic_src,
                # what the memory system did: measured bytes (FETCH x 2 + WRITE of the launches from the 16th on) / this run's average launch time / peak.  `frac` counts
                # ALGORITHMIC bytes (every row's w and acc read and written once per occurrence); store policy 4 issues fewer accumulator writes than that on
                # hot rows (one example in eight adds eight times its g^2), so the two differ by what thinning skips -- plus what the caches absorb on the head rows.
                "frac_traffic": (traffic / (avg_kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if traffic else None,
                "traffic_over_algorithmic": (traffic / alg_bytes) if traffic else None,
                "pattern_ceiling_note": "profiles/r02_rowceil.txt (tools/rowceil.hip): read w+acc rows and write both back as whole lines = 0.62 of the 8 TB/s peak; this kernel on UNIFORM ids "
                                        "(every access a miss of every cache): 0.64 (profiles/r05_skew_sweep.txt) -- what is lost on the bench's Zipf stream is write-through serialisation on "
                                        "hot accumulator lines (L2 tag stalls 6.4x, profiles/r05_skew_pmc_counters.txt), which store policies 3 / 4 thin",
                "algorithmic_bytes_per_launch": alg_bytes,
                "avg_launch_ms": avg_kernel_ms,
                "launch_ms_min_median_max": [float(np.min(kernel_ms)), float(np.median(kernel_ms)), float(np.max(kernel_ms))],
            },
        }
        if use_dist:
            nb = batches[W]
            tb = 8.0 * ((1 << args.ffm_bits) + args.fields * args.k) + 8.0 * (1 << args.bits)
            out["link_bytes_per_example"] = link_bytes_per_example(args, world, nb.n_ffm / max(nb.n, 1), nb.n_lr / max(nb.n, 1), words[W] / max(nb.n, 1),
                                                                   sync_every, tb)
        if args.full and args.config_e and world == 1 and not use_dist and not sync_steps and not args.nn_layers and args.k == 8 and args.cpu:
            # (released first: the child allocates its own 28-bit tables)
            out["config_e"] = "pending"
        if pcie is not None:
            out["pcie_inclusive"] = pcie
        if sparse_main:
            out["sparse_exchange"] = sparse_exchange
        if args.full and args.cpu and world == 1:
            n_cpu = args.cpu_examples or 20000
            try:
                out["cpu_baseline"] = cpu_baseline(args, n_cpu)
            except Exception as e:  # the baseline is a reported side figure; never lose the GPU line over it
                out["cpu_baseline"] = {"value": None, "unit": "examples/sec", "cores": os.cpu_count(), "kind": "port",
                                       "sample": f"failed: {e!r}"}
    else:
        out = None
    if args.full and use_dist and dist_rank is not None and not sharded_main and args.other_modes:
        import threading

        def bail():  # the legs hang (a collective that never completes): the line as it stands, then out -- on every rank
            if out is not None:
                out["dp_modes"] = {"replica": "the timed mode of this line", "error": f"the sparse / sharded legs did not finish within {args.other_modes_timeout} s"}
                sys.stdout.flush()
                print(json.dumps(out), flush=True)
            os._exit(3)  # a hung collective is a failure: the line is out, the exit status says so (no re-exec, no restart from here)

        dog = threading.Timer(args.other_modes_timeout, bail)
        dog.daemon = True
        dog.start()
        try:
            dp_modes = run_other_modes()
        except Exception as e:  # a reported side figure: never lose the line over it
            dp_modes = {"replica": "the timed mode of this line", "error": f"failed: {e!r}"}
        dog.cancel()
        if out is not None:
            out["dp_modes"] = dp_modes
    if out is not None and out.get("config_e") == "pending":
        for bb in batches:
            bb.close()
        hbatch.close()
        re.close()
        out["config_e"] = config_e_leg(args)
        if args.config_b:
            out["config_b"] = config_b_leg(args)
            out["no_kept_rows"] = no_kept_rows_leg(args, K, W)
    result_line = json.dumps(out) if out is not None else None
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    # RCCL prints a version banner through C stdio; flush it first so that the JSON line is the LAST line on stdout
    try:
        import ctypes

        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    sys.stdout.flush()
    if result_line is not None:
        print(result_line, flush=True)


if __name__ == "__main__":
    main()
