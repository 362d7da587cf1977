"""bench.py --dump-outputs: after the timed steps the last step's records run through the same learn entry on a fresh model in the in-order
mode, then through a predict-only concurrent launch on that model; the predictions of both and the tables the step updated (whole, or a seeded
sample of a large one) are written as float32 .npy files within 64 MiB -- the same every run on the same arguments; --steps sets the number of
timed steps and the line carries ms_per_step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_dump(out):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    # LR table of 2 x 2^18 floats: dumped whole; FFM tables of 2^21 + 240 floats: sampled (256 of their 512 blocks)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "4096", "--bits", "18", "--ffm-bits", "21",
                        "--holdout", "1024", "--no-cpu-baseline", "--no-traffic", "--no-config-e", "--no-config-b", "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    return {f[:-4]: np.load(out / f) for f in os.listdir(out)}


def test_dump_outputs_writes_the_last_steps_predictions_and_tables_the_same_every_run(tmp_path):
    a = _bench_dump(tmp_path / "a")
    assert set(a) == {"inorder_predictions", "concurrent_predictions", "inorder_lr_table", "inorder_ffm_weights_sample", "inorder_ffm_accumulators_sample"}, sorted(a)
    assert all(v.dtype == np.float32 and v.ndim == 1 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in ("inorder_predictions", "concurrent_predictions"):
        pr = a[k]
        assert pr.shape == (4096,) and np.all((pr > 0) & (pr < 1)) and pr.std() > 0, k
    assert a["inorder_lr_table"].shape == (2 << 18,) and a["inorder_ffm_weights_sample"].shape == (256 * 4096,) == a["inorder_ffm_accumulators_sample"].shape
    assert all(np.isfinite(v).all() for v in a.values())
    b = _bench_dump(tmp_path / "b")  # a second run on the same arguments: the same outputs, bit for bit
    assert set(b) == set(a) and all(np.array_equal(a[k], b[k]) for k in a), [k for k in a if not np.array_equal(a[k], b.get(k))]
