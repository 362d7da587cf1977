"""Progressive and hold-out loss scored on the device (csrc/metrics.hip; fwgpu_debug_metrics, fwgpu_batch_metrics, fwgpu_trainer_set_metrics /
fwgpu_trainer_metrics) against the float64 yardstick tests/metrics_ref.py, whose docstring derives the tolerance: counts and histograms equal,
every f64 sum within (n + 4) * 2^-52, twice that between two device runs.

The trainer tests keep ONE example in flight: a hogwild launch is then the in-order walk, so a twin regressor driven by hand through
fwgpu_record_batch_create + fwgpu_learn_batch with the trainer's cuts makes the trainer's predictions bit for bit, and metrics_ref on the twin's
predictions is the expectation.  The stream: 1 500 lines of VW text (a handful with an importance, three without a label, one the device parser
hands to the host), parsed once by the host parser; examples from number 1 001 on are held out."""
import ctypes as C
import random

import numpy as np
import pytest

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import capi
from fwumious_wabbit_amd.feed import DeviceVowpalParser, VowpalParser, VwNamespaceMap
from helpers import make_pair
from test_gpu_textparse import CSV
from test_gpu_trainer_text import HOST_WEIGHT, _mi

import metrics_ref as mr

pytestmark = pytest.mark.gpu

TABLES = (capi.TABLE_LR, capi.TABLE_FFM_W, capi.TABLE_FFM_ACC)
N, MB, WINDOW, HOLDOUT = 1500, 64, 37, 1001
IMPORTANCE = {10: "0.25", 200: "8", 640: "2", 998: "0.5", 1003: "4", 1400: "0.25"}
UNLABELLED = (77, 990, 1234)
HOST_LINE = 300


# ---------------------------------------------------------------- 1. the kernel alone
SPECIAL = np.array([0.0, 1.0, 1e-20, 1.0 - 2.0 ** -24, 1e-40, np.nan, np.inf, -np.inf, 1 / 256, 37 / 256, 128 / 256, 255 / 256, 2 / 256, -0.25, 1.5,
                    3e38, 254 / 256], dtype=np.float32)


def _kernel_case(n, window):
    rng = np.random.default_rng(1000 * n + window)
    pred = rng.random(n, dtype=np.float32)
    k = len(pred[::3])
    pred[::3] = SPECIAL[(np.arange(k) + window) % len(SPECIAL)]
    label = rng.choice(np.array([0.0, 1.0, 255.0], dtype=np.float32), size=n, p=[0.45, 0.45, 0.1])
    imp = rng.choice(np.array([0.25, 0.5, 1.0, 1.0, 1.0, 2.0, 3.5, 8.0], dtype=np.float32), size=n)
    learned = rng.random(n) < 0.6
    first = 3 * window + window // 2 + 1  # the first window is entered mid-way (a window of one has no middle)
    return pred, label, imp, learned, first


@pytest.mark.parametrize("window", [1, 37, 5000])
@pytest.mark.parametrize("n,launch", [(1, 0), (63, 0), (64, 0), (65, 0), (4099, 0), (4099, 1000)])
def test_kernel_alone(n, launch, window):
    pred, label, imp, learned, first = _kernel_case(n, window)
    assert np.isfinite(SPECIAL[4]) and 0 < SPECIAL[4] < np.finfo(np.float32).tiny  # the denormal
    rows, lt, ht = fw.debug_metrics(pred, label, imp, learned, first, window, launch=launch)
    want = mr.windows(pred, label, imp, learned, first, window)
    assert len(want) == (first + n - 2) // window - (first - 1) // window + 1
    mr.check_rows(rows, want)
    wl, wh = mr.totals(pred, label, imp, learned)
    mr.check_total(lt, wl, "learned total")
    mr.check_total(ht, wh, "held-out total")
    if n >= 63:
        assert int(lt["sums"]["n_bad"]) + int(ht["sums"]["n_bad"]) > 0 and int(lt["sums"]["n_unlabelled"]) + int(ht["sums"]["n_unlabelled"]) > 0
        assert lt["hist"][:, 255].sum() + ht["hist"][:, 255].sum() > 0 and lt["hist"][:, 0].sum() + ht["hist"][:, 0].sum() > 0


@pytest.mark.parametrize("window", [37, 5000])
@pytest.mark.parametrize("kind", [True, False], ids=["learned", "held-out"])
def test_kernel_alone_one_kind(kind, window):
    """examples of one kind, as a trainer's launch has them: a workgroup whose examples all fall into one window adds that row once, from its LDS
    totals (window 5000: most workgroups, and one that straddles number 20 000); with windows of 37 no workgroup does"""
    pred, label, imp, _, first = _kernel_case(4099, window)
    learned = np.full(4099, kind)
    rows, lt, ht = fw.debug_metrics(pred, label, imp, learned, first, window)
    mr.check_rows(rows, mr.windows(pred, label, imp, learned, first, window))
    wl, wh = mr.totals(pred, label, imp, learned)
    mr.check_total(lt, wl, "learned total")
    mr.check_total(ht, wh, "held-out total")
    assert int((ht if kind else lt)["sums"]["n"]) == 0 and int((lt if kind else ht)["sums"]["n"]) > 3000


# ---------------------------------------------------------------- 2. one batch
def test_batch_metrics_entry_and_record_batches():
    mi, _, _ = make_pair(6, 4, 12, 12, fw.Optimizer.AdagradLUT)
    recs, off = fw.synth_records(6, 1.0, 1.1, 1000, 0.3, 99, 0, 300)
    re = fw.Regressor(mi)
    fbt = fw.FeatureBufferTranslator(mi)
    warm = re.record_batch(fbt, recs, off)
    re.learn_batch(warm, capi.MODE_SEQUENTIAL, True)  # (predictions that differ from example to example)
    warm.close()
    recs = recs.copy()
    first_word = off[:-1].astype(np.int64)
    for i in (3, 150, 299):
        recs[first_word[i] + 1] = 255  # NO_LABEL
    for i, v in ((0, 0.25), (64, 8.0), (150, 2.0), (255, 3.5)):
        recs[first_word[i] + 2] = np.float32(v).view(np.uint32)
    label = recs[first_word + 1].astype(np.float32)
    imp = recs[first_word + 2].copy().view(np.float32)
    got = {}
    for kind in ("entries", "records"):
        b = re.batch_from_records(fbt, recs, off) if kind == "entries" else re.record_batch(fbt, recs, off)
        re.learn_batch(b, capi.MODE_HOGWILD, False)
        pred = b.predictions()
        assert len(np.unique(pred)) > 100
        for first, n, learned in ((0, 300, False), (37, 200, True), (299, 1, False)):
            s, h = b.metrics(first, n, learned)
            sl = slice(first, first + n)
            mr.check_sums(s, mr.sums(pred[sl], label[sl], imp[sl]), f"{kind} {first}+{n}")
            assert np.array_equal(h, mr.hist(pred[sl], label[sl])) and int(h.sum()) == int(s["n"])
            got[kind, first] = (s, h, pred)
        with pytest.raises(capi.FwgpuError) as ei:
            b.metrics(200, 101)
        assert ei.value.code == capi.ERR_RANGE
        b.close()
    re.close()
    for first in (0, 37, 299):
        (se, he, pe), (sr, hr, pr) = got["entries", first], got["records", first]
        assert np.array_equal(pe, pr)
        assert [int(se[f]) for f in mr.COUNTS] == [int(sr[f]) for f in mr.COUNTS] and np.array_equal(he, hr)
    assert int(got["records", 0][0]["n"]) == 297 and int(got["records", 0][0]["n_unlabelled"]) == 3


# ---------------------------------------------------------------- 3. the trainer
def _stream_lines(n=N):
    rng = random.Random(5)
    lines = []
    for i in range(n):
        head = rng.choice(["1", "-1"]) + (" " + IMPORTANCE[i] if i in IMPORTANCE else "")
        toks = ["|A " + " ".join("a%d" % rng.randrange(30) for _ in range(rng.choice([1, 1, 2])))]
        for ns in ("Bb", "C", "Ddd", "E"):
            if rng.random() < 0.8:
                toks.append("|" + ns + " " + " ".join("%s%d" % (ns[0].lower(), rng.randrange(30)) for _ in range(rng.choice([1, 1, 2]))))
        if rng.random() < 0.5:
            toks.append("|F ab" + rng.choice(["0.5", "1.25", "2"]))
        lines.append((" ".join(toks)) if i in UNLABELLED else head + " " + " ".join(toks))
    if n > HOST_LINE:
        lines[HOST_LINE] = HOST_WEIGHT
    return lines


def _text(lines):
    return ("\n".join(lines) + "\n").encode()


def _cuts(n, mb, holdout_after):
    """the launches of the host-fed trainer: micro-batches of mb, none across the hold-out boundary -> [(begin, end, learned)]"""
    edge = min(n, holdout_after - 1) if holdout_after else n
    out = [(a, min(a + mb, edge), True) for a in range(0, edge, mb)]
    return out + [(a, min(a + mb, n), False) for a in range(edge, n, mb)]


def _checksums(re):
    return [re.table_checksum(t) for t in TABLES]


def _twin(mi, recs, off, cuts):
    """the same stream through fwgpu_record_batch_create + fwgpu_learn_batch, cut alike -> (predictions, learned flags, checksums, routes)"""
    re = fw.Regressor(mi)
    re.set_max_in_flight(1)
    fbt = fw.FeatureBufferTranslator(mi)
    pred, learned, routes = [], [], []
    for a, e, upd in cuts:
        w0 = int(off[a])
        b = re.record_batch(fbt, recs[w0:int(off[e])], off[a:e + 1] - off[a])
        re.learn_batch(b, capi.MODE_HOGWILD, upd)
        routes.append(re.last_route())
        pred.append(b.predictions())
        learned += [upd] * (e - a)
        b.close()
    sums = _checksums(re)
    re.close()
    return np.concatenate(pred), np.array(learned), sums, routes


class TrainerRun:
    def __init__(self, mi, recs=None, off=None, mb=MB, window=WINDOW, holdout_after=HOLDOUT, call=None, in_flight=1, text=None, dparser=None):
        re = fw.Regressor(mi)
        if in_flight:
            re.set_max_in_flight(in_flight)
        tr = fw.Trainer(re, mi, micro_batch=mb)
        if holdout_after:
            tr.set_holdout(holdout_after)
        if window is not None:
            tr.set_metrics(window)
        if text is not None:
            n, used, rc = tr.digest_text_device(dparser, text)
            assert (used, rc) == (len(text), capi.OK)
        else:
            n = len(off) - 1
            call = call or n
            for a in range(0, n, call):
                tr.digest_records(recs, off[a:min(a + call, n) + 1])
        tr.block_until_workers_finished()
        self.n = n
        self.rows, self.learned, self.held_out = tr.metrics()
        self.preds = tr.predictions()
        self.sums = _checksums(re)
        tr.close()
        re.close()


@pytest.fixture(scope="module")
def stream():
    """the text, its records, the twin's predictions with the expectation they give, and the host-fed trainer's run -- made once, read by every test"""
    vw = VwNamespaceMap(CSV)
    host = VowpalParser(vw)
    lines = _stream_lines()
    text = _text(lines)
    recs, off, used, rc = host.parse_buffer(text)
    host.close()
    assert rc == capi.OK and used == len(text) and len(off) == N + 1
    first_word = off[:-1].astype(np.int64)
    label = recs[first_word + 1].astype(np.float32)
    imp = recs[first_word + 2].copy().view(np.float32)
    assert sorted(np.flatnonzero(label == 255).tolist()) == sorted(UNLABELLED) and set(np.unique(label)) == {0.0, 1.0, 255.0}
    assert sorted(np.flatnonzero(imp != 1).tolist()) == sorted(IMPORTANCE) and imp.min() == 0.25 and imp.max() == 8
    mi = _mi()
    pred, learned, sums, routes = _twin(mi, recs, off, _cuts(N, MB, HOLDOUT))
    assert learned.sum() == HOLDOUT - 1 and set(routes) == {capi.ROUTE_FUSED}

    class S:
        pass

    s = S()
    s.vw, s.mi, s.lines, s.text, s.recs, s.off, s.label, s.imp = vw, mi, lines, text, recs, off, label, imp
    s.pred, s.learned, s.twin_sums = pred, learned, sums
    s.want_rows = mr.windows(pred, label, imp, learned, 1, WINDOW)
    s.want_totals = mr.totals(pred, label, imp, learned)
    s.host = TrainerRun(mi, recs, off)
    return s


def test_trainer_host_fed_in_order(stream):
    s, run = stream, stream.host
    assert len(run.rows) == (N + WINDOW - 1) // WINDOW
    mr.check_rows(run.rows, s.want_rows)
    mr.check_total(run.learned, s.want_totals[0], "learned total")
    mr.check_total(run.held_out, s.want_totals[1], "held-out total")
    edge = run.rows[(HOLDOUT - 1) // WINDOW]  # the window that holds example 1 001: one learned example, 36 held out
    assert int(edge["first_number"]) == 1000 and int(edge["learned"]["n"]) == 1 and int(edge["held_out"]["n"]) == 36
    assert edge["learned"]["sum_loss"] > 0 and edge["held_out"]["sum_loss"] > 0
    # what the trainer hands out for the held-out examples is what it scored
    assert np.array_equal(run.preds, s.pred[HOLDOUT - 1:])
    held = slice(HOLDOUT - 1, N)
    mr.check_total(run.held_out, (mr.sums(run.preds, s.label[held], s.imp[held]), mr.hist(run.preds, s.label[held])), "held-out total from trainer_predictions")
    assert int(run.learned["sums"]["n"]) == 998 and int(run.learned["sums"]["n_unlabelled"]) == 2 and int(run.held_out["sums"]["n_unlabelled"]) == 1
    assert run.learned["sums"]["sum_importance"] == 998 - 4 + 0.25 + 8 + 2 + 0.5
    # scoring changed nothing: the trainer's tables are the twin's, byte for byte
    assert run.sums == s.twin_sums
    assert 0.0 <= fw.binned_auc(run.held_out["hist"]) <= 1.0


@pytest.mark.parametrize("mb", [64, 100])
@pytest.mark.parametrize("call", [1, 7, 1500])
def test_same_stream_cut_differently(stream, call, mb):
    run = TrainerRun(stream.mi, stream.recs, stream.off, mb=mb, call=call)
    assert len(run.rows) == len(stream.host.rows)
    for got, ref in zip(run.rows, stream.host.rows):
        assert int(got["first_number"]) == int(ref["first_number"])
        mr.check_sums(got["learned"], ref["learned"], "learned", sides=2)
        mr.check_sums(got["held_out"], ref["held_out"], "held out", sides=2)
    for got, ref in ((run.learned, stream.host.learned), (run.held_out, stream.host.held_out)):
        mr.check_sums(got["sums"], ref["sums"], "total", sides=2)
        assert np.array_equal(got["hist"], ref["hist"])
    assert run.sums == stream.host.sums


def test_device_text_route(stream, monkeypatch):
    monkeypatch.setenv("FWGPU_TRAINER_TEXT_PIECE", "4096")  # many pieces, several launch windows in each
    dev = DeviceVowpalParser(stream.vw)
    try:
        run = TrainerRun(stream.mi, text=stream.text, dparser=dev)
        took, by_host = dev.last_lines()
    finally:
        dev.close()
    assert run.n == N and by_host >= 1
    assert len(run.rows) == len(stream.host.rows)
    for got, ref in zip(run.rows, stream.host.rows):
        assert int(got["first_number"]) == int(ref["first_number"])
        mr.check_sums(got["learned"], ref["learned"], "learned", sides=2)
        mr.check_sums(got["held_out"], ref["held_out"], "held out", sides=2)
    for got, ref in ((run.learned, stream.host.learned), (run.held_out, stream.host.held_out)):
        mr.check_sums(got["sums"], ref["sums"], "total", sides=2)
        assert np.array_equal(got["hist"], ref["hist"])
    # ... and against the yardstick itself
    mr.check_rows(run.rows, stream.want_rows)
    assert run.sums == stream.host.sums and np.array_equal(run.preds, stream.host.preds)


def test_oversize_record_is_counted_once(stream):
    lines = list(stream.lines[:100])
    lines.insert(50, "-1 |C " + " ".join("f%d" % i for i in range(4100)))  # more features than the example kernel stages: that micro-batch is walked
    host = VowpalParser(stream.vw)
    recs, off, used, rc = host.parse_buffer(_text(lines))
    host.close()
    assert rc == capi.OK and len(off) == 102
    first_word = off[:-1].astype(np.int64)
    label, imp = recs[first_word + 1].astype(np.float32), recs[first_word + 2].copy().view(np.float32)
    pred, learned, sums, routes = _twin(stream.mi, recs, off, _cuts(101, MB, 0))
    assert routes == [capi.ROUTE_HOST_WALK, capi.ROUTE_FUSED]
    run = TrainerRun(stream.mi, recs, off, holdout_after=0)
    mr.check_rows(run.rows, mr.windows(pred, label, imp, learned, 1, WINDOW))
    assert sum(int(r["learned"]["n"]) + int(r["learned"]["n_unlabelled"]) for r in run.rows) == 101
    row = run.rows[50 // WINDOW]  # the oversize example is number 51
    assert int(row["learned"]["n"]) + int(row["learned"]["n_unlabelled"]) == WINDOW and int(row["held_out"]["n"]) == 0
    assert int(run.learned["sums"]["n"]) + int(run.learned["sums"]["n_unlabelled"]) == 101 and run.sums == sums


def test_default_concurrency_counts_are_exact(stream):
    run = TrainerRun(stream.mi, stream.recs, stream.off, in_flight=0)
    assert len(run.rows) == (N + WINDOW - 1) // WINDOW
    for j, r in enumerate(run.rows):
        size = min(WINDOW, N - j * WINDOW)
        assert sum(int(r[side][f]) for side in ("learned", "held_out") for f in mr.COUNTS) == size
        assert int(r["learned"]["n_bad"]) == 0 and int(r["held_out"]["n_bad"]) == 0
    for t, n in ((run.learned, HOLDOUT - 1), (run.held_out, N - HOLDOUT + 1)):
        assert int(t["hist"].sum()) == int(t["sums"]["n"]) and int(t["sums"]["n_bad"]) == 0
        assert int(t["sums"]["n"]) + int(t["sums"]["n_unlabelled"]) == n


def test_metrics_off_and_the_order_of_the_calls(stream):
    off_run = TrainerRun(stream.mi, stream.recs, stream.off, window=None)
    assert len(off_run.rows) == 0 and int(off_run.learned["sums"]["n"]) == 0 and int(off_run.held_out["hist"].sum()) == 0
    assert off_run.sums == stream.host.sums and np.array_equal(off_run.preds, stream.host.preds)
    re = fw.Regressor(stream.mi)
    tr = fw.Trainer(re, stream.mi, micro_batch=MB)
    tr.set_metrics(0)
    tr.set_metrics(2)
    tr.digest_records(stream.recs, stream.off[:5])
    with pytest.raises(capi.FwgpuError) as ei:
        tr.set_metrics(WINDOW)  # refused once examples have been digested
    assert ei.value.code == capi.ERR_INVALID
    tr.block_until_workers_finished()
    n = C.c_uint64(7)
    capi.check(capi.lib().fwgpu_trainer_metrics(tr.h, None, 0, C.byref(n), None, None))  # the count alone
    assert n.value == 2
    one = np.zeros(1, dtype=capi.METRIC_WINDOW)
    assert capi.lib().fwgpu_trainer_metrics(tr.h, capi.ptr(one), 1, C.byref(n), None, None) == capi.ERR_RANGE and n.value == 2
    rows, lt, ht = tr.metrics()
    assert [int(r["learned"]["n"]) for r in rows] == [2, 2] and int(lt["sums"]["n"]) == 4 and int(ht["sums"]["n"]) == 0
    tr.close()
    re.close()


def test_window_of_one_grows_the_table(stream):
    """1 500 windows: the table starts at 64 rows and is regrown on the trainer's stream while launches are in flight"""
    run = TrainerRun(stream.mi, stream.recs, stream.off, window=1)
    assert len(run.rows) == N
    per = np.array([[int(r[side][f]) for f in mr.COUNTS] for r in run.rows for side in ("learned", "held_out")]).reshape(N, 2, 3)
    assert np.all(per.sum(axis=(1, 2)) == 1) and np.all(per[:HOLDOUT - 1, 1] == 0) and np.all(per[HOLDOUT - 1:, 0] == 0)
    mr.check_rows(run.rows, mr.windows(stream.pred, stream.label, stream.imp, stream.learned, 1, 1))
    for got, ref in ((run.learned, stream.host.learned), (run.held_out, stream.host.held_out)):
        mr.check_sums(got["sums"], ref["sums"], "total", sides=2)
        assert np.array_equal(got["hist"], ref["hist"])
