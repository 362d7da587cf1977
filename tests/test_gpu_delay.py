"""`--prediction_model_delay N` in the trainer (HogwildTrainer.set_delay / delay_state; include/fwgpu.h "predicting with a model delayed by N
examples"; csrc/trainer.cpp: the ring of record batches between a window's predict launch and its learn launch) against tests/delay_ref.py on the
CPU oracle: the reference's loop where micro_batch == 1, the header's window rule everywhere else.

Bounds.  In order (one example in flight) a hogwild launch is the reference's single-thread walk, so the project's in-order bound holds: per
example |d logloss| < 1e-4 and tables within 2e-5 + 1e-5 |ref| (tests/test_gpu_parity.py).  The concurrent case runs on examples that share no
table entry inside a window, so it is deterministic too and its predictions are held to 1e-4."""
import random

import numpy as np
import pytest

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import capi
from fwumious_wabbit_amd.feed import DeviceVowpalParser, RecordCache, VowpalParser, VwNamespaceMap
from oracle import fwo

import delay_ref
import metrics_ref as mr
from helpers import LOGLOSS_TOL, check_disjoint, disjoint_models, disjoint_stream, logloss, make_pair, record_labels

pytestmark = pytest.mark.gpu

TABLES = (capi.TABLE_LR, capi.TABLE_FFM_W, capi.TABLE_FFM_ACC)
CSV5 = "A,fa\nB,fb\nC,fc\nD,fd\nE,fe\n"
N_TEXT = 400


def _close(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref).reshape(-1)
    bad = np.abs(got - ref) > 2e-5 + 1e-5 * np.abs(ref)
    worst = int(np.abs(got - ref).argmax())
    assert not bad.any(), (what, int(bad.sum()), float(np.abs(got - ref).max()), worst, float(got[worst]), float(ref[worst]))


def _check_preds(got, ref, y, what=""):
    assert len(got) == len(ref) == len(y), (what, len(got), len(ref), len(y))
    d = np.abs(logloss(got, y) - logloss(ref, y))
    print(f"{what}: max per-example |d logloss| = {d.max():.3e}, max |dp| = {np.abs(got - ref).max():.3e}")
    assert d.max() < LOGLOSS_TOL, (what, float(d.max()), int(d.argmax()))


def _oracle_tables(om, head_layers=0):
    out = {capi.TABLE_LR: om.lr_table, capi.TABLE_FFM_W: om.ffm_weights, capi.TABLE_FFM_ACC: om.ffm_acc}
    if head_layers:
        out[capi.TABLE_NN_W] = np.concatenate([om.nn_weights(l) for l in range(head_layers + 1)])
    return {t: np.array(a, dtype=np.float32).reshape(-1) for t, a in out.items()}


class Run:
    """one regressor + trainer in the delayed protocol"""

    def __init__(self, mi, mb, delay, pa=0, in_flight=1, nn_w=None, metrics=None):
        self.re = fw.Regressor(mi)
        if in_flight:
            self.re.set_max_in_flight(in_flight)
        if nn_w is not None:
            self.re.table_write(capi.TABLE_NN_W, nn_w)
        self.tr = fw.Trainer(self.re, mi, micro_batch=mb)
        if metrics:
            self.tr.set_metrics(metrics)
        self.tr.set_delay(delay, pa)

    def digest(self, recs, off, a=0, e=None):
        e = len(off) - 1 if e is None else e
        self.tr.digest_records(recs[int(off[a]):int(off[e])], off[a:e + 1] - off[a])

    def finish(self, tables=TABLES):
        self.tr.block_until_workers_finished()
        self.preds = self.tr.predictions()
        self.state = self.tr.delay_state()
        self.tables = {t: self.re.table_read(t) for t in tables}
        self.sums = [self.re.table_checksum(t) for t in tables]
        return self

    def check_tables(self, want):
        for t, ref in want.items():
            _close(self.tables[t], ref, f"table {t}")

    def close(self):
        self.tr.close()
        self.re.close()


def _final_state(windows, delay):
    through, pend_ex, pend_w = delay_ref.plan(windows, delay)[-1]
    return dict(learned_through=through, pending_examples=pend_ex, pending_windows=pend_w)


def _state_matches(state, want):
    assert {k: state[k] for k in want} == want, (state, want)


# ---------------------------------------------------------------- 1. micro_batch == 1: the reference's loop
HEAD = [(8, "relu", "hu"), (8, "relu", "hu")]
LOOP_CASES = [(fw.Optimizer.AdagradLUT, d, pa, False) for d in (1, 5, 64) for pa in (0, 7)] + [
    (fw.Optimizer.AdagradFlex, 5, 0, False), (fw.Optimizer.SGD, 5, 7, False), (fw.Optimizer.AdagradLUT, 5, 0, True)]


@pytest.mark.parametrize("opt,delay,pa,head", LOOP_CASES, ids=lambda v: str(v))
def test_micro_batch_of_one_is_the_reference_loop(opt, delay, pa, head):
    """The head case's stream is one on which PLAIN in-order learning (one sequential launch, no trainer) meets the in-order bound, asserted below:
    a ReLU whose input the two implementations round to different sides of zero is a step, not a rounding error, and it shows in about 90 LR
    accumulators of such a stream with or without a delay (synth seed 22: 2.5e-3 on accumulators of 45, the trainer bit-equal to the loop
    driven by hand through record batches).  The bound is about the protocol, so the stream must not have one."""
    n = 300
    kw = dict(lr=0.05, ffm_lr=0.05) if opt == fw.Optimizer.SGD else {}
    mi, ocfg, ots = make_pair(5, 4, 14, 14, opt, **kw)
    nn, nn_w = None, None
    if head:
        mi.nn_layers = [dict(width=w, activation=a, init=i) for w, a, i in HEAD]
        mi.nn_topology = "one"
        mi.nn_learning_rate, mi.nn_power_t, mi.nn_init_acc_gradient = 0.02, 0.45, 0.0
        nn = fwo.make_nn_config(HEAD, "one", 0.02, 0.45, 0.0)
    recs, off = fw.synth_records(5, 1.0, 1.1, 40, 0.2, 23 if head else 17 + delay, 0, n)
    y = record_labels(recs, off)
    om = fwo.Model(ocfg, nn=nn)
    if head:
        nn_w = np.concatenate([om.nn_weights(l).copy() for l in range(len(HEAD) + 1)])
        plain = fwo.Model(ocfg, nn=nn)
        _, p_plain = plain.run_stream(ots, recs, off, holdout_after=0, nthreads=1)
        re = fw.Regressor(mi)
        re.table_write(capi.TABLE_NN_W, nn_w)
        b = re.record_batch(fw.FeatureBufferTranslator(mi), recs, off)
        re.learn_batch(b, capi.MODE_SEQUENTIAL, True)
        _check_preds(b.predictions(), p_plain, y, "the stream without a delay, in order")
        _close(re.table_read(capi.TABLE_LR), plain.lr_table, "the stream without a delay, in order: LR table")
        b.close()
        re.close()
        plain.close()
    want = delay_ref.reference_loop(om, ots, recs, off, delay, pa)
    tables = TABLES + ((capi.TABLE_NN_W,) if head else ())
    run = Run(mi, 1, delay, pa, nn_w=nn_w)
    run.digest(recs, off, 0, 120)
    mid = run.tr.delay_state()
    run.digest(recs, off, 120, n)
    run.finish(tables)
    run.close()
    assert len(run.preds) == n - pa
    _check_preds(run.preds, want, y[pa:], f"delay {delay}, predictions_after {pa}")
    run.check_tables(_oracle_tables(om, len(HEAD) if head else 0))
    _state_matches(mid, dict(learned_through=max(0, 120 - delay), pending_examples=min(120, delay), pending_windows=min(120, delay)))
    _state_matches(run.state, dict(learned_through=n - delay, pending_examples=min(n, delay), pending_windows=min(n, delay)))
    assert run.state["ring_bytes"] > 0


# ---------------------------------------------------------------- the text stream of tests 2, 4, 5, 6
def _lines(n, seed=3):
    rng = random.Random(seed)
    lines = []
    for _ in range(n):
        toks = []
        for ns in "ABCDE":
            if rng.random() < 0.85:
                feats = []
                for _ in range(rng.choice([1, 1, 2])):
                    f = "%s%d" % (ns.lower(), rng.randrange(25))
                    if rng.random() < 0.2:
                        f += ":" + rng.choice(["0.5", "2", "1.25"])
                    feats.append(f)
                toks.append("|" + ns + " " + " ".join(feats))
        lines.append(rng.choice(["1", "-1"]) + " " + " ".join(toks or ["|A a0"]))
    return lines


def _text(lines):
    return ("\n".join(lines) + "\n").encode()


class Stream:
    def __init__(self, lines):
        self.vw = VwNamespaceMap(CSV5)
        self.lines, self.text = lines, _text(lines)
        host = VowpalParser(self.vw)
        self.recs, self.off, used, rc = host.parse_buffer(self.text)
        host.close()
        assert rc == capi.OK and used == len(self.text) and len(self.off) == len(lines) + 1
        self.n = len(lines)
        first = self.off[:-1].astype(np.int64)
        self.y = self.recs[first + 1].astype(np.float32)
        self.imp = self.recs[first + 2].copy().view(np.float32)
        self.mi, self.ocfg, self.ots = make_pair(5, 4, 14, 14, fw.Optimizer.AdagradLUT)
        self._rule = {}

    def rule(self, windows, delay, pa=0):
        """(predictions, tables) of the window rule on the oracle, computed once per case and left unchanged"""
        key = (tuple(windows), delay, pa)
        if key not in self._rule:
            om = fwo.Model(self.ocfg)
            p = delay_ref.window_rule(om, self.ots, self.recs, self.off, list(windows), delay, pa)
            self._rule[key] = (p, _oracle_tables(om))
            om.close()
        return self._rule[key]


@pytest.fixture(scope="module")
def stream():
    return Stream(_lines(N_TEXT))


# ---------------------------------------------------------------- 2. the window rule, in order
@pytest.mark.parametrize("mb,delay,pa", [(mb, d, 0) for mb in (16, 24) for d in (1, 16, 40, 100)] + [(16, 40, 7)])
def test_window_rule_in_order(stream, mb, delay, pa):
    s = stream
    windows = delay_ref.cut(s.n, mb, pa)
    want, tables = s.rule(windows, delay, pa)
    run = Run(s.mi, mb, delay, pa)
    run.digest(s.recs, s.off)
    run.finish()
    run.close()
    assert len(run.preds) == s.n - pa
    _check_preds(run.preds, want, s.y[pa:], f"micro_batch {mb}, delay {delay}")
    run.check_tables(tables)
    _state_matches(run.state, _final_state(windows, delay))
    assert run.state["pending_examples"] >= delay


# ---------------------------------------------------------------- 3. the window rule with the default examples in flight
@pytest.mark.parametrize("delay", [32, 50])
@pytest.mark.parametrize("P,reps", [(64, 6), (32, 12)])
def test_window_rule_concurrent_on_disjoint_windows(P, reps, delay):
    """A stream of period P: P mutually disjoint examples, repeated.  A window of 32 holds examples of one period only, so the default examples
    in flight change nothing, and every prediction shows how often its example has been learned.

    Teeth (a condition on the inputs, asserted on the oracle alone): the rule moved by one window must move a prediction by more than 1e-3.
    With P = 64 a window is HALF a period, so learning it matters only to the windows two, four, ... steps on, and a rule moved by one window shows
    in one direction per delay: later at delay 32 (the window is learned one step after it is taken; a step more and the window two on misses it),
    earlier at delay 50 (learned two steps after; a step less and the window two on sees it).  The other direction moves nothing there, whatever
    the seed; the two delays together have both.  With P = 32 every window is the whole period and both directions show at both delays."""
    mb = 32
    st = disjoint_stream(4, 4, P, per_field=(1, 2), p_weighted=0.3, seed=5)
    mi, ocfg, ots = disjoint_models(st, fw.Optimizer.AdagradLUT)
    check_disjoint(st, mi)  # any window holds examples of ONE period only (mb divides P): no two of them share a table entry
    assert P % mb == 0 and 14 <= st.ffm_bits <= 16
    recs = np.tile(st.recs, reps)
    off = np.concatenate([[0], (np.arange(reps)[:, None] * int(st.off[-1]) + st.off[1:].astype(np.int64)[None, :]).reshape(-1)]).astype(np.uint64)
    n = P * reps
    windows = delay_ref.cut(n, mb)
    got = {}
    for shift in (0, 1, -1):
        om = fwo.Model(ocfg)
        got[shift] = delay_ref.window_rule(om, ots, recs, off, windows, delay, shift=shift)
        if shift == 0:
            tables = _oracle_tables(om)
        om.close()
    want = got[0]
    later, earlier = float(np.abs(got[1] - want).max()), float(np.abs(got[-1] - want).max())
    print(f"P {P}, delay {delay}: the rule one window later moves a prediction by {later:.3e}, one window earlier by {earlier:.3e}")
    if P == mb:
        assert later > 1e-3 and earlier > 1e-3
    else:
        assert (later if delay == 32 else earlier) > 1e-3
    run = Run(mi, mb, delay, in_flight=0)
    run.digest(recs, off)
    run.finish()
    run.close()
    assert len(run.preds) == n
    print(f"P {P}, delay {delay}: max |dp| = {np.abs(run.preds - want).max():.3e}")
    assert np.abs(run.preds - want).max() < 1e-4
    run.check_tables(tables)
    _state_matches(run.state, _final_state(windows, delay))


# ---------------------------------------------------------------- 4. every route into the ring
ROUTE_CASE = (16, 40, 7)  # micro_batch, delay, predictions_after: a case of test 2


def _pieces(text, piece):
    """lines per piece of fwgpu_trainer_digest_text_device: cut at the last line break inside `piece` bytes"""
    out, pos = [], 0
    while pos < len(text):
        cut = min(len(text) - pos, piece)
        if pos + cut < len(text):
            nl = text.rfind(b"\n", pos, pos + cut)
            if nl < 0:
                nl = text.find(b"\n", pos + cut)
            cut = nl - pos + 1 if nl >= 0 else len(text) - pos
        out.append(text[pos:pos + cut].count(b"\n"))
        pos += cut
    return out


def test_routes(stream, tmp_path, monkeypatch):
    s = stream
    mb, delay, pa = ROUTE_CASE
    windows = delay_ref.cut(s.n, mb, pa)
    want, tables = s.rule(windows, delay, pa)
    runs = {}
    # fwgpu_digest_records in ragged calls
    run = Run(s.mi, mb, delay, pa)
    a, k = 0, 0
    while a < s.n:
        e = min(s.n, a + (1, 7, 30, 3, 50, 16)[k % 6])
        run.digest(s.recs, s.off, a, e)
        a, k = e, k + 1
    runs["records"] = run.finish()
    # fwgpu_trainer_digest_text with the host parser, writing a cache ...
    inp = str(tmp_path / "train.vw")
    open(inp, "wb").write(s.text)
    host = VowpalParser(s.vw)
    cache = RecordCache(inp, True, s.vw)
    assert cache.writing
    run = Run(s.mi, mb, delay, pa)
    assert run.tr.digest_text(host, s.text, cache=cache, threads=3) == (s.n, len(s.text), capi.OK)
    runs["text"] = run.finish()
    cache.write_finish()
    cache.close()
    host.close()
    # ... and the cache read back
    cache = RecordCache(inp, True, s.vw)
    assert cache.reading
    run = Run(s.mi, mb, delay, pa)
    assert run.tr.digest_cache(cache) == s.n
    runs["cache"] = run.finish()
    cache.close()
    for name, run in runs.items():
        run.close()
        _check_preds(run.preds, want, s.y[pa:], name)
        run.check_tables(tables)
        _state_matches(run.state, _final_state(windows, delay))
        # the in-order host-fed routes agree bit for bit
        assert np.array_equal(run.preds.view(np.uint32), runs["records"].preds.view(np.uint32)) and run.sums == runs["records"].sums, name
    # the device text route: one piece (the windows of the host-fed routes), then many pieces (every piece closes its last window)
    for piece in (None, 1024):
        if piece:
            monkeypatch.setenv("FWGPU_TRAINER_TEXT_PIECE", str(piece))
            per_piece = _pieces(s.text, piece)
            assert len(per_piece) > 8 and sum(per_piece) == s.n
            w, seen = [], 0
            for m in per_piece:
                w += delay_ref.cut(m, mb, max(0, pa - seen))
                seen += m
            want_p, tables_p = s.rule(w, delay, pa)
        else:
            monkeypatch.delenv("FWGPU_TRAINER_TEXT_PIECE", raising=False)
            w, want_p, tables_p = windows, want, tables
        dev = DeviceVowpalParser(s.vw)
        run = Run(s.mi, mb, delay, pa)
        try:
            assert run.tr.digest_text_device(dev, s.text) == (s.n, len(s.text), capi.OK)
            run.finish()
            took, by_host = dev.last_lines()
        finally:
            run.close()
            dev.close()
        assert by_host == 0  # no line of this stream goes through the host
        _check_preds(run.preds, want_p, s.y[pa:], f"device text route, piece {piece}")
        run.check_tables(tables_p)
        _state_matches(run.state, _final_state(w, delay))
        if not piece:
            assert np.array_equal(run.preds.view(np.uint32), runs["records"].preds.view(np.uint32)) and run.sums == runs["records"].sums


# ---------------------------------------------------------------- 5. fwgpu_finish in mid-stream, an oversize example
def test_finish_in_mid_stream_and_an_oversize_example():
    mb, delay = 16, 40
    lines = _lines(150, seed=9)
    # 4100 features, more than the example kernel stages: its window is walked example by example (two namespaces: the oracle's translator takes 4096 each)
    lines.insert(70, "-1 |C " + " ".join("f%d:0.01" % i for i in range(2050)) + " |D " + " ".join("g%d:0.01" % i for i in range(2050)))
    s = Stream(lines)
    run = Run(s.mi, mb, delay)
    windows, a = [], 0
    steps = [50, 30, 71]
    assert sum(steps) == s.n == 151
    for take in steps:
        before = run.tr.delay_state()
        _state_matches(before, _final_state(windows, delay) if windows else dict(learned_through=0, pending_examples=0, pending_windows=0))
        run.digest(s.recs, s.off, a, a + take)
        a += take
        full = [mb] * (take // mb)
        _state_matches(run.tr.delay_state(), _final_state(windows + full, delay))  # the open micro-batch is not in the ring yet
        run.tr.block_until_workers_finished()
        windows += full + ([take % mb] if take % mb else [])
        _state_matches(run.tr.delay_state(), _final_state(windows, delay))
        assert len(run.tr.predictions()) == a
    assert windows == [16, 16, 16, 2, 16, 14, 16, 16, 16, 16, 7]
    run.finish()
    run.close()
    want, tables = s.rule(windows, delay)
    _check_preds(run.preds, want, s.y, "variable windows")
    run.check_tables(tables)
    assert run.state["learned_through"] == 96 and run.state["pending_examples"] == 55  # the oversize example (number 71) has been learned
    # ... by the example-by-example walk: its window (examples 67 .. 80) is one the fused kernel does not take
    re = fw.Regressor(s.mi)
    b = re.record_batch(fw.FeatureBufferTranslator(s.mi), s.recs[int(s.off[66]):int(s.off[80])], s.off[66:81] - s.off[66])
    re.learn_batch(b, capi.MODE_HOGWILD, False)
    assert re.last_route() == capi.ROUTE_HOST_WALK
    b.close()
    re.close()


# ---------------------------------------------------------------- 6. metrics: an example counts once, on the learned side
def test_metrics_count_every_predicted_example_once(stream):
    s = stream
    mb, delay, pa, window = 16, 40, 7, 37
    run = Run(s.mi, mb, delay, pa, metrics=window)
    run.digest(s.recs, s.off)
    run.finish()
    rows, learned, held_out = run.tr.metrics()
    run.close()
    assert len(run.preds) == s.n - pa
    assert int(learned["sums"]["n"]) == s.n - pa and int(learned["sums"]["n_unlabelled"]) == 0
    assert int(held_out["sums"]["n"]) == 0 and int(held_out["sums"]["n_unlabelled"]) == 0 and int(held_out["hist"].sum()) == 0
    y, imp = s.y[pa:], s.imp[pa:]
    mr.check_total(learned, (mr.sums(run.preds, y, imp), mr.hist(run.preds, y)), "learned total")
    mr.check_rows(rows, mr.windows(run.preds, y, imp, True, pa + 1, window))
    # scoring changed nothing
    plain = Run(s.mi, mb, delay, pa)
    plain.digest(s.recs, s.off)
    plain.finish()
    plain.close()
    assert plain.sums == run.sums and np.array_equal(plain.preds, run.preds)


# ---------------------------------------------------------------- 7. refusals, and the off state
def _refused(call, *names):
    with pytest.raises(capi.FwgpuError) as ei:
        call()
    assert ei.value.code == capi.ERR_INVALID
    for name in names:
        assert name in ei.value.message, (name, ei.value.message)


def test_refusals_leave_the_trainer_usable(stream):
    s = stream
    re = fw.Regressor(s.mi)
    re.set_max_in_flight(1)

    def usable(tr, n_pred):
        tr.digest_records(s.recs[: int(s.off[40])], s.off[:41])
        tr.block_until_workers_finished()
        assert tr.examples_seen() == 40 and len(tr.predictions()) == n_pred
        tr.close()

    # a delay, then a hold-out or test-only
    tr = fw.Trainer(re, s.mi, micro_batch=16)
    tr.set_delay(5, 3)
    _refused(lambda: tr.set_holdout(10), "prediction_model_delay", "holdout_after")
    _refused(lambda: tr.set_holdout(0, True), "prediction_model_delay", "testonly")
    tr.set_holdout(0, False)  # (no hold-out: nothing to refuse)
    assert tr.delay_state()["pending_examples"] == 0
    tr.digest_records(s.recs[: int(s.off[20])], s.off[:21])
    _refused(lambda: tr.set_delay(6), "prediction_model_delay")  # once examples have been digested
    _refused(lambda: tr.set_delay(0), "prediction_model_delay")
    tr.digest_records(s.recs[int(s.off[20]): int(s.off[40])], s.off[20:41] - s.off[20])
    tr.block_until_workers_finished()
    assert len(tr.predictions()) == 37 and tr.delay_state()["learned_through"] == 35
    tr.close()
    # a hold-out or test-only, then a delay
    tr = fw.Trainer(re, s.mi, micro_batch=16)
    tr.set_holdout(30)
    _refused(lambda: tr.set_delay(5), "prediction_model_delay", "holdout_after")
    tr.set_delay(0, 0)  # the off state conflicts with nothing
    usable(tr, 11)
    tr = fw.Trainer(re, s.mi, micro_batch=16)
    tr.set_holdout(0, True)
    _refused(lambda: tr.set_delay(5, 2), "prediction_model_delay", "testonly")
    usable(tr, 40)
    re.close()


def test_delay_zero_is_the_trainer_as_it_was(stream):
    s = stream
    sums = []
    for call in (True, False):
        re = fw.Regressor(s.mi)
        re.set_max_in_flight(1)
        tr = fw.Trainer(re, s.mi, micro_batch=16)
        if call:
            tr.set_delay(0, 0)
        tr.digest_records(s.recs, s.off)
        tr.block_until_workers_finished()
        assert len(tr.predictions()) == 0 and tr.delay_state() == dict(learned_through=0, pending_examples=0, pending_windows=0, ring_bytes=0)
        sums.append([re.table_checksum(t) for t in TABLES])
        tr.close()
        re.close()
    assert sums[0] == sums[1]
    # ... and it is not the delayed trainer's result
    run = Run(s.mi, 16, 40)
    run.digest(s.recs, s.off)
    run.finish()
    run.close()
    assert run.sums != sums[0]
