"""Many requests' candidates from their TEXT in one device launch (fwgpu_predictor_predict_requests_text, csrc/requests_text.hip): bit for bit what
fwgpu_predictor_predict_requests returns for the same lines, on the four kernel families of the requests route, through that family's kernel; every
family also against the float64 forward pass over the whole request, at the bars of tests/test_gpu_requests.py (ffm_ref.judge_prediction) and
tests/test_gpu_head_requests.py (head_ref, PRED_TOL); the whole-call fallbacks; the refusals.  Field 1 holds two namespaces (1 and the last one), so that a candidate can repeat a cached feature from a namespace its context leaves out."""
from types import SimpleNamespace

import numpy as np
import pytest

import cache_cases as cc
import ffm_ref
import head_ref as hr
import test_gpu_head_cache as hc
import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import _capi as capi
from fwumious_wabbit_amd import persistence as P
from fwumious_wabbit_amd import serving
from fwumious_wabbit_amd.feed import VowpalParser, VwNamespaceMap

pytestmark = pytest.mark.gpu

SHAPES = [(6, 4), (30, 8)]  # the two smallest of requests_cases.SHAPES
# family -> (deep head, the predictor's tokens, the requests kernel its launch must be)
FAMILIES = {"f32": (False, "", capi.KERNEL_REQUESTS), "packed": (False, "--packed_weights --packed_context_cache", capi.KERNEL_PACKED_REQUESTS),
            "head": (True, "--head_requests", capi.KERNEL_HEAD_REQUESTS),
            "packed_head": (True, "--packed_weights --packed_head_requests", capi.KERNEL_PACKED_HEAD_REQUESTS)}
LAYERS = [(10, "relu")]
TABLES = (capi.TABLE_FFM_W, capi.TABLE_FFM_ACC, capi.TABLE_LR)
SCAN_BLOCK = 1024  # requests_text.h kRtScanThreads
CONTEXTS = ["|N0 ca |N1 cb1 cb2:0.5 ", "|N0 cx cy:2 |N1 cz |N3 cw ", "|N0 cq |N1 cr:0.5 cs ct "]
_BUILT = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _candidate(j, F):
    """line j: several features and a value; the f32-format namespace 5; namespace 2 of the LR combo (0, 2), whose namespace 0 is the context's; no
    feature at all (no FFM entry of its own); namespace F, the second of field 1, whose first namespace the context fills"""
    return [f"|N2 x{j} y{j}:0.5 z{j} |N4 q{j}\n", f"|N5 ab{j}.5 ab2 |N2:2 p{j}\n", f"|N4 s{j}:1.25 |N{F} w{j % 7} ww:2\n", "|N2\n",
            f"|N2 t{j}  |N4 u{j} v{j}:3\n"][j % 5]


@pytest.fixture
def model(tmp_path_factory):
    def build(F, k, family):
        if (F, k, family) in _BUILT:
            return _BUILT[(F, k, family)]
        head, flags, kernel = FAMILIES[family]
        nd = fw.NamespaceDescriptor
        m = SimpleNamespace(F=F, k=k, flags=flags, kernel=kernel)
        m.mi = fw.ModelInstance(learning_rate=0.1, ffm_learning_rate=0.1, bit_precision=12, power_t=0.5, ffm_power_t=0.5, add_constant_feature=True,
                                feature_combo_descs=[fw.FeatureComboDesc([nd(i)]) for i in range(F + 1)] + [fw.FeatureComboDesc([nd(0), nd(2)])],
                                ffm_fields=[[nd(f)] + ([nd(F)] if f == 1 else []) for f in range(F)], ffm_k=k, ffm_bit_precision=12,
                                init_acc_gradient=1.0, ffm_init_acc_gradient=1.0, optimizer=fw.Optimizer.AdagradLUT)
        if head:
            m.mi.nn_layers = [dict(width=w, activation=a, init="hu") for w, a in LAYERS]
            m.mi.nn_topology = "one"
        m.vw = VwNamespaceMap("".join(f"N{i},n{i}{',f32' if i == 5 else ''}\n" for i in range(F + 1)) + "_namespace_skip_prefix,2\n")
        re = fw.Regressor(m.mi)
        for t, v in zip(TABLES, cc.warm_tables(F, k, 12, 12, seed=9)):
            assert re.table_len(t) == len(v)
            re.table_write(t, v)
        d = tmp_path_factory.mktemp(f"rt{F}x{k}{family}")
        m.path = str(d / "model.fw")
        P.save_regressor_to_filename(m.path, m.mi, m.vw, re)
        re.close()
        if "--packed_weights" in flags:
            whole, m.path = m.path, str(d / "quantised.fw")
            P.convert_inference_regressor(whole, m.path, quantize_weights=True)
        return _BUILT.setdefault((F, k, family), m)

    return build


def _predictors(m, contexts):
    prs = [serving.Predictor(f"fw -i {m.path} -t --foreground {m.flags}")]
    prs += [prs[0].clone_lite() for _ in contexts[1:]]
    for pr, ctx in zip(prs, contexts):
        assert pr.setup_cache(ctx + "\n") == 0.0
    return prs


def _both(m, prs, requests, last_newline=True):
    """(the text call's outputs, predict_requests' on the same lines); the text call must not have fallen back, and its launch is the family's kernel"""
    texts = ["".join(r).encode() for r in requests]
    if not last_newline:
        texts = [t[:-1] if t else t for t in texts]
    got = serving.predict_requests_text(prs, texts)
    lines, host_lines, fell_back = prs[0].last_text_route()
    assert (lines, host_lines, fell_back) == (sum(len(r) for r in requests), 0, False)
    route, launch = prs[0].last_launch()
    assert (route, launch["family"]) == (capi.ROUTE_REQUESTS, m.kernel), (route, launch)
    return got, serving.predict_requests(prs, requests)


# name -> (lines per request, the predictor of each request).  "three requests": different contexts, a workgroup of four lines that holds lines of
# two requests (7 | 65), the same predictor twice, a request without lines
REQUEST_SETS = {"one line": ([1], [0]), "three requests": ([7, 65, 0], [1, 0, 1]), "scan block + 1": ([SCAN_BLOCK - 2, 3], [0, 2]),
                "no last newline": ([3, 0, 2], [0, 1, 2])}


@pytest.mark.parametrize("F,k", SHAPES, ids=[f"{F}x{k}" for F, k in SHAPES])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_text_call_equals_predict_requests_bit_for_bit(model, family, F, k):
    m = model(F, k, family)
    prs = _predictors(m, CONTEXTS)
    try:
        for name, (counts, who) in REQUEST_SETS.items():
            requests = [[_candidate(j + 2 * r, F) for j in range(n)] for r, n in enumerate(counts)]  # (no candidate names namespace 3, which context 1 fills)
            got, want = _both(m, [prs[i] for i in who], requests, last_newline=name != "no last newline")
            for r, (g, w) in enumerate(zip(got, want)):
                assert len(g) == counts[r] and np.all(g > 0.0), (name, r)  # (-1.0: a line that gave no prediction)
                assert np.array_equal(_bits(g), _bits(w)), f"{family} {F}x{k}, {name}: request {r} differs from predict_requests"
    finally:
        for pr in prs:
            pr.close()


@pytest.mark.parametrize("family", list(FAMILIES))
def test_text_call_against_float64(model, family):
    """every prediction against the float64 forward pass over context + candidate on the predictor's own tables (the quantised file's dequantised
    weights for the packed families): the bar of tests/test_gpu_requests.py (ffm_ref.judge_prediction) without a head, that of
    tests/test_gpu_head_requests.py (head_ref, PRED_TOL) with one"""
    F, k = SHAPES[0]
    m = model(F, k, family)
    prs = _predictors(m, CONTEXTS)
    _, _, twin = P.new_regressor_from_filename(m.path, immutable=True)
    host, fbt = VowpalParser(m.vw), fw.FeatureBufferTranslator(m.mi)
    try:
        w, lr = twin.table_read(capi.TABLE_FFM_W), twin.table_read(capi.TABLE_LR)
        requests = [[_candidate(j + r, F) for j in range(20)] for r in range(3)]
        got, _ = _both(m, prs, requests)
        for r, ctx in enumerate(CONTEXTS):
            fbs = [fbt.translate(host.next_vowpal((ctx + line).encode())) for line in requests[r]]
            if FAMILIES[family][0]:
                en = hr.Entries([np.asarray(fb.lr_buffer, dtype=hr.fwo.LR_ENTRY) for fb in fbs], [np.asarray(fb.ffm_buffer, dtype=hr.fwo.FFM_ENTRY) for fb in fbs])
                x64, _, _ = hr.head_inputs64(lr, w, m.mi.num_combos, F, k, en)
                p64, _ = hr.head_forward64(x64, twin.table_read(capi.TABLE_NN_W), LAYERS, "one")
                hc._close(got[r], p64, hr.PRED_TOL, f"REQUESTS TEXT {family} request {r} against the float64 head")
                continue
            for j, fb in enumerate(fbs):
                ref = ffm_ref.predict(SimpleNamespace(F=F, k=k), w, lr, fb.lr_buffer, fb.ffm_buffer)
                err, bound, _ = ffm_ref.judge_prediction(got[r][j], *ref)
                print(f"REQUESTS TEXT {family} request {r} line {j}: p = {got[r][j]!r}, float64 {ref[0]!r}, |d| = {err:.3e}, bound {bound:.3e}")
                assert err <= bound, (family, r, j, got[r][j], ref[0], err, bound)
    finally:
        for x in prs + [host, twin]:
            x.close()


def _cached_repeat(m, parser):
    """a feature of namespace F (field 1, which context 0 leaves out) whose masked hash is that of the context's `cb1` in namespace 1 (field 1 too)"""
    mask = capi.lib().fwgpu_ffm_hash_mask(12, m.k)
    want = int(parser.next_vowpal(b"|N1 cb1\n")[3 + 1]) & mask
    for i in range(200000):
        if int(parser.next_vowpal(f"|N{m.F} r{i}\n".encode())[3 + m.F]) & mask == want:
            return f"|N{m.F} r{i}\n"
    raise AssertionError("no collision found")


@pytest.mark.parametrize("what", ["covered namespace again", "cached feature repeated", "label", "NONE value"])
def test_one_line_sends_the_whole_call_to_the_host_route(model, what):
    m = model(*SHAPES[0], "f32")
    prs = _predictors(m, CONTEXTS[:2])
    parser = VowpalParser(m.vw)
    try:
        line = {"covered namespace again": "|N0 other\n", "label": "1 |N2 x\n", "NONE value": "|N2 a:NONE b\n"}.get(what) or _cached_repeat(m, parser)
        requests = [[_candidate(0, m.F), line, _candidate(2, m.F), _candidate(3, m.F), _candidate(4, m.F)], [_candidate(j, m.F) for j in range(3)]]  # (context 0's request)
        got = serving.predict_requests_text(prs, ["".join(r).encode() for r in requests])
        assert prs[0].last_text_route() == (8, 8, True), what
        for g, w in zip(got, serving.predict_requests(prs, requests)):
            assert np.array_equal(_bits(g), _bits(w)), what
    finally:
        for x in prs + [parser]:
            x.close()


def test_refusals_are_those_of_predict_requests(model):
    m = model(*SHAPES[0], "f32")
    prs = _predictors(m, CONTEXTS[:1])
    try:
        text = b"|N2 a\n|N2 b\n"
        with pytest.raises(capi.FwgpuError) as e:
            serving.predict_requests_text(prs, [text], caps=[1])
        assert e.value.code == capi.ERR_RANGE
        fresh = prs[0].clone_lite()
        prs.append(fresh)
        other = serving.Predictor(f"fw -i {m.path} -t --foreground")
        prs.append(other)
        assert other.setup_cache(CONTEXTS[0] + "\n") == 0.0
        for group, words in (([fresh], "fw_setup_cache"), ([prs[0], other], "ONE model")):
            with pytest.raises(capi.FwgpuError) as e:
                serving.predict_requests_text(group, [text] * len(group))
            assert e.value.code == capi.ERR_INVALID and words in e.value.message and "fwgpu_predictor_predict_batch" in e.value.message
        plain = serving.Predictor(f"fw -i {model(*SHAPES[0], 'packed').path} -t --foreground --packed_weights")
        prs.append(plain)
        assert plain.setup_cache(CONTEXTS[0] + "\n") == 0.0
        nohead = serving.Predictor(f"fw -i {model(*SHAPES[0], 'head').path} -t --foreground")
        prs.append(nohead)
        assert nohead.setup_cache(CONTEXTS[0] + "\n") == 0.0
        for pr, words in ((plain, "keeps no device cache"), (nohead, "deep head")):
            with pytest.raises(capi.FwgpuError) as e:
                serving.predict_requests_text([pr], [text])
            assert e.value.code == capi.ERR_INVALID and words in e.value.message
    finally:
        for pr in prs:
            pr.close()
