"""A request's candidates scored from their text on the device: DeviceVowpalParser.parse_candidates (csrc/textparse.hip, candidate mode)
against the host's fwgpu_parser_parse_candidate line by line, its per-line entry counts and record rule against fwgpu_translate and
fwgpu_block_cache_record_ok on the merged record, and Predictor.predict_text against predict_batch and predict."""
import random

import numpy as np
import pytest

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import capi
from fwumious_wabbit_amd import persistence as P
from fwumious_wabbit_amd.feed import DeviceVowpalParser, VowpalParser, VwNamespaceMap
from fwumious_wabbit_amd.serving import Predictor
from helpers import make_pair
from text_candidates import CSV, gen_candidate, host_candidate

pytestmark = pytest.mark.gpu

CACHE_TOL = 5e-6  # the reference's assert_epsilon! (block_helpers.rs:30-40) between cached and plain routes
UNCOVERED = ["C", "Ddd", "E", "F"]  # namespaces the serving context below leaves to the candidates
CTX = "|A ca |Bb cb1 cb2:0.5 "


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _trained(nn=False, interactions=(), shared_field=False, seed=31):
    mi, _, _ = make_pair(6, 4, 12, 12, fw.Optimizer.AdagradLUT, lr=0.05, ffm_lr=0.05, interactions=interactions)
    if shared_field:  # namespaces 0 and 1 feed one field
        mi.ffm_fields = [[fw.NamespaceDescriptor(0), fw.NamespaceDescriptor(1)]] + [[fw.NamespaceDescriptor(i)] for i in range(2, 6)]
    if nn:
        mi.nn_layers = [dict(width="9", activation="relu"), dict(width="5", activation="relu", init="xavier")]
    re = fw.Regressor(mi)
    if not shared_field and not interactions:
        recs, off = fw.synth_records(6, 1.0, 1.1, 3000, 0.2, seed, 0, 600)
        b = re.record_batch(fw.FeatureBufferTranslator(mi), recs, off)
        re.learn_batch(b, capi.MODE_SEQUENTIAL, True)
        b.close()
    return mi, re


class Ctx:
    """a context on every layer: its text, record, scan, and the device cache that knows the record"""

    def __init__(self, host, re, fbt, text):
        self.text = text.encode()
        self.rec = host.next_vowpal(self.text)
        self.px = host.scan_context(self.text)
        assert self.px.is_record(self.rec)
        self.cache = re.setup_cache(fbt.translate(self.rec))
        self.cache.cover_record(fbt, self.rec)


@pytest.fixture(scope="module")
def rig():
    vw = VwNamespaceMap(CSV)
    mi, re = _trained()
    host, dev = VowpalParser(vw), DeviceVowpalParser(vw)
    yield vw, mi, re, fw.FeatureBufferTranslator(mi), host, dev
    dev.close()
    host.close()
    re.close()


def _line_of(length, tok):
    """a plain line of exactly `length` bytes with its newline, tokens of `tok` bytes"""
    if length == 1:
        return "\n"
    if length == 2:
        return "|\n"
    body = "|A"
    while len(body) + 1 + tok + 1 <= length - 1:
        body += " " + "x" * (tok - 2) + "%02d" % (len(body) % 97)
    pad = length - 1 - len(body)
    if pad >= 2:
        body += " " + "y" * (pad - 1)
    elif pad == 1:
        body += "z"
    assert len(body) == length - 1
    return body + "\n"


def _check_against_host(host, dev, fbt, ctx, lines, text=None):
    """parse_candidates == fwgpu_parser_parse_candidate line by line; -> info"""
    text = b"".join(lines) if text is None else text
    words, off, info = dev.parse_candidates(ctx.px, ctx.cache, fbt, text)
    assert len(info) == len(lines) and len(off) == len(lines) + 1 and off[0] == 0 and off[-1] == len(words)
    for i, line in enumerate(lines):
        rc, rec, is_delta = host_candidate(host, ctx.px, line)
        got = words[int(off[i]): int(off[i + 1])]
        assert info["code"][i] == rc, (i, line[:80])
        assert np.array_equal(got, rec), (i, line[:80], info[i])
        assert bool(info["is_delta"][i]) == is_delta, (i, line[:80])
    return info


# ---------------------------------------------------------------- 3. records
SPECIAL = ["\n", "|\n", "|Zz a\n", "|A a:x\n", "|A a:NONE b\n", "|A a:inf\n", "|Bb q:nan\n", "|F abinf\n", "|A a  \n", "f7 |A a\n", "17 |C x\n",
           "1abc |E k\n", "-x |A y\n", "-1 |A y\n", "1 |C labelled\n", "flush\n"]


@pytest.mark.parametrize("ctx_text,again,other", [
    ("1 0.5 |A ca |Bb cb1 cb2 cb3 ", "|A ca", "|A other"),
    ("|F ab1.5 |C cc ", "|C cc", "|C cd |F ab2"),
    ("-1 |Ddd d1 d2 d3 |E e1:2 |G:1.0 g ", "|G g", "|Ddd d1 d2 d3"),
], ids=["label-importance", "f32", "ranges"])
def test_records_are_the_host_parsers(rig, ctx_text, again, other):
    vw, mi, re, fbt, host, dev = rig
    ctx = Ctx(host, re, fbt, ctx_text)
    rng = random.Random(len(ctx_text))
    lines = [gen_candidate(rng) + "\n" for _ in range(300)]
    lines += SPECIAL + [again + "\n", other + "\n", "|E e " + again + " |Ddd q:2\n"]
    for length in (15, 16, 17, 63, 64, 65, 4095, 4096, 4097):
        lines += [_line_of(length, 7), _line_of(length, 21)]
    for ntok in (64, 65, 512, 513):  # tokens: the namespace and ntok - 1 features
        lines.append("|Bb" + " k" * (ntok - 1) + "\n")
        lines.append("|Bb" + "".join(" k%d:2" % j for j in range(ntok - 1)) + "\n")
    rng.shuffle(lines)
    lines = [l.encode() for l in lines]
    info = _check_against_host(host, dev, fbt, ctx, lines)
    starts_bar = np.array([l[:1] == b"|" for l in lines])
    assert not info["by_host"][starts_bar].all() and info["by_host"][~starts_bar].all()
    assert (info["by_host"][starts_bar] == 0).sum() >= 300  # the device took the plain ones
    # a last line without its newline: its last byte is ignored, as the host ignores it
    text = b"".join(lines[:40]) + b"|C last|Bb  tail:2 t2_"
    _check_against_host(host, dev, fbt, ctx, lines[:40] + [b"|C last|Bb  tail:2 t2_"], text=text)
    ctx.cache.close()


def test_long_context_start_positions_keep_14_bits(rig):
    """in the merged record a candidate's ranges lie L0 - H further on: beyond 16383 words the line is the host's"""
    vw, mi, re, fbt, host, dev = rig
    ctx = Ctx(host, re, fbt, "|A ca |G " + " ".join("g%d:2" % i for i in range(7000)) + " ")  # (G feeds no field: the cache stays small)
    L0, H = len(ctx.rec), 3 + vw.num_namespaces
    assert L0 == H + 14000
    lines = []
    for nfeat in (1100, 1186, 1187, 1250):  # stand-alone length H + 2 * nfeat; 14000 + H + 2 * 1186 = 16382 < 16383 < 14000 + H + 2 * 1187
        lines.append(("|C" + "".join(" c%d:3" % j for j in range(nfeat)) + "\n").encode())
    lines.append(b"|E e\n")
    info = _check_against_host(host, dev, fbt, ctx, lines)
    assert H == 10 and info["by_host"].tolist() == [0, 0, 1, 1, 0]
    ctx.cache.close()


def test_refusals(rig):
    vw, mi, re, fbt, host, dev = rig
    ctx = Ctx(host, re, fbt, CTX)
    bare = re.setup_cache(fbt.translate(ctx.rec))  # never went through cover_record
    with pytest.raises(capi.FwgpuError) as e:
        dev.parse_candidates(ctx.px, bare, fbt, b"|C a\n")
    assert e.value.code == capi.ERR_INVALID
    px_other = host.scan_context(b"|A ca |Bb cb1 ")  # a scan of another context
    with pytest.raises(capi.FwgpuError) as e:
        dev.parse_candidates(px_other, ctx.cache, fbt, b"|C a\n")
    assert e.value.code == capi.ERR_INVALID
    with pytest.raises(capi.FwgpuError) as e:
        dev.parse_candidates(ctx.px, ctx.cache, fbt, b"|C a\n|C b\n|C c\n", max_lines=2)
    assert e.value.code == capi.ERR_RANGE
    with pytest.raises(capi.FwgpuError) as e:
        dev.parse_candidates(ctx.px, ctx.cache, fbt, b"|C a\n|C b\n", words_cap=15)
    assert e.value.code == capi.ERR_RANGE
    words, off, info = dev.parse_candidates(ctx.px, ctx.cache, fbt, b"")
    assert len(words) == 0 and off.tolist() == [0] and len(info) == 0
    bare.close()
    ctx.cache.close()


# ---------------------------------------------------------------- 4. counts and the record rule
def test_counts_and_record_rule_equal_the_hosts_on_the_merged_record():
    vw = VwNamespaceMap(CSV)
    mi, re = _trained(interactions=[(0, 2)], shared_field=True)  # LR combo A x C: A in the context, C in the candidates; A and Bb share field 0
    fbt = fw.FeatureBufferTranslator(mi)
    host, dev = VowpalParser(vw), DeviceVowpalParser(vw)
    ctx = Ctx(host, re, fbt, "|A ca1 ca2:0.5 ca3 |Ddd cd ")
    # a Bb feature with the masked hash of the cached A feature ca1: same field, so the filter would drop it
    want = int(ctx.rec[ctx.rec[3] >> 16 & 0x3fff]) & fbt.ffm_hash_mask
    twin = next(n for n in ("t%d" % i for i in range(200000)) if int(host.next_vowpal(("|Bb %s\n" % n).encode())[4]) & fbt.ffm_hash_mask == want)
    rng = random.Random(9)
    lines = [gen_candidate(rng, namespaces=["Bb", "C", "E", "F"], f32_nan=False) + "\n" for _ in range(300)]
    lines += ["|Bb %s\n" % twin, "|Bb a b %s:2 c |C x\n" % twin, "|Bb a |Bb %s\n" % twin, "|Bb %s |Bb a\n" % twin,  # cached twin: in place, in a range, in the live run, in a dead run
              "|C c1 c2 c3 c4\n", "|C\n", "|A ca1\n", "|Ddd cd\n", "|Ddd cd |E e\n", "|Ddd other\n", "|Ddd cd cd\n",  # combo 3 x 4, 3 x 0; covered slots again
              "f7 |C a\n", "|Zz a\n", "\n"]
    lines = [l.encode() for l in lines]
    info = _check_against_host(host, dev, fbt, ctx, lines)
    seen_ok = {0: 0, 1: 0}
    for i, line in enumerate(lines):
        if info["code"][i] != capi.OK:
            assert info["n_lr"][i] == 0 and info["n_ffm"][i] == 0 and info["record_ok"][i] == 0
            continue
        merged = host.next_vowpal_with_cache(ctx.text, line)
        fb = fbt.translate(merged)
        assert (info["n_lr"][i], info["n_ffm"][i]) == (len(fb.lr_buffer), len(fb.ffm_buffer)), (line, info[i])
        assert bool(info["record_ok"][i]) == ctx.cache.record_ok(fbt, merged), (line, info[i])
        seen_ok[int(info["record_ok"][i])] += 1
    assert seen_ok[1] > 200 and seen_ok[0] >= 6
    by = dict(zip(lines, info))
    assert by[("|Bb %s\n" % twin).encode()]["record_ok"] == 0 and by[("|Bb %s |Bb a\n" % twin).encode()]["record_ok"] == 1
    assert by[b"|Ddd cd\n"]["record_ok"] == 1 and by[b"|Ddd other\n"]["record_ok"] == 0  # the context's own feature again is "as in the context"
    assert by[b"|C c1 c2 c3 c4\n"]["n_lr"] == 3 + 4 + 1 + 3 * 4 + 1 and by[b"|C c1 c2 c3 c4\n"]["by_host"] == 0
    ctx.cache.close()
    dev.close()
    re.close()


# ---------------------------------------------------------------- 5. / 6. serving
@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("serving_text")
    vw = VwNamespaceMap(CSV)
    out = {}
    for name, nn in (("headless", False), ("head", True)):
        mi, re = _trained(nn=nn)
        out[name] = str(d / (name + ".fw"))
        P.save_regressor_to_filename(out[name], mi, vw, re)
        re.close()
    return out


def _candidates(n, seed):
    rng = random.Random(seed)
    return [gen_candidate(rng, namespaces=UNCOVERED, f32_nan=False) + "\n" for _ in range(n)]


def test_plain_candidates_never_reach_the_host_parser(rig, models):
    vw, mi, re, fbt, host, dev = rig
    ctx = Ctx(host, re, fbt, CTX)
    cands = _candidates(3000, 11)
    words, off, info = dev.parse_candidates(ctx.px, ctx.cache, fbt, "".join(cands).encode())
    assert len(info) == 3000 and not info["by_host"].any() and info["record_ok"].all() and info["is_delta"].all()
    assert dev.last_lines() == (3000, 0)
    ctx.cache.close()
    pr = Predictor(f"fw -i {models['headless']} -t --foreground")
    assert pr.setup_cache(CTX + "\n") == 0.0
    p = pr.predict_text("".join(cands).encode(), with_cache=True)
    assert len(p) == 3000 and pr.last_text_route() == (3000, 0, False)
    pr.close()


@pytest.mark.parametrize("n", [40, 300])
@pytest.mark.parametrize("model", ["headless", "head"])
def test_predict_text_is_predict_batch_to_the_bit(models, model, n):
    pr = Predictor(f"fw -i {models[model]} -t --foreground")
    cands = _candidates(n, 3 * n)
    assert pr.setup_cache(CTX + "\n") == 0.0
    text = "".join(cands).encode()
    got = pr.predict_text(text, with_cache=True)
    assert pr.last_text_route() == (n, 0, False)
    want = pr.predict_batch(cands, with_cache=True)
    assert np.array_equal(_bits(got), _bits(want))
    whole = np.array([pr.predict(CTX + c) for c in cands], dtype=np.float32)
    assert whole.std() > 0.01 and (whole > 0).all()
    assert np.abs(got - whole).max() < CACHE_TOL
    # the last line without its newline is the same request
    assert np.array_equal(_bits(pr.predict_text(text[:-1], with_cache=True)), _bits(want))
    # whole lines, no cache
    lines = [CTX + c for c in cands]
    plain = pr.predict_text("".join(lines).encode(), with_cache=False)
    assert pr.last_text_route() == (n, 0, False)
    assert np.array_equal(_bits(plain), _bits(pr.predict_batch(lines)))
    pr.close()


def test_bad_lines_fallbacks_and_limits(models):
    pr = Predictor(f"fw -i {models['headless']} -t --foreground")
    cands = _candidates(40, 5)
    assert pr.predict_text(b"", with_cache=True).size == 0 and pr.last_text_route() == (0, 0, False)
    # before any fw_setup_cache there is no device cache: the existing route
    assert np.array_equal(_bits(pr.predict_text("".join(cands).encode(), with_cache=True)), _bits(pr.predict_batch(cands, with_cache=True)))
    assert pr.last_text_route() == (40, 40, True)
    assert pr.setup_cache(CTX + "\n") == 0.0
    want = pr.predict_batch(cands, with_cache=True)
    # one line that does not parse, one the host parses (a weight the device does not prove): -1.0 there, the others unchanged
    bad = cands[:20] + ["|Zz a\n", "|C a:0.12345678901234567\n"] + cands[20:]
    got = pr.predict_text("".join(bad).encode(), with_cache=True)
    n, host_lines, fell_back = pr.last_text_route()
    assert (n, fell_back) == (42, False) and 1 <= host_lines <= 2
    assert got[20] == -1.0 and np.array_equal(_bits(np.delete(got, [20, 21])), _bits(want))
    assert np.array_equal(_bits(got), _bits(pr.predict_batch(bad, with_cache=True)))
    # a candidate that names a covered namespace with another feature: the whole request takes the existing route
    again = cands[:7] + ["|A other |C x\n"] + cands[7:]
    got = pr.predict_text("".join(again).encode(), with_cache=True)
    assert pr.last_text_route() == (41, 41, True)
    assert np.array_equal(_bits(got), _bits(pr.predict_batch(again, with_cache=True)))
    assert np.abs(got - np.array([pr.predict(CTX + c) for c in again], dtype=np.float32)).max() < CACHE_TOL
    # ... and so does one that goes on in the context's last namespace
    got = pr.predict_text(("more |C x\n" + "".join(cands)).encode(), with_cache=True)
    assert pr.last_text_route()[2] and np.array_equal(_bits(got), _bits(pr.predict_batch(["more |C x\n"] + cands, with_cache=True)))
    # the output's capacity
    with pytest.raises(capi.FwgpuError) as e:
        pr.predict_text("".join(cands).encode(), with_cache=True, cap=39)
    assert e.value.code == capi.ERR_RANGE
    assert len(pr.predict_text("".join(cands).encode(), with_cache=True, cap=40)) == 40
    # a second fw_setup_cache replaces the first
    ctx2 = "|Bb z1 |A z2 z3 "
    assert pr.setup_cache(ctx2 + "\n") == 0.0
    got = pr.predict_text("".join(cands).encode(), with_cache=True)
    assert pr.last_text_route() == (40, 0, False)
    assert np.array_equal(_bits(got), _bits(pr.predict_batch(cands, with_cache=True))) and not np.array_equal(_bits(got), _bits(want))
    assert np.abs(got - np.array([pr.predict(ctx2 + c) for c in cands], dtype=np.float32)).max() < CACHE_TOL
    # a clone_lite copy has its own context and its own route report
    cl = pr.clone_lite()
    assert cl.last_text_route() == (0, 0, False)
    assert cl.setup_cache(CTX + "\n") == 0.0
    assert np.array_equal(_bits(cl.predict_text("".join(cands[:9]).encode(), with_cache=True)), _bits(want[:9]))
    assert cl.last_text_route() == (9, 0, False) and pr.last_text_route() == (40, 0, False)
    assert np.array_equal(_bits(pr.predict_text("".join(cands).encode(), with_cache=True)), _bits(got))  # the prototype still serves its own
    cl.close()
    pr.close()


def test_several_pieces_give_the_same_bits(models, monkeypatch):
    pr = Predictor(f"fw -i {models['head']} -t --foreground")
    cands = _candidates(300, 77)
    text = "".join(cands).encode()
    assert len(text) > 3 * 4096
    assert pr.setup_cache(CTX + "\n") == 0.0
    want = pr.predict_text(text, with_cache=True)
    monkeypatch.setenv("FWGPU_SERVING_TEXT_PIECE", "4096")
    got = pr.predict_text(text, with_cache=True)
    assert pr.last_text_route() == (300, 0, False) and np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(pr.predict_text(text, with_cache=False)), _bits(pr.predict_batch(cands)))
    # a line longer than a piece is the host's, wherever it stands
    long_line = "|C" + "".join(" c%d" % j for j in range(900)) + "\n"
    assert len(long_line) > 4096
    for at in (0, 150, 300):
        mixed = cands[:at] + [long_line] + cands[at:]
        got = pr.predict_text("".join(mixed).encode(), with_cache=True)
        assert pr.last_text_route() == (301, 1, False) and np.array_equal(_bits(got), _bits(pr.predict_batch(mixed, with_cache=True)))
    monkeypatch.delenv("FWGPU_SERVING_TEXT_PIECE")
    monkeypatch.setenv("FWGPU_SERVING_HOST_PARSE", "1")
    assert np.array_equal(_bits(pr.predict_text(text, with_cache=True)), _bits(want)) and pr.last_text_route() == (300, 300, True)
    pr.close()


def test_packed_predictor_takes_the_existing_route(models):
    pr = Predictor(f"fw -i {models['headless']} -t --foreground --packed_weights")
    cands = _candidates(40, 5)
    assert pr.setup_cache(CTX + "\n") == 0.0
    got = pr.predict_text("".join(cands).encode(), with_cache=True)
    assert pr.last_text_route() == (40, 40, True)
    assert np.array_equal(_bits(got), _bits(pr.predict_batch(cands, with_cache=True)))
    lines = [CTX + c for c in cands]
    assert np.array_equal(_bits(pr.predict_text("".join(lines).encode(), with_cache=False)), _bits(pr.predict_batch(lines)))
    pr.close()
