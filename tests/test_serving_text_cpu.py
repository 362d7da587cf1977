"""Serving from text, the part that needs no device: the new entry points exist and refuse NULL arguments, and the rule the device parser's
candidate mode rests on -- the candidate-only record of a line that starts with '|' is the line's stand-alone record with four small
adjustments (text_candidates.adjusted) -- holds on the host parser."""
import ctypes as C
import random

import numpy as np

from fwumious_wabbit_amd import capi
from fwumious_wabbit_amd.feed import VowpalParser, VwNamespaceMap
from text_candidates import CSV, adjusted, gen_candidate, host_candidate

# a label and an importance + a three-feature namespace; an f32 namespace; ranges only; a bare one.  Each ends with a space: the scan
# reaches the context's end and requests resume from the context's own record.  (context, a namespace of it with the feature it holds)
CONTEXTS = [
    ("1 0.5 |A ca |Bb cb1 cb2 cb3 ", "|A ca"),
    ("|F ab1.5 |C cc ", "|C cc"),
    ("-1 |Ddd d1 d2 d3 |E e1:2 ", "|Ddd d1"),
    ("|A x |C y |E:1.0 z |G g1 g2 ", "|E z"),
]


def test_new_symbols_refuse_null_arguments():
    from fwumious_wabbit_amd import serving
    L = serving._lib()
    n, w = C.c_uint64(), C.c_uint64()
    assert L.fwgpu_text_parser_parse_candidates(None, None, None, None, b"", 0, 0, None, 0, None, None, C.byref(n), C.byref(w)) == capi.ERR_INVALID
    out = np.zeros(4, dtype=np.float32)
    assert L.fwgpu_predictor_predict_text(None, b"|A a\n", 5, 1, capi.ptr(out), 4, C.byref(n)) == capi.ERR_INVALID
    f = C.c_int()
    assert L.fwgpu_predictor_last_text_route(None, C.byref(n), C.byref(w), C.byref(f)) == capi.ERR_INVALID


def test_candidate_only_record_is_the_adjusted_stand_alone_record():
    vw = VwNamespaceMap(CSV)
    parser = VowpalParser(vw)
    n_ns = vw.num_namespaces
    fired_all = 0
    for ci, (ctx, again) in enumerate(CONTEXTS):
        ctx = ctx.encode()
        px = parser.scan_context(ctx)
        ctx_rec = parser.next_vowpal(ctx)
        assert px.is_record(ctx_rec)
        rng = random.Random(100 + ci)
        for k in range(3000):
            cand = gen_candidate(rng)
            if k % 50 == 0:
                cand += " " + again  # a context namespace again, with the feature the context gave it
            line = (cand + "\n").encode()
            rc, got, is_delta = host_candidate(parser, px, line)
            assert rc == capi.OK and is_delta, line
            want, fired = adjusted(parser.next_vowpal(line), ctx_rec, n_ns)
            fired_all += fired
            assert got[0] == len(got) and np.array_equal(got, want), (ctx, line)
    assert fired_all >= 100  # "slot equals the context's" was exercised (contexts 0, 1 and 3 hold the repeated feature in place)
    # a feature token first goes on in the context's last namespace: where that one left feature words behind, no candidate-only form
    for ctx in (CONTEXTS[0][0], CONTEXTS[2][0]):
        px = parser.scan_context(ctx.encode())
        for cand in (b"17 |C x\n", b"f7 |A a\n", b"-x |A y\n", b"1abc\n"):
            rc, got, is_delta = host_candidate(parser, px, cand)
            assert rc == capi.OK and not is_delta
            assert np.array_equal(got, parser.next_vowpal_with_cache(ctx.encode(), cand))
