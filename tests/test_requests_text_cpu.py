"""Many requests' candidates from their text, the part that needs no device: the entry point is declared, exported and bound, and refuses NULL
arguments before it touches a predictor."""
import ctypes as C
import os
import re

import numpy as np

from fwumious_wabbit_amd import capi, serving

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "fw_ffi.h")) as f:
        assert re.search(r"\bint fwgpu_predictor_predict_requests_text\(", f.read())
    assert capi.lib().fwgpu_predictor_predict_requests_text is not None
    assert serving._lib().fwgpu_predictor_predict_requests_text.restype is C.c_int
    assert callable(serving.predict_requests_text) and callable(serving.Predictor.last_launch)
    assert capi.lib().fwgpu_predictor_last_launch is not None


def test_null_arguments_are_refused_without_a_device():
    L = serving._lib()
    one = (C.c_void_p * 1)(None)
    texts, lens, caps, n = (C.c_char_p * 1)(b"|A a\n"), (C.c_uint64 * 1)(5), (C.c_uint64 * 1)(4), (C.c_uint64 * 1)()
    out = np.zeros(4, dtype=np.float32)
    outs = (C.c_void_p * 1)(out.ctypes.data)
    assert L.fwgpu_predictor_predict_requests_text(None, 1, texts, lens, outs, caps, n) == capi.ERR_INVALID
    assert L.fwgpu_predictor_predict_requests_text(one, 1, texts, lens, outs, caps, n) == capi.ERR_INVALID  # (a NULL predictor)
    assert L.fwgpu_predictor_predict_requests_text(one, 1, None, lens, outs, caps, None) == capi.ERR_INVALID
    assert L.fwgpu_predictor_predict_requests_text(None, 0, None, None, None, None, None) == capi.OK  # (no requests: nothing to do)
    assert L.fwgpu_predictor_last_launch(None, None, None, 0) == capi.ERR_INVALID
