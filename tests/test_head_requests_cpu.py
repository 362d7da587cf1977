"""The requests route on deep-head models (fwgpu_enable_head_requests, --head_requests) where no GPU is needed: the symbols, their NULL checks, and the
serving token on a model without a head."""
import ctypes as C

import numpy as np
import pytest

from fwumious_wabbit_amd import _capi as capi
from fwumious_wabbit_amd.feed import VwNamespaceMap
from test_model_file_cpu import _mi, _training_file


def test_symbols_exist_and_refuse_null():
    L = capi.lib()
    assert capi.KERNEL_HEAD_REQUESTS == 6
    on = C.c_int32(7)
    assert L.fwgpu_enable_head_requests(None) == capi.ERR_INVALID
    assert L.fwgpu_head_requests_state(None, C.byref(on)) == capi.ERR_INVALID and on.value == 7


def test_head_requests_token_needs_a_deep_head(tmp_path):
    """new_fw_predictor_prototype reads the file's header and refuses the token on a headless model before it touches a device"""
    from fwumious_wabbit_amd.serving import Predictor
    path = str(tmp_path / "headless.fw")
    _training_file(path, _mi(), VwNamespaceMap("A,featureA\nB,featureB,f32\n"), np.zeros(32), np.zeros(36), np.zeros(36))
    with pytest.raises(capi.FwgpuError) as e:
        Predictor(f"fw -i {path} -t --foreground --head_requests")
    assert "--head_requests" in e.value.message and "deep head" in e.value.message, e.value
