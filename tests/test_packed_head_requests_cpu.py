"""--packed_head_requests (serving: context caches and the requests route of a deep-head model on packed weights), what needs no device."""
import pytest


def test_packed_head_requests_token_needs_packed_weights():
    """new_fw_predictor_prototype refuses the token on its own before it looks for a model or a device"""
    from fwumious_wabbit_amd import _capi as capi
    from fwumious_wabbit_amd.serving import Predictor

    with pytest.raises(capi.FwgpuError) as e:
        Predictor("fw -i /nonexistent/model.fw -t --foreground --packed_head_requests")
    assert "--packed_head_requests" in e.value.message and "--packed_weights" in e.value.message, e.value
