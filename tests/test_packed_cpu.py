"""Packed FFM weights (fwgpu_model_load_packed: the quantised inference file's f16 buckets stay as they are in device memory), the part that needs
no GPU: the entry points exist and reject bad arguments before they touch a device, and the packed predict kernels keep the register budget of the
other hot kernels (compiled for gfx950 the way tests/test_kernel_registers_cpu.py does it)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from fwumious_wabbit_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_entry_points_exist_and_reject_bad_arguments_without_a_device(tmp_path):
    L = capi.lib()
    assert hasattr(L, "fwgpu_model_load_packed") and hasattr(L, "fwgpu_ffm_storage")
    assert L.fwgpu_abi_version() == 1
    vw, mi, r = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.fwgpu_model_load_packed(None, 0, C.byref(vw), C.byref(mi), C.byref(r)) == capi.ERR_INVALID
    assert L.fwgpu_model_load_packed(b"x.fw", 0, C.byref(vw), C.byref(mi), None) == capi.ERR_INVALID
    missing = str(tmp_path / "no_such_model.fw").encode()
    assert L.fwgpu_model_load_packed(missing, 0, C.byref(vw), C.byref(mi), C.byref(r)) == capi.ERR_IO
    assert not r.value and b"cannot open" in L.fwgpu_last_error()
    st, nb = C.c_int32(-1), C.c_uint64(0)
    assert L.fwgpu_ffm_storage(None, C.byref(st), C.byref(nb)) == capi.ERR_INVALID
    assert (capi.FFM_F32, capi.FFM_F16_BUCKETS) == (0, 1)
    # a file that is not a model file is a format error, still without a device
    junk = tmp_path / "junk.fw"
    junk.write_bytes(b"not a model file at all")
    assert L.fwgpu_model_load_packed(str(junk).encode(), 0, None, None, C.byref(r)) == 5  # FWGPU_ERR_FORMAT


PACKED_KERNELS = [
    "fw_example_kernel_r<100, false, 0, false, 1, 4, false, true>",  # single-chunk rows (R <= 256: k = 4 / 8)
    "fw_example_kernel_r<100, false, 0, false, 2, 4, false, true>",  # two-chunk rows (R <= 512: k = 16 x 30 fields)
]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("kernel", PACKED_KERNELS)
def test_packed_predict_kernels_keep_the_register_budget(kernel):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "hot_probe.py"), kernel], capture_output=True, text=True, timeout=600).stdout
    sg = re.search(r"SGPRs Spill: (\d+)", out)
    vg = re.search(r"VGPRs Spill: (\d+)", out)
    vr = re.search(r"\bVGPRs: (\d+)", out)
    sc = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", out)
    assert sg and vg and vr and sc, out
    assert "true>" in out  # (the packed instantiation itself was compiled, not a default)
    assert int(sg.group(1)) == 0 and int(vg.group(1)) == 0 and int(sc.group(1)) == 0, out
    assert int(vr.group(1)) <= 128, out
