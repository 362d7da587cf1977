"""fwgpu_head_set_step_rule / fwgpu_head_get_step_rule are declared to Python as include/fwgpu.h declares them (the style of test_quantize_cpu.py)."""
import ctypes as C
import os
import re

from fwumious_wabbit_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_step_rule_prototypes_and_constants_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "fwgpu.h")).read()
    ctype = {"fwgpu_regressor *": C.c_void_p, "const fwgpu_regressor *": C.c_void_p, "int": C.c_int, "int *": C.POINTER(C.c_int)}
    L = capi.lib()
    for name, n_args in (("fwgpu_head_set_step_rule", 2), ("fwgpu_head_get_step_rule", 2)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/fwgpu.h"
        want = [ctype[re.sub(r"\s+", " ", re.sub(r"\w+$", "", arg.strip())).strip()] for arg in m.group(1).split(",")]
        fn = getattr(L, name)
        assert len(want) == n_args and list(fn.argtypes) == want and fn.restype is C.c_int, (name, fn.argtypes, want)
    for name, value in (("HEAD_STEP_SUMMED", capi.HEAD_STEP_SUMMED), ("HEAD_STEP_PER_EXAMPLE", capi.HEAD_STEP_PER_EXAMPLE)):
        assert int(re.search(r"#define\s+FWGPU_" + name + r"\s+(\d+)", hdr).group(1)) == value
