"""Training from text parsed on the device: the parts that need no GPU -- the C ABI declares the calls, the built library exports them and
the Python mirror reaches them."""
import os
import re

import fwumious_wabbit_amd as fw
from fwumious_wabbit_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fwgpu_trainer_digest_text_device", "fwgpu_trainer_digest_file_device", "fwgpu_debug_text_plan")


def test_library_exports_and_capi_resolves_the_new_calls():
    L = capi.lib()
    for name in NEW:
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is not None, name
    # same shapes as the header's prototypes: (tr, tp, cache, text, len, &n, &consumed), (tr, tp, cache, filename, &n), 12 arguments
    assert [len(getattr(L, n).argtypes) for n in NEW] == [7, 5, 12]


def test_python_mirror_has_both_methods():
    for name in ("digest_text_device", "digest_file_device"):
        assert callable(getattr(fw.HogwildTrainer, name))


def test_header_declares_the_new_calls():
    header = open(os.path.join(ROOT, "include", "fwgpu.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert re.search(r"fwgpu_trainer_digest_text_device\(fwgpu_trainer \*tr, fwgpu_text_parser \*tp, fwgpu_cache \*cache,\s*const char \*text, uint64_t len,"
                     r"\s*uint64_t \*n_examples, uint64_t \*consumed\);", header)
