"""The host side of the device quantiser (csrc/quantize.hip): the header-forming routine factored out of the host quantiser for the device route
leaves fwgpu_quantize_ffm_weights what it was, and the new entry points are declared to Python as include/fwgpu.h declares them."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

from fwumious_wabbit_amd import _capi as capi
from fwumious_wabbit_amd import persistence as P
import quantize_cases as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# sha256 (first 24 hex digits) of fwgpu_quantize_ffm_weights on quantize_cases.crafted(n), recorded from the library as it was BEFORE
# quantize_header was factored out of quantize_ffm
RECORDED = {
    65: {
        "min-first": "85893213f8ea96bf054d9f57",
        "max-first": "503061417f254d605b2609af",
        "min-last": "9e97763253e4cfe04e3069d8",
        "max-last": "8705a60b110bb525e8302a51",
        "min-in-tail": "ee03f28daf3c8825f38046cb",
        "max-in-tail": "1c95533e24f5cda9191f2420",
        "quotients-on-half": "07e01f4280e16e3c8fcb5b40",
        "f16-ties": "fcdffa80975b2553876bd1be",
        "negative-buckets": "9a15dd1bf7852da73b4086e3",
        "overflow-to-infinity": "edc8926c0de232a5716a677f",
        "denormal-weights": "be2ee47da744eceb29eee9b8",
        "denormal-minimum": "f613a654a0edc24bd8892695",
        "negative-zero-inside": "fafe271dc4cb05f3ab6911df",
    },
    257: {
        "min-first": "5d96abb668941394ce00f1c3",
        "max-first": "e7c96cf5b525f9f2aaedf470",
        "min-last": "c54c4b802764538445668f43",
        "max-last": "5e479b90220de39ae41612a5",
        "min-in-tail": "fc10d48ce1ef11a32d1e777c",
        "max-in-tail": "bcb3f64a5ab958b64ca3c1c2",
        "quotients-on-half": "f9cb8f9ea7f5cb3de7fdbf44",
        "f16-ties": "f9d6f37c3935167bca7c337d",
        "negative-buckets": "e4edea76e562bec35478f75b",
        "overflow-to-infinity": "6ce4f7e5df41c9cfbe350456",
        "denormal-weights": "45f8c00b86664bee761b343d",
        "denormal-minimum": "da53e00927be4968e4d3fe28",
        "negative-zero-inside": "35e49d67287bd65206115b10",
    },
    4099: {
        "min-first": "64d2859be18f8cddd86f011b",
        "max-first": "39bab94e71cabf2d6b446604",
        "min-last": "5d1b6babf3436c0eb80d511a",
        "max-last": "006d981b8c9553dee21e7427",
        "min-in-tail": "aedce5444475bae1b4ce9a89",
        "max-in-tail": "7b84c047d7880bfe1240ccaa",
        "quotients-on-half": "1b844a9af9f0beb6a202c491",
        "f16-ties": "6ca3992e0a8b556e07d898fe",
        "negative-buckets": "1ede54380c4663fdfc865134",
        "overflow-to-infinity": "4c1d1bc6f9fcd8f8988ac74c",
        "denormal-weights": "c43479b76abc2b38b0f96776",
        "denormal-minimum": "c52cbc47117f38cf7f117e36",
        "negative-zero-inside": "3c9a368c5acc906a11e870cf",
    },
}


@pytest.mark.parametrize("n", sorted(RECORDED))
def test_host_quantiser_is_byte_identical_on_the_crafted_tables(n):
    cases = Q.crafted(n)
    assert [name for name, _, _ in cases] == list(RECORDED[n])
    for name, table, check in cases:
        blob = P.quantize_ffm_weights(table)
        assert hashlib.sha256(blob).hexdigest()[:24] == RECORDED[n][name], name
        inc, mn, q = Q.split(blob, n)
        check(q, inc, mn)  # ... and the table does produce the bucket pattern it was made for
        assert Q.takes_device_route(blob, table), name


def test_crafted_tables_hold_their_patterns_at_every_length_the_gpu_test_uses():
    for n in Q.LENGTHS:
        for name, table, check in Q.crafted(n):
            assert table.dtype == np.float32 and table.shape == (n,)
            if n >= Q.MIN_CHECKED_LEN:
                inc, mn, q = Q.split(P.quantize_ffm_weights(table), n)
                check(q, inc, mn)


def test_host_route_tables_are_what_the_contract_names():
    for name, table in Q.host_route_tables():
        assert not Q.takes_device_route(P.quantize_ffm_weights(table), table), name


def test_new_prototypes_are_declared_as_the_header_declares_them():
    hdr = open(os.path.join(ROOT, "include", "fwgpu.h")).read()
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
    ctype = {"fwgpu_regressor *": vp, "fwgpu_regressor **": C.POINTER(vp), "uint8_t *": vp, "uint64_t": u64, "uint64_t *": C.POINTER(u64),
             "const char *": C.c_char_p, "const fwgpu_vwmap *": vp, "const fwgpu_model_instance *": vp, "int": i32, "int *": C.POINTER(i32),
             "const float *": vp}
    L = capi.lib()
    for name, n_args in (("fwgpu_quantize_ffm_table", 4), ("fwgpu_model_save_inference", 5), ("fwgpu_pack_regressor", 2), ("fwgpu_debug_quantize", 6)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/fwgpu.h"
        want = []
        for arg in m.group(1).split(","):
            t = re.sub(r"\s+", " ", re.sub(r"\w+$", "", arg.strip())).strip()  # the type: the declarator without its name
            want.append(ctype[t.replace("* *", "**")])
        fn = getattr(L, name)
        assert len(want) == n_args and list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is i32
