"""The byte-diff stream's host codec (csrc/diff_stream.h behind fwgpu_diff_bytes / fwgpu_diff_apply_bytes) against the reference's known
answers (weight_patcher/src/main.rs: its tests and the format) and against a restatement of the format written here from its description.
The device kernels are judged against this codec (tests/test_gpu_publish_diff.py), so it is pinned without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fwumious_wabbit_amd import capi
from fwumious_wabbit_amd import persistence as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_VALUES = (0, 1, 127, 128, 16383, 16384, 2097151, 2097152, 2**64 - 1)  # main.rs test_read_write_varint
VARINT_KAT = {12345: "b960", 16383: "ff7f", 16384: "808001", 2097151: "ffff7f", 2097152: "80808001"}
HELLO_WORLD = "0077016f01720264"


def restated_varint(v):
    out = bytearray()
    while v >= 0x80:  # 7 bits per byte, little end first, the top bit on every byte but the last
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def restated_diff(a, b, base_offset=0, prev_index=0, fault=None):
    """the format from its description: for every differing index, ascending, varint(index - prev) then the new byte; prev starts at
    prev_index (0 for a whole file).  fault: one of two planted mistakes, which the known answers must catch."""
    assert len(a) == len(b)
    out, prev = bytearray(), prev_index
    for i in range(len(a)):
        if a[i] == b[i]:
            continue
        index = base_offset + i
        out += restated_varint(index - (base_offset if fault == "delta from the range start" else prev))
        out.append(a[i] if fault == "writes a[i]" else b[i])
        prev = index
    return bytes(out)


def decode_varint(s):
    v = 0
    for k, byte in enumerate(s):
        v |= (byte & 0x7F) << (7 * k)
        if not byte & 0x80:
            return v, k + 1
    raise ValueError("unterminated")


def known_answers(diff):
    """every known answer through `diff(a, b, base_offset, prev_index)`; returns the list of those it misses"""
    missed = []

    def expect(name, got, want):
        if got != want:
            missed.append(name)

    for v, hexes in VARINT_KAT.items():  # the value is the first entry's delta: one differing byte at index v
        expect(f"varint {v}", diff(b"\1", b"\2", v, 0), bytes.fromhex(hexes) + b"\2")
    expect("varint u64::MAX", len(diff(b"\1", b"\2", 2**64 - 1, 0)), 10 + 1)
    expect("hello -> world", diff(b"hello", b"world", 0, 0), bytes.fromhex(HELLO_WORLD))
    expect("equal inputs", diff(b"hello world", b"hello world", 0, 0), b"")
    expect("delta 0 at index 0", diff(b"ab", b"xb", 0, 0), b"\0x")
    # the reference's value list as the delta between prev_index and the entry, and as the delta between two entries of one range
    for v in REFERENCE_VALUES:
        if v <= 2**64 - 1 - 1000:
            expect(f"prev_index, {v}", diff(b"\1", b"\2", 1000 + v, 1000), restated_varint(v) + b"\2")
        if 0 < v < 2**22:
            a = bytes(v + 1)
            b = b"\7" + bytes(v - 1) + b"\5"
            expect(f"second entry, {v}", diff(a, b, 0, 0), b"\0\7" + restated_varint(v) + b"\5")
    return missed


def test_known_answers():
    assert known_answers(P.diff_bytes) == []
    for v in REFERENCE_VALUES:  # the varint round trip
        stream = P.diff_bytes(b"\1", b"\2", v, 0)
        assert decode_varint(stream) == (v, len(stream) - 1) and stream[-1] == 2
    assert len(P.diff_bytes(b"\1", b"\2", 2**64 - 1, 0)) == 11
    # changed counts the entries; prev_index beyond base_offset has no meaning
    assert P.diff_bytes(b"hello", b"world", with_changed=True)[1] == 4
    with pytest.raises(capi.FwgpuError) as e:
        P.diff_bytes(b"a", b"b", 5, 6)
    assert e.value.code == capi.ERR_INVALID


def test_the_restatement_passes_the_known_answers_and_two_planted_faults_do_not():
    assert known_answers(restated_diff) == []
    for fault in ("delta from the range start", "writes a[i]"):
        missed = known_answers(lambda a, b, base, prev: restated_diff(a, b, base, prev, fault=fault))
        assert missed, fault
    # ... each caught by the reference's own example among others
    assert "hello -> world" in known_answers(lambda a, b, base, prev: restated_diff(a, b, base, prev, fault="writes a[i]"))
    assert "hello -> world" in known_answers(lambda a, b, base, prev: restated_diff(a, b, base, prev, fault="delta from the range start"))


@pytest.mark.parametrize("density", [0.0, 1e-3, 0.5, 1.0])
def test_the_codec_agrees_with_the_restatement_on_random_arrays(density):
    rng = np.random.default_rng(int(density * 1000) + 3)
    n = 20011
    a = rng.integers(0, 256, size=n, dtype=np.uint8)
    b = a.copy()
    hit = rng.random(n) < density
    b[hit] ^= rng.integers(1, 256, size=int(hit.sum()), dtype=np.uint8)
    a, b = a.tobytes(), b.tobytes()
    for base, prev in ((0, 0), (12345, 0), (12345, 12000), (2**32 - 100, 2**32 - 4096), (12345, 12345)):
        want = restated_diff(a, b, base, prev)
        got, changed = P.diff_bytes(a, b, base, prev, with_changed=True)
        assert got == want, (base, prev)
        assert changed == int(hit.sum())
        if prev == 0:  # a whole file's stream, or its tail's: the round trip
            assert P.apply_diff_bytes(a, got, base) == b
    if density == 0.0:
        assert P.diff_bytes(a, b) == b""


def test_round_trip_and_entries_below_base_offset():
    rng = np.random.default_rng(9)
    a = rng.integers(0, 256, size=5000, dtype=np.uint8)
    b = a.copy()
    b[rng.random(5000) < 0.1] ^= 0x11
    a, b = a.tobytes(), b.tobytes()
    stream = P.diff_bytes(a, b)
    assert P.apply_diff_bytes(a, stream) == b
    assert P.apply_diff_bytes(a[2500:], stream, base_offset=2500) == b[2500:]  # the second half patched alone
    assert P.apply_diff_bytes(a, b"") == a


def test_two_call_protocol():
    L = capi.lib()
    a, b = np.frombuffer(b"hello", dtype=np.uint8), np.frombuffer(b"world", dtype=np.uint8)
    n, changed = C.c_uint64(0), C.c_uint64(0)
    args = (capi.ptr(a), capi.ptr(b), 5, 0, 0)
    assert L.fwgpu_diff_bytes(*args, None, 0, C.byref(n), C.byref(changed)) == capi.ERR_RANGE and (n.value, changed.value) == (8, 4)
    out = np.full(9, 0xEE, dtype=np.uint8)
    assert L.fwgpu_diff_bytes(*args, capi.ptr(out), 7, C.byref(n), None) == capi.ERR_RANGE and n.value == 8
    assert out[7] == 0xEE and out[8] == 0xEE  # nothing beyond cap was written
    assert L.fwgpu_diff_bytes(*args, capi.ptr(out), 8, C.byref(n), None) == capi.OK and out[:8].tobytes().hex() == HELLO_WORLD and out[8] == 0xEE


BAD_STREAMS = [
    ("a truncated varint", bytes([0x01, 0x6F, 0x80]), "ends inside an entry"),
    ("a stream missing its `to` byte", bytes([0x01, 0x6F, 0x02]), "ends inside an entry"),
    ("an 11-byte varint", bytes([0x01, 0x6F] + [0x80] * 10 + [0x00, 0x64]), "varint"),
    ("a varint beyond 64 bits", bytes([0x01, 0x6F] + [0xFF] * 9 + [0x02, 0x64]), "varint"),
    ("an index equal to n", bytes([0x01, 0x6F, 0x04, 0x64]), "beyond"),
    ("a zero delta in a second entry", bytes([0x01, 0x6F, 0x00, 0x64]), "zero delta"),
]


@pytest.mark.parametrize("name,stream,word", BAD_STREAMS, ids=[b[0] for b in BAD_STREAMS])
def test_bad_streams_are_refused_and_change_nothing(name, stream, word):
    L = capi.lib()
    t = np.frombuffer(b"hello", dtype=np.uint8).copy()
    d = np.frombuffer(stream, dtype=np.uint8)
    applied = C.c_uint64(99)
    assert L.fwgpu_diff_apply_bytes(capi.ptr(t), t.size, 0, capi.ptr(d), d.size, C.byref(applied)) == capi.ERR_FORMAT
    assert word in L.fwgpu_last_error().decode()
    assert t.tobytes() == b"hello" and applied.value == 0
    # (the same stream without its bad end is applied)
    assert P.apply_diff_bytes(b"hello", stream[:2]) == b"hollo"


def test_prototypes_are_declared_as_the_headers_declare_them():
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    ctype = {"fwgpu_regressor *": vp, "uint8_t *": vp, "const uint8_t *": vp, "uint64_t": u64, "uint64_t *": C.POINTER(u64), "const char *": C.c_char_p,
             "const fwgpu_vwmap *": vp, "const fwgpu_model_instance *": vp, "int": i32, "fwgpu_image **": C.POINTER(vp), "const fwgpu_image *": vp,
             "uint32_t *": C.POINTER(u32), "float *": vp}
    hdr = open(os.path.join(ROOT, "include", "fwgpu.h")).read()
    L = capi.lib()
    assert L.fwgpu_abi_version() == 1
    for name in ("fwgpu_diff_bytes", "fwgpu_diff_apply_bytes", "fwgpu_image_capture", "fwgpu_image_load", "fwgpu_image_len", "fwgpu_image_read",
                 "fwgpu_image_diff", "fwgpu_packed_apply_diff", "fwgpu_debug_diff", "fwgpu_debug_diff_geometry", "fwgpu_debug_diff_rates"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/fwgpu.h"
        want = [ctype[re.sub(r"\s+", " ", re.sub(r"\w+$", "", arg.strip())).strip().replace("* *", "**")] for arg in m.group(1).split(",")]
        fn = getattr(L, name)
        assert list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is i32
    assert re.search(r"\bint\s+fwgpu_predictor_apply_diff\s*\(FfiPredictor \*p, const uint8_t \*diff, uint64_t len\)\s*;",
                     open(os.path.join(ROOT, "include", "fw_ffi.h")).read())
